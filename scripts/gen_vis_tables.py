#!/usr/bin/env python3
"""Write refnerf-pl_amd/vis_tables.py: the 256-entry `turbo` colour table of the installed matplotlib, as data.

Run:  python scripts/gen_vis_tables.py
refnerf_pl_amd.vis must not import matplotlib (validation runs where it is not installed), so the table ships with the
package.  It is sampled as the module samples any Colormap object: cmap(np.arange(cmap.N))[:, :3], cast to float32, and
stored as the hexadecimal bit patterns of the float32 values, so the file reproduces them bit for bit.  `gray` is k / 255
and is computed, not stored.
"""
import os

import matplotlib
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    cmap = matplotlib.colormaps["turbo"]
    lut = np.ascontiguousarray(cmap(np.arange(cmap.N))[:, :3], dtype=np.float32)
    assert lut.shape == (256, 3)
    words = lut.view(np.uint32).reshape(-1)
    lines = ['"""Colour tables of refnerf_pl_amd.vis, as data (written by scripts/gen_vis_tables.py from matplotlib %s).' % matplotlib.__version__,
             "",
             "TURBO_BITS: the 256 x 3 float32 values of matplotlib.colormaps['turbo'](np.arange(256))[:, :3], as uint32 bit patterns.",
             '"""',
             "TURBO_N = 256",
             "TURBO_BITS = ("]
    for i in range(0, words.size, 12):
        lines.append("    " + " ".join("0x%08x," % w for w in words[i:i + 12]))
    lines.append(")")
    path = os.path.join(ROOT, "refnerf-pl_amd", "vis_tables.py")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

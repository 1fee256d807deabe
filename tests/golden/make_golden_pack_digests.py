#!/usr/bin/env python3
"""Record the bytes of the seven weight images tests/test_guard_bands.py packs, as SHA-256 digests (needs the GPU).

Run:  python tests/golden/make_golden_pack_digests.py [--commit ID]
on a checkout of the commit whose packers are to be pinned, with its library built -- or with REFNERF_LIB naming a library built
from that commit and --commit naming the commit.  The digests pin a layout: they are recorded BEFORE a change to the packers
(refnerf-pl_amd/csrc/refnerf_pack.h) and never from the changed code; a change that moves bytes on purpose records them again
and says in its message which bytes moved.

tests/golden/pack_digests.json
  commit          the commit the library was built from
  sentinel_word   the 32-bit word every destination is pre-filled with (tests/guards.py): the prefetch pads, which the packers
                  never write, are part of the digests
  inputs          SHA-256 of the inputs: blob-G0 (synthetic.make_params), blob-G2 / blob-G7 (make_basis_params), basis-G2 / basis-G7
                  (geopoly.generate_basis 'icosahedron' 1 / 2), all as little-endian fp32
  images          per case id of test_guard_bands.py (pack_weights-{f32, bf16, f16, f16x2, f16x2_train}, pack_weights_basis-G{2, 7}):
                  bytes, sha256
"""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import guards  # noqa: E402
import refnerf_pl_amd  # noqa: E402,F401
from refnerf_pl_amd import _hip, geopoly, synthetic  # noqa: E402

PARAM_KW = dict(seed=3, bias_scale=0.05, sharpen=8.0)        # test_guard_bands.PARAM_KW
DEV = "cuda:0"


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def blob(groups):
    return synthetic.make_basis_params(n_basis=3 * groups, **PARAM_KW) if groups > 1 else synthetic.make_params(**PARAM_KW)


def basis(groups):
    return np.ascontiguousarray(geopoly.generate_basis("icosahedron", {2: 1, 7: 2}[groups]), np.float32)


def cases():
    for name, kind in (("f32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16), ("f16", _hip.PREC_F16), ("f16x2", _hip.PREC_F16X2),
                       ("f16x2_train", _hip.IMAGE_F16X2_TRAIN)):
        yield f"pack_weights-{name}", kind, 0
    for groups in (2, 7):
        yield f"pack_weights_basis-G{groups}", _hip.PREC_F32, groups


def image_digest(P, kind, groups=0, B=None):
    """bytes and SHA-256 of the image of blob P (device) packed into a sentinel-filled destination"""
    n = int(_hip.lib().refnerf_packed_weights_bytes_basis(kind, groups)) // 4
    img = torch.full((n,), guards.SENTINEL_I32, dtype=torch.int32, device=DEV).view(torch.float32)
    assert _hip.pack_weights(P, img, precision=kind, basis=B) is img
    torch.cuda.synchronize()
    return dict(bytes=4 * n, sha256=sha(img.cpu().numpy()))


def main():
    _hip.require_device()
    if "--commit" in sys.argv:
        commit = sys.argv[sys.argv.index("--commit") + 1]
    else:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    out = dict(commit=commit, sentinel_word=f"0x{guards.SENTINEL_I32 & 0xffffffff:08x}", inputs={}, images={})
    for groups in (0, 2, 7):
        out["inputs"][f"blob-G{groups}"] = sha(blob(groups))
        if groups:
            out["inputs"][f"basis-G{groups}"] = sha(basis(groups))
    for id, kind, groups in cases():
        P = torch.from_numpy(blob(groups)).to(DEV)
        B = torch.from_numpy(basis(groups)).to(DEV) if groups else None
        out["images"][id] = image_digest(P, kind, groups, B)
        print(id, out["images"][id])
    path = os.path.join(HERE, "pack_digests.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, "from", _hip.LIB_PATH, "at", commit)


if __name__ == "__main__":
    main()

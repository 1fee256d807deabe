#!/usr/bin/env python3
"""Capture the distortion-loss fixture from the upstream reference (build container only, CPU).

Run:  python tests/golden/make_golden_distortion.py
Needs the reference checkout (see _ref_harness.py).  Arrays and names only; no reference source travels.

tests/golden/distortion.npz
  The reference's stepfun.lossfun_distortion (stepfun.py:261-272) in float32 on the CPU, and its autograd gradient to w, on
  the inputs of tests/distortion_cases.py::rows (which the fixture stores too: the tests check their generator against it).
    shapes [S, 2]            (N, R) pairs, a few of the GPU tests' shapes
    kinds [K]                random, plateau, tiny
    seed                     the `seed` argument of distortion_cases.rows
    s<i>_<kind>_t [R, N+1], _w [R, N]          float32 inputs
    s<i>_<kind>_loss [R], _grad_w [R, N]       float32: the reference's value, d (sum of the R values) / d w
  The reference's stepfun.interval_distortion (stepfun.py:275-291) on float32 intervals, overlapping (partly, nested, equal,
  touching) and disjoint (either order):
    iv_t0_lo, iv_t0_hi, iv_t1_lo, iv_t1_hi [C], iv_value [C]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import _ref_harness  # noqa: E402

_ref_harness.install()
import torch  # noqa: E402

from internal import stepfun  # noqa: E402

import distortion_cases as DC  # noqa: E402

SHAPES = [(1, 3), (2, 3), (65, 5), (129, 3), (512, 1)]
KINDS = ["random", "plateau", "tiny"]
SEED = 7


def intervals():
    g = np.random.default_rng(23)
    lo0 = g.random(6).astype(np.float32)
    hi0 = (lo0 + 0.1 + g.random(6)).astype(np.float32)
    cases = []
    for a, b in zip(lo0, hi0):
        length = b - a
        cases += [(a, b, a + 0.5 * length, b + 0.5 * length),      # partly overlapping
                  (a, b, a + 0.25 * length, a + 0.75 * length),    # nested
                  (a, b, a, b),                                    # equal
                  (a, b, b, b + length),                           # touching: not disjoint by the reference's test
                  (a, b, b + 0.5, b + 1.0),                        # disjoint, t1 above
                  (a + 2.0, b + 2.0, a, b)]                        # disjoint, t1 below
    return [np.array(c, np.float32) for c in zip(*cases)]


def main():
    out = dict(shapes=np.array(SHAPES, np.int32), kinds=np.array(KINDS), seed=np.int32(SEED))
    for i, (N, R) in enumerate(SHAPES):
        for kind in KINDS:
            t, w = DC.rows(kind, R, N, SEED)
            wt = torch.tensor(w, requires_grad=True)
            loss = stepfun.lossfun_distortion(torch.tensor(t), wt)
            loss.sum().backward()
            assert loss.dtype == torch.float32 and loss.shape == (R,)
            l64, g64 = DC.truth(t, w)
            print(f"N={N:3d} R={R} {kind:9s} reference fp32 vs float64: loss rel {np.max(np.abs(loss.detach().numpy() - l64) / np.where(l64 > 0, l64, 1)):.2e}, "
                  f"grad rel {np.max(np.abs(wt.grad.numpy() - g64) / np.where(g64 > 0, g64, 1)):.2e}")
            p = f"s{i}_{kind}_"
            out[p + "t"], out[p + "w"], out[p + "loss"], out[p + "grad_w"] = t, w, loss.detach().numpy(), wt.grad.numpy()
    lo0, hi0, lo1, hi1 = intervals()
    val = stepfun.interval_distortion(*(torch.tensor(x) for x in (lo0, hi0, lo1, hi1))).numpy()
    assert val.dtype == np.float32 and np.isfinite(val).all()
    out.update(iv_t0_lo=lo0, iv_t0_hi=hi0, iv_t1_lo=lo1, iv_t1_hi=hi1, iv_value=val)
    path = os.path.join(HERE, "distortion.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

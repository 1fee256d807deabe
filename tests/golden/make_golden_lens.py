#!/usr/bin/env python3
"""Capture the lens-distortion vectors from the upstream reference (build container only).

Run:  python tests/golden/make_golden_lens.py
Needs the reference checkout (see _ref_harness.py).  Writes tests/golden/camera_distortion.npz: the inputs of
camera_utils.pixels_to_rays / cast_ray_batch with `distortion_params` (internal/camera_utils.py:409-493, 558-565) and
the reference's five outputs, computed from int64 pixel coordinates (so in float64, as the reference's dataset path
does) and kept in float64.  No reference source travels.

Layout: `cases` lists the case names; per case `<case>_pix_x`, `_pix_y` (int32), `_pixtocam` [3,3] (multi: [3,3,3]),
`_camtoworld` [3,4] (multi: [3,3,4]), `_pixtocam_ndc` (NDC cases only), `_distortion` (the dict, as JSON),
`_cam_idx` [n,1] (multi only) and `_origins`, `_directions`, `_viewdirs`, `_radii`, `_imageplane`.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import _ref_harness  # noqa: E402

_ref_harness.install()

import refnerf_pl_amd  # noqa: E402,F401
from refnerf_pl_amd import synthetic  # noqa: E402

CAMERAS = dict(llff=(1008, 756, 815.0), blender=(800, 800, 1111.111))
DISTORTIONS = dict(
    simple_radial=dict(k1=-0.08),
    radial=dict(k1=0.05, k2=-0.02),
    opencv=dict(k1=-0.1, k2=0.03, p1=1e-3, p2=-5e-4),
    k3k4=dict(k1=0.02, k2=-0.01, k3=0.004, k4=-0.001, p1=2e-4, p2=3e-4),
    strong=dict(k1=-0.25, k2=0.08, p1=2e-3, p2=-1e-3),
)
NO_NDC = ("strong",)      # float32 NDC radii of `strong` sit beyond the ray generator's bars (see the tests)
N = 256
KEYS = ("origins", "directions", "viewdirs", "radii", "imageplane")


def pixtocam(w, h, focal):
    return np.linalg.inv(np.array([[focal, 0, w / 2.0], [0, focal, h / 2.0], [0, 0, 1.0]])).astype(np.float32)


def pixels(rng, w, h, n=N):
    px = rng.integers(0, w, n).astype(np.int32)
    py = rng.integers(0, h, n).astype(np.int32)
    px[:4] = [0, w - 1, 0, w - 1]
    py[:4] = [0, 0, h - 1, h - 1]
    return px, py


def world_pose(seed):
    c2w = np.zeros((3, 4), np.float32)
    c2w[:3, :3] = synthetic._rot(seed).astype(np.float32)
    c2w[:3, 3] = (synthetic._rot(seed) @ np.array([0.0, 0.0, 4.0])).astype(np.float32)
    return c2w


def forward_pose():
    """A forward-facing pose (the LLFF setting NDC is defined for)."""
    c2w = np.zeros((3, 4), np.float32)
    c2w[:3, :3] = np.eye(3)
    c2w[:3, 3] = [0.11, -0.07, 0.03]
    return c2w


def main():
    from internal import camera_utils, utils
    rng = np.random.default_rng(2024)
    out, cases = {}, []
    for cam, (w, h, focal) in CAMERAS.items():
        p2c = pixtocam(w, h, focal)
        for dname, dist in DISTORTIONS.items():
            for ndc in (False, True):
                if ndc and dname in NO_NDC:
                    continue
                case = f"{cam}_{dname}_{'ndc' if ndc else 'world'}"
                px, py = pixels(rng, w, h)
                c2w = forward_pose() if ndc else world_pose(5 if cam == "blender" else 11)
                res = camera_utils.pixels_to_rays(px.astype(np.int64), py.astype(np.int64), p2c, c2w,
                                                  distortion_params=dict(dist), pixtocam_ndc=p2c if ndc else None, xnp=np)
                out[case + "_pix_x"], out[case + "_pix_y"] = px, py
                out[case + "_pixtocam"], out[case + "_camtoworld"] = p2c, c2w
                if ndc:
                    out[case + "_pixtocam_ndc"] = p2c
                out[case + "_distortion"] = np.array(json.dumps(dist))
                for k, v in zip(KEYS, res):
                    assert v.dtype == np.float64 or k == "origins", (case, k)   # world-space origins: the float32 pose
                    out[f"{case}_{k}"] = np.asarray(v, np.float64)
                cases.append(case)

    # three cameras of different focal length and pose sharing one dict, through cast_ray_batch with cam_idx
    case, (w, h, _), dist = "multi_opencv_world", CAMERAS["llff"], DISTORTIONS["opencv"]
    p2cs = np.stack([pixtocam(w, h, f) for f in (815.0, 700.0, 930.0)])
    c2ws = np.stack([world_pose(s) for s in (21, 22, 23)])
    px, py = pixels(rng, w, h)
    cam_idx = rng.integers(0, 3, (N, 1)).astype(np.int32)
    cam_idx[:3, 0] = [0, 1, 2]
    ones = np.ones((N, 1), np.float32)
    pix = utils.Pixels(pix_x_int=px.astype(np.int64), pix_y_int=py.astype(np.int64), lossmult=ones, near=ones, far=ones,
                       cam_idx=cam_idx.astype(np.int64))
    rays = camera_utils.cast_ray_batch((p2cs, c2ws, dict(dist), None), pix, xnp=np)
    out[case + "_pix_x"], out[case + "_pix_y"], out[case + "_cam_idx"] = px, py, cam_idx
    out[case + "_pixtocam"], out[case + "_camtoworld"] = p2cs, c2ws
    out[case + "_distortion"] = np.array(json.dumps(dist))
    for k in KEYS:
        v = getattr(rays, k)
        assert v.dtype == np.float64 or k == "origins", (case, k)
        out[f"{case}_{k}"] = np.asarray(v, np.float64)
    cases.append(case)

    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "camera_distortion.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(cases), "cases")


if __name__ == "__main__":
    main()

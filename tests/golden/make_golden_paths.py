#!/usr/bin/env python3
"""Capture the render-path and panorama vectors from the upstream reference (build container only).

Run:  python tests/golden/make_golden_paths.py
Needs the reference checkout (see _ref_harness.py).  Writes tests/golden/camera_paths.npz: inputs and the reference's
float64 outputs of the pose / path functions of internal/camera_utils.py:100-377 and of cast_spherical_rays (:700-746).
Arrays only; no reference source travels.

Layout
  inward_poses [12,3,4], forward_poses [10,3,4], forward_bounds [10,2]     the seeded inputs
  <set>_recenter_poses / _recenter_transform, <set>_pca_poses / _pca_transform, <set>_focus_point   (<set> = inward, forward)
  forward_spiral [8,3,4]                      generate_spiral_path(forward_poses, forward_bounds, n_frames=8)
  inward_ellipse, inward_ellipse_wave [8,3,4] generate_ellipse_path(inward_poses, 8) / (..., const_speed=False, z_variation=.5, z_phase=.25)
  inward_interpolated [33,3,4]                generate_interpolated_path(inward_poses, 3)
  interp1d_x [7], interp1d_out [18]           interpolate_1d(x, 3, 3, 0.)
  spline_image_names, spline_keyframes (str), spline_n_interp / _degree / _smoothness, spline_indices, spline_poses
                                              create_render_spline_path on inward_poses with a keyframe text file
  ff_* / pca_*                                the two branches of LLFF._load_renderings (datasets.py:649-679) on the seeded
                                              sets: ff_poses, ff_bounds, ff_transform, ff_spiral; pca_ellipse (= ellipse of inward_pca_poses)
  sample_t [2,9], sample_logits [2,8], sample_n, sample_out / sample_out_center     stepfun.sample on float64
  pano_cases (str), per case <case>_camtoworld [3,4] float32, _height, _width and the nine Rays fields [H,W,.] (the
                                              near / far passed in are the constants of the _near / _far fields)
"""
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import _ref_harness  # noqa: E402

_ref_harness.install()

RAY_FIELDS = ("origins", "directions", "viewdirs", "radii", "imageplane", "lossmult", "near", "far", "cam_idx")
PANO_SIZES = ((6, 8), (9, 37))      # (H, W)


def look_at(position, target, up):
    z = position - target
    z = z / np.linalg.norm(z)
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z, position], axis=1)


def inward_poses(rng, n=12):
    """Cameras on a tilted, noisy ring looking at a point near the origin."""
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n + rng.normal(0, 0.05)
        pos = np.array([3.1 * np.cos(a), 2.4 * np.sin(a), 0.8 + 0.3 * np.sin(2 * a)]) + rng.normal(0, 0.1, 3)
        out.append(look_at(pos, rng.normal(0, 0.05, 3), np.array([0.05, -0.02, 1.0])))
    tilt = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(tilt) < 0:
        tilt[:, 0] = -tilt[:, 0]
    poses = np.stack(out)
    return np.concatenate([tilt @ poses[:, :, :3], tilt @ poses[:, :, 3:] + np.array([[0.4], [-0.3], [0.2]])], -1)


def forward_poses(rng, n=10):
    """Cameras on a jittered plane looking down -z, with per-view depth bounds."""
    out = []
    for _ in range(n):
        pos = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.normal(0, 0.1)])
        out.append(look_at(pos, np.array([0.1, -0.05, -6.0]) + rng.normal(0, 0.2, 3), np.array([0.02, 1.0, 0.03])))
    bounds = np.stack([rng.uniform(2.0, 3.0, n), rng.uniform(20.0, 40.0, n)], -1)
    return np.stack(out), bounds


def main():
    from internal import camera_utils, stepfun, utils
    # create_render_spline_path (:364-366) opens the keyframe list in text mode and then decodes it as bytes, which
    # Python 3 refuses; hand it the bytes it expects (a run-time shim, like the harness's stubs)
    utils.open_file = lambda pth, mode='r': open(pth, mode='rb' if mode == 'r' else mode)
    rng = np.random.default_rng(20240611)
    out = {}
    inward = inward_poses(rng)
    forward, bounds = forward_poses(rng)
    out["inward_poses"], out["forward_poses"], out["forward_bounds"] = inward, forward, bounds

    for name, poses in (("inward", inward), ("forward", forward)):
        out[name + "_recenter_poses"], out[name + "_recenter_transform"] = camera_utils.recenter_poses(poses.copy())
        out[name + "_pca_poses"], out[name + "_pca_transform"] = camera_utils.transform_poses_pca(poses.copy())
        out[name + "_focus_point"] = camera_utils.focus_point_fn(poses)
    out["forward_spiral"] = camera_utils.generate_spiral_path(forward, bounds, n_frames=8)
    out["inward_ellipse"] = camera_utils.generate_ellipse_path(inward, n_frames=8)
    out["inward_ellipse_wave"] = camera_utils.generate_ellipse_path(inward, n_frames=8, const_speed=False, z_variation=.5, z_phase=.25)
    out["inward_interpolated"] = camera_utils.generate_interpolated_path(inward, 3)
    x = rng.normal(size=7)
    out["interp1d_x"], out["interp1d_out"] = x, np.asarray(camera_utils.interpolate_1d(x, 3, 3, 0.))

    names = [f"view_{i:02d}.png" for i in range(len(inward))]
    keyframes = [names[i] for i in (0, 2, 3, 5, 7, 8, 10, 11)]
    cfg = types.SimpleNamespace(render_spline_n_interp=4, render_spline_degree=5, render_spline_smoothness=.03)
    with tempfile.TemporaryDirectory() as tmp:
        cfg.render_spline_keyframes = os.path.join(tmp, "keyframes.txt")
        with open(cfg.render_spline_keyframes, "w") as fh:
            fh.write("\n".join(keyframes) + "\n")
        rets = camera_utils.create_render_spline_path(cfg, names, inward)
    out["spline_image_names"], out["spline_keyframes"] = np.array(names), np.array(keyframes)
    out["spline_n_interp"], out["spline_degree"], out["spline_smoothness"] = 4, 5, .03
    out["spline_indices"], out["spline_poses"] = np.asarray(rets[0]), np.asarray(rets[1])

    # the two branches of LLFF._load_renderings (datasets.py:649-679), composed from the reference's functions as there
    p, b = forward.copy(), bounds.copy()
    scale = 1. / (b.min() * .75)
    p[:, :3, 3] *= scale
    b *= scale
    p, transform = camera_utils.recenter_poses(p)
    out["ff_poses"], out["ff_bounds"], out["ff_transform"] = p, b, transform @ np.diag([scale] * 3 + [1])
    out["ff_spiral"] = camera_utils.generate_spiral_path(p, b, n_frames=8)
    out["pca_ellipse"] = camera_utils.generate_ellipse_path(out["inward_pca_poses"], n_frames=8, z_variation=0., z_phase=0.)
    with tempfile.TemporaryDirectory() as tmp:
        cfg.render_spline_keyframes = os.path.join(tmp, "keyframes.txt")
        with open(cfg.render_spline_keyframes, "w") as fh:
            fh.write("\n".join(keyframes) + "\n")
        rets = camera_utils.create_render_spline_path(cfg, names, out["inward_pca_poses"])
    out["pca_spline_indices"], out["pca_spline_poses"] = np.asarray(rets[0]), np.asarray(rets[1])

    t = np.sort(rng.uniform(0., 1., (2, 9)), axis=-1)
    logits = rng.normal(0, 1.5, (2, 8))
    out["sample_t"], out["sample_logits"], out["sample_n"] = t, logits, 6
    for key, center in (("sample_out", False), ("sample_out_center", True)):
        res = stepfun.sample(torch.tensor(t), torch.tensor(logits), 6, deterministic_center=center)
        assert res.dtype == torch.float64
        out[key] = res.numpy()

    cases = []
    for n, (h, w) in enumerate(PANO_SIZES):
        case = f"pano_{h}x{w}"
        c2w = np.concatenate([np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.normal(0, 2., (3, 1))], -1).astype(np.float32)
        near, far = 0.2 + n, 1e6 if n else 30.
        rays = camera_utils.cast_spherical_rays(c2w.astype(np.float64), h, w, near, far, xnp=np)
        out[case + "_camtoworld"], out[case + "_height"], out[case + "_width"] = c2w, h, w
        for k in RAY_FIELDS:
            out[f"{case}_{k}"] = np.asarray(getattr(rays, k), np.float64)
            assert out[f"{case}_{k}"].shape[:2] == (h, w), (case, k)
        cases.append(case)
    out["pano_cases"] = np.array(cases)

    for k, v in out.items():
        v = np.asarray(v)
        assert v.dtype.kind in "fiuU" and (v.dtype.kind != "f" or v.dtype == np.float64 or k.endswith("_camtoworld")), (k, v.dtype)
    path = os.path.join(HERE, "camera_paths.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()

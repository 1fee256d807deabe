#!/usr/bin/env python3
"""Capture the image-metric vectors from the upstream reference (build container only).

Run:  python tests/golden/make_golden_image.py
Needs the reference checkout (see _ref_harness.py).  Writes tests/golden/image_metrics.npz: recipe parameters and the
reference's float64 outputs, arrays only.  The inputs are NOT stored: tests/test_image_metrics.py regenerates them from the
seeded numpy.random.default_rng recipes this script imports from it (low-frequency sinusoids plus noise).

  cc_cases, cc_<case>_params (kind, H, W, seed as JSON), cc_<case>_it1 / _it5   image.color_correct (internal/image.py:84-127)
  psnr_mse / psnr_out                                                           image.mse_to_psnr on float64 values
  srgb_in / linear_to_srgb_out / srgb_to_linear_out                             on float64 values around both thresholds
  downsample_params, downsample_f2 / _f4                                        image.downsample
  wmae_params, wmae_out                                                         ref_utils.compute_weighted_mae
  disp_params, disp_mse                                                         the disparity MSE line of test_step
  step_params, step_<key>                                                       nerf_system.py:391-444 restated call by call
                                                                                with the reference's functions, quantised and
                                                                                cropped (eval_crop_borders = 3)
dm_pix is not installed where this runs (the harness stubs it), so the file holds no SSIM value.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import _ref_harness  # noqa: E402

_ref_harness.install()

import test_image_metrics as T  # noqa: E402  (the recipes)


def main():
    from internal import image, ref_utils
    out = {}
    f64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float64))  # noqa: E731

    out["cc_cases"] = np.array(list(T.CC_CASES))
    for case, prm in T.CC_CASES.items():
        img, ref = T.cc_pair(**prm)
        out[f"cc_{case}_params"] = np.array(json.dumps(prm))
        for it in (1, 5):
            res = image.color_correct(f64(img), f64(ref), num_iters=it)
            assert res.dtype == torch.float64
            out[f"cc_{case}_it{it}"] = res.numpy()
        print(case, "clipped fraction %.3f" % np.mean((img <= 0) | (img >= 1)))

    mse = np.array([1e-6, 3.7e-4, 0.0123, 0.25, 2.5])
    out["psnr_mse"] = mse
    out["psnr_out"] = image.mse_to_psnr(f64(mse)).numpy()
    assert out["psnr_out"].dtype == np.float64

    x = np.concatenate([np.linspace(0.0, 1.0, 41), [0.0031308, 0.00313, 0.0032, 0.04045, 0.0404, 0.0405, 1e-9]])
    out["srgb_in"] = x
    out["linear_to_srgb_out"] = image.linear_to_srgb(f64(x)).numpy()
    out["srgb_to_linear_out"] = image.srgb_to_linear(f64(x)).numpy()

    out["downsample_params"] = np.array(json.dumps(T.DOWNSAMPLE))
    img = T.sinus_image(**T.DOWNSAMPLE)
    for f in (2, 4):
        out[f"downsample_f{f}"] = image.downsample(f64(img), f).numpy()

    out["wmae_params"] = np.array(json.dumps(T.WMAE))
    w, n, g = T.wmae_inputs(**T.WMAE)
    out["wmae_out"] = ref_utils.compute_weighted_mae(f64(w), f64(n), f64(g)).numpy()

    out["disp_params"] = np.array(json.dumps(T.DISP))
    dist, disps = T.disp_inputs(**T.DISP)
    out["disp_mse"] = np.float64(float(((1 / (1 + f64(dist)) - f64(disps)) ** 2).mean()))

    # test_step, nerf_system.py:391-444, line by line on a synthetic rendering (float32, as the model returns it)
    out["step_params"] = np.array(json.dumps(T.STEP))
    rend, batch = T.step_inputs(**T.STEP)
    crop = T.STEP_CROP
    rendering = {k: torch.from_numpy(v).double() for k, v in rend.items() if not k.startswith('ray_')}
    gt_rgb = torch.tensor(batch["rgb"], dtype=torch.float64)
    rendering['rgb_cc'] = image.color_correct(rendering['rgb'], gt_rgb)
    out["step_rgb_cc"] = rendering['rgb_cc'].numpy()
    rgb, rgb_cc, rgb_gt = rendering['rgb'], rendering['rgb_cc'], gt_rgb
    rgb = torch.round(rgb * 255) / 255
    rgb_cc = torch.round(rgb_cc * 255) / 255
    crop_fn = lambda x, c=crop: x[c:-c, c:-c]  # noqa: E731
    rgb, rgb_cc, rgb_gt = crop_fn(rgb), crop_fn(rgb_cc), crop_fn(rgb_gt)
    out["step_psnr"] = np.float64(float(image.mse_to_psnr(((rgb - rgb_gt) ** 2).mean())))
    out["step_cc_psnr"] = np.float64(float(image.mse_to_psnr(((rgb_cc - rgb_gt) ** 2).mean())))
    for tag in ['mean', 'median']:
        disparity = 1 / (1 + rendering[f'distance_{tag}'])
        out[f"step_disparity_{tag}_mse"] = np.float64(float(((disparity - torch.from_numpy(batch["disps"])) ** 2).mean()))
    weights = rendering['acc'] * torch.from_numpy(batch["alphas"])
    normals_gt = ref_utils.l2_normalize(torch.tensor(batch["normals"]))
    keys = []
    for key, val in rendering.items():
        if key.startswith('normals') and val is not None:
            out[f"step_{key}_mae"] = np.float64(float(ref_utils.compute_weighted_mae(weights, ref_utils.l2_normalize(val), normals_gt)))
            keys.append(key + "_mae")
    out["step_normal_keys"] = np.array(keys)

    path = os.path.join(HERE, "image_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()

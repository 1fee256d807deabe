#!/usr/bin/env python3
"""Capture the data-term and depth-smoothness fixture from the upstream reference (build container only, CPU).

Run:  python tests/golden/make_golden_data_terms.py
Needs the reference checkout (see _ref_harness.py).  Arrays and settings only; no reference source travels.

tests/golden/data_terms.npz
  The reference's train_utils.compute_data_loss on seeded two-level renderings of R = 37 rays with a non-uniform lossmult and
  both statistics on (Config.compute_disp_metrics, compute_normal_metrics), for the four combinations of data_loss_type
  'mse' / 'charb' and supervised_by_linear_rgb, each with and without renderings['normals'] (eight cases, one set of inputs):
    data_bindings            the gin bindings every case shares (multipliers, the two metric flags)
    data_cases               the case names `<penalty>_<srgb|linear>_<normals|nonormals>`
    data_L<l>_<key>          the inputs: rgb, acc, distance_mean, normals per level; data_gt_rgb, data_disps, data_alphas,
                             data_normals_gt, data_lossmult
    <case>_loss, <case>_stat_keys (the keys of stats in the reference's order), <case>_stat_<key>, <case>_g_rgb_L<l>
                             (autograd's d loss / d renderings[l]['rgb'])
  and its train_utils.compute_depth_smoothness_loss on two levels of P = 5 patches of 4 x 4 rays, patch 1 with acc = 0 and
  patch 3 with a constant depth, both multipliers non-zero:
    smooth_bindings, smooth_L<l>_{distance, acc, rgb}, smooth_loss, smooth_g_distance_L<l>
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import _ref_harness  # noqa: E402

_ref_harness.install()
import torch  # noqa: E402
import gin  # noqa: E402

from internal import configs, train_utils, utils  # noqa: E402

REF_CFG = os.path.join(_ref_harness.REFERENCE_ROOT, "configs", "blender_refnerf.gin")
R, P, S = 37, 5, 4
DATA_BINDINGS = ["Config.compute_disp_metrics = True", "Config.compute_normal_metrics = True",
                 "Config.data_coarse_loss_mult = 0.4", "Config.data_loss_mult = 1.7", "Config.charb_padding = 0.001"]
SMOOTH_BINDINGS = ["Config.patch_size = 4", "Config.depth_smoothness_coarse_loss_mult = 0.3",
                   "Config.depth_smoothness_loss_mult = 1.2"]


def config(bindings):
    gin.clear_config()
    gin.parse_config_files_and_bindings([REF_CFG], list(bindings))
    return configs.Config()


def ref_rays(lossmult):
    """only lossmult is read by compute_data_loss; the other fields are placeholders of the right shapes"""
    z = lambda w: torch.zeros(R, w)     # noqa: E731
    return utils.Rays(origins=z(3), directions=z(3), viewdirs=z(3), radii=z(1), imageplane=z(2), lossmult=torch.tensor(lossmult),
                      near=z(1), far=z(1), cam_idx=z(1))


def data_terms(out):
    rng = np.random.default_rng(41)
    f = lambda *shape: rng.random(shape).astype(np.float32)     # noqa: E731
    levels = [dict(rgb=f(R, 3), acc=f(R), distance_mean=(2 + 4 * f(R)).astype(np.float32),
                   normals=rng.standard_normal((R, 3)).astype(np.float32)) for _ in range(2)]
    gt, disps, alphas = f(R, 3), f(R), f(R)
    normals_gt = rng.standard_normal((R, 3)).astype(np.float32)
    lossmult = (0.25 + 1.5 * f(R, 1)).astype(np.float32)
    for lvl, d in enumerate(levels):
        for k, v in d.items():
            out[f"data_L{lvl}_{k}"] = v
    out["data_gt_rgb"], out["data_disps"], out["data_alphas"], out["data_normals_gt"], out["data_lossmult"] = \
        gt, disps, alphas, normals_gt, lossmult
    out["data_bindings"] = np.array(DATA_BINDINGS)
    rays = ref_rays(lossmult)
    cases = []
    for penalty in ("mse", "charb"):
        for linear in (False, True):
            for with_normals in (True, False):
                case = f"{penalty}_{'linear' if linear else 'srgb'}_{'normals' if with_normals else 'nonormals'}"
                cases.append(case)
                cfg = config(DATA_BINDINGS + [f"Config.data_loss_type = '{penalty}'", f"Config.supervised_by_linear_rgb = {linear}"])
                assert cfg.data_loss_type == penalty and cfg.supervised_by_linear_rgb is linear and cfg.compute_disp_metrics
                rend = [{k: torch.tensor(v) for k, v in d.items() if with_normals or k != "normals"} for d in levels]
                for r in rend:
                    r["rgb"].requires_grad_(True)
                batch = utils.Batch(rays=rays, rgb=gt, disps=torch.tensor(disps), normals=torch.tensor(normals_gt),
                                    alphas=torch.tensor(alphas))
                loss, stats = train_utils.compute_data_loss(batch, rend, rays, cfg)
                loss.backward()
                out[case + "_loss"] = float(loss)
                out[case + "_stat_keys"] = np.array(list(stats))
                for k, v in stats.items():
                    out[f"{case}_stat_{k}"] = v.numpy()
                for lvl, r in enumerate(rend):
                    out[f"{case}_g_rgb_L{lvl}"] = r["rgb"].grad.numpy()
                print(case, float(loss), {k: v.numpy() for k, v in stats.items()})
    out["data_cases"] = np.array(cases)


def depth_smoothness(out):
    rng = np.random.default_rng(42)
    f = lambda *shape: rng.random(shape).astype(np.float32)     # noqa: E731
    cfg = config(SMOOTH_BINDINGS)
    assert cfg.depth_smoothness_coarse_loss_mult == 0.3 and cfg.depth_smoothness_loss_mult == 1.2
    rend = []
    for lvl in range(2):
        distance, acc, rgb = (2 + 4 * f(P, S, S, 1)).astype(np.float32), f(P, S, S), f(P, S, S, 3)
        acc[1] = 0.0                     # a patch that hit nothing
        distance[3] = distance[3, 0, 0]  # a patch of constant depth
        out[f"smooth_L{lvl}_distance"], out[f"smooth_L{lvl}_acc"], out[f"smooth_L{lvl}_rgb"] = distance, acc, rgb
        rend.append(dict(distance=torch.tensor(distance, requires_grad=True), acc=torch.tensor(acc), rgb=torch.tensor(rgb)))
    loss = train_utils.compute_depth_smoothness_loss(rend, cfg)
    loss.backward()
    out["smooth_loss"] = float(loss)
    for lvl, r in enumerate(rend):
        out[f"smooth_g_distance_L{lvl}"] = r["distance"].grad.numpy()
    out["smooth_bindings"] = np.array(SMOOTH_BINDINGS)
    print("smoothness", float(loss))


if __name__ == "__main__":
    out = {}
    data_terms(out)
    depth_smoothness(out)
    path = os.path.join(HERE, "data_terms.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")

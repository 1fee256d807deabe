#!/usr/bin/env python3
"""Capture the optimiser fixtures from the upstream reference (build container only, CPU).

Run:  python tests/golden/make_golden_optim.py [optim] [trajectory_clipped]
Needs the reference checkout (see _ref_harness.py).  Arrays only; no reference source travels.

tests/golden/optim.npz
  `sched_cases`, `sched_steps`, per case `sched_<case>_kw` (lr_init, lr_final, max_steps, lr_delay_steps, lr_delay_mult)
  and `sched_<case>` = the reference's math.learning_rate_decay at `sched_steps` (float64).
  Synthetic trajectories (refnerf_pl_amd.synthetic.optim_params / optim_gradient regenerate the inputs): the reference's
  train_utils.create_optimizer + torch's clip_grad_value_ / clip_grad_norm_ (as nerf_system.configure_gradient_clipping
  calls them) + Adam.step + scheduler.step, over 9 tensors (synthetic.OPTIM_SEGMENTS), in float32 and again in float64
  from the same float32 inputs.  `traj_config` holds the optimiser settings.  Per case `<n>_<clip>`:
    _idx            the stored elements (synthetic.optim_sample_index: the full trajectories would be 30 MB)
    _p32 / _p64     [K, len(idx)] parameters after every step (float32 run / float64 run)
    _lr             [K] the learning rate each step used
    _total_norm     [K] float64: the norm clip_grad_norm_ returns (of the value-clipped gradients)
    _grad_norms, _grad_maxes, _weights_l2s   [K, n_seg] float64: nerf_system.on_after_backward's statistics (raw gradient,
                    parameters before the step)
    _grad_check     [K, 8] float32: the first eight gradient elements of each step (guards the generator)

tests/golden/trajectory_clipped.npz
  make_golden.golden_trajectory's recipe (20 steps, 256 rays x 48 samples, seed 3) through the reference's
  create_optimizer, both clips and the scheduler, with the shipped grad_max_norm = 1e-3, lr_delay_steps = 8 and
  max_steps = 40: per-step losses, total_norm, lr, update_sub = (blob - init)[::97] and gt_rgb.
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the reference import shim)
import torch  # noqa: E402

from refnerf_pl_amd import layout, synthetic  # noqa: E402
from internal import configs, math as ref_math, train_utils, utils  # noqa: E402

SCHED_STEPS = lambda max_steps: [0, 1, 2, 255, 256, 511, 512, 513, 10 ** 4, max_steps, max_steps + 1]  # noqa: E731
TRAJ_CONFIG = dict(lr_init=2e-3, lr_final=2e-5, max_steps=16, lr_delay_steps=4, lr_delay_mult=0.01,
                   adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-6)


def shipped_config(name):
    import gin
    gin.clear_config()
    gin.parse_config_files_and_bindings([os.path.join(MG._ref_harness.REFERENCE_ROOT, "configs", name)], [])
    return configs.Config()


def schedule(out):
    cases = {}
    for name, gin_file in (("blender", "blender_refnerf.gin"), ("llff", "llff_refnerf.gin")):
        c = shipped_config(gin_file)
        cases[name] = dict(lr_init=c.lr_init, lr_final=c.lr_final, max_steps=c.max_steps, lr_delay_steps=c.lr_delay_steps,
                           lr_delay_mult=c.lr_delay_mult)
    cases["nodelay"] = dict(cases["blender"], lr_delay_steps=0)
    for name, kw in cases.items():
        steps = SCHED_STEPS(kw["max_steps"])
        out[f"sched_{name}_kw"] = np.array([kw[k] for k in ("lr_init", "lr_final", "max_steps", "lr_delay_steps", "lr_delay_mult")], np.float64)
        out[f"sched_{name}_steps"] = np.array(steps, np.int64)
        out[f"sched_{name}"] = np.array([ref_math.learning_rate_decay(s, **kw) for s in steps], np.float64)
    out["sched_cases"] = np.array(list(cases))


def segments_of(n):
    return list(synthetic.OPTIM_SEGMENTS) if n == synthetic.OPTIM_N else [n]


def run_trajectory(n, clip, dtype):
    val, norm, scale = synthetic.OPTIM_CLIPS[clip]
    cfg = configs.Config(grad_max_val=val, grad_max_norm=norm, **TRAJ_CONFIG)
    p0 = torch.tensor(synthetic.optim_params(n)).to(dtype)
    params = [torch.nn.Parameter(t.clone()) for t in torch.split(p0, segments_of(n))]
    opt, sched = train_utils.create_optimizer(cfg, params)
    res = {k: [] for k in ("p", "lr", "total_norm", "grad_norms", "grad_maxes", "weights_l2s", "grad_check")}
    idx = synthetic.optim_sample_index(n)
    for k in range(synthetic.OPTIM_STEPS):
        g = synthetic.optim_gradient(n, k, scale)
        for p, gs in zip(params, torch.split(torch.tensor(g).to(dtype), segments_of(n))):
            p.grad = gs.clone()
        # nerf_system.on_after_backward
        res["weights_l2s"].append([float(p.detach().norm() ** 2) for p in params])
        res["grad_norms"].append([float(p.grad.norm()) for p in params])
        res["grad_maxes"].append([float(p.grad.abs().max()) for p in params])
        # nerf_system.configure_gradient_clipping
        if cfg.grad_max_val > 0:
            torch.nn.utils.clip_grad_value_(params, clip_value=cfg.grad_max_val)
        if cfg.grad_max_norm > 0:
            tn = torch.nn.utils.clip_grad_norm_(params, max_norm=cfg.grad_max_norm)
        else:
            tn = torch.linalg.vector_norm(torch.cat([p.grad for p in params]))
        res["total_norm"].append(float(tn))
        res["lr"].append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        res["p"].append(torch.cat([p.detach() for p in params]).numpy()[idx].copy())
        res["grad_check"].append(g[:8])
    return idx, res


def optim():
    out = {}
    schedule(out)
    out["traj_config"] = np.array([TRAJ_CONFIG[k] for k in ("lr_init", "lr_final", "max_steps", "lr_delay_steps", "lr_delay_mult",
                                                            "adam_beta1", "adam_beta2", "adam_eps")], np.float64)
    worst = 0.0
    for n in (synthetic.OPTIM_N, 1, 3):
        for clip in synthetic.OPTIM_CLIPS:
            idx, r32 = run_trajectory(n, clip, torch.float32)
            _, r64 = run_trajectory(n, clip, torch.float64)
            c = f"{n}_{clip}"
            out[c + "_idx"] = idx.astype(np.int32)
            out[c + "_p32"] = np.stack(r32["p"]).astype(np.float32)
            out[c + "_p64"] = np.stack(r64["p"]).astype(np.float64)
            out[c + "_lr"] = np.array(r64["lr"], np.float64)
            out[c + "_grad_check"] = np.stack(r64["grad_check"]).astype(np.float32)
            for k in ("total_norm", "grad_norms", "grad_maxes", "weights_l2s"):
                out[f"{c}_{k}"] = np.array(r64[k], np.float64)
            # the reference's own float32 run against its float64 run, in units of the test's bar
            kk = np.arange(1, synthetic.OPTIM_STEPS + 1)[:, None]
            bar = kk * (2.0 ** -24 * np.abs(out[c + "_p64"]) + 2.0 ** -17 * TRAJ_CONFIG["lr_init"])
            frac = float((np.abs(out[c + "_p32"] - out[c + "_p64"]) / bar).max())
            worst = max(worst, frac)
            print(f"{c}: torch float32 vs float64 reaches {frac:.2f} of the bar; total_norm {out[c + '_total_norm']}")
    print("worst fraction of the bar:", worst)
    MG.save("optim", **out)


def trajectory_clipped(steps=20, n_rays=256, n_samples=48, lr_delay_steps=8, max_steps=40):
    pk = dict(seed=3, bias_scale=0.0)
    model, cfg = MG.build_model([f"Model.num_prop_samples = {n_samples}", f"Model.num_nerf_samples = {n_samples}",
                                 f"Config.lr_delay_steps = {lr_delay_steps}", f"Config.max_steps = {max_steps}"], pk)
    assert cfg.grad_max_norm == 1e-3 and cfg.lr_delay_steps == lr_delay_steps and cfg.max_steps == max_steps
    model.train()
    opt, sched = train_utils.create_optimizer(cfg, model.parameters())
    out = {"total": [], "data": [], "orientation": [], "normal": [], "total_norm": [], "lr": []}
    gts = []
    for it in range(steps):
        rays = synthetic.blender_rays(n_rays, seed=9100 + it, center_frac=0.85)
        gt = MG.analytic_target(rays)
        gts.append(gt)
        r = MG.to_rays(rays)
        opt.zero_grad()
        rend, hist = model(r, 1.0, False)
        batch = utils.Batch(rays=r, rgb=gt)
        data_loss, _ = train_utils.compute_data_loss(batch, rend, r, cfg)
        o_loss = train_utils.orientation_loss(r, model, hist, cfg)
        n_loss = train_utils.predicted_normal_loss(model, hist, cfg)
        loss = data_loss + o_loss + n_loss
        loss.backward()
        if cfg.grad_max_val > 0:
            torch.nn.utils.clip_grad_value_(model.parameters(), clip_value=cfg.grad_max_val)
        tn = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=cfg.grad_max_norm)
        out["total_norm"].append(float(tn))
        out["lr"].append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        for k, v in (("total", loss), ("data", data_loss), ("orientation", o_loss), ("normal", n_loss)):
            out[k].append(float(v))
        print(it, float(loss), float(tn), out["lr"][-1], flush=True)
    assert len(list(model.parameters())) == 2 * len(layout.PARAM_SPECS)
    blob = np.zeros(layout.NUM_PARAMS, np.float32)
    sd = model.nerf_mlp.state_dict()
    for spec in layout.PARAM_SPECS:
        blob[spec.w_off:spec.w_off + spec.out_dim * spec.in_dim] = sd[spec.name + ".weight"].numpy().reshape(-1)
        blob[spec.b_off:spec.b_off + spec.out_dim] = sd[spec.name + ".bias"].numpy()
    init = synthetic.make_params(**pk)
    MG.save("trajectory_clipped",
            recipe=np.array([steps, n_rays, n_samples, cfg.lr_init, cfg.adam_eps, pk["seed"], lr_delay_steps, max_steps, cfg.grad_max_norm,
                             cfg.grad_max_val]),
            update_sub=(blob - init)[::97].copy(), gt_rgb=np.stack(gts), total_norm=np.array(out["total_norm"], np.float64),
            lr=np.array(out["lr"], np.float64),
            **{"loss_" + k: np.array(out[k], np.float64) for k in ("total", "data", "orientation", "normal")})


if __name__ == "__main__":
    for w in sys.argv[1:] or ["optim", "trajectory_clipped"]:
        globals()[w]()

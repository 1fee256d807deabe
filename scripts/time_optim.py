"""The fused optimiser step against the sequences a loop had before it, on the C2 (Blender) model's blob:
    python scripts/time_optim.py
HIP-event pairs around every step, 200 steps after 20 warm-up steps, median and mean in us; one JSON line at the end.
  fused_flat / fused_tensors   ClippedAdam (stats + finalize + Adam kernels) on the flat blob / the 46 parameters
  torch_flat / torch_tensors   clip_grad_value_ + clip_grad_norm_ + torch.optim.Adam(fused=True) + mark_updated()
Launch counts come from the kernels' structure (fused: 2 k + 1) and, for the torch sequences, from torch.profiler."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import refnerf_pl_amd  # noqa: E402,F401
from refnerf_pl_amd import _hip, configs, models, synthetic, train_utils, utils  # noqa: E402

STEPS, WARM = 200, 20
GRAD_MAX_VAL = 0.1       # the shipped default is 0 (off); on here so that the parent sequence pays for both clips as the fused step does


def build(flat):
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "refnerf_blender.gin")],
                                            [f"Config.grad_max_val = {GRAD_MAX_VAL}"] + (["Config.hip_flat_grads = True"] if flat else []))
    cfg = configs.Config()
    model = models.construct_model(utils.dummy_rays(), cfg).to("cuda:0").train()
    model.nerf_mlp.load_flat_params(synthetic.make_params(seed=0))
    params = [model.nerf_mlp.flat_parameter()] if flat else list(model.parameters())
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda:0", generator=gen) * 1e-3
    return model, cfg, params


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return dict(median_us=float(np.median(us)), mean_us=float(us.mean()), p10_us=float(np.percentile(us, 10)), p90_us=float(np.percentile(us, 90)))


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))


def main():
    _hip.require_device()
    out = {}
    for flat in (True, False):
        tag = "flat" if flat else "tensors"
        model, cfg, params = build(flat)
        opt, _ = train_utils.create_optimizer(cfg, model)
        out["fused_" + tag] = dict(timed(opt.step), launches=2 * len(params) + 1)

        model, cfg, params = build(flat)
        adam = torch.optim.Adam(params, lr=cfg.lr_init, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_eps, fused=True)

        def parent():
            torch.nn.utils.clip_grad_value_(params, clip_value=cfg.grad_max_val)
            torch.nn.utils.clip_grad_norm_(params, max_norm=cfg.grad_max_norm)
            adam.step()
            model.nerf_mlp.mark_updated()
        res = timed(parent)
        try:
            res["launches"] = launches(parent)
        except Exception as e:      # the profiler is a convenience here, the timing is the result
            res["launches"] = None
            res["launches_error"] = repr(e)
        out["torch_" + tag] = res
        for k in ("fused_" + tag, "torch_" + tag):
            print(k, {a: (round(b, 1) if isinstance(b, float) else b) for a, b in out[k].items()}, flush=True)
    configs.clear_config()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

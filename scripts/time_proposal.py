"""The two host-side stages of the proposal-network configuration with and without Config.hip_fused_proposal, on the
constructor-default proposal model (Model(): 3 levels of 64 / 64 / 32 samples, a separate PropMLP, dilation_bias 0.0025,
dilation_multiplier 0.5, Config.interlevel_loss_mult 1.0) at 4096 rays:
    python scripts/time_proposal.py
Three measurements, each with the flag off and on IN THE SAME PROCESS, alternating blocks of steps so that both variants
see the same machine state:
  dilation     the two dilations of one Model.__call__ (64 -> 190 intervals, dilation 0.0025 + 0.5 / 64 and 0.0025 + 0.5 / 4096)
               on seeded step functions: stepfun.max_dilate_weights + [..., 1:-1] against _hip.max_dilate_weights;
  interlevel   train_utils.interlevel_loss against fused_interlevel_loss, forward + backward to the proposal weights, on
               seeded ray histories of 64 / 64 / 32 intervals;
  step         train_utils.training_losses + backward on the model (seeded rays, random-init networks; the MLP heads, the
               three Ref-NeRF losses and the f16x2 chains of configs/refnerf_blender.gin).
HIP-event pairs around every step, median / p10 / p90 in us over BLOCKS x STEPS steps per variant after warm-up; kernel
launches per step from torch.profiler (a separate, untimed step).  One JSON line at the end; ratio = unfused / fused
(>= 1: the fused path does not lose)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAYS = 4096
BLOCKS, STEPS, WARM = 4, 25, 5


def main():
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, configs, models, stepfun, synthetic, train_utils, utils
    _hip.require_device()
    dev = torch.device("cuda:0")
    # the shipped blender config (Ref-NeRF heads, the three Ref-NeRF losses, f16x2 chains) with the Model bindings put back to
    # the constructor's defaults and the proposal network given the same Ref-NeRF heads as the NeRF MLP
    gin = os.path.join(ROOT, "configs", "refnerf_blender.gin")
    mlp_bindings = [ln.strip() for ln in open(gin) if ln.startswith("NerfMLP.")]
    configs.clear_config()
    configs.parse_config_files_and_bindings([gin], [b.replace("NerfMLP.", "PropMLP.", 1) for b in mlp_bindings] + [
        "Model.num_levels = 3", "Model.num_prop_samples = 64", "Model.num_nerf_samples = 32", "Model.single_mlp = False",
        "Model.dilation_bias = 0.0025", "Model.dilation_multiplier = 0.5", "Model.anneal_slope = 10", "Model.resample_padding = 0.0",
        "Model.single_jitter = True", "Config.interlevel_loss_mult = 1.0"])
    cfg = configs.Config()
    torch.manual_seed(0)
    model = models.construct_model(utils.dummy_rays(), cfg).to(dev).train()
    assert (model.num_levels, model.num_prop_samples, model.num_nerf_samples) == (3, 64, 32) and model.prop_mlp is not model.nerf_mlp
    assert model.dilation_bias == 0.0025 and model.dilation_multiplier == 0.5 and cfg.interlevel_loss_mult == 1.0
    gen = torch.Generator(device=dev).manual_seed(0)

    def step_function(n, grad=False):
        t = torch.sort(torch.rand((RAYS, n + 1), device=dev, generator=gen), dim=-1).values
        t[:, 0], t[:, -1] = 0.0, 1.0
        w = 0.25 + torch.rand((RAYS, n), device=dev, generator=gen)
        w = (w / w.sum(-1, keepdim=True)).contiguous()
        return t.contiguous(), w.requires_grad_(grad)

    # -- the dilations of one forward pass
    sf = [step_function(64) for _ in range(2)]
    dil = [model.dilation_bias + model.dilation_multiplier / p for p in (64, 64 * 64)]

    def dilation(fused):
        for (t, w), d in zip(sf, dil):
            if fused:
                _hip.max_dilate_weights(t, w, d, 0.0, 1.0)
            else:
                sd, wd = stepfun.max_dilate_weights(t, w, d, domain=(0.0, 1.0), renormalize=True)
                sd, wd = sd[..., 1:-1].contiguous(), wd[..., 1:-1].contiguous()

    # -- the interlevel loss of one step
    hist = [dict(zip(("sdist", "weights"), step_function(n, grad=n_i < 2))) for n_i, n in enumerate((64, 64, 32))]
    for h in hist[:-1]:
        h["weights"] = h["weights"].detach().mul(0.6).requires_grad_(True)      # the penalty is active on most intervals

    def interlevel(fused):
        for h in hist[:-1]:
            h["weights"].grad = None
        (train_utils.fused_interlevel_loss if fused else train_utils.interlevel_loss)(hist, cfg).backward()

    # -- the whole step
    rays_np = synthetic.blender_rays(RAYS, seed=1, center_frac=0.4)
    rays = utils.rays_from_dict(dict(rays_np), dev)
    batch = utils.Batch(rays=rays, rgb=synthetic.target_rgb(RAYS, seed=5))

    def step(fused):
        cfg.hip_fused_proposal = fused
        for p in model.parameters():
            p.grad = None
        total, _, _, _ = train_utils.training_losses(model, batch, rays, cfg, global_step=cfg.max_steps // 2)
        total.backward()

    def timed(fn):
        """median / p10 / p90 per variant, blocks of STEPS steps alternating between the two variants"""
        us = {False: [], True: []}
        for fused in (False, True):
            for _ in range(WARM):
                fn(fused)
        torch.cuda.synchronize()
        for _ in range(BLOCKS):
            for fused in (False, True):
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
                for e0, e1 in ev:
                    e0.record()
                    fn(fused)
                    e1.record()
                torch.cuda.synchronize()
                us[fused] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        out = {}
        for fused, name in ((False, "unfused"), (True, "fused")):
            a = np.array(us[fused])
            out[name] = dict(median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)), p90_us=float(np.percentile(a, 90)),
                             launches=launches(lambda: fn(fused)))
        out["ratio"] = out["unfused"]["median_us"] / out["fused"]["median_us"]
        return out

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
        except Exception as e:      # the profiler is a convenience here, the timing is the result
            return repr(e)

    out = {}
    for name, fn in (("dilation", dilation), ("interlevel", interlevel), ("step", step)):
        out[name] = timed(fn)
        u, f = out[name]["unfused"], out[name]["fused"]
        print(f"{name}: unfused {u['median_us']:.0f} us (p10 {u['p10_us']:.0f}, p90 {u['p90_us']:.0f}; {u['launches']} launches), "
              f"fused {f['median_us']:.0f} us (p10 {f['p10_us']:.0f}, p90 {f['p90_us']:.0f}; {f['launches']} launches), "
              f"ratio {out[name]['ratio']:.2f}", flush=True)
    train_utils.flush_finite_check(cfg)
    out["shape"] = dict(rays=RAYS, levels=3, samples=[64, 64, 32], dilated_intervals=190)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

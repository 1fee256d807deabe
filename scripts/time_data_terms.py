"""The data term ('charb', both statistics) and the patch depth smoothness with and without Config.hip_fused_losses, at 2048
rays as 512 patches of 2 x 2, 2 levels:
    python scripts/time_data_terms.py
Times train_utils.compute_losses + backward to the seeds on synthetic device tensors shaped like the renderings of a patch
batch -- no MLP and no other loss term (Config's defaults leave the regularisers off; the interlevel loss is switched off),
so the number is these two terms' alone: compute_data_loss + compute_depth_smoothness_loss through ATen, against
refnerf_data_terms_* + refnerf_depth_smoothness_*.  HIP-event pairs around every step, 100 steps after 10 warm-up steps,
median / mean in us; kernel launches per step from torch.profiler.  Each variant runs in a fresh child process under a time
limit; the first failure ends the run.  One JSON line at the end: both variants and ratio = unfused / fused (>= 1: the fused
path does not lose)."""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARM = 100, 10
PATCHES, PATCH = 512, 2
CHILD_TIMEOUT_S = 240


def variant(fused):
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, configs, train_utils, utils
    _hip.require_device()
    dev = torch.device("cuda:0")
    configs.clear_config()
    cfg = configs.Config(hip_fused_losses=fused, data_loss_type="charb", compute_disp_metrics=True, compute_normal_metrics=True,
                         data_coarse_loss_mult=0.1, interlevel_loss_mult=0.0, patch_size=PATCH, depth_smoothness_loss_mult=0.1,
                         depth_smoothness_coarse_loss_mult=0.01)
    gen = torch.Generator(device=dev).manual_seed(0)
    lead = (PATCHES, PATCH, PATCH)

    def rand(*shape):
        return torch.rand(shape, device=dev, generator=gen)

    def randn(*shape):
        return torch.randn(shape, device=dev, generator=gen)
    rend = [dict(rgb=rand(*lead, 3), acc=rand(*lead), distance=2 + 4 * rand(*lead, 1), distance_mean=2 + 4 * rand(*lead),
                 normals=randn(*lead, 3)) for _ in range(2)]
    seeds = [t for r in rend for t in r.values()]
    for t in seeds:
        t.requires_grad_(True)
    rays = types.SimpleNamespace(lossmult=0.25 + rand(*lead, 1), viewdirs=randn(*lead, 3), origins=randn(*lead, 3))
    batch = utils.Batch(rays=rays, rgb=rand(*lead, 3), disps=rand(*lead), normals=randn(*lead, 3), alphas=rand(*lead))
    model = types.SimpleNamespace(num_levels=2)
    hist = [{"weights": torch.zeros((1, 1), device=dev)}] * 2

    def step():
        for t in seeds:
            t.grad = None
        total, losses, stats = train_utils.compute_losses(model, batch, rays, rend, hist, cfg)
        total.backward()
        return losses, stats

    def timed(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])
        return dict(median_us=float(np.median(us)), mean_us=float(us.mean()), p10_us=float(np.percentile(us, 10)),
                    p90_us=float(np.percentile(us, 90)))

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
        except Exception as e:      # the profiler is a convenience here, the timing is the result
            return repr(e)
    losses, stats = step()
    out = dict(losses=timed(step))
    out["losses"]["launches"] = launches(step)
    out["terms"] = {k: float(v.detach()) for k, v in losses.items()}
    out["stats"] = {k: [float(x) for x in v] for k, v in stats.items()}
    train_utils.flush_finite_check(cfg)
    configs.clear_config()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", choices=["unfused", "fused"], help="(internal) time one variant in this process")
    a = ap.parse_args()
    if a.variant:
        variant(a.variant == "fused")
        return
    out = {}
    for name in ("unfused", "fused"):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", name], stdout=subprocess.PIPE, text=True,
                             timeout=CHILD_TIMEOUT_S)
        if res.returncode != 0:
            sys.exit(f"time_data_terms: the {name} variant ended with status {res.returncode}; nothing further is run")
        out[name] = json.loads(res.stdout.strip().splitlines()[-1])
        print(name, {x: (round(y, 1) if isinstance(y, float) else y) for x, y in out[name]["losses"].items()}, out[name]["terms"],
              flush=True)
    # both variants saw the same seeded tensors: the same terms and statistics, or the timing compares different work
    for k, v in out["unfused"]["terms"].items():
        if abs(out["fused"]["terms"][k] - v) > 1e-5 * abs(v):
            sys.exit(f"time_data_terms: the variants disagree on the {k} term: {out['fused']['terms'][k]} vs {v}")
    if list(out["fused"]["stats"]) != list(out["unfused"]["stats"]):
        sys.exit("time_data_terms: the variants disagree on the statistics' keys")
    out["ratio"] = out["unfused"]["losses"]["median_us"] / out["fused"]["losses"]["median_us"]
    out["shape"] = dict(rays=PATCHES * PATCH * PATCH, patches=PATCHES, patch_size=PATCH, levels=2, terms=2)
    print(f"data term + depth smoothness + backward: unfused {out['unfused']['losses']['median_us']:.0f} us, fused "
          f"{out['fused']['losses']['median_us']:.0f} us, ratio {out['ratio']:.2f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

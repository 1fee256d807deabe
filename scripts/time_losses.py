"""The loss assembly of the nine-term step with and without Config.hip_fused_regularisers, at the per-GPU shard of C5
(configs/refnerf_llff_geometry_losses.gin: 2048 clean rays, sample_noise_size x sample_noise_angles = 512 noisy rays,
256 samples, 2 levels):
    python scripts/time_losses.py
Times train_utils.compute_losses + backward to the level seeds on synthetic device tensors shaped like the renderings and
the ray history -- no MLP, so the number is the assembly's alone -- and, separately, sample_utils.sample_noisy_rays.
Config.hip_fused_losses is on in both variants (as in bench.py's C5 leg), so the pair differs by the one flag.  HIP-event
pairs around every step, 100 steps after 10 warm-up steps, median / mean in us; kernel launches per step from
torch.profiler.  Each variant runs in a fresh child process under a time limit; the first failure ends the run.  One JSON
line at the end: both variants and ratio = unfused / fused (>= 1: the fused path does not lose)."""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARM = 100, 10
RAYS, SAMPLES = 2048, 256
CHILD_TIMEOUT_S = 240


def variant(fused):
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, configs, sample_utils, train_utils, utils
    _hip.require_device()
    dev = torch.device("cuda:0")
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "refnerf_llff_geometry_losses.gin")],
                                            ["Config.hip_fused_losses = True", f"Config.hip_fused_regularisers = {fused}"])
    cfg = configs.Config()
    n, a = cfg.sample_noise_size // cfg.patch_size ** 2, cfg.sample_noise_angles
    gen = torch.Generator(device=dev).manual_seed(0)

    def rand(*shape):
        return torch.rand(shape, device=dev, generator=gen)

    def unit(*shape):
        v = rand(*shape) - 0.5
        return v / v.norm(dim=-1, keepdim=True)

    def rays_of(R):
        return utils.Rays(origins=rand(R, 3), directions=unit(R, 3), viewdirs=unit(R, 3), radii=rand(R, 1) * 1e-3, imageplane=rand(R, 2),
                          lossmult=torch.ones(R, 1, device=dev), near=torch.zeros(R, 1, device=dev), far=torch.ones(R, 1, device=dev),
                          cam_idx=torch.zeros(R, 1, device=dev))

    def level(R, history):
        rend = dict(rgb=rand(R, 3), diffuse=rand(R, 3), specular=rand(R, 3), distance=rand(R, 1), acc=rand(R), normals=unit(R, 3),
                    normals_pred=unit(R, 3))
        w = rand(R, SAMPLES)
        hist = dict(weights=w / w.sum(-1, keepdim=True) * rend["acc"][:, None], normals=unit(R, SAMPLES, 3),
                    normals_pred=unit(R, SAMPLES, 3)) if history else {}
        return rend, hist
    rays, noisy_rays = rays_of(RAYS), rays_of(n * a)
    batch = utils.Batch(rays=rays, rgb=rand(RAYS, 3))
    clean, noisy = [level(RAYS, True) for _ in range(2)], [level(n * a, False) for _ in range(2)]
    seeds = [t for rend, hist in clean + noisy for d in (rend, hist) for t in d.values()]
    for t in seeds:
        t.requires_grad_(True)
    model = types.SimpleNamespace(num_levels=2)
    ratio = train_utils.consistency_warmup_ratio(cfg, cfg.max_steps // 2)

    def step():
        for t in seeds:
            t.grad = None
        total, _, _ = train_utils.compute_losses(model, batch, rays, [r for r, _ in clean], [h for _, h in clean], cfg,
                                                 renderings_noise=[r for r, _ in noisy], noisy_rays=noisy_rays, warmup_ratio=ratio)
        total.backward()

    def sampler():
        sample_utils.sample_noisy_rays(rays, clean[-1][0], cfg.sample_angle_range, n, a, ratio, fused=fused)

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
    out = dict(losses=timed(step), sampler=timed(sampler))
    out["losses"]["launches"] = launches(step)
    out["sampler"]["launches"] = launches(sampler)
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
            sys.exit(f"time_losses: the {name} variant ended with status {res.returncode}; nothing further is run")
        out[name] = json.loads(res.stdout.strip().splitlines()[-1])
        for k, v in out[name].items():
            print(name, k, {x: (round(y, 1) if isinstance(y, float) else y) for x, y in v.items()}, flush=True)
    out["ratio"] = out["unfused"]["losses"]["median_us"] / out["fused"]["losses"]["median_us"]
    out["sampler_ratio"] = out["unfused"]["sampler"]["median_us"] / out["fused"]["sampler"]["median_us"]
    out["shape"] = dict(rays=RAYS, samples=SAMPLES, levels=2, terms=9)
    print(f"loss assembly + backward: unfused {out['unfused']['losses']['median_us']:.0f} us, fused "
          f"{out['fused']['losses']['median_us']:.0f} us, ratio {out['ratio']:.2f}; noisy rays: ratio {out['sampler_ratio']:.2f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

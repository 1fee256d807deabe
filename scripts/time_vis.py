"""visualize_suite of refnerf_pl_amd.vis at the size of one validation view (800 x 800, float32, every optional key, 16 rays x
3 levels of 64 / 64 / 32 samples), through the kernels of csrc/refnerf_vis.h and through the ATen float64 path of the same
module, in one run on one device:
    python scripts/time_vis.py
Times visualize_suite as a whole, and its per-pixel half (one weighted percentile and visualize_cmap of the depth map) and
its ray half (visualize_rays at resolution 2048) on their own.  HIP-event pairs around every call, 10 calls after 3 warm-up
calls, median / p10 / p90 in ms; device kernel launches per call from torch.profiler (sorts and other plumbing included),
and the launches of the library's own entries from its bindings' counter.  The two paths alternate call by call so that
both see the same machine.  Nothing is asserted on time.  One JSON line at the end: per stage both variants and
ratio = aten / fused (> 1: the kernels are faster), and the largest distance between the two paths' panels."""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARM = 10, 3
H, W = 800, 800
RAYS, LEVELS = 16, (64, 64, 32)


def main():
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, vis
    _hip.require_device()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)

    def rand(*shape):
        return torch.rand(shape, device=dev, generator=gen)

    def unit(*shape):
        v = rand(*shape) - 0.5
        return v / v.norm(dim=-1, keepdim=True)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev) / H, torch.arange(W, device=dev) / W, indexing="ij")
    dist = 2.0 + 2.0 * (1 + torch.sin(6.0 * xx + 4.0 * yy)) + 0.05 * rand(H, W)
    dist[3, 5] = dist[700, 100] = float("nan")
    rendering = dict(rgb=rand(H, W, 3), acc=rand(H, W), distance_mean=dist, distance_median=dist + 0.05 * rand(H, W),
                     distance_percentile_5=dist - 0.3 * rand(H, W), distance_percentile_95=dist + 0.3 * rand(H, W),
                     normals=unit(H, W, 3), normals_pred=unit(H, W, 3), roughness=rand(H, W, 1) - 0.5, diffuse=rand(H, W, 3),
                     specular=rand(H, W, 3), tint=rand(H, W, 3), rgb_cc=rand(H, W, 3))
    sd, ws, cs = [], [], []
    for N in LEVELS:
        sd.append(torch.sort(rand(RAYS, N + 1), -1).values)
        w = rand(RAYS, N)
        ws.append(w / w.sum(-1, keepdim=True))
        cs.append(1.2 * rand(RAYS, N, 3))
    rendering.update(ray_sdist=sd, ray_weights=ws, ray_rgbs=cs)
    rays = types.SimpleNamespace(origins=rand(H, W, 3) - 0.5, directions=unit(H, W, 3))

    stages = dict(visualize_suite=lambda: vis.visualize_suite(rendering, rays, True),
                  depth_cmap=lambda: vis.visualize_cmap(dist, rendering["acc"], "turbo", curve_fn=vis.depth_curve_fn),
                  visualize_rays=lambda: vis.visualize_rays(sd, (0, 1), ws, cs))
    real_dispatch = vis._kernels

    def use(variant):
        vis._kernels = real_dispatch if variant == "fused" else (lambda t: False)

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
    for name, fn in stages.items():
        ms = dict(fused=[], aten=[])
        for i in range(WARM + STEPS):
            for variant in ("fused", "aten"):
                use(variant)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= WARM:
                    ms[variant].append(e0.elapsed_time(e1))
        out[name] = {}
        for variant in ("fused", "aten"):
            use(variant)
            v = np.array(ms[variant])
            before = _hip.VIS_LAUNCHES
            fn()
            torch.cuda.synchronize()
            out[name][variant] = dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)),
                                      library_launches=_hip.VIS_LAUNCHES - before, device_launches=launches(fn))
        out[name]["ratio"] = out[name]["aten"]["median_ms"] / out[name]["fused"]["median_ms"]
        print(name, {k: ({x: (round(y, 3) if isinstance(y, float) else y) for x, y in v.items()} if isinstance(v, dict) else round(v, 2))
                     for k, v in out[name].items()}, flush=True)
    # the two paths agree at this size (the ATen path's cumsum is a parallel scan on the device, in another order)
    use("fused")
    a = vis.visualize_suite(rendering, rays, True)
    use("aten")
    b = vis.visualize_suite(rendering, rays, True)
    use("fused")
    out["fused_vs_aten_linf"] = {k: float(torch.nan_to_num(a[k].double() - b[k].double()).abs().max()) for k in a}
    out["shape"] = [H, W]
    out["rays"] = [RAYS, list(LEVELS)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

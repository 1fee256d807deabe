"""The per-test-image metrics of refnerf_pl_amd.image at the size of a Blender test view (800 x 800 x 3, float64), through the
kernels of csrc/refnerf_image.h and through the ATen float64 path of the same module, in one run on one device:
    python scripts/time_metrics.py
Times image.evaluate_test_image as a whole (quantised, eval_crop_borders = 0, disparity and normal metrics on: colour
correction, two PSNR / SSIM pairs, two disparity errors, two angular errors), and colour correction and SSIM each on their
own.  HIP-event pairs around every call, 20 calls after 3 warm-up calls, median / p10 / p90 in us; device kernel launches per
call from torch.profiler.  The two paths alternate call by call inside each timed loop's variant order (fused, aten, fused,
aten ...) so that both see the same machine.  One JSON line at the end: per stage both variants and ratio = aten / fused
(> 1: the kernels are faster)."""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARM = 20, 3
H, W = 800, 800


def main():
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, image
    _hip.require_device()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)

    def rand(*shape, dtype=torch.float32):
        return torch.rand(shape, device=dev, generator=gen, dtype=dtype)

    def unit(*shape):
        v = rand(*shape) - 0.5
        return v / v.norm(dim=-1, keepdim=True)
    # a smooth image, a colour warp of it plus noise (what colour correction is for), and the other fields of a rendering
    yy, xx = torch.meshgrid(torch.arange(H, device=dev) / H, torch.arange(W, device=dev) / W, indexing="ij")
    # (a direction of its own per channel: three channels of one sinusoid would put every pixel on one curve in colour space,
    # and the ten-term system of the correction would be close to singular)
    gt = torch.stack([0.5 + 0.3 * torch.sin(fx * xx + fy * yy + p) for fx, fy, p in ((6.0, 4.0, 0.0), (3.0, 7.0, 1.0), (8.0, -2.0, 2.0))], -1)
    gt = gt + 0.03 * (rand(H, W, 3) - 0.5)
    gt = gt.clamp(0, 1).float()
    rgb = (0.9 * gt ** 1.1 + 0.03 + 0.01 * (rand(H, W, 3) - 0.5)).clamp(0, 1)
    dist = 2.0 + 4.0 * rand(H, W)
    rendering = dict(rgb=rgb, distance_mean=dist, distance_median=dist + 0.05 * rand(H, W), acc=rand(H, W), normals=unit(H, W, 3),
                     normals_pred=unit(H, W, 3))
    batch = types.SimpleNamespace(rgb=gt, disps=1 / (1 + dist) + 0.01 * rand(H, W), normals=unit(H, W, 3), alphas=rand(H, W))
    cfg = types.SimpleNamespace(eval_quantize_metrics=True, eval_crop_borders=0, compute_disp_metrics=True, compute_normal_metrics=True)
    a64, b64 = rgb.double(), gt.double()

    stages = dict(evaluate_test_image=lambda: image.evaluate_test_image(rendering, batch, cfg),
                  color_correct=lambda: image.color_correct(a64, b64),
                  ssim=lambda: image.ssim(a64, b64))
    real_dispatch = image._kernels

    def use(variant):
        image._kernels = real_dispatch if variant == "fused" else (lambda t: False)

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
        us = dict(fused=[], aten=[])
        for i in range(WARM + STEPS):
            for variant in ("fused", "aten"):
                use(variant)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= WARM:
                    us[variant].append(e0.elapsed_time(e1) * 1e3)
        out[name] = {}
        for variant in ("fused", "aten"):
            use(variant)
            v = np.array(us[variant])
            out[name][variant] = dict(median_us=float(np.median(v)), p10_us=float(np.percentile(v, 10)),
                                      p90_us=float(np.percentile(v, 90)), launches=launches(fn))
        out[name]["ratio"] = out[name]["aten"]["median_us"] / out[name]["fused"]["median_us"]
        print(name, {k: ({x: (round(y, 1) if isinstance(y, float) else y) for x, y in v.items()} if isinstance(v, dict) else round(v, 2))
                     for k, v in out[name].items()}, flush=True)
    use("fused")
    # the two paths agree at this size (the ATen path's pinv is torch's, the kernels' a Jacobi solve)
    cc_f = image.color_correct(a64, b64)
    use("aten")
    cc_a = image.color_correct(a64, b64)
    use("fused")
    out["color_correct_fused_vs_aten_linf"] = float((cc_f - cc_a).abs().max())
    out["shape"] = [H, W, 3]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

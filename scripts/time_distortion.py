"""mip-NeRF 360's distortion loss, forward + backward to the last level's weights, through the ATen definition
(train_utils.distortion_loss: O(N^2) per ray, [R, N, N] intermediates) and through the O(N) kernels
(train_utils.fused_distortion_loss -> refnerf_distortion_forward / _backward):
    python scripts/time_distortion.py
Shapes (rays x samples): 4096 x 32, 4096 x 128 and 2048 x 256 (one shard of a 16384-ray batch at 256 samples), seeded step
functions (sorted uniform knots on [0, 1], softmax weights).  Both paths IN THE SAME PROCESS, alternating call by call so that
both see the same machine state: a HIP-event pair around every call, 20 calls per path after 5 warm-up calls, median
(p10 - p90) in us.  Kernel launches per call from torch.profiler and torch.cuda.max_memory_allocated above the resident inputs
(each from a separate, untimed call).  One JSON line at the end; ratio = ATen / fused (>= 1: the fused path does not lose)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 32), (4096, 128), (2048, 256)]
CALLS, WARM = 20, 5


def main():
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, configs, train_utils
    _hip.require_device()
    dev = torch.device("cuda:0")
    configs.clear_config()
    cfg = configs.Config(hip_distortion_loss=True)
    assert cfg.distortion_loss_mult > 0
    gen = torch.Generator(device=dev).manual_seed(0)
    paths = (("aten", train_utils.distortion_loss), ("fused", train_utils.fused_distortion_loss))

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
    for R, N in SHAPES:
        t = torch.sort(torch.rand((R, N + 1), device=dev, generator=gen), dim=-1).values
        t[:, 0], t[:, -1] = 0.0, 1.0
        w = torch.softmax(2.0 * torch.randn((R, N), device=dev, generator=gen), dim=-1).requires_grad_(True)
        hist = [dict(sdist=t.contiguous(), weights=w)]
        assert train_utils.fused_distortion_supported(hist)

        def call(fn):
            w.grad = None
            fn(hist, cfg).backward()

        us = {name: [] for name, _ in paths}
        for _ in range(WARM):
            for _, fn in paths:
                call(fn)
        torch.cuda.synchronize()
        for _ in range(CALLS):
            for name, fn in paths:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(fn)
                e1.record()
                torch.cuda.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3)
        res = {}
        for name, fn in paths:
            a = np.array(us[name])
            w.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            call(fn)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            res[name] = dict(median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)), p90_us=float(np.percentile(a, 90)),
                             launches=launches(lambda: call(fn)), peak_bytes_above_inputs=int(peak),
                             loss=float(fn(hist, cfg).detach()))
        res["ratio"] = res["aten"]["median_us"] / res["fused"]["median_us"]
        out[f"{R}x{N}"] = res
        a, f = res["aten"], res["fused"]
        print(f"{R} x {N}: ATen {a['median_us']:.0f} us ({a['p10_us']:.0f} - {a['p90_us']:.0f}; {a['launches']} launches, "
              f"{a['peak_bytes_above_inputs'] / 2 ** 20:.1f} MiB), fused {f['median_us']:.0f} us ({f['p10_us']:.0f} - {f['p90_us']:.0f}; "
              f"{f['launches']} launches, {f['peak_bytes_above_inputs'] / 2 ** 20:.2f} MiB), ratio {res['ratio']:.1f}; "
              f"loss {a['loss']:.6e} / {f['loss']:.6e}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

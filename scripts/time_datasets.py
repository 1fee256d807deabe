"""The two device stages of the scene loaders against what they replace, in one run on one device:
    python scripts/time_datasets.py
1. Image preparation: a Blender-sized stack, 100 x 800 x 800 x 4 uint8, composited on white at factor 1 and 2:
   (a) datasets.prepare_images on the device: refnerf_prepare_images on the resident uint8 stack (one launch), and the same
       including the upload of the 256 MB stack from pageable host memory;
   (b) datasets.prepare_images_host: the numpy float32 path of the same module (the reference's operations).
   (a) is timed with HIP-event pairs, 20 calls after 5 warm-up calls; (b) with the wall clock, 3 calls after 1 (a call takes
   seconds).  The two results are compared bit for bit.
2. One training batch of 4096 and of 512 rays, patch_size 1, 'all_images', from the 100 prepared images:
   (a) SceneDataset.next(): three torch.randint draws + ONE launch of refnerf_train_batch;
   (b) TrainRayBatcher.next(): the step-by-step ATen path + refnerf_pixels_to_rays.
   HIP-event pairs around every call, 20 calls after 5 warm-up calls, the two paths alternating call by call so that both
   see the same machine; median / p10 / p90 in ms, the library launches of one call from the timing families and the device
   kernels of one call from torch.profiler.
Nothing is asserted on time.  One JSON line at the end."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARM = 20, 5
HOST_STEPS, HOST_WARM = 3, 1
N, H, W = 100, 800, 800
NEAR, FAR = 2.0, 6.0


def stats(ms):
    import numpy as np
    t = np.array(ms)
    return dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)))


def main():
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, camera_utils, configs, datasets, synthetic
    _hip.require_device()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rgba = rng.integers(0, 256, (N, H, W, 4), dtype=np.uint8)
    resident = torch.from_numpy(rgba).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), res

    def kernels_of(fn):
        from torch.profiler import ProfilerActivity, profile
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return {e.key: int(e.count) for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA}
        except Exception as e:      # the profiler is a convenience here, the timing is the result
            return repr(e)

    def library_launches(fn):
        torch.cuda.synchronize()
        _hip.set_timing(True)
        fn()
        n = sum(_hip.get_timing(f)[1] for f in range(5))
        _hip.set_timing(False)
        return n

    out = dict(prepare={}, train_batch={}, stack=[N, H, W, 4], threads_per_block=256)
    images = None
    for factor in (1, 2):
        variants = dict(kernel=lambda: _hip.prepare_images(resident, _hip.PREP_WHITE, factor, return_alpha=True),
                        upload_and_kernel=lambda: datasets.prepare_images(rgba, _hip.PREP_WHITE, factor, return_alpha=True, device=dev))
        ms = {v: [] for v in variants}
        for i in range(WARM + STEPS):
            for v, fn in variants.items():
                t, res = timed(fn)
                if i >= WARM:
                    ms[v].append(t)
                del res
        row = {v: stats(ms[v]) for v in variants}
        host_ms = []
        for i in range(HOST_WARM + HOST_STEPS):
            t0 = time.perf_counter()
            want = datasets.prepare_images_host(rgba, _hip.PREP_WHITE, factor, return_alpha=True)
            if i >= HOST_WARM:
                host_ms.append(1e3 * (time.perf_counter() - t0))
        row["host_numpy"] = stats(host_ms)
        got = variants["kernel"]()
        row["bit_equal"] = all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))
        src_bytes, out_bytes = rgba.nbytes, sum(g.numel() * 4 for g in got)
        row["kernel_GBps"] = (src_bytes + out_bytes) / (row["kernel"]["median_ms"] * 1e-3) / 1e9
        row["host_over_kernel"] = row["host_numpy"]["median_ms"] / row["kernel"]["median_ms"]
        row["host_over_upload_and_kernel"] = row["host_numpy"]["median_ms"] / row["upload_and_kernel"]["median_ms"]
        out["prepare"][f"factor_{factor}"] = row
        print("prepare factor", factor, {k: ({x: round(y, 3) for x, y in v.items()} if isinstance(v, dict) else v) for k, v in row.items()}, flush=True)
        if factor == 1:
            images = got[0]
        del got, want
    del resident

    p2c = camera_utils.get_pixtocam(1111.0, W, H)
    c2w = np.stack([np.concatenate([synthetic._rot(k), synthetic._rot(k) @ np.array([[0.0], [0.0], [4.0]])], -1) for k in range(N)]).astype(np.float32)
    cams = (p2c, c2w, None, None)
    for batch_size in (4096, 512):
        cfg = configs.Config(batch_size=batch_size, patch_size=1, batching="all_images", near=NEAR, far=FAR)
        fused = datasets.ArrayScene(cfg, images, cams, device=dev, seed=1)
        steps = datasets.TrainRayBatcher(images, cams, NEAR, FAR, batch_size, 1, "all_images", seed=1, device=dev)
        variants = dict(train_batch=fused.next, ray_batcher=steps.next)
        a, b = fused.next(), steps.next()
        equal = all(torch.equal(getattr(a.rays, k), getattr(b.rays, k)) for k in _hip.RAY_FIELDS) and torch.equal(a.rgb, b.rgb)
        ms = {v: [] for v in variants}
        for i in range(WARM + STEPS):
            for v, fn in variants.items():
                t, _ = timed(fn)
                if i >= WARM:
                    ms[v].append(t)
        row = {}
        for v, fn in variants.items():
            kernels = kernels_of(fn)
            row[v] = dict(stats(ms[v]), library_launches=library_launches(fn),
                          device_kernels=sum(kernels.values()) if isinstance(kernels, dict) else kernels, kernels=kernels)
        row["ratio"] = row["ray_batcher"]["median_ms"] / row["train_batch"]["median_ms"]
        row["bit_equal"] = equal
        out["train_batch"][f"rays_{batch_size}"] = row
        print("train batch", batch_size, {k: ({x: (round(y, 4) if isinstance(y, float) else y) for x, y in v.items() if x != "kernels"}
                                               if isinstance(v, dict) else v) for k, v in row.items()}, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""The rays of one whole frame, cast on the device two ways, in one run on one device:
    python scripts/time_render_path.py
(a) camera_utils.cast_image_rays: refnerf_image_rays, all nine Rays fields from (width, height, camera, pose) in one launch,
    the pose path resident on the device as datasets.PathCameras keeps it;
(b) camera_utils.cast_pinhole_rays: pixel_coordinates (a meshgrid, two int32 pixel images) + pixels_to_rays + four fills.
Both at 1008 x 756 (an LLFF frame at factor 4), and (a) alone for the 1024 x 512 panorama (cast_spherical_rays has no
counterpart before refnerf_image_rays).  HIP-event pairs around every call, 20 calls after 5 warm-up calls, the two paths
alternating call by call so that both see the same machine; median / p10 / p90 in ms, and the device kernel launches of
one call from torch.profiler.  Nothing is asserted on time; the structural claim is: (a) is ONE device launch per frame.
One JSON line at the end."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WARM = 20, 5
W, H, FOCAL = 1008, 756, 815.0
PANO_W, PANO_H = 1024, 512
NEAR, FAR = 0.0, 1.0


def main():
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, camera_utils, synthetic
    _hip.require_device()
    dev = torch.device("cuda:0")
    c2w = np.concatenate([synthetic._rot(11), synthetic._rot(11) @ np.array([[0.0], [0.0], [4.0]])], -1).astype(np.float32)
    path = torch.as_tensor(np.stack([c2w] * 4), device=dev)              # a 4-frame path, uploaded once
    p2c = torch.as_tensor(camera_utils.get_pixtocam(FOCAL, W, H), device=dev)

    stages = dict(
        pinhole=dict(image_rays=lambda: camera_utils.cast_image_rays((p2c, path, None, None), 3, H, W, NEAR, FAR, device=dev),
                     pixels_to_rays=lambda: camera_utils.cast_pinhole_rays(c2w, H, W, FOCAL, NEAR, FAR, device=dev)),
        spherical=dict(image_rays=lambda: camera_utils.cast_image_rays((None, path, None, None), 3, PANO_H, PANO_W, NEAR, FAR,
                                                                       spherical=True, device=dev)))

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return {e.key: int(e.count) for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA}
        except Exception as e:      # the profiler is a convenience here, the timing is the result
            return repr(e)

    out = {}
    for name, variants in stages.items():
        ms = {v: [] for v in variants}
        for i in range(WARM + STEPS):
            for v, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= WARM:
                    ms[v].append(e0.elapsed_time(e1))
        out[name] = {}
        for v, fn in variants.items():
            t = np.array(ms[v])
            kernels = launches(fn)
            out[name][v] = dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)),
                                device_launches=sum(kernels.values()) if isinstance(kernels, dict) else kernels, kernels=kernels)
        if len(variants) == 2:
            out[name]["ratio"] = out[name]["pixels_to_rays"]["median_ms"] / out[name]["image_rays"]["median_ms"]
        print(name, {k: ({x: (round(y, 4) if isinstance(y, float) else y) for x, y in v.items() if x != "kernels"}
                         if isinstance(v, dict) else round(v, 2)) for k, v in out[name].items()}, flush=True)
    a, b = stages["pinhole"]["image_rays"](), stages["pinhole"]["pixels_to_rays"]()
    out["pinhole"]["bit_equal"] = all(torch.equal(getattr(a, k), getattr(b, k)) for k in _hip.RAY_FIELDS[:-1])
    out["pinhole"]["shape"], out["spherical"]["shape"] = [H, W], [PANO_H, PANO_W]
    out["bytes_per_ray_out"] = 4 * sum(_hip.RAY_FIELD_WIDTHS)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

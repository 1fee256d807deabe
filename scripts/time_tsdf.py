"""Geometry export (refnerf_pl_amd.geometry): fusing one 800 x 800 view into a 256^3 colour TSDF volume through the kernel
(refnerf_tsdf_integrate) and through the ATen float64 formulation of the same update (geometry.integrate_aten: projection,
gather, masked running average), and extracting the mesh of the fused sphere (refnerf_tsdf_mesh_count + _emit; against
nothing: recorded only):
    python scripts/time_tsdf.py
The scene is analytic: a sphere of radius 0.5 in front of a back plane behind the volume, six views on the axes at distance
2.5, focal 1111.
Both integrate paths IN THE SAME PROCESS, alternating call by call, each on a volume of its own that keeps accumulating the
same view (the update touches the same voxels every call): a HIP-event pair around every call, 20 calls per path after 5
warm-up calls, median (p10 - p90) in us.  Kernel launches per call from torch.profiler (a separate, untimed call).  Bytes
moved: 40 B per updated voxel (tsdf, weight and colour read and written) plus the view, against the 8 TB/s of the project's
rooflines.  One JSON line at the end; ratio = ATen / kernel."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES, SIZE, FOCAL, RADIUS, DIST, BACK = 256, 800, 1111.0, 0.5, 2.5, 3.6
CALLS, WARM = 20, 5
PEAK_BYTES_PER_S = 8e12


def look_at(eye):
    import numpy as np
    eye = np.asarray(eye, np.float64)
    z = eye / np.linalg.norm(eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1).astype(np.float32)


def view_of_the_sphere(torch, dev):
    """(depth [H,W], acc, rgb) of the sphere seen from distance DIST along the optical axis: the z-depth of the first hit, the
    back plane at z-depth BACK elsewhere -- the same image for every pose on a sphere around the origin"""
    x = (torch.arange(SIZE, device=dev, dtype=torch.float64) + 0.5 - SIZE / 2) / FOCAL
    dx, dy = torch.meshgrid(x, x, indexing="xy")
    a = dx * dx + dy * dy + 1.0                       # |d|^2 of d = (dx, dy, 1), origin at z = -DIST from the centre
    disc = DIST * DIST - a * (DIST * DIST - RADIUS * RADIUS)
    depth = torch.where(disc > 0, (DIST - torch.sqrt(disc.clamp(min=0))) / a, torch.full_like(a, BACK))
    rgb = torch.stack([dx, dy, torch.ones_like(dx)], -1).abs().clamp(0, 1)
    return depth.float().contiguous(), torch.ones_like(depth).float(), rgb.float().contiguous()


def main():
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, camera_utils, geometry
    _hip.require_device()
    dev = torch.device("cuda:0")
    depth, acc, rgb = view_of_the_sphere(torch, dev)
    p2c = torch.as_tensor(camera_utils.get_pixtocam(FOCAL, SIZE, SIZE), dtype=torch.float32, device=dev).contiguous()
    poses = [look_at(e) for e in ((DIST, 0, 0), (-DIST, 0, 0), (0, DIST, 0), (0, -DIST, 0), (0, 0, DIST), (0, 0, -DIST))]
    c2w = torch.as_tensor(np.stack(poses), device=dev)

    def volume():
        return geometry.TSDFVolume((-1, -1, -1), (1, 1, 1), resolution=RES, device=dev)
    vols = {"aten": volume(), "kernel": volume()}
    v = vols["kernel"]

    def integrate(name):
        vol = vols[name]
        if name == "kernel":
            _hip.tsdf_integrate(vol.grid, vol.tsdf, vol.weight, vol.rgb, p2c, c2w, 0, depth, acc, 0.5, rgb, 1.0, 0.0)
        else:
            geometry.integrate_aten(vol.dims, vol.origin, vol.voxel_size, vol.trunc, vol.tsdf, vol.weight, vol.rgb, p2c, c2w[0], depth,
                                    acc, 0.5, rgb, 1.0, 0.0)

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
        except Exception as e:      # the profiler is a convenience here, the timing is the result
            return repr(e)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    def stats(us):
        a = np.array(us)
        return dict(median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)), p90_us=float(np.percentile(a, 90)))

    us = {name: [] for name in vols}
    for _ in range(WARM):
        for name in vols:
            integrate(name)
    torch.cuda.synchronize()
    for _ in range(CALLS):
        for name in vols:
            us[name].append(timed(lambda: integrate(name))[0])
    same = all(torch.equal(getattr(vols["aten"], k), getattr(vols["kernel"], k)) for k in ("tsdf", "weight", "rgb"))
    updated = int((v.weight > 0).sum())
    moved = 40 * updated + 4 * 5 * SIZE * SIZE
    out = {"integrate": {name: dict(stats(us[name]), launches=launches(lambda: integrate(name))) for name in vols}}
    res = out["integrate"]
    res.update(voxels=RES ** 3, updated_voxels=updated, bytes_moved=moved, bit_equal=bool(same),
               ratio=res["aten"]["median_us"] / res["kernel"]["median_us"],
               kernel_fraction_of_peak=moved / (res["kernel"]["median_us"] * 1e-6) / PEAK_BYTES_PER_S)
    a, k = res["aten"], res["kernel"]
    print(f"integrate {SIZE} x {SIZE} into {RES}^3 with colour ({updated} voxels updated, {moved / 1e6:.0f} MB): ATen "
          f"{a['median_us']:.0f} us ({a['p10_us']:.0f} - {a['p90_us']:.0f}; {a['launches']} launches), kernel {k['median_us']:.0f} us "
          f"({k['p10_us']:.0f} - {k['p90_us']:.0f}; {k['launches']} launches, {100 * res['kernel_fraction_of_peak']:.0f} % of 8 TB/s), "
          f"ratio {res['ratio']:.1f}; bit-equal {same}", flush=True)

    # the mesh of the sphere fused from six views
    vol = volume()
    for frame in range(len(poses)):
        _hip.tsdf_integrate(vol.grid, vol.tsdf, vol.weight, vol.rgb, p2c, c2w, frame, depth, acc, 0.5, rgb, 1.0, 0.0)
    del vols, v
    ex = []
    for n in range(WARM + CALLS):
        t, mesh = timed(vol.extract_mesh)
        if n >= WARM:
            ex.append(t)
    vertices, faces, colors = mesh
    radius = vertices.double().norm(dim=1)
    out["extract_mesh"] = dict(stats(ex), launches=launches(vol.extract_mesh), vertices=int(vertices.shape[0]), triangles=int(faces.shape[0]),
                               workspace_bytes=_hip.tsdf_mesh_workspace_bytes(vol.grid),
                               radius_min=float(radius.min()), radius_max=float(radius.max()))
    e = out["extract_mesh"]
    print(f"extract_mesh of the fused sphere at {RES}^3: {e['median_us']:.0f} us ({e['p10_us']:.0f} - {e['p90_us']:.0f}; {e['launches']} "
          f"launches incl. the read of the two counts), {e['vertices']} vertices, {e['triangles']} triangles, |v| in "
          f"[{e['radius_min']:.4f}, {e['radius_max']:.4f}], workspace {e['workspace_bytes'] / 1e6:.1f} MB", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

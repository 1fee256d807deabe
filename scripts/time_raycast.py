"""Views of the exported volume (refnerf_pl_amd.geometry): one 800 x 800 ray-cast view of the six-view sphere volume of
scripts/time_tsdf.py at 256^3 with colour, through the kernel (refnerf_tsdf_raycast) and through an ATen float64 formulation
of the same march (`raycast_aten` below: the lines of include/refnerf_raycast.h on whole-image tensors, one masked update per
sample index k, no compaction):
    python scripts/time_raycast.py
Both paths IN THE SAME PROCESS, alternating call by call on the same volume: a HIP-event pair around every call, 20 calls per
path after 5 warm-up calls, median (p10 - p90) in us; the four output images compared bit for bit afterwards.  Recorded, not
gated: there is no earlier ray caster to compare with.  One JSON line at the end; ratio = ATen / kernel."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEP, REFINE = 0.5, 4


def raycast_aten(torch, vol, p2c, c2w, W, H, iso=0.0, min_weight=1.0, step=STEP, refine=REFINE, t_near=0.0, t_far=float("inf")):
    """(depth, normals, rgb, acc) of include/refnerf_raycast.h as ATen operations in float64 on the volume's device"""
    f64, dev = torch.float64, vol.tsdf.device
    nx, ny, nz = vol.dims
    n = (nx, ny, nz)
    flat, seen, colour = vol.tsdf.reshape(-1), vol.weight.reshape(-1) >= min_weight, vol.rgb.reshape(-1, 3)
    org, h = [float(v) for v in vol.origin], float(vol.voxel_size)
    K, M = p2c.to(f64), c2w.to(f64)
    sy, sz = nx, nx * ny
    corner = torch.tensor([(m & 1) + (m >> 1 & 1) * sy + (m >> 2 & 1) * sz for m in range(8)], device=dev)[:, None]
    zero_f = torch.zeros((), dtype=f64, device=dev)

    def cell(t):
        i, fr = [], []
        for a in range(3):
            g = ((o[a] + t * d[a]) - org[a]) / h
            f = torch.floor(g)
            ia = torch.where(f > 0, torch.where(f < n[a] - 2, f, torch.full_like(f, n[a] - 2)), zero_f)
            i.append(ia.long())
            fr.append(g - ia)
        p = (i[2] * sz + i[1] * sy) + i[0]
        q = p[None, :] + corner
        return flat[q].to(f64), fr, seen[q].all(0), q

    def lerp3(c, fr):
        x = [c[2 * r] + fr[0] * (c[2 * r + 1] - c[2 * r]) for r in range(4)]
        y = [x[2 * r] + fr[1] * (x[2 * r + 1] - x[2 * r]) for r in range(2)]
        return y[0] + fr[2] * (y[1] - y[0])

    py, px = torch.meshgrid(torch.arange(H, device=dev, dtype=f64) + 0.5, torch.arange(W, device=dev, dtype=f64) + 0.5, indexing="ij")
    px, py = px.reshape(-1), py.reshape(-1)
    cx = K[0, 0] * px + K[0, 1] * py + K[0, 2]
    cy = -(K[1, 0] * px + K[1, 1] * py + K[1, 2])
    d = [M[a, 0] * cx + M[a, 1] * cy + M[a, 2] * -1.0 for a in range(3)]
    o = [M[a, 3] for a in range(3)]
    t0, t1 = torch.full_like(px, t_near), torch.full_like(px, t_far)
    miss = torch.zeros_like(px, dtype=torch.bool)
    for a in range(3):
        lo, hi = org[a], org[a] + float(n[a] - 1) * h
        zero = d[a] == 0
        miss |= zero & ~((lo <= o[a]) & (o[a] <= hi))
        ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
        lo_t, hi_t = torch.where(ta < tb, ta, tb), torch.where(ta > tb, ta, tb)
        t0 = torch.where(zero, t0, torch.where(t0 > lo_t, t0, lo_t))
        t1 = torch.where(zero, t1, torch.where(t1 < hi_t, t1, hi_t))
    miss |= ~(t1 >= t0)
    dt = step * h / torch.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    N = torch.floor((t1 - t0) / dt)
    miss |= ~(N <= float(nx + ny + nz) / step)
    last = int(torch.where(miss, torch.full_like(N, -1.0), N).max())           # the one host read: the length of the loop

    prev, hit = torch.zeros_like(miss), torch.zeros_like(miss)
    v_prev, t_prev = torch.zeros_like(px), torch.zeros_like(px)
    a_t, b_t, fa, fb = (torch.zeros_like(px) for _ in range(4))
    for k in range(last + 1):
        active = ~miss & ~hit & (N >= k)
        t = t0 + float(k) * dt
        c, fr, ok, _ = cell(t)
        v = lerp3(c, fr) - iso
        new = active & ok & prev & (v_prev >= 0) & (v < 0)
        a_t, b_t, fa, fb = torch.where(new, t_prev, a_t), torch.where(new, t, b_t), torch.where(new, v_prev, fa), torch.where(new, v, fb)
        hit |= new
        keep = active & ~new
        prev = torch.where(keep, ok, prev)
        v_prev, t_prev = torch.where(keep & ok, v, v_prev), torch.where(keep & ok, t, t_prev)
    for _ in range(refine):
        tm = 0.5 * (a_t + b_t)
        c, fr, _, _ = cell(tm)
        vm = lerp3(c, fr) - iso
        neg = vm < 0
        a_t, fa, b_t, fb = torch.where(neg, a_t, tm), torch.where(neg, fa, vm), torch.where(neg, tm, b_t), torch.where(neg, vm, fb)
    ts = a_t + (fa / (fa - fb)) * (b_t - a_t)
    c, fr, _, q = cell(ts)
    u = [1.0 - fr[a] for a in range(3)]
    gx = u[1] * u[2] * (c[1] - c[0]) + fr[1] * u[2] * (c[3] - c[2]) + u[1] * fr[2] * (c[5] - c[4]) + fr[1] * fr[2] * (c[7] - c[6])
    gy = u[0] * u[2] * (c[2] - c[0]) + fr[0] * u[2] * (c[3] - c[1]) + u[0] * fr[2] * (c[6] - c[4]) + fr[0] * fr[2] * (c[7] - c[5])
    gz = u[0] * u[1] * (c[4] - c[0]) + fr[0] * u[1] * (c[5] - c[1]) + u[0] * fr[1] * (c[6] - c[2]) + fr[0] * fr[1] * (c[7] - c[3])
    s = torch.sqrt(gx * gx + gy * gy + gz * gz)
    zero32 = torch.zeros((), dtype=torch.float32, device=dev)
    depth = torch.where(hit, ts.float(), zero32)
    normals = torch.where((hit & (s > 0))[:, None], torch.stack([gx / s, gy / s, gz / s], -1).float(), zero32)
    rgb = torch.where(hit[:, None], torch.stack([lerp3(colour[:, ch][q].to(f64), fr) for ch in range(3)], -1).float(), zero32)
    return depth.reshape(H, W), normals.reshape(H, W, 3), rgb.reshape(H, W, 3), hit.float().reshape(H, W)


def main():
    import numpy as np
    import torch

    import refnerf_pl_amd  # noqa: F401
    import time_tsdf as TT
    from refnerf_pl_amd import _hip, camera_utils, geometry
    _hip.require_device()
    dev = torch.device("cuda:0")
    RES, SIZE, CALLS, WARM = TT.RES, TT.SIZE, TT.CALLS, TT.WARM
    depth, acc, rgb = TT.view_of_the_sphere(torch, dev)
    p2c = torch.as_tensor(camera_utils.get_pixtocam(TT.FOCAL, SIZE, SIZE), dtype=torch.float32, device=dev).contiguous()
    D = TT.DIST
    poses = [TT.look_at(e) for e in ((D, 0, 0), (-D, 0, 0), (0, D, 0), (0, -D, 0), (0, 0, D), (0, 0, -D))]
    c2w = torch.as_tensor(np.stack(poses), device=dev)
    vol = geometry.TSDFVolume((-1, -1, -1), (1, 1, 1), resolution=RES, device=dev)
    for frame in range(len(poses)):
        _hip.tsdf_integrate(vol.grid, vol.tsdf, vol.weight, vol.rgb, p2c, c2w, frame, depth, acc, 0.5, rgb, 1.0, 0.0)
    # the view: an oblique pose none of the six fused ones, at the same distance
    eye = np.array([1.0, 0.7, 0.5]) / np.linalg.norm([1.0, 0.7, 0.5]) * D
    view = torch.as_tensor(TT.look_at(eye)[None], device=dev)

    paths = {"aten": lambda: raycast_aten(torch, vol, p2c, view[0], SIZE, SIZE),
             "kernel": lambda: _hip.tsdf_raycast(vol.grid, vol.tsdf, vol.weight, vol.rgb, p2c, view, 0, SIZE, SIZE, 0.0, 1.0, STEP, REFINE)}

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

    us, outs = {name: [] for name in paths}, {}
    for _ in range(WARM):
        for name, fn in paths.items():
            fn()
    torch.cuda.synchronize()
    for _ in range(CALLS):
        for name, fn in paths.items():
            t, outs[name] = timed(fn)
            us[name].append(t)
    same = {k: bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for k, a, b in zip(("depth", "normals", "rgb", "acc"), outs["aten"], outs["kernel"])}
    worst = {k: float((a.double() - b.double()).abs().max()) for k, a, b in zip(("depth", "normals", "rgb", "acc"), outs["aten"], outs["kernel"])}
    k_depth, k_normals, _, k_acc = outs["kernel"]
    hit = k_acc > 0
    # the hit points, from the header's camera lines in double: their radii and the normals' angles to the sphere's
    ys, xs = torch.meshgrid(torch.arange(SIZE, device=dev, dtype=torch.float64) + 0.5, torch.arange(SIZE, device=dev, dtype=torch.float64) + 0.5,
                            indexing="ij")
    K, M = p2c.double(), view[0].double()
    cam = torch.stack([K[0, 0] * xs + K[0, 1] * ys + K[0, 2], -(K[1, 0] * xs + K[1, 1] * ys + K[1, 2]), -torch.ones_like(xs)], -1)
    P = M[:, 3] + k_depth.double()[..., None] * (cam @ M[:, :3].T)
    radius = P[hit].norm(dim=-1)
    cosine = (k_normals.double()[hit] * (P[hit] / radius[:, None])).sum(-1)
    angle = torch.rad2deg(torch.acos(cosine.clamp(-1, 1)))
    res = {name: stats(us[name]) for name in paths}
    res.update(view=[SIZE, SIZE], voxels=RES ** 3, step=STEP, refine=REFINE, hits=int(hit.sum()), bit_equal=same, worst_abs_difference=worst,
               ratio=res["aten"]["median_us"] / res["kernel"]["median_us"], radius_min=float(radius.min()), radius_max=float(radius.max()),
               normal_angle_median_deg=float(angle.median()), normal_angle_max_deg=float(angle.max()))
    a, k = res["aten"], res["kernel"]
    print(f"raycast {SIZE} x {SIZE} of {RES}^3 with colour, step {STEP}, refine {REFINE} ({res['hits']} hits): ATen {a['median_us']:.0f} us "
          f"({a['p10_us']:.0f} - {a['p90_us']:.0f}), kernel {k['median_us']:.0f} us ({k['p10_us']:.0f} - {k['p90_us']:.0f}), ratio "
          f"{res['ratio']:.1f}; bit-equal {same}; |P| in [{res['radius_min']:.4f}, {res['radius_max']:.4f}] for r = {TT.RADIUS}, normal "
          f"against the sphere's: median {res['normal_angle_median_deg']:.2f} deg, worst {res['normal_angle_max_deg']:.2f} deg", flush=True)
    print(json.dumps({"raycast": res}))


if __name__ == "__main__":
    main()

"""Fixtures and the plain-loop mirror of include/refnerf_raycast.h for tests/test_raycast.py and
tests/test_guard_bands_raycast.py.

`raycast_mirror` is the header's definition as one Python loop per pixel, per sample, per corner, on float64 scalars, in the
header's order, each stored value rounded once to float32: an exact restatement, which geometry.raycast_host (vectorised) and
the kernel must equal bit for bit.  The volumes and views come from tsdf_cases (seeds and formulas; nothing is captured)."""
import functools

import numpy as np

import tsdf_cases as TC

INF = float("inf")


def raycast_mirror(dims, origin, h, tsdf, weight, rgb, pixtocam, camtoworld, width, height, iso=0.0, min_weight=1.0, step=0.5, refine=4,
                   t_near=0.0, t_far=INF, trace=None):
    """(depth [H,W], normals [H,W,3], rgb [H,W,3] | None, acc [H,W]) float32.  trace: a dict that receives `invalid` [H,W],
    the number of invalid samples each ray met before its hit (or its end), and `a`, `fa` [H,W]: the near end of the hit
    bracket and its value before refinement (NaN without a hit)."""
    f64 = np.float64
    n = tuple(int(v) for v in dims)
    W, H = int(width), int(height)
    f = np.asarray(tsdf, np.float32)
    w = np.asarray(weight, np.float32)
    col = None if rgb is None else np.asarray(rgb, np.float32)
    org = [f64(np.float32(v)) for v in origin]
    h, iso, step, mw = f64(np.float32(h)), f64(np.float32(iso)), f64(np.float32(step)), np.float32(min_weight)
    near, far = f64(np.float32(t_near)), f64(np.float32(t_far))
    K, M = np.asarray(pixtocam, np.float32).astype(f64), np.asarray(camtoworld, np.float32).astype(f64)
    depth, acc = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    normals = np.zeros((H, W, 3), np.float32)
    view_rgb = None if col is None else np.zeros((H, W, 3), np.float32)
    invalid = np.zeros((H, W), np.int64)
    near_end, near_value = np.full((H, W), np.nan), np.full((H, W), np.nan)
    if trace is not None:
        trace.update(invalid=invalid, a=near_end, fa=near_value)

    def sample(o, d, t):
        i, fr = [], []
        for a in range(3):
            g = ((o[a] + t * d[a]) - org[a]) / h
            fl = np.floor(g)
            ia = 0 if not fl > 0 else (int(fl) if fl < n[a] - 2 else n[a] - 2)
            i.append(ia)
            fr.append(g - f64(ia))
        corners = [(i[2] + (m >> 2 & 1), i[1] + (m >> 1 & 1), i[0] + (m & 1)) for m in range(8)]
        ok = True
        for idx in corners:
            ok = ok and bool(w[idx] >= mw)
        return [f64(f[idx]) for idx in corners], fr, ok, corners

    def lerp3(c, fr):
        x = [c[m] + fr[0] * (c[m + 1] - c[m]) for m in (0, 2, 4, 6)]
        y = [x[0] + fr[1] * (x[1] - x[0]), x[2] + fr[1] * (x[3] - x[2])]
        return y[0] + fr[2] * (y[1] - y[0])

    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                px, py = f64(x + 0.5), f64(y + 0.5)
                cx = K[0, 0] * px + K[0, 1] * py + K[0, 2]
                cy = -(K[1, 0] * px + K[1, 1] * py + K[1, 2])
                cz = f64(-1.0)
                d = [M[a, 0] * cx + M[a, 1] * cy + M[a, 2] * cz for a in range(3)]
                o = [M[a, 3] for a in range(3)]
                t0, t1, miss = near, far, False
                for a in range(3):
                    lo, hi = org[a], org[a] + f64(n[a] - 1) * h
                    if d[a] == 0:
                        if not (lo <= o[a] and o[a] <= hi):
                            miss = True
                    else:
                        ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
                        lo_t, hi_t = (ta if ta < tb else tb), (ta if ta > tb else tb)
                        t0 = t0 if t0 > lo_t else lo_t
                        t1 = t1 if t1 < hi_t else hi_t
                if miss or not t1 >= t0:
                    continue
                dt = step * h / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                N = np.floor((t1 - t0) / dt)
                if not N <= f64(n[0] + n[1] + n[2]) / step:
                    continue
                prev, v_prev, t_prev = False, f64(0), f64(0)
                for k in range(int(N) + 1):
                    t = t0 + f64(k) * dt
                    c, fr, ok, _ = sample(o, d, t)
                    if not ok:
                        prev = False
                        invalid[y, x] += 1
                        continue
                    v = lerp3(c, fr) - iso
                    if prev and v_prev >= 0 and v < 0:
                        a_t, b_t, fa, fb = t_prev, t, v_prev, v
                        near_end[y, x], near_value[y, x] = a_t, fa
                        for _ in range(int(refine)):
                            tm = 0.5 * (a_t + b_t)
                            c, fr, _, _ = sample(o, d, tm)
                            vm = lerp3(c, fr) - iso
                            if vm < 0:
                                b_t, fb = tm, vm
                            else:
                                a_t, fa = tm, vm
                        ts = a_t + (fa / (fa - fb)) * (b_t - a_t)
                        c, fr, _, corners = sample(o, d, ts)
                        u = [1.0 - fr[a] for a in range(3)]
                        gx = u[1] * u[2] * (c[1] - c[0]) + fr[1] * u[2] * (c[3] - c[2]) + u[1] * fr[2] * (c[5] - c[4]) + fr[1] * fr[2] * (c[7] - c[6])
                        gy = u[0] * u[2] * (c[2] - c[0]) + fr[0] * u[2] * (c[3] - c[1]) + u[0] * fr[2] * (c[6] - c[4]) + fr[0] * fr[2] * (c[7] - c[5])
                        gz = u[0] * u[1] * (c[4] - c[0]) + fr[0] * u[1] * (c[5] - c[1]) + u[0] * fr[1] * (c[6] - c[2]) + fr[0] * fr[1] * (c[7] - c[3])
                        s = np.sqrt(gx * gx + gy * gy + gz * gz)
                        depth[y, x], acc[y, x] = np.float32(ts), 1.0
                        if s > 0:
                            normals[y, x] = (np.float32(gx / s), np.float32(gy / s), np.float32(gz / s))
                        if col is not None:
                            for ch in range(3):
                                view_rgb[y, x, ch] = np.float32(lerp3([f64(col[idx + (ch,)]) for idx in corners], fr))
                        break
                    prev, v_prev, t_prev = True, v, t
    return depth, normals, view_rgb, acc


def ray_dirs(pixtocam, camtoworld, width, height):
    """(directions [H,W,3], origin [3]) in float64: the header's camera lines, for the analytic checks"""
    K, M = np.asarray(pixtocam, np.float64), np.asarray(camtoworld, np.float64)
    x, y = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5, indexing="xy")
    cam = np.stack([K[0, 0] * x + K[0, 1] * y + K[0, 2], -(K[1, 0] * x + K[1, 1] * y + K[1, 2]), -np.ones_like(x)], -1)
    return cam @ M[:, :3].T, M[:, 3]


# ------------------------------------------------------------------------------------------------------------ fixtures
PLANE = dict(dims=(17, 13, 9), h=1 / 8, origin=(0.25, -0.5, 0.125), normal=(2.0, 1.0, 2.0), offset=3.0, size=(13, 11), focal=14.0,
             eye=(2.6, 1.4, 2.3), target=(1.1, 0.2, 0.55))


def plane_volume():
    """f = (2x + y + 2z - 3) / 4 on the dyadic PLANE grid: exact in float32, and its trilinear interpolant is the field"""
    nx, ny, nz = PLANE["dims"]
    o, h = PLANE["origin"], PLANE["h"]
    X, Y, Z = (o[a] + np.arange(n) * h for a, n in enumerate((nx, ny, nz)))
    f = ((2 * X[None, None, :] + Y[None, :, None] + 2 * Z[:, None, None]) - PLANE["offset"]) / 4
    assert (f.astype(np.float32) == f).all()
    return PLANE["dims"], o, h, f.astype(np.float32), np.ones(f.shape, np.float32), None


def axis_view(width, height, eye, focal=8.0):
    """(pixtocam, camtoworld) of a camera at `eye` looking along -z with the world's axes, no skew, an odd image: the centre
    pixel's direction is exactly (0, 0, -1) and the centre column's / row's x / y component exactly 0"""
    assert width % 2 == 1 and height % 2 == 1
    p2c = np.array([[1 / focal, 0, -(width / 2) / focal], [0, 1 / focal, -(height / 2) / focal], [0, 0, 1]], np.float32)
    c2w = np.concatenate([np.eye(3), np.asarray(eye, np.float64)[:, None]], 1).astype(np.float32)
    return p2c, c2w


def _box(dims, origin, h):
    lo = np.asarray(origin, np.float64)
    return lo, lo + (np.asarray(dims) - 1) * np.float64(np.float32(h))


def random_case(dims, size, seed=0):
    """random_volume seen obliquely from outside: brackets and invalid samples interleave"""
    tsdf, weight, rgb = TC.random_volume(dims, seed=seed)
    origin, h = (0.1, -0.2, 0.3), 0.125
    lo, hi = _box(dims, origin, h)
    ext = (hi - lo).max()
    c2w = TC.look_at((lo + hi) / 2 + np.array([1.1, 0.8, 0.9]) * ext, (lo + hi) / 2)
    return dict(dims=dims, origin=origin, h=h, tsdf=tsdf, weight=weight, rgb=rgb, pixtocam=TC.pixtocam(*size, 1.1 * size[0]),
                camtoworld=c2w, size=size)


def fused_case(view):
    """the fused 33 x 17 x 9 scene seen by one of its own cameras: 0 oblique, 1 standing inside the grid, 2 narrow (part of
    the image misses the box)"""
    S, (tsdf, weight, rgb) = TC.fused_volume()
    v = S["views"][view]
    return dict(dims=S["dims"], origin=S["origin"], h=S["h"], tsdf=tsdf, weight=weight, rgb=rgb, pixtocam=v["pixtocam"],
                camtoworld=v["camtoworld"], size=(40, 24))


def sheet_case(dims, size, towards=(0.35, 0.8, 0.9), distance=3.0, zoom=1.0):
    """a gently wavy sheet through the centre of a grid of `dims`, facing a camera that stands `distance` box lengths from
    the centre in the direction `towards` and sees the whole box (at `zoom` 1; a thin box needs more); one corner voxel is
    unobserved where the grid has more than one cell: most rays that enter the box hit"""
    nx, ny, nz = dims
    origin, h = (0.1, -0.2, 0.3), 0.125
    lo, hi = _box(dims, origin, h)
    centre, ext = (lo + hi) / 2, (hi - lo).max()
    e = np.asarray(towards, np.float64) / np.linalg.norm(towards)
    eye = centre + e * distance * ext
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    P = lo + np.stack([i, j, k], -1) * h
    tsdf = ((P - centre) @ e + 0.02 * np.sin(7 * P[..., 0] + 3 * P[..., 1] + 5 * P[..., 2])).astype(np.float32)
    weight = np.ones((nz, ny, nx), np.float32)
    if nx > 2:
        weight[0, 0, nx // 2] = 0
    rgb = np.random.default_rng([13, nx, ny, nz]).uniform(0, 1, (nz, ny, nx, 3)).astype(np.float32)
    return dict(dims=dims, origin=origin, h=h, tsdf=tsdf, weight=weight, rgb=rgb, pixtocam=TC.pixtocam(*size, 0.7 * size[0] * distance * zoom),
                camtoworld=TC.look_at(eye, centre), size=size)


def sphere_case(size=(40, 24), focal=30.0, eye=(2.4, 1.9, 2.2), **kw):
    dims, origin, h, tsdf, weight, rgb = TC.sphere_volume(**kw)
    return dict(dims=dims, origin=origin, h=h, tsdf=tsdf, weight=weight, rgb=rgb, pixtocam=TC.pixtocam(*size, focal),
                camtoworld=TC.look_at(eye, TC.SPHERE["centre"]), size=size)


def zero_component_case(inside):
    """the sphere seen along -z by an axis-aligned camera whose centre column and row have direction components exactly 0;
    `inside`: the camera's x, y lie inside the box's slab (the centre ray goes down through the sphere), else outside it in
    x (the rays of the centre column have d[0] == 0 and o[0] outside [lo, hi]: they miss by the d == 0 branch)"""
    dims, origin, h, tsdf, weight, rgb = TC.sphere_volume()
    eye = (0.70, 0.66, 2.5) if inside else (-0.5, 0.66, 2.5)
    p2c, c2w = axis_view(9, 7, eye, focal=8.0 if inside else 4.0)
    return dict(dims=dims, origin=origin, h=h, tsdf=tsdf, weight=weight, rgb=rgb, pixtocam=p2c, camtoworld=c2w, size=(9, 7))


CASES = {
    "cell-5x4": lambda: sheet_case((2, 2, 2), (5, 4)),                       # the single cell: the index clamp does all the work
    "9x6x5-13x11": lambda: sheet_case((9, 6, 5), (13, 11)),                  # image sides off the 8 x 8 tile
    "65x3x2-40x24": lambda: sheet_case((65, 3, 2), (40, 24), towards=(0.0, 0.6, 0.8), distance=0.5, zoom=4.0),      # nx one over a wave
    "random-9x7": lambda: random_case((9, 6, 5), (9, 7), seed=1),
    "random-65x3": lambda: random_case((7, 6, 5), (65, 3), seed=2),
    "fused-view0": lambda: fused_case(0),                                    # the round trip: what fusion saw, cast back
    "inside-the-grid": lambda: fused_case(1),
    "narrow": lambda: fused_case(2),
    "zero-inside": lambda: zero_component_case(True),
    "zero-outside": lambda: zero_component_case(False),
    "quantum": lambda: sphere_case(quantum=0.25),
    "sphere": sphere_case,
    "unobserved": lambda: sphere_case(eye=(2.4, 1.9, 0.6), unobserved=True),     # some rays cross the unobserved block, then hit
}
SWEEP = [(colour, refine, step) for colour in (True, False) for refine in (0, 4) for step in (0.5, 1.75)]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def truth(name, colour=True, refine=4, step=0.5, **kw):
    """the mirror's (depth, normals, rgb | None, acc) of a case: computed once, left unchanged"""
    c = case(name)
    out = raycast_mirror(c["dims"], c["origin"], c["h"], c["tsdf"], c["weight"], c["rgb"] if colour else None, c["pixtocam"], c["camtoworld"],
                         *c["size"], refine=refine, step=step, **kw)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out

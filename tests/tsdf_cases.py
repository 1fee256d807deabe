"""Fixtures and pure-numpy mirrors of include/refnerf_tsdf.h for tests/test_tsdf.py and tests/test_guard_bands_tsdf.py.

The reference has no TSDF: there are no golden captures, every input comes from a seed or a formula.  `integrate_mirror` is
the header's per-voxel lines in float64 numpy, in the header's order, rounded once to float32; `extract_mirror` is a plain
loop over cells, tetrahedra, cases and edges written from the header's definition (its triangle rule is applied by
permutation parity, not read from a table).  Both are exact restatements: the kernels must equal them bit for bit."""
import functools
import itertools

import numpy as np

# ------------------------------------------------------------------------------------------------------------ volumes
SPHERE = dict(dims=(12, 11, 10), h=1 / 8, centre=(0.70, 0.66, 0.61), r=0.45)


def sphere_volume(quantum=None, unobserved=False):
    """(dims, origin, h, tsdf, weight, rgb): the signed distance to SPHERE on its 12 x 11 x 10 grid (unclamped), weight 1.
    quantum: tsdf rounded to its multiples (corners exactly on the iso value).  unobserved: a block of voxels has weight 0."""
    nx, ny, nz = SPHERE["dims"]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    P = np.stack([i, j, k], -1) * SPHERE["h"]
    d = np.linalg.norm(P - np.asarray(SPHERE["centre"]), axis=-1) - SPHERE["r"]
    if quantum:
        d = np.round(d / quantum) * quantum
    weight = np.ones((nz, ny, nx), np.float32)
    if unobserved:
        weight[4:7, 3:8, 6:] = 0
    rgb = np.random.default_rng(5).uniform(0, 1, (nz, ny, nx, 3)).astype(np.float32)
    return SPHERE["dims"], (0.0, 0.0, 0.0), SPHERE["h"], d.astype(np.float32), weight, rgb


def random_volume(dims, seed=0):
    """a volume with a surface in every neighbourhood: uniform tsdf in [-1, 1], a few unobserved voxels"""
    rng = np.random.default_rng([11, seed])
    nx, ny, nz = dims
    tsdf = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    weight = np.where(rng.uniform(size=(nz, ny, nx)) < 0.1, 0.0, 2.0).astype(np.float32)
    weight[:2, :2, :2] = 2.0                          # at least the first cell contributes (the 2 x 2 x 2 grid has no other)
    rgb = rng.uniform(0, 1, (nz, ny, nx, 3)).astype(np.float32)
    return tsdf, weight, rgb


# -------------------------------------------------------------------------------------------------------------- views
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """float32 [3,4] camera-to-world of an OpenGL camera (x right, y up, looking along -z)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), eye[:, None]], 1).astype(np.float32)


def pixtocam(width, height, focal, skew=1e-3):
    """float32 inverse intrinsics with the third row (0, 0, 1) and a small skew"""
    k = np.array([[focal, skew * focal, width / 2], [0, focal, height / 2], [0, 0, 1]], np.float64)
    p = np.linalg.inv(k).astype(np.float32)
    p[2] = (0, 0, 1)
    return p


def _render_depth(p2c, c2w, width, height, centre, radius, plane_point):
    """z-depth [H,W] of the nearest of a sphere and a plane through plane_point facing +z (float32; inf where neither is hit)"""
    x, y = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5, indexing="xy")
    cam = np.stack([x, y, np.ones_like(x)], -1) @ p2c.astype(np.float64).T
    d = (cam * np.array([1.0, -1.0, -1.0])) @ c2w[:, :3].astype(np.float64).T
    o = c2w[:, 3].astype(np.float64)
    oc = o - np.asarray(centre)
    a, b, c = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - radius ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        t_sphere = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), np.inf)
        t_plane = (plane_point[2] - o[2]) / d[..., 2]
    t_sphere = np.where(t_sphere > 0, t_sphere, np.inf)
    t_plane = np.where(t_plane > 0, t_plane, np.inf)
    return np.minimum(t_sphere, t_plane).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(dims, size):
    """A grid of `dims` voxels spanning about one unit and three oblique views of `size` = (W, H) pixels of a sphere in front
    of a plane, with holes.  View 1 stands inside the grid (part of it is behind the camera), view 2 is narrow (part of the
    grid is off-image).  Returns dict(dims, origin, h, trunc, views=[dict(pixtocam, camtoworld, depth, acc, rgb)])."""
    nx, ny, nz = dims
    W, H = size
    h = np.float32(1.0 / (max(dims) - 1))
    origin = np.array([-0.5, -0.31, -0.27], np.float32)
    extent = (np.asarray(dims) - 1) * np.float64(h)
    centre = origin.astype(np.float64) + extent / 2
    radius = 0.3 * extent.min() + 0.05
    rng = np.random.default_rng([3, nx, ny, nz, W, H])
    views = []
    for n, (eye, focal) in enumerate((((1.3, 0.9, 0.8), 0.9 * W), ((0.1, 0.05, 0.3), 0.5 * W), ((-0.9, 1.1, 0.5), 2.5 * W))):
        c2w = look_at(centre + np.asarray(eye) * max(extent.max(), 0.5), centre + (0.02 * n, -0.01, 0.0))
        p2c = pixtocam(W, H, focal)
        depth = _render_depth(p2c, c2w, W, H, centre, radius, origin.astype(np.float64) + 0.1 * extent)
        flat = depth.reshape(-1)
        holes = rng.permutation(flat.size)[:max(flat.size // 6, 5)]
        flat[holes] = np.resize(np.array([np.inf, np.nan, 0.0, -1.0, -np.inf], np.float32), holes.size)
        acc = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
        views.append(dict(pixtocam=p2c, camtoworld=c2w, depth=depth, acc=acc, rgb=rng.uniform(0, 1, (H, W, 3)).astype(np.float32)))
    return dict(dims=dims, origin=tuple(float(o) for o in origin), h=float(h), trunc=float(np.float32(3.5 * h)), views=views)


SENTINEL = dict(tsdf=-3.0, weight=0.0, rgb=9.0)        # what an untouched voxel of the integrate tests holds


def sentinel_state(dims):
    nx, ny, nz = dims
    return (np.full((nz, ny, nx), SENTINEL["tsdf"], np.float32), np.full((nz, ny, nx), SENTINEL["weight"], np.float32),
            np.full((nz, ny, nx, 3), SENTINEL["rgb"], np.float32))


# ------------------------------------------------------------------------------------------------------------ mirrors
def integrate_mirror(dims, origin, h, trunc, tsdf, weight, rgb, pixtocam, camtoworld, depth, acc=None, acc_min=0.0, view_rgb=None,
                     view_weight=1.0, z_min=0.0):
    """refnerf_tsdf_integrate in float64 numpy: returns (tsdf, weight, rgb | None, updated mask) as new arrays."""
    f64 = np.float64
    nx, ny, nz = dims
    h, trunc, w = f64(np.float32(h)), f64(np.float32(trunc)), f64(np.float32(view_weight))
    o = [f64(np.float32(v)) for v in origin]
    k, j, i = np.meshgrid(np.arange(nz, dtype=f64), np.arange(ny, dtype=f64), np.arange(nx, dtype=f64), indexing="ij")
    m = np.asarray(camtoworld, np.float32).astype(f64)
    dx, dy, dz = (o[0] + i * h) - m[0, 3], (o[1] + j * h) - m[1, 3], (o[2] + k * h) - m[2, 3]
    q0 = m[0, 0] * dx + m[1, 0] * dy + m[2, 0] * dz
    q1 = -(m[0, 1] * dx + m[1, 1] * dy + m[2, 1] * dz)
    z = -(m[0, 2] * dx + m[1, 2] * dy + m[2, 2] * dz)
    (a, b, c), (d, e, f) = np.asarray(pixtocam, np.float32).astype(f64)[:2]
    det = a * e - b * d
    with np.errstate(all="ignore"):
        u = ((e / det) * q0 + (-b / det) * q1 + ((b * f - c * e) / det) * z) / z
        v = ((-d / det) * q0 + (a / det) * q1 + ((c * d - a * f) / det) * z) / z
        H, W = depth.shape
        fx, fy = np.floor(u), np.floor(v)
        ok = (z > f64(np.float32(z_min))) & (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
        pix = np.where(ok, fy * W + fx, 0).astype(np.int64)
        D = np.asarray(depth, np.float32).reshape(-1)[pix]
        ok &= np.isfinite(D) & (D > 0)
        if acc is not None:
            ok &= ~(np.asarray(acc, np.float32).reshape(-1)[pix] < np.float32(acc_min))
        sdf = D.astype(f64) - z
        ok &= ~(sdf < -trunc)
        obs = np.minimum(1.0, sdf / trunc)
        Wo = weight.astype(f64)
        Wn = Wo + w
        new_tsdf = np.where(ok, ((Wo * tsdf.astype(f64) + w * obs) / Wn).astype(np.float32), tsdf)
        new_rgb = None
        if rgb is not None:
            seen = np.asarray(view_rgb, np.float32).reshape(-1, 3)[pix].astype(f64)
            new_rgb = np.where(ok[..., None], ((Wo[..., None] * rgb.astype(f64) + w * seen) / Wn[..., None]).astype(np.float32), rgb)
        new_weight = np.where(ok, Wn.astype(np.float32), weight)
    return new_tsdf, new_weight, new_rgb, ok


def _odd(perm):
    return sum(x > y for x, y in itertools.combinations(perm, 2)) % 2


def _tet_triangles(inside):
    """inside: 4 booleans of the corners v0..v3 of a tetrahedron of even parity -> triangles as triples of corner pairs"""
    ins = [n for n in range(4) if inside[n]]
    out = [n for n in range(4) if not inside[n]]
    if not ins or not out:
        return []
    if len(ins) == 1 or len(out) == 1:
        i = ins[0] if len(ins) == 1 else out[0]
        j, k, l = [n for n in range(4) if n != i]
        if _odd((i, j, k, l)):
            k, l = l, k
        return [((i, j), (i, k), (i, l))] if len(ins) == 1 else [((i, j), (i, l), (i, k))]
    (i, j), (k, l) = ins, out
    if _odd((i, j, k, l)):
        k, l = l, k
    return [((i, k), (i, l), (j, l)), ((i, k), (j, l), (j, k))]


def extract_mirror(dims, origin, h, tsdf, weight, rgb=None, iso=0.0, min_weight=1.0):
    """refnerf_tsdf_mesh_count + _emit as plain loops: (vertices [V,3] f32, triangles [T,3] i32, colours [V,3] f32 | None)."""
    nx, ny, nz = dims
    iso32, mw = np.float32(iso), np.float32(min_weight)
    t = np.asarray(tsdf, np.float32).reshape(-1)
    wgt = np.asarray(weight, np.float32).reshape(-1)

    def index(i, j, k):
        return (k * ny + j) * nx + i
    offs = [((m & 1), (m >> 1) & 1, (m >> 2) & 1) for m in range(8)]
    tris = []              # triples of edge keys (voxel index, slot), in (cell, tetrahedron, triangle) order
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                corners = [index(i + a, j + b, k + c) for a, b, c in offs]
                if not all(wgt[p] >= mw for p in corners):
                    continue
                for order in itertools.permutations(range(3)):
                    v = [0, 1 << order[0], (1 << order[0]) | (1 << order[1]), 7]
                    for tri in _tet_triangles([bool(t[corners[c]] < iso32) for c in v]):
                        if _odd(order):
                            tri = (tri[0], tri[2], tri[1])
                        tris.append(tuple((corners[v[min(r, s)]], (v[max(r, s)] ^ v[min(r, s)]) - 1) for r, s in tri))
    edges = sorted({e for tri in tris for e in tri})
    number = {e: n for n, e in enumerate(edges)}
    triangles = np.array([[number[e] for e in tri] for tri in tris], np.int32).reshape(-1, 3)
    vertices = np.zeros((len(edges), 3), np.float32)
    colors = None if rgb is None else np.zeros((len(edges), 3), np.float32)
    c = None if rgb is None else np.asarray(rgb, np.float32).reshape(-1, 3).astype(np.float64)
    hh = np.float64(np.float32(h))
    for n, (p, slot) in enumerate(edges):
        m = slot + 1
        ijk = (p % nx, p // nx % ny, p // (nx * ny))
        q = index(ijk[0] + (m & 1), ijk[1] + ((m >> 1) & 1), ijk[2] + ((m >> 2) & 1))
        A, B = np.float64(t[p]) - np.float64(iso32), np.float64(t[q]) - np.float64(iso32)
        s = A / (A - B)
        for axis in range(3):
            vertices[n, axis] = np.float32(np.float64(np.float32(origin[axis])) + (np.float64(ijk[axis]) + (s if m >> axis & 1 else 0.0)) * hh)
        if c is not None:
            colors[n] = (c[p] + s * (c[q] - c[p])).astype(np.float32)
    return vertices, triangles, colors


# ----------------------------------------------------------------------------------------------------------- topology
def topology(vertices, triangles):
    """dict(V, E, F, manifold: every directed edge once and its reverse once, boundary: directed edges without a reverse)"""
    from collections import Counter
    directed = Counter()
    for a, b, c in np.asarray(triangles).tolist():
        for e in ((a, b), (b, c), (c, a)):
            directed[e] += 1
    boundary = [e for e in directed if (e[1], e[0]) not in directed]
    return dict(V=len(vertices), E=len({tuple(sorted(e)) for e in directed}), F=len(triangles),
                once=all(n == 1 for n in directed.values()), boundary=boundary, used=len({v for e in directed for v in e}))


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(triangles)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6)


@functools.lru_cache(maxsize=None)
def fused_volume():
    """the 33 x 17 x 9 scene fused by the mirror from an empty volume (tsdf 1, weight 0, colour 0), three views of weight 1"""
    S = scene((33, 17, 9), (40, 24))
    nx, ny, nz = S["dims"]
    state = (np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx, 3), np.float32))
    for view in S["views"]:
        state = integrate_mirror(S["dims"], S["origin"], S["h"], S["trunc"], *state, view["pixtocam"], view["camtoworld"], view["depth"],
                                 view["acc"], 0.5, view["rgb"])[:3]
    return S, state

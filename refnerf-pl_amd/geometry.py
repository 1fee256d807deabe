"""Geometry export: fuse rendered depth maps into a truncated signed distance function (TSDF) on a voxel grid and extract
its iso-surface as a triangle mesh.  Not part of the reference, which stops at images; the definition of both stages is
include/refnerf_tsdf.h, and this module is its interface:

    volume = geometry.TSDFVolume(aabb_min, aabb_max, resolution=256)
    geometry.fuse_views(lambda rays: model(rays, 1., True), dataset, config, volume)
    vertices, faces, colors = volume.extract_mesh()
    geometry.save_ply('mesh.ply', vertices, faces, colors)
    view = volume.raycast_view(dataset, 0)                  # depth, normals, rgb, acc of the surface seen by a camera
    scores = geometry.surface_metrics(volume, dataset)      # normals_mae against the dataset's normals, coverage

On a HIP device both stages are the kernels of csrc/refnerf_tsdf.h (no fallback: a missing library raises).  With
device='cpu' the volume runs the float64 restatement below -- the header's lines in its order, rounded once to float32 --
which the kernels reproduce bit for bit; `integrate_aten` is the same restatement on tensors of any device.  The ray caster
that renders the volume back into images is include/refnerf_raycast.h: csrc/refnerf_raycast.h on the device, `raycast_host`
here."""
import itertools

import numpy as np
import torch

from . import _hip

EDGE_SLOTS = 7                                    # per voxel: the edges to p + m, m = 1..7 (bit 0 = x, 1 = y, 2 = z), slot m - 1
TET_ORDERS = tuple(itertools.permutations(range(3)))        # the six axis orders of the Kuhn decomposition, lexicographic


def _odd(perm):
    return sum(a > b for a, b in itertools.combinations(perm, 2)) % 2


def tet_triangles(case):
    """The triangles of a tetrahedron of even parity whose corners n with bit n of `case` set are inside: a list of
    triples of edges (r, s), r < s corner numbers -- the rule of include/refnerf_tsdf.h."""
    ins = [n for n in range(4) if case >> n & 1]
    out = [n for n in range(4) if not case >> n & 1]

    def e(r, s):
        return (min(r, s), max(r, s))
    if not ins or not out:
        return []
    if len(ins) == 1 or len(out) == 1:
        i = (ins if len(ins) == 1 else out)[0]
        j, k, l = (n for n in range(4) if n != i)
        if _odd((i, j, k, l)):
            k, l = l, k
        return [[e(i, j), e(i, k), e(i, l)]] if len(ins) == 1 else [[e(i, j), e(i, l), e(i, k)]]
    (i, j), (k, l) = ins, out
    if _odd((i, j, k, l)):
        k, l = l, k
    return [[e(i, k), e(i, l), e(j, l)], [e(i, k), e(j, l), e(j, k)]]


def _grid_points(dims, origin, voxel_size):
    """float64 [nz, ny, nx] coordinate arrays of the voxel centres: origin + index * voxel_size"""
    nx, ny, nz = dims
    o = [torch.tensor(float(np.float32(v)), dtype=torch.float64) for v in origin]
    h = float(np.float32(voxel_size))
    ax = [o[a] + torch.arange(n, dtype=torch.float64) * h for a, n in enumerate((nx, ny, nz))]
    return ax[0].reshape(1, 1, nx), ax[1].reshape(1, ny, 1), ax[2].reshape(nz, 1, 1)


def integrate_aten(dims, origin, voxel_size, trunc, tsdf, weight, rgb, pixtocam, camtoworld, depth, acc=None, acc_min=0.0,
                   view_rgb=None, view_weight=1.0, z_min=0.0):
    """The update of refnerf_tsdf_integrate as ATen operations in float64, in the header's order (projection, gather,
    masked running average): tsdf / weight [nz,ny,nx] and rgb [nz,ny,nx,3] (or None) are updated in place.  float32
    tensors on one device; pixtocam [3,3], camtoworld [3,4]."""
    dev = tsdf.device
    f64 = torch.float64
    X, Y, Z = (t.to(dev) for t in _grid_points(dims, origin, voxel_size))
    m = camtoworld.to(f64)
    k = pixtocam.to(f64)
    dx, dy, dz = X - m[0, 3], Y - m[1, 3], Z - m[2, 3]
    q0 = m[0, 0] * dx + m[1, 0] * dy + m[2, 0] * dz
    q1 = -(m[0, 1] * dx + m[1, 1] * dy + m[2, 1] * dz)
    z = -(m[0, 2] * dx + m[1, 2] * dy + m[2, 2] * dz)
    a, b, c, d, e, f = k[0, 0], k[0, 1], k[0, 2], k[1, 0], k[1, 1], k[1, 2]
    det = a * e - b * d
    u = ((e / det) * q0 + (-b / det) * q1 + ((b * f - c * e) / det) * z) / z
    v = ((-d / det) * q0 + (a / det) * q1 + ((c * d - a * f) / det) * z) / z
    H, W = depth.shape
    fx, fy = torch.floor(u), torch.floor(v)
    ok = (z > float(np.float32(z_min))) & (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    pix = torch.where(ok, fy * W + fx, torch.zeros_like(fx)).long()
    D = depth.reshape(-1)[pix]
    ok &= (D > 0) & (D < float('inf'))
    if acc is not None:
        ok &= ~(acc.reshape(-1)[pix] < float(np.float32(acc_min)))
    t = float(np.float32(trunc))
    sdf = D.to(f64) - z
    ok &= ~(sdf < -t)
    obs = torch.clamp(sdf / t, max=1.0)
    w = float(np.float32(view_weight))
    Wo = weight.to(f64)
    Wn = Wo + w
    tsdf.copy_(torch.where(ok, ((Wo * tsdf.to(f64) + w * obs) / Wn).to(torch.float32), tsdf))
    if rgb is not None:
        seen = view_rgb.reshape(-1, 3)[pix].to(f64)
        rgb.copy_(torch.where(ok[..., None], ((Wo[..., None] * rgb.to(f64) + w * seen) / Wn[..., None]).to(torch.float32), rgb))
    weight.copy_(torch.where(ok, Wn.to(torch.float32), weight))


def extract_mesh_host(dims, origin, voxel_size, tsdf, weight, rgb, iso=0.0, min_weight=1.0):
    """Marching tetrahedra of include/refnerf_tsdf.h on numpy arrays tsdf / weight [nz,ny,nx], rgb [nz,ny,nx,3] or None:
    (vertices [V,3] float32, triangles [T,3] int32, colours [V,3] float32 or None), in the header's order, bit for bit."""
    nx, ny, nz = dims
    tsdf = np.ascontiguousarray(tsdf, np.float32)
    inside = tsdf < np.float32(iso)
    seen = np.asarray(weight, np.float32) >= np.float32(min_weight)
    code = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for m in range(8):
        sl = tuple(slice(s, n - 1 + s) for s, n in (((m >> 2) & 1, nz), ((m >> 1) & 1, ny), (m & 1, nx)))
        code |= inside[sl].astype(np.int32) << m
        ok &= seen[sl]
    cells = np.argwhere(ok & (code != 0) & (code != 255))             # C order: ascending cell index
    step = [(m & 1) + ((m >> 1) & 1) * nx + ((m >> 2) & 1) * nx * ny for m in range(8)]
    table = [tet_triangles(c) for c in range(16)]
    keys = []                                                         # 7 * voxel + slot of every triangle corner
    for k, j, i in cells:
        p, cc = (int(k) * ny + int(j)) * nx + int(i), int(code[k, j, i])
        for order in TET_ORDERS:
            corner = (0, 1 << order[0], (1 << order[0]) | (1 << order[1]), 7)
            case = sum(((cc >> corner[n]) & 1) << n for n in range(4))
            for tri in table[case]:
                if _odd(order):
                    tri = [tri[0], tri[2], tri[1]]
                keys.extend(EDGE_SLOTS * (p + step[corner[r]]) + (corner[s] ^ corner[r]) - 1 for r, s in tri)
    keys = np.asarray(keys, np.int64)
    edges = np.unique(keys)                                           # sorted: by (voxel index, slot)
    triangles = np.searchsorted(edges, keys).astype(np.int32).reshape(-1, 3)
    p, m = edges // EDGE_SLOTS, edges % EDGE_SLOTS + 1
    q = p + np.asarray(step, np.int64)[m]
    flat = tsdf.reshape(-1).astype(np.float64)
    A, B = flat[p] - float(np.float32(iso)), flat[q] - float(np.float32(iso))
    t = A / (A - B)
    index = (p % nx, p // nx % ny, p // (nx * ny))
    h = float(np.float32(voxel_size))
    vertices = np.stack([float(np.float32(origin[a])) + (index[a].astype(np.float64) + np.where(m >> a & 1, t, 0.0)) * h
                         for a in range(3)], -1).astype(np.float32).reshape(-1, 3)
    colors = None
    if rgb is not None:
        c = np.asarray(rgb, np.float32).reshape(-1, 3).astype(np.float64)
        colors = (c[p] + t[:, None] * (c[q] - c[p])).astype(np.float32).reshape(-1, 3)
    return vertices, triangles, colors


def raycast_host(dims, origin, voxel_size, tsdf, weight, rgb, pixtocam, camtoworld, width, height, iso=0.0, min_weight=1.0, step=0.5,
                 refine=4, t_near=0.0, t_far=float('inf')):
    """refnerf_tsdf_raycast of include/refnerf_raycast.h on numpy arrays tsdf / weight [nz,ny,nx], rgb [nz,ny,nx,3] or None,
    pixtocam [3,3], camtoworld [3,4]: (depth [H,W], normals [H,W,3], rgb [H,W,3] or None, acc [H,W]) float32, the header's
    lines in its order in float64, vectorised over the pixels with a loop over the sample index k, bit for bit."""
    f64 = np.float64
    nx, ny, nz = (int(n) for n in dims)
    n = (nx, ny, nz)
    W, H = int(width), int(height)
    flat = np.ascontiguousarray(tsdf, np.float32).reshape(-1)
    seen = np.ascontiguousarray(weight, np.float32).reshape(-1) >= np.float32(min_weight)
    colour = None if rgb is None else np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    org = [f64(np.float32(v)) for v in origin]
    h, iso, step = f64(np.float32(voxel_size)), f64(np.float32(iso)), f64(np.float32(step))
    K, M = np.asarray(pixtocam, np.float32).astype(f64), np.asarray(camtoworld, np.float32).astype(f64)
    sy, sz = nx, nx * ny
    corner = np.array([(m & 1) + (m >> 1 & 1) * sy + (m >> 2 & 1) * sz for m in range(8)], np.int64)

    def cell(o, d, t):
        """SAMPLE: (corner values [8,n], fr [3,n], valid [n], cell index [n]) at o + t d"""
        i, fr = [], []
        for a in range(3):
            g = ((o[a] + t * d[a]) - org[a]) / h
            f = np.floor(g)
            ia = np.where(f > 0, np.where(f < n[a] - 2, f, f64(n[a] - 2)), 0.0)       # a NaN gives 0
            i.append(ia.astype(np.int64))
            fr.append(g - ia)
        p = (i[2] * sz + i[1] * sy) + i[0]
        q = p[None, :] + corner[:, None]
        return flat[q].astype(f64), fr, seen[q].all(0), p

    def lerp3(c, fr):
        x = [c[2 * q] + fr[0] * (c[2 * q + 1] - c[2 * q]) for q in range(4)]
        y = [x[2 * r] + fr[1] * (x[2 * r + 1] - x[2 * r]) for r in range(2)]
        return y[0] + fr[2] * (y[1] - y[0])

    with np.errstate(all='ignore'):
        px, py = np.meshgrid(np.arange(W, dtype=f64) + .5, np.arange(H, dtype=f64) + .5, indexing='xy')
        px, py = px.reshape(-1), py.reshape(-1)
        cx = K[0, 0] * px + K[0, 1] * py + K[0, 2]
        cy = -(K[1, 0] * px + K[1, 1] * py + K[1, 2])
        cz = f64(-1.0)
        d = [M[a, 0] * cx + M[a, 1] * cy + M[a, 2] * cz for a in range(3)]
        o = [M[a, 3] for a in range(3)]
        t0, t1 = np.full(px.shape, f64(np.float32(t_near))), np.full(px.shape, f64(np.float32(t_far)))
        miss = np.zeros(px.shape, bool)
        for a in range(3):
            lo, hi = org[a], org[a] + f64(n[a] - 1) * h
            zero = d[a] == 0
            if not (lo <= o[a] and o[a] <= hi):
                miss |= zero
            ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
            lo_t, hi_t = np.where(ta < tb, ta, tb), np.where(ta > tb, ta, tb)
            t0 = np.where(zero, t0, np.where(t0 > lo_t, t0, lo_t))
            t1 = np.where(zero, t1, np.where(t1 < hi_t, t1, hi_t))
        miss |= ~(t1 >= t0)
        dt = step * h / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        N = np.floor((t1 - t0) / dt)
        miss |= ~(N <= f64(nx + ny + nz) / step)

        # MARCH over the rays still looking for their bracket; `ray` indexes the pixels
        ray = np.flatnonzero(~miss)
        prev, v_prev, t_prev = np.zeros(ray.size, bool), np.zeros(ray.size), np.zeros(ray.size)
        hits, brackets = [], []
        k = 0
        while ray.size:
            go = N[ray] >= k
            ray, prev, v_prev, t_prev = ray[go], prev[go], v_prev[go], t_prev[go]
            if not ray.size:
                break
            t = t0[ray] + f64(k) * dt[ray]
            c, fr, ok, _ = cell(o, [d[a][ray] for a in range(3)], t)
            v = lerp3(c, fr) - iso
            hit = ok & prev & (v_prev >= 0) & (v < 0)
            if hit.any():
                hits.append(ray[hit])
                brackets.append(np.stack([t_prev[hit], t[hit], v_prev[hit], v[hit]]))
            prev, v_prev, t_prev = ok, np.where(ok, v, v_prev), np.where(ok, t, t_prev)
            keep = ~hit
            ray, prev, v_prev, t_prev = ray[keep], prev[keep], v_prev[keep], t_prev[keep]
            k += 1

        depth, acc = np.zeros(H * W, np.float32), np.zeros(H * W, np.float32)
        normals = np.zeros((H * W, 3), np.float32)
        view_rgb = None if colour is None else np.zeros((H * W, 3), np.float32)
        if hits:
            ray = np.concatenate(hits)
            a_t, b_t, fa, fb = np.concatenate(brackets, 1)
            dr = [d[a][ray] for a in range(3)]
            for _ in range(int(refine)):                                 # REFINE
                tm = 0.5 * (a_t + b_t)
                c, fr, _, _ = cell(o, dr, tm)
                vm = lerp3(c, fr) - iso
                neg = vm < 0
                a_t, fa, b_t, fb = np.where(neg, a_t, tm), np.where(neg, fa, vm), np.where(neg, tm, b_t), np.where(neg, vm, fb)
            ts = a_t + (fa / (fa - fb)) * (b_t - a_t)                    # HIT
            c, fr, _, p = cell(o, dr, ts)
            u = [1.0 - fr[a] for a in range(3)]
            gx = u[1] * u[2] * (c[1] - c[0]) + fr[1] * u[2] * (c[3] - c[2]) + u[1] * fr[2] * (c[5] - c[4]) + fr[1] * fr[2] * (c[7] - c[6])
            gy = u[0] * u[2] * (c[2] - c[0]) + fr[0] * u[2] * (c[3] - c[1]) + u[0] * fr[2] * (c[6] - c[4]) + fr[0] * fr[2] * (c[7] - c[5])
            gz = u[0] * u[1] * (c[4] - c[0]) + fr[0] * u[1] * (c[5] - c[1]) + u[0] * fr[1] * (c[6] - c[2]) + fr[0] * fr[1] * (c[7] - c[3])
            s = np.sqrt(gx * gx + gy * gy + gz * gz)
            depth[ray], acc[ray] = ts.astype(np.float32), 1.0
            normals[ray] = np.where((s > 0)[:, None], np.stack([gx / s, gy / s, gz / s], -1), 0.0).astype(np.float32)
            if colour is not None:
                q = p[None, :] + corner[:, None]
                view_rgb[ray] = np.stack([lerp3(colour[q, ch].astype(f64), fr) for ch in range(3)], -1).astype(np.float32)
    return (depth.reshape(H, W), normals.reshape(H, W, 3), None if view_rgb is None else view_rgb.reshape(H, W, 3), acc.reshape(H, W))


def _camera_tuple(cameras):
    """(pixtocams, camtoworlds, distortion_params, pixtocam_ndc, spherical) of a PathCameras / SceneDataset or of the
    reference's camera tuple"""
    tup = getattr(cameras, 'cameras', cameras)
    if len(tup) != 4:
        raise ValueError('cameras: a dataset with `.cameras`, or the tuple (pixtocams, camtoworlds, distortion_params, pixtocam_ndc)')
    return tuple(tup) + (bool(getattr(cameras, 'spherical', False)),)


class TSDFVolume:
    """A TSDF voxel grid over the box [aabb_min, aabb_max]: voxel (0, 0, 0) is centred on aabb_min, and the grid is the
    smallest one of isotropic `voxel_size` whose centres reach aabb_max.  Give `voxel_size`, or `resolution`: the number of
    voxels along the longest side (an int) or (nx, ny, nz).  `trunc` (world units) defaults to 4 voxel sizes.  Unobserved
    voxels hold tsdf 1 (free space), weight 0 and colour 0.  `device`: a HIP device (default 'cuda'), or 'cpu' for the
    float64 restatement.  Arrays: `.tsdf`, `.weight` [nz,ny,nx], `.rgb` [nz,ny,nx,3] or None, float32 on the device."""

    def __init__(self, aabb_min, aabb_max, resolution=None, voxel_size=None, trunc=None, color=True, device=None):
        lo, hi = np.asarray(aabb_min, np.float64).reshape(3), np.asarray(aabb_max, np.float64).reshape(3)
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
            raise ValueError('TSDFVolume: aabb_max must exceed aabb_min on every axis')
        if (resolution is None) == (voxel_size is None):
            raise ValueError('TSDFVolume: give exactly one of resolution and voxel_size')
        dims = None
        if voxel_size is None and np.ndim(resolution) != 0:
            dims = tuple(int(r) for r in resolution)
            if len(dims) != 3 or min(dims) < 2:
                raise ValueError('TSDFVolume: resolution is an int or (nx, ny, nz), each at least 2')
            voxel_size = float(((hi - lo) / (np.asarray(dims) - 1)).max())
        elif voxel_size is None:
            if int(resolution) < 2:
                raise ValueError('TSDFVolume: resolution must be at least 2')
            voxel_size = float((hi - lo).max()) / (int(resolution) - 1)
        voxel_size = float(np.float32(voxel_size))
        if not (voxel_size > 0 and np.isfinite(voxel_size)):
            raise ValueError('TSDFVolume: voxel_size must be positive')
        if dims is None:
            dims = tuple(max(int(np.ceil(e / voxel_size - 1e-4)) + 1, 2) for e in hi - lo)
        trunc = 4.0 * voxel_size if trunc is None else float(trunc)
        if not trunc > 0:
            raise ValueError('TSDFVolume: trunc must be positive')
        if 7 * dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise ValueError(f'TSDFVolume: {dims[0]} x {dims[1]} x {dims[2]} voxels: 7 nx ny nz must stay below 2^31')
        self.dims, self.origin = dims, tuple(float(np.float32(v)) for v in lo)
        self.voxel_size, self.trunc = voxel_size, float(np.float32(trunc))
        self.device = torch.device('cuda' if device is None else device)
        self.grid = _hip.tsdf_grid(dims, self.origin, self.voxel_size, self.trunc)
        shape = (dims[2], dims[1], dims[0])
        self.tsdf = torch.ones(shape, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.rgb = torch.zeros(shape + (3,), dtype=torch.float32, device=self.device) if color else None

    def _f32(self, x, what, shape):
        if x is None:
            return None
        t = torch.as_tensor(np.asarray(x, np.float32) if not torch.is_tensor(x) else x).detach()
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'TSDFVolume.integrate: {what} has shape {tuple(t.shape)}, not {tuple(shape)}')
        return t

    def integrate(self, depth, pixtocam, camtoworld, rgb=None, acc=None, acc_threshold=0.5, weight=1.0, z_min=0.):
        """Fuse one view: `depth` [H,W] the distance along the (unnormalised) ray directions of a pinhole camera whose
        pixtocam has the third row (0, 0, 1) -- the z-depth; `camtoworld` [3,4] or [4,4]; `rgb` [H,W,3] (required by a colour
        volume); pixels with `acc` [H,W] below `acc_threshold`, or a depth that is not a positive finite number, are holes."""
        depth = torch.as_tensor(depth) if not torch.is_tensor(depth) else depth
        if depth.dim() == 3 and depth.shape[-1] == 1:
            depth = depth[..., 0]
        if depth.dim() != 2:
            raise ValueError(f'TSDFVolume.integrate: depth must be [H, W], got {tuple(depth.shape)}')
        H, W = depth.shape
        depth = self._f32(depth, 'depth', (H, W))
        if acc is not None and torch.is_tensor(acc) and acc.dim() == 3:
            acc = acc[..., 0]
        acc = self._f32(acc, 'acc', (H, W))
        if (self.rgb is not None) and rgb is None:
            raise ValueError('TSDFVolume.integrate: a colour volume needs rgb [H, W, 3] (or build the volume with color=False)')
        view_rgb = self._f32(rgb, 'rgb', (H, W, 3)) if self.rgb is not None else None
        c2w = torch.as_tensor(np.asarray(camtoworld, np.float32) if not torch.is_tensor(camtoworld) else camtoworld)
        if c2w.dim() != 2 or c2w.shape[0] < 3 or c2w.shape[1] != 4:
            raise ValueError(f'TSDFVolume.integrate: camtoworld must be [3, 4] or [4, 4], got {tuple(c2w.shape)}')
        c2w = self._f32(c2w[:3, :4], 'camtoworld', (3, 4))
        p2c = self._f32(pixtocam, 'pixtocam', (3, 3))
        if not (float(weight) > 0 and float(z_min) >= 0):
            raise ValueError('TSDFVolume.integrate: weight must be positive and z_min non-negative')
        if self.device.type == 'cpu':
            if not bool((p2c[2] == torch.tensor([0., 0., 1.])).all()):
                raise ValueError('TSDFVolume.integrate: the third row of pixtocam must be (0, 0, 1): the depth is a z-depth only then')
            integrate_aten(self.dims, self.origin, self.voxel_size, self.trunc, self.tsdf, self.weight, self.rgb, p2c, c2w, depth,
                           acc, acc_threshold, view_rgb, weight, z_min)
        else:
            with torch.cuda.device(self.device):
                _hip.tsdf_integrate(self.grid, self.tsdf, self.weight, self.rgb, p2c, c2w[None], 0, depth, acc, acc_threshold,
                                    view_rgb, weight, z_min)
        return self

    def integrate_rendering(self, rendering, cameras, idx, depth_key='distance_median', **kw):
        """Fuse view `idx` of `cameras` (a PathCameras / SceneDataset, or the reference's camera tuple) from what
        `models.render_image` returned for it: its `depth_key`, 'acc' and 'rgb'."""
        pixtocams, camtoworlds, distortion, ndc, spherical = _camera_tuple(cameras)
        if ndc is not None:
            raise ValueError('TSDF fusion: pixtocam_ndc is set: depths of NDC space are not metric')
        if distortion is not None:
            raise ValueError('TSDF fusion: distortion_params is set: lens-distorted views are not fused')
        if spherical:
            raise ValueError('TSDF fusion: spherical (panorama) cameras are not fused')
        p2c = np.asarray(pixtocams.cpu() if torch.is_tensor(pixtocams) else pixtocams, np.float32)
        c2w = np.asarray(camtoworlds.cpu() if torch.is_tensor(camtoworlds) else camtoworlds, np.float32)
        return self.integrate(rendering[depth_key], p2c[idx] if p2c.ndim == 3 else p2c, c2w[idx][:3, :4],
                              rgb=rendering.get('rgb') if self.rgb is not None else None, acc=rendering.get('acc'), **kw)

    def extract_mesh(self, iso=0., min_weight=1.):
        """(vertices [V,3] float32, faces [T,3] int32, colors [V,3] float32 or None) on the volume's device: the iso-surface
        through the cells all of whose corners have weight >= min_weight, normals towards free space.  One host read: the
        two counts."""
        if self.device.type == 'cpu':
            v, f, c = extract_mesh_host(self.dims, self.origin, self.voxel_size, self.tsdf.numpy(), self.weight.numpy(),
                                        None if self.rgb is None else self.rgb.numpy(), iso, min_weight)
            return torch.from_numpy(v), torch.from_numpy(f), None if c is None else torch.from_numpy(c)
        with torch.cuda.device(self.device):
            workspace, counts = _hip.tsdf_mesh_count(self.grid, self.tsdf, self.weight, iso, min_weight)
            n_vertices, n_triangles = (int(n) for n in counts.cpu())
            vertices, colors, faces = _hip.tsdf_mesh_emit(self.grid, self.tsdf, self.rgb, iso, workspace, n_vertices, n_triangles)
        return vertices, faces, colors

    def raycast(self, pixtocam, camtoworld, width, height, iso=0., min_weight=1., step=0.5, refine=4, near=0., far=float('inf')):
        """The volume seen by a pinhole camera (include/refnerf_raycast.h): a dict of `depth` [H,W] -- the distance along the
        unnormalised ray directions, what `integrate` takes --, `normals` [H,W,3] (unit, towards free space), `rgb` [H,W,3]
        (colour volumes only) and `acc` [H,W] (1 on a hit; a miss is all zero), float32 on the volume's device.  The march
        takes `step` voxels at a time through the cells whose corners all have weight >= min_weight, from `near` to `far`
        along the ray, and bisects the first crossing from free space into the surface `refine` times."""
        what = 'TSDFVolume.raycast: '
        W, H = int(width), int(height)
        if W != width or H != height or W < 1 or H < 1:
            raise ValueError(what + f'width and height must be positive integers, got {width!r} x {height!r}')
        if not (np.isfinite(iso) and np.isfinite(min_weight)):
            raise ValueError(what + 'iso and min_weight must be finite')
        if not 1 / 64 <= float(np.float32(step)) <= 64:
            raise ValueError(what + f'step must lie in [1/64, 64] voxels, got {step!r}')
        if int(refine) != refine or not 0 <= int(refine) <= 32:
            raise ValueError(what + f'refine must be an integer in [0, 32], got {refine!r}')
        if not near >= 0 or np.isnan(far):
            raise ValueError(what + 'near must be >= 0 and far must not be NaN')
        c2w = torch.as_tensor(np.asarray(camtoworld, np.float32) if not torch.is_tensor(camtoworld) else camtoworld)
        if c2w.dim() != 2 or c2w.shape[0] < 3 or c2w.shape[1] != 4:
            raise ValueError(what + f'camtoworld must be [3, 4] or [4, 4], got {tuple(c2w.shape)}')
        p2c = torch.as_tensor(np.asarray(pixtocam, np.float32) if not torch.is_tensor(pixtocam) else pixtocam)
        if tuple(p2c.shape) != (3, 3):
            raise ValueError(what + f'pixtocam must be [3, 3], got {tuple(p2c.shape)}')
        c2w = c2w[:3, :4].detach().to(device=self.device, dtype=torch.float32).contiguous()
        p2c = p2c.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if self.device.type == 'cpu':
            out = raycast_host(self.dims, self.origin, self.voxel_size, self.tsdf.numpy(), self.weight.numpy(),
                               None if self.rgb is None else self.rgb.numpy(), p2c.numpy(), c2w.numpy(), W, H, iso, min_weight, step,
                               int(refine), near, far)
            depth, normals, view_rgb, acc = (None if a is None else torch.from_numpy(a) for a in out)
        else:
            with torch.cuda.device(self.device):
                depth, normals, view_rgb, acc = _hip.tsdf_raycast(self.grid, self.tsdf, self.weight, self.rgb, p2c, c2w[None], 0, W, H, iso,
                                                                  min_weight, step, int(refine), near, far)
        out = dict(depth=depth, normals=normals, acc=acc)
        if view_rgb is not None:
            out['rgb'] = view_rgb
        return out

    def raycast_view(self, cameras, idx, width=None, height=None, **kw):
        """`raycast` of view `idx` of `cameras` (a PathCameras / SceneDataset, or the reference's camera tuple).  The image
        size is the dataset's; a bare tuple needs `width=` and `height=`."""
        pixtocams, camtoworlds, distortion, ndc, spherical = _camera_tuple(cameras)
        if ndc is not None:
            raise ValueError('TSDF ray casting: pixtocam_ndc is set: depths of NDC space are not metric')
        if distortion is not None:
            raise ValueError('TSDF ray casting: distortion_params is set: lens-distorted views are not ray cast')
        if spherical:
            raise ValueError('TSDF ray casting: spherical (panorama) cameras are not ray cast')
        width = getattr(cameras, 'width', None) if width is None else width
        height = getattr(cameras, 'height', None) if height is None else height
        if width is None or height is None:
            raise ValueError('TSDF ray casting: a camera tuple carries no image size: give width= and height=')
        # the one view is indexed where the stacks live (tensors stay on their device), `raycast` moves it to the volume's
        p2c, c2w = (x if torch.is_tensor(x) else np.asarray(x, np.float32) for x in (pixtocams, camtoworlds))
        return self.raycast(p2c[idx] if p2c.ndim == 3 else p2c, c2w[idx][:3, :4], int(width), int(height), **kw)


def surface_metrics(volume, dataset, indices=None, renderings=None, depth_key='distance_median', **kw):
    """Scores of the exported surface against a dataset's views `indices` (default: all), each ray cast with
    `volume.raycast_view(dataset, idx, **kw)`:
        normals_mae  image.compute_weighted_mae(acc * alphas, normals, the dataset's normals), in degrees -- the score of the
                     model's normals, on the surface's; present when the dataset has `normal_images` and `alphas`;
        depth_l1     the mean of |depth - renderings[idx][depth_key]| over the pixels where both have acc >= 0.5; present when
                     `renderings` (a dict or sequence indexed by view, of what models.render_image returned) is given;
        coverage     the mean of acc.
    Returns dict(views={idx: {...}}, and each key's mean over the views that have it), float64 host scalars: nothing but the
    scalars leaves the device, in one transfer at the end."""
    from . import image
    indices = [int(i) for i in (range(dataset.size) if indices is None else indices)]
    normals_gt, alphas = getattr(dataset, 'normal_images', None), getattr(dataset, 'alphas', None)
    keys, rows = ['coverage'], []
    if normals_gt is not None and alphas is not None:
        keys.append('normals_mae')
    if renderings is not None:
        keys.append('depth_l1')
    for idx in indices:
        view = volume.raycast_view(dataset, idx, **kw)
        acc, dev = view['acc'], view['acc'].device
        row = dict(coverage=acc.double().mean())
        if 'normals_mae' in keys:
            w = acc * torch.as_tensor(alphas[idx], dtype=torch.float32, device=dev).reshape(acc.shape)
            gt = torch.as_tensor(normals_gt[idx], dtype=torch.float32, device=dev).reshape(view['normals'].shape)
            row['normals_mae'] = image.compute_weighted_mae(w.contiguous(), view['normals'], gt.contiguous()).double().reshape(())
        if 'depth_l1' in keys:
            r = renderings[idx]
            r_acc = torch.as_tensor(r['acc'], dtype=torch.float32, device=dev).reshape(acc.shape)
            r_depth = torch.as_tensor(r[depth_key], dtype=torch.float32, device=dev).reshape(acc.shape)
            both = ((acc >= 0.5) & (r_acc >= 0.5)).double()
            row['depth_l1'] = ((view['depth'].double() - r_depth.double()).abs() * both).sum() / both.sum()
        rows.append(torch.stack([row[k] for k in keys]))
    table = torch.stack(rows).cpu().numpy() if rows else np.zeros((0, len(keys)))
    out = dict(views={idx: {k: float(table[r, c]) for c, k in enumerate(keys)} for r, idx in enumerate(indices)})
    for c, k in enumerate(keys):
        out[k] = float(np.nanmean(table[:, c])) if len(indices) and not np.isnan(table[:, c]).all() else float('nan')
    return out


def fuse_views(render_fn, cameras, config, volume, indices=None, depth_key='distance_median', keep=None, **kw):
    """Render the views `indices` (default: all) of `cameras` -- anything with `.size`, `generate_ray_batch(idx)` and
    `.cameras` -- with `models.render_image` and fuse each into `volume`; renderings stay on the device.  `render_fn(rays)`
    is the eval forward, e.g. `lambda rays: model(rays, 1., True)`.  `keep`: a dict that receives, per view index, the
    rendering's `depth_key` and 'acc' -- what `surface_metrics` compares the surface's depth with.  Returns the volume."""
    from . import models
    _camera_tuple(cameras)
    for idx in (range(cameras.size) if indices is None else indices):
        batch = cameras.generate_ray_batch(int(idx))
        with torch.no_grad():
            rendering = models.render_image(render_fn, batch.rays, config, verbose=False, device=batch.rays.origins.device)
        volume.integrate_rendering(rendering, cameras, int(idx), depth_key=depth_key, **kw)
        if keep is not None:
            keep[int(idx)] = {depth_key: rendering[depth_key], 'acc': rendering['acc']}
    return volume


def write_surface_views(volume, cameras, out_dir, indices=None, **kw):
    """Ray cast the views `indices` (default: all) of `cameras` and write, per view, `surface_normals_<idx>.png` (n / 2 + .5,
    misses black) and `surface_depth_<idx>.png` (the hits' depths scaled to [0, 1] over the view, near bright, misses black)
    through the writer `models.render_path` uses (utils.save_img_u8), named like its artefacts.  Returns the paths written."""
    import os
    from . import utils
    indices = [int(i) for i in (range(cameras.size) if indices is None else indices)]
    zpad = max(3, len(str(max(indices, default=0))))
    os.makedirs(out_dir, exist_ok=True)
    done = []
    for idx in indices:
        view = volume.raycast_view(cameras, idx, **kw)
        depth, acc = view['depth'], view['acc']
        hit = acc > 0
        lo = torch.where(hit, depth, torch.full_like(depth, float('inf'))).min()
        hi = (depth * acc).max()
        panel = torch.where(hit, 1 - (depth - lo) / torch.clamp(hi - lo, min=torch.finfo(torch.float32).tiny), torch.zeros_like(depth))
        s = str(idx).zfill(zpad)
        for img, name in (((view['normals'] / 2 + .5) * acc[..., None], f'surface_normals_{s}.png'), (panel, f'surface_depth_{s}.png')):
            utils.save_img_u8(img, os.path.join(out_dir, name))
            done.append(os.path.join(out_dir, name))
    return done


def save_ply(path, vertices, faces, colors=None):
    """Binary little-endian PLY: float32 x y z (and uint8 red green blue, quantised as `utils.save_img_u8` does: NaN -> 0,
    clipped to [0, 1], times 255, truncated), faces as `list uchar int vertex_indices`."""
    def host(x):
        return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    v = np.ascontiguousarray(host(vertices), '<f4').reshape(-1, 3)
    f = np.ascontiguousarray(host(faces), '<i4').reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}', 'property float x', 'property float y',
              'property float z']
    if colors is not None:
        c = (np.clip(np.nan_to_num(host(colors).astype(np.float32)), 0., 1.) * 255).astype(np.uint8).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f'save_ply: {len(c)} colours for {len(v)} vertices')
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        header += ['property uchar red', 'property uchar green', 'property uchar blue']
    header += [f'element face {len(f)}', 'property list uchar int vertex_indices', 'end_header']
    vert = np.empty(len(v), dtype=fields)
    vert['x'], vert['y'], vert['z'] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        vert['red'], vert['green'], vert['blue'] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(f), dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    face['n'], face['v'] = 3, f
    with open(path, 'wb') as fp:
        fp.write(('\n'.join(header) + '\n').encode('ascii'))
        fp.write(vert.tobytes())
        fp.write(face.tobytes())

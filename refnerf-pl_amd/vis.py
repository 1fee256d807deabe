"""Validation visualisations: the reference's internal/vis.py (visualize_suite and its helpers), evaluated where the
rendering already is.  visualize_suite replaces the call at nerf_system.py:307; the panels stay on the device for
summary_writer.add_image.

Device tensors go through the kernels of csrc/refnerf_vis.h: the weighted percentiles from a deterministic float64 scan,
every per-pixel panel in one launch, the ray lines one launch per level, the ray panels one launch each.  The only ATen work
on that path is plumbing: the stable sorts the percentiles are taken from (torch.sort on the device), the float64 sort key
of the depth triplet, torch.linspace for the bin edges and torch.amax for `renormalize`.  visualize_suite never waits for
the device and never reads a device value on the host.  CPU tensors, or a library that has not been built, take a vectorised
ATen float64 path that implements the same definitions (no per-ray Python loop); it is also the baseline
scripts/time_vis.py times the kernels against.

Arithmetic: inputs are read as they are (float32 or float64), everything is computed in float64 and a float32 panel is
rounded once.  The results have the reference's keys, shapes and dtypes: for float32 renderings every panel is float32,
except `ray_colors`, which the reference's interp makes float64.

Reference behaviour kept where it surprises:
  * weighted_percentile evaluates its targets ps * acc_w[-1] / 100 in FLOAT32 when `ps` is a list of Python floats:
    torch.tensor(ps) is a float32 tensor and wins the promotion against the 0-dim float64 total.
  * a value map with more elements than the weight map ([H, W, 3] against [H, W]: the depth triplet) takes the weight of
    flat element j at j % len(weight), not at its pixel (vis.py:32).
  * interp extrapolates linearly outside its knots: a percentile target below the first cumulative weight gives a `lo`
    below every value, and a ray whose sdist does not cover dist_range is extrapolated, not clamped.
  * the reference's unstable argsort leaves the order of tied values undefined; here ties are taken in index order.
  * visualize_cmap's `lo = lo or ...` treats lo = torch.tensor(0) as unset, so visualize_suite's ray_weights panel takes
    its lower bound from a percentile over the whole panel with unit weights; hi = torch.tensor(1) is kept.
  * pixels of the ray_weights panel with ray_alpha == 0 become (1, 0, 0).
  * coords_mod is NaN where distance_mean is NaN (NaN * 0), as every product with a NaN is.
  * visualize_rays(renormalize=True) raises a TypeError in the reference (torch.max(float, Tensor)); here it divides by
    max(eps, max(vis_alpha)), which is what that line means.
n < 2 values raise ValueError (the reference: IndexError).  create_videos is not provided (it needs mediapy).
"""
import os

import numpy as np
import torch

from . import _hip, vis_tables

_EPS32 = float(torch.finfo(torch.float32).eps)
_FLOATS = (torch.float32, torch.float64)
MATTE_DARK, MATTE_LIGHT, MATTE_WIDTH = 0.8, 1.0, 8


def _kernels(t) -> bool:
    """Device tensors run through the library; CPU tensors (or no built library) through the ATen float64 path."""
    return bool(t.is_cuda) and os.path.exists(_hip.LIB_PATH)


# ------------------------------------------------------------------------------------------------- curves and tables
def identity_curve_fn(x):
    return x


def depth_curve_fn(x):
    """visualize_suite's curve of the depth panels"""
    return -torch.log(x + _EPS32)


def log_curve_fn(x):
    """visualize_suite's curve of the depth triplet"""
    return torch.log(x + _EPS32)


_CURVES = {identity_curve_fn: "none", depth_curve_fn: "neg_log", log_curve_fn: "log"}
_table_cache = {}


def _host_table(colormap):
    """float32 [N, 3] on the host, and the cache key"""
    if isinstance(colormap, str):
        if colormap == "turbo":
            return np.array(vis_tables.TURBO_BITS, dtype=np.uint32).view(np.float32).reshape(vis_tables.TURBO_N, 3), colormap
        if colormap == "gray":
            return (np.arange(256) / 255.0).astype(np.float32)[:, None].repeat(3, 1), colormap      # matplotlib's 'gray': k / 255
        raise ValueError(f"colormap {colormap!r}: 'turbo', 'gray', an [N, 3] tensor or a Colormap object is required")
    if callable(colormap) and hasattr(colormap, "N"):
        # sampled once, as Colormap.__call__ looks floats in [0, 1] up: entry min(int(v N), N - 1)
        return np.ascontiguousarray(np.asarray(colormap(np.arange(colormap.N)))[:, :3], dtype=np.float32), ("obj", id(colormap))
    raise ValueError("colormap: 'turbo', 'gray', an [N, 3] tensor or an object callable like a matplotlib Colormap with .N is required")


def color_table(colormap, device):
    """The [N, 3] float32 table of a `colormap` argument on `device` (cached), or None."""
    if colormap is None:
        return None
    if torch.is_tensor(colormap):
        if colormap.dim() != 2 or colormap.shape[1] != 3:
            raise ValueError(f"colormap: a table must be [N, 3], not {tuple(colormap.shape)}")
        return colormap.to(device=device, dtype=torch.float32).contiguous()
    key = colormap if isinstance(colormap, str) else ("obj", id(colormap))
    hit = _table_cache.get((key, str(device)))
    if hit is None:
        lut, key = _host_table(colormap)
        hit = (torch.from_numpy(lut).to(device), colormap)          # (the object is kept so that its id stays its own)
        _table_cache[(key, str(device))] = hit
    return hit[0]


# ------------------------------------------------------------------------------------------------- interp, percentiles
def _interp(x, xp, fp):
    """math.interp (math.py:114-142) along the last axis, batched: x [..., Q], xp [..., K], fp [..., K]; float64."""
    m = (fp[..., 1:] - fp[..., :-1]) / (xp[..., 1:] - xp[..., :-1])
    b = fp[..., :-1] - m * xp[..., :-1]
    idx = torch.sum(torch.ge(x.unsqueeze(-1), xp.unsqueeze(-2)), -1) - 1
    idx = torch.clamp(idx, 0, m.shape[-1] - 1)
    shape = torch.broadcast_shapes(idx.shape[:-1], m.shape[:-1]) + idx.shape[-1:]
    idx = idx.expand(shape)
    return torch.gather(m.expand(shape[:-1] + m.shape[-1:]), -1, idx) * x + torch.gather(b.expand(shape[:-1] + b.shape[-1:]), -1, idx)


def _percentile_targets(ps):
    """`ps` as a flat host tensor (nothing is uploaded on the kernel path), and whether the targets are float32"""
    ps_t = ps.detach().cpu() if torch.is_tensor(ps) else torch.tensor(ps)
    f32 = ps_t.dtype == torch.float32              # the reference's promotion: a float32 `ps` keeps the target in float32
    return ps_t.reshape(-1).to(torch.float32 if f32 else torch.float64), f32


def _percentiles(x, weight, ps, nan_mask=None, assume_sorted=False):
    """weighted_percentile on flat tensors; weight None = all ones; the weights are 0 where `nan_mask` is NaN."""
    n = x.numel()
    if n < 2:
        raise ValueError(f"weighted_percentile: at least two values are required, not {n}")
    ps_t, f32 = _percentile_targets(ps)
    if _kernels(x):
        if ps_t.numel() > _hip.VIS_MAX_PS:
            return torch.cat([_percentiles(x, weight, ps_t[i:i + _hip.VIS_MAX_PS], nan_mask, assume_sorted)
                              for i in range(0, ps_t.numel(), _hip.VIS_MAX_PS)])
        x = (x if x.dtype in _FLOATS else x.double()).contiguous()
        if weight is not None:
            weight = (weight if weight.dtype in _FLOATS else weight.double()).contiguous()
            if weight.numel() > n:                 # order % len(weight) never reaches past the first n weights
                weight = weight[:n]
            if nan_mask is not None:
                nan_mask = nan_mask.reshape(-1)[:weight.numel()].to(weight.dtype).contiguous()
        # plumbing: the stable ascending order (NaNs last) comes from torch.sort on the device
        order = torch.arange(n, device=x.device) if assume_sorted else torch.sort(x, stable=True).indices
        return _hip.vis_weighted_percentile(x, weight, order, ps_t.tolist(), f32, nan_mask)
    ps_t = ps_t.to(x.device)
    xd = x.double()
    wd = torch.ones(1, dtype=torch.float64, device=x.device) if weight is None else weight.double()
    if nan_mask is not None:
        wd = torch.where(torch.isnan(nan_mask), torch.zeros_like(wd), wd)
    if assume_sorted:
        w = wd.expand(n) if weight is None else wd
    else:
        xd, order = torch.sort(xd, stable=True)
        w = wd[torch.remainder(order, wd.numel())]
    acc_w = torch.cumsum(w, 0)
    total = acc_w[-1].to(ps_t.dtype)
    target = torch.div(ps_t * total, torch.full((), 100.0, dtype=ps_t.dtype, device=x.device)).double()   # a true division
    return _interp(target, acc_w, xd)


def weighted_percentile(x, weight, ps, assume_sorted=False):
    """vis.py:26-36: the weighted percentile(s) of a single vector, float64 [len(ps)] on x's device."""
    return _percentiles(x.reshape([-1]), weight.reshape([-1]), ps, assume_sorted=assume_sorted)


def sinebow(h):
    """vis.py:39-42: a cyclic and uniform colormap."""
    def f(x):
        return torch.sin(torch.pi * x) ** 2
    return torch.stack([f(3 / 6 - h), f(5 / 6 - h), f(7 / 6 - h)], -1)


# ------------------------------------------------------------------------------------------------- matte, cmap
def _checker(H, W, dark, light, width, device):
    ys = (torch.arange(H, device=device) % (2 * width) // width)[:, None]
    xs = (torch.arange(W, device=device) % (2 * width) // width)[None, :]
    return torch.where(torch.logical_xor(ys, xs), light, dark).double()      # a float32 tensor in the reference: float32(0.8)


def _matte64(vis, acc, dark=MATTE_DARK, light=MATTE_LIGHT, width=MATTE_WIDTH):
    bg = _checker(acc.shape[0], acc.shape[1], dark, light, width, vis.device)
    return vis * acc[:, :, None] + (bg * (1 - acc))[:, :, None]


def _default_matte(dark, light, width):
    return dark == MATTE_DARK and light == MATTE_LIGHT and width == MATTE_WIDTH


def matte(vis, acc, dark=0.8, light=1.0, width=8):
    """vis.py:45-52: set non-accumulated pixels to a Photoshop-esque checker pattern."""
    out_dtype = torch.promote_types(vis.dtype, acc.dtype)
    if (_kernels(vis) and _default_matte(dark, light, width) and vis.dim() == 3 and 1 <= vis.shape[-1] <= 4
            and vis.dtype == acc.dtype and vis.dtype in _FLOATS and tuple(acc.shape) == tuple(vis.shape[:2])):
        H, W, Cn = vis.shape
        return _hip.vis_cmap(vis.contiguous(), H, W, Cn, out_dtype, acc=acc.contiguous())
    return _matte64(vis.double(), acc.double(), dark, light, width).to(out_dtype)


def _bound(b):
    """visualize_cmap's `lo or auto`: None, 0 and a tensor holding 0 all count as unset (a device tensor is read)."""
    return b is not None and bool(b)


def visualize_cmap(value, weight, colormap, lo=None, hi=None, percentile=99., curve_fn=identity_curve_fn, modulus=None,
                   matte_background=True):
    """vis.py:55-116: visualize a 1D image and a 1D weighting according to some colormap.

    `colormap`: None (value must be [H, W, 3]), 'turbo', 'gray', an [N, 3] tensor, or an object callable like a matplotlib
    Colormap with .N (sampled once and cached).  `curve_fn`: identity_curve_fn, depth_curve_fn and log_curve_fn run inside
    the kernel; any other callable is applied with ATen.  The bounds follow the reference's `lo = lo or (lo_auto - eps)`:
    a bound that is None or zero is replaced by the percentile."""
    pct = weighted_percentile(value, weight, [50 - percentile / 2, 50 + percentile / 2])
    table = color_table(colormap, value.device)
    if table is None:
        if value.dim() != 3:
            raise ValueError(f'value must have 3 dims but has {value.dim()}')
        if value.shape[-1] != 3:
            raise ValueError(f'value must have 3 channels but has {value.shape[-1]}')
    col_dtype = torch.float32 if table is not None else (value.dtype if value.dtype.is_floating_point else torch.float32)
    out_dtype = torch.promote_types(col_dtype, weight.dtype) if matte_background else col_dtype
    lo_set, hi_set = _bound(lo), _bound(hi)

    def host_number(b):
        return not torch.is_tensor(b) or not b.is_cuda
    if (_kernels(value) and curve_fn in _CURVES and not modulus and value.dtype in _FLOATS and out_dtype in _FLOATS
            and value.dim() == (2 if table is not None else 3) and (not lo_set or host_number(lo)) and (not hi_set or host_number(hi))
            and (not matte_background or (weight.dtype == value.dtype and tuple(weight.shape) == tuple(value.shape[:2])))):
        H, W = value.shape[:2]
        return _hip.vis_cmap(value.contiguous(), H, W, 1 if table is not None else 3, out_dtype, curve=_CURVES[curve_fn], normalise=True,
                             d_lo=None if lo_set else pct[0:1], lo_bias=float(lo) if lo_set else -_EPS32,
                             d_hi=None if hi_set else pct[1:2], hi_bias=float(hi) if hi_set else _EPS32, table=table,
                             acc=weight.contiguous() if matte_background else None)
    v = value.double()
    lo_v = torch.as_tensor(lo, device=v.device).double() if lo_set else pct[0] - _EPS32
    hi_v = torch.as_tensor(hi, device=v.device).double() if hi_set else pct[1] + _EPS32
    v, lo_v, hi_v = [curve_fn(z) for z in (v, lo_v, hi_v)]
    if modulus:
        v = torch.remainder(v, modulus) / modulus
    else:
        v = torch.nan_to_num(torch.clip((v - torch.minimum(lo_v, hi_v)) / torch.abs(hi_v - lo_v), 0, 1))
    if table is not None:
        v = _lookup(v, table)
    return (_matte64(v, weight.double()) if matte_background else v).to(out_dtype)


def _lookup(v, table):
    """Colormap.__call__ on floats: entry min(int(v N), N - 1), the first entry below 0, zeros for a NaN; float64 [..., 3]"""
    n = table.shape[0]
    idx = torch.clamp((torch.nan_to_num(v) * n).long(), 0, n - 1)
    return torch.where(torch.isnan(v)[..., None], torch.zeros((), dtype=torch.float64, device=v.device), table[idx].double())


def visualize_coord_mod(coords, acc):
    """vis.py:119-121: the coordinate of each point within its "cell"."""
    out_dtype = torch.promote_types(coords.dtype, acc.dtype)
    v = torch.remainder(coords.double() + 1, 2) / 2
    if _kernels(coords):
        return _hip.vis_cmap(v.contiguous(), v.shape[0], v.shape[1], v.shape[2], out_dtype, acc=acc.double().contiguous())
    return _matte64(v, acc.double()).to(out_dtype)


# ------------------------------------------------------------------------------------------------- ray bundles
def _ray_lines_aten(ds, vs, ws, edges, accumulate):
    """one level: ds [n, N+1], vs [n, N, C], ws [n, N] (float64) -> (values [n, res, C], alpha [n, res])"""
    if accumulate:                                   # vis.py:138-143
        w_csum = torch.cumsum(ws, 1)
        rw_csum = torch.cumsum(vs * ws[..., None], 1)
        vs, ws = (rw_csum + _EPS32) / (w_csum[..., None] + 2 * _EPS32), w_csum
    wp = torch.diff(ds, dim=-1)
    fn = torch.cat([vs * wp[..., None], (ws * wp)[..., None], wp[..., None]], -1)            # [n, N, C + 2]
    acc0 = torch.cat([torch.zeros_like(fn[:, :1]), torch.cumsum(fn, 1)], 1).transpose(1, 2)   # [n, C + 2, N + 1]
    at = _interp(edges.expand(ds.shape[0], 1, -1), ds[:, None, :], acc0)                      # [n, C + 2, res + 1]
    v = torch.diff(at, dim=-1)
    v = v[:, :-1] / torch.clamp(v[:, -1:], min=_EPS32)                                        # numer / max(eps, denom)
    return v[:, :-1].transpose(1, 2), v[:, -1]


def _visualize_rays(dist, dist_range, weights, values, value_op, accumulate, renormalize, resolution, bg_color):
    """visualize_rays with the suite's input operations folded in: weights None = all ones, value_op 'clip01' / 'sqrt'."""
    L, n = len(dist), dist[0].shape[0]
    dev = dist[0].device
    edges = torch.linspace(*dist_range, resolution + 1, device=dev).double()     # a float32 linspace, as in the reference
    Cn = values[0].shape[-1]
    rep = 0
    if resolution > n:
        rep = resolution // (n * L + 1)
        if rep == 0:
            raise ValueError(f"visualize_rays: resolution {resolution} leaves no row for {n} rays x {L} levels")
    if _kernels(dist[0]):
        lines_v = torch.empty((n, L, resolution, Cn), dtype=torch.float64, device=dev)
        lines_a = torch.empty((n, L, resolution), dtype=torch.float64, device=dev)
        for lvl in range(L):
            dt = dist[lvl].dtype if dist[lvl].dtype in _FLOATS else torch.float64
            w = None if weights is None else weights[lvl].to(dt).contiguous()
            _hip.vis_resample_rays(dist[lvl].to(dt).contiguous(), values[lvl].to(dt).contiguous(), w, edges, lines_v, lines_a, lvl,
                                   accumulate=accumulate, value_op=value_op)
        alpha_max = torch.amax(lines_a) if renormalize else None      # plumbing: no synchronisation
        return _hip.vis_ray_panel(lines_v, lines_a, rep, bg_color, alpha_max)
    lv, la = [], []
    for lvl in range(L):
        v = values[lvl].double()
        v = torch.clip(v, 0, 1) if value_op == "clip01" else (torch.sqrt(v) if value_op == "sqrt" else v)
        w = torch.ones(v.shape[:2], dtype=torch.float64, device=dev) if weights is None else weights[lvl].double()
        a, b = _ray_lines_aten(dist[lvl].double(), v, w, edges, accumulate)
        lv.append(a)
        la.append(b)
    lines_v, lines_a = torch.stack(lv, 1), torch.stack(la, 1)
    if renormalize:
        lines_a = lines_a / torch.clamp(torch.amax(lines_a), min=_EPS32)
    vis = lines_v * lines_a[..., None] + (bg_color * (1 - lines_a))[..., None]     # the matte commutes with the tiling
    if rep == 0:
        return vis[:-1], lines_a[:-1]
    strip = torch.full((n, 1, resolution, Cn), 0.0 * 0.0 + bg_color * (1 - 0.0), dtype=torch.float64, device=dev)
    body = vis[:, :, None].expand(n, L, rep, resolution, Cn).reshape(n, L * rep, resolution, Cn)
    body_a = lines_a[:, :, None].expand(n, L, rep, resolution).reshape(n, L * rep, resolution)
    vis = torch.cat([body, strip], 1).reshape(-1, resolution, Cn)[:-1]
    alpha = torch.cat([body_a, torch.zeros_like(body_a[:, :1])], 1).reshape(-1, resolution)[:-1]
    return vis, alpha


def visualize_rays(dist, dist_range, weights, rgbs, accumulate=False, renormalize=False, resolution=2048, bg_color=0.8):
    """vis.py:124-181: visualize a bundle of rays.  `dist`, `weights`, `rgbs`: one [n, N+1] / [n, N] / [n, N, C] tensor per
    level.  Returns (vis [rows, resolution, C], vis_alpha [rows, resolution]) in float64, rows = n (L rep + 1) - 1 with
    rep = resolution // (n L + 1); resolution <= n skips the tiling and returns the [n - 1, L, resolution(, C)] lines."""
    vis, alpha = _visualize_rays(list(dist), dist_range, list(weights), list(rgbs), "none", accumulate, renormalize, int(resolution),
                                 float(bg_color))
    if int(resolution) <= dist[0].shape[0]:
        n, L = dist[0].shape[0], len(dist)
        return vis.reshape(n - 1, L, resolution, -1), alpha.reshape(n - 1, L, resolution)
    return vis, alpha


# ------------------------------------------------------------------------------------------------- the suite
_PS = [50 - 99. / 2, 50 + 99. / 2]


def visualize_suite(rendering, rays, linear_to_srgb):
    """vis.py:184-292: a wrapper around the other visualizations; `rendering` is the dict of models.render_image
    ([H, W, ...] tensors plus the ray_* lists), `rays` carries origins and directions.  On device tensors nothing here
    waits for the device."""
    rgb = rendering['rgb']
    dt = rgb.dtype if rgb.dtype in _FLOATS else torch.float64
    H, W = rendering['acc'].shape
    normal_keys = [k for k, v in rendering.items() if k.startswith('normals') and v is not None]
    dist, weights, rgbs = rendering['ray_sdist'], rendering['ray_weights'], rendering['ray_rgbs']
    ray_colors, _ = _visualize_rays(dist, (0, 1), weights, rgbs, "clip01", False, False, 2048, 0.8)
    sqrt_ray_weights, ray_alpha = _visualize_rays(dist, (0, 1), None, [w[..., None] for w in weights], "sqrt", False, False, 2048, 0.)
    sqrt_ray_weights = sqrt_ray_weights[..., 0]
    # The reference passes lo=torch.tensor(0), hi=torch.tensor(1): `lo or ...` takes the zero for "unset", so the lower bound
    # is the 0.5th percentile of the whole panel with unit weights (minus eps); the upper bound 1 is kept.
    pct_rw = _percentiles(sqrt_ray_weights.reshape(-1), None, _PS)

    if _kernels(rgb):
        def g(x):
            return x.to(dt).contiguous()
        acc, dmean, dmedian = g(rendering['acc']), g(rendering['distance_mean']), g(rendering['distance_median'])
        p5, p95 = g(rendering['distance_percentile_5']), g(rendering['distance_percentile_95'])
        # plumbing: the float64 sort key of the triplet's percentiles (the kernel recomputes the triplet per pixel)
        triplet = torch.stack([2 * dmedian.double() - p5.double(), dmedian.double(), p95.double()], dim=-1)
        flat_acc, flat_nan = acc.reshape(-1), dmean.reshape(-1)                 # acc counts as 0 where distance_mean is NaN
        lohi = [_percentiles(z.reshape(-1), flat_acc, _PS, nan_mask=flat_nan) for z in (dmean, dmedian, triplet)]
        inputs = dict(rgb=g(rgb), acc=acc, distance_mean=dmean, distance_median=dmedian, distance_p5=p5, distance_p95=p95,
                      origins=g(rays.origins), directions=g(rays.directions))
        outputs = ['acc_out', 'color_matte', 'depth_mean', 'depth_median', 'depth_triplet', 'coords_mod']
        if linear_to_srgb:
            outputs.append('color')
        rc = 1
        if 'roughness' in rendering:
            inputs['roughness'] = g(rendering['roughness'])
            rc = inputs['roughness'].numel() // (H * W)
            outputs.append('roughness_out')
        for key in ('diffuse', 'specular'):
            if key in rendering:
                inputs[key] = g(rendering[key])
                outputs += [key + '_matte'] + ([key + '_out'] if linear_to_srgb else [])
        if 'tint' in rendering:
            inputs['tint'] = g(rendering['tint'])
            outputs.append('tint_matte')
        normals = [g(rendering[k]) for k in normal_keys]
        table = color_table('turbo', rgb.device)
        out = _hip.vis_panels(H, W, dt, linear_to_srgb, table, inputs, outputs, lohi, normals[:_hip.VIS_MAX_NORMALS], rc)
        normals_out = out['normals_out']
        for i in range(_hip.VIS_MAX_NORMALS, len(normals), _hip.VIS_MAX_NORMALS):      # more than four maps: further launches
            normals_out += _hip.vis_panels(H, W, dt, False, None, dict(acc=acc, distance_mean=dmean), [], normals=normals[i:i + 4])['normals_out']
        if 'roughness_out' in out:
            out['roughness_out'] = out['roughness_out'].reshape(rendering['roughness'].shape)
        rh, rw = sqrt_ray_weights.shape
        ray_weights = _hip.vis_cmap(sqrt_ray_weights, rh, rw, 1, torch.float32, normalise=True, d_lo=pct_rw[0:1], lo_bias=-_EPS32,
                                    hi_bias=1.0, table=color_table('gray', rgb.device), alpha=ray_alpha, null_color=(1., 0., 0.))
    else:
        def d(x):
            return x.double()
        srgb = _linear_to_srgb64 if linear_to_srgb else (lambda x: x)
        dmean = d(rendering['distance_mean'])
        acc = torch.where(torch.isnan(dmean), torch.zeros_like(dmean), d(rendering['acc']))
        dmedian, p5, p95 = d(rendering['distance_median']), d(rendering['distance_percentile_5']), d(rendering['distance_percentile_95'])
        triplet = torch.stack([2 * dmedian - p5, dmedian, p95], dim=-1)
        turbo = color_table('turbo', rgb.device)

        def cmap(value, pct, curve, table):
            lo, hi = curve(pct[0] - _EPS32), curve(pct[1] + _EPS32)
            v = torch.nan_to_num(torch.clip((curve(value) - torch.minimum(lo, hi)) / torch.abs(hi - lo), 0, 1))
            return _matte64(v if table is None else _lookup(v, table), acc)
        flat_acc = acc.reshape(-1)
        out = dict(acc_out=acc, color=srgb(d(rgb)))
        out['color_matte'] = _matte64(out['color'], acc)
        out['depth_mean'] = cmap(dmean, _percentiles(dmean.reshape(-1), flat_acc, _PS), depth_curve_fn, turbo)
        out['depth_median'] = cmap(dmedian, _percentiles(dmedian.reshape(-1), flat_acc, _PS), depth_curve_fn, turbo)
        out['depth_triplet'] = cmap(triplet, _percentiles(triplet.reshape(-1), flat_acc, _PS), log_curve_fn, None)
        coords = d(rays.origins) + d(rays.directions) * dmean[:, :, None]
        out['coords_mod'] = _matte64(torch.remainder(coords + 1, 2) / 2, acc)
        normals_out = [_matte64(d(rendering[k]) / 2. + 0.5, acc) for k in normal_keys]
        if 'roughness' in rendering:
            out['roughness_out'] = _matte64(torch.tanh(d(rendering['roughness'])), acc)
        for key in ('diffuse', 'specular'):
            if key in rendering:
                out[key + '_out'] = srgb(d(rendering[key]))
                out[key + '_matte'] = _matte64(out[key + '_out'], acc)
        if 'tint' in rendering:
            out['tint_matte'] = _matte64(d(rendering['tint']), acc)
        out = {k: v.to(dt) for k, v in out.items()}
        normals_out = [v.to(dt) for v in normals_out]
        lo, hi = pct_rw[0] - _EPS32, torch.ones((), dtype=torch.float64, device=rgb.device)
        v = torch.nan_to_num(torch.clip((sqrt_ray_weights - torch.minimum(lo, hi)) / torch.abs(hi - lo), 0, 1))
        ray_weights = _lookup(v, color_table('gray', rgb.device)).float()
        null_color = torch.tensor([1., 0., 0.], device=rgb.device)
        ray_weights = torch.where(ray_alpha[:, :, None] == 0, null_color[None, None], ray_weights)      # vis.py:249-253

    vis = {
        'color': out['color'] if linear_to_srgb else rgb,
        'acc': out['acc_out'],
        'color_matte': out['color_matte'],
        'depth_mean': out['depth_mean'],
        'depth_median': out['depth_median'],
        'depth_triplet': out['depth_triplet'],
        'coords_mod': out['coords_mod'],
        'ray_colors': ray_colors,
        'ray_weights': ray_weights,
    }
    if 'rgb_cc' in rendering:
        vis['color_corrected'] = rendering['rgb_cc']
    for key, val in zip(normal_keys, normals_out):
        vis[key] = val
    if 'roughness' in rendering:
        vis['roughness'] = out['roughness_out']
    for key in ('diffuse', 'specular'):
        if key in rendering:
            vis[key] = out[key + '_out'] if linear_to_srgb else rendering[key]
            vis[key + '_matte'] = out[key + '_matte']
    if 'tint' in rendering:
        vis['tint'] = rendering['tint']
        vis['tint_matte'] = out['tint_matte']
    return vis


def _linear_to_srgb64(linear):
    """image.py:51-59 on a float64 tensor (torch.maximum keeps a NaN, and so does this)"""
    srgb0 = 323 / 25 * linear
    srgb1 = (211 * torch.clamp(linear, min=_EPS32) ** (5 / 12) - 11) / 200
    return torch.where(linear <= 0.0031308, srgb0, srgb1)

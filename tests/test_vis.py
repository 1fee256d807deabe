"""refnerf_pl_amd.vis: the reference's visualize_suite and its helpers on the device (csrc/refnerf_vis.h).

Truth.  tests/golden/vis_suite.npz (make_golden_vis.py) holds the outputs of the reference's internal/vis.py on FLOAT64
copies of the float32-representable inputs that the seeded recipes below regenerate, plus the outputs of its float32 run of
the suite (stored losslessly as the distance in float32 steps from the rounded float64 truth).  Ray panels are stored as
their distinct lines (n L lines and the background strip) and the panel shape; the full panel is checked row by row against
its representative line.

Bars, all against the reference's float64 outputs:
  float32 panels with values in [0, 1]   2^-24 + 1e-9 absolute (half a step of the one output rounding + the device bar
                                         of the project's float64 kernels)
  float64 outputs                        1e-9, absolute or relative to max(1, |x|) (percentiles, ray_colors, ray lines)
  table indices                          identical on every pixel: the ray_weights panel (float32 table entries, no matte)
                                         must EQUAL the reference's
  NaN positions                          identical
  against the reference's float32 run    the bar above + the fixture's own |float32 run - float64 run| of that panel
test_fixture_conditions asserts what keeps these gates honest: no tied values in any weighted percentile input (the
reference's unstable argsort is undefined there; the module takes ties in index order, and with unit weights ties change
nothing), no percentile target within 1e-9 (relative to the total weight) of a cumulative knot, no normalised value within
1e-7 of a k / 256 table boundary, and depth panels that differ from a constant image by more than 0.1.

MEASURED on an MI355X (the GPU tests print these lines)
  visualize_suite on float32 renderings, L-inf against the reference's float64 run (bar 2^-24 + 1e-9 = 6.06e-8), both
  settings of linear_to_srgb: every per-pixel panel 2.98e-8 (= 2^-25, the one output rounding), acc 0; against the reference's
  float32 run 5.96e-8 .. 2.98e-7 (depth_triplet), each below the bar plus that run's own distance (7.6e-8 .. 2.77e-7);
  ray_colors 0 (bar 1e-9), against the float32 run 7.90e-7 (its own distance 7.90e-7); ray_weights equal
  visualize_suite on the float64 copies (bar 1e-9): 0 .. 2.2e-16 on every panel
  weighted percentiles (weighted and unit weights, mirror and entry, float32 and float64 inputs): 0 on all four cases
  visualize_cmap heavy_ends 2.98e-8 (float32) / 0 (float64), empty 0; visualize_rays (all five cases, panel and alpha) 0
  the entries from the fixture's own percentiles: panels 2.98e-8, ray panel and alpha 0
"""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_suite.npz")
DEV = "cuda:0"
EPS32 = 2.0 ** -23
BAR32 = 2.0 ** -24 + 1e-9
BAR64 = 1e-9
PS = [0.5, 5.0, 37.0, 95.0, 99.5]       # (no unit-weight target of the cases below is a whole number: none sits on a knot)
SUITE_PS = [50 - 99. / 2, 50 + 99. / 2]


# ------------------------------------------------------------------------------------------------- recipes
def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def smooth(rng, H, W, C):
    """two low-frequency sinusoids per channel in [0, 1]"""
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    out = np.empty((H, W, C))
    for c in range(C):
        f = rng.uniform(0.4, 1.6, 4)
        ph = rng.uniform(0.0, 2.0 * np.pi, 2)
        out[..., c] = 0.5 + 0.3 * np.sin(2 * np.pi * (f[0] * xx + f[1] * yy) + ph[0]) + 0.2 * np.sin(2 * np.pi * (f[2] * xx - f[3] * yy) + ph[1])
    return out


def unit(rng, shape):
    v = rng.standard_normal(shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


SUITE = dict(seed=58, H=37, W=53)        # (a seed at which test_fixture_conditions holds: no ties, no value on a table boundary)
ZERO_ACC_ROWS = (4, 17, 30)
NAN_PIXELS = ((2, 3), (10, 40), (36, 52))
RAYS = dict(seed=51, n=3, levels=(5, 9))


def ray_inputs(seed, n, levels):
    """(sdist [n, N+1], weights [n, N], rgbs [n, N, 3]) per level, float32.  Ray 1 spans only [0.1, 0.9] (the reference
    extrapolates outside), the colours reach 1.2 (the suite clips them)."""
    rng = np.random.default_rng(seed)
    sdist, weights, rgbs = [], [], []
    for N in levels:
        s = np.sort(rng.uniform(0.0, 1.0, (n, N + 1)), -1)
        s[:, 0], s[:, -1] = 0.0, 1.0
        s[1] = 0.1 + 0.8 * s[1]
        w = rng.uniform(0.05, 1.0, (n, N))
        w /= w.sum(-1, keepdims=True) * rng.uniform(1.0, 1.5, (n, 1))
        sdist.append(_f32(s))
        weights.append(_f32(w))
        rgbs.append(_f32(rng.uniform(0.0, 1.2, (n, N, 3))))
    return sdist, weights, rgbs


def suite_inputs(seed, H, W):
    """a synthetic rendering of one validation view (every optional key present) and its rays, float32"""
    rng = np.random.default_rng(seed)
    r = {}
    r["rgb"] = np.clip(smooth(rng, H, W, 3) + 0.03 * rng.standard_normal((H, W, 3)), 0.0, 1.0)
    acc = rng.uniform(0.2, 1.0, (H, W))
    acc[list(ZERO_ACC_ROWS)] = 0.0
    r["acc"] = acc
    dmean = 2.0 + 4.0 * smooth(rng, H, W, 1)[..., 0] + 0.05 * rng.standard_normal((H, W))
    dmedian = dmean + 0.05 * rng.standard_normal((H, W))
    r["distance_mean"], r["distance_median"] = dmean, dmedian
    r["distance_percentile_5"] = dmedian - rng.uniform(0.05, 0.5, (H, W))
    r["distance_percentile_95"] = dmedian + rng.uniform(0.05, 0.5, (H, W))
    for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
        for y, x in NAN_PIXELS:
            r[k][y, x] = np.nan
    r["normals"] = unit(rng, (H, W)) * rng.uniform(0.5, 1.0, (H, W, 1))
    r["normals_pred"] = unit(rng, (H, W)) * rng.uniform(0.5, 1.0, (H, W, 1))
    r["roughness"] = rng.standard_normal((H, W, 1))
    r["diffuse"] = rng.uniform(0.0, 1.0, (H, W, 3))
    r["diffuse"][0, :8] *= 0.003                       # the linear branch of the sRGB curve
    r["specular"] = rng.uniform(0.0, 1.0, (H, W, 3))
    r["tint"] = rng.uniform(0.0, 1.0, (H, W, 3))
    r["rgb_cc"] = rng.uniform(0.0, 1.0, (H, W, 3))
    r = {k: _f32(v) for k, v in r.items()}
    r["ray_sdist"], r["ray_weights"], r["ray_rgbs"] = ray_inputs(**RAYS)
    origins = _f32(rng.uniform(-1.0, 1.0, (H, W, 3)))
    directions = _f32(unit(rng, (H, W)))
    return r, origins, directions


PCT_CASES = {
    "small_5x7": dict(kind="random", H=5, W=7, seed=41),            # fewer elements than one block
    "blocks_96x128": dict(kind="random", H=96, W=128, seed=42),     # six blocks of block sums
    "heavy_ends": dict(kind="heavy_ends", H=12, W=21, seed=43),     # the target falls below the first knot: extrapolation
    "empty": dict(kind="empty", H=12, W=21, seed=44),               # all weights 0: NaN percentiles
}


def pct_inputs(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    # a jittered permutation of a grid: no two values tie after the rounding to float32
    value = _f32(2.1 + 3.8 * ((rng.permutation(H * W) + rng.uniform(0.1, 0.9, H * W)) / (H * W)).reshape(H, W))
    if kind == "random":
        weight = rng.random((H, W))
    elif kind == "heavy_ends":
        weight = rng.uniform(1e-3, 2e-3, (H, W))
        weight.flat[np.argmin(value)] = 0.5
        weight.flat[np.argmax(value)] = 0.5
    else:
        weight = np.zeros((H, W))
    return value, _f32(weight)


RAY_CASES = {
    "plain": dict(accumulate=False, renormalize=False, resolution=64),
    "accumulate": dict(accumulate=True, renormalize=False, resolution=64),
    "renormalize": dict(accumulate=False, renormalize=True, resolution=64),
    "both": dict(accumulate=True, renormalize=True, resolution=64),
    "untiled": dict(accumulate=False, renormalize=False, resolution=3),       # resolution <= n skips the tiling
}
PARAMS = dict(suite=SUITE, rays=RAYS, pct=PCT_CASES, ray_cases=RAY_CASES, ps=PS)
PASSTHROUGH = {"color": "rgb", "color_corrected": "rgb_cc", "tint": "tint", "diffuse": "diffuse", "specular": "specular"}
SRGB_KEYS = ("color", "color_matte", "diffuse", "diffuse_matte", "specular", "specular_matte")


def neg_log_curve(x):
    return -torch.log(x + EPS32)


def ray_panel_rows(n, L, rep):
    """line index of every panel row (n L = the background strip)"""
    per = L * rep + 1
    rows = np.arange(n * per - 1)
    j = rows % per
    return np.where(j == L * rep, n * L, (rows // per) * L + j // rep)


def ulps_encode(run32, truth64):
    """the float32 run as whole float32 steps away from the rounded truth (lossless, and it compresses)"""
    a = np.ascontiguousarray(run32, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(truth64.astype(np.float32)).view(np.int32).astype(np.int64)
    return np.where(np.isnan(run32), 0, a - b).astype(np.int32)


def ulps_decode(ulps, truth64):
    b = np.ascontiguousarray(truth64.astype(np.float32)).view(np.int32).astype(np.int64)
    out = (b + ulps).astype(np.int32).view(np.float32)
    return np.where(np.isnan(truth64), np.float32(np.nan), out)


# ------------------------------------------------------------------------------------------------- shared
@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    assert json.loads(str(g["params"])) == json.loads(json.dumps(PARAMS))
    return g


@functools.lru_cache(maxsize=None)
def suite_np():
    return suite_inputs(**SUITE)


def suite_torch(device, f64):
    r, o, d = suite_np()

    def t(x):
        x = torch.from_numpy(x)
        return (x.double() if f64 else x).to(device)
    rendering = {k: [t(z) for z in v] if isinstance(v, list) else t(v) for k, v in r.items()}
    return rendering, types.SimpleNamespace(origins=t(o), directions=t(d))


def npy(x):
    return x.detach().cpu().numpy()


def err(got, want, what, relative=False):
    """L-inf distance, with identical NaN positions"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    d = np.abs(got - want)
    if relative:
        d = d / np.maximum(1.0, np.abs(want))
    return float(np.nanmax(d)) if d.size and not np.all(np.isnan(d)) else 0.0


def suite_truth(g, srgb, key):
    """the float64-run panel `key`, or None where the reference returns its input"""
    if srgb and key in SRGB_KEYS:
        return g["suite64_srgb_" + key]
    return g.get("suite64_" + key)


def check_ray_panel(panel, lines, strip, n, L, rep, what, bar, exact=False):
    """every row of the device (or host) panel against its representative line"""
    ext = np.concatenate([lines, np.broadcast_to(strip, (1,) + lines.shape[1:])], 0)
    idx = torch.from_numpy(ray_panel_rows(n, L, rep)).to(panel.device)
    want = torch.from_numpy(np.ascontiguousarray(ext)).to(panel.device)[idx]
    assert tuple(panel.shape) == tuple(want.shape), (what, tuple(panel.shape), tuple(want.shape))
    assert not bool(torch.isnan(panel).any())
    if exact:
        assert torch.equal(panel, want), what
        return 0.0
    e = float(((panel - want).abs() / torch.clamp(want.abs(), min=1.0)).max())
    print(f"MEASURED {what}: {e:.2e} (bar {bar:.2e})")
    assert e <= bar, (what, e)
    return e


def check_suite(vis, g, srgb, f64, inputs, tag):
    """one visualize_suite result against the fixture: keys, shapes, dtypes, every panel"""
    rendering, _ = inputs
    meta = json.loads(str(g["suite_meta"]))["f64" if f64 else "f32"]
    assert list(vis) == [k for k, _, _ in meta], (list(vis), [k for k, _, _ in meta])
    n, L = RAYS["n"], len(RAYS["levels"])
    rep = 2048 // (n * L + 1)
    for key, dtype, shape in meta:
        got = vis[key]
        assert str(got.dtype) == dtype and list(got.shape) == shape, (key, got.dtype, tuple(got.shape), dtype, shape)
        if key == "ray_colors":
            check_ray_panel(got, g["suite64_ray_colors_lines"], g["suite64_ray_colors_strip"], n, L, rep, f"{tag} ray_colors", BAR64)
            if not f64:
                e32 = float(np.abs(g["suite32_ray_colors_lines"] - g["suite64_ray_colors_lines"]).max())
                check_ray_panel(got, g["suite32_ray_colors_lines"], g["suite64_ray_colors_strip"], n, L, rep,
                                f"{tag} ray_colors vs the float32 run", BAR64 + e32)
            continue
        if key == "ray_weights":      # float32 table entries and the null colour: identical indices <=> equality
            check_ray_panel(got, g["suite64_ray_weights_lines"], g["suite64_ray_weights_strip"], n, L, rep, f"{tag} ray_weights", 0.0, exact=True)
            continue
        truth = suite_truth(g, srgb, key)
        if truth is None:                 # the reference returns its input there, and so does the module
            assert key in PASSTHROUGH and got is rendering[PASSTHROUGH[key]], key
            continue
        bar = BAR64 if f64 else BAR32
        e = err(npy(got), truth, f"{tag} {key}")
        line = f"MEASURED {tag} {key}: {e:.2e} (bar {bar:.2e})"
        assert e <= bar, line
        if not f64:
            name = ("suite32_srgb_" if srgb and key in SRGB_KEYS else "suite32_") + key + "_ulps"
            run32 = ulps_decode(g[name], truth)
            own = err(run32, truth, key)
            e2 = err(npy(got), run32, f"{tag} {key} vs the float32 run")
            line += f"; vs the float32 run {e2:.2e} (its own distance {own:.2e})"
            assert e2 <= bar + own, line
        print(line)


def knot_margin(values, weights, ps):
    """min |target - knot| / total over the percentiles, as the reference evaluates the targets (float32)"""
    v = values.reshape(-1).astype(np.float64)
    order = np.argsort(v, kind="stable")
    w = np.ones(v.size) if weights is None else weights.reshape(-1).astype(np.float64)[order % weights.size]
    acc = np.cumsum(w)
    if not acc[-1] > 0:
        return np.inf
    t = (np.array(ps, np.float32) * np.float32(acc[-1]) / np.float32(100)).astype(np.float64)
    return float(np.abs(t[:, None] - acc[None, :]).min() / acc[-1])


def table_margin(u):
    """distance of the unclipped normalised values inside (0, 1) to the nearest interior k / 256"""
    u = u[np.isfinite(u) & (u > 0) & (u < 1)]
    k = np.clip(np.rint(u * 256), 1, 255)
    return float(np.abs(u - k / 256).min()) if u.size else np.inf


def suite_acc0():
    r = suite_np()[0]
    return np.where(np.isnan(r["distance_mean"]), np.float32(0), r["acc"])


def suite_triplet64():
    r = {k: v.astype(np.float64) for k, v in suite_np()[0].items() if not k.startswith("ray_")}
    return np.stack([2 * r["distance_median"] - r["distance_percentile_5"], r["distance_median"], r["distance_percentile_95"]], -1)


# ------------------------------------------------------------------------------------------------- CPU
def test_fixture_conditions():
    g = golden()
    r = suite_np()[0]
    acc0, trip = suite_acc0(), suite_triplet64()
    with np.errstate(invalid="ignore", divide="ignore"):
        for name, x in (("distance_mean", r["distance_mean"]), ("distance_median", r["distance_median"]), ("triplet", trip)):
            fin = x[np.isfinite(x)]
            assert np.unique(fin).size == fin.size, f"{name}: tied values"
            wts = acc0
            pct_key = {"distance_mean": "mean", "distance_median": "median", "triplet": "triplet"}[name]
            assert knot_margin(x, wts, SUITE_PS) > 1e-9, name
            lo_a, hi_a = g["suite_pct_" + pct_key]
            if name != "triplet":
                c = lambda z: -np.log(z + EPS32)  # noqa: E731
                lo, hi = c(lo_a - EPS32), c(hi_a + EPS32)
                u = (c(x.astype(np.float64)) - min(lo, hi)) / abs(hi - lo)
                assert table_margin(u) > 1e-7, name
        for case, prm in PCT_CASES.items():
            value, weight = pct_inputs(**prm)
            assert np.unique(value).size == value.size, case
            assert knot_margin(value, weight, PS) > 1e-9 and knot_margin(value, None, PS) > 1e-9, case
        assert g["pct_heavy_ends"][0] < 0 and 2.1 <= pct_inputs(**PCT_CASES["heavy_ends"])[0].min()      # extrapolated below every value
        assert np.all(np.isnan(g["pct_empty"])) and not np.isnan(g["cmap_empty"]).any()
        turbo0 = g["turbo_lut"][0].astype(np.float64)
        yy, xx = np.meshgrid(np.arange(12), np.arange(21), indexing="ij")
        checker = np.where(((yy % 16) // 8) ^ ((xx % 16) // 8), 1.0, float(np.float32(0.8)))[..., None]
        # heavy_ends: lo < 0, its curve is NaN, nan_to_num makes every normalised value 0: table entry 0 under the matte
        w = pct_inputs(**PCT_CASES["heavy_ends"])[1].astype(np.float64)[..., None]
        assert np.abs(g["cmap_heavy_ends"] - (turbo0 * w + checker * (1 - w))).max() < 1e-15
        assert np.array_equal(g["cmap_empty"], np.broadcast_to(checker, (12, 21, 3)))         # the bare checkerboard
        # the ray_weights panel: unit weights over the whole panel (ties change nothing there), the gray table
        lines = g["suite64_sqrt_ray_weights_lines"]
        n, L = RAYS["n"], len(RAYS["levels"])
        rows = ray_panel_rows(n, L, 2048 // (n * L + 1))
        panel = np.concatenate([lines, np.zeros_like(lines[:1])], 0)[rows]
        # Unit weights: the knots are the whole numbers 1..n, exact in float64 in ANY order of summation, and the float32
        # target comes from the same three IEEE operations everywhere.  The 99.5th percentile of this panel sits ON a knot
        # (float32(99.5 * 3592192 / 100) = 3574231): it compares equal in the reference and in the kernels alike, so the
        # margin is asserted for the weighted inputs above, where rounding can move a knot, and only the size here.
        assert panel.size == 1754 * 2048 < 2 ** 24 * 256 and knot_margin(panel, None, SUITE_PS[:1]) > 1e-9
        lo =g["suite_pct_ray_weights"][0] - EPS32
        assert table_margin((lines - min(lo, 1.0)) / abs(1.0 - lo)) > 1e-7
    for key in ("depth_mean", "depth_median"):
        p = g["suite64_" + key]
        assert np.abs(p - p.reshape(-1, 3).mean(0)).max() > 0.1, key


def test_turbo_table_is_matplotlibs():
    from refnerf_pl_amd import vis, vis_tables
    g = golden()
    lut = np.array(vis_tables.TURBO_BITS, dtype=np.uint32).view(np.float32).reshape(vis_tables.TURBO_N, 3)
    assert lut.tobytes() == np.ascontiguousarray(g["turbo_lut"], np.float32).tobytes()
    assert vis.color_table("turbo", "cpu").numpy().tobytes() == lut.tobytes()
    gray = vis.color_table("gray", "cpu").numpy()
    assert np.array_equal(gray, np.repeat((np.arange(256) / 255.0).astype(np.float32)[:, None], 3, 1))
    try:
        import matplotlib
    except ImportError:
        return
    for name, mine in (("turbo", lut), ("gray", gray)):
        cmap = matplotlib.colormaps[name]
        assert np.array_equal(cmap(np.arange(cmap.N))[:, :3].astype(np.float32), mine), name
        assert np.array_equal(vis.color_table(cmap, "cpu").numpy(), mine)           # a Colormap object, sampled once
    assert vis.color_table(cmap, "cpu") is vis.color_table(cmap, "cpu")


def check_percentile_cases(device, tag):
    from refnerf_pl_amd import vis
    g = golden()
    for case, prm in PCT_CASES.items():
        value, weight = pct_inputs(**prm)
        for f64 in (False, True):
            v, w = torch.from_numpy(value).to(device), torch.from_numpy(weight).to(device)
            if f64:
                v, w = v.double(), w.double()
            got = vis.weighted_percentile(v, w, PS)
            assert got.dtype == torch.float64 and tuple(got.shape) == (len(PS),)
            e = err(npy(got), g["pct_" + case], case, relative=True)
            ones = vis.weighted_percentile(v, torch.ones_like(w), PS)
            null = vis._percentiles(v.reshape(-1), None, PS)                    # the NULL-weights path of the entry
            e1 = max(err(npy(ones), g["pct_unit_" + case], case, relative=True), err(npy(null), g["pct_unit_" + case], case, relative=True))
            print(f"MEASURED {tag} percentiles {case} f64={f64}: weighted {e:.2e}, unit weights {e1:.2e} (bar {BAR64:.0e})")
            assert e <= BAR64 and e1 <= BAR64, (case, e, e1)
            if case in ("heavy_ends", "empty"):
                for colormap in ("turbo", torch.from_numpy(g["turbo_lut"])):
                    panel = vis.visualize_cmap(v, w, colormap, curve_fn=vis.depth_curve_fn)
                    assert panel.dtype == v.dtype
                    ep = err(npy(panel), g["cmap_" + case], case)
                    print(f"MEASURED {tag} visualize_cmap {case} f64={f64}: {ep:.2e}")
                    assert ep <= (BAR64 if f64 else BAR32), (case, ep)
                generic = vis.visualize_cmap(v, w, "turbo", curve_fn=neg_log_curve)      # an unknown curve: applied with ATen
                assert err(npy(generic), g["cmap_" + case], case) <= (BAR64 if f64 else BAR32)


def check_ray_cases(device, tag):
    from refnerf_pl_amd import vis
    g = golden()
    sd, ws, cs = [[torch.from_numpy(z).to(device) for z in lst] for lst in ray_inputs(**RAYS)]
    n, L = RAYS["n"], len(RAYS["levels"])
    for case, prm in RAY_CASES.items():
        for f64 in (False, True):
            cast = (lambda z: z.double()) if f64 else (lambda z: z)
            got, alpha = vis.visualize_rays([cast(z) for z in sd], (0, 1), [cast(z) for z in ws], [cast(z) for z in cs], **prm)
            assert got.dtype == torch.float64 and alpha.dtype == torch.float64
            if case == "untiled":
                e = max(err(npy(got), g["rays_untiled_vis"], case, relative=True), err(npy(alpha), g["rays_untiled_alpha"], case, relative=True))
                print(f"MEASURED {tag} visualize_rays {case} f64={f64}: {e:.2e} (bar {BAR64:.0e})")
                assert e <= BAR64, (case, e)
                continue
            rep = prm["resolution"] // (n * L + 1)
            assert list(got.shape) == list(g[f"rays_{case}_shape"])
            check_ray_panel(got, g[f"rays_{case}_lines"], g[f"rays_{case}_strip"], n, L, rep, f"{tag} visualize_rays {case} f64={f64}", BAR64)
            check_ray_panel(alpha, g[f"rays_{case}_alpha_lines"], np.zeros(()), n, L, rep, f"{tag} visualize_rays {case} alpha f64={f64}", BAR64)


@pytest.mark.parametrize("srgb", [False, True])
def test_aten_path_reproduces_the_suite(srgb):
    from refnerf_pl_amd import vis
    g = golden()
    for f64 in (False, True):
        inputs = suite_torch("cpu", f64)
        out = vis.visualize_suite(inputs[0], inputs[1], srgb)
        check_suite(out, g, srgb, f64, inputs, f"aten srgb={srgb} f64={f64}")


def test_aten_path_reproduces_percentiles_cmaps_and_rays():
    check_percentile_cases("cpu", "aten")
    check_ray_cases("cpu", "aten")


def test_small_helpers_and_refusals():
    from refnerf_pl_amd import vis
    x = torch.tensor([0.3])
    with pytest.raises(ValueError, match="at least two"):
        vis.weighted_percentile(x, torch.ones_like(x), [50.0])
    with pytest.raises(ValueError, match="at least two"):
        vis.visualize_cmap(x[None], torch.ones(1, 1), "turbo")
    with pytest.raises(ValueError, match="3 dims"):
        vis.visualize_cmap(torch.rand(4, 5), torch.rand(4, 5), None)
    with pytest.raises(ValueError, match="colormap"):
        vis.visualize_cmap(torch.rand(4, 5), torch.rand(4, 5), "viridis")
    h = torch.linspace(0, 1, 7, dtype=torch.float64)
    s = vis.sinebow(h)
    assert tuple(s.shape) == (7, 3) and torch.allclose(s.sum(-1), torch.full((7,), 1.5, dtype=torch.float64))
    # matte and visualize_coord_mod against their definitions, on sizes that are no multiple of the checker
    acc = torch.rand(19, 21, dtype=torch.float64)
    img = torch.rand(19, 21, 3, dtype=torch.float64)
    yy, xx = np.meshgrid(np.arange(19), np.arange(21), indexing="ij")
    bg = torch.from_numpy(np.where(((yy % 16) // 8) ^ ((xx % 16) // 8), 1.0, float(np.float32(0.8))))
    want = img * acc[..., None] + (bg * (1 - acc))[..., None]
    assert (vis.matte(img, acc) - want).abs().max() <= 1e-15
    coords = 3 * torch.randn(19, 21, 3, dtype=torch.float64)
    want = torch.remainder(coords + 1, 2) / 2 * acc[..., None] + (bg * (1 - acc))[..., None]
    assert (vis.visualize_coord_mod(coords, acc) - want).abs().max() <= 1e-15
    # modulus wraps instead of scaling; lo = 0 counts as unset (the reference's `lo or ...`), hi = 1 is kept
    v = torch.rand(6, 9, dtype=torch.float64) * 3
    m = vis.visualize_cmap(v, torch.ones_like(v), "gray", modulus=0.5, matte_background=False)
    assert m.dtype == torch.float32 and (m[..., 0].double() - torch.floor(torch.remainder(v, 0.5) / 0.5 * 256).clamp(max=255) / 255).abs().max() < 1e-7
    a = vis.visualize_cmap(v, torch.ones_like(v), "gray", lo=torch.tensor(0), hi=torch.tensor(1), matte_background=False)
    b = vis.visualize_cmap(v, torch.ones_like(v), "gray", lo=None, hi=1.0, matte_background=False)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("srgb", [False, True])
def test_kernel_path_reproduces_the_suite(srgb):
    from refnerf_pl_amd import vis
    g = golden()
    for f64 in (False, True):
        inputs = suite_torch(DEV, f64)
        out = vis.visualize_suite(inputs[0], inputs[1], srgb)
        assert all(v.is_cuda for v in out.values())
        check_suite(out, g, srgb, f64, inputs, f"kernels srgb={srgb} f64={f64}")


@pytest.mark.gpu
def test_kernel_path_reproduces_percentiles_cmaps_and_rays():
    check_percentile_cases(DEV, "kernels")
    check_ray_cases(DEV, "kernels")


@pytest.mark.gpu
def test_c_entries_directly():
    """the entries through _hip alone: the caller's own order, the fixture's percentiles, hand-built lines"""
    from refnerf_pl_amd import _hip
    g = golden()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    for case, prm in PCT_CASES.items():
        value, weight = pct_inputs(**prm)
        order = dev(np.argsort(value.reshape(-1), kind="stable").astype(np.int64))
        got = _hip.vis_weighted_percentile(dev(value.reshape(-1)), dev(weight.reshape(-1)), order, PS)
        null = _hip.vis_weighted_percentile(dev(value.reshape(-1).astype(np.float64)), None, order, PS)
        e = max(err(npy(got), g["pct_" + case], case, relative=True), err(npy(null), g["pct_unit_" + case], case, relative=True))
        print(f"MEASURED entry percentiles {case}: {e:.2e}")
        assert e <= BAR64
    with pytest.raises(ValueError):
        _hip.vis_weighted_percentile(dev(np.ones(1, np.float32)), None, dev(np.zeros(1, np.int64)), PS)
    with pytest.raises(ValueError):
        _hip.vis_weighted_percentile(dev(np.ones(4, np.float32)), None, dev(np.arange(4)), [1.0] * 9)
    bad = _hip.vis_weighted_percentile(dev(np.arange(4, dtype=np.float32)), dev(np.ones(4, np.float32)), dev(np.array([0, 1, 7, -3])), [50.0])
    assert bool(torch.isnan(bad).all())            # not an order of these values: poisoned, nothing read out of bounds
    # the panels from the reference's own percentiles
    r, o, d = suite_np()
    H, W = SUITE["H"], SUITE["W"]
    inputs = dict(rgb=dev(r["rgb"]), acc=dev(r["acc"]), distance_mean=dev(r["distance_mean"]), distance_median=dev(r["distance_median"]),
                  distance_p5=dev(r["distance_percentile_5"]), distance_p95=dev(r["distance_percentile_95"]), origins=dev(o), directions=dev(d),
                  roughness=dev(r["roughness"]), tint=dev(r["tint"]), rgb_cc=dev(r["rgb_cc"]))
    lohi = [dev(g["suite_pct_" + k]) for k in ("mean", "median", "triplet")]
    out = _hip.vis_panels(H, W, torch.float32, False, dev(g["turbo_lut"]), inputs,
                          ["acc_out", "color_matte", "depth_mean", "depth_median", "depth_triplet", "coords_mod", "roughness_out", "tint_matte",
                           "color_corrected"], lohi, [dev(r["normals"])])
    names = dict(acc_out="acc", roughness_out="roughness")
    for k, v in out.items():
        if k == "normals_out":
            k, v = "normals", v[0]
        elif k == "color_corrected":
            assert torch.equal(v, inputs["rgb_cc"])
            continue
        e = err(npy(v), g["suite64_" + names.get(k, k)], k)
        print(f"MEASURED entry panels {k}: {e:.2e}")
        assert e <= BAR32, (k, e)
    # ray lines and the panel
    sd, ws, cs = ray_inputs(**RAYS)
    n, L, res = RAYS["n"], len(RAYS["levels"]), 64
    edges = torch.linspace(0, 1, res + 1, device=DEV).double()
    lv = torch.empty((n, L, res, 3), dtype=torch.float64, device=DEV)
    la = torch.empty((n, L, res), dtype=torch.float64, device=DEV)
    for lvl in range(L):
        _hip.vis_resample_rays(dev(sd[lvl]), dev(cs[lvl]), dev(ws[lvl]), edges, lv, la, lvl)
    vis_panel, alpha = _hip.vis_ray_panel(lv, la, res // (n * L + 1), 0.8)
    check_ray_panel(vis_panel, g["rays_plain_lines"], g["rays_plain_strip"], n, L, res // (n * L + 1), "entry ray panel", BAR64)
    check_ray_panel(alpha, g["rays_plain_alpha_lines"], np.zeros(()), n, L, res // (n * L + 1), "entry ray alpha", BAR64)


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal():
    from refnerf_pl_amd import vis
    inputs = suite_torch(DEV, False)
    a = vis.visualize_suite(inputs[0], inputs[1], True)
    b = vis.visualize_suite(inputs[0], inputs[1], True)
    for k in a:
        assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), k
        assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])), k


@pytest.mark.gpu
def test_suite_never_synchronises():
    from refnerf_pl_amd import vis
    inputs = suite_torch(DEV, False)
    vis.visualize_suite(inputs[0], inputs[1], True)                      # warm-up: code objects, the tables, the allocator's pool
    torch.cuda.synchronize()
    probe = torch.ones(4, device=DEV)
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.sum().item()
            tripped = False
        except RuntimeError:
            tripped = True
        finally:
            torch.cuda.set_sync_debug_mode("default")
    except (RuntimeError, AttributeError):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available in this build")
    if not tripped:
        pytest.skip("this build's sync debug mode does not flag .item(): nothing can be shown with it")
    torch.cuda.set_sync_debug_mode("error")                              # any synchronising torch call raises
    try:
        out = vis.visualize_suite(inputs[0], inputs[1], True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(v.is_cuda for v in out.values())


@pytest.mark.gpu
def test_full_size_view_is_finite():
    from refnerf_pl_amd import vis
    H = W = 800
    gen = torch.Generator(device=DEV).manual_seed(3)
    rnd = lambda *s: torch.rand(*s, device=DEV, generator=gen)  # noqa: E731
    dist = 2 + 4 * rnd(H, W)
    nan = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    nan[5, 7] = nan[799, 799] = True
    dist = torch.where(nan, torch.full_like(dist, float("nan")), dist)
    rendering = dict(rgb=rnd(H, W, 3), acc=rnd(H, W), distance_mean=dist, distance_median=dist + 0.01, distance_percentile_5=dist - 0.2,
                     distance_percentile_95=dist + 0.2, normals=rnd(H, W, 3) - 0.5, roughness=rnd(H, W, 1), diffuse=rnd(H, W, 3),
                     specular=rnd(H, W, 3), tint=rnd(H, W, 3))
    sd, ws, cs = [], [], []
    for N in (64, 64, 32):
        s = torch.sort(rnd(16, N + 1), -1).values
        sd.append(s)
        ws.append(rnd(16, N) / N)
        cs.append(rnd(16, N, 3))
    rendering.update(ray_sdist=sd, ray_weights=ws, ray_rgbs=cs)
    rays = types.SimpleNamespace(origins=rnd(H, W, 3), directions=rnd(H, W, 3) - 0.5)
    out = vis.visualize_suite(rendering, rays, True)
    torch.cuda.synchronize()
    for k, v in out.items():
        if v.dim() >= 2 and tuple(v.shape[:2]) == (H, W) and k == "coords_mod":
            assert bool(torch.isnan(v[nan]).all()) and bool(torch.isfinite(v[~nan]).all()), k     # NaN * 0, as in the reference
        else:
            assert bool(torch.isfinite(v).all()), k
    assert tuple(out["ray_colors"].shape) == (16 * (3 * (2048 // 49) + 1) - 1, 2048, 3)

#!/usr/bin/env python3
"""Capture the visualisation vectors from the upstream reference (build container only).

Run:  python tests/golden/make_golden_vis.py
Needs the reference checkout (see _ref_harness.py) and matplotlib.  Writes tests/golden/vis_suite.npz: recipe parameters and
the reference's outputs, arrays only.  The inputs are NOT stored: tests/test_vis.py regenerates them from the seeded recipes
this script imports from it.  Every input is float32-representable and is fed to the reference as float64 (the truth); the
suite is also run on the float32 inputs themselves.

  params                                the recipes' parameters (JSON); turbo_lut: matplotlib's 256 x 3 table, float32
  pct_<case>, pct_unit_<case>           vis.weighted_percentile with the case's weights / with unit weights
  cmap_heavy_ends, cmap_empty           vis.visualize_cmap(value, weight, turbo, curve_fn = -log(x + eps))
  rays_<case>_lines / _alpha_lines / _strip / _shape   vis.visualize_rays at resolution 64: the distinct lines of the panel
                                        (checked here to BE the panel, row by row); rays_untiled_vis / _alpha at resolution 3
  suite_meta                            keys, dtypes and shapes of visualize_suite's float64 and float32 runs (JSON)
  suite_pct_{mean,median,triplet,ray_weights}   the weighted percentiles visualize_suite's colour maps take their bounds from
  suite64_<key>, suite64_srgb_<key>     the float64 run's panels (linear_to_srgb False; the panels True changes); panels the
                                        reference returns as its own input are left out
  suite64_ray_*_lines / _strip          the distinct lines of the two ray panels; suite64_sqrt_ray_weights_lines: the values
                                        the ray_weights colour map is applied to
  suite32_<key>_ulps, suite32_srgb_<key>_ulps   the float32 run, as float32 steps from the rounded float64 truth (lossless)
  suite32_ray_colors_lines              the float32 run's ray_colors lines (float64, as the reference returns them)

Two names the installed libraries no longer provide are supplied at run time, nothing of the reference is changed or
copied: matplotlib 3.10 has no cm.get_cmap, and torch.max(float, Tensor), which visualize_rays(renormalize=True) calls,
is not an overload of torch.max (the float is wrapped in a tensor).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import _ref_harness  # noqa: E402

_ref_harness.install()

import matplotlib  # noqa: E402
from matplotlib import cm  # noqa: E402

cm.get_cmap = lambda n: matplotlib.colormaps[n]

import test_vis as T  # noqa: E402  (the recipes)

_torch_max = torch.max


def _max(a, *rest, **kw):
    return _torch_max(torch.tensor(a) if isinstance(a, float) else a, *rest, **kw)


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


def distinct_lines(panel, n, L, rep):
    """(lines [n L, ...], strip [...]) of a visualize_rays panel; asserts that the panel is nothing but these rows"""
    rows = T.ray_panel_rows(n, L, rep)
    first = np.array([int(np.argmax(rows == k)) for k in range(n * L + 1)])
    lines, strip = panel[first[:-1]], panel[first[-1]]
    ext = np.concatenate([lines, strip[None]], 0)
    assert panel.shape[0] == rows.size and np.array_equal(ext[rows], panel, equal_nan=True)
    assert np.all(strip == strip.reshape(-1, *strip.shape[1:])[0])        # the strip is one colour
    return lines, strip[0]


def main():
    from internal import vis
    out = {"params": np.array(json.dumps(T.PARAMS))}
    turbo = matplotlib.colormaps["turbo"]
    out["turbo_lut"] = np.ascontiguousarray(turbo(np.arange(turbo.N))[:, :3], np.float32)

    # ---- percentiles and the two colour-map cases
    for case, prm in T.PCT_CASES.items():
        value, weight = T.pct_inputs(**prm)
        assert np.unique(value).size == value.size, case
        assert T.knot_margin(value, weight, T.PS) > 1e-9 and T.knot_margin(value, None, T.PS) > 1e-9, case
        out["pct_" + case] = vis.weighted_percentile(t64(value), t64(weight), T.PS).numpy()
        out["pct_unit_" + case] = vis.weighted_percentile(t64(value), torch.ones_like(t64(weight)), T.PS).numpy()
        assert out["pct_" + case].dtype == np.float64
        print(case, out["pct_" + case], out["pct_unit_" + case])
        if case in ("heavy_ends", "empty"):
            out["cmap_" + case] = vis.visualize_cmap(t64(value), t64(weight), cm.get_cmap("turbo"), curve_fn=T.neg_log_curve).numpy()
            assert out["cmap_" + case].dtype == np.float64
    assert out["pct_heavy_ends"][0] < 0 and np.all(np.isnan(out["pct_empty"]))

    # ---- visualize_rays directly
    sd, ws, cs = T.ray_inputs(**T.RAYS)
    n, L = T.RAYS["n"], len(T.RAYS["levels"])
    for case, prm in T.RAY_CASES.items():
        torch.max = _max
        try:
            v, a = vis.visualize_rays([t64(z) for z in sd], (0, 1), [t64(z) for z in ws], [t64(z) for z in cs], **prm)
        finally:
            torch.max = _torch_max
        v, a = v.numpy(), a.numpy()
        assert v.dtype == np.float64 and a.dtype == np.float64
        if case == "untiled":
            out["rays_untiled_vis"], out["rays_untiled_alpha"] = v, a
            continue
        rep = prm["resolution"] // (n * L + 1)
        out[f"rays_{case}_shape"] = np.array(v.shape)
        out[f"rays_{case}_lines"], out[f"rays_{case}_strip"] = distinct_lines(v, n, L, rep)
        out[f"rays_{case}_alpha_lines"], strip_a = distinct_lines(a, n, L, rep)
        assert strip_a == 0
        print("rays", case, v.shape, "alpha max %.4f" % a.max(), "min colour %.3f max %.3f" % (v.min(), v.max()))

    # ---- the suite
    r, o, d = T.suite_np()
    acc0, trip = T.suite_acc0(), T.suite_triplet64()
    for name, x in (("mean", r["distance_mean"]), ("median", r["distance_median"]), ("triplet", trip)):
        fin = x[np.isfinite(x)]
        assert np.unique(fin).size == fin.size and T.knot_margin(x, acc0, T.SUITE_PS) > 1e-9, name
        out["suite_pct_" + name] = vis.weighted_percentile(t64(x), t64(acc0), T.SUITE_PS).numpy()
    meta = {}
    runs = {}
    for f64 in (True, False):
        for srgb in (False, True):
            rendering, rays = T.suite_torch("cpu", f64)
            res = vis.visualize_suite(rendering, rays, srgb)
            runs[(f64, srgb)] = res
            this = [[k, str(v.dtype), list(v.shape)] for k, v in res.items()]
            assert meta.setdefault("f64" if f64 else "f32", this) == this
            for key, src in T.PASSTHROUGH.items():
                if not (srgb and key in T.SRGB_KEYS):
                    assert res[key] is rendering[src], key
    out["suite_meta"] = np.array(json.dumps(meta))
    print(meta["f32"])
    rep = 2048 // (n * L + 1)
    for srgb in (False, True):
        r64, r32 = runs[(True, srgb)], runs[(False, srgb)]
        for key, v in r64.items():
            if key in ("ray_colors", "ray_weights") or (key in T.PASSTHROUGH and not (srgb and key in T.SRGB_KEYS)):
                continue
            if srgb and key not in T.SRGB_KEYS:
                assert np.array_equal(v.numpy(), out["suite64_" + key], equal_nan=True), key
                continue
            pre = "srgb_" if srgb else ""
            truth = v.numpy()
            assert truth.dtype == np.float64
            out[f"suite64_{pre}{key}"] = truth
            run32 = r32[key].numpy()
            assert run32.dtype == np.float32 and np.array_equal(np.isnan(run32), np.isnan(truth)), key
            out[f"suite32_{pre}{key}_ulps"] = T.ulps_encode(run32, truth)
            assert np.array_equal(T.ulps_decode(out[f"suite32_{pre}{key}_ulps"], truth), run32, equal_nan=True), key
            print("%-16s srgb=%d  |f32 run - f64 run| = %.2e" % (key, srgb, np.nanmax(np.abs(run32.astype(np.float64) - truth))))
    r64, r32 = runs[(True, False)], runs[(False, False)]
    out["suite64_ray_colors_lines"], out["suite64_ray_colors_strip"] = distinct_lines(r64["ray_colors"].numpy(), n, L, rep)
    out["suite32_ray_colors_lines"], strip32 = distinct_lines(r32["ray_colors"].numpy(), n, L, rep)
    assert np.array_equal(strip32, out["suite64_ray_colors_strip"])
    print("ray_colors |f32 run - f64 run| = %.2e" % np.abs(out["suite32_ray_colors_lines"] - out["suite64_ray_colors_lines"]).max())
    out["suite64_ray_weights_lines"], out["suite64_ray_weights_strip"] = distinct_lines(r64["ray_weights"].numpy(), n, L, rep)
    assert out["suite64_ray_weights_lines"].dtype == np.float32 and list(out["suite64_ray_weights_strip"]) == [1.0, 0.0, 0.0]
    # the values under the ray_weights colour map, and its automatic lower bound: visualize_suite's own calls again
    sq, _ = vis.visualize_rays([t64(z) for z in sd], (0, 1), [torch.ones_like(t64(z)) for z in ws], [torch.sqrt(t64(z))[..., None] for z in ws],
                               bg_color=0)
    sq = sq[..., 0]
    out["suite64_sqrt_ray_weights_lines"], _ = distinct_lines(sq.numpy(), n, L, rep)
    out["suite_pct_ray_weights"] = vis.weighted_percentile(sq, torch.ones_like(sq), T.SUITE_PS).numpy()
    out["suite_ray_shape"] = np.array(r64["ray_colors"].shape)

    path = os.path.join(HERE, "vis_suite.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 1000 * 1000
    T.golden.cache_clear()
    T.test_fixture_conditions()


if __name__ == "__main__":
    main()

"""Config.hip_fused_losses beyond the shipped loss set: the data term with either penalty ('mse' / 'charb'), the linear-rgb
target and the disparity / normal statistics of compute_data_loss (train_utils.py:33-88) through refnerf_data_terms_forward /
_backward, and compute_depth_smoothness_loss (:90-119) of a [P, S, S, .] patch batch through refnerf_depth_smoothness_forward /
_backward.

CPU test: the ATen functions against the reference's own values (tests/golden/data_terms.npz).  GPU tests: the kernels
against the ATen functions evaluated on the same inputs in float64 (column sums, values, gradients), the fused path on the
reference's vectors, the whole step with the flag off and on (flat and 2 x 2 patch batches), the routing, no host
synchronisation, and the argument checks of the four entries.

Bar of a fused fp32 value / gradient (relative; gradients rel-L2) against float64: the larger of 2e-6 (the bar of
test_fused_refnerf_losses_match_train_utils and test_fused_regularisers.py) and twice the fp32 ATen path's own distance from
float64 (the factor DESIGN.md section 4 gives the exact-fp32 kernels).
"""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import torch

from helpers import load_golden, params_from_golden, rays_from_golden

GIN = os.path.join(os.path.dirname(__file__), "..", "configs", "refnerf_blender.gin")
DEV = "cuda:0"
PENALTIES = ("mse", "charb")
STAT_KEYS = ("mses", "disparity_mses", "normal_maes")
UPSTREAM = 0.37                                    # a non-unit upstream gradient
ENTRIES = ("refnerf_data_terms_forward", "refnerf_data_terms_backward", "refnerf_depth_smoothness_forward",
           "refnerf_depth_smoothness_backward")


def _rel(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def _bar(aten32, ref64):
    """the larger of 2e-6 and twice the fp32 ATen path's own distance from float64"""
    return max(2e-6, 2.0 * _rel(aten32, ref64))


def _no_regularisers(cfg):
    cfg.orientation_loss_mult = cfg.orientation_coarse_loss_mult = 0.0
    cfg.predicted_normal_loss_mult = cfg.predicted_normal_coarse_loss_mult = 0.0
    return cfg


def _parse(bindings):
    from refnerf_pl_amd import configs
    configs.clear_config()
    configs.parse_config_files_and_bindings([GIN], [str(b) for b in bindings if str(b)])
    cfg = configs.Config()
    configs.clear_config()
    return cfg


def _rays_of(lossmult, device):
    return types.SimpleNamespace(lossmult=torch.as_tensor(lossmult, device=device), viewdirs=torch.zeros(lossmult.shape[:-1] + (3,), device=device))


# ------------------------------------------------------------------------------------------- the reference's vectors
def _golden_data_case(g, case, device, dtype=torch.float32):
    """(cfg, batch, rays, renderings with rgb as leaves) of one compute_data_loss case of data_terms.npz"""
    from refnerf_pl_amd import utils
    penalty, colour, normals = case.split("_")
    cfg = _no_regularisers(_parse(list(g["data_bindings"]) + [f"Config.data_loss_type = '{penalty}'",
                                                              f"Config.supervised_by_linear_rgb = {colour == 'linear'}"]))
    rays = _rays_of(g["data_lossmult"], device)
    batch = utils.Batch(rays=rays, rgb=g["data_gt_rgb"], disps=torch.tensor(g["data_disps"], device=device, dtype=dtype),
                        normals=g["data_normals_gt"], alphas=g["data_alphas"])
    rend = []
    for lvl in range(2):
        keys = ("rgb", "acc", "distance_mean") + (("normals",) if normals == "normals" else ())
        rend.append({k: torch.tensor(g[f"data_L{lvl}_{k}"], device=device, dtype=dtype) for k in keys})
        rend[-1]["rgb"].requires_grad_(True)
    return cfg, batch, rays, rend


def _golden_smooth(g, device):
    cfg = _parse(g["smooth_bindings"])
    rend = [{k: torch.tensor(g[f"smooth_L{lvl}_{k}"], device=device) for k in ("distance", "acc", "rgb")} for lvl in range(2)]
    for r in rend:
        r["distance"].requires_grad_(True)
    return cfg, rend


def _check_golden_data(g, case, loss, stats, rend, tol):
    assert float(loss.detach()) == pytest.approx(float(g[case + "_loss"]), rel=tol), case
    assert tuple(stats) == tuple(str(k) for k in g[case + "_stat_keys"]) == STAT_KEYS, case
    for k, v in stats.items():
        np.testing.assert_allclose(v.detach().cpu().numpy(), g[f"{case}_stat_{k}"], rtol=tol, atol=0, equal_nan=True, err_msg=f"{case} {k}")
    for lvl, r in enumerate(rend):
        rel = _rel(r["rgb"].grad.cpu().numpy(), g[f"{case}_g_rgb_L{lvl}"])
        print(f"{case} L{lvl}: d loss / d rgb rel-L2 {rel:.2e}")
        assert rel < tol, (case, lvl, rel)


def test_aten_losses_match_the_reference():
    """The unfused compute_data_loss (both penalties, both targets, both statistics, with and without 'normals') and
    compute_depth_smoothness_loss against the reference's own loss, stats and autograd gradients at 2e-6."""
    from refnerf_pl_amd import train_utils
    g = load_golden("data_terms")
    assert len(g["data_cases"]) == 8
    for case in (str(c) for c in g["data_cases"]):
        cfg, batch, rays, rend = _golden_data_case(g, case, "cpu")
        loss, stats = train_utils.compute_data_loss(batch, rend, rays, cfg)
        loss.backward()
        _check_golden_data(g, case, loss, stats, rend, 2e-6)
        assert np.isnan(g[case + "_stat_normal_maes"]).all() == case.endswith("nonormals")
    cfg, rend = _golden_smooth(g, "cpu")
    assert cfg.depth_smoothness_coarse_loss_mult > 0 and cfg.depth_smoothness_loss_mult > 0
    loss = train_utils.compute_depth_smoothness_loss(rend, cfg)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(g["smooth_loss"]), rel=2e-6)
    for lvl, r in enumerate(rend):
        assert _rel(r["distance"].grad.numpy(), g[f"smooth_g_distance_L{lvl}"]) < 2e-6, lvl
        assert np.all(g[f"smooth_g_distance_L{lvl}"][[1, 3]] == 0.0)       # the acc = 0 patch and the constant-depth patch


@pytest.mark.gpu
def test_fused_path_matches_the_reference():
    """The fused data term and depth smoothness on data_terms.npz, and the fused data term on normal_metrics.npz: loss and
    stats at rel 1e-5 (the bar test_fused_refnerf_losses_match_train_utils uses against loss_data), gradients at rel-L2
    1e-5, the stats keys in the reference's order, normal_maes NaN where the renderings carry no normals."""
    from refnerf_pl_amd import _hip, train_utils, utils
    _hip.require_device()
    model = types.SimpleNamespace(num_levels=2)
    hist = [{"weights": torch.zeros((1, 1), device=DEV)}] * 2
    g = load_golden("data_terms")
    for case in (str(c) for c in g["data_cases"]):
        cfg, batch, rays, rend = _golden_data_case(g, case, DEV)
        loss, stats, o_loss, n_loss = train_utils.fused_refnerf_losses(model, batch, rays, rend, hist, cfg)
        assert o_loss is None and n_loss is None
        loss.backward()
        _check_golden_data(g, case, loss, stats, rend, 1e-5)
    cfg, rend = _golden_smooth(g, DEV)
    assert train_utils.fused_depth_smoothness_supported(rend)
    loss = train_utils.fused_depth_smoothness_loss(rend, cfg)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(g["smooth_loss"]), rel=1e-5)
    for lvl, r in enumerate(rend):
        grad = r["distance"].grad.cpu().numpy()
        assert grad.shape == g[f"smooth_g_distance_L{lvl}"].shape
        assert _rel(grad, g[f"smooth_g_distance_L{lvl}"]) < 1e-5, lvl
        assert np.all(grad[[1, 3]] == 0.0)

    g = load_golden("normal_metrics")
    cfg = _no_regularisers(_parse(["Config.compute_normal_metrics = True", "Config.compute_disp_metrics = True"]))
    rays = utils.rays_from_dict(rays_from_golden(g), DEV)
    for tag in ("train", "eval"):
        rend = [{k: torch.tensor(g[f"{tag}_L{lvl}_{k}"], device=DEV) for k in ("rgb", "acc", "distance_mean", "normals")
                 if f"{tag}_L{lvl}_{k}" in g.files} for lvl in range(2)]
        batch = utils.Batch(rays=rays, rgb=g[tag + "_gt_rgb"], disps=g[tag + "_disps"], normals=g[tag + "_normals"], alphas=g[tag + "_alphas"])
        loss, stats, _, _ = train_utils.fused_refnerf_losses(model, batch, rays, rend, hist, cfg)
        assert float(loss) == pytest.approx(float(g[tag + "_loss"]), rel=1e-5)
        assert tuple(stats) == STAT_KEYS
        for k, v in stats.items():
            np.testing.assert_allclose(v.cpu().numpy(), g[f"{tag}_stat_{k}"], rtol=1e-5, atol=0, equal_nan=True, err_msg=f"{tag} {k}")
    assert np.isnan(stats["normal_maes"].cpu().numpy()).all()              # the eval case: no 'normals'


# ------------------------------------------------------------------------------------------- GPU: the kernels, stage by stage
def _data_arrays(R):
    """uniform O(1) renderings-like arrays (float32), a non-uniform lossmult, normals from randn (angles near 0 or pi,
    where acos is ill-conditioned, are rare)"""
    rng = np.random.default_rng(500 + R)
    f = lambda *shape: rng.random(shape).astype(np.float32)     # noqa: E731
    return dict(rgb=f(R, 3), gt=f(R, 3), lossmult=(0.25 + 1.5 * f(R, 1)).astype(np.float32),
                distance_mean=(2 + 4 * f(R)).astype(np.float32), disps=f(R), acc=f(R), alphas=f(R),
                normals=rng.standard_normal((R, 3)).astype(np.float32), normals_gt=rng.standard_normal((R, 3)).astype(np.float32))


def _stage_cfg(penalty, groups):
    from refnerf_pl_amd import configs
    configs.clear_config()
    return configs.Config(data_loss_type=penalty, charb_padding=0.001, data_loss_mult=1.7, data_coarse_loss_mult=0.4,
                          compute_disp_metrics=groups, compute_normal_metrics=groups)


def _aten_data(a, penalty, groups, dtype):
    """Column sums, d (UPSTREAM x column 1) / d rgb, and compute_data_loss's loss, stats and d loss / d rgb, from the ATen
    functions of train_utils on the CPU in `dtype`."""
    from refnerf_pl_amd import train_utils, utils
    cfg = _stage_cfg(penalty, groups)
    t = {k: torch.tensor(v, dtype=dtype) for k, v in a.items()}
    rgb = t["rgb"].clone().requires_grad_(True)
    sq = (rgb - t["gt"]) ** 2
    cols = [(t["lossmult"] * sq).sum(), (t["lossmult"] * train_utils._pixel_penalty(sq, cfg)).sum()]
    if groups:
        w = t["acc"] * t["alphas"]
        lim = 1 - torch.finfo(torch.float32).eps
        cos = (train_utils._l2_normalize(t["normals"]) * train_utils._l2_normalize(t["normals_gt"])).sum(-1)
        cols += [((1 / (1 + t["distance_mean"]) - t["disps"]) ** 2).sum(), (w * torch.arccos(torch.clip(cos, -lim, lim))).sum(), w.sum()]
    else:
        cols += [torch.zeros((), dtype=dtype)] * 3
    (UPSTREAM * cols[1]).backward()
    res = dict(cols=np.array([float(c.detach()) for c in cols]), g_cols=rgb.grad.numpy().copy())
    rgb2 = t["rgb"].clone().requires_grad_(True)
    rend = [dict(rgb=rgb2, acc=t["acc"], distance_mean=t["distance_mean"], normals=t["normals"])]
    rays = _rays_of(a["lossmult"], "cpu")
    batch = utils.Batch(rays=rays, rgb=a["gt"], disps=t["disps"], normals=a["normals_gt"], alphas=a["alphas"])
    loss, stats = train_utils.compute_data_loss(batch, rend, rays, cfg)
    loss.backward()
    res.update(loss=float(loss.detach()), stats={k: float(v[0]) for k, v in stats.items()}, g_loss=rgb2.grad.numpy().copy())
    return res


def _fused_data(a, penalty, groups):
    from refnerf_pl_amd import _hip, train_utils, utils
    _hip.require_device()
    cfg = _stage_cfg(penalty, groups)
    t = {k: torch.tensor(v, device=DEV) for k, v in a.items()}
    lm = t["lossmult"].reshape(-1).contiguous()
    opt = {k: t[k] for k in ("distance_mean", "disps", "acc", "alphas", "normals", "normals_gt")} if groups else {}
    A = _hip.data_terms_args(t["rgb"], t["gt"], lm, penalty, cfg.charb_padding, **opt)
    terms = _hip.data_terms_forward(A, t["rgb"].device)
    assert terms.shape == (a["rgb"].shape[0], 5)
    up = torch.full((1,), UPSTREAM, device=DEV)
    res = dict(cols=terms.double().sum(dim=0).cpu().numpy(), cols32=terms.sum(dim=0).cpu().numpy(),
               g_cols=_hip.data_terms_backward(A, up).cpu().numpy(), rows=terms.cpu().numpy())
    rgb2 = t["rgb"].clone().requires_grad_(True)
    rend = [dict(rgb=rgb2, acc=t["acc"], distance_mean=t["distance_mean"], normals=t["normals"])]
    rays = _rays_of(a["lossmult"], DEV)
    batch = utils.Batch(rays=rays, rgb=a["gt"], disps=t["disps"], normals=a["normals_gt"], alphas=a["alphas"])
    # ('mse' without statistics rides in the node of the two regularisers, which reads the ray history: N = 3 samples)
    R = a["rgb"].shape[0]
    hist = [{"weights": torch.zeros((R, 3), device=DEV), "normals_pred": torch.zeros((R, 3, 3), device=DEV), "normals": None}]
    loss, stats, _, _ = train_utils.fused_refnerf_losses(types.SimpleNamespace(num_levels=1), batch, rays, rend, hist, cfg)
    loss.backward()
    res.update(loss=float(loss.detach()), stats={k: float(v[0]) for k, v in stats.items()}, g_loss=rgb2.grad.cpu().numpy())
    return res


@functools.lru_cache(maxsize=None)
def _data_case(R, penalty, groups):
    a = _data_arrays(R)
    return _fused_data(a, penalty, groups), _aten_data(a, penalty, groups, torch.float64), _aten_data(a, penalty, groups, torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [True, False])
@pytest.mark.parametrize("penalty", PENALTIES)
@pytest.mark.parametrize("R", [1, 5, 64, 257])
def test_data_terms_stage_matches_f64(R, penalty, groups):
    """Every column sum of refnerf_data_terms_forward, d_g_rgb with a non-unit device upstream, and the normalised loss,
    stats and gradient of the autograd node, against the ATen functions in float64 (R = 257: a second, partial block)."""
    fused, ref, aten32 = _data_case(R, penalty, groups)
    for j in range(5):
        if not groups and j >= 2:
            assert np.all(fused["rows"][:, j] == 0.0) and ref["cols"][j] == 0.0       # an absent group leaves its columns 0
            continue
        for name, cols in (("column sum in double", fused["cols"]), ("column sum", fused["cols32"])):
            rel, bar = abs(cols[j] - ref["cols"][j]) / abs(ref["cols"][j]), _bar(aten32["cols"][j], ref["cols"][j])
            print(f"R={R} {penalty} groups={groups} {name} {j}: fused {cols[j]:.9g}  f64 {ref['cols'][j]:.9g}  rel {rel:.2e}  bar {bar:.2e}")
            assert rel <= bar, (j, name, rel, bar)
    if penalty == "mse":
        assert np.array_equal(fused["rows"][:, 0], fused["rows"][:, 1])
    for k in ("g_cols", "g_loss"):
        rel, bar = _rel(fused[k], ref[k]), _bar(aten32[k], ref[k])
        print(f"R={R} {penalty} groups={groups} {k}: rel-L2 {rel:.2e}  bar {bar:.2e}")
        assert fused[k].shape == ref[k].shape and rel <= bar, (k, rel, bar)
    rel, bar = abs(fused["loss"] - ref["loss"]) / abs(ref["loss"]), _bar(aten32["loss"], ref["loss"])
    print(f"R={R} {penalty} groups={groups} loss: fused {fused['loss']:.9g}  f64 {ref['loss']:.9g}  rel {rel:.2e}  bar {bar:.2e}")
    assert rel <= bar
    assert tuple(fused["stats"]) == tuple(ref["stats"]) == (STAT_KEYS if groups else STAT_KEYS[:1])
    for k, v in ref["stats"].items():
        rel, bar = abs(fused["stats"][k] - v) / abs(v), _bar(aten32["stats"][k], v)
        print(f"R={R} {penalty} groups={groups} stats[{k}]: fused {fused['stats'][k]:.9g}  f64 {v:.9g}  rel {rel:.2e}  bar {bar:.2e}")
        assert rel <= bar, (k, rel, bar)


def _smooth_arrays(P, S):
    rng = np.random.default_rng(900 + 10 * P + S)
    f = lambda *shape: rng.random(shape).astype(np.float32)     # noqa: E731
    distance, acc, rgb = (2 + 4 * f(P, S, S, 1)).astype(np.float32), f(P, S, S), f(P, S, S, 3)
    if P >= 3:
        acc[1] = 0.0                           # a patch that hit nothing
        distance[2] = distance[2, 0, 0]        # a patch of constant depth
    return distance, acc, rgb


def _smooth_cfg(S):
    from refnerf_pl_amd import configs
    configs.clear_config()
    return configs.Config(patch_size=S, depth_smoothness_loss_mult=1.3, depth_smoothness_coarse_loss_mult=0.3)


def _run_smooth(P, S, fused, dtype=torch.float32):
    from refnerf_pl_amd import train_utils
    distance, acc, rgb = _smooth_arrays(P, S)
    kw = dict(device=DEV if fused else "cpu", dtype=dtype)
    rend = [dict(distance=torch.tensor(distance, **kw).requires_grad_(True), acc=torch.tensor(acc, **kw), rgb=torch.tensor(rgb, **kw))]
    if fused:
        assert train_utils.fused_depth_smoothness_supported(rend)
        loss = train_utils.fused_depth_smoothness_loss(rend, _smooth_cfg(S))
    else:
        loss = train_utils.compute_depth_smoothness_loss(rend, _smooth_cfg(S))
    (UPSTREAM * loss).backward()
    return float(loss.detach()), rend[0]["distance"].grad.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("P,S", [(1, 2), (3, 3), (130, 8)])
def test_depth_smoothness_stage_matches_f64(P, S):
    """Loss and d_g_distance (non-unit upstream) against float64 autograd of compute_depth_smoothness_loss: one cell; a
    partial block of waves; 33 blocks of patches and a lane loop of 49 cells.  The acc = 0 patch and the constant-depth
    patch get exactly zero gradients."""
    (loss, grad), (ref, ref_grad), (l32, g32) = _run_smooth(P, S, True), _run_smooth(P, S, False, torch.float64), _run_smooth(P, S, False)
    rel, bar = abs(loss - ref) / abs(ref), _bar(l32, ref)
    print(f"P={P} S={S} loss: fused {loss:.9g}  f64 {ref:.9g}  rel {rel:.2e}  bar {bar:.2e}")
    assert rel <= bar
    rel, bar = _rel(grad, ref_grad), _bar(g32, ref_grad)
    print(f"P={P} S={S} d/d distance: rel-L2 {rel:.2e}  bar {bar:.2e}")
    assert grad.shape == ref_grad.shape == (P, S, S, 1) and rel <= bar
    if P >= 3:
        assert np.all(grad[1:3] == 0.0) and np.all(ref_grad[1:3] == 0.0)
        assert np.all(np.abs(grad[0]).sum() > 0.0)


# ------------------------------------------------------------------------------------------- GPU: the whole step
def _hip_losses(extra, fused, patches):
    """compute_losses on model_blender_sharp_train + backward to the parameters, as test_fused_refnerf_losses_match_train_utils"""
    import dataclasses
    from refnerf_pl_amd import _hip, configs, layout, models, train_utils, utils
    _hip.require_device()
    g = load_golden("model_blender_sharp_train")
    configs.clear_config()
    configs.parse_config_files_and_bindings([GIN], [str(b) for b in g["bindings"] if str(b)] + list(extra) + [f"Config.hip_fused_losses = {fused}"])
    cfg = configs.Config()
    model = models.construct_model(utils.dummy_rays(), cfg).to(DEV).train()
    model.nerf_mlp.load_flat_params(params_from_golden(g))
    rays = utils.rays_from_dict(rays_from_golden(g), DEV)
    gt = np.asarray(g["gt_rgb"], np.float32)
    if patches:
        rays = dataclasses.replace(rays, **{f.name: getattr(rays, f.name).reshape((-1, 2, 2) + getattr(rays, f.name).shape[1:])
                                            for f in dataclasses.fields(rays)})
        gt = gt.reshape(-1, 2, 2, 3)
    batch = utils.Batch(rays=rays, rgb=gt)
    renderings, history = model(rays, 1.0, False)
    total, terms, stats = train_utils.compute_losses(model, batch, rays, renderings, history, cfg)
    total.backward()
    flat = torch.zeros(layout.NUM_PARAMS)
    for spec, lin in model.nerf_mlp._named_linears():
        flat[spec.w_off:spec.w_off + spec.out_dim * spec.in_dim] = lin.weight.grad.reshape(-1).cpu()
        flat[spec.b_off:spec.b_off + spec.out_dim] = lin.bias.grad.cpu()
    configs.clear_config()
    return float(total.detach()), {k: float(v.detach()) for k, v in terms.items()}, stats["mses"].cpu().numpy(), flat.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("patches", [False, True])
def test_charb_step_fused_matches_unfused(patches):
    """compute_losses on model_blender_sharp_train with Config.data_loss_type = 'charb', Config.hip_fused_losses off and on:
    terms, total (2e-6) and parameter gradient (rel-L2 < 2e-6) as test_fused_refnerf_losses_match_train_utils checks them;
    then with the rays as 2 x 2 patches and depth smoothness on: the same keys in the same order, the same bars."""
    extra = ["Config.data_loss_type = 'charb'"]
    if patches:
        extra += ["Config.patch_size = 2", "Config.depth_smoothness_loss_mult = 0.5", "Config.depth_smoothness_coarse_loss_mult = 0.1"]
    (t0, terms0, mses0, g0), (t1, terms1, mses1, g1) = _hip_losses(extra, False, patches), _hip_losses(extra, True, patches)
    assert tuple(terms0) == tuple(terms1) == ("data", "orientation", "predicted_normals") + (("smoothness",) if patches else ())
    for k in terms0:
        print(f"patches={patches} {k}: fused {terms1[k]:.9g}  unfused {terms0[k]:.9g}")
    rel = np.linalg.norm(g1 - g0) / np.linalg.norm(g0)
    print(f"patches={patches}: total {t1:.8f} / {t0:.8f}, gradient rel-L2 {rel:.2e}")
    assert t1 == pytest.approx(t0, rel=2e-6)
    for k in terms0:
        assert terms1[k] == pytest.approx(terms0[k], rel=2e-6, abs=1e-12), k
    np.testing.assert_allclose(mses1, mses0, rtol=2e-6)
    assert rel < 2e-6, rel


def _synthetic_step(P, S, seed=0):
    """patch-shaped device renderings of two levels as leaves, batch and rays, for compute_losses without a model"""
    from refnerf_pl_amd import utils
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def rand(*shape):
        return torch.rand(shape, device=DEV, generator=gen)

    def randn(*shape):
        return torch.randn(shape, device=DEV, generator=gen)
    lead = (P, S, S)
    rend = [dict(rgb=rand(*lead, 3), acc=rand(*lead), distance=2 + 4 * rand(*lead, 1), distance_mean=2 + 4 * rand(*lead),
                 normals=randn(*lead, 3)) for _ in range(2)]
    for r in rend:
        r["rgb"].requires_grad_(True)
        r["distance"].requires_grad_(True)
    rays = types.SimpleNamespace(lossmult=0.25 + rand(*lead, 1), viewdirs=randn(*lead, 3), origins=randn(*lead, 3))
    batch = utils.Batch(rays=rays, rgb=rand(*lead, 3), disps=rand(*lead), normals=randn(*lead, 3), alphas=rand(*lead))
    return rend, rays, batch


def _routing_cfg(penalty="charb", S=2):
    from refnerf_pl_amd import configs
    configs.clear_config()
    return configs.Config(hip_fused_losses=True, data_loss_type=penalty, compute_normal_metrics=True, compute_disp_metrics=True,
                          data_coarse_loss_mult=0.4, interlevel_loss_mult=0.0, patch_size=S, depth_smoothness_loss_mult=0.5,
                          depth_smoothness_coarse_loss_mult=0.1, hip_check_finite=False)


@pytest.mark.gpu
def test_flag_routes_charb_statistics_and_smoothness_through_the_kernels(monkeypatch):
    """Config.hip_fused_losses with 'charb' and compute_normal_metrics: neither compute_data_loss nor
    compute_depth_smoothness_loss is called, stats carries the reference's keys in its order, the library exports the four
    entries.  (Without the kernels the flag fell back to compute_data_loss for 'charb', and dropped normal_maes for 'mse'.)"""
    from refnerf_pl_amd import _hip, train_utils
    _hip.require_device()
    for name in ENTRIES:
        assert hasattr(_hip.lib(), name), name

    def refuse(*a, **kw):
        raise AssertionError("the ATen path was taken")
    monkeypatch.setattr(train_utils, "compute_data_loss", refuse)
    monkeypatch.setattr(train_utils, "compute_depth_smoothness_loss", refuse)
    rend, rays, batch = _synthetic_step(6, 2)
    model = types.SimpleNamespace(num_levels=2)
    for penalty in PENALTIES:
        cfg = _routing_cfg(penalty)
        for r in rend:
            r["rgb"].grad = r["distance"].grad = None
        total, losses, stats = train_utils.compute_losses(model, batch, rays, rend, [{"weights": torch.zeros((1, 1), device=DEV)}] * 2, cfg)
        total.backward()
        assert tuple(losses) == ("data", "smoothness") and tuple(stats) == STAT_KEYS
        assert all(v.shape == (2,) and bool(torch.isfinite(v).all()) for v in stats.values())
        assert np.isfinite(float(total)) and float(rend[0]["rgb"].grad.abs().sum()) > 0 and float(rend[1]["distance"].grad.abs().sum()) > 0


@pytest.mark.gpu
def test_fused_data_terms_and_smoothness_do_not_synchronise_the_host():
    """The fused data term (charb, both statistics) and depth smoothness + backward to the seeds under
    torch.cuda.set_sync_debug_mode('error'): clean."""
    from refnerf_pl_amd import _hip, train_utils
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    _hip.require_device()
    rend, rays, batch = _synthetic_step(6, 2)
    cfg = _routing_cfg()
    model = types.SimpleNamespace(num_levels=2)
    hist = [{"weights": torch.zeros((1, 1), device=DEV)}] * 2

    def step():
        loss, stats, _, _ = train_utils.fused_refnerf_losses(model, batch, rays, rend, hist, cfg)
        (loss + train_utils.fused_depth_smoothness_loss(rend, cfg)).backward()
        return loss, stats
    step()                                         # library load and allocator warm-up stay outside
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, stats = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(stats) == STAT_KEYS and np.isfinite(float(loss.detach()))
    assert float(rend[0]["rgb"].grad.abs().sum()) > 0 and float(rend[1]["distance"].grad.abs().sum()) > 0


# ------------------------------------------------------------------------------------------- GPU: argument checks
@pytest.mark.gpu
def test_entries_refuse_bad_arguments():
    """REFNERF_EINVAL (-1, with a message) before any launch: a null required pointer, R <= 0, an unknown penalty, a negative or
    non-finite padding, half of an optional group; a null pointer, P <= 0, S < 2, P S S >= 2^31.  Every pointer that reaches
    a launch is a live tensor of the right size."""
    from refnerf_pl_amd import _hip
    _hip.require_device()
    lib, EINVAL = _hip.lib(), -1
    stream = _hip.stream_ptr()
    R = 4
    t3, t1 = [torch.rand((R, 3), device=DEV) for _ in range(4)], [torch.rand((R,), device=DEV) for _ in range(5)]
    terms, up, g_rgb = torch.zeros((R, 5), device=DEV), torch.ones(1, device=DEV), torch.zeros((R, 3), device=DEV)

    def data_args(**kw):
        A = _hip.DataTermsArgs()
        A.R, A.penalty, A.charb_padding = R, 1, 0.001
        A.d_rgb, A.d_gt_rgb, A.d_lossmult = t3[0].data_ptr(), t3[1].data_ptr(), t1[0].data_ptr()
        A.d_distance_mean, A.d_disps = t1[1].data_ptr(), t1[2].data_ptr()
        A.d_acc, A.d_alphas, A.d_normals, A.d_normals_gt = t1[3].data_ptr(), t1[4].data_ptr(), t3[2].data_ptr(), t3[3].data_ptr()
        A.d_terms, A.d_upstream, A.d_g_rgb = terms.data_ptr(), up.data_ptr(), g_rgb.data_ptr()
        for k, v in kw.items():
            setattr(A, k, v)
        return A
    bad_data = [dict(d_rgb=None), dict(d_gt_rgb=None), dict(d_lossmult=None), dict(R=0), dict(R=-3), dict(penalty=2), dict(penalty=-1),
                dict(charb_padding=-0.5), dict(charb_padding=float("inf")), dict(charb_padding=float("nan")),
                dict(d_disps=None), dict(d_distance_mean=None), dict(d_acc=None), dict(d_alphas=None), dict(d_normals=None),
                dict(d_normals_gt=None), dict(d_acc=None, d_alphas=None, d_normals=None)]
    for entry, own in ((lib.refnerf_data_terms_forward, [dict(d_terms=None)]),
                       (lib.refnerf_data_terms_backward, [dict(d_upstream=None), dict(d_g_rgb=None)])):
        assert entry(C.byref(data_args()), stream) == 0
        assert entry(C.byref(data_args(d_distance_mean=None, d_disps=None, d_acc=None, d_alphas=None, d_normals=None,
                                       d_normals_gt=None, penalty=0, charb_padding=0.0)), stream) == 0
        for bad in bad_data + own:
            assert entry(C.byref(data_args(**bad)), stream) == EINVAL, bad
            assert lib.refnerf_last_error().decode().startswith("refnerf_data_terms_"), bad
        assert entry(None, stream) == EINVAL

    P, S = 3, 2
    dist, acc, rgb = torch.rand((P, S, S), device=DEV), torch.rand((P, S, S), device=DEV), torch.rand((P, S, S, 3), device=DEV)
    s_terms, g_dist = torch.zeros((P, 2), device=DEV), torch.zeros((P, S, S), device=DEV)

    def smooth_args(**kw):
        A = _hip.DepthSmoothnessArgs()
        A.P, A.S = P, S
        A.d_distance, A.d_acc, A.d_rgb = dist.data_ptr(), acc.data_ptr(), rgb.data_ptr()
        A.d_terms, A.d_upstream, A.d_g_distance = s_terms.data_ptr(), up.data_ptr(), g_dist.data_ptr()
        for k, v in kw.items():
            setattr(A, k, v)
        return A
    bad_smooth = [dict(d_distance=None), dict(d_acc=None), dict(d_rgb=None), dict(P=0), dict(P=-1), dict(S=1), dict(S=0),
                  dict(P=2 ** 29, S=2), dict(P=1, S=46341)]
    for entry, own in ((lib.refnerf_depth_smoothness_forward, [dict(d_terms=None)]),
                       (lib.refnerf_depth_smoothness_backward, [dict(d_upstream=None), dict(d_g_distance=None)])):
        assert entry(C.byref(smooth_args()), stream) == 0
        for bad in bad_smooth + own:
            assert entry(C.byref(smooth_args(**bad)), stream) == EINVAL, bad
            assert lib.refnerf_last_error().decode().startswith("refnerf_depth_smoothness_"), bad
        assert entry(None, stream) == EINVAL
    torch.cuda.synchronize()
    assert float(terms[:, 4].sum()) == 0.0 and float(terms[:, 0].sum()) > 0      # the last good forward had no optional group
    assert float(g_rgb.abs().sum()) > 0 and float(s_terms.sum()) > 0 and float(g_dist.abs().sum()) > 0

    # the Python wrappers check every shape before a pointer is taken
    with pytest.raises(ValueError):
        _hip.data_terms_args(t3[0], t3[1], t1[0][:3].contiguous(), "charb", 0.001)
    with pytest.raises(ValueError):
        _hip.data_terms_args(t3[0], t3[1], t1[0], "huber", 0.001)
    with pytest.raises(ValueError):
        _hip.depth_smoothness_args(dist, acc, rgb[..., :2].contiguous())

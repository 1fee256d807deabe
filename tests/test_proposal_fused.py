"""Config.hip_fused_proposal: the dilation of the step function between proposal levels (refnerf_max_dilate_weights) and the
interlevel loss (refnerf_interlevel_forward / _backward) as kernels.

Stage tests against the fp32 mirror (stepfun.max_dilate_weights) / the mirror in float64 (stepfun.lossfun_outer) on the CPU,
then the two call sites end to end on the fixtures that pin the proposal configuration (model_dilation_anneal_eval,
propmlp_interlevel) with the bars of the existing tests of those fixtures.
"""
import os
import types

import numpy as np
import pytest
import torch

from helpers import load_golden, params_from_golden, rays_from_golden
from test_geometry_losses import _check_fingerprint, _fingerprint, _propmlp_setup

GIN = os.path.join(os.path.dirname(__file__), "..", "configs", "refnerf_blender.gin")
DEV = "cuda:0"
EPS = float(torch.finfo(torch.float32).eps)
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------- CPU
def test_flag_defaults_off():
    from refnerf_pl_amd import configs
    configs.clear_config()
    assert configs.Config().hip_fused_proposal is False
    assert configs.Config(hip_fused_proposal=True).hip_fused_proposal is True


def _interlevel_inputs(R, N, Np, seed):
    """fp32 step functions on [0, 1]: (t [R,N+1], w [R,N]) the final level, (t_env [R,Np+1], w_env [R,Np]) a proposal level
    whose weights are scaled by 0.6 (the penalty is active on most intervals); one proposal knot per ray is copied into the
    fine knots, clamped between its neighbours (the <= / > tie of the searches)."""
    g = torch.Generator().manual_seed(seed)

    def knots(n):
        t = torch.sort(torch.rand((R, n + 1), generator=g), dim=-1).values
        t[:, 0], t[:, -1] = 0.0, 1.0
        return t

    def weights(n):
        w = 0.25 + torch.rand((R, n), generator=g)
        return w / w.sum(-1, keepdim=True)
    t, t_env = knots(N), knots(Np)
    j = torch.randint(1, N, (R,), generator=g) if N > 1 else torch.zeros(R, dtype=torch.long)
    k = torch.randint(0, Np + 1, (R,), generator=g)
    rows = torch.arange(R)
    lo = t[rows, torch.clamp(j - 1, min=0)]
    hi = t[rows, torch.clamp(j + 1, max=N)]
    t[rows, j] = torch.minimum(torch.maximum(t_env[rows, k], lo), hi)
    assert bool((t[:, 1:] >= t[:, :-1]).all())
    return t, weights(N), t_env, (0.6 * weights(Np)).contiguous()


def _mirror_interlevel(t, w, t_env, w_env, upstream, dtype):
    """(per-ray loss sums, d (upstream * sum) / d w_env) of the mirror stepfun.lossfun_outer in `dtype` on the CPU"""
    from refnerf_pl_amd import stepfun
    t, w, t_env = (x.to(dtype) for x in (t, w, t_env))
    w_env = w_env.to(dtype).clone().requires_grad_(True)
    per_ray = stepfun.lossfun_outer(t, w, t_env, w_env).sum(-1)
    (per_ray.sum() * upstream).backward()
    return per_ray.detach(), w_env.grad


def test_flag_on_cpu_tensors_keeps_the_aten_interlevel_loss(monkeypatch):
    """With the flag set and CPU tensors compute_losses takes the ATen function (the kernels are never reached)."""
    from refnerf_pl_amd import _hip, configs, train_utils, utils
    configs.clear_config()
    cfg = configs.Config(hip_fused_proposal=True, data_loss_type='mse', hip_check_finite=False)
    assert cfg.interlevel_loss_mult == 1.0

    def boom(*a, **k):
        raise AssertionError("the fused interlevel kernel was called on CPU tensors")
    monkeypatch.setattr(_hip, "interlevel_forward", boom)
    R = 5
    t, w, t_env, w_env = _interlevel_inputs(R, 8, 6, seed=0)
    history = [dict(sdist=t_env, weights=w_env.clone().requires_grad_(True)), dict(sdist=t, weights=w)]
    assert not train_utils.fused_interlevel_supported(history)
    rgb = torch.full((R, 3), 0.5)
    renderings = [dict(rgb=rgb), dict(rgb=rgb)]
    rays = utils.rays_from_dict({k: np.zeros((R, c), np.float32) + 1 for k, c in (
        ("origins", 3), ("directions", 3), ("viewdirs", 3), ("radii", 1), ("imageplane", 2), ("lossmult", 1), ("near", 1),
        ("far", 1), ("cam_idx", 1))}, "cpu")
    batch = utils.Batch(rays=rays, rgb=np.full((R, 3), 0.25, np.float32))
    model = types.SimpleNamespace(num_levels=2)
    total, losses, _ = train_utils.compute_losses(model, batch, rays, renderings, history, cfg)
    assert list(losses) == ["data", "interlevel"]
    want = train_utils.interlevel_loss(history, cfg)
    assert float(want.detach()) > 0 and torch.equal(losses["interlevel"].detach(), want.detach())


# ------------------------------------------------------------------------------------------- GPU: dilation stage
DILATIONS = (1e-7, 0.0025, 0.0025 + 0.5 / 64, 2.0)      # the last clamps every shifted knot
KINDS = ("random", "sampled", "zero_width", "zero_weights")


def _dilate_inputs(kind, R, M, seed):
    """(t [R,M+1] nondecreasing in [0,1], w [R,M]) as fp32 CPU tensors"""
    from refnerf_pl_amd import _hip
    g = torch.Generator().manual_seed(seed)
    t = torch.sort(torch.rand((R, M + 1), generator=g), dim=-1).values
    w = torch.rand((R, M), generator=g) + 1e-3
    if kind == "sampled":
        # knots the fused resampler wrote: M + 1 (it takes num_samples > 1, so for M = 1 the first two of three)
        n = max(M, 2)
        coarse = torch.sort(torch.rand((R, 9), generator=g), dim=-1).values
        coarse[:, 0], coarse[:, -1] = 0.0, 1.0
        logits = torch.randn((R, 8), generator=g)
        sd, _ = _hip.sample_intervals(coarse.to(DEV), logits.to(DEV), n)
        t = sd.cpu()[:, :M + 1].contiguous()
    elif kind == "zero_width":
        j = torch.randint(0, M, (R,), generator=g)
        t[torch.arange(R), j + 1] = t[torch.arange(R), j]
        t = torch.sort(t, dim=-1).values
    elif kind == "zero_weights":
        w = torch.where(torch.rand((R, M), generator=g) < 0.3, torch.zeros(()), w)
    w = w / torch.clamp(w.sum(-1, keepdim=True), min=1e-6)
    return t.contiguous(), w.contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 37, 300])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 128, 171])
def test_hip_max_dilate_weights_vs_mirror(M, R):
    """Knots bit-equal to the mirror's t_dilate[..., 1:-1]; weights within (3M + 4) 2^-24 (relative, elementwise) of the
    mirror's un-normalised fp32 weights u renormalised in float64: u depends on correctly rounded operations and an exact
    max only, any order of the 3M-term fp32 sum is within (3M - 1) 2^-24, the division adds one rounding, 4 is slack."""
    from refnerf_pl_amd import _hip, stepfun
    _hip.require_device()
    worst = 0.0
    for ki, kind in enumerate(KINDS):
        t, w = _dilate_inputs(kind, R, M, seed=1000 * M + 10 * R + ki)
        t_d, w_d = t.to(DEV), w.to(DEV)
        for d in DILATIONS:
            td, u = stepfun.max_dilate_weights(t, w, d, domain=(0.0, 1.0), renormalize=False)
            u64 = u.double()
            ref = (u64 / torch.clamp(u64.sum(-1, keepdim=True), min=EPS ** 2))[..., 1:-1].numpy()
            sd, wd = _hip.max_dilate_weights(t_d, w_d, d, 0.0, 1.0)
            assert sd.shape == (R, 3 * M - 1) and wd.shape == (R, 3 * M - 2)
            np.testing.assert_array_equal(sd.cpu().numpy(), td[..., 1:-1].numpy(), err_msg=f"{kind} d={d}")
            got = wd.cpu().numpy().astype(np.float64)
            err = np.abs(got - ref)
            bound = (3 * M + 4) * U24 * ref
            rel = float((err[ref > 0] / ref[ref > 0]).max()) if (ref > 0).any() else 0.0
            worst = max(worst, rel)
            assert (err <= bound).all(), f"{kind} d={d}: worst relative error {rel:.3e} vs bound {(3 * M + 4) * U24:.3e}"
    print(f"max_dilate_weights M={M} R={R}: worst relative weight error {worst:.3e} (bound {(3 * M + 4) * U24:.3e})")


@pytest.mark.gpu
def test_hip_max_dilate_weights_argument_checks():
    from refnerf_pl_amd import _hip
    _hip.require_device()
    for M in (0, 172):
        with pytest.raises(ValueError):
            _hip.max_dilate_weights(torch.zeros((3, M + 1), device=DEV), torch.zeros((3, M), device=DEV), 0.0025, 0.0, 1.0)
    sd, wd = _hip.max_dilate_weights(torch.zeros((0, 65), device=DEV), torch.zeros((0, 64), device=DEV), 0.0025, 0.0, 1.0)
    assert sd.shape == (0, 191) and wd.shape == (0, 190)


# ------------------------------------------------------------------------------------------- GPU: dilation end to end
@pytest.mark.gpu
def test_hip_dilation_model_options_fused():
    """model_dilation_anneal_eval through Model.__call__ with the flag set: the assertions and bars of
    test_dilation_and_anneal_model_options, and level 0 bit-equal to the flag-off run of the same process."""
    from refnerf_pl_amd import _hip, configs, models, utils
    _hip.require_device()
    g = load_golden("model_dilation_anneal_eval")
    out = {}
    for flag in (False, True):
        configs.clear_config()
        configs.parse_config_files_and_bindings([GIN], [str(b) for b in g["bindings"]] + [f"Config.hip_fused_proposal = {flag}"])
        cfg = configs.Config()
        assert cfg.hip_fused_proposal is flag
        model = models.construct_model(utils.dummy_rays(), cfg).to(DEV).eval()
        assert model.dilation_bias == 0.0025 and model.anneal_slope == 10.
        model.nerf_mlp.load_flat_params(params_from_golden(g))
        with torch.no_grad():
            out[flag] = model(utils.rays_from_dict(rays_from_golden(g), DEV), float(g["train_frac"]), True)
    rend, hist = out[True]
    np.testing.assert_array_equal(hist[0]["sdist"].cpu().numpy(), g["L0_h_sdist"])
    sd1 = hist[1]["sdist"].cpu().numpy()
    ok = np.abs(sd1 - g["L1_h_sdist"]).max(-1) < 2e-6
    assert ok.mean() >= 0.9                                   # a renormalisation sum 1 ulp apart can move a knot
    np.testing.assert_allclose(rend[1]["rgb"].cpu().numpy()[ok], g["L1_r_rgb"][ok], atol=1e-5)
    np.testing.assert_allclose(rend[1]["rgb"].cpu().numpy(), g["L1_r_rgb"], atol=1e-3)
    np.testing.assert_allclose(rend[0]["rgb"].cpu().numpy(), g["L0_r_rgb"], atol=1e-5)
    rend_off, hist_off = out[False]
    for k in ("sdist", "weights"):
        assert torch.equal(hist[0][k], hist_off[0][k]), k
    assert torch.equal(rend[0]["rgb"], rend_off[0]["rgb"])
    big = models.Model(config=cfg, num_prop_samples=192, num_nerf_samples=192, dilation_bias=0.0025, num_levels=2,
                       single_mlp=True, resample_padding=0.01, anneal_slope=0.).to(DEV).eval()
    with pytest.raises(ValueError, match="dilated step function has 574 intervals"), torch.no_grad():
        big(utils.rays_from_dict(rays_from_golden(g), DEV), 1.0, False)


@pytest.mark.gpu
def test_hip_fused_dilation_replays_from_a_graph():
    """Nothing in the fused dilation synchronises or allocates outside torch: the eval call of the dilation fixture is
    captured by graphs.GraphedForward and replays bit-equal to the eager call."""
    from refnerf_pl_amd import _hip, configs, graphs, models, utils
    _hip.require_device()
    g = load_golden("model_dilation_anneal_eval")
    configs.clear_config()
    configs.parse_config_files_and_bindings([GIN], [str(b) for b in g["bindings"]] + ["Config.hip_fused_proposal = True"])
    cfg = configs.Config()
    model = models.construct_model(utils.dummy_rays(), cfg).to(DEV).eval()
    model.nerf_mlp.load_flat_params(params_from_golden(g))
    rays = utils.rays_from_dict(rays_from_golden(g), DEV)
    with torch.no_grad():
        rend, hist = model(rays, float(g["train_frac"]), True)
    replay = graphs.GraphedForward(model, rays, float(g["train_frac"]), True)
    rend_g, hist_g = replay(rays)
    torch.cuda.synchronize()
    for lvl in range(2):
        assert torch.equal(hist_g[lvl]["sdist"], hist[lvl]["sdist"]) and torch.equal(rend_g[lvl]["rgb"], rend[lvl]["rgb"]), lvl


# ------------------------------------------------------------------------------------------- GPU: interlevel stage
def _rel_l2(a, b):
    """relative L2 distance of a from the reference b; a reference that is all zeros (no interval penalised) asks for equality"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.any(b):
        return 0.0 if not np.any(a) else float("inf")
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _check_interlevel_stage(t, w, t_env, w_env, upstream, what):
    """The kernels against the float64 mirror: rel-L2 of the per-ray sums and of g_w_env within
    max(4 x the fp32 mirror's own distance, 32 x 2^-24); exact zeros where nothing penalised covers an element; two
    backward calls bit-identical.  Returns the per-ray sums of the kernel."""
    from refnerf_pl_amd import _hip
    loss64, g64 = _mirror_interlevel(t, w, t_env, w_env, upstream, torch.float64)
    loss32, g32 = _mirror_interlevel(t, w, t_env, w_env, upstream, torch.float32)
    d_loss32, d_g32 = _rel_l2(loss32, loss64), _rel_l2(g32, g64)
    assert d_g32 <= 1e-4, f"{what}: ill-conditioned inputs (fp32 mirror gradient {d_g32:.2e} from float64)"
    dev = [x.to(DEV) for x in (t, w, t_env, w_env)]
    up = torch.tensor([upstream], dtype=torch.float32, device=DEV)
    ray_loss = _hip.interlevel_forward(*dev)
    g_a = _hip.interlevel_backward(*dev, up)
    g_b = _hip.interlevel_backward(*dev, up)
    assert torch.equal(g_a, g_b), what
    assert ray_loss.shape == (t.shape[0],) and g_a.shape == w_env.shape
    d_loss, d_g = _rel_l2(ray_loss.cpu(), loss64), _rel_l2(g_a.cpu(), g64)
    floor = 32 * U24
    msg = (f"{what}: per-ray sums rel-L2 {d_loss:.2e} (fp32 mirror {d_loss32:.2e}), "
           f"g_w_env rel-L2 {d_g:.2e} (fp32 mirror {d_g32:.2e}), floor {floor:.2e}")
    print(msg)
    assert d_loss <= max(4 * d_loss32, floor), msg
    assert d_g <= max(4 * d_g32, floor), msg
    # exact zeros: elements of w_env that no penalised fine interval's range [idx_lo(t_i), idx_hi(t_{i+1})) covers
    t64, te64 = t.double(), t_env.double()
    cnt = torch.searchsorted(te64.contiguous(), t64.contiguous(), right=True)
    Np = w_env.shape[-1]
    lo, hi = torch.clamp(cnt - 1, min=0)[..., :-1], torch.clamp(cnt, max=Np)[..., 1:]
    cy = torch.cat([torch.zeros_like(te64[..., :1]), torch.cumsum(w_env.double(), -1)], -1)
    pen = (w.double() - (torch.take_along_dim(cy, hi, -1) - torch.take_along_dim(cy, lo, -1))) > 0
    cover = torch.zeros((t.shape[0], Np + 1), dtype=torch.int64)       # difference array of the penalised ranges (exact: integers)
    cover.scatter_add_(1, lo, pen.long())
    cover.scatter_add_(1, hi, -pen.long())
    covered = torch.cumsum(cover, dim=1)[:, :Np] > 0
    must_be_zero = (g64 == 0) & ~covered
    assert bool((g_a.cpu()[must_be_zero] == 0).all()), what
    return ray_loss


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 37, 300])
@pytest.mark.parametrize("N,Np", [(2, 2), (32, 64), (33, 63), (64, 65), (128, 128), (192, 171), (512, 512)])
def test_hip_interlevel_stage_vs_float64_mirror(N, Np, R):
    from refnerf_pl_amd import _hip
    _hip.require_device()
    t, w, t_env, w_env = _interlevel_inputs(R, N, Np, seed=100000 + 1000 * N + 10 * Np + R)
    _check_interlevel_stage(t, w, t_env, w_env, 0.37, f"N={N} Np={Np} R={R}")


@pytest.mark.gpu
def test_hip_interlevel_argument_checks():
    from refnerf_pl_amd import _hip
    _hip.require_device()
    up = torch.ones(1, device=DEV)

    def call(R, N, Np):
        args = [torch.zeros(s, device=DEV) for s in ((R, N + 1), (R, N), (R, Np + 1), (R, Np))]
        return _hip.interlevel_forward(*args), _hip.interlevel_backward(*args, up)
    for N, Np in ((513, 64), (64, 513), (0, 64), (64, 0)):
        with pytest.raises(ValueError):
            call(3, N, Np)
    loss, g = call(0, 64, 48)
    assert loss.shape == (0,) and g.shape == (0, 48)


@pytest.mark.gpu
def test_hip_interlevel_stage_on_the_propmlp_fixture():
    """The stage on the propmlp_interlevel fixture's level outputs (12 rays, 48 proposal and 64 final intervals): the mean
    is the golden's interlevel loss (rel 5e-5, the oracle test's bar), the gradient meets the stage bar."""
    from refnerf_pl_amd import _hip
    _hip.require_device()
    g = load_golden("propmlp_interlevel")
    t, w, t_env, w_env = (torch.tensor(np.asarray(g[k], np.float32)) for k in ("L1_h_sdist", "L1_h_weights", "L0_h_sdist", "L0_h_weights"))
    ray_loss = _check_interlevel_stage(t, w, t_env, w_env, 1.0 / w.numel(), "propmlp_interlevel")
    assert float(ray_loss.sum()) / w.numel() == pytest.approx(float(g["loss_interlevel"]), rel=5e-5)


# ------------------------------------------------------------------------------------------- GPU: interlevel end to end
def _flat_grads(mlp):
    from refnerf_pl_amd import layout
    out = np.zeros(layout.NUM_PARAMS, np.float32)
    for spec, lin in mlp._named_linears():
        if lin.weight.grad is not None:
            out[spec.w_off:spec.w_off + spec.out_dim * spec.in_dim] = lin.weight.grad.reshape(-1).cpu().numpy()
        if lin.bias.grad is not None:
            out[spec.b_off:spec.b_off + spec.out_dim] = lin.bias.grad.cpu().numpy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("chains", ["f32", "f16x2"])
def test_hip_separate_propmlp_and_fused_interlevel_loss(chains, monkeypatch):
    """propmlp_interlevel with the flag set: the assertions and bars of test_hip_separate_propmlp_and_interlevel_loss; the
    interlevel loss alone leaves the NeRF MLP's gradient exactly zero and gives the proposal network the golden's."""
    from refnerf_pl_amd import _hip, models, train_utils, utils
    _hip.require_device()
    g = load_golden("propmlp_interlevel")
    cfg, prop = _propmlp_setup(g)
    cfg.hip_train_precision = cfg.hip_bwd_precision = chains
    cfg.hip_fused_proposal = True
    calls = []
    real = _hip.interlevel_backward
    monkeypatch.setattr(_hip, "interlevel_backward", lambda *a: (calls.append(1), real(*a))[1])

    def make():
        model = models.construct_model(utils.dummy_rays(), cfg).to(DEV).train()
        assert model.prop_mlp is not model.nerf_mlp and model.prop_mlp.density_bias == -3.0
        model.nerf_mlp.load_flat_params(params_from_golden(g))
        model.prop_mlp.load_flat_params(prop)
        return model
    model = make()
    rays = utils.rays_from_dict(rays_from_golden(g), DEV)
    batch = utils.Batch(rays=rays, rgb=np.asarray(g["gt_rgb"], np.float32))
    renderings, history = model(rays, 1.0, False)
    total, losses, _ = train_utils.compute_losses(model, batch, rays, renderings, history, cfg)
    assert list(losses)[:2] == ["data", "interlevel"]
    for k in ("data", "interlevel", "orientation", "predicted_normals"):
        assert float(losses[k].detach()) == pytest.approx(float(g["loss_" + k]), rel=2e-4), k
    total.backward()
    assert len(calls) == 1                                   # the fused node ran: one proposal level
    _check_fingerprint(_fingerprint(_flat_grads(model.nerf_mlp)), g["fp_nerf"], 2e-4, "nerf")
    _check_fingerprint(_fingerprint(_flat_grads(model.prop_mlp)), g["fp_prop"], 2e-4, "prop")
    model = make()
    _, history = model(rays, 1.0, False)
    train_utils.fused_interlevel_loss(history, cfg).backward()
    assert np.abs(_flat_grads(model.nerf_mlp)).max() == 0.0            # the final level is detached in this loss
    _check_fingerprint(_fingerprint(_flat_grads(model.prop_mlp)), g["fp_prop_interlevel_only"], 2e-4, "prop, interlevel only")

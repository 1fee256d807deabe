"""mip-NeRF 360's distortion loss: stepfun.lossfun_distortion / interval_distortion (ATen restatements), the O(N) kernels
refnerf_distortion_forward / _backward (include/refnerf_distortion.h, csrc/refnerf_distortion.h) and the opt-in loss term
Config.hip_distortion_loss.

Truth is the O(N^2) definition in float64 on the float32 inputs (distortion_cases.truth).  The kernels' bar, for the per-ray
loss and elementwise for grad_w, is |hip - f64| <= (2N + 16) eps32 f64 (distortion_cases.bound): both are sums of at most 2N
non-negative products, so the bar holds for any summation order, and where the float64 value is exactly 0 the kernel's is too.
A sequential float32 emulation of the recurrence stays below 8e-7 relative at N <= 512.
MEASURED on an MI355X over every shape and row kind below: the kernels' worst relative distance from float64 is
1.90e-07 (loss) and 3.34e-07 (grad_w, a two-hot row at N = 512), against bars from 2.15e-06 (N = 1) to 1.24e-04 (N = 512).
Against the reference's own float32 values (tests/golden/distortion.npz; on the 'tiny' rows, where its midpoint differences
cancel, up to 3.9e-05 (loss) and 3.1e-04 (grad_w) from float64, the kernels 1.2e-07 and 2.2e-07 there):
|hip - ref32| <= |ref32 - f64| + the bar above.
"""
import os
import types

import numpy as np
import pytest
import torch

import distortion_cases as DC
from helpers import load_golden

DEV = "cuda:0"
EPS = DC.EPS32
NS = [1, 2, 63, 64, 65, 128, 129, 257, 512]      # off the 64-lane trip (63 / 64 / 65) and off the per-lane run (128 / 129, 257)
RS = [1, 3, 4, 5, 9]                             # off the four-waves-per-block trip
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "refnerf_distortion.h")
ENTRIES = ["refnerf_distortion_forward", "refnerf_distortion_backward"]


# ------------------------------------------------------------------------------------------- CPU
def _fixture_cases():
    g = load_golden("distortion")
    for i, (N, R) in enumerate(g["shapes"]):
        for kind in g["kinds"]:
            p = f"s{i}_{kind}_"
            yield int(N), int(R), str(kind), int(g["seed"]), {k: g[p + k] for k in ("t", "w", "loss", "grad_w")}


def test_aten_restatement_is_the_reference_bit_for_bit():
    """stepfun.lossfun_distortion and its w gradient on the CPU equal the reference's float32 values; the fixture's inputs
    are the generator's (the GPU tests draw from the same generator)."""
    from refnerf_pl_amd import stepfun
    seen = 0
    for N, R, kind, seed, f in _fixture_cases():
        t, w = DC.rows(kind, R, N, seed)
        assert np.array_equal(t, f["t"]) and np.array_equal(w, f["w"]), (N, R, kind)
        wt = torch.tensor(f["w"], requires_grad=True)
        loss = stepfun.lossfun_distortion(torch.tensor(f["t"]), wt)
        loss.sum().backward()
        assert torch.equal(loss.detach(), torch.tensor(f["loss"])), (N, R, kind)
        assert torch.equal(wt.grad, torch.tensor(f["grad_w"])), (N, R, kind)
        seen += 1
    assert seen == 15


def test_aten_restatement_is_differentiable_in_t_and_follows_dtype_and_batch_shape():
    from refnerf_pl_amd import stepfun
    t, w = DC.rows("random", 6, 5, 1)
    t64 = torch.tensor(t, dtype=torch.float64).reshape(2, 3, 6).requires_grad_(True)
    w64 = torch.tensor(w, dtype=torch.float64).reshape(2, 3, 5).requires_grad_(True)
    loss = stepfun.lossfun_distortion(t64, w64)
    assert loss.shape == (2, 3) and loss.dtype == torch.float64
    l64, g64 = DC.truth(t, w)
    np.testing.assert_allclose(loss.detach().numpy().reshape(-1), l64, rtol=1e-13)
    gt, gw = torch.autograd.grad(loss.sum(), (t64, w64))
    np.testing.assert_allclose(gw.numpy().reshape(6, 5), g64, rtol=1e-13)
    assert bool(torch.isfinite(gt).all()) and float(gt.abs().sum()) > 0


def test_interval_distortion_is_the_reference_bit_for_bit():
    from refnerf_pl_amd import stepfun
    g = load_golden("distortion")
    args = [torch.tensor(g[k]) for k in ("iv_t0_lo", "iv_t0_hi", "iv_t1_lo", "iv_t1_hi")]
    assert len(g["iv_value"]) == 36
    disjoint = (args[0] > args[3]) | (args[2] > args[1])
    assert 0 < int(disjoint.sum()) < len(disjoint)
    assert torch.equal(stepfun.interval_distortion(*args), torch.tensor(g["iv_value"]))


def test_new_header_parses_and_declares_exactly_the_two_entries():
    import ctypes as C
    from refnerf_pl_amd import _abi, _hip
    constants, structs, prototypes = _abi.load(HEADER)
    assert list(prototypes) == ENTRIES and not structs
    assert constants == {}                        # the error codes stay refnerf_hip.h's
    ptr, i32 = C.c_void_p, C.c_int32
    assert prototypes["refnerf_distortion_forward"] == (C.c_int, [ptr, ptr, i32, i32, ptr, ptr])
    assert prototypes["refnerf_distortion_backward"] == (C.c_int, [ptr, ptr, ptr, i32, i32, ptr, ptr])
    assert os.path.samefile(_hip.DISTORTION_HEADER, HEADER)
    assert callable(_hip.distortion_forward) and callable(_hip.distortion_backward)


def test_refnerf_hip_h_is_closed():
    """the main header keeps the counts tests/test_abi.py pins, and none of the new names"""
    from refnerf_pl_amd import _abi
    assert (len(_abi.prototypes), len(_abi.constants), len(_abi.structs)) == (61, 59, 16)
    assert not set(ENTRIES) & set(_abi.prototypes)
    assert _abi.constants["REFNERF_ABI_VERSION"] == 11


def _cpu_history(R=5, N=8, Np=6):
    t, w = DC.rows("random", R, N, 3)
    te, we = DC.rows("random", R, Np, 4)
    return [dict(sdist=torch.tensor(te), weights=torch.tensor(we).requires_grad_(True)),
            dict(sdist=torch.tensor(t), weights=torch.tensor(w).requires_grad_(True))]


def _cpu_losses(cfg, history, R=5):
    from refnerf_pl_amd import train_utils, utils
    rgb = torch.full((R, 3), 0.5)
    renderings = [dict(rgb=rgb), dict(rgb=rgb)]
    rays = utils.rays_from_dict({k: np.zeros((R, c), np.float32) + 1 for k, c in (
        ("origins", 3), ("directions", 3), ("viewdirs", 3), ("radii", 1), ("imageplane", 2), ("lossmult", 1), ("near", 1),
        ("far", 1), ("cam_idx", 1))}, "cpu")
    batch = utils.Batch(rays=rays, rgb=np.full((R, 3), 0.25, np.float32))
    return train_utils.compute_losses(types.SimpleNamespace(num_levels=2), batch, rays, renderings, history, cfg)


def test_flag_off_changes_nothing_and_flag_on_appends_the_aten_term_on_cpu(monkeypatch):
    from refnerf_pl_amd import _hip, configs, stepfun, train_utils
    configs.clear_config()
    assert configs.Config().hip_distortion_loss is False and configs.Config().distortion_loss_mult == 0.01

    def boom(*a, **k):
        raise AssertionError("the fused distortion kernel was called on CPU tensors")
    monkeypatch.setattr(_hip, "distortion_forward", boom)
    history = _cpu_history()
    assert not train_utils.fused_distortion_supported(history)
    kw = dict(data_loss_type='mse', hip_check_finite=False)
    total_0, losses_0, _ = _cpu_losses(configs.Config(**kw), history)
    total_off, losses_off, _ = _cpu_losses(configs.Config(hip_distortion_loss=False, distortion_loss_mult=0.5, **kw), history)
    assert list(losses_0) == list(losses_off) == ["data", "interlevel"]
    assert torch.equal(total_0, total_off) and all(torch.equal(losses_0[k], losses_off[k]) for k in losses_0)
    # the multiplier at 0 keeps the term away even with the flag on
    _, losses_zero, _ = _cpu_losses(configs.Config(hip_distortion_loss=True, distortion_loss_mult=0.0, **kw), history)
    assert list(losses_zero) == ["data", "interlevel"]
    cfg = configs.Config(hip_distortion_loss=True, distortion_loss_mult=0.5, **kw)
    total_on, losses_on, _ = _cpu_losses(cfg, history)
    assert list(losses_on) == ["data", "interlevel", "distortion"]
    want = 0.5 * torch.mean(stepfun.lossfun_distortion(history[-1]["sdist"], history[-1]["weights"]))
    assert float(want.detach()) > 0 and torch.equal(losses_on["distortion"].detach(), want.detach())
    assert torch.equal(train_utils.distortion_loss(history, cfg).detach(), want.detach())
    assert all(torch.equal(losses_on[k], losses_0[k]) for k in losses_0)
    assert float(total_on.detach()) == pytest.approx(float(total_0.detach()) + float(want.detach()), rel=1e-6)
    (g,) = torch.autograd.grad(losses_on["distortion"], history[-1]["weights"])
    _, g64 = DC.truth(history[-1]["sdist"].numpy(), history[-1]["weights"].detach().numpy())
    np.testing.assert_allclose(g.numpy(), 0.5 / 5 * g64, rtol=1e-4)


def test_fused_support_rule():
    from refnerf_pl_amd import train_utils
    meta = lambda n_t, n_w: [dict(sdist=torch.empty((2, n_t), device="meta"), weights=torch.empty((2, n_w), device="meta"))]   # noqa: E731
    assert not train_utils.fused_distortion_supported(meta(9, 8))            # not a CUDA tensor
    fake = lambda n_t, n_w: [dict(sdist=types.SimpleNamespace(is_cuda=True, shape=(2, n_t)),                                # noqa: E731
                                  weights=types.SimpleNamespace(is_cuda=True, shape=(2, n_w)))]
    assert train_utils.fused_distortion_supported(fake(2, 1)) and train_utils.fused_distortion_supported(fake(513, 512))
    assert not train_utils.fused_distortion_supported(fake(514, 513))
    assert not train_utils.fused_distortion_supported(fake(1, 0))
    assert not train_utils.fused_distortion_supported(fake(8, 8))


# ------------------------------------------------------------------------------------------- GPU: the kernels
WORST = {"loss": 0.0, "grad_w": 0.0}


def _rel(a, b):
    """elementwise |a - b| / b where b > 0; where b == 0 the distance itself (must be 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.where(b > 0, np.abs(a - b) / np.where(b > 0, b, 1.0), np.abs(a))


def _hip_pair(t, w, up=1.0):
    from refnerf_pl_amd import _hip
    td, wd = torch.tensor(t, device=DEV), torch.tensor(w, device=DEV)
    g = torch.tensor([up], dtype=torch.float32, device=DEV)
    return _hip.distortion_forward(td, wd), _hip.distortion_backward(td, wd, g)


def _check_vs_float64(t, w, what):
    """the bar, exact zeros, two calls bit-equal; returns (loss, grad_w) as numpy"""
    N = w.shape[-1]
    l64, g64 = DC.truth(t, w)
    loss, grad = _hip_pair(t, w)
    loss_b, grad_b = _hip_pair(t, w)
    assert torch.equal(loss, loss_b) and torch.equal(grad, grad_b), what
    assert loss.shape == (t.shape[0],) and grad.shape == w.shape and loss.dtype == grad.dtype == torch.float32
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    assert np.isfinite(loss).all() and np.isfinite(grad).all(), what
    rl, rg = _rel(loss, l64), _rel(grad, g64)
    WORST["loss"], WORST["grad_w"] = max(WORST["loss"], float(rl.max())), max(WORST["grad_w"], float(rg.max()))
    print(f"{what}: loss rel {rl.max():.2e}, grad_w rel {rg.max():.2e}, bar {DC.bound(N):.2e}; worst so far {WORST['loss']:.2e} / {WORST['grad_w']:.2e}")
    assert (loss[l64 == 0] == 0).all() and (grad[g64 == 0] == 0).all(), what
    assert rl.max() <= DC.bound(N), f"{what}: loss {rl.max():.3e} > {DC.bound(N):.3e} at ray {int(rl.argmax())}"
    assert rg.max() <= DC.bound(N), f"{what}: grad_w {rg.max():.3e} > {DC.bound(N):.3e} at {np.unravel_index(int(rg.argmax()), rg.shape)}"
    return loss, grad


@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("N", NS)
def test_hip_distortion_vs_float64(N, R):
    """every row kind at (R, N): the bar, exact zeros, determinism, and each row alone bit-equal to the row in its batch"""
    from refnerf_pl_amd import _hip
    _hip.require_device()
    for kind in DC.KINDS:
        t, w = DC.rows(kind, R, N, 100 + R)
        loss, grad = _check_vs_float64(t, w, f"{kind} N={N} R={R}")
        if kind == "zero":
            assert not loss.any() and not grad.any()
        if kind == "onehot":                    # L = delta_k / 3 on the hot interval
            np.testing.assert_allclose(loss, ((t[:, 1:] - t[:, :-1]) * w).sum(-1) / 3, rtol=4 * EPS)
        if R > 1:
            for r in range(R):
                one_l, one_g = _hip_pair(t[r:r + 1], w[r:r + 1])
                assert np.array_equal(one_l.cpu().numpy(), loss[r:r + 1]) and np.array_equal(one_g.cpu().numpy(), grad[r:r + 1]), (kind, r)


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS[1:])
def test_hip_distortion_two_hot_rows(N):
    """weight 0.5 on two intervals: a dropped or doubled term of either scan is O(1) of the value.  The pairs: the ends, the
    first two, the last two, every neighbouring pair across two lanes' runs, and pairs a power-of-two number of lanes apart."""
    from refnerf_pl_amd import _hip
    _hip.require_device()
    t, w, pairs = DC.two_hot_rows(N)
    assert {(0, N - 1), (0, 1), (N - 2, N - 1)} <= set(pairs)
    C = DC.run_length(N)
    assert all((b - 1, b) in pairs for b in range(C, N, C))
    loss, grad = _check_vs_float64(t, w, f"two-hot N={N} ({len(pairs)} pairs)")
    for r, (i, j) in enumerate(pairs):          # the closed form: 0.5 |u_i - u_j| + (delta_i + delta_j) / 12
        u = (t[r, 1:].astype(np.float64) + t[r, :-1]) / 2
        d = t[r, 1:].astype(np.float64) - t[r, :-1]
        assert loss[r] == pytest.approx(0.5 * abs(u[i] - u[j]) + (d[i] + d[j]) / 12, rel=DC.bound(N)), (i, j)


@pytest.mark.gpu
def test_hip_distortion_vs_the_reference_float32():
    """|hip - ref32| <= |ref32 - f64| + the bar, on the fixture's inputs"""
    from refnerf_pl_amd import _hip
    _hip.require_device()
    for N, R, kind, _, f in _fixture_cases():
        l64, g64 = DC.truth(f["t"], f["w"])
        loss, grad = _hip_pair(f["t"], f["w"])
        for hip, ref32, f64, name in ((loss.cpu().numpy(), f["loss"], l64, "loss"), (grad.cpu().numpy(), f["grad_w"], g64, "grad_w")):
            ref_gap = np.abs(ref32.astype(np.float64) - f64)
            slack = ref_gap + DC.bound(N) * f64
            worst = np.abs(hip.astype(np.float64) - ref32) - slack
            print(f"{kind} N={N} R={R} {name}: reference fp32 within {(_rel(ref32, f64)).max():.2e} of float64, hip within {(_rel(hip, f64)).max():.2e}")
            assert (worst <= 0).all(), (N, R, kind, name, float(worst.max()))


@pytest.mark.gpu
def test_hip_distortion_upstream_scales_the_gradient():
    from refnerf_pl_amd import _hip
    _hip.require_device()
    t, w = DC.rows("random", 5, 65, 9)
    _, g1 = _hip_pair(t, w, 1.0)
    _, g2 = _hip_pair(t, w, -0.25)               # a power of two: exact
    assert torch.equal(g2, -0.25 * g1)
    _, g3 = _hip_pair(t, w, 0.37)
    np.testing.assert_allclose(g3.cpu().numpy(), np.float32(0.37) * g1.cpu().numpy(), rtol=2 * EPS)


@pytest.mark.gpu
def test_hip_distortion_argument_checks():
    """R = 0 succeeds without a launch; N = 0, N = 513, null pointers, non-contiguous and wrong-dtype tensors raise"""
    from refnerf_pl_amd import _hip
    _hip.require_device()
    up = torch.ones(1, device=DEV)

    def call(R, N):
        t, w = torch.zeros((R, N + 1), device=DEV), torch.zeros((R, N), device=DEV)
        return _hip.distortion_forward(t, w), _hip.distortion_backward(t, w, up)
    loss, g = call(0, 64)
    assert loss.shape == (0,) and g.shape == (0, 64)
    for N in (0, 513):
        with pytest.raises(ValueError, match=r"N outside \[1, 512\]"):
            call(3, N)
    lib = _hip.lib()
    t, w = torch.zeros((3, 9), device=DEV), torch.zeros((3, 8), device=DEV)
    out_l, out_g = torch.full((3,), 7.0, device=DEV), torch.full((3, 8), 7.0, device=DEV)
    p = lambda x: x.data_ptr()      # noqa: E731
    assert lib.refnerf_distortion_forward(None, p(w), 3, 8, p(out_l), None) == _hip.EINVAL
    assert lib.refnerf_distortion_forward(p(t), None, 3, 8, p(out_l), None) == _hip.EINVAL
    assert lib.refnerf_distortion_forward(p(t), p(w), 3, 8, None, None) == _hip.EINVAL
    assert "null pointer" in lib.refnerf_last_error().decode()
    assert lib.refnerf_distortion_backward(p(t), p(w), None, 3, 8, p(out_g), None) == _hip.EINVAL
    assert lib.refnerf_distortion_backward(p(t), p(w), p(up), 3, 8, None, None) == _hip.EINVAL
    assert lib.refnerf_distortion_forward(p(t), p(w), -1, 8, p(out_l), None) == _hip.EINVAL
    assert lib.refnerf_distortion_backward(p(t), p(w), p(up), 3, 513, p(out_g), None) == _hip.EINVAL
    assert lib.refnerf_distortion_forward(None, None, 0, 8, None, None) == _hip.OK       # R == 0: nothing is read
    torch.cuda.synchronize()
    assert bool((out_l == 7.0).all()) and bool((out_g == 7.0).all())                     # nothing was launched
    with pytest.raises(ValueError, match="is not contiguous"):
        _hip.distortion_forward(torch.zeros((9, 3), device=DEV).t(), w)
    with pytest.raises(ValueError, match="torch.float64"):
        _hip.distortion_forward(t.double(), w)
    with pytest.raises(ValueError, match=r"has shape \(3, 8\), not \(3, 9\)"):
        _hip.distortion_forward(w, w)
    with pytest.raises(ValueError, match="is not on a HIP device"):
        _hip.distortion_backward(t, w, torch.ones(1))
    with pytest.raises(ValueError, match="t \\[R, N\\+1\\] and w \\[R, N\\]"):
        _hip.distortion_forward(t, w.reshape(-1))


# ------------------------------------------------------------------------------------------- GPU: end to end
@pytest.mark.gpu
def test_hip_distortion_loss_end_to_end(monkeypatch):
    """The two-level proposal model of the propmlp_interlevel fixture (12 rays, 48 proposal and 64 final intervals).
    Flag off: training_losses is bit-equal to a config whose field was never touched.  Flag on: losses['distortion'] is the
    last key, within the bar of mult x the mean of the float64 definition on ray_history[-1], its gradient to the last
    level's weights within the bar of the float64 gradient, total.backward() leaves finite parameter gradients that differ
    from the flag-off ones, and the fused and the ATen paths agree within the sum of their bounds.
    The mean adds R - 1 additions, a division and the multiplier's product to the per-ray values: (R + 4) eps32 on top of
    the bar for the value, 8 eps32 for the gradient (the upstream scalar's three roundings and its product).  The ATen
    path's bound is the bar (its sums) plus eps32 max|t| (sum w)^2 per ray: each rounded midpoint is within eps32 / 2 max|t|
    of the true one, so each |u_i - u_j| within eps32 max|t|."""
    from refnerf_pl_amd import _hip, models, train_utils, utils
    from test_geometry_losses import _propmlp_setup
    from test_proposal_fused import _flat_grads
    _hip.require_device()
    g = load_golden("propmlp_interlevel")
    from helpers import params_from_golden, rays_from_golden
    cfg, prop = _propmlp_setup(g)
    cfg.hip_check_finite = False
    assert cfg.hip_distortion_loss is False
    mult = 0.01
    assert cfg.distortion_loss_mult == mult
    model = models.construct_model(utils.dummy_rays(), cfg).to(DEV).train()
    model.nerf_mlp.load_flat_params(params_from_golden(g))
    model.prop_mlp.load_flat_params(prop)
    rays = utils.rays_from_dict(rays_from_golden(g), DEV)
    batch = utils.Batch(rays=rays, rgb=np.asarray(g["gt_rgb"], np.float32))
    calls = []
    real_f, real_b = _hip.distortion_forward, _hip.distortion_backward
    monkeypatch.setattr(_hip, "distortion_forward", lambda *a: (calls.append("f"), real_f(*a))[1])
    monkeypatch.setattr(_hip, "distortion_backward", lambda *a: (calls.append("b"), real_b(*a))[1])

    def step():
        for prm in model.parameters():
            prm.grad = None
        torch.manual_seed(0)
        total, losses, _, aux = train_utils.training_losses(model, batch, rays, cfg, global_step=cfg.max_steps // 2)
        return total, losses, aux

    total_0, losses_0, _ = step()                      # the field never touched
    total_0.backward()
    grads_0 = np.concatenate([_flat_grads(model.nerf_mlp), _flat_grads(model.prop_mlp)])
    cfg.hip_distortion_loss = False
    total_off, losses_off, _ = step()
    assert list(losses_off) == list(losses_0) and "distortion" not in losses_0 and not calls
    assert torch.equal(total_off, total_0) and all(torch.equal(losses_off[k], losses_0[k]) for k in losses_0)

    cfg.hip_distortion_loss = True
    total_on, losses_on, aux = step()
    assert list(losses_on) == list(losses_0) + ["distortion"] and calls == ["f"]
    assert all(torch.equal(losses_on[k], losses_0[k]) for k in losses_0)
    last = aux["ray_history"][-1]
    assert train_utils.fused_distortion_supported(aux["ray_history"]) and last["weights"].requires_grad
    t, w = last["sdist"].detach().cpu().numpy(), last["weights"].detach().cpu().numpy()
    R, N = w.shape
    assert (R, N) == (12, 64) and (np.diff(t, axis=-1) >= 0).all()
    l64, g64 = DC.truth(t, w)
    want = mult * l64.mean()
    got = float(losses_on["distortion"].detach())
    bar_value = (DC.bound(N) + (R + 4) * EPS) * want
    print(f"end to end: distortion {got:.9e}, float64 {want:.9e}, rel {abs(got - want) / want:.2e}, bar {DC.bound(N) + (R + 4) * EPS:.2e}")
    assert want > 0 and abs(got - want) <= bar_value
    (gw,) = torch.autograd.grad(losses_on["distortion"], last["weights"], retain_graph=True)
    assert calls == ["f", "b"]
    want_g = mult / R * g64
    rg = _rel(gw.cpu().numpy(), want_g)
    print(f"end to end: grad to the weights rel {rg.max():.2e}, bar {DC.bound(N) + 8 * EPS:.2e}")
    assert rg.max() <= DC.bound(N) + 8 * EPS
    total_on.backward()
    grads_on = np.concatenate([_flat_grads(model.nerf_mlp), _flat_grads(model.prop_mlp)])
    assert np.isfinite(grads_on).all() and np.abs(grads_on - grads_0).max() > 0
    # the ATen path on the same history
    aten = float(train_utils.distortion_loss(aux["ray_history"], cfg).detach())
    aten_bound = mult * float(np.mean(DC.bound(N) * l64 + EPS * np.abs(t).max(-1) * w.astype(np.float64).sum(-1) ** 2)) + (R + 4) * EPS * want
    print(f"end to end: ATen {aten:.9e} ({abs(aten - want) / want:.2e} from float64), fused {got:.9e}; bounds {aten_bound / want:.2e} + {bar_value / want:.2e}")
    assert abs(aten - want) <= aten_bound
    assert abs(got - aten) <= aten_bound + bar_value


@pytest.mark.gpu
def test_hip_distortion_falls_back_to_aten_beyond_512_intervals(monkeypatch):
    """compute_losses takes the fused path where it is supported and the ATen definition otherwise (N = 513 on the device)"""
    from refnerf_pl_amd import _hip, configs, train_utils
    _hip.require_device()
    configs.clear_config()
    cfg = configs.Config(hip_distortion_loss=True)
    t, w = DC.rows("random", 3, 513, 5)
    hist = [dict(sdist=torch.tensor(t, device=DEV), weights=torch.tensor(w, device=DEV).requires_grad_(True))]
    assert not train_utils.fused_distortion_supported(hist)
    l64, _ = DC.truth(t, w)
    got = float(train_utils.distortion_loss(hist, cfg).detach())
    assert got == pytest.approx(cfg.distortion_loss_mult * l64.mean(), rel=1e-4)
    t, w = t[:, :513], w[:, :512]
    hist = [dict(sdist=torch.tensor(t, device=DEV), weights=torch.tensor(w, device=DEV).requires_grad_(True))]
    assert train_utils.fused_distortion_supported(hist)
    fused = train_utils.fused_distortion_loss(hist, cfg)
    l64, g64 = DC.truth(t, w)
    assert float(fused.detach()) == pytest.approx(cfg.distortion_loss_mult * l64.mean(), rel=DC.bound(512) + 8 * EPS)
    fused.backward()
    assert _rel(hist[0]["weights"].grad.cpu().numpy(), cfg.distortion_loss_mult / 3 * g64).max() <= DC.bound(512) + 8 * EPS

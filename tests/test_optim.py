"""The optimiser step: LR schedule, create_optimizer, ClippedAdam (CPU restatement and the HIP kernels of
csrc/refnerf_optim.h) against fixtures captured from the reference (tests/golden/make_golden_optim.py).

The per-element bar of the synthetic trajectories after step k (1-based), against the reference's float64 run:
    k * (2^-24 |p| + 2^-17 lr_init)
half an ulp of the stored parameter per step, plus eight fp32 roundings on an update bounded by lr.  torch's own float32
run of the recipe stays below 0.2 of it (printed by make_golden_optim.py)."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import load_golden

import refnerf_pl_amd  # noqa: F401
from refnerf_pl_amd import configs, layout, optim, synthetic, train_utils

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS = list(synthetic.OPTIM_CLIPS)
TRAJ_KEYS = ("lr_init", "lr_final", "max_steps", "lr_delay_steps", "lr_delay_mult", "adam_beta1", "adam_beta2", "adam_eps")


@pytest.fixture(scope="module")
def G():
    return load_golden("optim")


@pytest.fixture(scope="module")
def hip():
    from refnerf_pl_amd import _hip
    _hip.require_device()          # fails loudly: no fallback
    return _hip


def traj_config(G, clip):
    configs.clear_config()
    cfg = configs.Config()
    for k, v in zip(TRAJ_KEYS, G["traj_config"]):
        setattr(cfg, k, int(v) if k in ("max_steps", "lr_delay_steps") else float(v))
    cfg.grad_max_val, cfg.grad_max_norm, _ = synthetic.OPTIM_CLIPS[clip]
    return cfg


def bar(G, k, p64):
    return k * (2.0 ** -24 * np.abs(p64) + 2.0 ** -17 * float(G["traj_config"][0]))


def seg_offsets(n):
    return np.concatenate([[0], np.cumsum(synthetic.OPTIM_SEGMENTS)]).tolist() if n == synthetic.OPTIM_N else [0, n]


def run_synthetic(G, n, clip, device, flat, offset_view=False):
    """The fixture's recipe through create_optimizer; returns (params [K, len(idx)], lr [K], stats per step)."""
    cfg = traj_config(G, clip)
    scale = synthetic.OPTIM_CLIPS[clip][2]
    off = seg_offsets(n)
    names = [f"seg{i}" for i in range(len(off) - 1)]
    p0 = torch.tensor(synthetic.optim_params(n), device=device)
    if offset_view:                # base pointer one element past a 16-byte boundary
        buf = torch.zeros(n + 1, device=device)
        buf[1:] = p0
        p0 = buf[1:]
        assert p0.data_ptr() % 16 == 4
    if flat:
        blob = p0.requires_grad_(True) if offset_view else p0.clone().requires_grad_(True)
        params = [blob]
        opt = optim.ClippedAdam(params, lr=cfg.lr_init, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_eps,
                                grad_max_val=cfg.grad_max_val, grad_max_norm=cfg.grad_max_norm, segments={id(blob): (names, off)})
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: train_utils.learning_rate_decay(
            s, cfg.lr_init, cfg.lr_final, cfg.max_steps, cfg.lr_delay_steps, cfg.lr_delay_mult))
    else:
        params = [t.clone().requires_grad_(True) for t in torch.split(p0, list(np.diff(off)))]
        opt, sched = train_utils.create_optimizer(cfg, params)
        names = [str(i) for i in range(len(params))]
    idx = torch.tensor(G[f"{n}_{clip}_idx"].astype(np.int64), device=device)
    out_p, out_lr, out_stats = [], [], []
    for k in range(synthetic.OPTIM_STEPS):
        g = synthetic.optim_gradient(n, k, scale)
        assert np.array_equal(g[:8], G[f"{n}_{clip}_grad_check"][k][:len(g[:8])]), "the gradient generator moved"
        gt = torch.tensor(g, device=device)
        if offset_view:            # the gradient one element off the boundary as well
            gb = torch.zeros(n + 1, device=device)
            gb[1:] = gt
            gt = gb[1:]
        for p, gs in zip(params, torch.split(gt, [p.numel() for p in params])):
            p.grad = gs if offset_view else gs.clone()
        out_lr.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        st = opt.stats()
        out_stats.append(dict(total_norm=st["total_norm"].clone(), clip_coef=st["clip_coef"].clone(),
                              **{key: torch.stack([st[key][nm] for nm in names]) for key in ("grad_norms", "grad_maxes", "weights_l2s")}))
        out_p.append(torch.cat([p.detach().reshape(-1) for p in params])[idx].clone())
    P = torch.stack(out_p).cpu().numpy().astype(np.float64)
    S = {key: np.stack([s[key].cpu().numpy().astype(np.float64) for s in out_stats]) for key in out_stats[0]}
    return P, np.array(out_lr), S


def check_synthetic(G, n, clip, P, lr, S, label):
    c = f"{n}_{clip}"
    p64 = G[c + "_p64"]
    np.testing.assert_allclose(lr, G[c + "_lr"], rtol=1e-12)
    worst = 0.0
    for k in range(1, synthetic.OPTIM_STEPS + 1):
        frac = np.abs(P[k - 1] - p64[k - 1]) / bar(G, k, p64[k - 1])
        worst = max(worst, float(frac.max()))
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))  # noqa: E731
    figures = dict(param_bar_fraction=worst, total_norm=rel(S["total_norm"], G[c + "_total_norm"]),
                   grad_norms=rel(S["grad_norms"], G[c + "_grad_norms"]), weights_l2s=rel(S["weights_l2s"], G[c + "_weights_l2s"]))
    print(f"[{label} {c}] " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert worst <= 1.0, f"{label} {c}: parameters at {worst:.2f} of the bar"
    assert figures["total_norm"] <= 1e-6 and figures["grad_norms"] <= 1e-6 and figures["weights_l2s"] <= 1e-6, figures
    assert np.array_equal(S["grad_maxes"], G[c + "_grad_maxes"]), f"{label} {c}: grad_maxes are not exact"
    # clip_coef takes the value 1 on the small-gradient steps and values below 1 on the others (where the norm clip is on)
    want = np.minimum(1.0, synthetic.OPTIM_CLIPS[clip][1] / (G[c + "_total_norm"] + 1e-6)) if synthetic.OPTIM_CLIPS[clip][1] > 0 else np.ones(8)
    np.testing.assert_allclose(S["clip_coef"], want, rtol=2e-6)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_schedule_matches_the_reference(G):
    for case in G["sched_cases"]:
        lr_init, lr_final, max_steps, delay_steps, delay_mult = G[f"sched_{case}_kw"]
        got = [train_utils.learning_rate_decay(int(s), lr_init, lr_final, int(max_steps), int(delay_steps), delay_mult)
               for s in G[f"sched_{case}_steps"]]
        np.testing.assert_allclose(np.array(got, np.float64), G[f"sched_{case}"], rtol=1e-12, atol=0)
    assert {"blender", "llff", "nodelay"} <= set(str(c) for c in G["sched_cases"])


def test_log_lerp_rejects_non_positive_interpolants():
    for v0, v1 in ((0.0, 1.0), (-1e-3, 1.0), (1.0, 0.0)):
        with pytest.raises(ValueError):
            train_utils.log_lerp(0.5, v0, v1)
    assert train_utils.log_lerp(0.5, 1e-2, 1e-4) == pytest.approx(1e-3, rel=1e-12)


def test_create_optimizer_carries_the_configured_hyper_parameters(G):
    cfg = traj_config(G, "val_norm")
    params = [torch.zeros(5, requires_grad=True), torch.zeros(3, requires_grad=True)]
    opt, sched = train_utils.create_optimizer(cfg, params)
    assert isinstance(opt, torch.optim.Optimizer) and isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    g = opt.param_groups[0]
    assert g["betas"] == (cfg.adam_beta1, cfg.adam_beta2) and g["eps"] == cfg.adam_eps
    assert g["grad_max_val"] == cfg.grad_max_val == 1e-3 and g["grad_max_norm"] == cfg.grad_max_norm == 1e-3
    lrs = []
    for _ in range(synthetic.OPTIM_STEPS):
        lrs.append(opt.param_groups[0]["lr"])
        for p in params:
            p.grad = torch.ones_like(p)
        opt.step()
        sched.step()
    np.testing.assert_allclose(lrs, G[f"{synthetic.OPTIM_N}_val_norm_lr"], rtol=1e-12)
    unclipped, _ = train_utils.create_optimizer(cfg, params, fused_clipping=False)
    assert unclipped.param_groups[0]["grad_max_val"] == 0.0 and unclipped.param_groups[0]["grad_max_norm"] == 0.0
    configs.clear_config()


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "tensors"])
@pytest.mark.parametrize("n", [synthetic.OPTIM_N, 1, 3])
def test_cpu_path_follows_the_reference_trajectory(G, n, flat):
    for clip in CLIPS:
        P, lr, S = run_synthetic(G, n, clip, "cpu", flat)
        check_synthetic(G, n, clip, P, lr, S, "cpu")
    configs.clear_config()


def test_a_torch_adam_state_dict_loads_and_continues():
    n, lr, eps, max_norm = 1021, 1e-3, 1e-6, 1e-3
    mk = lambda: [torch.tensor(synthetic.optim_params(n)).requires_grad_(True), torch.tensor(synthetic.optim_params(7, seed=5)).requires_grad_(True)]  # noqa: E731
    ref_p, new_p = mk(), mk()
    ref = torch.optim.Adam(ref_p, lr=lr, eps=eps)

    def grads(ps, k):
        for j, p in enumerate(ps):
            p.grad = torch.tensor(synthetic.optim_gradient(p.numel(), k, seed=20 + j))

    def ref_step(k):
        grads(ref_p, k)
        torch.nn.utils.clip_grad_norm_(ref_p, max_norm=max_norm)
        ref.step()
    for k in range(3):
        ref_step(k)
    new = optim.ClippedAdam(new_p, lr=lr, eps=eps, grad_max_norm=max_norm)
    with torch.no_grad():
        for a, b in zip(new_p, ref_p):
            a.copy_(b)
    new.load_state_dict(copy.deepcopy(ref.state_dict()))      # (a checkpoint; torch shares a live state_dict's tensors)
    assert set(new.state[new_p[0]]) == {"step", "exp_avg", "exp_avg_sq"} and float(new.state[new_p[0]]["step"]) == 3.0
    assert new.param_groups[0]["grad_max_norm"] == max_norm
    for k in range(3, 6):
        ref_step(k)
        grads(new_p, k)
        new.step()
    for a, b in zip(new_p, ref_p):
        assert float(new.state[a]["step"]) == 6.0
        assert np.all(np.abs(a.detach().numpy() - b.detach().numpy()) <= 3 * (2.0 ** -24 * np.abs(b.detach().numpy()) + 2.0 ** -17 * lr))
    # and back: torch.optim.Adam reads what ClippedAdam wrote
    back = torch.optim.Adam(mk(), lr=lr, eps=eps)
    back.load_state_dict(copy.deepcopy(new.state_dict()))
    assert float(back.state[back.param_groups[0]["params"][0]]["step"]) == 6.0


def test_segments_must_tile_the_tensor():
    p = torch.zeros(10, requires_grad=True)
    for off in ([0, 5, 5, 10], [1, 10], [0, 9], [0, 6, 4, 10]):
        with pytest.raises(ValueError):
            optim.ClippedAdam([p], segments={id(p): ([str(i) for i in range(len(off) - 1)], off)})


def test_create_optimizer_on_a_model_with_its_own_prop_mlp():
    """Model.single_mlp = False (the reference's constructor default; the shipped configs share one MLP): two distinct
    MLPs.  Flat mode steps two blobs cut at each MLP's layers, per-tensor mode every parameter of both; the statistics carry
    the reference's names, `prop_mlp/...` and `nerf_mlp/...`; one CPU step runs the global norm over both."""
    from refnerf_pl_amd import models, utils
    gin_file = os.path.join(ROOT, "configs", "refnerf_blender.gin")
    # the proposal MLP as a second Ref-NeRF network: the shipped NerfMLP bindings, said again for PropMLP
    prop = [ln.replace("NerfMLP.", "PropMLP.", 1).strip() for ln in open(gin_file) if ln.startswith("NerfMLP.")]
    for flat in (True, False):
        configs.clear_config()
        configs.parse_config_files_and_bindings([gin_file], ["Model.single_mlp = False"] + prop +
                                                (["Config.hip_flat_grads = True"] if flat else []))
        cfg = configs.Config()
        model = models.construct_model(utils.dummy_rays(), cfg)
        assert model.prop_mlp is not model.nerf_mlp
        opt, _ = train_utils.create_optimizer(cfg, model)
        params = opt.param_groups[0]["params"]
        n_layers = len(model.nerf_mlp.specs)
        if flat:
            assert len(params) == 2 and params[0] is model.prop_mlp.flat_parameter() and params[1] is model.nerf_mlp.flat_parameter()
            names, off = opt._segments[id(params[0])]
            assert names[:2] == ["prop_mlp/spatial_net/0/weight", "prop_mlp/spatial_net/0/bias"] and len(names) == 2 * n_layers
            spec = model.prop_mlp.specs[0]
            assert off[:3] == [0, spec.b_off, spec.b_off + spec.out_dim] and off[-1] == model.prop_mlp.num_params == params[0].numel()
        else:
            assert len(params) == len(list(model.parameters())) == 4 * n_layers
        for j, p in enumerate(params):
            p.grad = torch.tensor(synthetic.optim_gradient(p.numel(), 0, seed=40 + j)).reshape(p.shape)
        want = torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1).double() for p in params]))
        before = [p.detach().clone() for p in params]
        opt.step()
        st = opt.stats()
        want_names = {k.replace(".", "/") for k, _ in model.named_parameters()}
        assert set(st["grad_norms"]) == set(st["grad_maxes"]) == set(st["weights_l2s"]) == want_names
        assert any(k.startswith("prop_mlp/") for k in want_names) and any(k.startswith("nerf_mlp/") for k in want_names)
        assert float(st["total_norm"]) == pytest.approx(float(want), rel=1e-6) and float(st["clip_coef"]) < 1.0
        assert all(not torch.equal(a, b.detach()) for a, b in zip(before, params))
        w = model.prop_mlp.spatial_net[0].weight
        assert float(st["grad_maxes"]["prop_mlp/spatial_net/0/weight"]) == float(
            (params[0].grad[:w.numel()] if flat else w.grad).abs().max())
    configs.clear_config()


def test_add_param_group_after_construction():
    a, b = torch.zeros(5, requires_grad=True), torch.ones(7, requires_grad=True)
    opt = optim.ClippedAdam([a], lr=1e-2, grad_max_norm=1e-3)
    a.grad = torch.full((5,), 1e-2)
    opt.step()
    opt.add_param_group(dict(params=[b]))
    a.grad, b.grad = torch.full((5,), 1e-2), torch.full((7,), -1e-2)
    opt.step()
    assert set(opt.stats()["grad_norms"]) == {"0", "1"} and float(b.detach().max()) > 1.0 and float(opt.state[b]["step"]) == 1.0


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_adam_kernel_head_and_tail_on_a_shared_odd_phase(hip):
    """Parameter, gradient, exp_avg and exp_avg_sq all one element past a 16-byte boundary (`[1:]` views, as a checkpoint's
    state laid out beside its blob would be): the Adam kernel takes its float4 body with a 3-element scalar head and a
    scalar tail (n = 4102 = 3 + 4 * 1024 + 3).  Eight steps against the CPU restatement from the same inputs, within the
    sum of both sides' bars (each is fp32 within k (2^-24 |p| + 2^-17 lr) of the exact result); the moments within fp32
    rounding of the gradients they average.  Then the clip alone
    (no_step, written back) on such a gradient."""
    n, lr = 4102, 2e-3
    view = lambda x: torch.cat([torch.zeros(1), x]).to(DEV)[1:]  # noqa: E731
    p0 = torch.tensor(synthetic.optim_params(n))
    dev_p, cpu_p = view(p0).requires_grad_(True), p0.clone().requires_grad_(True)
    assert dev_p.data_ptr() % 16 == 4
    kw = dict(lr=lr, eps=1e-6, grad_max_val=0.1, grad_max_norm=1e-3)
    dev_opt, cpu_opt = optim.ClippedAdam([dev_p], **kw), optim.ClippedAdam([cpu_p], **kw)
    dev_opt.state[dev_p] = dict(step=torch.tensor(0.0), exp_avg=view(torch.zeros(n)), exp_avg_sq=view(torch.zeros(n)))
    assert dev_opt.state[dev_p]["exp_avg"].data_ptr() % 16 == 4 and dev_opt.state[dev_p]["exp_avg_sq"].data_ptr() % 16 == 4
    for k in range(1, synthetic.OPTIM_STEPS + 1):
        g = torch.tensor(synthetic.optim_gradient(n, k - 1))
        dev_p.grad, cpu_p.grad = view(g), g.clone()
        dev_opt.step()
        cpu_opt.step()
        a, b = dev_p.detach().cpu().numpy().astype(np.float64), cpu_p.detach().numpy().astype(np.float64)
        assert np.all(np.abs(a - b) <= 2 * k * (2.0 ** -24 * np.abs(b) + 2.0 ** -17 * lr)), k
        # the moments: m + (1 - b1)(g - m) cancels, so its rounding is relative to the largest clipped gradient the element
        # has seen, not to m: per step a subtraction, a product and a sum on each side, <= 8 half-ulps of 2 gmax between them
        ghat = (g.double().clamp(-0.1, 0.1) * float(cpu_opt.stats()["clip_coef"])).abs().numpy()
        gmax = ghat if k == 1 else np.maximum(gmax, ghat)
        for key, scale in (("exp_avg", gmax), ("exp_avg_sq", gmax * gmax)):
            d = np.abs(dev_opt.state[dev_p][key].cpu().numpy().astype(np.float64) - cpu_opt.state[cpu_p][key].numpy())
            assert np.all(d <= k * 8 * 2.0 ** -24 * scale), (key, k, float((d / scale).max()))
    assert np.abs(dev_p.detach().cpu().numpy() - p0.numpy()).max() > 1e-4
    # head (0..2), body and tail (4099..4101) all moved
    moved = dev_p.detach().cpu().numpy() != p0.numpy()
    assert moved[:3].all() and moved[-3:].all() and moved.mean() > 0.99
    cfg = configs.Config()
    cfg.grad_max_val, cfg.grad_max_norm = 0.1, 1e-3
    g = torch.tensor(synthetic.optim_gradient(n, 0))
    q = view(torch.zeros(n)).requires_grad_(True)
    q.grad = view(g)
    assert q.grad.data_ptr() % 16 == 4
    clipper = train_utils.clip_gradients([q], cfg)
    c = g.double().clamp(-0.1, 0.1)
    coef = min(1.0, 1e-3 / (float(torch.linalg.vector_norm(c)) + 1e-6))
    np.testing.assert_allclose(q.grad.cpu().numpy(), (c * coef).numpy(), rtol=3e-7)
    assert float(clipper.stats()["clip_coef"]) == pytest.approx(coef, rel=1e-6) and coef < 1.0
    configs.clear_config()


@pytest.mark.gpu
@pytest.mark.parametrize("clip", CLIPS)
def test_kernels_follow_the_reference_trajectory(hip, G, clip):
    """N = 70 003 in 9 unaligned segments (1 .. 32 103 elements: several work items per segment and one-element segments),
    as ONE flat tensor with the segment table and as 9 tensors; flat vs tensors within the same bar; two runs bit-equal."""
    n = synthetic.OPTIM_N
    Pf, lr, Sf = run_synthetic(G, n, clip, DEV, flat=True)
    check_synthetic(G, n, clip, Pf, lr, Sf, "flat")
    Pt, lr, St = run_synthetic(G, n, clip, DEV, flat=False)
    check_synthetic(G, n, clip, Pt, lr, St, "tensors")
    for k in range(1, synthetic.OPTIM_STEPS + 1):
        assert np.all(np.abs(Pf[k - 1] - Pt[k - 1]) <= bar(G, k, G[f"{n}_{clip}_p64"][k - 1]))
    P2, _, S2 = run_synthetic(G, n, clip, DEV, flat=True)
    assert np.array_equal(Pf, P2) and all(np.array_equal(Sf[k], S2[k]) for k in Sf), "two identical runs differ"
    configs.clear_config()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_kernels_on_tiny_tensors(hip, G, n):
    for clip in CLIPS:
        P, lr, S = run_synthetic(G, n, clip, DEV, flat=True)
        check_synthetic(G, n, clip, P, lr, S, "flat")
    configs.clear_config()


@pytest.mark.gpu
def test_kernels_on_a_tensor_one_element_off_a_16_byte_boundary(hip, G):
    for clip in ("val_norm", "tiny"):
        P, lr, S = run_synthetic(G, synthetic.OPTIM_N, clip, DEV, flat=True, offset_view=True)
        check_synthetic(G, synthetic.OPTIM_N, clip, P, lr, S, "offset")
    configs.clear_config()


@pytest.mark.gpu
def test_real_layout_one_step_against_torch(hip):
    """REFNERF_NUM_PARAMS elements cut at layout.PARAM_SPECS (46 segments), one step with both clips against
    clip_grad_value_ + clip_grad_norm_ + torch.optim.Adam on the same device tensors.  Both sides are fp32 within the
    one-step bar of the exact result, so they are within twice that bar of each other."""
    n, lr, eps, val, max_norm = layout.NUM_PARAMS, 2e-3, 1e-6, 1e-4, 1e-3
    assert n == hip.NUM_PARAMS
    gen = torch.Generator(device=DEV).manual_seed(7)
    p = torch.tensor(synthetic.make_params(seed=4, bias_scale=0.05), device=DEV)
    g = torch.randn(n, device=DEV, generator=gen) * 1e-4
    names, off = [], []
    for spec in layout.PARAM_SPECS:
        names += [spec.name + "/weight", spec.name + "/bias"]
        off += [spec.w_off, spec.b_off]
    off.append(n)
    mine = p.clone().requires_grad_(True)
    mine.grad = g.clone()
    opt = optim.ClippedAdam([mine], lr=lr, eps=eps, grad_max_val=val, grad_max_norm=max_norm, segments={id(mine): (names, off)})
    opt.step()
    theirs = p.clone().requires_grad_(True)
    theirs.grad = g.clone()
    torch.nn.utils.clip_grad_value_([theirs], clip_value=val)
    tn = torch.nn.utils.clip_grad_norm_([theirs], max_norm=max_norm)
    torch.optim.Adam([theirs], lr=lr, eps=eps).step()
    a, b = mine.detach().cpu().numpy().astype(np.float64), theirs.detach().cpu().numpy().astype(np.float64)
    assert np.abs(a - p.cpu().numpy()).max() > 1e-4, "the step did not move the parameters"
    assert np.all(np.abs(a - b) <= 2 * (2.0 ** -24 * np.abs(b) + 2.0 ** -17 * lr))
    st = opt.stats()
    assert float(st["total_norm"]) == pytest.approx(float(tn), rel=2e-6) and float(st["clip_coef"]) < 1.0
    g64, p64 = g.double(), p.double()
    for i, nm in enumerate(names):
        lo, hi = off[i], off[i + 1]
        assert float(st["grad_norms"][nm]) == pytest.approx(float(g64[lo:hi].norm()), rel=1e-6)
        assert float(st["weights_l2s"][nm]) == pytest.approx(float((p64[lo:hi] ** 2).sum()), rel=1e-6, abs=1e-30)
        assert float(st["grad_maxes"][nm]) == float(g[lo:hi].abs().max())


@pytest.mark.gpu
def test_clip_gradients_alone_and_nan_propagation(hip):
    cfg = configs.Config()
    cfg.grad_max_val, cfg.grad_max_norm = 1e-3, 1e-3
    ps = [torch.zeros(n, device=DEV, requires_grad=True) for n in (5, 4099)]
    for j, p in enumerate(ps):
        p.grad = torch.tensor(synthetic.optim_gradient(p.numel(), 0, seed=30 + j), device=DEV)
    want = [p.grad.clone() for p in ps]
    for w in want:
        w.clamp_(-1e-3, 1e-3)
    tn = torch.linalg.vector_norm(torch.cat(want).double())
    coef = min(1.0, 1e-3 / (float(tn) + 1e-6))
    clipper = train_utils.clip_gradients(ps, cfg)
    for p, w in zip(ps, want):
        np.testing.assert_allclose(p.grad.cpu().numpy(), (w.double() * coef).cpu().numpy(), rtol=3e-7)
        assert float(p.detach().abs().max()) == 0.0               # no step
    assert float(clipper.stats()["total_norm"]) == pytest.approx(float(tn), rel=1e-6)
    # a NaN gradient: grad_max is NaN (not dropped), the norm is NaN, and it reaches the parameters as in torch
    q = torch.ones(300, device=DEV, requires_grad=True)
    q.grad = torch.full((300,), 1e-3, device=DEV)
    q.grad[17] = float("nan")
    opt = optim.ClippedAdam([q], grad_max_norm=1e-3, names={id(q): "q"})
    opt.step()
    st = opt.stats()
    assert np.isnan(float(st["grad_maxes"]["q"])) and np.isnan(float(st["total_norm"])) and np.isnan(float(st["clip_coef"]))
    assert bool(torch.isnan(q).all())
    configs.clear_config()


@pytest.mark.gpu
def test_bad_arguments_raise_value_error(hip):
    for n, off in ((10, [0, 5, 5, 10]), (10, [1, 10]), (10, [0, 9]), (0, [0, 0]), (10, [0, 6, 4, 10]), (2, [0, 1, 2, 3])):
        with pytest.raises(ValueError):
            hip.optim_plan(n, off, DEV)
    ws, seg_stats, n_items = hip.optim_plan(10, [0, 4, 10], DEV)
    assert n_items == 2
    state = hip.optim_state(1, DEV)
    g, p = torch.zeros(10, device=DEV), torch.zeros(10, device=DEV)
    with pytest.raises(ValueError):
        hip.optim_stats(g, p, 2, n_items, 0.0, ws, seg_stats, state, 1)          # slot outside the state
    with pytest.raises(ValueError):
        hip.optim_stats(g, p, 2, 99, 0.0, ws, seg_stats, state, 0)               # not the plan's work-item count
    with pytest.raises(ValueError):
        hip.optim_stats(g, p[:9], 2, n_items, 0.0, ws, seg_stats, state, 0)      # sizes differ
    with pytest.raises(ValueError):
        hip.optim_stats(g, p, 2, n_items, 0.0, ws[:16], seg_stats, state, 0)     # workspace too small
    with pytest.raises(ValueError):
        hip.optim_finalize(state, 2, 1e-3)
    with pytest.raises(ValueError):
        hip.optim_adam_step(None, g, None, None, hip.AdamCfg(no_step=0, write_grad=0), state)   # null pointers
    with pytest.raises(ValueError):
        hip.optim_adam_step(p, g.double(), g, g, hip.AdamCfg(bias_correction1=0.1, sqrt_bias_correction2=0.1), state)
    q = torch.zeros(8, device=DEV, dtype=torch.float64, requires_grad=True)
    q.grad = torch.zeros_like(q)
    with pytest.raises(ValueError):
        optim.ClippedAdam([q]).step()                                             # no eager fall-back on a device


def _model(bindings, blob=None):
    from refnerf_pl_amd import models, utils
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "refnerf_blender.gin")], bindings)
    cfg = configs.Config()
    model = models.construct_model(utils.dummy_rays(), cfg).to(DEV)
    if blob is not None:
        model.nerf_mlp.load_flat_params(blob)
    return model, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "tensors"])
def test_step_through_create_optimizer_needs_no_mark_updated(hip, flat):
    """eval (caches the weight image), one training step through create_optimizer(cfg, model), eval again: the second eval
    runs on the new weights -- the same pixels as a twin model that was handed a copy of the stepped blob."""
    from refnerf_pl_amd import utils
    bindings = ["Model.num_prop_samples = 32", "Model.num_nerf_samples = 32"] + (["Config.hip_flat_grads = True"] if flat else [])
    init = synthetic.make_params(seed=3, bias_scale=0.0)
    model, cfg = _model(bindings, init)
    opt, sched = train_utils.create_optimizer(cfg, model)
    assert len(opt.param_groups[0]["params"]) == (1 if flat else 2 * len(layout.PARAM_SPECS))
    rd = synthetic.blender_rays(64, seed=2, center_frac=0.85)
    rays = utils.rays_from_dict(rd, DEV)
    model.eval()
    with torch.no_grad():
        before = model(rays, 1.0, True)[0][-1]["rgb"].clone()
    model.train()
    rend, hist = model(rays, 1.0, False)
    total, _, _ = train_utils.compute_losses(model, utils.Batch(rays=rays, rgb=synthetic.target_rgb(64, seed=5)), rays, rend, hist, cfg)
    total.backward()
    opt.param_groups[0]["lr"] = 1e-2                    # a step large enough to see in the pixels
    opt.step()
    assert not model.nerf_mlp._step_pending             # the post-hook has called mark_updated()
    model.eval()
    with torch.no_grad():
        after = model(rays, 1.0, True)[0][-1]["rgb"].clone()
    stepped = model.nerf_mlp.flat_params().detach().clone()
    assert float((stepped.cpu() - torch.tensor(init)).abs().max()) > 1e-3
    names = set(opt.stats()["grad_norms"])
    assert "nerf_mlp/spatial_net/0/weight" in names and "nerf_mlp/rgb/bias" in names and len(names) == 2 * len(layout.PARAM_SPECS)
    twin, _ = _model(bindings, stepped)
    twin.eval()
    with torch.no_grad():
        want = twin(rays, 1.0, True)[0][-1]["rgb"]
    assert torch.equal(after, want) and not torch.equal(after, before)
    configs.clear_config()


# measured on an MI355X against the reference fixture (worst of the 20 steps / after them; flat and per-tensor agree to 1 %):
#   f32 chains    total_norm 4.9e-5   update rel-L2 9.6e-5
#   f16x2 chains  total_norm 1.4e-5   update rel-L2 2.0e-4
# the bars are ~2x those (the unclipped trajectory's update bars are 1.5e-3 / 9e-3: clipping to norm 1e-3 is no worse)
E2E_BARS = {"f32": dict(total_norm=1e-4, update=2e-4), "f16x2": dict(total_norm=3e-5, update=4e-4)}


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "tensors"])
@pytest.mark.parametrize("chains", ["f32", "f16x2"])
def test_twenty_clipped_steps_follow_the_reference(hip, chains, flat):
    """The reference's whole loop -- forward, the three losses, backward, clip_grad_norm_(1e-3), Adam, LambdaLR with an
    8-step delay ramp and max_steps = 40 -- for 20 steps from the seeded init (tests/golden/trajectory_clipped.npz), against
    Model + create_optimizer here.  Per-step loss within 2e-5 relative (the unclipped trajectory test's bar), lr to 1e-12;
    total_norm per step and the accumulated update against E2E_BARS (measured: 4.9e-5 / 9.6e-5 with f32 chains, 1.4e-5 / 2.0e-4
    with f16x2 chains; loss deviation 3.3e-6 / 1.7e-6)."""
    from refnerf_pl_amd import utils
    g = load_golden("trajectory_clipped")
    steps, n_rays, n_samples, lr_init, eps, seed, delay, max_steps, max_norm, max_val = g["recipe"]
    model, cfg = _model([f"Model.num_prop_samples = {int(n_samples)}", f"Model.num_nerf_samples = {int(n_samples)}",
                         f"Config.hip_train_precision = '{chains}'", f"Config.hip_bwd_precision = '{chains}'",
                         f"Config.lr_delay_steps = {int(delay)}", f"Config.max_steps = {int(max_steps)}"] +
                        (["Config.hip_flat_grads = True"] if flat else []))
    assert (cfg.lr_init, cfg.adam_eps, cfg.grad_max_norm, cfg.grad_max_val) == (lr_init, eps, max_norm, max_val)
    model.train()
    init = synthetic.make_params(seed=int(seed), bias_scale=0.0)
    model.nerf_mlp.load_flat_params(init)
    opt, sched = train_utils.create_optimizer(cfg, model)
    norms, worst = [], 0.0
    for it in range(int(steps)):
        rays = utils.rays_from_dict(synthetic.blender_rays(int(n_rays), seed=9100 + it, center_frac=0.85), DEV)
        opt.zero_grad(set_to_none=True)
        rend, hist = model(rays, 1.0, False)
        total, terms, _ = train_utils.compute_losses(model, utils.Batch(rays=rays, rgb=g["gt_rgb"][it]), rays, rend, hist, cfg)
        total.backward()
        assert opt.param_groups[0]["lr"] == pytest.approx(g["lr"][it], rel=1e-12)
        opt.step()
        sched.step()
        norms.append(opt.stats()["total_norm"].clone())
        rel = abs(float(total.detach()) - g["loss_total"][it]) / g["loss_total"][it]
        worst = max(worst, rel)
        assert rel < 2e-5, (it, float(total.detach()), g["loss_total"][it])
    norms = torch.stack(norms).cpu().numpy().astype(np.float64)
    rel_n = float(np.max(np.abs(norms - g["total_norm"]) / g["total_norm"]))
    upd = (model.nerf_mlp.flat_params().detach().cpu().numpy() - init)[::97]
    rel_u = float(np.linalg.norm(upd - g["update_sub"]) / np.linalg.norm(g["update_sub"]))
    print(f"[{chains} chains, flat={flat}] worst per-step loss deviation {worst:.2e}; total_norm worst rel {rel_n:.2e}; "
          f"accumulated update vs the reference's: rel-L2 {rel_u:.2e}")
    bars = E2E_BARS[chains]
    assert rel_n < bars["total_norm"] and rel_u < bars["update"], (rel_n, rel_u)
    configs.clear_config()

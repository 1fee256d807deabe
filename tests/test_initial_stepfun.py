"""The implicit initial step function and the per-ray outputs Model.__call__ hands on without ATen glue.

Level 0 of every Model.__call__ resamples the step function [s_near, s_far] with weight 1.  The level entries take NULL for
it and the resampler then uses its closed form, centre k = s_near + u_k (s_far - s_near): the softmax of a single
logit is exactly 1, the CDF {0, 1}, (u - 0) / (1 - 0) = u, so the general path ends in the same expression on the same
values.  The CPU test holds the closed form against the oracle's sampler, the GPU tests hold the implicit launch against the
explicit one bit for bit, in every kernel family that shares `resample_phase`; then the two new outputs of the compositing
phase (`refnerf_level_out_extra`: `d_r_percentiles_soa`, `d_r_rgb_fg`) and what they are for: an eval step that launches the
two level kernels only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from refnerf_pl_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, BF16, F16X2 = 0, 1, 3
_BLOB = synthetic.make_params(seed=0, bias_scale=0.05, sharpen=20.0)
_RAYS = synthetic.blender_rays(2048, seed=21, center_frac=0.5)
_packed = {}


def _clip01(x):
    return np.minimum(np.maximum(x, np.float32(0)), np.float32(1))


@pytest.mark.parametrize("near,far", [(0.0, 1.0), (0.25, 0.75)])
@pytest.mark.parametrize("N", [2, 3, 16, 72, 128, 192, 256])
def test_closed_form_is_the_oracle_sampler_on_one_interval(N, near, far):
    """CPU.  The oracle's sampler on t = [near, far], w = [1] against fp0 + clip01(u_k) (fp1 - fp0) and the centre -> edge
    pass, every operation rounded to fp32 once (the kernels are built without fma contraction, as the oracle is)."""
    from oracle import oracle as O
    f = np.float32
    t = np.array([[near, far]], f)
    lg = O.resample_logits(t, np.ones((1, 1), f))
    sd_o, idx_o = O.sample_intervals(t, lg, N, smin=near, smax=far)
    u = O.linspace_u(N).astype(f)
    fp0, fp1 = f(near), f(far)
    c = (fp0 + (_clip01(u) * f(fp1 - fp0)).astype(f)).astype(f)
    sd = np.empty(N + 1, f)
    sd[1:N] = ((c[1:] + c[:-1]).astype(f) / f(2)).astype(f)
    sd[0] = max(fp0, f(f(2) * c[0]) - f(f(c[1] + c[0]) / f(2)))
    sd[N] = min(fp1, f(f(2) * c[N - 1]) - f(f(c[N - 1] + c[N - 2]) / f(2)))
    assert np.array_equal(sd.view(np.uint32), sd_o[0].view(np.uint32)), (N, near, far, float(np.abs(sd - sd_o[0]).max()))
    assert not idx_o.any()


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip
    _hip.require_device()          # fails loudly: no fallback
    return _hip


def _image(hip, prec, training):
    key = hip.level_image(prec, training, 0)
    if key not in _packed:
        _packed[key] = hip.pack_weights(torch.tensor(_BLOB, device=DEV), precision=key)
    return _packed[key]


def _rays(n):
    out = {}
    for k, v in _RAYS.items():
        t = torch.tensor(np.asarray(v[:n], np.float32), device=DEV)
        out[k] = t.reshape(-1) if k in ("radii", "near", "far") else t
    return out


def _level0(hip, prec, R, N, implicit, training=False, **kw):
    cfg = hip.default_cfg(n_samples=N, n_in=1, precision=prec, compute_extras=1, training=int(training))
    sd = w = None
    if not implicit:
        sd = torch.tensor([[cfg.s_near, cfg.s_far]], device=DEV).repeat(R, 1)
        w = torch.ones((R, 1), device=DEV)
    res = hip.level_forward(_image(hip, prec, training), cfg, _rays(R), sd, w, save_activations=training, **kw)
    torch.cuda.synchronize()
    # (the activation buffer of a training forward is opaque and comes from torch.empty: its padding is not written)
    return {k: v.cpu().numpy() for k, v in res.items() if k not in ("activations", "activations_format")}


def _bits(x):
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    assert {"sdist", "bin_idx", "weights", "r_rgb", "r_rgb_fg", "rgb", "density"} <= a.keys()
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))
    assert not a["bin_idx"].any()


def _assert_fg(res, N, what):
    """r_rgb_fg against sum_i w_i rgb_i in float64: an fp32 sum of N rounded products, in any order, is within
    (N + 1) 2^-24 sum_i |w_i rgb_i| of it"""
    p = res["weights"].astype(np.float64)[..., None] * res["rgb"].astype(np.float64)
    err = np.abs(res["r_rgb_fg"].astype(np.float64) - p.sum(axis=1))
    bound = (N + 1) * 2.0 ** -24 * np.abs(p).sum(axis=1)
    print(f"{what}: r_rgb_fg max err {err.max():.3e}, smallest bound / err margin {float((bound - err).min()):.3e}")
    assert np.all(err <= bound), (what, float((err - bound).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [72, 128])
@pytest.mark.parametrize("R", [1, 5, 9])
@pytest.mark.parametrize("prec", [F32, F16X2, BF16], ids=["f32", "f16x2", "bf16"])
def test_implicit_level0_same_bits_as_explicit(hip, prec, R, N):
    """A lone ray, idle waves, a half-filled pass; N = 72 takes the other 16-sample run."""
    _assert_same_bits(_level0(hip, prec, R, N, True), _level0(hip, prec, R, N, False), (prec, R, N))


@pytest.mark.gpu
def test_implicit_level0_ring_variant(hip):
    """2048 x 192 is the smallest batch that selects level_fwd_f16x2_ring (tests/test_stream_wrap.py); its compositing path
    (cross-lane sums through shuffles) writes r_rgb_fg too."""
    a = _level0(hip, F16X2, 2048, 192, True)
    _assert_same_bits(a, _level0(hip, F16X2, 2048, 192, False), "ring")
    _assert_fg(a, 192, "ring")


@pytest.mark.gpu
def test_implicit_level0_training_forward(hip):
    """The f16x2 training chains (refnerf_sq_train: rnsq::forward), activations saved."""
    _assert_same_bits(_level0(hip, F16X2, 5, 128, True, training=True), _level0(hip, F16X2, 5, 128, False, training=True), "train")


@pytest.mark.gpu
def test_null_step_function_argument_errors(hip):
    """One pointer NULL and the other not, NULL with n_in != 1, NULL with s_far <= s_near: REFNERF_EINVAL, nothing launched."""
    R = 2
    r = _rays(R)
    rs = hip.RaysStruct()
    for name in ("origins", "directions", "viewdirs", "radii", "near", "far"):
        setattr(rs, "d_" + name, r[name].data_ptr())
    out = hip.LevelOut()
    packed = _image(hip, F32, False)
    sd = torch.tensor([[0.0, 1.0]], device=DEV).repeat(R, 1)
    w = torch.ones((R, 1), device=DEV)

    def call(cfg, sd_t, w_t):
        return hip.lib().refnerf_level_forward(hip.ptr(packed), C.byref(cfg), C.byref(rs), R, hip.ptr(sd_t), hip.ptr(w_t),
                                               C.byref(out), hip.stream_ptr())
    ok = hip.default_cfg(n_samples=16, n_in=1, precision=F32)
    assert call(ok, None, w) == -1 and b"together" in hip.lib().refnerf_last_error()
    assert call(ok, sd, None) == -1
    assert call(hip.default_cfg(n_samples=16, n_in=2, precision=F32), None, None) == -1
    assert call(hip.default_cfg(n_samples=16, n_in=1, precision=F32, s_near=0.5, s_far=0.5), None, None) == -1
    assert call(hip.default_cfg(n_samples=16, n_in=1, precision=F32, s_near=0.75, s_far=0.25), None, None) == -1
    act = torch.empty(hip.lib().refnerf_activation_workspace_bytes_basis(R, 16, 0), dtype=torch.uint8, device=DEV)
    tr = hip.default_cfg(n_samples=16, n_in=1, precision=F32, training=1)
    assert hip.lib().refnerf_level_forward_train(hip.ptr(packed), C.byref(tr), C.byref(rs), R, hip.ptr(sd), None, C.byref(out),
                                                 hip.ptr(act), act.numel(), hip.stream_ptr()) == -1
    with pytest.raises(ValueError, match="together"):
        hip.level_forward(packed, ok, r, sd, None)
    assert call(ok, None, None) == 0          # the valid call (every output pointer NULL: nothing stored)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 9])
@pytest.mark.parametrize("prec", [F32, F16X2], ids=["f32", "f16x2"])
def test_percentiles_soa_is_the_transpose(hip, prec, R):
    """soa[p, r] = aos[r, p], bit for bit (the fp32 kernels interpolate on lane 0, the 16-bit ones on lane p)."""
    soa = _level0(hip, prec, R, 128, True, percentiles_soa=True)
    aos = _level0(hip, prec, R, 128, True)
    assert "r_percentiles" not in soa and soa["r_percentiles_soa"].shape == (3, R) and aos["r_percentiles"].shape == (R, 3)
    assert np.array_equal(_bits(soa["r_percentiles_soa"]), _bits(np.ascontiguousarray(aos["r_percentiles"].T)))
    assert np.all(np.isfinite(aos["r_percentiles"]))
    for k in aos.keys() - {"r_percentiles"}:
        assert np.array_equal(_bits(soa[k]), _bits(aos[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [F32, F16X2, BF16], ids=["f32", "f16x2", "bf16"])
def test_foreground_colour(hip, prec):
    res = _level0(hip, prec, 9, 128, True)
    _assert_fg(res, 128, prec)
    # default configuration: white background, no render-time curve -> r_rgb = fg + max(0, 1 - acc) * 1
    bg = np.maximum(np.float32(0), np.float32(1) - res["r_acc"])[:, None]
    assert np.array_equal(_bits((res["r_rgb_fg"] + bg).astype(np.float32)), _bits(res["r_rgb"]))


@pytest.mark.gpu
def test_eval_step_launches_the_two_level_kernels_only(hip):
    """One Model.__call__ in eval mode with compute_extras, 9 rays x 128 samples, under torch.profiler: exactly two device
    kernels, both rn::level_fwd_* (no fill / cat / copy / mul / sum round them); ray_rgbs of level 0 is the kernel's r_rgb_fg."""
    from torch.profiler import ProfilerActivity, profile
    from refnerf_pl_amd import configs, models, utils
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "refnerf_blender.gin")], [])
    cfg = configs.Config()
    cfg.hip_precision = "f16x2"
    model = models.construct_model(None, cfg).to(DEV).eval()
    model.nerf_mlp.load_flat_params(_BLOB)
    rays = utils.rays_from_dict({k: v[:9] for k, v in _RAYS.items()}, torch.device(DEV))
    with torch.no_grad():
        model(rays, 1.0, True)                    # packs the weights, sets the kernel attributes
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            renderings, history = model(rays, 1.0, True)
            torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    print("device events:", names)
    assert len(names) == 2 and all("level_fwd_" in n for n in names), names
    for k in ("distance_percentile_5", "distance_median", "distance_percentile_95"):
        x = renderings[-1][k]
        assert x.dtype == torch.float64 and x.shape == (9,) and x.is_contiguous()
    fg = renderings[0]["ray_rgbs"]
    assert fg.shape == renderings[-1]["ray_rgbs"].shape == (9, 128, 3)
    want = (history[-1]["weights"].double()[..., None] * history[-1]["rgb"].double()).sum(dim=-2)
    bound = 129 * 2.0 ** -24 * (history[-1]["weights"].double()[..., None] * history[-1]["rgb"].double()).abs().sum(dim=-2)
    assert bool(((fg[:, 0, :].double() - want).abs() <= bound).all())
    configs.clear_config()

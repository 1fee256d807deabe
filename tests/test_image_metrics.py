"""refnerf_pl_amd.image: colour correction, PSNR, SSIM and the angular error of a test image on the device
(csrc/refnerf_image.h, the metric half of the reference's test_step).

Truths.  Colour correction, mse_to_psnr, the sRGB curves, downsample, compute_weighted_mae, the disparity MSE and the
test_step sequence are gated against the reference's float64 outputs in tests/golden/image_metrics.npz
(make_golden_image.py); the inputs are regenerated here from seeded recipes (low-frequency sinusoids plus noise).  dm_pix is
not installed where the fixture is made, so SSIM is gated against the definition (include/refnerf_hip.h) restated below as
a numpy double loop, which a CPU test checks against an independent conv2d formulation.

Bars.  Colour correction by normal equations: <= 1e-10 (float64 restatement and ATen path on the CPU), <= 1e-9 on the
device, L-inf against the reference's lstsq; everything else <= 1e-12 relative (MSE on the device: 1e-13); SSIM mean
<= 1e-11, map <= 1e-10 per element.  test_restatements_reproduce_the_fixture asserts what keeps those gates honest: every
masked Gram matrix has condition number <= 1e10, no value sits within 1e-9 of a mask threshold (a 1e-13 difference cannot
flip a mask), the corrected image differs from the input by more than 1e-3 (an identity warp cannot pass), and no value of
the test_step image sits within 1e-6 of an 8-bit rounding boundary.

Quantisation is q(x) = rint(x * 255) / 255 with an IEEE division, which is what torch.round(x * 255) / 255 gives on the
CPU (where the fixture was made); torch's DEVICE kernel for tensor / number multiplies by the rounded reciprocal and differs
in the last bit for some k / 255, so the bit-for-bit comparison takes torch's CPU result (_torch_quantized).

MEASURED on an MI355X (the GPU tests print these lines)
  colour correction, L-inf against the reference's float64 output (bar 1e-9), num_iters 1 / 5:
    warp_24x40 6.4e-14 / 4.9e-14   sat_24x40 3.7e-14 / 6.5e-14   odd_37x53 7.5e-14 / 5.3e-14   big_96x128 6.9e-14 / 4.6e-13
    the test_step image (32 x 40, 5 iterations) 2.4e-13
  SSIM against the restatement, mean (bar 1e-11) / map (bar 1e-10), quantised or not:
    11x11x3 0 / 0   12x27x3 1.1e-16 / 0   45x70x3 0 / 0   33x40x1 1.1e-16 / 4.3e-14
  squared error, relative (bar 1e-13): 0 .. 3.2e-16 on all eight shapes; weighted angular error (bar 1e-12): 0
"""
import ctypes as C
import functools
import json
import math
import os
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_metrics.npz")
DEV = "cuda:0"
EPS_CC = 0.5 / 255
E23 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------- recipes
def sinus_image(seed, H, W, C=3, amp=0.3, noise=0.03):
    """two low-frequency sinusoids per channel around 0.5, plus white noise, clipped to [0, 1]; float64 [H, W, C]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    img = np.empty((H, W, C))
    for c in range(C):
        f = rng.uniform(0.4, 1.6, 4)
        ph = rng.uniform(0.0, 2.0 * np.pi, 2)
        img[..., c] = 0.5 + amp * (0.6 * np.sin(2 * np.pi * (f[0] * xx + f[1] * yy) + ph[0])
                                   + 0.4 * np.sin(2 * np.pi * (f[2] * xx - f[3] * yy) + ph[1]))
    img += noise * rng.standard_normal(img.shape)
    return np.clip(img, 0.0, 1.0)


def cc_pair(kind, H, W, seed):
    """(img, ref): `warp` a smooth colour warp of ref plus noise, `sat` a gain that clips about 28 % of the values"""
    ref = sinus_image(seed, H, W, amp=0.45 if kind == "sat" else 0.3)
    n = np.random.default_rng(seed + 1000).standard_normal(ref.shape)
    if kind == "warp":
        img = 0.9 * ref ** 1.1 + 0.03 + 0.01 * n
    else:
        img = 1.75 * ref - 0.375 + 0.01 * n
    return np.clip(img, 0.0, 1.0), ref


CC_CASES = {
    "warp_24x40": dict(kind="warp", H=24, W=40, seed=11),
    "sat_24x40": dict(kind="sat", H=24, W=40, seed=12),
    "odd_37x53": dict(kind="warp", H=37, W=53, seed=13),        # neither the width nor the pixel count a multiple of the block
    "big_96x128": dict(kind="warp", H=96, W=128, seed=14),      # 12 workgroups of partials
}
DOWNSAMPLE = dict(seed=21, H=24, W=40)
WMAE = dict(seed=22, H=37, W=53)
DISP = dict(seed=23, H=24, W=40)
STEP = dict(seed=24, H=32, W=40)
STEP_CROP = 3


def _unit(rng, shape):
    v = rng.standard_normal(shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def wmae_inputs(seed, H, W):
    rng = np.random.default_rng(seed)
    g = _unit(rng, (H, W))
    n = g + 0.3 * rng.standard_normal(g.shape)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n[0, 0], n[0, 1] = g[0, 0], -g[0, 1]            # both ends of the clip
    return rng.random((H, W)), n, g


def disp_inputs(seed, H, W):
    rng = np.random.default_rng(seed)
    dist = 2.0 + sinus_image(seed + 1, H, W, C=1)[..., 0] * 4.0
    return dist, 1.0 / (1.0 + dist) + 0.01 * rng.standard_normal((H, W))


def step_inputs(seed, H, W):
    """a synthetic rendering and batch of one test view, float32 as the model and the dataset return them"""
    rng = np.random.default_rng(seed)
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    img, gt = cc_pair("warp", H, W, seed + 1)
    dist, disps = disp_inputs(seed + 2, H, W)
    ngt = _unit(rng, (H, W)) * rng.uniform(0.5, 2.0, (H, W, 1))          # the dataset's normals need not be unit length
    rend = dict(rgb=f32(img), distance_mean=f32(dist), distance_median=f32(dist + 0.05 * rng.standard_normal((H, W))),
                acc=f32(rng.uniform(0.2, 1.0, (H, W))), normals=f32(ngt + 0.2 * rng.standard_normal((H, W, 3))),
                normals_pred=f32(ngt + 0.4 * rng.standard_normal((H, W, 3))), ray_origins=f32(rng.random((H, W, 3))))
    # (the true normals stay float64: normalising them is then a float64 operation wherever it runs, and the 1e-12 gate does
    # not hinge on the order in which a device adds three float32 squares)
    batch = dict(rgb=f32(gt), disps=f32(disps), normals=ngt, alphas=f32(rng.uniform(0.0, 1.0, (H, W))))
    return rend, batch


# ------------------------------------------------------------------------------------------------- float64 restatements
def quantize(x):
    return np.rint(x * 255.0) / 255.0          # numpy's rint rounds half to even, as torch.round


def expand(x):
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    return np.stack([r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, np.ones_like(r)], -1)


def cc_restated(img, ref, num_iters=5, eps=EPS_CC, stats=None):
    """image.color_correct with the masked lstsq replaced by the masked normal equations and a pseudo-inverse that drops
    eigenvalues <= 10 * 2^-52 * lambda_max.  `stats` collects the worst condition number and the margin to the thresholds."""
    x, b = img.reshape(-1, 3).copy(), ref.reshape(-1, 3)
    unclipped = lambda z: (z >= eps) & (z <= 1 - eps)  # noqa: E731
    margin = lambda z: float(np.minimum(np.abs(z - eps), np.abs(z - (1 - eps))).min())  # noqa: E731
    mask0 = unclipped(x)
    if stats is not None:
        stats["margin"] = min(stats.get("margin", 1.0), margin(x), margin(b))
    for _ in range(num_iters):
        a = expand(x)
        warp = np.zeros((10, 3))
        for c in range(3):
            m = (mask0[:, c] & unclipped(x[:, c]) & unclipped(b[:, c])).astype(np.float64)
            ma = a * m[:, None]
            G, r = ma.T @ a, ma.T @ b[:, c]
            warp[:, c] = np.linalg.pinv(G, rcond=10 * 2.0 ** -52, hermitian=True) @ r
            if stats is not None and m.any():
                ev = np.linalg.eigvalsh(G)
                stats["cond"] = max(stats.get("cond", 0.0), float(ev[-1] / ev[0]) if ev[0] > 0 else math.inf)
        x = np.clip(a @ warp, 0.0, 1.0)
        if stats is not None:
            stats["margin"] = min(stats["margin"], margin(x))
    return x.reshape(img.shape)


def ssim_taps():
    g = [math.exp(-0.5 * (((i - 5) / 1.5) ** 2)) for i in range(11)]
    s = 0.0
    for v in g:
        s += v
    return np.array([v / s for v in g])


def ssim_restated(a, b):
    """(mean, map [H-10, W-10, C]) of the definition in include/refnerf_hip.h, one output pixel at a time"""
    g = ssim_taps()
    H, W, Cn = a.shape
    eps, c1, c2 = E23 ** 2, 0.01 ** 2, 0.03 ** 2
    F = lambda win: (g[:, None] * (g[:, None, None] * win).sum(0)).sum(0)   # noqa: E731  along H, then along W; [C]
    out = np.empty((H - 10, W - 10, Cn))
    for i in range(H - 10):
        for j in range(W - 10):
            wa, wb = a[i:i + 11, j:j + 11], b[i:i + 11, j:j + 11]
            mu_a, mu_b = F(wa), F(wb)
            s_aa = np.maximum(eps, F(wa * wa) - mu_a * mu_a)
            s_bb = np.maximum(eps, F(wb * wb) - mu_b * mu_b)
            s = F(wa * wb) - mu_a * mu_b
            s_ab = np.sign(s) * np.minimum(np.sqrt(s_aa * s_bb), np.abs(s))
            out[i, j] = ((2 * mu_a * mu_b + c1) * (2 * s_ab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (s_aa + s_bb + c2))
    return float(out.mean()), out


def ssim_conv2d(a, b):
    """the same definition through torch.nn.functional.conv2d with the outer-product kernel"""
    g = torch.from_numpy(ssim_taps())
    k = torch.outer(g, g)[None, None]
    F = lambda z: torch.nn.functional.conv2d(z.permute(2, 0, 1)[:, None], k)[:, 0].permute(1, 2, 0)  # noqa: E731
    a, b = torch.from_numpy(a), torch.from_numpy(b)
    eps, c1, c2 = E23 ** 2, 0.01 ** 2, 0.03 ** 2
    mu_a, mu_b = F(a), F(b)
    s_aa = torch.clamp(F(a * a) - mu_a ** 2, min=eps)
    s_bb = torch.clamp(F(b * b) - mu_b ** 2, min=eps)
    s = F(a * b) - mu_a * mu_b
    s_ab = torch.sign(s) * torch.minimum(torch.sqrt(s_aa * s_bb), s.abs())
    m = (2 * mu_a * mu_b + c1) * (2 * s_ab + c2) / ((mu_a ** 2 + mu_b ** 2 + c1) * (s_aa + s_bb + c2))
    return float(m.mean()), m.numpy()


def l2n(x):
    return x / np.sqrt(np.maximum((x ** 2).sum(-1, keepdims=True), x.dtype.type(E23)))


def wmae_restated(w, n, g):
    one = 1.0 - E23
    return float((w * np.arccos(np.clip((n * g).sum(-1), -one, one))).sum() / w.sum() * 180.0 / np.pi)


PSNR_FACTOR = float(np.float32(-10.0) / np.log(np.float32(10.0)))      # the reference's float32 factor


def psnr_restated(mse):
    return PSNR_FACTOR * math.log(mse)


def step_restated(rend, batch, rgb_cc, crop=STEP_CROP):
    """test_step's metric lines in numpy float64 on a given colour-corrected image (SSIM left out)"""
    r = {k: v.astype(np.float64) for k, v in rend.items() if not k.startswith("ray_")}
    gt = batch["rgb"].astype(np.float64)
    cr = lambda x: x[crop:-crop, crop:-crop]  # noqa: E731
    out = dict(psnr=psnr_restated(((cr(quantize(r["rgb"])) - cr(gt)) ** 2).mean()),
               cc_psnr=psnr_restated(((cr(quantize(rgb_cc)) - cr(gt)) ** 2).mean()))
    for tag in ("mean", "median"):
        out[f"disparity_{tag}_mse"] = float(((1 / (1 + r[f"distance_{tag}"]) - batch["disps"]) ** 2).mean())
    w = r["acc"] * batch["alphas"]
    ngt = l2n(batch["normals"]).astype(np.float64)
    for k in ("normals", "normals_pred"):
        out[k + "_mae"] = wmae_restated(w, l2n(r[k]), ngt)
    return out


def rel(a, b):
    return abs(a - b) / abs(b)


# ------------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def cc_case(case):
    prm = json.loads(str(golden()[f"cc_{case}_params"]))
    assert prm == CC_CASES[case]
    return cc_pair(**prm)


SSIM_SHAPES = [(11, 11, 3), (12, 27, 3), (45, 70, 3), (33, 40, 1)]


@functools.lru_cache(maxsize=None)
def ssim_case(shape, quant):
    H, W, Cn = shape
    b = sinus_image(100 + H, H, W, Cn)
    a = np.clip(0.9 * b + 0.04 + 0.05 * np.random.default_rng(200 + W).standard_normal(b.shape), 0.0, 1.0)
    mean, smap = ssim_restated(quantize(a) if quant else a, b)
    return a, b, mean, smap


# ------------------------------------------------------------------------------------------------- CPU
def test_restatements_reproduce_the_fixture():
    g = golden()
    for case in CC_CASES:
        img, ref = cc_case(case)
        for it in (1, 5):
            stats = {}
            got = cc_restated(img, ref, it, stats=stats)
            err = np.abs(got - g[f"cc_{case}_it{it}"]).max()
            print(f"cc {case} it{it}: restatement vs reference {err:.2e}, cond {stats['cond']:.2e}, margin {stats['margin']:.2e}, "
                  f"moved {np.abs(got - img).max():.2e}")
            assert err <= 1e-10, (case, it, err)
            assert stats["cond"] <= 1e10, (case, it, stats)
            assert stats["margin"] > 1e-9, (case, it, stats)
            assert np.abs(got - img).max() > 1e-3, (case, it)
    img, _ = cc_case("sat_24x40")
    assert 0.22 <= np.mean((img <= 0) | (img >= 1)) <= 0.34
    for m, want in zip(g["psnr_mse"], g["psnr_out"]):
        assert rel(psnr_restated(float(m)), want) <= 1e-12
    assert rel(wmae_restated(*wmae_inputs(**WMAE)), float(g["wmae_out"])) <= 1e-12
    dist, disps = disp_inputs(**DISP)
    assert rel(float(((1 / (1 + dist) - disps) ** 2).mean()), float(g["disp_mse"])) <= 1e-12
    rend, batch = step_inputs(**STEP)
    stats = {}
    cc = cc_restated(rend["rgb"].astype(np.float64), batch["rgb"].astype(np.float64), 5, stats=stats)
    assert np.abs(cc - g["step_rgb_cc"]).max() <= 1e-10 and stats["cond"] <= 1e10 and stats["margin"] > 1e-9
    for x in (g["step_rgb_cc"], rend["rgb"].astype(np.float64)):
        frac = x * 255.0 - np.floor(x * 255.0)
        assert np.abs(frac - 0.5).min() > 1e-6          # a 1e-9 difference cannot change an 8-bit value
    got = step_restated(rend, batch, cc)
    assert list(g["step_normal_keys"]) == ["normals_mae", "normals_pred_mae"]
    for k, v in got.items():
        assert rel(v, float(g["step_" + k])) <= 1e-12, (k, v, float(g["step_" + k]))


def test_ssim_restatement_against_conv2d():
    for shape in SSIM_SHAPES:
        for quant in (False, True):
            a, b, mean, smap = ssim_case(shape, quant)
            m2, map2 = ssim_conv2d(quantize(a) if quant else a, b)
            assert abs(mean - m2) <= 1e-12 and np.abs(smap - map2).max() <= 1e-12, shape
            assert 0.05 < mean < 0.98, (shape, mean)            # neither 0 nor 1: the comparison sees the formula
    a = ssim_case((12, 27, 3), False)[0]
    assert abs(ssim_restated(a, a)[0] - 1.0) <= 1e-12
    p, q, c1, c2, e = 0.3, 0.7, 1e-4, 9e-4, E23 ** 2
    # constant images: F(z^2) - mu^2 = 0 up to rounding, so sigma_aa = sigma_bb = eps and |s| <= 1e-16 ~ 0
    want = (2 * p * q + c1) * c2 / ((p * p + q * q + c1) * (2 * e + c2))
    got = ssim_restated(np.full((11, 13, 2), p), np.full((11, 13, 2), q))[0]
    assert abs(got - want) <= 1e-12


def test_aten_path_on_cpu_tensors_against_the_fixture():
    from refnerf_pl_amd import image
    g = golden()
    t = torch.from_numpy
    for case in CC_CASES:
        img, ref = cc_case(case)
        for it in (1, 5):
            got = image.color_correct(t(img), t(ref), num_iters=it)
            assert got.dtype == torch.float64
            assert np.abs(got.numpy() - g[f"cc_{case}_it{it}"]).max() <= 1e-10, (case, it)
    img, ref = cc_case("warp_24x40")
    assert torch.equal(image.color_correct(t(img), t(ref), num_iters=0), t(img))
    got32 = image.color_correct(t(img).float(), t(ref).float())
    assert got32.dtype == torch.float32 and np.abs(got32.numpy() - g["cc_warp_24x40_it5"]).max() < 1e-5
    np.testing.assert_allclose(image.mse_to_psnr(t(g["psnr_mse"])).numpy(), g["psnr_out"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(image.psnr_to_mse(t(g["psnr_out"])).numpy(), g["psnr_mse"], rtol=1e-6)
    np.testing.assert_allclose(image.linear_to_srgb(t(g["srgb_in"])).numpy(), g["linear_to_srgb_out"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(image.srgb_to_linear(t(g["srgb_in"])).numpy(), g["srgb_to_linear_out"], rtol=1e-12, atol=0)
    x = t(sinus_image(**DOWNSAMPLE))
    for f in (2, 4):
        np.testing.assert_allclose(image.downsample(x, f).numpy(), g[f"downsample_f{f}"], rtol=1e-12)
    assert float(image.dssim_to_ssim(image.ssim_to_dssim(torch.tensor(0.3)))) == pytest.approx(0.3)
    w, n, ng = wmae_inputs(**WMAE)
    assert rel(float(image.compute_weighted_mae(t(w), t(n), t(ng))), float(g["wmae_out"])) <= 1e-12
    a, b, mean, smap = ssim_case((12, 27, 3), True)
    m, mp = image.ssim(t(a), t(b), quantize_a=True, return_map=True)
    assert abs(float(m) - mean) <= 1e-12 and np.abs(mp.numpy() - smap).max() <= 1e-12
    # the test_step sequence on CPU tensors
    rend, batch = step_inputs(**STEP)
    cfg = types.SimpleNamespace(eval_quantize_metrics=True, eval_crop_borders=STEP_CROP, compute_disp_metrics=True,
                                compute_normal_metrics=True)
    metric, metric_cc, rgb_cc = image.evaluate_test_image({k: t(v) for k, v in rend.items()}, types.SimpleNamespace(**batch), cfg)
    assert np.abs(rgb_cc.numpy() - g["step_rgb_cc"]).max() <= 1e-10
    assert sorted(metric) == sorted(["psnr", "ssim", "disparity_mean_mse", "disparity_median_mse", "normals_mae", "normals_pred_mae"])
    assert sorted(metric_cc) == ["psnr", "ssim"]
    for k in metric:
        if k != "ssim":
            assert rel(float(metric[k]), float(g["step_" + k])) <= 1e-12, k
    assert rel(float(metric_cc["psnr"]), float(g["step_cc_psnr"])) <= 1e-12
    # refusals
    with pytest.raises(ValueError, match="evenly divide"):
        image.downsample(x, 5)
    with pytest.raises(ValueError, match="channels must match"):
        image.color_correct(t(img), t(ref)[..., :2])
    with pytest.raises(ValueError, match="LPIPS"):
        image.MetricHarness(compute_lpips=True)
    with pytest.raises(ValueError):
        image.ssim(t(img)[:10], t(ref)[:10])


# ------------------------------------------------------------------------------------------------- GPU
def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _torch_quantized(x):
    """torch.round(x * 255) / 255 as nerf_system.py:411 writes it, evaluated by torch on the CPU, where `/ 255` is the IEEE
    division of the definition q(x) = rint(x * 255) / 255 (torch's device kernel for a tensor divided by a Python number
    multiplies by the rounded reciprocal instead, which is another number in the last bit for some k / 255)."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (torch.round(t * 255) / 255).to(DEV)


def _pitched(x, border=2):
    """x as the interior of a larger device tensor: a view with a row pitch (and an offset), bit-equal to x"""
    H, W, Cn = x.shape
    big = torch.full((H + 2 * border, W + 2 * border + 1, Cn), 0.123, dtype=torch.float64, device=DEV)
    big[border:border + H, border:border + W] = _dev(x)
    return big[border:border + H, border:border + W]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CC_CASES))
def test_color_correct_against_the_reference(case):
    from refnerf_pl_amd import _hip, image
    g = golden()
    img, ref = cc_case(case)
    for it in (1, 5):
        got = image.color_correct(_dev(img), _dev(ref), num_iters=it)
        again = image.color_correct(_dev(img), _dev(ref), num_iters=it)
        assert got.dtype == torch.float64 and got.is_cuda and torch.equal(got, again)
        err = np.abs(got.cpu().numpy() - g[f"cc_{case}_it{it}"]).max()
        print(f"MEASURED cc {case} it{it}: L-inf vs reference {err:.2e}")
        assert err <= 1e-9, (case, it, err)
        view = image.color_correct(_pitched(img), _pitched(ref, 3), num_iters=it)
        assert torch.equal(view, got)
    out, warp = _hip.color_correct(_dev(img), _dev(ref), return_warp=True)
    a = torch.from_numpy(expand(cc_restated(img, ref, 4).reshape(-1, 3))).to(DEV)
    assert (torch.clip(a @ warp, 0, 1).reshape(out.shape) - out).abs().max() <= 1e-9
    assert torch.equal(image.color_correct(_dev(img), _dev(ref), num_iters=0), _dev(img))


@pytest.mark.gpu
def test_color_correct_all_clipped_gives_zeros():
    from refnerf_pl_amd import image
    img = np.zeros((13, 17, 3))
    img[::2] = 1.0
    ref = sinus_image(5, 13, 17)
    got = image.color_correct(_dev(img), _dev(ref))
    assert torch.equal(got, torch.zeros_like(got))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SSIM_SHAPES)
def test_ssim_against_the_restatement(shape):
    from refnerf_pl_amd import image
    for quant in (False, True):
        a, b, mean, smap = ssim_case(shape, quant)
        m, mp = image.ssim(_dev(a), _dev(b), quantize_a=quant, return_map=True)
        m2, mp2 = image.ssim(_dev(a), _dev(b), quantize_a=quant, return_map=True)
        assert m.is_cuda and m.dtype == torch.float64 and torch.equal(m, m2) and torch.equal(mp, mp2)
        e_mean, e_map = abs(float(m) - mean), np.abs(mp.cpu().numpy() - smap).max()
        print(f"MEASURED ssim {shape} quantize={quant}: mean {e_mean:.2e}, map {e_map:.2e}")
        assert e_mean <= 1e-11 and e_map <= 1e-10, (shape, quant, e_mean, e_map)
        assert torch.equal(image.ssim(_dev(a), _dev(b), quantize_a=quant), m)          # without the map
        if shape == (45, 70, 3):
            mv, mpv = image.ssim(_pitched(a), _pitched(b, 1), quantize_a=quant, return_map=True)
            assert torch.equal(mv, m) and torch.equal(mpv, mp)
            if quant:                          # bit for bit torch.round(x * 255) / 255
                assert torch.equal(image.ssim(_torch_quantized(a), _dev(b)), m)


@pytest.mark.gpu
def test_squared_error_psnr_and_angular_error():
    from refnerf_pl_amd import _hip, image
    g = golden()
    shapes = [(p["H"], p["W"], 3) for p in CC_CASES.values()] + SSIM_SHAPES
    for H, W, Cn in shapes:
        b = sinus_image(300 + H, H, W, Cn)
        a = np.clip(b + 0.05 * np.random.default_rng(400 + W).standard_normal(b.shape), 0.0, 1.0)
        for quant in (False, True):
            want = float((((quantize(a) if quant else a) - b) ** 2).mean())
            mse, psnr = image.mse_psnr(_dev(a), _dev(b), quantize_a=quant)
            e = rel(float(mse), want)
            print(f"MEASURED mse {(H, W, Cn)} quantize={quant}: rel {e:.2e}")
            assert e <= 1e-13 and rel(float(psnr), psnr_restated(want)) <= 1e-12
            mse_v, _ = image.mse_psnr(_pitched(a), _pitched(b, 3), quantize_a=quant)
            assert torch.equal(mse_v, mse)
            assert torch.equal(image.mse_psnr(_dev(a), _dev(b), quantize_a=quant)[0], mse)
    # quantisation bit for bit: every half-way point (k + 0.5) / 255 and random values
    x = np.concatenate([(np.arange(255) + 0.5) / 255.0, np.random.default_rng(7).random(255 * 4 - 255)]).reshape(17, 20, 3)
    b = sinus_image(8, 17, 20)
    q = _torch_quantized(x)
    assert torch.equal(q.cpu(), torch.from_numpy(quantize(x)))
    assert torch.equal(image.mse_psnr(_dev(x), _dev(b), quantize_a=True)[0], image.mse_psnr(q, _dev(b))[0])
    assert not torch.equal(image.mse_psnr(_dev(x), _dev(b), quantize_a=True)[0], image.mse_psnr(_dev(x), _dev(b))[0])
    assert torch.equal(image.ssim(_dev(x), _dev(b), quantize_a=True), image.ssim(q, _dev(b)))
    # the disparity MSE (C = 1) and the angular error against the fixture
    dist, disps = disp_inputs(**DISP)
    d = image.mse_psnr((1 / (1 + _dev(dist)))[..., None], _dev(disps)[..., None])[0]
    assert rel(float(d), float(g["disp_mse"])) <= 1e-12
    w, n, ng = wmae_inputs(**WMAE)
    mae = image.compute_weighted_mae(_dev(w), _dev(n), _dev(ng))
    e = rel(float(mae), float(g["wmae_out"]))
    print(f"MEASURED weighted mae: rel {e:.2e}")
    assert mae.is_cuda and e <= 1e-12
    assert torch.equal(_hip.weighted_mae(_dev(w), _dev(n), _dev(ng)), mae)


@pytest.mark.gpu
def test_evaluate_test_image_end_to_end():
    from refnerf_pl_amd import _hip, image
    g = golden()
    rend, batch = step_inputs(**STEP)
    cfg = types.SimpleNamespace(eval_quantize_metrics=True, eval_crop_borders=STEP_CROP, compute_disp_metrics=True,
                                compute_normal_metrics=True)
    rendering = {k: _dev(v) for k, v in rend.items()}
    dbatch = types.SimpleNamespace(**{k: _dev(v) for k, v in batch.items()})
    image.evaluate_test_image(rendering, dbatch, cfg)                    # warm-up: code objects, the allocator's pool
    torch.cuda.synchronize()
    _hip.set_timing(True)
    torch.cuda.set_sync_debug_mode("error")                              # any synchronising torch call raises
    try:
        metric, metric_cc, rgb_cc = image.evaluate_test_image(rendering, dbatch, cfg)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _, entries = _hip.get_timing(_hip.TIMER_IMAGE)
    _hip.set_timing(False)
    # colour correction, then (squared error, SSIM) twice, two disparity errors, two angular errors: nothing but launches
    assert entries == 1 + 4 + 2 + 2
    for d in (metric, metric_cc):
        assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float64 and v.dim() == 0 for v in d.values())
    assert sorted(metric) == sorted(["psnr", "ssim", "disparity_mean_mse", "disparity_median_mse", "normals_mae", "normals_pred_mae"])
    assert sorted(metric_cc) == ["psnr", "ssim"]
    e_cc = np.abs(rgb_cc.cpu().numpy() - g["step_rgb_cc"]).max()
    print(f"MEASURED test_step rgb_cc: L-inf vs reference {e_cc:.2e}")
    assert e_cc <= 1e-9
    for k in metric:
        if k != "ssim":
            bar = 1e-13 if k.endswith("_mse") else 1e-12
            assert rel(float(metric[k]), float(g["step_" + k])) <= bar, (k, float(metric[k]), float(g["step_" + k]))
    assert rel(float(metric_cc["psnr"]), float(g["step_cc_psnr"])) <= 1e-12
    c = STEP_CROP
    gt = batch["rgb"].astype(np.float64)[c:-c, c:-c]
    for d, src in ((metric, rend["rgb"].astype(np.float64)), (metric_cc, g["step_rgb_cc"])):
        want = ssim_restated(quantize(src)[c:-c, c:-c], gt)[0]
        assert abs(float(d["ssim"]) - want) <= 1e-11
    # MetricHarness.__call__: Python floats, equal to the device values
    h = image.MetricHarness()
    pred, true = rendering["rgb"].double(), dbatch.rgb.double()
    floats = h(pred, true, lambda s: "x_" + s)
    dm = h.device_metrics(pred, true)
    assert floats == {"x_psnr": float(dm["psnr"]), "x_ssim": float(dm["ssim"])} and all(type(v) is float for v in floats.values())


@pytest.mark.gpu
def test_c_entry_refusals():
    from refnerf_pl_amd import _hip
    L = _hip.lib()
    H, W = 16, 20
    a = torch.rand((H, W, 3), dtype=torch.float64, device=DEV)
    b = torch.rand((H, W, 3), dtype=torch.float64, device=DEV)
    out = torch.zeros((H, W, 3), dtype=torch.float64, device=DEV)
    res = torch.zeros(2, dtype=torch.float64, device=DEV)
    ws = _hip.image_workspace(H, W, 3, DEV)
    nb, st = ws.numel() * 8, _hip.stream_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    nan = float("nan")

    def refused(rc):
        assert rc == -1 and L.refnerf_last_error()          # REFNERF_EINVAL, with a message
    assert L.refnerf_image_mse(P(a), W * 3, P(b), W * 3, H, W, 3, 0, P(res), P(ws), nb, st) == 0
    # null pointers
    refused(L.refnerf_image_mse(None, W * 3, P(b), W * 3, H, W, 3, 0, P(res), P(ws), nb, st))
    refused(L.refnerf_image_mse(P(a), W * 3, P(b), W * 3, H, W, 3, 0, None, P(ws), nb, st))
    refused(L.refnerf_image_ssim(P(a), W * 3, None, W * 3, H, W, 3, 0, P(res), None, P(ws), nb, st))
    refused(L.refnerf_image_ssim(P(a), W * 3, P(b), W * 3, H, W, 3, 0, P(res), None, None, nb, st))
    refused(L.refnerf_color_correct(P(a), W * 3, P(b), W * 3, H, W, 3, 5, EPS_CC, None, None, P(ws), nb, st))
    refused(L.refnerf_weighted_mae(P(a), None, P(b), H * W, P(res), P(ws), nb, st))
    # C outside 1..4; colour correction: C != 3
    refused(L.refnerf_image_mse(P(a), W * 3, P(b), W * 3, H, W, 0, 0, P(res), P(ws), nb, st))
    refused(L.refnerf_image_ssim(P(a), W * 5, P(b), W * 5, H, W, 5, 0, P(res), None, P(ws), nb, st))
    refused(L.refnerf_color_correct(P(a), W * 4, P(b), W * 4, H, W, 4, 5, EPS_CC, P(out), None, P(ws), nb, st))
    # a pitch below W * C
    refused(L.refnerf_image_mse(P(a), W * 3 - 1, P(b), W * 3, H, W, 3, 0, P(res), P(ws), nb, st))
    refused(L.refnerf_image_ssim(P(a), W * 3, P(b), W * 3 - 1, H, W, 3, 0, P(res), None, P(ws), nb, st))
    refused(L.refnerf_color_correct(P(a), W * 3 - 1, P(b), W * 3, H, W, 3, 5, EPS_CC, P(out), None, P(ws), nb, st))
    # num_iters outside 0..64, non-finite eps
    refused(L.refnerf_color_correct(P(a), W * 3, P(b), W * 3, H, W, 3, -1, EPS_CC, P(out), None, P(ws), nb, st))
    refused(L.refnerf_color_correct(P(a), W * 3, P(b), W * 3, H, W, 3, 65, EPS_CC, P(out), None, P(ws), nb, st))
    refused(L.refnerf_color_correct(P(a), W * 3, P(b), W * 3, H, W, 3, 5, nan, P(out), None, P(ws), nb, st))
    refused(L.refnerf_color_correct(P(a), W * 3, P(b), W * 3, H, W, 3, 5, math.inf, P(out), None, P(ws), nb, st))
    # a workspace that is too small
    refused(L.refnerf_image_mse(P(a), W * 3, P(b), W * 3, H, W, 3, 0, P(res), P(ws), 0, st))
    refused(L.refnerf_image_ssim(P(a), W * 3, P(b), W * 3, H, W, 3, 0, P(res), None, P(ws), 0, st))
    refused(L.refnerf_color_correct(P(a), W * 3, P(b), W * 3, H, W, 3, 5, EPS_CC, P(out), None, P(ws), nb - 8, st))
    refused(L.refnerf_weighted_mae(P(a), P(a), P(b), H * W, P(res), P(ws), 8, st))
    # SSIM of an image smaller than the filter
    refused(L.refnerf_image_ssim(P(a), W * 3, P(b), W * 3, 10, W, 3, 0, P(res), None, P(ws), nb, st))
    refused(L.refnerf_image_ssim(P(a), W * 3, P(b), W * 3, H, 10, 3, 0, P(res), None, P(ws), nb, st))
    assert L.refnerf_image_workspace_bytes(H, W, 0) == 0 and L.refnerf_image_workspace_bytes(0, W, 3) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))           # no refused call wrote anything

"""Image helpers and the per-test-image metrics of the reference (internal/image.py, the metric half of
nerf_system.py:test_step), evaluated where the rendering already is.

Device tensors go through the float64 kernels of csrc/refnerf_image.h (squared error / PSNR, SSIM, colour correction, the
weighted angular error): no host synchronisation, no device-to-host copy, every sum in one fixed order.  CPU tensors, or a
library that has not been built, take an ATen float64 path that implements the same definitions; it is also the baseline
scripts/time_metrics.py times the kernels against.

SSIM is dm_pix.ssim with its defaults, restated (include/refnerf_hip.h spells the definition out).  Colour correction solves
the reference's masked least-squares problems through their normal equations in float64: it agrees with the reference's
lstsq to 1e-13 on images whose masked systems are well conditioned and is NOT a restatement of lstsq on near-rank-deficient
input (an image of one constant colour).  LPIPS is not available (it needs the VGG weights).
"""
import math
import os

import numpy as np
import torch

from . import _hip

_EPS32 = float(torch.finfo(torch.float32).eps)
SSIM_TAPS, SSIM_SIGMA, SSIM_K1, SSIM_K2 = 11, 1.5, 0.01, 0.03


def mse_to_psnr(mse):
    """image.py:31-33.  The factor is a float32 tensor there (-10 / log(tensor(10.))), and so it is here."""
    return -10. / torch.log(torch.tensor(10.)) * torch.log(mse)


def psnr_to_mse(psnr):
    """image.py:36-38"""
    return torch.exp(-0.1 * torch.log(torch.tensor(10.)) * psnr)


def ssim_to_dssim(ssim):
    return (1 - ssim) / 2


def dssim_to_ssim(dssim):
    return 1 - 2 * dssim


def linear_to_srgb(linear, eps=None):
    """image.py:51-59 (`linear` in [0, 1])"""
    if eps is None:
        eps = _EPS32
    srgb0 = 323 / 25 * linear
    srgb1 = (211 * torch.clamp(linear, min=eps) ** (5 / 12) - 11) / 200
    return torch.where(linear <= 0.0031308, srgb0, srgb1)


def srgb_to_linear(srgb, eps=None):
    """image.py:62-70 (`srgb` in [0, 1])"""
    if eps is None:
        eps = _EPS32
    linear0 = 25 / 323 * srgb
    linear1 = torch.clamp((200 * srgb + 11) / 211, min=eps) ** (12 / 5)
    return torch.where(srgb <= 0.04045, linear0, linear1)


def downsample(img, factor):
    """image.py:73-81: area downsampling; `factor` must divide the height and the width."""
    sh = tuple(img.shape)
    if not (sh[0] % factor == 0 and sh[1] % factor == 0):
        raise ValueError(f'Downsampling factor {factor} does not evenly divide image shape {sh[:2]}')
    img = img.reshape((sh[0] // factor, factor, sh[1] // factor, factor) + sh[2:])
    return img.mean((1, 3))


# ------------------------------------------------------------------------------------------------- dispatch
def _kernels(t) -> bool:
    """Device tensors run through the library; CPU tensors (or no built library) through the ATen float64 path."""
    return bool(t.is_cuda) and os.path.exists(_hip.LIB_PATH)


def _quantize(x):
    return torch.round(x * 255) / 255      # nerf_system.py:411


def _image3(x):
    """[..., C] as a [H, W, C] image (leading axes folded into H)"""
    if x.dim() == 3:
        return x
    if x.dim() < 3:
        return x.reshape(1, -1, x.shape[-1])
    return x.reshape(-1, x.shape[-2], x.shape[-1])


def ssim_taps():
    """The 11 taps of dm_pix.ssim's Gaussian (sigma 1.5), normalised to sum 1, exactly as the library computes them (double,
    summed in index order)."""
    g = [math.exp(-0.5 * (((i - SSIM_TAPS // 2) / SSIM_SIGMA) ** 2)) for i in range(SSIM_TAPS)]
    s = 0.0
    for v in g:
        s += v
    return [v / s for v in g]


def _ssim_aten(a, b, return_map=False):
    g = torch.tensor(ssim_taps(), dtype=torch.float64, device=a.device)

    def filt(z):      # 'valid' correlation along H, then along W, per channel
        z = (z.unfold(0, SSIM_TAPS, 1) * g).sum(-1)
        return (z.unfold(1, SSIM_TAPS, 1) * g).sum(-1)
    eps, c1, c2 = _EPS32 ** 2, SSIM_K1 ** 2, SSIM_K2 ** 2
    mu_a, mu_b = filt(a), filt(b)
    mu_aa, mu_bb, mu_ab = mu_a * mu_a, mu_b * mu_b, mu_a * mu_b
    s_aa = torch.clamp(filt(a * a) - mu_aa, min=eps)
    s_bb = torch.clamp(filt(b * b) - mu_bb, min=eps)
    s = filt(a * b) - mu_ab
    s_ab = torch.sign(s) * torch.minimum(torch.sqrt(s_aa * s_bb), torch.abs(s))
    smap = ((2 * mu_ab + c1) * (2 * s_ab + c2)) / ((mu_aa + mu_bb + c1) * (s_aa + s_bb + c2))
    return (smap.mean(), smap) if return_map else smap.mean()


def ssim(a, b, quantize_a=False, return_map=False):
    """dm_pix.ssim(a, b) with its defaults on [H, W, C] images, in float64: the mean of the [H-10, W-10, C] map (and the map
    when asked for).  `quantize_a` rounds `a` to 8 bits first."""
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"ssim: two [H, W, C] images of one shape are required, not {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[0] < SSIM_TAPS or a.shape[1] < SSIM_TAPS:
        raise ValueError(f"ssim: the image must be at least {SSIM_TAPS} x {SSIM_TAPS}, not {tuple(a.shape[:2])}")
    a, b = a.double(), b.double()
    if _kernels(a):
        return _hip.image_ssim(a, b, quantize_a=quantize_a, return_map=return_map)
    return _ssim_aten(_quantize(a) if quantize_a else a, b, return_map)


def mse_psnr(a, b, quantize_a=False):
    """(mean squared error, PSNR) of [..., C] images in float64, as scalars on the images' device."""
    if a.shape != b.shape:
        raise ValueError(f"mse_psnr: the images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = a.double(), b.double()
    if _kernels(a) and a.dim() >= 1 and 1 <= a.shape[-1] <= 4:
        out = _hip.image_mse(_image3(a), _image3(b), quantize_a=quantize_a)
        return out[0], out[1]
    mse = (((_quantize(a) if quantize_a else a) - b) ** 2).mean()
    return mse, mse_to_psnr(mse)


def _color_correct_aten(img, ref, num_iters, eps):
    x, b = img.reshape(-1, 3), ref.reshape(-1, 3)

    def unclipped(z):
        return (z >= eps) & (z <= 1 - eps)
    mask0 = unclipped(x)
    for _ in range(num_iters):
        a_mat = torch.cat([x[:, 0:1] * x[:, 0:], x[:, 1:2] * x[:, 1:], x[:, 2:3] * x[:, 2:], x, torch.ones_like(x[:, :1])], -1)
        warp = []
        for c in range(3):
            m = (mask0[:, c] & unclipped(x[:, c]) & unclipped(b[:, c])).to(x.dtype)
            ma = a_mat * m[:, None]
            warp.append(torch.linalg.pinv(ma.T @ a_mat, hermitian=True) @ (ma.T @ b[:, c]))
        x = torch.clip(a_mat @ torch.stack(warp, -1), 0, 1)
    return x.reshape(img.shape)


def color_correct(img, ref, num_iters=5, eps=0.5 / 255):
    """image.py:84-127: warp `img` to match the colours of `ref` (three channels).  Computed in float64 whatever the input
    type (the reference's caller casts first) and returned in `img`'s type."""
    if img.shape[-1] != ref.shape[-1]:
        raise ValueError(f'img\'s {img.shape[-1]} and ref\'s {ref.shape[-1]} channels must match')
    if img.shape[-1] != 3:
        raise ValueError(f"color_correct: three channels are required, not {img.shape[-1]}")
    if img.shape != ref.shape:
        raise ValueError(f"color_correct: the images differ in shape: {tuple(img.shape)} and {tuple(ref.shape)}")
    if not 0 <= int(num_iters) <= 64 or not math.isfinite(eps):
        raise ValueError("color_correct: num_iters must be in [0, 64] and eps finite")
    x, r = img.double(), ref.double()
    if _kernels(x):
        out = _hip.color_correct(_image3(x), _image3(r), num_iters=int(num_iters), eps=float(eps)).reshape(img.shape)
    else:
        out = _color_correct_aten(x, r, int(num_iters), float(eps))
    return out.to(img.dtype)


def l2_normalize(x, eps=_EPS32):
    """ref_utils.py:40-42"""
    return x / torch.sqrt(torch.clamp(torch.sum(x ** 2, dim=-1, keepdim=True), min=eps))


def compute_weighted_mae(weights, normals, normals_gt):
    """ref_utils.py:45-50: the weighted mean angular error in degrees (unit normals), in float64, as a scalar on the device."""
    w, n, g = weights.double(), normals.double(), normals_gt.double()
    if _kernels(w):
        return _hip.weighted_mae(w, n, g)
    one_eps = 1 - _EPS32
    return (w.reshape(-1) * torch.arccos(torch.clip((n * g).sum(-1), -one_eps, one_eps)).reshape(-1)).sum() / w.sum() * 180.0 / math.pi


class MetricHarness:
    """image.py:130-156: PSNR and SSIM of a predicted image against the true one."""

    def __init__(self, compute_lpips=False):
        if compute_lpips:
            raise ValueError("MetricHarness: LPIPS is not available (it needs the VGG weights of the lpips package)")
        self.compute_lpips = False

    def device_metrics(self, rgb_pred, rgb_gt, name_fn=lambda s: s, quantize_pred=False):
        """{psnr, ssim} as float64 scalars on the images' device: nothing is copied to the host and nothing waits.
        `quantize_pred` rounds the prediction to 8 bits inside the kernels (Config.eval_quantize_metrics)."""
        _, psnr = mse_psnr(rgb_pred, rgb_gt, quantize_a=quantize_pred)
        return {name_fn('psnr'): psnr, name_fn('ssim'): ssim(rgb_pred, rgb_gt, quantize_a=quantize_pred)}

    def __call__(self, rgb_pred, rgb_gt, name_fn=lambda s: s):
        """Evaluate the error between a predicted rgb image and the true image: Python floats, as the reference returns."""
        return {k: float(v) for k, v in self.device_metrics(rgb_pred, rgb_gt, name_fn).items()}


def _on(x, like, dtype=None):
    return torch.as_tensor(x, device=like.device) if dtype is None else torch.as_tensor(x, dtype=dtype, device=like.device)


def evaluate_test_image(rendering, batch, config, metric_harness=None):
    """The metric part of test_step (nerf_system.py:391-444) for one rendered test view: (metric, metric_cc, rgb_cc).

    `rendering` is the dict of models.render_image ([H, W, ...] tensors), `batch` carries rgb (and disps / normals / alphas
    for the optional metrics).  Everything is cast to float64 first, as in the reference.  `metric` holds psnr, ssim,
    disparity_{mean,median}_mse (Config.compute_disp_metrics) and `<key>_mae` for every rendering entry that starts with
    'normals' (Config.compute_normal_metrics); `metric_cc` holds psnr and ssim of the colour-corrected image `rgb_cc`
    (returned unquantised and uncropped, as rendering['rgb_cc'] is).  The values are float64 scalars on the rendering's
    device: the function never waits for it.  Config.eval_quantize_metrics rounds both images to 8 bits and
    Config.eval_crop_borders cuts the border off as a view (the kernels take the row pitch)."""
    harness = metric_harness or MetricHarness()
    rendering = {k: v.double() for k, v in rendering.items() if not k.startswith('ray_') and v is not None}
    rgb = rendering['rgb']
    rgb_gt = _on(batch.rgb, rgb, torch.float64)
    rgb_cc = color_correct(rgb, rgb_gt)
    quant = bool(config.eval_quantize_metrics)
    crop = int(config.eval_crop_borders)

    def cropped(x):
        return x[crop:-crop, crop:-crop] if crop > 0 else x
    metric = harness.device_metrics(cropped(rgb), cropped(rgb_gt), quantize_pred=quant)
    metric_cc = harness.device_metrics(cropped(rgb_cc), cropped(rgb_gt), quantize_pred=quant)
    if config.compute_disp_metrics:
        for tag in ('mean', 'median'):
            key = f'distance_{tag}'
            if key in rendering:
                disparity = 1 / (1 + rendering[key])
                disps = _on(batch.disps, rgb).double().reshape(disparity.shape)
                metric[f'disparity_{tag}_mse'] = mse_psnr(disparity[..., None], disps[..., None])[0]
    if config.compute_normal_metrics:
        weights = rendering['acc'] * _on(batch.alphas, rgb).reshape(rendering['acc'].shape)
        normals_gt = l2_normalize(_on(batch.normals, rgb))
        for key, val in rendering.items():
            if key.startswith('normals'):
                metric[key + '_mae'] = compute_weighted_mae(weights, l2_normalize(val), normals_gt)
    return metric, metric_cc, rgb_cc

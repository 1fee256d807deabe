"""Step-function helpers the losses need on the host -- mirror of the reference's internal/stepfun.py
searchsorted (:31-56), inner_outer (:67-80) and lossfun_outer (:83-89).  (The resampler of the same
file, sample_intervals / invert_cdf, is inside the fused level kernel: rn::sample_intervals_wave.)
integrate_weights / invert_cdf / sample (:134-206) and math.sorted_interp (math.py:88-111) are here in their general,
dtype-preserving torch form for host-side callers -- camera_utils.generate_ellipse_path resamples its angles with
`sample` on float64 -- and are not on the hot path.
"""
import torch


def searchsorted(a, v):
    """(idx_lo, idx_hi) with a[idx_lo] <= v < a[idx_hi]; both clamp to the first / last index of `a`
    when v lies outside [a[0], a[-1]] (stepfun.py:31-56).  Binary search instead of the reference's
    O(len(a) * len(v)) comparison masks."""
    cnt = torch.searchsorted(a.contiguous(), v.contiguous(), right=True)          # number of a_i <= v
    last = a.shape[-1] - 1
    return torch.clamp(cnt - 1, min=0), torch.clamp(cnt, max=last)


def inner_outer(t0, t1, y1):
    """Inner and outer measures of the step function (t1, y1) on the intervals of t0 (stepfun.py:67-80)."""
    cy1 = torch.cat([torch.zeros_like(y1[..., :1]), torch.cumsum(y1, dim=-1)], dim=-1)
    idx_lo, idx_hi = searchsorted(t1, t0)
    cy1_lo = torch.take_along_dim(cy1, idx_lo, dim=-1)
    cy1_hi = torch.take_along_dim(cy1, idx_hi, dim=-1)
    y0_outer = cy1_hi[..., 1:] - cy1_lo[..., :-1]
    y0_inner = torch.where(idx_hi[..., :-1] <= idx_lo[..., 1:], cy1_lo[..., 1:] - cy1_hi[..., :-1],
                           torch.zeros_like(y0_outer))
    return y0_inner, y0_outer


def lossfun_outer(t, w, t_env, w_env, eps=torch.finfo(torch.float32).eps):
    """The proposal weights (t_env, w_env) should be an upper envelope of the NeRF weights (t, w):
    scaled half-quadratic penalty on the excess (stepfun.py:83-89)."""
    _, w_outer = inner_outer(t, t_env, w_env)
    return torch.clamp(w - w_outer, min=0.0) ** 2 / (w + eps)


def lossfun_distortion(t, w):
    """mip-NeRF 360's distortion loss of the step function (t, w), per ray (stepfun.py:261-272): the double integral of
    w_i w_j |x - y| over all pairs of intervals.  The O(N^2) definition in the reference's order of operations (bit-equal
    values on the CPU), any device, differentiable in t and w; the hot path is refnerf_distortion_forward / _backward
    (train_utils.fused_distortion_loss), which needs sorted knots and gives the weights' gradient only."""
    mid = (t[..., 1:] + t[..., :-1]) / 2
    gaps = torch.abs(mid[..., :, None] - mid[..., None, :])
    between = torch.sum(w * torch.sum(w[..., None, :] * gaps, dim=-1), dim=-1)       # pairs of intervals
    within = torch.sum(w ** 2 * (t[..., 1:] - t[..., :-1]), dim=-1) / 3              # an interval with itself
    return between + within


def interval_distortion(t0_lo, t0_hi, t1_lo, t1_hi):
    """mean |x - y| for x uniform on [t0_lo, t0_hi] and y uniform on [t1_lo, t1_hi] (stepfun.py:275-291), in the reference's
    order of operations."""
    apart = torch.abs((t1_lo + t1_hi) / 2 - (t0_lo + t0_hi) / 2)                     # disjoint intervals: the midpoints' distance
    cubes = 2 * (torch.minimum(t0_hi, t1_hi) ** 3 - torch.maximum(t0_lo, t1_lo) ** 3)
    cross = 3 * (t1_hi * t0_hi * torch.abs(t1_hi - t0_hi) + t1_lo * t0_lo * torch.abs(t1_lo - t0_lo) +
                 t1_hi * t0_lo * (t0_lo - t1_hi) + t1_lo * t0_hi * (t1_lo - t0_hi))
    overlapping = (cubes + cross) / (6 * (t0_hi - t0_lo) * (t1_hi - t1_lo))
    return torch.where((t0_lo > t1_hi) | (t1_lo > t0_hi), apart, overlapping)


def weight_to_pdf(t, w, eps=torch.finfo(torch.float32).eps ** 2):
    """stepfun.py:92-94."""
    return w / torch.clamp(t[..., 1:] - t[..., :-1], min=eps)


def pdf_to_weight(t, p):
    """stepfun.py:97-99."""
    return p * (t[..., 1:] - t[..., :-1])


def sorted_interp(x, xp, fp):
    """np.interp along the last axis for sorted `xp` / `fp` (math.py:88-111), in the dtype of the arguments: each x is
    bracketed by the largest xp <= x and the smallest xp > x (the ends of `xp` where there is none), found with the
    reference's comparison mask, and `fp` is interpolated linearly between them (0 / 0 -> 0, offset clipped to [0, 1])."""
    below = x[..., None, :] >= xp[..., :, None]                      # [..., len(xp), len(x)]

    def bracket(v):
        lo = torch.where(below, v[..., None], v[..., :1, None]).amax(dim=-2)
        hi = torch.where(~below, v[..., None], v[..., -1:, None]).amin(dim=-2)
        return lo, hi
    fp0, fp1 = bracket(fp)
    xp0, xp1 = bracket(xp)
    offset = torch.clip(torch.nan_to_num((x - xp0) / (xp1 - xp0), 0), 0, 1)
    return fp0 + offset * (fp1 - fp0)


def integrate_weights(w):
    """CDF at the knots of a step function whose weights sum to 1 along the last axis: [..., n] -> [..., n + 1] that
    starts at exactly 0 and ends at exactly 1 (stepfun.py:134-154).  Keeps the dtype and device of `w`."""
    cw = torch.clamp(torch.cumsum(w[..., :-1], dim=-1), max=1)
    end = cw.shape[:-1] + (1,)
    return torch.cat([cw.new_zeros(end), cw, cw.new_ones(end)], dim=-1)


def invert_cdf(u, t, w_logits):
    """Invert the CDF of the step function (t, softmax(w_logits)) at u in [0, 1) (stepfun.py:157-165)."""
    return sorted_interp(u, integrate_weights(torch.softmax(w_logits, dim=-1)), t)


def sample(t, w_logits, num_samples, single_jitter=False, deterministic_center=False):
    """`num_samples` deterministic samples of the piecewise-constant PDF (t [..., n+1] sorted, w_logits [..., n]):
    the inverse CDF at a linspace of [0, 1 - eps], or at the bin centres of that linspace with `deterministic_center`
    (stepfun.py:168-206; eps is float32's, as there).  General, dtype-preserving torch -- the render-path generator
    calls it on float64; the float32 hot path is the fused refnerf_sample_intervals, which does not come through here."""
    del single_jitter                        # only read with a random generator, which the reference's port never passes
    eps = torch.finfo(torch.float32).eps
    pad = 1 / (2 * num_samples) if deterministic_center else 0
    # the reference draws u in float32 whatever the dtype of t; keep those values so float64 callers get its samples
    u = torch.linspace(pad, 1. - pad - eps, num_samples, dtype=torch.float32, device=t.device).to(t.dtype)
    return invert_cdf(torch.broadcast_to(u, t.shape[:-1] + (num_samples,)), t, w_logits)


def max_dilate(t, w, dilation, domain=(-float('inf'), float('inf')), rows_per_block=512):
    """Dilate (max-pool) a non-negative step function by `dilation` on both sides (stepfun.py:102-115):
    knots = sort(t, t[:-1] - d, t[1:] + d) clipped to `domain`; the value on a new interval is the largest
    old value whose widened interval [t_i - d, t_{i+1} + d) contains its left knot.  Same comparison masks
    as the reference, built for `rows_per_block` rays at a time to bound the [rays, 3M+1, M] transient."""
    t0 = t[..., :-1] - dilation
    t1 = t[..., 1:] + dilation
    t_dilate = torch.sort(torch.cat([t, t0, t1], dim=-1), dim=-1).values
    t_dilate = torch.clamp(t_dilate, min=float(domain[0]), max=float(domain[1]))
    lead = t.shape[:-1]
    t0f, t1f, tdf, wf = (x.reshape(-1, x.shape[-1]) for x in (t0, t1, t_dilate, w))
    out = []
    for i in range(0, tdf.shape[0], rows_per_block):
        s = slice(i, i + rows_per_block)
        inside = (t0f[s, None, :] <= tdf[s, :, None]) & (t1f[s, None, :] > tdf[s, :, None])
        out.append(torch.where(inside, wf[s, None, :], torch.zeros((), dtype=wf.dtype, device=wf.device)).max(dim=-1).values[..., :-1])
    w_dilate = torch.cat(out, dim=0).reshape(lead + (t_dilate.shape[-1] - 1,))
    return t_dilate, w_dilate


def max_dilate_weights(t, w, dilation, domain=(-float('inf'), float('inf')), renormalize=False,
                       eps=torch.finfo(torch.float32).eps ** 2):
    """Dilate a set of weights through their PDF (stepfun.py:118-131)."""
    p = weight_to_pdf(t, w)
    t_dilate, p_dilate = max_dilate(t, p, dilation, domain=domain)
    w_dilate = pdf_to_weight(t_dilate, p_dilate)
    if renormalize:
        w_dilate = w_dilate / torch.clamp(torch.sum(w_dilate, dim=-1, keepdim=True), min=eps)
    return t_dilate, w_dilate

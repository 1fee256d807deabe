"""Losses of the training step, host side.

Same names / signatures / arithmetic as the reference's internal/train_utils.py:
compute_data_loss (:33-88), compute_depth_smoothness_loss (:90-119), orientation_loss (:165-183),
interlevel_loss (:150-162), predicted_normal_loss (:186-204), noisy_consistency_loss (:207-279), noisy_distance_consistency_loss
(:282-310), accumulated_weights_loss (:313-316), weights_entropy_loss (:318-329) and the loss assembly of
NeRFSystem.training_step (nerf_system.py:77-188) as `training_losses`.  They are a few elementwise torch
ops on the level outputs; their gradients w.r.t. the renderings / ray_history entries are the seeds
refnerf_level_backward consumes (models.py::_LevelFunction).  The optimiser side of the step -- the LR schedule,
create_optimizer (train_utils.py:448-467) and the two gradient clips of nerf_system.configure_gradient_clipping --
is at the end of this file; its kernels are optim.ClippedAdam's.
"""
import collections
import functools

import numpy as np
import torch


def srgb_to_linear(srgb, eps=None):
    """image.py:62-70."""
    if eps is None:
        eps = torch.finfo(torch.float32).eps
    linear0 = 25 / 323 * srgb
    linear1 = torch.clamp(((200 * srgb + 11) / 211), min=eps) ** (12 / 5)
    return torch.where(srgb <= 0.04045, linear0, linear1)


def _l2_normalize(x):
    """ref_utils.py:40-42"""
    eps = torch.finfo(torch.float32).eps
    return x / torch.sqrt(torch.clamp(torch.sum(x ** 2, dim=-1, keepdim=True), min=eps))


def _pixel_penalty(sq_err, config):
    """per-channel penalty of the data term: plain L2 or Charbonnier (train_utils.py:53-61)"""
    kind = config.data_loss_type
    if kind == 'mse':
        return sq_err
    if kind == 'charb':
        return torch.sqrt(sq_err + config.charb_padding ** 2)
    assert False


def _angular_error_deg(weight, a, b):
    """weighted mean angle between unit vectors, in degrees (ref_utils.py:45-50)"""
    lim = 1 - torch.finfo(torch.float32).eps
    angle = torch.arccos(torch.clip((a * b).sum(-1), -lim, lim))
    return (weight * angle).sum() / weight.sum() * 180.0 / torch.pi


def _coarse_fine(per_level, n_levels, coarse_mult, fine_mult):
    """sum over levels in level order with the coarse multiplier on all but the last level (the reference's accumulation order)"""
    acc = 0.
    for lvl, term in enumerate(per_level):
        acc = acc + (fine_mult if lvl >= n_levels - 1 else coarse_mult) * term
    return acc


def compute_data_loss(batch, renderings, rays, config):
    """Data loss terms for RGB, and the disparity / normal statistics (train_utils.py:33-88).  Returns (loss, stats)."""
    dev = renderings[0]['rgb'].device
    target = torch.as_tensor(batch.rgb, dtype=torch.float32, device=dev)[..., :3]
    if config.supervised_by_linear_rgb:
        target = srgb_to_linear(target)
    # per-ray weight of the residual (mosaic masks, multiscale up-weighting: rays.lossmult), one copy per channel
    ray_w = torch.broadcast_to(torch.as_tensor(rays.lossmult, dtype=torch.float32, device=dev), target.shape)
    if config.disable_multiscale_loss:
        ray_w = torch.ones_like(ray_w)
    norm = ray_w.sum()
    per_level, stats = [], collections.defaultdict(list)
    for out in renderings:
        sq_err = (out['rgb'] - target) ** 2
        stats['mses'].append((ray_w * sq_err).sum() / norm)
        per_level.append((ray_w * _pixel_penalty(sq_err, config)).sum() / norm)
        if config.compute_disp_metrics:                       # train_utils.py:62-67 (disparity from the mean distance)
            disparity = 1 / (1 + out['distance_mean'])
            stats['disparity_mses'].append(((disparity - torch.as_tensor(batch.disps, device=dev)) ** 2).mean())
        if config.compute_normal_metrics:                     # train_utils.py:69-84
            if 'normals' in out:
                w = out['acc'] * torch.as_tensor(batch.alphas, dtype=torch.float32, device=dev)
                stats['normal_maes'].append(_angular_error_deg(
                    w, _l2_normalize(out['normals']), _l2_normalize(torch.as_tensor(batch.normals, dtype=torch.float32, device=dev))))
            else:                                             # normals not computed (eval mode): NaN, as in the reference
                stats['normal_maes'].append(torch.tensor(float('nan'), device=dev))
    per_level = torch.stack(per_level)
    loss = config.data_coarse_loss_mult * torch.sum(per_level[:-1]) + config.data_loss_mult * per_level[-1]
    return loss, {k: torch.stack([x.detach() for x in v]) for k, v in stats.items()}


def orientation_loss(rays, model, ray_history, config):
    """Orientation regulariser of Ref-NeRF (train_utils.py:165-183): normals facing away from the camera, weighted by the
    sample's rendering weight."""
    terms = []
    for level in ray_history:
        normals = level[config.orientation_loss_target]
        if normals is None:
            raise ValueError('Normals cannot be None if orientation loss is on.')
        weights = level['weights']
        to_camera = -torch.as_tensor(rays.viewdirs, dtype=torch.float32, device=weights.device)
        facing = (normals * to_camera[..., None, :]).sum(dim=-1)
        terms.append(torch.mean((weights * torch.clamp(facing, max=0.0) ** 2).sum(dim=-1)))
    return _coarse_fine(terms, model.num_levels, config.orientation_coarse_loss_mult, config.orientation_loss_mult)


def predicted_normal_loss(model, ray_history, config):
    """Predicted-normal supervision of Ref-NeRF (train_utils.py:186-204): 1 - cos between the density normals and the predicted
    ones, weighted by the sample's rendering weight."""
    terms = []
    for level in ray_history:
        n_density, n_mlp = level['normals'], level['normals_pred']
        if n_density is None or n_mlp is None:
            raise ValueError('Predicted normals and gradient normals cannot be None if '
                             'predicted normal loss is on.')
        terms.append(torch.mean((level['weights'] * (1.0 - torch.sum(n_density * n_mlp, dim=-1))).sum(dim=-1)))
    return _coarse_fine(terms, model.num_levels, config.predicted_normal_coarse_loss_mult, config.predicted_normal_loss_mult)


class _FusedRefNerfLosses(torch.autograd.Function):
    """data (mse) + orientation + predicted-normal loss of ONE level as a single autograd node on the fused kernels
    refnerf_losses_forward / refnerf_losses_backward (Config.hip_fused_losses): what compute_data_loss,
    orientation_loss and predicted_normal_loss compute with ~25 elementwise ATen ops per level, in one pass each way.
    (The 'charb' penalty and the statistics of compute_data_loss: _FusedDataTerms.)"""

    @staticmethod
    def forward(ctx, rgb, weights, normals_pred, aux):
        from . import _hip
        rgb_c, w_c, np_c = rgb.detach().contiguous(), weights.detach().contiguous(), normals_pred.detach().contiguous()
        terms = _hip.losses_forward(rgb_c, aux["gt"], aux["lossmult"], w_c, aux["orient_n"], aux["normals"], np_c, aux["viewdirs"])
        sums = terms.sum(dim=0)
        ctx.set_materialize_grads(False)
        ctx.aux, ctx.t = aux, (rgb_c, w_c, np_c)
        per_term = sums * aux["scales"]
        ctx.mark_non_differentiable(sums)
        return per_term.sum(), per_term, sums

    @staticmethod
    def backward(ctx, g_total, g_terms, _g_sums):
        from . import _hip
        aux = ctx.aux
        rgb_c, w_c, np_c = ctx.t
        # upstream gradient of the three terms, on the device (no host sync): the total's plus each term's own
        if g_total is None and g_terms is None:
            return None, None, None, None
        if g_terms is None:
            up3 = g_total.to(torch.float32).expand(3)
        elif g_total is None:
            up3 = g_terms.to(torch.float32)
        else:
            up3 = g_terms.to(torch.float32) + g_total.to(torch.float32)
        g_rgb, g_w, g_np = _hip.losses_backward(rgb_c, aux["gt"], aux["lossmult"], w_c, aux["orient_n"], aux["orient_on_pred"],
                                                aux["normals"], np_c, aux["viewdirs"], 1.0, 1.0, 1.0,
                                                upstream=(up3 * aux["scales"]).contiguous())
        return g_rgb, g_w, g_np, None


class _FusedDataTerms(torch.autograd.Function):
    """The data term of ONE level with either penalty ('mse' / 'charb') and the disparity / normal statistics of
    compute_data_loss as a single autograd node on refnerf_data_terms_forward / _backward: returns (loss = scale x the
    penalty's column sum, sums [5] = the kernel's column sums).  aux['scale'] is a device scalar (multiplier / normaliser),
    so nothing is read back; the statistics are not differentiable, as in the reference."""

    @staticmethod
    def forward(ctx, rgb, aux):
        from . import _hip
        rgb_c = rgb.detach().to(torch.float32).reshape(-1, 3).contiguous()
        args = _hip.data_terms_args(rgb_c, aux['gt'], aux['lossmult'], aux['penalty'], aux['charb_padding'], **aux['groups'])
        sums = _hip.data_terms_forward(args, rgb_c.device).sum(dim=0)
        ctx.set_materialize_grads(False)
        ctx.args, ctx.keep, ctx.shape = args, (rgb_c, aux), rgb.shape     # keep: the tensors behind the struct's pointers
        ctx.mark_non_differentiable(sums)
        return sums[1] * aux['scale'], sums

    @staticmethod
    def backward(ctx, g_loss, _g_sums):
        from . import _hip
        if g_loss is None:
            return None, None
        # the upstream gradient times multiplier / normaliser, on the device (no host sync)
        up = (g_loss.to(torch.float32) * ctx.keep[1]['scale']).reshape(1).contiguous()
        return _hip.data_terms_backward(ctx.args, up).reshape(ctx.shape), None


def fused_losses_supported(config):
    """The fused path covers both penalties of the data term ('mse', 'charb'), Config.supervised_by_linear_rgb and the
    disparity / normal statistics, with the orientation and predicted-normal regularisers."""
    return config.data_loss_type in ('mse', 'charb')


def _fused_data_inputs_ok(batch, renderings, config):
    """What the fused data term cannot take keeps the ATen path: a `disps` whose shape differs from distance_mean's (the
    reference then broadcasts the two against each other), or renderings without distance_mean."""
    if not config.compute_disp_metrics:
        return True
    disps = getattr(batch, 'disps', None)
    return disps is not None and all(
        'distance_mean' in r and tuple(np.shape(disps)) == tuple(r['distance_mean'].shape) for r in renderings)


def fused_refnerf_losses(model, batch, rays, renderings, ray_history, config):
    """compute_data_loss + orientation_loss + predicted_normal_loss (train_utils.py:33-88,165-204) through the fused
    kernels: returns (data_loss, stats, orientation_loss, predicted_normal_loss) with the same values (fp32 summation
    order aside) and the same gradients into renderings['rgb'], ray_history['weights'], ray_history['normals_pred'].
    An 'mse' data term without statistics rides in the node of the two regularisers (refnerf_losses_forward / _backward,
    one launch each way per level); 'charb' or a statistic sends the data term of every level through _FusedDataTerms and
    leaves the regularisers to that node.  stats carries 'mses', then 'disparity_mses', then 'normal_maes', each exactly
    when compute_data_loss produces it; batch.disps / alphas / normals are taken flat."""
    dev = renderings[0]['rgb'].device
    f32 = dict(dtype=torch.float32, device=dev)
    gt = torch.as_tensor(batch.rgb, **f32)[..., :3]
    if config.supervised_by_linear_rgb:
        gt = srgb_to_linear(gt)                       # once per step, not once per level
    gt = gt.reshape(-1, 3).contiguous()
    lossmult = torch.as_tensor(rays.lossmult, **f32).reshape(-1).contiguous()
    if config.disable_multiscale_loss:
        lossmult = torch.ones_like(lossmult)
    denom = 3.0 * lossmult.sum()                      # sum of the lossmult broadcast to [R, 3]
    viewdirs = torch.as_tensor(rays.viewdirs, **f32).reshape(-1, 3).contiguous()
    R = gt.shape[0]
    inv_denom = 1.0 / denom                           # stays on the device: no host synchronisation in the step
    want_o = _any_positive(config, 'orientation_coarse_loss_mult', 'orientation_loss_mult')
    want_n = _any_positive(config, 'predicted_normal_coarse_loss_mult', 'predicted_normal_loss_mult')
    want_disp, want_mae = bool(config.compute_disp_metrics), bool(config.compute_normal_metrics)
    own_data_node = config.data_loss_type != 'mse' or want_disp or want_mae

    def flat(x, *tail):
        return torch.as_tensor(x, **f32).reshape((R,) + tail).contiguous()
    disps = flat(batch.disps) if want_disp else None
    if want_mae:
        alphas, normals_gt = flat(batch.alphas), flat(batch.normals, 3)
    data, orient, normal, mses, disp_mses, maes = [], [], [], [], [], []
    for i, (rendering, hist) in enumerate(zip(renderings, ray_history)):
        N = hist['weights'].shape[-1]
        fine = i == model.num_levels - 1
        data_scale = (config.data_loss_mult if fine else config.data_coarse_loss_mult) * inv_denom
        if own_data_node:
            groups = {}
            if want_disp:
                groups.update(distance_mean=flat(rendering['distance_mean'].detach()), disps=disps)
            if want_mae and 'normals' in rendering:
                groups.update(acc=flat(rendering['acc'].detach()), alphas=alphas, normals=flat(rendering['normals'].detach(), 3),
                              normals_gt=normals_gt)
            loss, sums = _FusedDataTerms.apply(rendering['rgb'], dict(
                gt=gt, lossmult=lossmult, penalty=config.data_loss_type, charb_padding=config.charb_padding, groups=groups,
                scale=data_scale))
            data.append(loss)
            mses.append(sums[0] * inv_denom)
            if want_disp:
                disp_mses.append(sums[2] / R)
            if want_mae:    # normals not computed (eval mode): NaN, as in the reference
                maes.append(sums[3] / sums[4] * 180.0 / torch.pi if 'normals' in rendering else torch.full((), float('nan'), **f32))
            if not (want_o or want_n):
                continue
        orient_n = None
        if want_o:
            orient_n = hist[config.orientation_loss_target]
            if orient_n is None:
                raise ValueError('Normals cannot be None if orientation loss is on.')
            orient_n = orient_n.detach().reshape(R, N, 3).contiguous()
        normals = None
        if want_n:
            if hist['normals'] is None or hist['normals_pred'] is None:
                raise ValueError('Predicted normals and gradient normals cannot be None if predicted normal loss is on.')
            normals = hist['normals'].detach().reshape(R, N, 3).contiguous()
        scales = torch.stack([torch.zeros_like(inv_denom) if own_data_node else data_scale,
                              torch.full_like(inv_denom, (config.orientation_loss_mult if fine else config.orientation_coarse_loss_mult) / R),
                              torch.full_like(inv_denom, (config.predicted_normal_loss_mult if fine else config.predicted_normal_coarse_loss_mult) / R)])
        aux = dict(gt=gt, lossmult=lossmult, viewdirs=viewdirs, orient_n=orient_n, normals=normals, scales=scales,
                   orient_on_pred=config.orientation_loss_target == 'normals_pred')
        rgb = rendering['rgb'].detach() if own_data_node else rendering['rgb']      # detached: its data term is the other node's
        _, per_term, sums = _FusedRefNerfLosses.apply(rgb.reshape(R, 3), hist['weights'].reshape(R, N),
                                                      hist['normals_pred'].reshape(R, N, 3), aux)
        orient.append(per_term[1]); normal.append(per_term[2])
        if not own_data_node:
            data.append(per_term[0])
            mses.append(sums[0] * inv_denom)
    stats = {'mses': torch.stack([m.detach() for m in mses])}
    if want_disp:
        stats['disparity_mses'] = torch.stack([m.detach() for m in disp_mses])
    if want_mae:
        stats['normal_maes'] = torch.stack([m.detach() for m in maes])
    return (torch.stack(data).sum(), stats, torch.stack(orient).sum() if want_o else None,
            torch.stack(normal).sum() if want_n else None)


def interlevel_loss(ray_history, config):
    """Interlevel (proposal) loss of mip-NeRF 360 (train_utils.py:150-162): the proposal levels' weights must
    envelope the final level's; the final level is detached, so only the proposal MLP is trained by it."""
    from . import stepfun
    c = ray_history[-1]['sdist'].detach()
    w = ray_history[-1]['weights'].detach()
    total = 0.
    for ray_results in ray_history[:-1]:
        total = total + torch.mean(stepfun.lossfun_outer(c, w, ray_results['sdist'], ray_results['weights']))
    return config.interlevel_loss_mult * total


class _FusedInterlevel(torch.autograd.Function):
    """sum over rays and intervals of stepfun.lossfun_outer(t, w, t_env, w_env) for ONE proposal level as a single autograd
    node on refnerf_interlevel_forward / _backward (Config.hip_fused_proposal): what the cumsum, the two searchsorted calls,
    the two gathers and their autograd compute, in one launch each way.  Only w_env gets a gradient: the final level's
    (t, w) are detached by the loss, and the knots t_env are not differentiable."""

    @staticmethod
    def forward(ctx, t, w, t_env, w_env):
        from . import _hip
        rows = tuple(x.detach().to(torch.float32).reshape(-1, x.shape[-1]).contiguous() for x in (t, w, t_env, w_env))
        ctx.rows, ctx.shape = rows, w_env.shape
        return _hip.interlevel_forward(*rows).sum()

    @staticmethod
    def backward(ctx, g_sum):
        from . import _hip
        # the upstream gradient stays on the device (no host synchronisation)
        g = _hip.interlevel_backward(*ctx.rows, g_sum.detach().to(torch.float32).reshape(1).contiguous())
        return None, None, None, g.reshape(ctx.shape)


_INTERLEVEL_MAX_INTERVALS = 512     # refnerf_interlevel_forward / _backward: N and Np in [1, 512]


def fused_interlevel_supported(ray_history):
    """The kernels take CUDA tensors of 1..512 intervals per level."""
    return all(h['weights'].is_cuda and h['sdist'].is_cuda and 1 <= h['weights'].shape[-1] <= _INTERLEVEL_MAX_INTERVALS and
               h['sdist'].shape[-1] == h['weights'].shape[-1] + 1 for h in ray_history)


def fused_interlevel_loss(ray_history, config):
    """interlevel_loss through the fused kernels, one autograd node per proposal level: the same value (fp32 summation
    order aside; the kernel accumulates in double) and the same gradient into the proposal levels' weights."""
    c = ray_history[-1]['sdist'].detach()
    w = ray_history[-1]['weights'].detach()
    total = 0.
    for ray_results in ray_history[:-1]:
        total = total + _FusedInterlevel.apply(c, w, ray_results['sdist'].detach(), ray_results['weights']) / float(w.numel())
    return config.interlevel_loss_mult * total


def distortion_loss(ray_history, config):
    """mip-NeRF 360's distortion loss on the last level (Config.hip_distortion_loss; the reference's stepfun.lossfun_distortion,
    which its own training step never calls): the O(N^2) ATen definition, [R, N, N] intermediates under autograd."""
    from . import stepfun
    last = ray_history[-1]
    return config.distortion_loss_mult * torch.mean(stepfun.lossfun_distortion(last['sdist'], last['weights']))


class _FusedDistortion(torch.autograd.Function):
    """sum over rays of stepfun.lossfun_distortion(t, w) as a single autograd node on refnerf_distortion_forward / _backward:
    O(N) per ray on the sorted knots, t and w read once, one launch each way.  Only w gets a gradient: every sdist the model
    emits is detached, and the kernels do not compute the knots' gradient."""

    @staticmethod
    def forward(ctx, t, w):
        from . import _hip
        rows = tuple(x.detach().to(torch.float32).reshape(-1, x.shape[-1]).contiguous() for x in (t, w))
        ctx.rows, ctx.shape = rows, w.shape
        return _hip.distortion_forward(*rows).sum()

    @staticmethod
    def backward(ctx, g_sum):
        from . import _hip
        # the upstream gradient stays on the device (no host synchronisation)
        g = _hip.distortion_backward(*ctx.rows, g_sum.detach().to(torch.float32).reshape(1).contiguous())
        return None, g.reshape(ctx.shape)


_DISTORTION_MAX_INTERVALS = 512     # refnerf_distortion_forward / _backward: N in [1, 512]


def fused_distortion_supported(ray_history):
    """The kernels take CUDA tensors of 1..512 intervals on the last level."""
    h = ray_history[-1]
    return bool(h['weights'].is_cuda and h['sdist'].is_cuda and 1 <= h['weights'].shape[-1] <= _DISTORTION_MAX_INTERVALS and
                h['sdist'].shape[-1] == h['weights'].shape[-1] + 1)


def fused_distortion_loss(ray_history, config):
    """distortion_loss through the fused kernels: the same value (fp32 summation order aside: the kernel's recurrence has no
    cancellation, the ATen midpoint differences do) and the same gradient into the last level's weights."""
    last = ray_history[-1]
    w = last['weights']
    rays = w.numel() // w.shape[-1]
    return config.distortion_loss_mult * (_FusedDistortion.apply(last['sdist'].detach(), w) / float(rays))


_REG_TERMS = ('weights_entropy', 'acc', 'diffuse_consistency', 'specular_consistency', 'normals_consistency',
              'distance_consistency')        # the order of the kernels' scales / of the node's per-term output
_REG_INPUTS = ('weights', 'acc', 'distance', 'diffuse', 'specular', 'normals')


class _FusedRayRegularisers(torch.autograd.Function):
    """The six geometry regularisers of ONE level (weights entropy, accumulated weights, diffuse / specular / normal /
    distance consistency) as a single autograd node on refnerf_ray_regularisers_forward / _backward
    (Config.hip_fused_regularisers): what noisy_consistency_loss, noisy_distance_consistency_loss, accumulated_weights_loss
    and weights_entropy_loss compute with a chain of ATen ops and boolean indexings per term, in one pass each way and
    without a host synchronisation.  Inputs that are None switch their term off.  Returns (per_term [6] in _REG_TERMS
    order, multipliers and warm-up applied; sums [8], the kernel's column sums)."""

    @staticmethod
    def forward(ctx, aux, weights, acc, distance, diffuse, specular, normals, n_distance, n_diffuse, n_specular, n_normals):
        from . import _hip
        R, na = acc.shape[0], aux['n'] * aux['a']
        ins = (weights, acc, distance, diffuse, specular, normals, n_distance, n_diffuse, n_specular, n_normals)

        def flat(t, rows, width):
            if t is None:
                return None
            return t.detach().to(torch.float32).reshape((rows,) if width == 1 else (rows, width)).contiguous()
        w_c = None if weights is None else weights.detach().to(torch.float32).reshape(R, -1).contiguous()
        clean = dict(zip(_REG_INPUTS[2:], (flat(t, R, w) for t, w in zip(ins[2:6], (1, 3, 3, 3)))))
        noisy = dict(zip(_REG_INPUTS[2:], (flat(t, na, w) for t, w in zip(ins[6:], (1, 3, 3, 3)))))
        acc_c = flat(acc, R, 1)
        args, _, _ = _hip.regularisers_args(w_c, acc_c, clean, noisy, aux['rays'], aux['noisy_rays'], aux['n'], aux['a'],
                                            aux['thr_entropy'], aux['thr_consistency'], aux['types'])
        sums = _hip.ray_regularisers_forward(args, acc.device).sum(dim=0)
        ctx.set_materialize_grads(False)
        ctx.aux, ctx.args, ctx.shapes = aux, args, [None if t is None else t.shape for t in ins]
        ctx.keep = (w_c, acc_c, clean, noisy)                # the tensors behind the argument struct's pointers
        consts = aux['consts']                        # device float[7]: the six scales, then the ray count
        values = torch.cat([sums[0:1], sums[2:7]])
        counts = torch.cat([sums[1:2], consts[6:7], sums[7:8].expand(4)])
        per_term = values / counts * consts[:6]
        ctx.sums = sums
        ctx.mark_non_differentiable(sums)
        return per_term, sums

    @staticmethod
    def backward(ctx, g_terms, _g_sums):
        from . import _hip
        if g_terms is None:
            return (None,) * 11
        # upstream gradient of the six terms times multiplier and warm-up, on the device (no host sync)
        up = (g_terms.to(torch.float32) * ctx.aux['consts'][:6]).contiguous()
        g = _hip.ray_regularisers_backward(ctx.args, ctx.sums, up)
        names = _REG_INPUTS + tuple('n_' + k for k in _REG_INPUTS[2:])
        return (None,) + tuple(None if shape is None or g[k] is None else g[k].reshape(shape)
                               for k, shape in zip(names, ctx.shapes))


def fused_regularisers_supported(config):
    """The fused path covers what the ATen functions accept: the three colour measures, the 'mse' distance measure and the
    two normal targets (anything else keeps the ATen path and its ValueError)."""
    from . import _hip
    return (config.consistency_diffuse_loss_type in _hip.CONSISTENCY_TYPES and
            config.consistency_specular_loss_type in _hip.CONSISTENCY_TYPES and
            config.consistency_distance_loss_type == 'mse' and
            config.consistency_normal_loss_target in ('normals', 'normals_pred'))


def fused_ray_regularisers(model, rays, noisy_rays, renderings, renderings_noise, ray_history, config, warmup_ratio=1.):
    """noisy_consistency_loss + noisy_distance_consistency_loss + accumulated_weights_loss + weights_entropy_loss
    (train_utils.py:207-329) through the fused kernels, one autograd node per level: returns a dict with those of
    'diffuse_consistency', 'specular_consistency', 'normals_consistency', 'acc', 'distance_consistency' and
    'weights_entropy' that Config switches on, with the same values (fp32 summation order aside) and the same gradients into
    the clean and the noisy renderings and ray_history['weights'].  Flat batches ([R, .] rays) on the device; nothing is
    read back to the host.  A patch batch ([P, S, S, .] rays) keeps the ATen regularisers; its depth smoothness has its own
    kernels (fused_depth_smoothness_loss, Config.hip_fused_losses), as the interlevel loss has (fused_interlevel_loss,
    Config.hip_fused_proposal)."""
    from . import _hip
    dev = renderings[0]['acc'].device
    f32 = dict(dtype=torch.float32, device=dev)
    want_c = wants_noisy_pass(config)
    want_d = _any_positive(config, 'consistency_distance_loss_mult', 'consistency_distance_coarse_loss_mult')
    want_e = _any_positive(config, 'weights_entropy_loss_mult', 'weights_entropy_coarse_loss_mult')
    want_a = config.accumulated_weights_loss_mult > 0
    if (want_c or want_d) and renderings_noise is None:
        raise ValueError('the consistency losses need the renderings of the noisy rays (training_losses)')
    if want_d and noisy_rays is None:
        raise ValueError('the distance consistency loss needs the noisy rays and their renderings')
    n = config.sample_noise_size // config.patch_size ** 2 if (want_c or want_d) else 0
    a = config.sample_noise_angles if n > 0 else 0
    target = config.consistency_normal_loss_target
    L = len(renderings)
    rows = []
    for i in range(L):
        def mult(name):
            fine = getattr(config, f'{name}_loss_mult')
            return fine if i >= model.num_levels - 1 else getattr(config, f'{name}_coarse_loss_mult')
        rows.append([warmup_ratio * mult('weights_entropy'),
                     config.accumulated_weights_loss_mult if i == L - 1 else 0.,
                     warmup_ratio * mult('consistency_diffuse'), -warmup_ratio * mult('consistency_specular'),
                     warmup_ratio * mult('consistency_normal'), warmup_ratio * mult('consistency_distance'),
                     float(renderings[i]['acc'].shape[0])])
    # one asynchronous upload per step: per level the six scales (multiplier x warm-up; the specular term is maximised) and R
    consts = torch.tensor(rows, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
    ray_pair = noisy_pair = None
    if want_d:
        ray_pair = tuple(torch.as_tensor(x, **f32).reshape(-1, 3).contiguous() for x in (rays.origins, rays.directions))
        noisy_pair = tuple(torch.as_tensor(x, **f32).reshape(-1, 3).contiguous() for x in (noisy_rays.origins, noisy_rays.directions))
    per_level = []
    for i, (clean, hist) in enumerate(zip(renderings, ray_history)):
        noisy = renderings_noise[i] if (want_c or want_d) else {}
        if want_c:
            if clean.get('normals') is None or clean.get('normals_pred') is None:
                raise ValueError('Predicted normals and gradient normals cannot be None if consistency loss is on.')
        aux = dict(n=n, a=a, rays=ray_pair, noisy_rays=noisy_pair, consts=consts[i],
                   thr_entropy=config.acc_threshold_for_weights_entropy_loss,
                   thr_consistency=config.acc_threshold_for_consistency_loss,
                   types=(_hip.CONSISTENCY_TYPES[config.consistency_diffuse_loss_type],
                          _hip.CONSISTENCY_TYPES[config.consistency_specular_loss_type],
                          _hip.CONSISTENCY_TYPES[config.consistency_distance_loss_type]))

        def pick(src, key, on):
            return src[key] if on else None
        per_term, _ = _FusedRayRegularisers.apply(
            aux, hist['weights'] if want_e else None, clean['acc'],
            pick(clean, 'distance', want_d), pick(clean, 'diffuse', want_c), pick(clean, 'specular', want_c), pick(clean, target, want_c),
            pick(noisy, 'distance', want_d), pick(noisy, 'diffuse', want_c), pick(noisy, 'specular', want_c), pick(noisy, target, want_c))
        per_level.append(per_term)
    totals = torch.stack(per_level).sum(dim=0)          # coarse levels first, as the reference accumulates
    on = dict(zip(_REG_TERMS, (want_e, want_a, want_c, want_c, want_c, want_d)))
    return {k: totals[j] for j, k in enumerate(_REG_TERMS) if on[k]}


def _level_mult(i, model, coarse, fine):
    return coarse if i < model.num_levels - 1 else fine


def compute_depth_smoothness_loss(renderings, config):
    """Edge-aware depth smoothness over [..., H, W, .] patches (train_utils.py:90-119)."""
    def l1(x):
        return torch.mean(torch.abs(x))

    def bilateral(x):
        return torch.exp(-torch.abs(x).mean(-1, keepdim=True))
    per_level = []
    for rendering in renderings:
        depths = rendering['distance']
        acc00 = rendering['acc'].detach()[..., :-1, :-1, None]
        guide = rendering['rgb'].detach()
        v00, v01, v10 = depths[..., :-1, :-1, :], depths[..., :-1, 1:, :], depths[..., 1:, :-1, :]
        w01 = bilateral(guide[..., :-1, :-1, :] - guide[..., :-1, 1:, :])
        w10 = bilateral(guide[..., :-1, :-1, :] - guide[..., 1:, :-1, :])
        per_level.append((l1(acc00 * w01 * (v00 - v01) ** 2) + l1(acc00 * w10 * (v00 - v10) ** 2)) / 2)
    per_level = torch.stack(per_level)
    return config.depth_smoothness_coarse_loss_mult * torch.sum(per_level[:-1]) + \
        config.depth_smoothness_loss_mult * per_level[-1]


class _FusedDepthSmoothness(torch.autograd.Function):
    """compute_depth_smoothness_loss of ONE level of a [P, S, S, .] patch batch as a single autograd node on
    refnerf_depth_smoothness_forward / _backward: scale x (the two column sums of the per-patch rows), what ~30 ATen ops
    and six [P, S-1, S-1, .] temporaries compute per level.  Only the distance gets a gradient (acc and the guide image
    are read under no_grad in the reference); the upstream gradient stays on the device."""

    @staticmethod
    def forward(ctx, distance, acc, rgb, scale):
        from . import _hip
        P, S = acc.shape[0], acc.shape[1]
        d_c, a_c = (t.detach().to(torch.float32).reshape(P, S, S).contiguous() for t in (distance, acc))
        c_c = rgb.detach().to(torch.float32).reshape(P, S, S, 3).contiguous()
        args = _hip.depth_smoothness_args(d_c, a_c, c_c)
        sums = _hip.depth_smoothness_forward(args, d_c.device).sum(dim=0)
        ctx.set_materialize_grads(False)
        ctx.args, ctx.keep, ctx.scale, ctx.shape = args, (d_c, a_c, c_c), scale, distance.shape
        return (sums[0] + sums[1]) * scale

    @staticmethod
    def backward(ctx, g_loss):
        from . import _hip
        if g_loss is None:
            return None, None, None, None
        up = (g_loss.to(torch.float32) * ctx.scale).reshape(1).contiguous()
        return _hip.depth_smoothness_backward(ctx.args, up).reshape(ctx.shape), None, None, None


def fused_depth_smoothness_supported(renderings):
    """The kernels take CUDA renderings of one patch axis: acc [P, S, S], distance [P, S, S, 1], rgb [P, S, S, 3], S >= 2
    (any other leading shape keeps the ATen path)."""
    def ok(r):
        acc = r['acc']
        return (acc.is_cuda and acc.ndim == 3 and acc.shape[0] >= 1 and acc.shape[1] == acc.shape[2] >= 2 and
                tuple(r['distance'].shape) == tuple(acc.shape) + (1,) and tuple(r['rgb'].shape) == tuple(acc.shape) + (3,))
    return all(ok(r) for r in renderings)


def fused_depth_smoothness_loss(renderings, config):
    """compute_depth_smoothness_loss through the fused kernels, one autograd node per level: the same value (fp32 summation
    order aside) and the same gradient into renderings['distance']."""
    per_level = []
    for i, rendering in enumerate(renderings):
        P, S = rendering['acc'].shape[0], rendering['acc'].shape[1]
        mult = config.depth_smoothness_loss_mult if i == len(renderings) - 1 else config.depth_smoothness_coarse_loss_mult
        # (mean over the P (S-1)^2 cells of either edge + the same of the other) / 2
        per_level.append(_FusedDepthSmoothness.apply(rendering['distance'], rendering['acc'], rendering['rgb'],
                                                     mult / (2.0 * P * (S - 1) ** 2)))
    return torch.stack(per_level).sum()                # coarse levels first, as the reference accumulates


def _colour_consistency(kind, clean, noisy, mask):
    """One of the three colour-consistency measures of train_utils.py:224-250 between the clean ray
    [n,1,3] and its noisy copies [n,a,3]; `mask` [n,1] selects the rays that count."""
    if kind == 'mse':
        per_ray = ((clean - noisy) ** 2).mean(dim=1, keepdim=True)
    elif kind == 'avg_mse':
        per_ray = ((clean - noisy.mean(dim=1, keepdim=True)) ** 2).mean(dim=1, keepdim=True)
    elif kind == 'var':
        both = torch.cat([clean, noisy], dim=1)
        return both.var(dim=1, keepdim=True).mean(dim=-1, keepdim=True).sum(dim=-1)[mask].mean()
    else:
        raise ValueError(f'unknown consistency loss type {kind!r}')
    return per_ray.sum(dim=-1)[mask].mean()


def noisy_consistency_loss(model, renderings, renderings_noise, config, warmup_ratio=1.):
    """Diffuse / specular / normal consistency between each of the first n rays and its
    `sample_noise_angles` perturbed copies (train_utils.py:207-279).  Returns the three totals."""
    n = config.sample_noise_size // config.patch_size ** 2
    a = config.sample_noise_angles
    totals = [0., 0., 0.]
    for i, (clean, noisy) in enumerate(zip(renderings, renderings_noise)):
        def group(x):
            return x.reshape((n, a) + tuple(x.shape[1:]))
        mask = clean['acc'][:n, None] > config.acc_threshold_for_consistency_loss
        diffuse = _colour_consistency(config.consistency_diffuse_loss_type, clean['diffuse'][:n, None],
                                      group(noisy['diffuse']), mask)
        # the specular term is maximised: view-dependent colour is pushed into the specular branch
        specular = -_colour_consistency(config.consistency_specular_loss_type, clean['specular'][:n, None],
                                        group(noisy['specular']), mask)
        if clean.get('normals') is None or clean.get('normals_pred') is None:
            raise ValueError('Predicted normals and gradient normals cannot be None if consistency loss is on.')
        target = config.consistency_normal_loss_target
        if target not in ('normals', 'normals_pred'):
            raise ValueError('Given an unknown type of consistency_normal_loss_target.')
        cos = torch.sum(clean[target][:n, None] * group(noisy[target]), dim=-1)
        normal = (1.0 - cos).mean(dim=1, keepdim=True)[mask].mean()
        for j, (term, coarse, fine) in enumerate((
                (diffuse, config.consistency_diffuse_coarse_loss_mult, config.consistency_diffuse_loss_mult),
                (specular, config.consistency_specular_coarse_loss_mult, config.consistency_specular_loss_mult),
                (normal, config.consistency_normal_coarse_loss_mult, config.consistency_normal_loss_mult))):
            totals[j] = totals[j] + warmup_ratio * _level_mult(i, model, coarse, fine) * term
    return tuple(totals)


def noisy_distance_consistency_loss(model, rays, noisy_rays, renderings, renderings_noise, config, warmup_ratio=1.):
    """The clean ray and its noisy copies should hit the same 3-D point (train_utils.py:282-310)."""
    n = config.sample_noise_size // config.patch_size ** 2
    a = config.sample_noise_angles
    total = 0.
    for i, (clean, noisy) in enumerate(zip(renderings, renderings_noise)):
        dev = clean['distance'].device

        def f32(x):
            return torch.as_tensor(x, dtype=torch.float32, device=dev)
        hit = f32(rays.origins)[:n, None] + f32(rays.directions)[:n, None] * clean['distance'][:n, None]
        hit_n = f32(noisy_rays.origins).reshape(n, a, 3) + \
            f32(noisy_rays.directions).reshape(n, a, 3) * noisy['distance'].reshape(n, a, 1)
        mask = clean['acc'][:n, None] > config.acc_threshold_for_consistency_loss
        if config.consistency_distance_loss_type != 'mse':
            raise ValueError('consistency_distance_loss_type must be mse')
        loss = ((hit - hit_n) ** 2).mean(dim=1, keepdim=True).sum(dim=-1)[mask].mean()
        total = total + warmup_ratio * _level_mult(i, model, config.consistency_distance_coarse_loss_mult,
                                                   config.consistency_distance_loss_mult) * loss
    return total


def accumulated_weights_loss(renderings, config):
    """Pushes the fine level's accumulated opacity towards 1 (train_utils.py:313-316)."""
    return config.accumulated_weights_loss_mult * ((1 - renderings[-1]['acc']) ** 2).mean()


def weights_entropy_loss(model, renderings, ray_history, config, warmup_ratio):
    """Entropy of the compositing weights on rays that hit something (train_utils.py:318-329)."""
    total = 0.
    for i, (rendering, ray_results) in enumerate(zip(renderings, ray_history)):
        w = ray_results['weights'][rendering['acc'] > config.acc_threshold_for_weights_entropy_loss]
        loss = (-w * (w + 1e-10).log()).sum(dim=-1).mean()
        total = total + warmup_ratio * _level_mult(i, model, config.weights_entropy_coarse_loss_mult,
                                                   config.weights_entropy_loss_mult) * loss
    return total


def consistency_warmup_ratio(config, global_step):
    """Warm-up / decay schedule of the consistency terms (nerf_system.py:92-108)."""
    if config.consistency_warmup_steps > config.consistency_decay_steps:
        raise ValueError("Consistency loss decay should be after whole warmup.")
    ratio = 1.
    if 0. < config.consistency_warmup_steps <= 1.:
        ratio = min(1., global_step / (config.consistency_warmup_steps * config.max_steps))
    if 0. < config.consistency_decay_steps <= 1. and global_step >= config.consistency_decay_steps * config.max_steps:
        left = config.max_steps - global_step
        ratio = max(0., left / (config.max_steps - config.consistency_decay_steps * config.max_steps))
    return ratio


def _any_positive(config, *names):
    return any(getattr(config, n) > 0 for n in names)


_CONSISTENCY_MULTS = tuple(f"consistency_{k}_{lvl}loss_mult" for k in ("diffuse", "specular", "normal")
                           for lvl in ("coarse_", ""))


def wants_noisy_pass(config):
    """nerf_system.py:110-116: the second, perturbed-ray forward is needed."""
    return config.sample_noise_size > 0 and _any_positive(config, *_CONSISTENCY_MULTS)


def training_losses(model, batch, rays, config, train_frac=1.0, global_step=None, noisy_rays=None):
    """Forward(s) + every loss term of NeRFSystem.training_step (nerf_system.py:77-188).

    Runs Model.__call__ on `rays` and, when a consistency term is on, on the perturbed rays of
    sample_utils.sample_noisy_rays (or on `noisy_rays` if given: reproducible tests).  Returns
    (total, dict of terms, stats, aux) with aux = dict(renderings, ray_history, noisy_rays, ...)."""
    from . import sample_utils
    compute_extras = bool(config.compute_disp_metrics or config.compute_normal_metrics or config.sample_noise_size > 0)
    renderings, ray_history = model(rays, train_frac, compute_extras)
    step = config.max_steps if global_step is None else global_step
    ratio = consistency_warmup_ratio(config, step)
    renderings_noise = None
    if wants_noisy_pass(config):
        if config.patch_size ** 2 > config.sample_noise_size:
            raise ValueError(f'Patch size {config.patch_size}^2 too large for '
                             f'sampling noise view points {config.sample_noise_size}')
        if noisy_rays is None:
            noisy_rays = sample_utils.sample_noisy_rays(
                rays, renderings[-1], config.sample_angle_range, config.sample_noise_size // config.patch_size ** 2,
                config.sample_noise_angles, ratio, fused=getattr(config, 'hip_fused_regularisers', False))
        renderings_noise, _ = model(noisy_rays, train_frac, True)
    total, losses, stats = compute_losses(model, batch, rays, renderings, ray_history, config,
                                          renderings_noise=renderings_noise, noisy_rays=noisy_rays, warmup_ratio=ratio)
    return total, losses, stats, dict(renderings=renderings, ray_history=ray_history, noisy_rays=noisy_rays,
                                      renderings_noise=renderings_noise, warmup_ratio=ratio)


def compute_losses(model, batch, rays, renderings, ray_history, config, renderings_noise=None, noisy_rays=None,
                   warmup_ratio=1.):
    """The loss assembly of NeRFSystem.training_step (nerf_system.py:118-180) on already computed
    renderings: returns (total, dict of terms, stats).  Config.hip_fused_losses / hip_fused_regularisers route the three Ref-NeRF
    terms / the six geometry regularisers through their fused kernels and Config.hip_fused_proposal the interlevel loss through
    its own (same keys, same order); Config.hip_distortion_loss appends mip-NeRF 360's distortion loss of the last level as
    losses['distortion'] when Config.distortion_loss_mult > 0.  Config.hip_fused_losses also covers the 'charb' penalty, the linear-rgb target, the
    disparity / normal statistics (the reference's stats keys in the reference's order) and the depth smoothness of a
    [P, S, S, .] patch batch; the geometry regularisers want flat batches, so a patch batch keeps their ATen path."""
    losses = {}
    fused = (getattr(config, 'hip_fused_losses', False) and fused_losses_supported(config) and renderings[0]['rgb'].is_cuda and
             _fused_data_inputs_ok(batch, renderings, config))
    if fused:      # opt-in: the three Ref-NeRF terms of every level through refnerf_losses_* / refnerf_data_terms_*
        data_loss, stats, o_loss, n_loss = fused_refnerf_losses(model, batch, rays, renderings, ray_history, config)
    else:
        data_loss, stats = compute_data_loss(batch, renderings, rays, config)
    losses['data'] = data_loss
    if config.interlevel_loss_mult > 0:
        # opt-in: one launch each way per proposal level (refnerf_interlevel_forward / _backward)
        fused_prop = getattr(config, 'hip_fused_proposal', False) and fused_interlevel_supported(ray_history)
        losses['interlevel'] = fused_interlevel_loss(ray_history, config) if fused_prop else interlevel_loss(ray_history, config)
    if _any_positive(config, 'orientation_coarse_loss_mult', 'orientation_loss_mult'):
        losses['orientation'] = o_loss if fused else orientation_loss(rays, model, ray_history, config)
    if _any_positive(config, 'predicted_normal_coarse_loss_mult', 'predicted_normal_loss_mult'):
        losses['predicted_normals'] = n_loss if fused else predicted_normal_loss(model, ray_history, config)
    if config.patch_size > 1 and _any_positive(config, 'depth_smoothness_coarse_loss_mult', 'depth_smoothness_loss_mult'):
        # opt-in: one launch each way per level (refnerf_depth_smoothness_forward / _backward) on one patch axis
        fused_smooth = getattr(config, 'hip_fused_losses', False) and fused_depth_smoothness_supported(renderings)
        losses['smoothness'] = fused_depth_smoothness_loss(renderings, config) if fused_smooth else \
            compute_depth_smoothness_loss(renderings, config)
    want_distance = _any_positive(config, 'consistency_distance_loss_mult', 'consistency_distance_coarse_loss_mult')
    # opt-in: the six geometry regularisers of every level through refnerf_ray_regularisers_forward / _backward (flat batches on
    # the device; a missing noisy pass falls through to the ATen branches below and their ValueErrors)
    want_entropy = _any_positive(config, 'weights_entropy_loss_mult', 'weights_entropy_coarse_loss_mult')
    fused_reg = (getattr(config, 'hip_fused_regularisers', False) and fused_regularisers_supported(config) and
                 (wants_noisy_pass(config) or want_distance or want_entropy or config.accumulated_weights_loss_mult > 0) and
                 renderings[0]['acc'].is_cuda and getattr(rays.origins, 'ndim', 0) == 2 and
                 not ((wants_noisy_pass(config) or want_distance) and renderings_noise is None) and
                 not (want_distance and noisy_rays is None))
    reg = fused_ray_regularisers(model, rays, noisy_rays, renderings, renderings_noise, ray_history, config,
                                 warmup_ratio) if fused_reg else None
    if wants_noisy_pass(config):
        if renderings_noise is None:
            raise ValueError('the consistency losses need the renderings of the noisy rays (training_losses)')
        (losses['diffuse_consistency'], losses['specular_consistency'], losses['normals_consistency']) = (
            reg['diffuse_consistency'], reg['specular_consistency'], reg['normals_consistency']) if fused_reg else \
            noisy_consistency_loss(model, renderings, renderings_noise, config, warmup_ratio)
    if config.accumulated_weights_loss_mult > 0:
        losses['acc'] = reg['acc'] if fused_reg else accumulated_weights_loss(renderings, config)
    if want_distance:
        if renderings_noise is None or noisy_rays is None:
            raise ValueError('the distance consistency loss needs the noisy rays and their renderings')
        losses['distance_consistency'] = reg['distance_consistency'] if fused_reg else noisy_distance_consistency_loss(
            model, rays, noisy_rays, renderings, renderings_noise, config, warmup_ratio)
    if want_entropy:
        losses['weights_entropy'] = reg['weights_entropy'] if fused_reg else \
            weights_entropy_loss(model, renderings, ray_history, config, warmup_ratio)
    if getattr(config, 'hip_distortion_loss', False) and config.distortion_loss_mult > 0:
        # opt-in, and the LAST key: no other term moves in the summation order.  One launch each way where the kernels apply
        # (refnerf_distortion_forward / _backward), the ATen definition elsewhere (CPU tensors, more than 512 intervals)
        losses['distortion'] = fused_distortion_loss(ray_history, config) if fused_distortion_supported(ray_history) else \
            distortion_loss(ray_history, config)
    total = torch.sum(torch.stack([torch.as_tensor(v, dtype=torch.float32, device=data_loss.device)
                                   for v in losses.values()]))
    if getattr(config, 'hip_check_finite', True):
        _FINITE_GUARD.watch(total, config)
    return total, losses, stats


class _FiniteGuard:
    """Loud failure for the operand-range limit of the 16-bit chain modes (include/refnerf_hip.h: beyond |x| = 65504 a split-f16
    unit becomes inf - inf and the level's outputs NaN).  No per-step synchronisation: every total is reduced to one flag on
    the device and copied to pinned host memory asynchronously; the flag of step k is read when step k + 1 asks (its copy has
    long completed by then), or on `flush()`.  Raises FloatingPointError naming the knobs that lift the limit."""

    def __init__(self):
        self.pending = None      # (host flag, event, step number)
        self.step = 0

    def _raise(self, step, config):
        raise FloatingPointError(
            f"non-finite training loss at step {step} of this process (hip_train_precision = {getattr(config, 'hip_train_precision', '?')!r}, "
            f"hip_bwd_precision = {getattr(config, 'hip_bwd_precision', '?')!r}): the split-f16 / f16 / bf16 chains hold operands up to 65504 only -- "
            "set Config.hip_precision = Config.hip_train_precision = Config.hip_bwd_precision = 'f32' (exact fp32 MFMA chains, no "
            "operand-range limit), or Config.hip_check_finite = False to train on regardless")

    def flush(self, config=None):
        if self.pending is not None:
            flag, event, step = self.pending
            self.pending = None
            if event is not None:
                event.synchronize()
            if not bool(flag.item()):
                self._raise(step, config)

    def watch(self, total, config):
        self.flush(config)                      # the previous step's flag: its copy was queued a whole step ago
        self.step += 1
        ok = torch.isfinite(total.detach())
        if total.is_cuda:
            flag = torch.empty((), dtype=torch.bool, pin_memory=True)
            flag.copy_(ok, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            self.pending = (flag, event, self.step)
        elif not bool(ok):
            self._raise(self.step, config)


_FINITE_GUARD = _FiniteGuard()


def flush_finite_check(config=None):
    """raise now if the LAST watched training loss was not finite (call at the end of a run / before a checkpoint)"""
    _FINITE_GUARD.flush(config)


# ---- the optimiser side of the step ------------------------------------------------------------------------------------
def log_lerp(t, v0, v1):
    """The geometric blend of two positive values, v0 at t <= 0 and v1 at t >= 1: v0^(1-t) v1^t (the reference's
    math.log_lerp, internal/math.py:37-43, which a ValueError for a non-positive end comes from as well).  numpy double."""
    ends = np.array([v0, v1], np.float64)
    if not np.all(ends > 0.0):
        raise ValueError(f"log_lerp: both ends must be positive to blend geometrically, got v0 = {v0}, v1 = {v1}")
    u = np.float64(min(max(float(t), 0.0), 1.0))
    return np.power(ends[0], 1.0 - u) * np.power(ends[1], u)


def _warmup_factor(step, lr_delay_steps, lr_delay_mult):
    """The delay ramp of the schedule: a quarter sine wave from lr_delay_mult at step 0 up to 1 at lr_delay_steps and after
    (1 throughout when there is no delay)."""
    if lr_delay_steps <= 0:
        return np.float64(1.0)
    phase = min(max(float(step) / float(lr_delay_steps), 0.0), 1.0)
    mult = np.float64(lr_delay_mult)
    return mult + (1.0 - mult) * np.sin(np.float64(phase) * (np.pi / 2.0))


def learning_rate_decay(step, lr_init, lr_final, max_steps, lr_delay_steps=0, lr_delay_mult=1):
    """The LambdaLR multiplier at `step`, signature and values of the reference's math.learning_rate_decay
    (internal/math.py:46-78): the rate falls geometrically from lr_init (step 0) to lr_final (max_steps and after), under
    the delay ramp of _warmup_factor; returned relative to lr_init.  numpy double throughout."""
    rate = log_lerp(float(step) / float(max_steps), lr_init, lr_final)
    return _warmup_factor(step, lr_delay_steps, lr_delay_mult) * rate / np.float64(lr_init)


def _distinct_mlps(model):
    mlps = [("nerf_mlp", model.nerf_mlp)]
    if model.prop_mlp is not model.nerf_mlp:
        mlps.insert(0, ("prop_mlp", model.prop_mlp))
    return mlps


def _optimizer_tensors(config, params_or_model):
    """(tensors, segments, names, mlps): what an optimiser over a Model (or a plain iterable of tensors) steps.  A Model with
    Config.hip_flat_grads: each distinct MLP's flat_parameter(), cut into its layers' weights and biases; otherwise
    model.parameters().  The names are the reference's statistics keys (state_dict names with '.' -> '/')."""
    if not isinstance(params_or_model, torch.nn.Module):
        return list(params_or_model), {}, {}, []
    model = params_or_model
    mlps = _distinct_mlps(model) if hasattr(model, "nerf_mlp") else []
    if mlps and getattr(config, "hip_flat_grads", False):
        tensors, segments = [], {}
        for attr, mlp in mlps:
            flat = mlp.flat_parameter()
            names, off = [], []
            for spec in mlp.specs:
                names += [f"{attr}/{spec.name}/weight".replace(".", "/"), f"{attr}/{spec.name}/bias".replace(".", "/")]
                off += [spec.w_off, spec.b_off]
            tensors.append(flat)
            segments[id(flat)] = (names, off + [mlp.num_params])
        return tensors, segments, {}, [m for _, m in mlps]
    named = list(model.named_parameters())
    return [p for _, p in named], {}, {id(p): k.replace(".", "/") for k, p in named}, [m for _, m in mlps]


def create_optimizer(config, params_or_model, fused_clipping=True):
    """(optimizer, LambdaLR) as the reference's train_utils.create_optimizer (:448-467) returns them: Adam with Config's
    lr_init / adam_beta1 / adam_beta2 / adam_eps under math.learning_rate_decay -- here optim.ClippedAdam, which also does
    the reference's two gradient clips (Config.grad_max_val, grad_max_norm) and its per-parameter statistics inside the
    step.  fused_clipping=False leaves the clipping to the caller (clip_gradients), which is the reference's split.
    Handed a Model, it steps the flat blob(s) under Config.hip_flat_grads and model.parameters() otherwise, and a step
    post-hook calls mark_updated() on each MLP, so the weight-image cache needs no attention from the loop.
    Set Config.hip_flat_grads for speed: the step is 3 launches (56 us) on the flat blob, but two host calls per tensor on the
    46 separate parameters of the default mode -- 957 us, slower than torch's foreach sequence (254 us; docs/EXPERIMENTS.md
    section 12).  The per-tensor mode is there for parity with the reference's layout (its checkpoints' optimizer_states
    load into it), not for throughput."""
    from . import optim
    tensors, segments, names, mlps = _optimizer_tensors(config, params_or_model)
    optimizer = optim.ClippedAdam(tensors, lr=config.lr_init, betas=(config.adam_beta1, config.adam_beta2), eps=config.adam_eps,
                                  grad_max_val=config.grad_max_val if fused_clipping else 0.0,
                                  grad_max_norm=config.grad_max_norm if fused_clipping else 0.0, segments=segments, names=names)
    if mlps:
        def _mark_updated(_opt, _args, _kwargs):
            for mlp in mlps:
                mlp.mark_updated()
        optimizer.register_step_post_hook(_mark_updated)
    lr_scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, functools.partial(
        learning_rate_decay, lr_init=config.lr_init, lr_final=config.lr_final, max_steps=config.max_steps,
        lr_delay_steps=config.lr_delay_steps, lr_delay_mult=config.lr_delay_mult))
    return optimizer, lr_scheduler


def clip_gradients(params_or_model, config):
    """nerf_system.configure_gradient_clipping (:205-210) alone: clip_grad_value_(Config.grad_max_val) then
    clip_grad_norm_(Config.grad_max_norm) over all the tensors, written back into their .grad (device tensors: the
    statistics, finalize and write-back kernels; 2 k + 1 launches).  Returns the ClippedAdam that did it: its stats()
    carry total_norm and the per-parameter statistics; keep it and call its clip_gradients() to spare the setup."""
    from . import optim
    tensors, segments, names, _ = _optimizer_tensors(config, params_or_model)
    clipper = optim.ClippedAdam(tensors, lr=0.0, grad_max_val=config.grad_max_val, grad_max_norm=config.grad_max_norm,
                                segments=segments, names=names)
    clipper.clip_gradients()
    return clipper

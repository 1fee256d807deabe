"""GPU: every launching entry of include/refnerf_hip.h under guard bands (tests/guards.py).

Each case of CASES makes one plain call and two guarded calls on the same inputs and asserts
  (a) Arena.check(): no red-zone byte changed, no input changed, every output element written;
  (b) the guarded outputs are bit-equal to the plain call's: results do not depend on where buffers live;
  (c) the guarded outputs with the float inputs' red zones all zero and all NaN are bit-equal: no stray read reaches a
      result.  (Red zones of integer inputs hold the same in-range value in both runs.)
A case is a function of one argument G -- PlainAlloc or GuardedAlloc below -- that builds its inputs through G, calls the
entry through the _hip wrappers (whose allocations guards.guarded routes into the arena) or, where those do not reach,
through _hip.lib() with the structs _hip exports, and returns {name: output tensor}.  Every entry is deterministic (the
header promises fixed summation orders throughout), so no case needs a tolerance: the `tol` column stays empty.

The second half compares the per-sample outputs at the ragged level shapes with the CPU oracle (f32 mode) and the 16-bit
modes with the f32 mode.  tests/test_guards_cpu.py holds the checker's self-tests and the coverage gate over CASES."""
import ctypes as C
import functools
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

import guards
from helpers import HIST_KEYS, load_golden, params_from_golden, rays_from_golden
from refnerf_pl_amd import _hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")

# host-only entries: nothing is launched, nothing on the device is read or written
EXEMPT = {
    "refnerf_level_cfg_default": "fills a host struct",
    "refnerf_abi_version": "host-only query",
    "refnerf_device_ok": "device probe: no launch",
    "refnerf_last_error": "host string of the last error",
    "refnerf_packed_weights_bytes": "size query",
    "refnerf_packed_weights_bytes_basis": "size query",
    "refnerf_activation_workspace_bytes": "size query",
    "refnerf_activation_workspace_bytes_basis": "size query",
    "refnerf_backward_workspace_bytes": "size query",
    "refnerf_backward_workspace_bytes_basis": "size query",
    "refnerf_optim_workspace_bytes": "size query",
    "refnerf_optim_state_bytes": "size query",
    "refnerf_image_workspace_bytes": "size query",
    "refnerf_vis_percentile_workspace_bytes": "size query",
    "refnerf_activations_format": "host-only rule over a cfg",
    "refnerf_level_image": "host-only rule over a cfg",
    "refnerf_set_timing": "timing setter: host state",
    "refnerf_get_timing": "timing getter: host state",
    "refnerf_get_timing_family": "timing getter: host state",
}


# ------------------------------------------------------------------------------------------------- the two allocators
class PlainAlloc:
    """the plain call: ordinary tensors of the caching allocator"""
    guarded = False
    zone = 0.0

    def f(self, t, name=None):
        return t

    def i(self, t, zone, name=None):
        return t

    def inout(self, t, reason, name=None):
        return t.clone()

    def out(self, shape, dtype=torch.float32, name=None):
        return torch.empty(shape, dtype=dtype, device=DEV)

    def scratch(self, shape, dtype, reason, fill=None, name=None):
        t = torch.empty(shape, dtype=dtype, device=DEV)
        return t if fill is None else t.fill_(fill)

    def loose(self, t, reason):
        pass


class GuardedAlloc:
    """the guarded call: inputs copied between red zones, outputs sentinel-filled (guards.Arena)"""
    guarded = True

    def __init__(self, arena):
        self.arena, self.zone = arena, arena.float_zone

    def f(self, t, name=None):                      # a float input
        return self.arena.put(t, name=name)

    def i(self, t, zone, name=None):                # an integer input; `zone`: the in-range value its red zones hold
        return self.arena.put(t, name=name, int_zone=zone)

    def inout(self, t, reason, name=None):          # updated in place: `reason` names the header line
        return self.arena.put(t, name=name, inout=reason, int_zone=None if t.dtype.is_floating_point else 0)

    def out(self, shape, dtype=torch.float32, name=None):      # an output every element of which must be written
        return self.arena.alloc(shape, dtype, DEV, "sentinel", name=name)

    def scratch(self, shape, dtype, reason, fill=None, name=None):     # red zones only: `reason` names the header line
        return self.arena.alloc(shape, dtype, DEV, fill, name=name, reason=reason)

    def loose(self, t, reason):
        self.arena.loose(t, reason)


class Case:
    def __init__(self, id, entries, fn, tol=None, note=""):
        self.id, self.entries, self.fn, self.tol, self.note = id, tuple(entries), fn, tol, note


CASES = []


def case(id, *entries, tol=None, note=""):
    def reg(fn):
        CASES.append(Case(id, entries, fn, tol, note))
        return fn
    return reg


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def rng(*seed):
    return np.random.default_rng([7] + [int(s) for s in seed])


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------- level family
PARAM_KW = dict(seed=3, bias_scale=0.05, sharpen=8.0)
LEVEL_SHAPES = [(1, 1, 2),          # the minimum
                (3, 33, 40),        # one partly filled pass, N not a multiple of 32
                (7, 128, 64),       # 2 or 4 rays per workgroup with a partly filled last workgroup
                (5, 64, 96),
                (3, 96, 192),       # one and a half passes
                (3, 256, 256)]      # two passes
RING_SHAPE = (2051, 192, 192)       # the record-ring variant of the 16-bit eval kernels (R / 4 >= 512)
PREC = {"f32": _hip.PREC_F32, "bf16": _hip.PREC_BF16, "f16": _hip.PREC_F16, "f16x2": _hip.PREC_F16X2}
BASIS_GROUPS = 7                    # 'icosahedron' / 2: 21 directions


@functools.lru_cache(maxsize=None)
def _blob(groups):
    from refnerf_pl_amd import synthetic
    if groups > 1:
        return synthetic.make_basis_params(n_basis=3 * groups, **PARAM_KW)
    return synthetic.make_params(**PARAM_KW)


@functools.lru_cache(maxsize=None)
def _basis_np(groups):
    from refnerf_pl_amd import geopoly
    basis = {7: geopoly.generate_basis("icosahedron", 2), 2: geopoly.generate_basis("icosahedron", 1)}[groups]
    assert basis.shape == (3 * groups, 3)
    return f32(basis)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _pack_digests():
    """tests/golden/pack_digests.json (make_golden_pack_digests.py): the images' bytes as the commit named in it packed them, and
    the digests of the inputs it packed, by this module's own _blob / _basis_np"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_digests.json")) as f:
        want = json.load(f)
    have = {f"blob-G{g}": _sha(_blob(g)) for g in (0, 2, 7)}
    have.update({f"basis-G{g}": _sha(_basis_np(g)) for g in (2, 7)})
    return want, have


_images = {}


def _plain_image(kind, groups=0):
    """the weight image of PARAM_KW of one kind, packed once into an ordinary tensor that lives as long as the module"""
    if (kind, groups) not in _images:
        basis = T(_basis_np(groups)) if groups > 1 else None
        _images[(kind, groups)] = (T(_blob(groups)), basis, _hip.pack_weights(T(_blob(groups)), precision=kind, basis=basis))
    return _images[(kind, groups)]


PADS = ("csrc/refnerf_layout.h, make_packed and the chunked 16-bit images: the tail pads the weight prefetch runs past an op are part of "
        "the image's size and are never written")
_pads = {}


def _sentinel_tensor(n_floats):
    return torch.full((n_floats,), guards.SENTINEL_I32, dtype=torch.int32, device=DEV).view(torch.float32)


def _pad_mask(kind, groups=0):
    """which 32-bit words of an image refnerf_pack_weights* leaves alone (the prefetch pads): packed once into a
    sentinel-filled tensor"""
    if (kind, groups) not in _pads:
        P, basis, img = _plain_image(kind, groups)
        probe = _hip.pack_weights(P, _sentinel_tensor(img.numel()), precision=kind, basis=basis)
        _pads[(kind, groups)] = probe.view(torch.int32) == guards.SENTINEL_I32
    return _pads[(kind, groups)]


def packed_image(G, kind, groups=0):
    """... and, under guard, its copy between red zones, with the prefetch pads holding what the red zones hold (all-zero
    or all-ones words: NaN in every operand format), so that a pad value that reached a result would show in (b) and (c).
    The library remembers the kind of every image it packs per device pointer (refnerf_hip.h, refnerf_level_image), so the
    copy is packed once more in place: the same bytes, the right kind."""
    P, basis, img = _plain_image(kind, groups)
    if not G.guarded:
        return img
    img = img.clone()
    img.view(torch.int32)[_pad_mask(kind, groups)] = 0 if G.zone == 0.0 else -1
    t = G.f(img, name="packed")
    assert _hip.pack_weights(P, t, precision=kind, basis=basis) is t
    return t


def level_rays(G, R):
    from refnerf_pl_amd import synthetic
    rays = synthetic.blender_rays(R, seed=R, center_frac=0.5)
    out = {}
    for k in ("origins", "directions", "viewdirs", "radii", "near", "far"):
        t = T(f32(rays[k]))
        out[k] = G.f(t.reshape(-1) if k in ("radii", "near", "far") else t, name=k)
    return out


def step_function(R, n_in):
    """(sdist [R, n_in + 1], weights [R, n_in]): the initial step function, or a peaky random one"""
    if n_in == 1:
        return np.tile(f32([[0.0, 1.0]]), (R, 1)), np.ones((R, 1), np.float32)
    g = rng(R, n_in)
    sd = np.sort(g.random((R, n_in + 1)), -1)
    sd[:, 0], sd[:, -1] = 0.0, 1.0
    w = g.random((R, n_in)) ** 6
    return f32(sd), f32(w / w.sum(-1, keepdims=True) * 0.9)


def level_fn(R, n_in, N, prec="f32", training=False, backward=False, history=True, extras=1, null_init=False, soa=False,
             groups=0, wgrad=None):
    def fn(G):
        kw = dict(n_samples=N, n_in=n_in, precision=PREC[prec], training=int(training), compute_extras=extras, ipe_groups=groups)
        if wgrad is not None:
            kw["wgrad_mode"] = wgrad
        cfg = _hip.default_cfg(**kw)
        packed = packed_image(G, _hip.level_image(PREC[prec], training, groups), groups)
        rays = level_rays(G, R)
        sd, w = (None, None) if null_init else (G.f(T(a), name=n) for a, n in zip(step_function(R, n_in), ("sdist_in", "weights_in")))
        res = _hip.level_forward(packed, cfg, rays, sd, w, history=history, save_activations=backward, percentiles_soa=soa)
        out = {k: v for k, v in res.items() if torch.is_tensor(v) and k != "activations"}     # (the activations are opaque)
        if backward:
            g = rng(R, N, 1)
            seeds = [G.f(T(f32(1e-2 * g.standard_normal(s))), name=n) for s, n in (((R, 3), "g_r_rgb"), ((R, N), "g_weights"), ((R, N, 3), "g_normals_pred"))]
            grads = G.scratch((_hip.NUM_PARAMS_EXT if groups > 1 else _hip.NUM_PARAMS,), torch.float32, fill=0.0, name="param_grads",
                              reason="refnerf_hip.h, refnerf_level_backward: ACCUMULATES dL/d(params) into d_param_grads")
            _hip.level_backward(packed, cfg, rays, res, *seeds, grads)
            out["param_grads"] = grads
        return out
    return fn


def _level_cases():
    ex, tr, bw = "refnerf_level_forward_ex", "refnerf_level_forward_train_ex", "refnerf_level_backward"
    for prec in ("f32", "bf16", "f16", "f16x2"):
        for s in LEVEL_SHAPES + ([RING_SHAPE] if prec != "f32" else []):
            CASES.append(Case(f"level-eval-{prec}-{s[0]}x{s[1]}x{s[2]}", [ex], level_fn(*s, prec=prec)))
    for s in ((3, 33, 40), (7, 128, 64)):
        tag = f"{s[0]}x{s[1]}x{s[2]}"
        CASES.append(Case(f"level-eval-f32-nohistory-{tag}", [ex], level_fn(*s, history=False)))
        CASES.append(Case(f"level-eval-f32-noextras-{tag}", [ex], level_fn(*s, extras=0)))
        CASES.append(Case(f"level-eval-f32-soa-{tag}", [ex], level_fn(*s, soa=True)))
        CASES.append(Case(f"level-eval-f16x2-somehistory-{tag}", [ex], level_fn(*s, prec="f16x2", history=("rgb", "density"))))
        CASES.append(Case(f"level-train-f32-forward-only-{tag}", [ex], level_fn(*s, training=True)))
    for prec in ("f32", "f16x2"):
        for R, N in ((1, 2), (7, 64), (3, 192)):       # d_sdist_in = d_weights_in = NULL: the initial step function
            CASES.append(Case(f"level-eval-{prec}-nullinit-{R}x1x{N}", [ex], level_fn(R, 1, N, prec=prec, null_init=True)))
    CASES.append(Case("level-train-f32-nullinit-7x1x64", [tr, bw], level_fn(7, 1, 64, training=True, backward=True, null_init=True)))
    for s in LEVEL_SHAPES:
        tag = f"{s[0]}x{s[1]}x{s[2]}"
        CASES.append(Case(f"level-train-f32-{tag}", [tr, bw], level_fn(*s, training=True, backward=True)))
        CASES.append(Case(f"level-train-f32-wgradf32-{tag}", [tr, bw], level_fn(*s, training=True, backward=True, wgrad=_hip.WGRAD_F32)))
        CASES.append(Case(f"level-train-bf16-{tag}", [tr, bw], level_fn(*s, prec="bf16", training=True, backward=True)))
        for name, mode in (("bf16x3", _hip.WGRAD_BF16X3), ("f16", _hip.WGRAD_F16)):
            CASES.append(Case(f"level-train-f16x2-wgrad{name}-{tag}", [tr, bw], level_fn(*s, prec="f16x2", training=True, backward=True, wgrad=mode)))
        for prec in ("f32", "f16x2"):
            CASES.append(Case(f"level-train-basis7-{prec}-{tag}", [tr, bw, "refnerf_pack_weights_basis"],
                              level_fn(*s, prec=prec, training=True, backward=True, groups=BASIS_GROUPS)))
    for prec in ("f32", "f16x2"):
        CASES.append(Case(f"level-eval-basis7-{prec}-3x33x40", [ex], level_fn(3, 33, 40, prec=prec, groups=BASIS_GROUPS)))


_level_cases()

def _direct_level(entry, R, n_in, N):
    """refnerf_level_forward / refnerf_level_forward_train: the entries without refnerf_level_out_extra, which the wrappers do
    not call -- through _hip.lib() with the structs _hip exports"""
    training = entry.endswith("_train")

    def fn(G):
        lib = _hip.lib()
        cfg = _hip.default_cfg(n_samples=N, n_in=n_in, training=int(training), compute_extras=1)
        packed = packed_image(G, _hip.level_image(_hip.PREC_F32, training, 0))
        rays = level_rays(G, R)
        rs = _hip.RaysStruct()
        for k, t in rays.items():
            setattr(rs, "d_" + k, t.data_ptr())
        sd, w = (G.f(T(a)) for a in step_function(R, n_in))
        shapes = {"sdist": (R, N + 1), "weights": (R, N), "density": (R, N), "roughness": (R, N), "r_distance": (R,), "r_acc": (R,),
                  "r_roughness": (R,), "r_distance_mean": (R,)}
        shapes.update({k: (R, N, 3) for k in ("rgb", "normals_pred", "grad_pred", "tint", "diffuse", "specular") + (("normals",) if training else ())})
        shapes.update({k: (R, 3) for k in ("r_rgb", "r_diffuse", "r_specular", "r_normals_pred", "r_tint") + (("r_normals",) if training else ())})
        res = {k: G.out(s, name=k) for k, s in shapes.items()}
        res["bin_idx"] = G.out((R, N), torch.int32, name="bin_idx")
        res["r_percentiles"] = G.out((R, 3), torch.float64, name="r_percentiles")
        out = _hip.LevelOut()
        for k, t in res.items():
            setattr(out, "d_" + k, t.data_ptr())
        if training:
            nbytes = int(lib.refnerf_activation_workspace_bytes(R, N))
            act = G.scratch((nbytes,), torch.uint8, name="activations",
                            reason="refnerf_hip.h, refnerf_level_forward_train: d_activations is opaque to the caller, only its size is part of the ABI")
            _hip.check(lib.refnerf_level_forward_train(_hip.ptr(packed), C.byref(cfg), C.byref(rs), R, _hip.ptr(sd), _hip.ptr(w), C.byref(out),
                                                       _hip.ptr(act), nbytes, _hip.stream_ptr()))
        else:
            _hip.check(lib.refnerf_level_forward(_hip.ptr(packed), C.byref(cfg), C.byref(rs), R, _hip.ptr(sd), _hip.ptr(w), C.byref(out),
                                                 _hip.stream_ptr()))
        return res
    return fn


for _s in ((3, 33, 40), (7, 128, 64)):
    for _e in ("refnerf_level_forward", "refnerf_level_forward_train"):
        CASES.append(Case(f"{_e[8:]}-direct-{_s[0]}x{_s[1]}x{_s[2]}", [_e], _direct_level(_e, *_s)))


def mlp_fn(R, N, training, full, groups=0):
    def fn(G):
        g = rng(R, N, 2)
        cfg = _hip.default_cfg(n_samples=N, training=int(training), ipe_groups=groups)
        packed = packed_image(G, _hip.level_image(_hip.PREC_F32, training, groups), groups)
        means = G.f(T(f32(g.uniform(-1, 1, (R, N, 3)))), name="means")
        diag = g.uniform(1e-4, 1e-2, (R, N, 3))
        if full:
            covs = np.zeros((R, N, 3, 3))
            for c in range(3):
                covs[..., c, c] = diag[..., c]
            covs[..., 0, 1] = covs[..., 1, 0] = 0.3 * np.sqrt(diag[..., 0] * diag[..., 1])
        else:
            covs = diag
        covs = G.f(T(f32(covs)), name="covs")
        view = G.f(T(f32(unit(g.standard_normal((R, 3))))), name="viewdirs")
        return _hip.mlp_forward(packed, cfg, means, covs, view)
    return fn


for _R, _N in ((1, 2), (3, 40), (7, 64), (3, 192)):
    for _tr in (False, True):
        for _full in (True, False):
            CASES.append(Case(f"mlp-{'train' if _tr else 'eval'}-{'full' if _full else 'diag'}-{_R}x{_N}", ["refnerf_mlp_forward"],
                              mlp_fn(_R, _N, _tr, _full)))
CASES.append(Case("mlp-eval-full-basis7-3x40", ["refnerf_mlp_forward"], mlp_fn(3, 40, False, True, BASIS_GROUPS)))


# ------------------------------------------------------------------------------------------------- stage entries
def _stage_cases():
    def sampler(R, M, N):
        def fn(G):
            g = rng(R, M, N)
            t = np.sort(g.random((R, M + 1)), -1)
            t[:, 0], t[:, -1] = 0.0, 1.0
            sd, bi = _hip.sample_intervals(G.f(T(f32(t)), name="t"), G.f(T(f32(3 * g.standard_normal((R, M)))), name="logits"), N)
            return dict(sdist=sd, bin_idx=bi)
        return fn
    for s in ((1, 1, 2), (3, 33, 40), (37, 128, 129), (5, 512, 7)):
        CASES.append(Case("sample_intervals-%dx%dx%d" % s, ["refnerf_sample_intervals"], sampler(*s)))

    def ipe(n):
        def fn(G):
            g = rng(n, 3)
            return dict(feat=_hip.integrated_pos_enc(G.f(T(f32(g.uniform(-2, 2, (n, 3)))), name="lmean"),
                                                     G.f(T(f32(g.uniform(1e-6, 1e-1, (n, 3)))), name="lvar")))
        return fn

    def ide(n):
        def fn(G):
            g = rng(n, 4)
            return dict(ide=_hip.integrated_dir_enc(G.f(T(f32(unit(g.standard_normal((n, 3))))), name="xyz"),
                                                    G.f(T(f32(g.uniform(0, 1, (n, 1)))), name="kappa_inv")))
        return fn
    for n in (1, 63, 257):
        CASES.append(Case(f"integrated_pos_enc-{n}", ["refnerf_integrated_pos_enc"], ipe(n)))
        CASES.append(Case(f"integrated_dir_enc-{n}", ["refnerf_integrated_dir_enc"], ide(n)))

    def render(R, N, optional):
        def fn(G):
            g = rng(R, N, 5)
            v3 = lambda name: G.f(T(f32(g.random((R, N, 3)))), name=name) if optional else None   # noqa: E731
            cfg = _hip.default_cfg(compute_extras=int(optional), render_srgb_mode=3 if optional else 0)
            tdist = np.sort(g.uniform(2, 6, (R, N + 1)), -1)
            return _hip.render_rays(cfg, G.f(T(f32(20 * g.random((R, N)) ** 3)), name="density"), G.f(T(f32(tdist)), name="tdist"),
                                    G.f(T(f32(unit(g.standard_normal((R, 3))))), name="directions"), G.f(T(f32(np.full(R, 6.0))), name="far"),
                                    rgb=G.f(T(f32(g.random((R, N, 3)))), name="rgb"), diffuse=v3("diffuse"), specular=v3("specular"),
                                    normals=v3("normals"), normals_pred=v3("normals_pred"),
                                    roughness=G.f(T(f32(g.random((R, N)))), name="roughness") if optional else None, tint=v3("tint"))
        return fn
    for R, N in ((1, 2), (3, 33), (5, 257)):
        for optional in (False, True):
            CASES.append(Case(f"render_rays-{R}x{N}-{'all' if optional else 'required'}", ["refnerf_render_rays"], render(R, N, optional)))

    def losses(R, N, optional, backward):
        def fn(G):
            g = rng(R, N, 6)
            a = lambda shape, name: G.f(T(f32(g.random(shape))), name=name)       # noqa: E731
            n3 = lambda name: G.f(T(f32(unit(g.standard_normal((R, N, 3))))), name=name) if optional else None    # noqa: E731
            rgb, gt, lm, w = a((R, 3), "r_rgb"), a((R, 3), "gt_rgb"), a((R,), "lossmult"), a((R, N), "weights")
            npred = G.f(T(f32(unit(g.standard_normal((R, N, 3))))), name="normals_pred")
            orient, nrm = (npred if optional else None), n3("normals")
            view = G.f(T(f32(unit(g.standard_normal((R, 3))))), name="viewdirs")
            if not backward:
                return dict(terms=_hip.losses_forward(rgb, gt, lm, w, orient, nrm, npred, view))
            up = a((3,), "upstream") if optional else None
            return dict(zip(("g_r_rgb", "g_weights", "g_normals_pred"),
                            _hip.losses_backward(rgb, gt, lm, w, orient, int(optional), nrm, npred, view, 0.5, 0.25, 2.0, upstream=up)))
        return fn
    for R in (1, 5, 257):
        for N in (3, 33, 128):
            for optional in (False, True):
                tag = f"{R}x{N}-{'all' if optional else 'data'}"
                CASES.append(Case(f"losses_forward-{tag}", ["refnerf_losses_forward"], losses(R, N, optional, False)))
                CASES.append(Case(f"losses_backward-{tag}", ["refnerf_losses_backward"], losses(R, N, optional, True)))

    # the pads of csrc/refnerf_layout.h in 32-bit words.  fp32 image: 8 fp32 prefetch steps of 64 x 8 floats, 4 bf16 steps and
    # 2 x 4 split steps of BT_STEP_FLOATS = 2048; its general-basis tail: another fp32 pad and another split pad; the chunked
    # 16-bit images: two chunks of 17 KB
    F32_PADS, CHUNK_PADS = 8 * 64 * 8 + 4 * 2048 + 8 * 2048, 2 * 17 * 1024 // 4

    def pack(id, kind, groups):
        pad_words = CHUNK_PADS if kind != _hip.PREC_F32 else F32_PADS + (8 * 64 * 8 + 8 * 2048 if groups > 1 else 0)

        def fn(G):
            P = G.f(T(_blob(groups)), name="params")
            basis = G.f(T(_basis_np(groups)), name="basis") if groups > 1 else None
            # the image starts out as sentinel words in the plain call too: whatever the entry leaves alone (PADS) then
            # compares equal, and must be the same words wherever the image lives
            n = int(_hip.lib().refnerf_packed_weights_bytes_basis(kind, groups)) // 4
            img = G.out((n,), name="image") if G.guarded else _sentinel_tensor(n)
            G.loose(img, PADS)
            assert _hip.pack_weights(P, img, precision=kind, basis=basis) is img
            left = int((img.view(torch.int32) == guards.SENTINEL_I32).sum())
            assert left == pad_words, f"{left} words of the image were left alone, the layout's pads are {pad_words}"
            want, have = _pack_digests()
            for key in [f"blob-G{groups}"] + ([f"basis-G{groups}"] if groups > 1 else []):
                assert have[key] == want["inputs"][key], (f"{key} is not the input tests/golden/pack_digests.json was recorded on: the INPUTS differ "
                                                          "(synthetic / geopoly or PARAM_KW changed), this says nothing about the packer")
            got = dict(bytes=4 * n, sha256=_sha(img.cpu().numpy()))
            assert got == want["images"][id], (f"{id}: the packed image is {got}, commit {want['commit'][:12]} packed {want['images'][id]} from the "
                                               "same inputs: the packer moved bytes (csrc/refnerf_pack.h)")
            return dict(image=img)
        return fn
    for name, kind in (("f32", _hip.PREC_F32), ("bf16", _hip.PREC_BF16), ("f16", _hip.PREC_F16), ("f16x2", _hip.PREC_F16X2),
                       ("f16x2_train", _hip.IMAGE_F16X2_TRAIN)):
        CASES.append(Case(f"pack_weights-{name}", ["refnerf_pack_weights"], pack(f"pack_weights-{name}", kind, 0)))
    for groups in (2, 7):
        CASES.append(Case(f"pack_weights_basis-G{groups}", ["refnerf_pack_weights_basis"], pack(f"pack_weights_basis-G{groups}", _hip.PREC_F32, groups)))


_stage_cases()


# ------------------------------------------------------------------------------------------------- rays and datasets
def _cameras(n_cams, W, H):
    """(pixtocam [3,3], camtoworlds [n,3,4], pixtocam_ndc [3,3]) of a small pinhole rig"""
    focal = 0.9 * W
    p2c = np.linalg.inv(np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1.0]]))
    g = rng(n_cams, W, H)
    c2w = np.zeros((n_cams, 3, 4))
    for k in range(n_cams):
        q, _ = np.linalg.qr(g.standard_normal((3, 3)))
        c2w[k, :, :3], c2w[k, :, 3] = q, g.uniform(-1, 1, 3) + np.array([0, 0, 4.0])
    return f32(p2c), f32(c2w), f32(p2c)


def _distortion():
    from refnerf_pl_amd import camera_utils
    return camera_utils.lens_distortion(dict(k1=-0.1, k2=0.02, p1=1e-3, p2=-2e-3))


def _ray_cases():
    W, H = 19, 13

    def p2r(n, distorted, ndc, per_ray):
        def fn(G):
            g = rng(n, 8)
            p2c, c2w, p2c_ndc = _cameras(n if per_ray else 1, W, H)
            px = G.i(T(g.integers(0, W, n).astype(np.int32)), 0, name="pix_x")
            py = G.i(T(g.integers(0, H, n).astype(np.int32)), 0, name="pix_y")
            p2c_t = G.f(T(np.tile(p2c, (n, 1, 1)) if per_ray else p2c), name="pixtocams")
            c2w_t = G.f(T(c2w if per_ray else c2w[0]), name="camtoworlds")
            res = _hip.pixels_to_rays(px, py, p2c_t, c2w_t, G.f(T(p2c_ndc), name="pixtocam_ndc") if ndc else None,
                                      _distortion() if distorted else None)
            return dict(zip(("origins", "directions", "viewdirs", "radii", "imageplane"), res))
        return fn
    for n in (1, 255, 257):
        for distorted in (False, True):
            for ndc in (False, True):
                CASES.append(Case(f"pixels_to_rays{'_distorted' if distorted else ''}-{n}{'-ndc' if ndc else ''}",
                                  ["refnerf_pixels_to_rays_distorted" if distorted else "refnerf_pixels_to_rays"], p2r(n, distorted, ndc, False)))
    CASES.append(Case("pixels_to_rays-257-per-ray-cameras", ["refnerf_pixels_to_rays"], p2r(257, False, False, True)))

    def image_rays(projection, first, count, distorted=False, ndc=False):
        W, H = (19, 13) if count is None else (29, 23)       # a whole small frame; a range inside 667 pixels

        def fn(G):
            p2c, c2w, p2c_ndc = _cameras(3, W, H)
            return _hip.image_rays(projection, W, H, G.f(T(p2c), name="pixtocam") if projection == _hip.PROJ_PINHOLE else None,
                                   G.f(T(c2w), name="camtoworlds"), 1, 2.0, 6.0, G.f(T(p2c_ndc), name="pixtocam_ndc") if ndc else None,
                                   _distortion() if distorted else None, first=first, count=count)
        return fn
    for name, proj in (("pinhole", _hip.PROJ_PINHOLE), ("spherical", _hip.PROJ_SPHERICAL)):
        CASES.append(Case(f"image_rays-{name}-frame", ["refnerf_image_rays"], image_rays(proj, 0, None)))
        CASES.append(Case(f"image_rays-{name}-range-37+301", ["refnerf_image_rays"], image_rays(proj, 37, 301)))
    CASES.append(Case("image_rays-pinhole-distorted-ndc-range-37+301", ["refnerf_image_rays"], image_rays(_hip.PROJ_PINHOLE, 37, 301, True, True)))

    def prepare(f32_src, op, Cn, factor, alpha):
        def fn(G):
            g = rng(Cn, factor, 9)
            shape = (2, 26, 38, Cn) if Cn > 1 else (2, 26, 38)
            src = g.integers(0, 256, shape)
            src = G.f(T(f32(src / 3.0)), name="src") if f32_src else G.i(T(src.astype(np.uint8)), None, name="src")
            res = _hip.prepare_images(src, op, factor, return_alpha=alpha)
            return dict(zip(("out", "alpha"), res)) if alpha else dict(out=res)
        return fn
    for f32_src in (False, True):
        for factor in (1, 2):
            for name, op, Cn, alpha in (("scale", _hip.PREP_SCALE, 3, False), ("white", _hip.PREP_WHITE, 4, True),
                                        ("normals", _hip.PREP_NORMALS, 3, False), ("raw", _hip.PREP_RAW, 1, False)):
                CASES.append(Case(f"prepare_images-{'f32' if f32_src else 'u8'}-{name}-factor{factor}", ["refnerf_prepare_images"],
                                  prepare(f32_src, op, Cn, factor, alpha)))

    def batch(P, ps, distorted, int64, side):
        def fn(G):
            g = rng(P, ps, 10)
            n = 3
            p2c, c2w, _ = _cameras(n, W, H)
            dt = np.int64 if int64 else np.int32
            px0 = G.i(T(g.integers(0, W - ps + 1, P).astype(dt)), 0, name="px0")
            py0 = G.i(T(g.integers(0, H - ps + 1, P).astype(dt)), 0, name="py0")
            cam = G.i(T(g.integers(0, n, P).astype(dt)), 0, name="cam")
            a = lambda shape, name: G.f(T(f32(g.random(shape))), name=name)       # noqa: E731
            extra = dict(disps=a((n, H, W), "disps"), normals=a((n, H, W, 3), "normals"), alphas=a((n, H, W), "alphas")) if side else {}
            rays, got = _hip.train_batch(px0, py0, cam, ps, a((n, H, W, 3), "images"), G.f(T(p2c), name="pixtocams"),
                                         G.f(T(c2w), name="camtoworlds"), 2.0, 6.0, distortion=_distortion() if distorted else None, **extra)
            return {**rays, **got}
        return fn
    for P in (1, 257):
        for ps in (1, 2):
            for distorted in (False, True):
                CASES.append(Case(f"train_batch-{P}-patch{ps}{'-distorted' if distorted else ''}", ["refnerf_train_batch"],
                                  batch(P, ps, distorted, int64=(ps == 2), side=(ps == 2) != distorted)))

    def noisy(n, a):
        def fn(G):
            g = rng(n, a, 11)
            rot = np.stack([np.linalg.qr(g.standard_normal((3, 3)))[0] for _ in range(a)])
            fields = [G.f(T(f32(g.random((n, w)))), name=name) for name, w in zip(_hip.RAY_FIELDS, _hip.RAY_FIELD_WIDTHS)]
            outs = _hip.noisy_rays(G.f(T(f32(rot)), name="rotations"), G.f(T(f32(g.uniform(2, 6, n))), name="distance"), fields)
            return dict(zip(_hip.RAY_FIELDS, outs))
        return fn
    for n, a in ((1, 1), (37, 3), (257, 2)):
        CASES.append(Case(f"noisy_rays-{n}x{a}", ["refnerf_noisy_rays"], noisy(n, a)))


_ray_cases()


# ------------------------------------------------------------------------------------------------- loss kernels
def _loss_cases():
    def regularisers(R, S, backward, everything):
        def fn(G):
            g = rng(R, S, 12)
            n, a = (max(R // 2, 1), 2) if everything else (0, 0)
            na = n * a
            r = lambda shape, name: G.f(T(f32(g.random(shape))), name=name)       # noqa: E731
            u = lambda m, name: G.f(T(f32(unit(g.standard_normal((m, 3))))), name=name)    # noqa: E731
            w = g.random((R, S)) ** 4
            weights = G.f(T(f32(w / w.sum(-1, keepdims=True) * g.uniform(0.2, 1.0, (R, 1)))), name="weights")
            acc = r((R,), "acc")
            clean, noisy_, rays, nrays = {}, {}, (None, None), (None, None)
            if everything:
                clean = dict(distance=r((R,), "distance"), diffuse=r((R, 3), "diffuse"), specular=r((R, 3), "specular"), normals=u(R, "normals"))
                noisy_ = dict(distance=r((na,), "n_distance"), diffuse=r((na, 3), "n_diffuse"), specular=r((na, 3), "n_specular"), normals=u(na, "n_normals"))
                rays, nrays = (r((R, 3), "origins"), u(R, "directions")), (r((na, 3), "n_origins"), u(na, "n_directions"))
            A, _, _ = _hip.regularisers_args(weights if everything or S == 33 else None, acc, clean, noisy_, rays, nrays, n, a, 0.3, 0.3,
                                             (_hip.CONSISTENCY_TYPES["mse"], _hip.CONSISTENCY_TYPES["var"], _hip.CONSISTENCY_TYPES["mse"]))
            if not backward:
                return dict(terms=_hip.ray_regularisers_forward(A, DEV))
            sums = G.f(T(f32([0.5 * R, max(R // 2, 1), 0.3 * R, 0.1, 0.2, 0.3, 0.4, max(n // 2, 1)])), name="sums")
            out = _hip.ray_regularisers_backward(A, sums, r((6,), "scales"))
            return {k: v for k, v in out.items() if v is not None}
        return fn
    for R in (1, 37, 257):
        for S in (33, 65):
            for everything in (True, False):
                tag = f"{R}x{S}-{'all' if everything else 'acc-entropy'}"
                CASES.append(Case(f"ray_regularisers_forward-{tag}", ["refnerf_ray_regularisers_forward"], regularisers(R, S, False, everything)))
                CASES.append(Case(f"ray_regularisers_backward-{tag}", ["refnerf_ray_regularisers_backward"], regularisers(R, S, True, everything)))

    def data_terms(R, penalty, groups, backward):
        def fn(G):
            g = rng(R, 13)
            r = lambda shape, name: G.f(T(f32(g.random(shape))), name=name)       # noqa: E731
            kw = {}
            if groups:
                kw = dict(distance_mean=r((R,), "distance_mean"), disps=r((R,), "disps"), acc=r((R,), "acc"), alphas=r((R,), "alphas"),
                          normals=G.f(T(f32(g.standard_normal((R, 3)))), name="normals"), normals_gt=G.f(T(f32(unit(g.standard_normal((R, 3))))), name="normals_gt"))
            keep = (r((R, 3), "rgb"), r((R, 3), "gt_rgb"), r((R,), "lossmult"), r((1,), "upstream"))   # (the struct holds pointers only)
            A = _hip.data_terms_args(*keep[:3], penalty, 1e-3, **kw)
            if backward:
                return dict(g_rgb=_hip.data_terms_backward(A, keep[3]))
            return dict(terms=_hip.data_terms_forward(A, DEV))
        return fn
    for R in (1, 37, 257):
        for penalty in ("mse", "charb"):
            groups = penalty == "charb" or R == 37
            CASES.append(Case(f"data_terms_forward-{R}-{penalty}", ["refnerf_data_terms_forward"], data_terms(R, penalty, groups, False)))
            CASES.append(Case(f"data_terms_backward-{R}-{penalty}", ["refnerf_data_terms_backward"], data_terms(R, penalty, groups, True)))

    def smoothness(P, S, backward):
        def fn(G):
            g = rng(P, S, 14)
            r = lambda shape, name: G.f(T(f32(g.random(shape))), name=name)       # noqa: E731
            keep = (r((P, S, S), "distance"), r((P, S, S), "acc"), r((P, S, S, 3), "rgb"), r((1,), "upstream"))   # (the struct holds pointers only)
            A = _hip.depth_smoothness_args(*keep[:3])
            if backward:
                return dict(g_distance=_hip.depth_smoothness_backward(A, keep[3]))
            return dict(terms=_hip.depth_smoothness_forward(A, DEV))
        return fn
    for P, S in ((1, 2), (130, 8)):
        CASES.append(Case(f"depth_smoothness_forward-{P}x{S}", ["refnerf_depth_smoothness_forward"], smoothness(P, S, False)))
        CASES.append(Case(f"depth_smoothness_backward-{P}x{S}", ["refnerf_depth_smoothness_backward"], smoothness(P, S, True)))

    def knots(g, R, n):
        t = np.sort(g.random((R, n + 1)), -1)
        t[:, 0], t[:, -1] = 0.0, 1.0
        return f32(t)

    def dilate(R, M):
        def fn(G):
            g = rng(R, M, 15)
            sd, wd = _hip.max_dilate_weights(G.f(T(knots(g, R, M)), name="t"), G.f(T(f32(g.random((R, M)) ** 3)), name="w"), 0.01, 0.0, 1.0)
            return dict(sdist=sd, weights=wd)
        return fn
    for R in (1, 37):
        for M in (1, 65, 171):
            CASES.append(Case(f"max_dilate_weights-{R}x{M}", ["refnerf_max_dilate_weights"], dilate(R, M)))

    def interlevel(R, N, Np, backward):
        def fn(G):
            g = rng(R, N, Np, 16)
            wn = lambda n: f32((lambda w: w / w.sum(-1, keepdims=True))(g.random((R, n)) ** 3))    # noqa: E731
            args = (G.f(T(knots(g, R, N)), name="t"), G.f(T(wn(N)), name="w"), G.f(T(knots(g, R, Np)), name="t_env"), G.f(T(wn(Np)), name="w_env"))
            if backward:
                return dict(g_w_env=_hip.interlevel_backward(*args, G.f(T(f32([0.7])), name="upstream")))
            return dict(ray_loss=_hip.interlevel_forward(*args))
        return fn
    for R in (1, 37, 257):
        for N, Np in ((33, 63), (512, 512)):
            CASES.append(Case(f"interlevel_forward-{R}x{N}x{Np}", ["refnerf_interlevel_forward"], interlevel(R, N, Np, False)))
            CASES.append(Case(f"interlevel_backward-{R}x{N}x{Np}", ["refnerf_interlevel_backward"], interlevel(R, N, Np, True)))


_loss_cases()


# ------------------------------------------------------------------------------------------------- optimiser
def _optim_cases():
    INPLACE = "refnerf_hip.h, refnerf_optim_adam_step: torch's Adam update in place (d_param, d_exp_avg, d_exp_avg_sq; d_grad with write_grad)"

    def step(n, off, no_step=False):
        def fn(G):
            g = rng(n, 17)
            if n == 1:
                seg = [0, 1]
            elif n == 3:
                seg = [0, 1, 2, 3]                         # segments of length 1 only
            else:
                seg = [0, 1, 2, n // 3, n // 3 + 1, n - 1, n]    # length-1 segments at both ends and in the middle
            base = [G.inout(T(f32(np.concatenate([np.full(off, 7.5), v]))), INPLACE, name=name)
                    for name, v in (("param", g.standard_normal(n)), ("grad", 3 * g.standard_normal(n)), ("exp_avg", 0.1 * g.standard_normal(n)),
                                    ("exp_avg_sq", 0.01 * g.random(n)))]
            p, gr, m, v = (b[off:] for b in base)        # off = 1: one element off a 16-byte boundary
            ws, stats, n_items = _hip.optim_plan(n, seg, DEV)
            state = _hip.optim_state(1, DEV)
            _hip.optim_stats(gr, p, len(seg) - 1, n_items, 2.0, ws, stats, state, 0)
            _hip.optim_finalize(state, 1, 1.5)
            cfg = _hip.AdamCfg(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, bias_correction1=1 - 0.9 ** 3, sqrt_bias_correction2=math.sqrt(1 - 0.999 ** 3),
                               grad_max_val=2.0, write_grad=1, no_step=int(no_step))
            if no_step:
                _hip.optim_adam_step(None, gr, None, None, cfg, state)
            else:
                _hip.optim_adam_step(p, gr, m, v, cfg, state)
            # (the rest of the state is the library's table of the step's tensors: their addresses)
            return dict(param=base[0], grad=base[1], exp_avg=base[2], exp_avg_sq=base[3], seg_stats=stats, norm_and_clip=state[:16])
        return fn
    entries = ["refnerf_optim_plan", "refnerf_optim_stats", "refnerf_optim_finalize", "refnerf_optim_adam_step"]
    for n in (1, 3, 255, 1025):
        CASES.append(Case(f"optim-step-{n}", entries, step(n, 0)))
        CASES.append(Case(f"optim-step-{n}-off-16B-boundary", entries, step(n, 1)))
    CASES.append(Case("optim-clip-only-255", entries, step(255, 0, no_step=True)))


_optim_cases()


# ------------------------------------------------------------------------------------------------- image metrics, panels
def _image_cases():
    H, W, Cn = 13, 17, 3
    WS = "refnerf_hip.h, image entries: d_workspace holds the per-workgroup partials (scratch)"

    def image(G, g, pitched, name, Cn=Cn):
        """a float64 [H, W, C] image: contiguous, or the interior crop of a [H+2, W+3, C] parent whose border -- the view's
        pitch padding -- holds what the red zones hold; the arena also checks that no byte of the parent changes"""
        x = g.random((H, W, Cn))
        if not pitched:
            return G.f(T(x), name=name)
        parent = np.full((H + 2, W + 3, Cn), G.zone)
        parent[1:H + 1, 2:W + 2] = x
        return G.f(T(parent), name=name + "_parent")[1:H + 1, 2:W + 2]

    def metric(which, pitched):
        def fn(G):
            g = rng(18)
            a, b = image(G, g, pitched, "a"), image(G, g, pitched, "b")
            ws = G.scratch((_hip.lib().refnerf_image_workspace_bytes(H, W, Cn) // 8,), torch.float64, WS, name="workspace")
            if which == "mse":
                return dict(out=_hip.image_mse(a, b, quantize_a=True, workspace=ws))
            if which == "ssim":
                s, smap = _hip.image_ssim(a, b, quantize_a=True, return_map=True, workspace=ws)
                return dict(ssim=s, map=smap)
            out, warp = _hip.color_correct(a, b, num_iters=3, return_warp=True, workspace=ws)
            return dict(out=out, warp=warp)
        return fn
    for pitched in (False, True):
        tag = "pitched" if pitched else "contiguous"
        CASES.append(Case(f"image_mse-{tag}", ["refnerf_image_mse"], metric("mse", pitched)))
        CASES.append(Case(f"image_ssim-{tag}", ["refnerf_image_ssim"], metric("ssim", pitched)))
        CASES.append(Case(f"color_correct-{tag}", ["refnerf_color_correct"], metric("cc", pitched)))

    def mae(pitched):
        def fn(G):
            g = rng(19)
            w = image(G, g, pitched, "weights", 1)
            n, ngt = (image(G, g, pitched, k) for k in ("normals", "normals_gt"))
            ws = G.scratch((_hip.lib().refnerf_image_workspace_bytes(1, H * W, 1) // 8,), torch.float64, WS, name="workspace")
            # (this entry takes dense tensors: the wrapper hands it its own dense copies of the crops)
            return dict(out=_hip.weighted_mae(w, n, ngt, workspace=ws))
        return fn
    CASES.append(Case("weighted_mae-contiguous", ["refnerf_weighted_mae"], mae(False)))
    CASES.append(Case("weighted_mae-from-pitched", ["refnerf_weighted_mae"], mae(True)))

    def percentile(Hh, Ww, f64, weighted):
        def fn(G):
            g = rng(Hh, Ww, 20)
            n = Hh * Ww
            value = 2.1 + 3.8 * ((g.permutation(n) + g.uniform(0.1, 0.9, n)) / n)
            value = value if f64 else f32(value)
            order = G.i(T(np.argsort(value, kind="stable").astype(np.int64)), 0, name="order")
            wt = g.random(n) if f64 else f32(g.random(n))
            mask = np.where(g.random(n) < 0.1, np.nan, 1.0).astype(wt.dtype)
            ws = G.scratch((_hip.lib().refnerf_vis_percentile_workspace_bytes(n) // 8,), torch.float64,
                           "refnerf_hip.h, refnerf_vis_weighted_percentile: d_workspace holds the block sums and the scan (scratch)", name="workspace")
            return dict(out=_hip.vis_weighted_percentile(G.f(T(value), name="values"), G.f(T(wt), name="weights") if weighted else None, order,
                                                         [0.5, 5.0, 37.0, 95.0, 99.5], nan_mask=G.f(T(mask), name="nan_mask") if weighted else None,
                                                         workspace=ws))
        return fn
    for Hh, Ww in ((5, 7), (12, 21), (37, 53), (96, 128)):      # tests/test_vis.py's sizes: 35, 252, 1961 and 12288 values
        CASES.append(Case(f"vis_weighted_percentile-{Hh}x{Ww}-f32", ["refnerf_vis_weighted_percentile"], percentile(Hh, Ww, False, True)))
    CASES.append(Case("vis_weighted_percentile-37x53-f64-unit", ["refnerf_vis_weighted_percentile"], percentile(37, 53, True, False)))

    def panels(Hh, Ww, f64):
        def fn(G):
            g = rng(Hh, Ww, 21)
            dt = np.float64 if f64 else np.float32
            r = lambda shape, name: G.f(T(g.random(shape).astype(dt)), name=name)      # noqa: E731
            dist = 2 + 4 * g.random((Hh, Ww))
            dist[g.random((Hh, Ww)) < 0.02] = np.nan
            d = lambda delta, name: G.f(T((dist + delta).astype(dt)), name=name)       # noqa: E731
            inputs = dict(rgb=r((Hh, Ww, 3), "rgb"), acc=r((Hh, Ww), "acc"), distance_mean=d(0, "distance_mean"), distance_median=d(0.01, "distance_median"),
                          distance_p5=d(-0.2, "distance_p5"), distance_p95=d(0.2, "distance_p95"), origins=r((Hh, Ww, 3), "origins"),
                          directions=G.f(T((g.random((Hh, Ww, 3)) - 0.5).astype(dt)), name="directions"), roughness=r((Hh, Ww, 1), "roughness"),
                          diffuse=r((Hh, Ww, 3), "diffuse"), specular=r((Hh, Ww, 3), "specular"), tint=r((Hh, Ww, 3), "tint"), rgb_cc=r((Hh, Ww, 3), "rgb_cc"))
            lohi = [G.f(T(np.array(v, np.float64)), name=k) for k, v in (("lohi_mean", [2.2, 5.7]), ("lohi_median", [2.3, 5.8]), ("lohi_triplet", [2.1, 5.9]))]
            normals = [G.f(T(unit(g.standard_normal((Hh, Ww, 3))).astype(dt)), name=f"normals{k}") for k in range(3)]
            table = G.f(T(f32(g.random((256, 3)))), name="table")
            out = _hip.vis_panels(Hh, Ww, torch.float64 if f64 else torch.float32, True, table, inputs,
                                  [n[2:] for n in _hip.VIS_PANEL_OUTPUTS + _hip.VIS_PANEL_OUTPUTS_2], lohi, normals)
            res = {k: v for k, v in out.items() if k != "normals_out"}
            res.update({f"normals_out{k}": v for k, v in enumerate(out["normals_out"])})
            return res
        return fn
    CASES.append(Case("vis_panels-37x53-f32", ["refnerf_vis_panels"], panels(37, 53, False)))
    CASES.append(Case("vis_panels-5x7-f64", ["refnerf_vis_panels"], panels(5, 7, True)))

    def cmap(Hh, Ww, table):
        def fn(G):
            g = rng(Hh, Ww, 22)
            ch = 1 if table else 3
            values = G.f(T(f32(2 + 4 * g.random((Hh, Ww, ch)))), name="values")
            alpha = np.where(g.random((Hh, Ww)) < 0.2, 0.0, 1.0)
            kw = dict(curve="neg_log", normalise=True, d_lo=G.f(T(np.array([2.2])), name="lo"), lo_bias=-1e-7, d_hi=G.f(T(np.array([5.8])), name="hi"),
                      hi_bias=1e-7, table=G.f(T(f32(g.random((256, 3)))), name="table"), alpha=G.f(T(alpha), name="alpha")) if table else {}
            return dict(out=_hip.vis_cmap(values, Hh, Ww, ch, torch.float32 if table else torch.float64, acc=G.f(T(f32(g.random((Hh, Ww)))), name="acc"), **kw))
        return fn
    for Hh, Ww in ((5, 7), (37, 53)):
        CASES.append(Case(f"vis_cmap-{Hh}x{Ww}-table", ["refnerf_vis_cmap"], cmap(Hh, Ww, True)))
        CASES.append(Case(f"vis_cmap-{Hh}x{Ww}-matte", ["refnerf_vis_cmap"], cmap(Hh, Ww, False)))

    def ray_lines(n, levels, res, accumulate):
        def fn(G):
            g = rng(n, res, 23)
            L = len(levels)
            edges = G.f(T(np.linspace(0, 1, res + 1)), name="edges")
            if accumulate:
                why = "refnerf_hip.h, refnerf_vis_resample_rays: accumulate adds visualize_rays' accumulated colour and weight into the lines"
                lv, la = G.scratch((n, L, res, 3), torch.float64, why, 0.0, "lines_values"), G.scratch((n, L, res), torch.float64, why, 0.0, "lines_alpha")
            else:
                lv, la = G.out((n, L, res, 3), torch.float64, "lines_values"), G.out((n, L, res), torch.float64, "lines_alpha")
            for lvl, N in enumerate(levels):
                s = np.sort(g.random((n, N + 1)), -1)
                s[:, 0], s[:, -1] = 0.0, 1.0
                if n > 1:
                    s[1] = 0.1 + 0.8 * s[1]        # a ray that spans [0.1, 0.9] only: the extrapolation outside
                _hip.vis_resample_rays(G.f(T(f32(s)), name=f"sdist{lvl}"), G.f(T(f32(1.2 * g.random((n, N, 3)))), name=f"values{lvl}"),
                                       G.f(T(f32(g.random((n, N)) / N)), name=f"weights{lvl}"), edges, lv, la, lvl, accumulate=accumulate,
                                       value_op="clip01" if accumulate else "none")
            out = dict(lines_values=lv, lines_alpha=la)
            if not accumulate:
                rep = max(res // (n * L + 1), 1)
                out["panel"], out["panel_alpha"] = _hip.vis_ray_panel(lv, la, rep, 0.8, G.f(T(np.array([0.7])), name="alpha_max"))
                out["panel0"], out["panel0_alpha"] = _hip.vis_ray_panel(lv, la, 0, 0.8)
            return out
        return fn
    both = ["refnerf_vis_resample_rays", "refnerf_vis_ray_panel"]
    CASES.append(Case("vis_rays-3x(5,9)-res64", both, ray_lines(3, (5, 9), 64, False)))
    CASES.append(Case("vis_rays-2x(33,)-res300", both, ray_lines(2, (33,), 300, False)))
    CASES.append(Case("vis_resample_rays-accumulate-3x(5,9)-res64", both[:1], ray_lines(3, (5, 9), 64, True)))


_image_cases()

assert len({c.id for c in CASES}) == len(CASES), "case ids repeat"


# ------------------------------------------------------------------------------------------------- the driver
def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b, tol, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        if tol is None or not x.dtype.is_floating_point:
            diff = (_bits(x) != _bits(y))
            assert not bool(diff.any()), f"{what}: {k} differs in {int(diff.sum())} bytes, first at element {int(diff.nonzero()[0]) // x.element_size()} of {tuple(x.shape)}"
        else:
            torch.testing.assert_close(x, y, rtol=tol[0], atol=tol[1], equal_nan=True, msg=lambda m: f"{what}: {k}: {m}")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_guard_bands(case):
    _hip.require_device()
    try:
        _run_case(case)
    except (_hip.HipLibraryError, RuntimeError) as e:
        if isinstance(e, _hip.HipLibraryError) or "HIP error" in str(e) or "hip error" in str(e):
            pytest.exit(f"{case.id}: the HIP runtime reported an error; nothing more is started on this device: {e}", returncode=3)
        raise


def _run_case(case):
    plain = case.fn(PlainAlloc())
    torch.cuda.synchronize()
    runs = []
    for zone in (0.0, NAN):
        arena = guards.Arena(DEV, float_zone=zone)
        with guards.guarded(arena, hip=_hip):
            runs.append(case.fn(GuardedAlloc(arena)))
        torch.cuda.synchronize()
        arena.check()                                                    # (a)
        for k, t in runs[-1].items():
            assert arena.holds(t), f"{k} was not allocated under guard"
    _same(plain, runs[0], case.tol, "plain vs guarded")                  # (b)
    _same(runs[0], runs[1], case.tol, "red zones 0 vs NaN")              # (c)


# ------------------------------------------------------------------------------------------------- per-sample parity
# bf16 has no project bound for per-sample values.  BF16_FIXTURE_GAP is the worst |bf16 mode - f32 mode| per key over both
# levels of the fixture batch model_blender_sharp_eval (24 rays x 128 samples, where test_bf16_mode_tolerance accepts the mode),
# both modes fed the same step function at each level, on rays whose bins agree; measured on an MI355X by
# test_bf16_fixture_gap_is_as_recorded below.  The ragged shapes, which differ in R and N only, get twice that.
BF16_FIXTURE_GAP = {"sdist": 5.97e-7, "weights": 4.26e-5, "density": 2.33e-3, "rgb": 2.91e-5, "normals_pred": 6.15e-2,       # MEASURED on
                    "roughness": 6.02e-5, "diffuse": 3.62e-5, "specular": 5.19e-5, "tint": 6.97e-5}                           # an MI355X:
# 5.960e-07, 4.252e-05, 2.329e-03, 2.909e-05, 6.146e-02, 6.017e-05, 3.618e-05, 5.180e-05, 6.962e-05 (the constants round them up).
BF16_RAGGED_FACTOR = 2.0


def _plain_rays(rays):
    return {k: (T(f32(rays[k])).reshape(-1) if k in ("radii", "near", "far") else T(f32(rays[k])))
            for k in ("origins", "directions", "viewdirs", "radii", "near", "far")}


@functools.lru_cache(maxsize=None)
def _oracle_chain(shape, training):
    """(rays, [(sdist_in, weights_in, the oracle's outputs)] level by level) of one ragged shape: level 0 resamples the
    initial step function into n_in samples, level 1 the ORACLE's level-0 output into N.  Computed once per shape and
    shared by the comparisons below, which leave it unchanged."""
    from oracle import oracle as O
    from refnerf_pl_amd import synthetic
    R, n_in, N = shape
    rays = synthetic.blender_rays(R, seed=R, center_frac=0.5)
    sd, w = step_function(R, 1)
    chain = []
    for n in ((n_in, N) if n_in > 1 else (N,)):
        orc = O.level_forward(_blob(0), O.default_cfg(n_samples=n, n_in=w.shape[1], training=int(training)), rays, sd, w, history=True)
        chain.append((sd, w, orc))
        sd, w = orc["sdist"], orc["weights"]
    return rays, chain


def _hip_level(prec, training, rays, sd, w, n):
    cfg = _hip.default_cfg(n_samples=n, n_in=w.shape[1], precision=PREC[prec], training=int(training))
    res = _hip.level_forward(_plain_image(_hip.level_image(PREC[prec], training, 0))[2], cfg, rays, T(sd), T(w))
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("shape", LEVEL_SHAPES, ids=["%dx%dx%d" % s for s in LEVEL_SHAPES])
def test_per_sample_outputs_at_ragged_shapes_vs_oracle(shape, mode):
    """f32 mode, eval and training forward: fed the oracle's own step function at every level, bin_idx and sdist are
    bit-equal to the oracle's (the fused-level contract of the README) and every per-sample output is within the project's
    per-sample bounds for random-init weights (test_hip_parity.hist_tol of a non-wide case); in training the density
    normals follow the bulk / tail rule of test_training_forward_density_normals."""
    from test_hip_parity import hist_tol
    _hip.require_device()
    training = mode == "train"
    rays_np, chain = _oracle_chain(shape, training)
    rays = _plain_rays(rays_np)
    for L, (sd, w, orc) in enumerate(chain):
        res = _hip_level("f32", training, rays, sd, w, orc["weights"].shape[1])
        assert np.array_equal(res["bin_idx"], orc["bin_idx"]), f"L{L}: bin_idx differs from the oracle's"
        assert np.array_equal(res["sdist"], orc["sdist"]), f"L{L}: sdist is not bit-equal to the oracle's"
        for k in HIST_KEYS:
            rtol, atol = hist_tol("ragged", L, k)
            err = float(np.abs(res[k] - orc[k].reshape(res[k].shape)).max())
            print(f"MEASURED {shape} {mode} L{L} {k}: {err:.2e} (bound {atol:.0e})")
            np.testing.assert_allclose(res[k], orc[k].reshape(res[k].shape), rtol=rtol, atol=atol, err_msg=f"L{L} {k}")
        if training:
            err = np.abs(res["normals"] - orc["normals"].reshape(res["normals"].shape)).max(-1)
            print(f"MEASURED {shape} train L{L} normals: median {np.median(err):.2e}, share below 1e-3 {np.mean(err < 1e-3):.4f}")
            # ill-conditioned where the density gradient is tiny: bulk tight, tail loose
            assert np.median(err) < 2e-5 and np.mean(err < 1e-3) > 0.99, (L, np.median(err), np.mean(err < 1e-3))


def _gap_to_f32_mode(prec, rays, sd, w, n, gap):
    """per-key worst |mode - f32 mode| of one level, both fed (sd, w), on the rays whose bins agree -> updates `gap`"""
    a, b = _hip_level("f32", False, rays, sd, w, n), _hip_level(prec, False, rays, sd, w, n)
    ok = (a["bin_idx"] == b["bin_idx"]).all(-1)
    for k in HIST_KEYS:
        if ok.any():
            gap[k] = max(gap.get(k, 0.0), float(np.abs(a[k][ok] - b[k][ok]).max()))
    return a, ok


@pytest.mark.parametrize("prec", ["f16x2", "bf16"])
@pytest.mark.parametrize("shape", LEVEL_SHAPES, ids=["%dx%dx%d" % s for s in LEVEL_SHAPES])
def test_per_sample_outputs_at_ragged_shapes_16bit_vs_f32_mode(shape, prec):
    """the same per-sample comparison of the 16-bit modes against the f32 mode, both fed the oracle's step functions, on
    the rays whose bins agree: f16x2 within hist_tol (which holds every per-sample key; its resampler is the fp32 parity
    code, so its bins and sdist are the f32 mode's bit for bit), bf16 within twice its gap on the fixture batch"""
    from test_hip_parity import hist_tol
    _hip.require_device()
    rays_np, chain = _oracle_chain(shape, False)
    rays = _plain_rays(rays_np)
    for L, (sd, w, orc) in enumerate(chain):
        gap = {}
        a, ok = _gap_to_f32_mode(prec, rays, sd, w, orc["weights"].shape[1], gap)
        print(f"MEASURED {shape} {prec} L{L}: rays whose bins agree {int(ok.sum())} of {ok.size}; gaps {gap}")
        if prec == "f16x2":
            assert ok.all(), f"L{L}: the f16x2 mode's bins differ from the f32 mode's on identical inputs"
        for k, v in gap.items():
            bound = hist_tol("ragged", L, k)[1] if prec == "f16x2" else BF16_RAGGED_FACTOR * BF16_FIXTURE_GAP[k]
            assert v <= bound, f"L{L} {k}: {v:.3e} > {bound:.3e}"


def test_bf16_fixture_gap_is_as_recorded():
    """BF16_FIXTURE_GAP is what this machine measures on the fixture batch"""
    from helpers import cfg_from_bindings
    _hip.require_device()
    g = load_golden("model_blender_sharp_eval")
    P, rays_np = params_from_golden(g), rays_from_golden(g)
    kw, lv = cfg_from_bindings(g["bindings"])
    assert not kw, "the fixture runs on the default level cfg"
    rays = _plain_rays(rays_np)
    images = {p: _hip.pack_weights(T(P), precision=PREC[p]) for p in ("f32", "bf16")}
    R = rays_np["origins"].shape[0]
    sd, w = (T(a) for a in step_function(R, 1))
    gap = {}
    for L in range(2):
        n = lv.get("num_prop_samples" if L == 0 else "num_nerf_samples", 128)
        res = {p: _hip.level_forward(images[p], _hip.default_cfg(n_samples=n, n_in=w.shape[1], precision=PREC[p]), rays, sd, w) for p in images}
        ok = (res["f32"]["bin_idx"] == res["bf16"]["bin_idx"]).all(-1)
        assert float(ok.float().mean()) >= 0.9
        for k in HIST_KEYS:
            gap[k] = max(gap.get(k, 0.0), float((res["f32"][k][ok] - res["bf16"][k][ok]).abs().max()))
        sd, w = res["f32"]["sdist"], res["f32"]["weights"]
    print("MEASURED bf16 - f32 mode on model_blender_sharp_eval:", {k: f"{v:.3e}" for k, v in gap.items()})
    for k in HIST_KEYS:
        assert gap[k] <= BF16_FIXTURE_GAP[k], f"{k}: measured {gap[k]:.3e}, recorded {BF16_FIXTURE_GAP[k]:.3e}"

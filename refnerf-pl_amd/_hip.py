"""ctypes binding of librefnerf_hip.so (include/refnerf_hip.h, include/refnerf_distortion.h for the distortion loss,
include/refnerf_tsdf.h for geometry export and include/refnerf_raycast.h for views of the exported volume).

PyTorch is used only for device memory and streams: every call takes raw
device pointers (``tensor.data_ptr()``) and the current HIP stream.  There is
no CPU fallback -- if the library or a gfx950 device is missing the call
raises.
"""
import ctypes as C
import os
import subprocess

import torch

from . import _abi
from ._abi import HipLibraryError  # noqa: F401

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "librefnerf_hip.so")
if os.environ.get("REFNERF_LIB"):      # A/B builds of the library (scripts/build_*_variant.sh -> ab/*.so): a debug knob, never a fallback
    LIB_PATH = os.path.abspath(os.environ["REFNERF_LIB"])

# Every integer constant of the header under its name without the REFNERF_ prefix: ABI_VERSION, NUM_PARAMS, NUM_PARAMS_EXT,
# PREC_*, IMAGE_F16X2_TRAIN, ACT_* (ACT_F16X2 = 2 is retired: nothing writes or reads it), WGRAD_*, DIRENC_*, PROJ_*, PREP_*,
# TIMER_*, VIS_MAX_PS, VIS_MAX_NORMALS, ...
globals().update({name[len("REFNERF_"):]: value for name, value in _abi.constants.items() if name.startswith("REFNERF_")})


def _enum(prefix):
    """{lower-case name: value} of the header's enumerators REFNERF_<prefix>_*: the strings the reference's configs use"""
    prefix = "REFNERF_" + prefix + "_"
    return {name[len(prefix):].lower(): value for name, value in _abi.constants.items() if name.startswith(prefix)}


RAYDIST = _enum("RAYDIST")
RAYDIST[None] = RAYDIST.pop("none")     # Model.raydist_fn = None
SRGB_MODES = _enum("SRGB")
CONSISTENCY_TYPES = _enum("CONSISTENCY")
PENALTIES = _enum("PENALTY")
VIS_CURVES = _enum("VIS_CURVE")
VIS_OPS = _enum("VIS_OP")
# the distortion loss has a header of its own (refnerf_hip.h and its ABI version are untouched by it): two entries, no constants
DISTORTION_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "refnerf_distortion.h")
_distortion_prototypes = _abi.load(DISTORTION_HEADER)[2]
# geometry export likewise: TSDF fusion and marching tetrahedra, one struct (the voxel grid), four entries
TSDF_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "refnerf_tsdf.h")
_tsdf_constants, _tsdf_structs, _tsdf_prototypes = _abi.load(TSDF_HEADER)
TsdfGrid = _tsdf_structs["refnerf_tsdf_grid"]
# the ray caster of the fused volume: a header that includes refnerf_tsdf.h for the grid struct (the same class as TsdfGrid:
# _abi.load parses a header once), one entry of its own
RAYCAST_HEADER = os.path.join(os.path.dirname(_abi.HEADER), "refnerf_raycast.h")
_raycast_prototypes = _abi.load(RAYCAST_HEADER)[2]
LEGACY_F16X2_TRAIN = False   # the round-4 training kernels (REFNERF_LEGACY_F16X2_TRAIN) are gone; bench.py still reads this name
IPE_MAX_GROUPS = 7           # rn::IPE_MAX_GROUPS of the library: not part of the header

# the header's argument structs (layouts checked against the C compiler in tests/test_abi.py)
LevelCfg = _abi.structs["refnerf_level_cfg"]
RaysStruct = _abi.structs["refnerf_rays"]
LevelOut = _abi.structs["refnerf_level_out"]
LevelOutExtra = _abi.structs["refnerf_level_out_extra"]
LevelSaved = _abi.structs["refnerf_level_saved"]
LevelGrads = _abi.structs["refnerf_level_grads"]
LensDistortion = _abi.structs["refnerf_lens_distortion"]       # the keyword parameters of the reference's _radial_and_tangential_undistort
ImageRaysOut = _abi.structs["refnerf_image_rays_out"]          # the nine utils.Rays fields
TrainBatchArgs = _abi.structs["refnerf_train_batch_args"]
AdamCfg = _abi.structs["refnerf_adam_cfg"]                     # one Adam step's scalars, computed by the host in double
RegularisersArgs = _abi.structs["refnerf_regularisers_args"]   # sizes, thresholds, type enums, then one level's device pointers (None = term off)
NoisyRaysArgs = _abi.structs["refnerf_noisy_rays_args"]
DataTermsArgs = _abi.structs["refnerf_data_terms_args"]        # one level's data term and statistics (None = optional group absent)
DepthSmoothnessArgs = _abi.structs["refnerf_depth_smoothness_args"]   # one level of a [P,S,S] patch batch
VisPanelsArgs = _abi.structs["refnerf_vis_panels_args"]
VisCmapArgs = _abi.structs["refnerf_vis_cmap_args"]

OUT_FIELDS = ("d_sdist", "d_bin_idx", "d_density", "d_rgb", "d_normals", "d_normals_pred", "d_grad_pred",
              "d_tint", "d_diffuse", "d_specular", "d_roughness", "d_weights", "d_r_rgb", "d_r_diffuse",
              "d_r_specular", "d_r_distance", "d_r_acc", "d_r_normals", "d_r_normals_pred", "d_r_tint",
              "d_r_roughness", "d_r_distance_mean", "d_r_percentiles")                      # the fields of LevelOut
OUT_EXTRA_FIELDS = ("d_r_percentiles_soa", "d_r_rgb_fg")                                    # the fields of LevelOutExtra
RAY_FIELDS = ("origins", "directions", "viewdirs", "radii", "imageplane", "lossmult", "near", "far", "cam_idx")   # utils.Rays
RAY_FIELD_WIDTHS = (3, 3, 3, 1, 2, 1, 1, 1, 1)
VIS_PANEL_INPUTS = ("d_rgb", "d_acc", "d_distance_mean", "d_distance_median", "d_distance_p5", "d_distance_p95", "d_origins",
                    "d_directions")
VIS_PANEL_INPUTS_2 = ("d_roughness", "d_diffuse", "d_specular", "d_tint", "d_rgb_cc")
VIS_PANEL_OUTPUTS = ("d_color", "d_acc_out", "d_color_matte", "d_depth_mean", "d_depth_median", "d_depth_triplet", "d_coords_mod")
VIS_PANEL_OUTPUTS_2 = ("d_roughness_out", "d_diffuse_out", "d_diffuse_matte", "d_specular_out", "d_specular_matte", "d_tint_matte",
                       "d_color_corrected")


def build(force: bool = False) -> str:
    """Compile the library in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC] + (["-B"] if force else []) + ["librefnerf_hip.so"]
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    """Load the library; raises HipLibraryError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the Ref-NeRF hot path has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for header, prototypes in ((_abi.HEADER, _abi.prototypes), (DISTORTION_HEADER, _distortion_prototypes),
                                   (TSDF_HEADER, _tsdf_prototypes), (RAYCAST_HEADER, _raycast_prototypes)):
            for name, (restype, argtypes) in prototypes.items():
                try:
                    fn = getattr(L, name)
                except AttributeError:
                    raise HipLibraryError(f"{LIB_PATH} does not export {name}, which {header} declares: rebuild the library") from None
                fn.restype, fn.argtypes = restype, argtypes
        if L.refnerf_abi_version() != ABI_VERSION:      # the loaded library against the header
            raise HipLibraryError(f"librefnerf_hip.so ABI version mismatch: {LIB_PATH} is not built from {_abi.HEADER}")
        _lib = L
    return _lib


def check(rc: int):
    if rc == 0:
        return
    msg = lib().refnerf_last_error().decode()
    if rc == -1:
        raise ValueError(msg)      # same exception type the reference raises for bad arguments
    raise HipLibraryError(f"librefnerf_hip error {rc}: {msg}")


def require_device():
    """Fail loudly unless the current device is an MI355X-class (gfx950) GPU."""
    if not torch.cuda.is_available():
        raise HipLibraryError("no HIP device visible: the Ref-NeRF hot path needs a gfx950 GPU (no CPU fallback)")
    check(lib().refnerf_device_ok())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return C.c_void_p(t.data_ptr())


def _arg(t, what, *, dtype=torch.float32, shape=None, numel=None, device=None, optional=False, empty_null=False, exc=ValueError):
    """The checked tensor argument: the data pointer of a contiguous device tensor of `dtype` -- of exactly `shape`, of `numel`
    elements, on `device`, where those are given -- or `exc` saying what `what` is instead.  optional: None passes through
    (an absent argument); empty_null: an empty tensor gives None (the library launches nothing then).  (`ptr` is the trusting
    pointer, for tensors this module made itself.)"""
    if t is None and optional:
        return None
    if not torch.is_tensor(t):
        raise exc(f"{what}: a tensor is required, not {type(t).__name__}")
    bad = []
    if t.dtype != dtype:
        bad.append(f"is {t.dtype}, not {dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        bad.append(f"has shape {tuple(t.shape)}, not {tuple(shape)}")
    if numel is not None and t.numel() != numel:
        bad.append(f"has {t.numel()} elements, not {numel}")
    if not t.is_contiguous():
        bad.append("is not contiguous")
    if not t.is_cuda:
        bad.append("is not on a HIP device")
    elif device is not None and t.device != device:
        bad.append(f"is on {t.device}, not {device}")
    if bad:
        raise exc(f"{what} " + ", ".join(bad))
    return None if empty_null and not t.numel() else t.data_ptr()


def default_cfg(**kw) -> LevelCfg:
    c = LevelCfg()
    lib().refnerf_level_cfg_default(C.byref(c))
    for k, v in kw.items():
        if k == "render_srgb_mode" and isinstance(v, str):
            v = SRGB_MODES[v]
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def level_image(precision: int, training: bool = False, ipe_groups: int = 0) -> int:
    """Which weight image refnerf_level_forward / _forward_train / _backward expect as `d_packed` for a level configuration:
    inference levels the image of their precision mode (a general IPE basis: the f32 image), training levels the f32 image --
    except REFNERF_PREC_F16X2 on the built-in basis, whose training kernels stream their own image (REFNERF_IMAGE_F16X2_TRAIN)."""
    # one rule, inside the library (ABI v11: refnerf_level_image)
    cfg = LevelCfg()
    cfg.precision, cfg.training, cfg.ipe_groups = int(precision), int(bool(training)), int(ipe_groups)
    return int(lib().refnerf_level_image(C.byref(cfg)))


def packed_weights_bytes(precision=PREC_F32) -> int:
    return int(lib().refnerf_packed_weights_bytes(precision))


def pack_weights(params: torch.Tensor, packed: torch.Tensor = None, precision=PREC_F32, basis: torch.Tensor = None) -> torch.Tensor:
    """canonical fp32 blob (device) -> MFMA operand image (device).  `basis` ([3 G, 3] fp32 device tensor, G = 2..7: a general
    IPE basis, refnerf_pack_weights_basis): `params` is then the extended blob (NUM_PARAMS_EXT)."""
    require_device()
    groups = 0 if basis is None else basis.shape[0] // 3
    assert params.dtype == torch.float32 and params.numel() == (NUM_PARAMS_EXT if groups > 1 else NUM_PARAMS)
    nbytes = int(lib().refnerf_packed_weights_bytes_basis(precision, groups))
    if nbytes == 0:
        if groups > 1:
            raise ValueError("a general IPE basis (NerfMLP.basis_shape / basis_subdivisions other than 'octahedron' / 1) has at most 21 "
                             "directions and runs on the f32 operand image ('f32' and 'f16x2' modes); the plain bf16 / f16 images have "
                             "no direction groups")
        raise HipLibraryError("precision mode not built")
    if packed is None or packed.numel() * packed.element_size() != nbytes or packed.device != params.device:
        packed = torch.empty(nbytes // 4, dtype=torch.float32, device=params.device)
    if groups > 1:
        assert basis.dtype == torch.float32 and basis.is_contiguous() and basis.device == params.device and basis.shape == (3 * groups, 3)
        check(lib().refnerf_pack_weights_basis(ptr(params), ptr(basis), groups, ptr(packed), precision, stream_ptr()))
    else:
        check(lib().refnerf_pack_weights(ptr(params), ptr(packed), precision, stream_ptr()))
    return packed


def level_forward(packed, cfg: LevelCfg, rays: dict, sdist_in=None, weights_in=None, history=True, save_activations=False,
                  percentiles_soa=False):
    """One fused level.  rays: dict of device tensors (origins, directions,
    viewdirs [R,3]; radii, near, far [R] or [R,1]).  Returns dict of tensors.
    sdist_in = weights_in = None (with cfg.n_in == 1): the model's initial step function, knots cfg.s_near / cfg.s_far and
    weight 1 -- the library gets NULL pointers, reads nothing and resamples it in closed form (same bits as the tensors).
    save_activations (training forward): also keeps the layer inputs for
    level_backward in res["activations"] (a byte tensor the backward consumes).
    percentiles_soa: the float64 percentiles come as res["r_percentiles_soa"] [3, R] (each row one contiguous per-ray
    output) instead of res["r_percentiles"] [R, 3].  res["r_rgb_fg"] [R, 3] = sum_i w_i rgb_i (r_rgb before the background)."""
    require_device()
    if (sdist_in is None) != (weights_in is None):
        raise ValueError("level_forward: sdist_in and weights_in are given together, or both None (the initial step function)")
    dev = rays["origins"].device
    R = rays["origins"].shape[0]
    N = cfg.n_samples
    rs = RaysStruct()
    keep = []
    for name in ("origins", "directions", "viewdirs", "radii", "near", "far"):
        t = rays[name].to(torch.float32).contiguous()
        keep.append(t)
        setattr(rs, "d_" + name, t.data_ptr())
    f32 = dict(dtype=torch.float32, device=dev)
    res = {
        "sdist": torch.empty((R, N + 1), **f32), "bin_idx": torch.empty((R, N), dtype=torch.int32, device=dev),
        "weights": torch.empty((R, N), **f32),
        "r_rgb": torch.empty((R, 3), **f32), "r_rgb_fg": torch.empty((R, 3), **f32), "r_diffuse": torch.empty((R, 3), **f32),
        "r_specular": torch.empty((R, 3), **f32), "r_distance": torch.empty((R,), **f32),
        "r_acc": torch.empty((R,), **f32),
    }
    # history: True = every per-sample output (the reference's ray_history), False = none, or the names wanted
    want = ("rgb", "normals_pred", "grad_pred", "tint", "diffuse", "specular", "density", "roughness", "normals") \
        if history is True else (tuple(history) if history else ())
    for k in ("rgb", "normals_pred", "grad_pred", "tint", "diffuse", "specular"):
        if k in want:
            res[k] = torch.empty((R, N, 3), **f32)
    for k in ("density", "roughness"):
        if k in want:
            res[k] = torch.empty((R, N), **f32)
    if cfg.training and "normals" in want:
        res["normals"] = torch.empty((R, N, 3), **f32)
    if cfg.compute_extras:
        res["r_normals_pred"] = torch.empty((R, 3), **f32)
        res["r_tint"] = torch.empty((R, 3), **f32)
        res["r_roughness"] = torch.empty((R,), **f32)
        res["r_distance_mean"] = torch.empty((R,), **f32)
        if percentiles_soa:
            res["r_percentiles_soa"] = torch.empty((3, R), dtype=torch.float64, device=dev)
        else:
            res["r_percentiles"] = torch.empty((R, 3), dtype=torch.float64, device=dev)
        if cfg.training:
            res["r_normals"] = torch.empty((R, 3), **f32)
    out, extra = LevelOut(), LevelOutExtra()
    for k, t in res.items():
        setattr(extra if "d_" + k in OUT_EXTRA_FIELDS else out, "d_" + k, t.data_ptr())
    sd = None if sdist_in is None else sdist_in.to(torch.float32).contiguous()
    w = None if weights_in is None else weights_in.to(torch.float32).contiguous()
    if save_activations:
        act = torch.empty(lib().refnerf_activation_workspace_bytes_basis(R, N, cfg.ipe_groups), dtype=torch.uint8, device=dev)
        check(lib().refnerf_level_forward_train_ex(ptr(packed), C.byref(cfg), C.byref(rs), R, ptr(sd), ptr(w), C.byref(out),
                                                   C.byref(extra), ptr(act), act.numel(), stream_ptr()))
        res["activations"] = act
        # REFNERF_ACT_*: what this forward wrote (f32 rows | bf16 pair-rows | REFNERF_ACT_SQ), as the library says
        res["activations_format"] = int(lib().refnerf_activations_format(C.byref(cfg)))
    else:
        check(lib().refnerf_level_forward_ex(ptr(packed), C.byref(cfg), C.byref(rs), R, ptr(sd), ptr(w), C.byref(out), C.byref(extra),
                                             stream_ptr()))
    return res


def pixels_to_rays(pix_x, pix_y, pixtocams, camtoworlds, pixtocam_ndc=None, distortion: LensDistortion = None):
    """Device tensors in, device tensors out: (origins, directions, viewdirs [n,3], radii [n,1], imageplane [n,2]).
    `distortion` (a LensDistortion): undistort first (refnerf_pixels_to_rays_distorted)."""
    require_device()
    dev = pix_x.device
    n = pix_x.numel()
    px = pix_x.reshape(-1).to(torch.int32).contiguous()
    py = pix_y.reshape(-1).to(torch.int32).contiguous()
    p2c = pixtocams.to(torch.float32).contiguous()
    c2w = camtoworlds.to(torch.float32)[..., :3, :4].contiguous()
    ndc = None if pixtocam_ndc is None else pixtocam_ndc.to(torch.float32).contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    o, d, v = (torch.empty((n, 3), **f32) for _ in range(3))
    r = torch.empty((n, 1), **f32)
    ip = torch.empty((n, 2), **f32)
    args = (ptr(px), ptr(py), ptr(p2c), int(p2c.dim() > 2), ptr(c2w), int(c2w.dim() > 2), ptr(ndc) if ndc is not None else None, n,
            ptr(o), ptr(d), ptr(v), ptr(r), ptr(ip))
    if distortion is None:
        check(lib().refnerf_pixels_to_rays(*args, stream_ptr()))
    else:
        check(lib().refnerf_pixels_to_rays_distorted(*args, C.byref(distortion), stream_ptr()))
    return o, d, v, r, ip


def image_rays(projection, width, height, pixtocam, camtoworlds, frame, near, far, pixtocam_ndc=None,
               distortion: LensDistortion = None, first=0, count=None):
    """refnerf_image_rays: the nine utils.Rays fields (a dict, RAY_FIELDS order, each [count, width of the field]) of the
    flat pixel range [first, first + count) of frame `frame` of the device-resident path `camtoworlds` [F,3,4], in one
    launch.  `pixtocam` [3,3] device tensor (None for PROJ_SPHERICAL)."""
    require_device()
    c2w = camtoworlds
    assert c2w.dtype == torch.float32 and c2w.dim() == 3 and tuple(c2w.shape[1:]) == (3, 4), "camtoworlds: float32 [F,3,4]"
    assert pixtocam is None or (pixtocam.dtype == torch.float32 and tuple(pixtocam.shape) == (3, 3)), "pixtocam: float32 [3,3]"
    assert pixtocam_ndc is None or (pixtocam_ndc.dtype == torch.float32 and tuple(pixtocam_ndc.shape) == (3, 3))
    width, height, first = int(width), int(height), int(first)
    count = width * height - first if count is None else int(count)
    if not 0 <= count < 2 ** 31:
        raise ValueError(f"refnerf_image_rays: count {count} outside [0, 2^31)")
    dev = c2w.device
    out, res = ImageRaysOut(), {}
    for name, w in zip(RAY_FIELDS, RAY_FIELD_WIDTHS):
        res[name] = torch.empty((count, w), dtype=torch.int32 if name == "cam_idx" else torch.float32, device=dev)
        setattr(out, "d_" + name, res[name].data_ptr())
    check(lib().refnerf_image_rays(int(projection), width, height, ptr(pixtocam), ptr(c2w), c2w.shape[0], int(frame),
                                   ptr(pixtocam_ndc), None if distortion is None else C.byref(distortion), float(near),
                                   float(far), first, count, C.byref(out), stream_ptr()))
    return res


def prepare_images(src, op: int, factor: int = 1, return_alpha: bool = False):
    """refnerf_prepare_images: a device stack [n,H,W,C] or [n,H,W] (uint8 or float32; any storage offset) -> the float32
    stack the reference's loaders keep, in one launch: block mean over `factor`, then PREP_SCALE (/ 255), PREP_WHITE
    (/ 255 and white background; with `return_alpha` also the alpha plane [n,h,w]), PREP_NORMALS (* 2 / 255 - 1) or
    PREP_RAW (the mean alone).  The result has the source's rank; WHITE and NORMALS have 3 channels."""
    require_device()
    assert src.is_cuda and src.dtype in (torch.uint8, torch.float32) and src.dim() in (3, 4), "uint8 / float32 [n,H,W(,C)] on the device"
    src = src.contiguous()
    n, H, W = src.shape[:3]
    Cn = src.shape[3] if src.dim() == 4 else 1
    factor = int(factor)
    if factor < 1 or H % factor or W % factor:
        h = w = 1                                      # refused by the library, with its message
    else:
        h, w = H // factor, W // factor
    c_out = 3 if op in (PREP_WHITE, PREP_NORMALS) else Cn
    out = torch.empty((n, h, w, c_out) if src.dim() == 4 else (n, h, w), dtype=torch.float32, device=src.device)
    alpha = torch.empty((n, h, w), dtype=torch.float32, device=src.device) if return_alpha else None
    check(lib().refnerf_prepare_images(ptr(src), int(src.dtype == torch.float32), n, H, W, Cn, factor, int(op),
                                       C.c_void_p(out.data_ptr()), None if alpha is None else C.c_void_p(alpha.data_ptr()),
                                       stream_ptr()))
    return (out, alpha) if return_alpha else out


def train_batch(px0, py0, cam, patch_size, images, pixtocams, camtoworlds, near, far, pixtocam_ndc=None,
                distortion: LensDistortion = None, disps=None, normals=None, alphas=None):
    """refnerf_train_batch: one training batch in one launch.  `px0`, `py0` [P] patch origins, `cam` [P] or [1], all
    three int32 or all three int64 (as torch.randint draws them: no conversion launch); `images` float32 [n,H,W,3] and the optional stacks `disps` [n,H,W], `normals` [n,H,W,3], `alphas` [n,H,W];
    `pixtocams` float32 [3,3] | [n,3,3], `camtoworlds` float32 [n,3,4].  Returns (rays, gathered): two dicts of device
    tensors shaped [P, patch, patch, .] -- the nine RAY_FIELDS, and 'rgb' plus whichever of 'disps' / 'normals' /
    'alphas' were given (those three without a channel axis where the stack has none)."""
    require_device()
    a, rays, got = TrainBatchArgs(), {}, {}
    assert px0.dtype in (torch.int32, torch.int64), "px0, py0, cam: int32 or int64"
    a.d_px0, a.d_py0, a.d_cam = (_arg(t, what, dtype=px0.dtype, exc=AssertionError) for t, what in ((px0, "px0"), (py0, "py0"), (cam, "cam")))
    P, ps = px0.numel(), int(patch_size)
    assert py0.numel() == P and cam.numel() in (1, P), "py0: [P]; cam: [P] or [1]"
    a.d_images = _arg(images, "images", exc=AssertionError)
    assert images.dim() == 4 and images.shape[3] == 3, "images: float32 [n,H,W,3]"
    n, H, W = images.shape[:3]
    a.d_pixtocams, a.d_camtoworlds = _arg(pixtocams, "pixtocams", exc=AssertionError), _arg(camtoworlds, "camtoworlds", exc=AssertionError)
    assert tuple(camtoworlds.shape) == (n, 3, 4), "camtoworlds: float32 [n,3,4]"
    assert tuple(pixtocams.shape) in ((3, 3), (n, 3, 3)), "pixtocams: float32 [3,3] or [n,3,3]"
    a.d_pixtocam_ndc = _arg(pixtocam_ndc, "pixtocam_ndc", shape=(3, 3), optional=True, exc=AssertionError)
    if not 0 < P * ps * ps < 2 ** 31:
        raise ValueError(f"refnerf_train_batch: {P} patches of {ps}^2 rays outside (0, 2^31)")
    dev, shape = images.device, (P, ps, ps)
    a.index_is_int64, a.cam_per_patch, a.n_patches, a.patch_size = int(px0.dtype == torch.int64), int(cam.numel() == P), P, ps
    a.n_images, a.height, a.width = n, H, W
    a.pixtocam_per_camera, a.near, a.far = int(pixtocams.dim() == 3), float(near), float(far)
    if distortion is not None:
        a.distortion = C.pointer(distortion)
    for name, w in zip(RAY_FIELDS, RAY_FIELD_WIDTHS):
        rays[name] = torch.empty(shape + (w,), dtype=torch.int32 if name == "cam_idx" else torch.float32, device=dev)
        setattr(a.rays, "d_" + name, rays[name].data_ptr())
    got["rgb"] = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
    a.d_rgb = got["rgb"].data_ptr()
    for name, stack, tail in (("disps", disps, ()), ("normals", normals, (3,)), ("alphas", alphas, ())):
        if stack is None:
            continue
        setattr(a, "d_" + name, _arg(stack, name, shape=(n, H, W) + tail, exc=AssertionError))
        got[name] = torch.empty(shape + tail, dtype=torch.float32, device=dev)
        setattr(a, "d_out_" + name, got[name].data_ptr())
    check(lib().refnerf_train_batch(C.byref(a), stream_ptr()))
    return rays, got


def mlp_forward(packed, cfg: LevelCfg, means, covs, viewdirs):
    """MLP.__call__ on caller-supplied Gaussians: means [R,N,3], covs [R,N,3,3] or [R,N,3], viewdirs [R,3]
    (device tensors) -> dict of per-sample tensors (the reference's `ray_results`)."""
    require_device()
    R, N = means.shape[0], means.shape[1]
    f32 = dict(dtype=torch.float32, device=means.device)
    m = means.to(torch.float32).contiguous()
    c = covs.to(torch.float32).contiguous()
    v = viewdirs.to(torch.float32).contiguous()
    full = 1 if c.dim() == 4 else 0
    res = {k: torch.empty((R, N, 3), **f32) for k in ("rgb", "normals_pred", "grad_pred", "tint", "diffuse", "specular")}
    res["density"] = torch.empty((R, N), **f32)
    res["roughness"] = torch.empty((R, N), **f32)
    if cfg.training:
        res["normals"] = torch.empty((R, N, 3), **f32)
    out = LevelOut()
    for k, t in res.items():
        setattr(out, "d_" + k, t.data_ptr())
    check(lib().refnerf_mlp_forward(ptr(packed), C.byref(cfg), ptr(m), ptr(c), full, ptr(v), R, N, C.byref(out), stream_ptr()))
    return res


_workspace = {}


def backward_workspace(R: int, n_samples: int, device, ipe_groups: int = 0) -> torch.Tensor:
    """Cached byte workspace for refnerf_level_backward (grown on demand, one per device)."""
    need = lib().refnerf_backward_workspace_bytes_basis(R, n_samples, ipe_groups)
    ws = _workspace.get(device)
    if ws is None or ws.numel() < need:
        _workspace[device] = None
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _workspace[device] = ws
    return ws


def level_backward(packed, cfg: LevelCfg, rays: dict, saved: dict, g_r_rgb, g_weights, g_normals_pred,
                   param_grads: torch.Tensor, g_r_acc=None, g_r_distance=None, sample_seeds=None):
    """Backward of one level: accumulates dL/d(params) into `param_grads`
    (canonical blob).  saved: dict with sdist, density, rgb, weights and
    activations of the training forward (save_activations=True); g_*: upstream
    gradients (g_weights / g_normals_pred may be None); sample_seeds: optional dict of
    per-sample seeds on ray_history {density, rgb, diffuse, specular, tint, roughness}."""
    require_device()
    R = rays["origins"].shape[0]
    N = cfg.n_samples
    rs = RaysStruct()
    keep = []
    for name in ("origins", "directions", "viewdirs", "radii", "near", "far"):
        t = rays[name].to(torch.float32).contiguous()
        keep.append(t)
        setattr(rs, "d_" + name, t.data_ptr())
    sv = LevelSaved()
    for name in ("sdist", "density", "rgb", "weights"):
        t = saved[name].to(torch.float32).contiguous()
        keep.append(t)
        setattr(sv, "d_" + name, t.data_ptr())
    if saved.get("activations") is None:
        raise ValueError("level_backward needs the activations saved by level_forward(..., save_activations=True)")
    sv.d_activations = saved["activations"].data_ptr()
    sv.activations_format = int(saved.get("activations_format", 0))      # REFNERF_ACT_*: the forward's precision
    gr = LevelGrads()
    for name, t in (("d_g_r_rgb", g_r_rgb), ("d_g_weights", g_weights), ("d_g_normals_pred", g_normals_pred),
                    ("d_g_r_acc", g_r_acc), ("d_g_r_distance", g_r_distance)) + tuple(
                        ("d_g_" + k, v) for k, v in (sample_seeds or {}).items()):
        if t is not None:
            t = t.to(torch.float32).contiguous()
            keep.append(t)
            setattr(gr, name, t.data_ptr())
    assert param_grads.dtype == torch.float32 and param_grads.is_contiguous() and param_grads.numel() == (NUM_PARAMS_EXT if cfg.ipe_groups > 1 else NUM_PARAMS)
    ws = backward_workspace(R, N, param_grads.device, cfg.ipe_groups)
    check(lib().refnerf_level_backward(ptr(packed), C.byref(cfg), C.byref(rs), R, C.byref(sv), C.byref(gr),
                                       ptr(param_grads), ptr(ws), ws.numel(), stream_ptr()))
    return param_grads


def render_rays(cfg: LevelCfg, density, tdist, directions, far, rgb=None, diffuse=None, specular=None, normals=None,
                normals_pred=None, roughness=None, tint=None):
    """render.compute_alpha_weights + render.volumetric_rendering (render.py:132-254) on caller-supplied per-sample
    device tensors: density / roughness [R,N], tdist [R,N+1], directions [R,3], far [R], the others [R,N,3] or None.
    cfg.n_samples is taken from `density`.  Returns dict(weights, r_rgb, ..., r_percentiles)."""
    require_device()
    dev = density.device
    R, N = density.shape
    cfg.n_samples = N
    f32 = dict(dtype=torch.float32, device=dev)
    keep = []

    def prep(t, shape):
        if t is None:
            return None
        t = t.to(torch.float32).reshape(shape).contiguous()
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    args = [prep(density, (R, N)), prep(tdist, (R, N + 1)), prep(directions, (R, 3)), prep(far, (R,)),
            prep(rgb, (R, N, 3)), prep(diffuse, (R, N, 3)), prep(specular, (R, N, 3)), prep(normals, (R, N, 3)),
            prep(normals_pred, (R, N, 3)), prep(roughness, (R, N)), prep(tint, (R, N, 3))]
    res = {"weights": torch.empty((R, N), **f32), "r_rgb": torch.empty((R, 3), **f32),
           "r_diffuse": torch.empty((R, 3), **f32), "r_specular": torch.empty((R, 3), **f32),
           "r_distance": torch.empty((R,), **f32), "r_acc": torch.empty((R,), **f32)}
    if cfg.compute_extras:
        res.update({"r_normals_pred": torch.empty((R, 3), **f32), "r_tint": torch.empty((R, 3), **f32),
                    "r_roughness": torch.empty((R,), **f32), "r_distance_mean": torch.empty((R,), **f32),
                    "r_percentiles": torch.empty((R, 3), dtype=torch.float64, device=dev)})
        if normals is not None:
            res["r_normals"] = torch.empty((R, 3), **f32)
    out = LevelOut()
    for k, t in res.items():
        setattr(out, "d_" + k, t.data_ptr())
    check(lib().refnerf_render_rays(C.byref(cfg), R, *args, C.byref(out), stream_ptr()))
    return res


def losses_forward(r_rgb, gt_rgb, lossmult, weights, orientation_normals, normals, normals_pred, viewdirs):
    """refnerf_losses_forward: per-ray terms [R,3] of the three Ref-NeRF losses of one level (device tensors; the
    normals arguments may be None = term off)."""
    require_device()
    R, N = weights.shape
    terms = torch.empty((R, 3), dtype=torch.float32, device=weights.device)
    check(lib().refnerf_losses_forward(R, N, ptr(r_rgb), ptr(gt_rgb), ptr(lossmult), ptr(weights), ptr(orientation_normals),
                                       ptr(normals), ptr(normals_pred), ptr(viewdirs), ptr(terms), stream_ptr()))
    return terms


def losses_backward(r_rgb, gt_rgb, lossmult, weights, orientation_normals, orientation_on_pred, normals, normals_pred,
                    viewdirs, g_data, g_orientation, g_normal, upstream=None):
    """refnerf_losses_backward -> (g_r_rgb [R,3], g_weights [R,N], g_normals_pred [R,N,3])."""
    require_device()
    R, N = weights.shape
    f32 = dict(dtype=torch.float32, device=weights.device)
    g_rgb, g_w, g_np = torch.empty((R, 3), **f32), torch.empty((R, N), **f32), torch.empty((R, N, 3), **f32)
    check(lib().refnerf_losses_backward(R, N, ptr(r_rgb), ptr(gt_rgb), ptr(lossmult), ptr(weights), ptr(orientation_normals),
                                        int(orientation_on_pred), ptr(normals), ptr(normals_pred), ptr(viewdirs),
                                        float(g_data), float(g_orientation), float(g_normal), ptr(upstream),
                                        ptr(g_rgb), ptr(g_w), ptr(g_np), stream_ptr()))
    return g_rgb, g_w, g_np


_REG_CLEAN = (("distance", 1), ("diffuse", 3), ("specular", 3), ("normals", 3))   # per-ray tensors of a consistency term, widths


def regularisers_args(weights, acc, clean, noisy, rays, noisy_rays, n, a, thr_entropy, thr_consistency, types):
    """(RegularisersArgs, R, S) over contiguous float32 device tensors, every shape checked here (the kernels trust them):
    weights [R,S] or None; acc [R]; clean / noisy: dicts distance [R] / [n a] and diffuse, specular, normals [R,3] / [n a,3],
    a missing or None entry = term off; rays / noisy_rays: (origins, directions) [R,3] / [n a,3], needed by the distance
    term; types: the three REFNERF_CONSISTENCY_* (diffuse, specular, distance)."""
    dev = acc.device

    def p(t, shape, what):
        return _arg(t, "ray regularisers: " + what, shape=shape, device=dev, optional=True)
    R = acc.shape[0]
    S = weights.shape[1] if weights is not None else 1
    A = RegularisersArgs()
    A.R, A.S, A.n, A.a = int(R), int(S), int(n), int(a)
    A.thr_entropy, A.thr_consistency = float(thr_entropy), float(thr_consistency)
    A.diffuse_type, A.specular_type, A.distance_type = (int(t) for t in types)
    # (sizes the library refuses are left to its message; the shapes below are then checked against clamped ones)
    na = max(int(n), 0) * max(int(a), 0)
    A.d_weights, A.d_acc = p(weights, (R, S), "weights"), p(acc, (R,), "acc")
    for k, w in _REG_CLEAN:
        setattr(A, "d_" + k, p(clean.get(k), (R,) if w == 1 else (R, w), k))
        setattr(A, "d_n_" + k, p(noisy.get(k), (na,) if w == 1 else (na, w), "noisy " + k))
    if clean.get("distance") is not None:
        A.d_origins, A.d_directions = p(rays[0], (R, 3), "origins"), p(rays[1], (R, 3), "directions")
        A.d_n_origins, A.d_n_directions = p(noisy_rays[0], (na, 3), "noisy origins"), p(noisy_rays[1], (na, 3), "noisy directions")
    return A, R, S


def ray_regularisers_forward(A: RegularisersArgs, device):
    """refnerf_ray_regularisers_forward on the arguments of regularisers_args -> terms [R,8] (see include/refnerf_hip.h)."""
    require_device()
    terms = torch.empty((max(int(A.R), 1), 8), dtype=torch.float32, device=device)
    A.d_terms = terms.data_ptr()
    check(lib().refnerf_ray_regularisers_forward(C.byref(A), stream_ptr()))
    return terms


def ray_regularisers_backward(A: RegularisersArgs, sums, scales):
    """refnerf_ray_regularisers_backward: sums float[8] (the forward's column sums), scales float[6] (multiplier x warm-up x
    upstream of entropy, acc, diffuse, specular, normal, distance), both on the device.  Returns dict(weights, acc, distance,
    diffuse, specular, normals, n_distance, ...) of the gradients of the terms that are on (the others None)."""
    require_device()
    if not (sums.is_cuda and sums.dtype == torch.float32 and sums.is_contiguous() and sums.numel() == 8 and
            scales.is_cuda and scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == 6):
        raise ValueError("ray regularisers: sums / scales must be contiguous float32 device tensors of 8 / 6 elements")
    f32 = dict(dtype=torch.float32, device=sums.device)
    R, S, na = max(int(A.R), 1), max(int(A.S), 1), max(int(A.n), 0) * max(int(A.a), 0)
    out = {"weights": torch.empty((R, S), **f32) if A.d_weights else None, "acc": torch.empty((R,), **f32)}
    for k, w in _REG_CLEAN:
        on = bool(getattr(A, "d_" + k))
        out[k] = torch.empty((R,) if w == 1 else (R, w), **f32) if on else None
        out["n_" + k] = torch.empty((na,) if w == 1 else (na, w), **f32) if on else None
    for k, t in out.items():
        setattr(A, "d_g_" + k, None if t is None else t.data_ptr())
    A.d_sums, A.d_scales = sums.data_ptr(), scales.data_ptr()
    check(lib().refnerf_ray_regularisers_backward(C.byref(A), stream_ptr()))
    return out


def noisy_rays(rotations, distance, fields):
    """refnerf_noisy_rays: rotations [a,3,3], distance [n], fields: the nine utils.Rays tensors [n, w] in RAY_FIELDS order
    (contiguous float32 device tensors) -> the nine [a n, w] tensors of the perturbed rays, angle-major."""
    require_device()
    dev = distance.device
    a, n = int(rotations.shape[0]), int(distance.shape[0])
    A = NoisyRaysArgs()
    A.n, A.a = n, a

    A.d_rotations = _arg(rotations, "noisy_rays: rotations", shape=(a, 3, 3), device=dev)
    A.d_distance = _arg(distance, "noisy_rays: distance", shape=(n,), device=dev)
    outs = []
    for name, w, t in zip(RAY_FIELDS, RAY_FIELD_WIDTHS, fields):
        setattr(A, "d_" + name, _arg(t, "noisy_rays: " + name, shape=(n, w), device=dev))
        outs.append(torch.empty((a * n, w), dtype=torch.float32, device=dev))
        setattr(A, "d_out_" + name, outs[-1].data_ptr())
    check(lib().refnerf_noisy_rays(C.byref(A), stream_ptr()))
    return outs


def data_terms_args(rgb, gt_rgb, lossmult, penalty, charb_padding, distance_mean=None, disps=None, acc=None, alphas=None,
                    normals=None, normals_gt=None):
    """DataTermsArgs over contiguous float32 device tensors, every shape checked here (the kernels trust them): rgb, gt_rgb
    [R,3]; lossmult [R]; the disparity group distance_mean, disps [R]; the normal group acc, alphas [R] and normals,
    normals_gt [R,3].  penalty: a key of PENALTIES.  The caller keeps the tensors alive while the struct is in use."""
    if penalty not in PENALTIES:
        raise ValueError(f"data terms: unknown penalty {penalty!r}")
    dev, R = rgb.device, int(rgb.shape[0])
    A = DataTermsArgs()
    A.R, A.penalty, A.charb_padding = R, PENALTIES[penalty], float(charb_padding)
    for name, t, shape in (("rgb", rgb, (R, 3)), ("gt_rgb", gt_rgb, (R, 3)), ("lossmult", lossmult, (R,)),
                           ("distance_mean", distance_mean, (R,)), ("disps", disps, (R,)), ("acc", acc, (R,)),
                           ("alphas", alphas, (R,)), ("normals", normals, (R, 3)), ("normals_gt", normals_gt, (R, 3))):
        setattr(A, "d_" + name, _arg(t, "data terms: " + name, shape=shape, device=dev, optional=True))
    return A


def data_terms_forward(A: DataTermsArgs, device):
    """refnerf_data_terms_forward on the arguments of data_terms_args -> terms [R,5] (see include/refnerf_hip.h)."""
    require_device()
    terms = torch.empty((max(int(A.R), 1), 5), dtype=torch.float32, device=device)
    A.d_terms = terms.data_ptr()
    check(lib().refnerf_data_terms_forward(C.byref(A), stream_ptr()))
    return terms


def data_terms_backward(A: DataTermsArgs, upstream):
    """refnerf_data_terms_backward: upstream = one device float (multiplier / normaliser x grad_output) -> g_rgb [R,3]."""
    require_device()
    A.d_upstream = _arg(upstream, "data terms: upstream", numel=1)
    g_rgb = torch.empty((max(int(A.R), 1), 3), dtype=torch.float32, device=upstream.device)
    A.d_g_rgb = g_rgb.data_ptr()
    check(lib().refnerf_data_terms_backward(C.byref(A), stream_ptr()))
    return g_rgb


def depth_smoothness_args(distance, acc, rgb):
    """DepthSmoothnessArgs over contiguous float32 device tensors: distance, acc [P,S,S]; rgb [P,S,S,3] (shapes checked here)."""
    dev = distance.device
    if distance.ndim != 3 or distance.shape[1] != distance.shape[2]:
        raise ValueError(f"depth smoothness: distance must be [P,S,S], got {tuple(distance.shape)}")
    P, S = int(distance.shape[0]), int(distance.shape[1])
    A = DepthSmoothnessArgs()
    A.P, A.S = P, S
    A.d_distance = _arg(distance, "depth smoothness: distance", shape=(P, S, S), device=dev, optional=True)
    A.d_acc = _arg(acc, "depth smoothness: acc", shape=(P, S, S), device=dev, optional=True)
    A.d_rgb = _arg(rgb, "depth smoothness: rgb", shape=(P, S, S, 3), device=dev, optional=True)
    return A


def depth_smoothness_forward(A: DepthSmoothnessArgs, device):
    """refnerf_depth_smoothness_forward -> terms [P,2] (see include/refnerf_hip.h)."""
    require_device()
    terms = torch.empty((max(int(A.P), 1), 2), dtype=torch.float32, device=device)
    A.d_terms = terms.data_ptr()
    check(lib().refnerf_depth_smoothness_forward(C.byref(A), stream_ptr()))
    return terms


def depth_smoothness_backward(A: DepthSmoothnessArgs, upstream):
    """refnerf_depth_smoothness_backward: upstream = one device float -> g_distance [P,S,S]."""
    require_device()
    A.d_upstream = _arg(upstream, "depth smoothness: upstream", numel=1)
    P, S = max(int(A.P), 1), max(int(A.S), 1)
    g = torch.empty((P, S, S), dtype=torch.float32, device=upstream.device)
    A.d_g_distance = g.data_ptr()
    check(lib().refnerf_depth_smoothness_backward(C.byref(A), stream_ptr()))
    return g


def optim_state_bytes(max_tensors: int) -> int:
    return int(lib().refnerf_optim_state_bytes(int(max_tensors)))


def optim_state(max_tensors: int, device) -> torch.Tensor:
    """The optimiser's device state (refnerf_optim_state_bytes): [0:4] total_norm, [4:8] clip_coef as float32."""
    nbytes = int(lib().refnerf_optim_state_bytes(int(max_tensors)))
    if nbytes == 0:
        raise ValueError("optim_state: max_tensors must be positive")
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def optim_plan(n: int, seg_off, device):
    """refnerf_optim_plan for a tensor of n elements cut at `seg_off` (n_seg + 1 element offsets, 0 .. n): allocates and fills
    the tensor's workspace (a setup call; synchronises).  Returns (workspace, seg_stats [n_seg, 3], n_items)."""
    require_device()
    seg = [int(x) for x in seg_off]
    n_seg = len(seg) - 1
    nbytes = int(lib().refnerf_optim_workspace_bytes(int(n), n_seg)) if n_seg >= 1 else 0
    if nbytes == 0 or any(not -2 ** 31 <= x < 2 ** 31 for x in seg):
        raise ValueError(f"optim_plan: n = {n} with {n_seg} segments is not a valid layout (n in [1, 2^31), 1 <= n_seg <= n)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    stats = torch.zeros((n_seg, 3), dtype=torch.float32, device=device)
    n_items = C.c_int32(0)
    with torch.cuda.device(ws.device):
        check(lib().refnerf_optim_plan(int(n), (C.c_int32 * (n_seg + 1))(*seg), n_seg, ptr(ws), nbytes, C.byref(n_items), stream_ptr()))
    return ws, stats, int(n_items.value)


def optim_stats(grad, param, n_seg: int, n_items: int, grad_max_val: float, workspace, seg_stats, state, slot: int):
    """refnerf_optim_stats: the four partial sums per work item of one tensor, and its entry `slot` in the state's table."""
    if grad.numel() != param.numel():
        raise ValueError("optim_stats: gradient and parameter differ in size")
    g, p, stats = (_arg(t, "optim_stats: " + what, optional=True) for t, what in ((grad, "grad"), (param, "param"), (seg_stats, "seg_stats")))
    check(lib().refnerf_optim_stats(g, p, param.numel(), n_seg, n_items, float(grad_max_val), ptr(workspace), workspace.numel(), stats,
                                    ptr(state), state.numel(), int(slot), stream_ptr()))


def optim_finalize(state, n_tensors: int, grad_max_norm: float):
    """refnerf_optim_finalize: per-segment statistics of the step's tensors, total_norm and clip_coef into the state."""
    check(lib().refnerf_optim_finalize(ptr(state), state.numel(), int(n_tensors), float(grad_max_norm), stream_ptr()))


def optim_adam_step(param, grad, exp_avg, exp_avg_sq, cfg: AdamCfg, state):
    """refnerf_optim_adam_step: g = clip_coef * clamp(g), then torch's Adam update in place (cfg.no_step: the clip alone)."""
    n = grad.numel()
    for t in (param, exp_avg, exp_avg_sq):
        if t is not None and t.numel() != n:
            raise ValueError("optim_adam_step: tensors differ in size")
    ptrs = [_arg(t, "optim_adam_step: " + what, optional=True)
            for t, what in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"))]
    check(lib().refnerf_optim_adam_step(*ptrs, n, C.byref(cfg), ptr(state), stream_ptr()))


def max_dilate_weights(t, w, dilation, lo, hi):
    """refnerf_max_dilate_weights: stepfun.max_dilate_weights(t, w, dilation, domain=(lo, hi), renormalize=True) and the
    [..., 1:-1] of Model.__call__ in one launch.  t [R, M+1], w [R, M] (contiguous float32 device tensors, t nondecreasing)
    -> (sdist [R, 3M-1], weights [R, 3M-2])."""
    require_device()
    if t.dim() != 2 or w.dim() != 2:
        raise ValueError("max_dilate_weights: t [R, M+1] and w [R, M]")
    R, M = w.shape
    sd = torch.empty((R, max(3 * M - 1, 0)), dtype=torch.float32, device=t.device)
    wd = torch.empty((R, max(3 * M - 2, 0)), dtype=torch.float32, device=t.device)
    check(lib().refnerf_max_dilate_weights(_arg(t, "max_dilate_weights: t", shape=(R, M + 1), empty_null=True),
                                           _arg(w, "max_dilate_weights: w", shape=(R, M), empty_null=True),
                                           R, M, float(dilation), float(lo), float(hi), ptr(sd) if sd.numel() else None,
                                           ptr(wd) if wd.numel() else None, stream_ptr()))
    return sd, wd


def _interlevel_args(t, w, t_env, w_env):
    if w.dim() != 2 or w_env.dim() != 2 or w.shape[0] != w_env.shape[0]:
        raise ValueError("interlevel loss: w [R, N] and w_env [R, Np]")
    (R, N), Np = w.shape, w_env.shape[1]
    shapes = (("t", t, (R, N + 1)), ("w", w, (R, N)), ("t_env", t_env, (R, Np + 1)), ("w_env", w_env, (R, Np)))
    return tuple(_arg(x, "interlevel loss: " + what, shape=shape, empty_null=True) for what, x, shape in shapes) + (R, N, Np)


def interlevel_forward(t, w, t_env, w_env):
    """refnerf_interlevel_forward: per-ray sums [R] of stepfun.lossfun_outer(t, w, t_env, w_env) (t [R, N+1], w [R, N]: the
    final level; t_env [R, Np+1], w_env [R, Np]: one proposal level; contiguous float32 device tensors)."""
    require_device()
    args = _interlevel_args(t, w, t_env, w_env)
    ray_loss = torch.empty((args[4],), dtype=torch.float32, device=w.device)
    check(lib().refnerf_interlevel_forward(*args, ptr(ray_loss) if ray_loss.numel() else None, stream_ptr()))
    return ray_loss


def interlevel_backward(t, w, t_env, w_env, upstream):
    """refnerf_interlevel_backward -> g_w_env [R, Np]; upstream: a one-element float32 device tensor, the gradient of the
    total w.r.t. the sum of interlevel_forward's per-ray sums."""
    require_device()
    args = _interlevel_args(t, w, t_env, w_env)
    g = torch.empty((args[4], args[6]), dtype=torch.float32, device=w.device)
    check(lib().refnerf_interlevel_backward(*args, _arg(upstream.reshape(1), "interlevel loss: upstream", shape=(1,), empty_null=True),
                                            ptr(g) if g.numel() else None, stream_ptr()))
    return g


def _distortion_args(t, w):
    if not torch.is_tensor(w) or w.dim() != 2:
        raise ValueError("distortion loss: t [R, N+1] and w [R, N]")
    R, N = w.shape
    return (_arg(t, "distortion loss: t", shape=(R, N + 1), empty_null=True), _arg(w, "distortion loss: w", shape=(R, N), empty_null=True)), R, N


def distortion_forward(t, w):
    """refnerf_distortion_forward: stepfun.lossfun_distortion(t, w) per ray, [R] (t [R, N+1] nondecreasing, w [R, N]; contiguous
    float32 device tensors, 1 <= N <= 512)."""
    require_device()
    rows, R, N = _distortion_args(t, w)
    ray_loss = torch.empty((R,), dtype=torch.float32, device=w.device)
    check(lib().refnerf_distortion_forward(*rows, R, N, ptr(ray_loss) if ray_loss.numel() else None, stream_ptr()))
    return ray_loss


def distortion_backward(t, w, g):
    """refnerf_distortion_backward -> grad_w [R, N] = g[0] * d lossfun_distortion / d w; g: a one-element float32 device
    tensor, the gradient of the total w.r.t. the sum of distortion_forward's per-ray values."""
    require_device()
    rows, R, N = _distortion_args(t, w)
    if not torch.is_tensor(g) or g.numel() != 1:
        raise ValueError("distortion loss: g is a one-element tensor")
    grad_w = torch.empty((R, N), dtype=torch.float32, device=w.device)
    check(lib().refnerf_distortion_backward(*rows, _arg(g.reshape(1), "distortion loss: g", shape=(1,)), R, N,
                                            ptr(grad_w) if grad_w.numel() else None, stream_ptr()))
    return grad_w


def tsdf_grid(dims, origin, voxel_size, trunc) -> TsdfGrid:
    """The host struct of a voxel grid: dims (nx, ny, nz), origin the centre of voxel (0, 0, 0)."""
    g = TsdfGrid()
    g.nx, g.ny, g.nz = (int(d) for d in dims)
    g.origin[0], g.origin[1], g.origin[2] = (float(o) for o in origin)
    g.voxel_size, g.trunc = float(voxel_size), float(trunc)
    return g


def tsdf_integrate(grid: TsdfGrid, tsdf, weight, rgb, pixtocam, camtoworlds, frame, depth, acc=None, acc_min=0.0, view_rgb=None,
                   view_weight=1.0, z_min=0.0):
    """refnerf_tsdf_integrate: fuses the view depth [H,W] (acc [H,W], view_rgb [H,W,3] optional) of pose `frame` of
    camtoworlds [F,3,4] into tsdf / weight [nz,ny,nx] and rgb [nz,ny,nx,3] (or None), in place.  All contiguous float32
    device tensors, every shape checked here."""
    require_device()
    dev, vox = tsdf.device if torch.is_tensor(tsdf) else None, (grid.nz, grid.ny, grid.nx)
    if not torch.is_tensor(depth) or depth.dim() != 2:
        raise ValueError("tsdf_integrate: depth [H, W]")
    H, W = depth.shape
    if not torch.is_tensor(camtoworlds) or camtoworlds.dim() != 3:
        raise ValueError("tsdf_integrate: camtoworlds [F, 3, 4]")
    what = "tsdf_integrate: "
    check(lib().refnerf_tsdf_integrate(
        C.byref(grid), _arg(tsdf, what + "tsdf", shape=vox), _arg(weight, what + "weight", shape=vox, device=dev),
        _arg(rgb, what + "rgb", shape=vox + (3,), device=dev, optional=True), _arg(pixtocam, what + "pixtocam", shape=(3, 3), device=dev),
        _arg(camtoworlds, what + "camtoworlds", shape=(camtoworlds.shape[0], 3, 4), device=dev), camtoworlds.shape[0], int(frame),
        W, H, _arg(depth, what + "depth", device=dev), _arg(acc, what + "acc", shape=(H, W), device=dev, optional=True), float(acc_min),
        _arg(view_rgb, what + "view_rgb", shape=(H, W, 3), device=dev, optional=True), float(view_weight), float(z_min), stream_ptr()))


def tsdf_mesh_workspace_bytes(grid: TsdfGrid) -> int:
    return int(lib().refnerf_tsdf_mesh_workspace_bytes(C.byref(grid)))


def tsdf_mesh_count(grid: TsdfGrid, tsdf, weight, iso=0.0, min_weight=1.0, workspace=None):
    """refnerf_tsdf_mesh_count -> (workspace, counts): the byte workspace refnerf_tsdf_mesh_emit reads and the device
    int64[2] {n_vertices, n_triangles}."""
    require_device()
    vox = (grid.nz, grid.ny, grid.nx)
    nbytes = tsdf_mesh_workspace_bytes(grid)
    t = _arg(tsdf, "tsdf_mesh_count: tsdf", shape=vox)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=tsdf.device)
    counts = torch.empty(2, dtype=torch.int64, device=tsdf.device)
    check(lib().refnerf_tsdf_mesh_count(C.byref(grid), t, _arg(weight, "tsdf_mesh_count: weight", shape=vox, device=tsdf.device),
                                        float(iso), float(min_weight), _arg(workspace, "tsdf_mesh_count: workspace", dtype=torch.uint8),
                                        workspace.numel(), ptr(counts), stream_ptr()))
    return workspace, counts


def tsdf_mesh_emit(grid: TsdfGrid, tsdf, rgb, iso, workspace, n_vertices: int, n_triangles: int):
    """refnerf_tsdf_mesh_emit -> (vertices [V,3] float32, vertex_rgb [V,3] float32 or None without `rgb`, triangles [T,3]
    int32); the counts are the host values of tsdf_mesh_count's."""
    require_device()
    vox, dev = (grid.nz, grid.ny, grid.nx), tsdf.device if torch.is_tensor(tsdf) else None
    V, T = int(n_vertices), int(n_triangles)
    t = _arg(tsdf, "tsdf_mesh_emit: tsdf", shape=vox)
    vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
    colors = None if rgb is None else torch.empty((V, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
    check(lib().refnerf_tsdf_mesh_emit(C.byref(grid), t, _arg(rgb, "tsdf_mesh_emit: rgb", shape=vox + (3,), device=dev, optional=True),
                                       float(iso), _arg(workspace, "tsdf_mesh_emit: workspace", dtype=torch.uint8, device=dev),
                                       workspace.numel(), V, T, ptr(vertices) if V else None,
                                       ptr(colors) if colors is not None and V else None, ptr(triangles) if T else None, stream_ptr()))
    return vertices, colors, triangles


def tsdf_raycast(grid: TsdfGrid, tsdf, weight, rgb, pixtocam, camtoworlds, frame, width, height, iso=0.0, min_weight=1.0, step=0.5,
                 refine=4, t_near=0.0, t_far=float("inf")):
    """refnerf_tsdf_raycast -> (depth [H,W], normals [H,W,3], view_rgb [H,W,3] or None without `rgb`, acc [H,W]): the view of
    pose `frame` of camtoworlds [F,3,4] through pixtocam [3,3] of the volume tsdf / weight [nz,ny,nx], rgb [nz,ny,nx,3] (or
    None).  All contiguous float32 device tensors, every shape checked here; `step` in voxels."""
    require_device()
    dev, vox = tsdf.device if torch.is_tensor(tsdf) else None, (grid.nz, grid.ny, grid.nx)
    if not torch.is_tensor(camtoworlds) or camtoworlds.dim() != 3:
        raise ValueError("tsdf_raycast: camtoworlds [F, 3, 4]")
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise ValueError("tsdf_raycast: width and height must be positive")
    what = "tsdf_raycast: "
    t = _arg(tsdf, what + "tsdf", shape=vox)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    normals = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    view_rgb = None if rgb is None else torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    acc = torch.empty((H, W), dtype=torch.float32, device=dev)
    check(lib().refnerf_tsdf_raycast(
        C.byref(grid), t, _arg(weight, what + "weight", shape=vox, device=dev),
        _arg(rgb, what + "rgb", shape=vox + (3,), device=dev, optional=True), _arg(pixtocam, what + "pixtocam", shape=(3, 3), device=dev),
        _arg(camtoworlds, what + "camtoworlds", shape=(camtoworlds.shape[0], 3, 4), device=dev), camtoworlds.shape[0], int(frame),
        W, H, float(iso), float(min_weight), float(step), int(refine), float(t_near), float(t_far), ptr(depth), ptr(normals),
        ptr(view_rgb), ptr(acc), stream_ptr()))
    return depth, normals, view_rgb, acc


def sample_intervals(t, logits, n, smin=0.0, smax=1.0):
    require_device()
    R, M = logits.shape
    sd = torch.empty((R, n + 1), dtype=torch.float32, device=t.device)
    bi = torch.empty((R, n), dtype=torch.int32, device=t.device)
    check(lib().refnerf_sample_intervals(ptr(t.contiguous()), ptr(logits.contiguous()), R, M, n, smin, smax,
                                         ptr(sd), ptr(bi), stream_ptr()))
    return sd, bi


def integrated_pos_enc(lmean, lvar):
    require_device()
    n = lmean.numel() // 3
    out = torch.empty(lmean.shape[:-1] + (96,), dtype=torch.float32, device=lmean.device)
    check(lib().refnerf_integrated_pos_enc(ptr(lmean.contiguous()), ptr(lvar.contiguous()), n, ptr(out), stream_ptr()))
    return out


def integrated_dir_enc(xyz, kappa_inv):
    require_device()
    n = xyz.numel() // 3
    out = torch.empty(xyz.shape[:-1] + (72,), dtype=torch.float32, device=xyz.device)
    k = kappa_inv.to(torch.float32).expand(xyz.shape[:-1] + (1,)).contiguous()
    check(lib().refnerf_integrated_dir_enc(ptr(xyz.contiguous()), ptr(k), n, ptr(out), stream_ptr()))
    return out


def _image64(t, what):
    """(pointer, row pitch in elements) of a float64 device image [H, W, C]; a view whose pixels are dense and whose rows are
    a fixed distance apart (a border crop) is passed as it is, anything else is made contiguous first."""
    if not (t.is_cuda and t.dtype == torch.float64 and t.dim() == 3):
        raise ValueError(f"{what}: a float64 device image [H, W, C] is required")
    H, W, Cn = t.shape
    if not (t.stride(2) == 1 and t.stride(1) == Cn and (H == 1 or t.stride(0) >= W * Cn)):
        t = t.contiguous()
    return t, C.c_void_p(t.data_ptr()), int(t.stride(0)) if H > 1 else W * Cn


def image_workspace(H: int, W: int, Cn: int, device) -> torch.Tensor:
    """The workspace of the image entries at one shape (refnerf_image_workspace_bytes)."""
    nbytes = int(lib().refnerf_image_workspace_bytes(int(H), int(W), int(Cn)))
    if nbytes == 0:
        raise ValueError(f"image_workspace: [{H}, {W}, {Cn}] is not a valid image shape (C in 1..4, H * W * C < 2^31)")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def _image_pair(a, b, what):
    if a.shape != b.shape:
        raise ValueError(f"{what}: the images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    a, pa, sa = _image64(a, what)
    b, pb, sb = _image64(b, what)
    return (a, b), (pa, sa, pb, sb) + tuple(int(s) for s in a.shape)


def image_mse(a, b, quantize_a=False, workspace=None):
    """refnerf_image_mse: a float64 device tensor [2] = (mean (q(a) - b)^2, its PSNR)."""
    keep, args = _image_pair(a, b, "image_mse")
    ws = image_workspace(*a.shape, a.device) if workspace is None else workspace
    out = torch.empty(2, dtype=torch.float64, device=a.device)
    check(lib().refnerf_image_mse(*args, int(bool(quantize_a)), ptr(out), ptr(ws), ws.numel() * 8, stream_ptr()))
    return out


def image_ssim(a, b, quantize_a=False, return_map=False, workspace=None):
    """refnerf_image_ssim: the mean SSIM as a float64 device scalar (and the [H-10, W-10, C] map when asked for)."""
    keep, args = _image_pair(a, b, "image_ssim")
    H, W, Cn = a.shape
    ws = image_workspace(H, W, Cn, a.device) if workspace is None else workspace
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    smap = torch.empty((max(H - 10, 0), max(W - 10, 0), Cn), dtype=torch.float64, device=a.device) if return_map else None
    check(lib().refnerf_image_ssim(*args, int(bool(quantize_a)), ptr(out), ptr(smap), ptr(ws), ws.numel() * 8, stream_ptr()))
    return (out[0], smap) if return_map else out[0]


def color_correct(img, ref, num_iters=5, eps=0.5 / 255, return_warp=False, workspace=None):
    """refnerf_color_correct: the corrected image, dense float64 [H, W, 3] (and the last [10, 3] warp when asked for)."""
    keep, args = _image_pair(img, ref, "color_correct")
    ws = image_workspace(*img.shape, img.device) if workspace is None else workspace
    out = torch.empty(tuple(img.shape), dtype=torch.float64, device=img.device)
    warp = torch.zeros((10, 3), dtype=torch.float64, device=img.device) if return_warp else None
    check(lib().refnerf_color_correct(*args, int(num_iters), float(eps), ptr(out), ptr(warp), ptr(ws), ws.numel() * 8, stream_ptr()))
    return (out, warp) if return_warp else out


def weighted_mae(weights, normals, normals_gt, workspace=None):
    """refnerf_weighted_mae: the weighted mean angular error in degrees as a float64 device scalar."""
    n = weights.numel()
    for t, m, what in ((weights, n, "weights"), (normals, 3 * n, "normals"), (normals_gt, 3 * n, "normals_gt")):
        if not (t.is_cuda and t.dtype == torch.float64 and t.numel() == m):
            raise ValueError(f"weighted_mae: {what} must be a float64 device tensor of {m} elements")
    w, a, b = weights.contiguous(), normals.contiguous(), normals_gt.contiguous()
    ws = image_workspace(1, max(n, 1), 1, w.device) if workspace is None else workspace
    out = torch.empty(1, dtype=torch.float64, device=w.device)
    check(lib().refnerf_weighted_mae(ptr(w), ptr(a), ptr(b), n, ptr(out), ptr(ws), ws.numel() * 8, stream_ptr()))
    return out[0]


# ---- validation visualisations (refnerf_vis_*): raw bindings; refnerf_pl_amd.vis is the interface ----
VIS_LAUNCHES = 0      # kernel launches of the vis entries since import (scripts/time_vis.py reads the difference)


def _vis_f64(t, what):
    """1 for a float64, 0 for a float32 dense device tensor"""
    if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.float32, torch.float64)):
        raise ValueError(f"{what}: a contiguous float32 or float64 device tensor is required")
    return int(t.dtype == torch.float64)


def vis_percentile_workspace(n: int, device) -> torch.Tensor:
    nbytes = int(lib().refnerf_vis_percentile_workspace_bytes(int(n)))
    if nbytes == 0:
        raise ValueError(f"weighted_percentile: {n} values (at least two are required, fewer than 2^31)")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def vis_weighted_percentile(values, weights, order, ps, target_f32=True, nan_mask=None, workspace=None):
    """refnerf_vis_weighted_percentile: a float64 device tensor [len(ps)].  `values` flat, `order` its stable ascending
    order (int64), `weights` flat or None (all ones), `nan_mask` of the weights' shape and type or None."""
    global VIS_LAUNCHES
    n = values.numel()
    ws = vis_percentile_workspace(n, values.device) if workspace is None else workspace
    if not (order.is_cuda and order.dtype == torch.int64 and order.is_contiguous() and order.numel() == n):
        raise ValueError("weighted_percentile: the order must be a contiguous int64 device tensor of the values' length")
    wf = 0 if weights is None else _vis_f64(weights, "weighted_percentile weights")
    if nan_mask is not None and (weights is None or nan_mask.dtype != weights.dtype or nan_mask.numel() != weights.numel()
                                 or _vis_f64(nan_mask, "weighted_percentile nan_mask") != wf):
        raise ValueError("weighted_percentile: the NaN mask must have the weights' type and size")
    ps = [float(p) for p in ps]
    out = torch.empty(len(ps), dtype=torch.float64, device=values.device)
    check(lib().refnerf_vis_weighted_percentile(ptr(values), _vis_f64(values, "weighted_percentile values"), ptr(weights), wf,
                                                0 if weights is None else weights.numel(), ptr(nan_mask), ptr(order), n,
                                                (C.c_double * len(ps))(*ps), len(ps), int(bool(target_f32)), ptr(out), ptr(ws),
                                                ws.numel() * 8, stream_ptr()))
    VIS_LAUNCHES += 5
    return out


def vis_panels(H, W, dtype, linear_to_srgb, table, inputs, outputs, lohi=(None, None, None), normals=(), roughness_channels=1):
    """refnerf_vis_panels.  `inputs` maps the names of VIS_PANEL_INPUTS* (without 'd_') to dense device tensors of `dtype`,
    `outputs` names the panels wanted (VIS_PANEL_OUTPUTS* without 'd_'); `normals` is a list of up to four normal maps.
    Returns {name: tensor} plus 'normals_out': [tensors]."""
    global VIS_LAUNCHES
    a = VisPanelsArgs()
    a.H, a.W, a.f64, a.linear_to_srgb, a.roughness_channels = int(H), int(W), int(dtype == torch.float64), int(bool(linear_to_srgb)), int(roughness_channels)
    dev = None
    for name, t in inputs.items():
        if "d_" + name not in VIS_PANEL_INPUTS + VIS_PANEL_INPUTS_2:
            raise KeyError(name)
        if t.dtype != dtype or _vis_f64(t, "vis_panels " + name) != a.f64:
            raise ValueError(f"vis_panels: {name} is not of the panels' type")
        width = 1 if name in ("acc", "distance_mean", "distance_median", "distance_p5", "distance_p95") else (
            roughness_channels if name == "roughness" else 3)
        if t.numel() != H * W * width:
            raise ValueError(f"vis_panels: {name} has {t.numel()} elements, not {H} x {W} x {width}")
        setattr(a, "d_" + name, t.data_ptr())
        dev = t.device
    if len(normals) > VIS_MAX_NORMALS:
        raise ValueError("vis_panels: at most four normal maps per call")
    if table is not None:
        if not (table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2 and table.shape[1] == 3):
            raise ValueError("vis_panels: the colour table must be a contiguous float32 device tensor [N, 3]")
        a.d_table, a.table_n = table.data_ptr(), int(table.shape[0])
    for field, t in zip(("d_lohi_mean", "d_lohi_median", "d_lohi_triplet"), lohi):
        if t is not None:
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= 2):
                raise ValueError("vis_panels: the percentile pairs are float64 device tensors [2]")
            setattr(a, field, t.data_ptr())
    out = {}
    widths = {"acc_out": None, "roughness_out": roughness_channels}
    for name in outputs:
        if "d_" + name not in VIS_PANEL_OUTPUTS + VIS_PANEL_OUTPUTS_2:
            raise KeyError(name)
        w = widths.get(name, 3)
        out[name] = torch.empty((H, W) if w is None else (H, W, w), dtype=dtype, device=dev)
        setattr(a, "d_" + name, out[name].data_ptr())
    out["normals_out"] = []
    for k, t in enumerate(normals):
        if t.dtype != dtype or _vis_f64(t, "vis_panels normals") != a.f64 or t.numel() != H * W * 3:
            raise ValueError("vis_panels: a normal map is not [H, W, 3] of the panels' type")
        o = torch.empty((H, W, 3), dtype=dtype, device=dev)
        a.d_normals[k], a.d_normals_out[k] = t.data_ptr(), o.data_ptr()
        out["normals_out"].append(o)
    check(lib().refnerf_vis_panels(C.byref(a), stream_ptr()))
    VIS_LAUNCHES += 1
    return out


def vis_cmap(values, H, W, channels, out_dtype, curve="none", normalise=False, d_lo=None, lo_bias=0.0, d_hi=None, hi_bias=0.0,
             table=None, acc=None, alpha=None, null_color=(1.0, 0.0, 0.0)):
    """refnerf_vis_cmap: [H, W, 3 with a table, else channels] of `out_dtype` (float32 or float64)."""
    global VIS_LAUNCHES
    a = VisCmapArgs()
    a.H, a.W, a.channels, a.f64 = int(H), int(W), int(channels), _vis_f64(values, "vis_cmap values")
    a.out_f64, a.curve, a.normalise = int(out_dtype == torch.float64), VIS_CURVES[curve], int(bool(normalise))
    a.lo_bias, a.hi_bias = float(lo_bias), float(hi_bias)
    a.null_color[0], a.null_color[1], a.null_color[2] = (float(c) for c in null_color)
    if values.numel() != H * W * channels:
        raise ValueError("vis_cmap: the values are not [H, W, channels]")
    a.d_values = values.data_ptr()
    if acc is not None:
        if acc.dtype != values.dtype or _vis_f64(acc, "vis_cmap acc") != a.f64 or acc.numel() != H * W:
            raise ValueError("vis_cmap: acc must be [H, W] of the values' type")
        a.d_acc = acc.data_ptr()
    for field, t, m in (("d_lo", d_lo, 1), ("d_hi", d_hi, 1), ("d_alpha", alpha, H * W)):
        if t is not None:
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= m):
                raise ValueError(f"vis_cmap: {field} must be a float64 device tensor")
            setattr(a, field, t.data_ptr())
    if table is not None:
        if not (table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2 and table.shape[1] == 3):
            raise ValueError("vis_cmap: the colour table must be a contiguous float32 device tensor [N, 3]")
        a.d_table, a.table_n = table.data_ptr(), int(table.shape[0])
    out = torch.empty((H, W, 3 if table is not None else channels), dtype=out_dtype, device=values.device)
    a.d_out = out.data_ptr()
    check(lib().refnerf_vis_cmap(C.byref(a), stream_ptr()))
    VIS_LAUNCHES += 1
    return out


def vis_resample_rays(sdist, values, weights, edges, out_values, out_alpha, level, accumulate=False, value_op="none"):
    """refnerf_vis_resample_rays for one level: sdist [n, N+1], values [n, N, C], weights [n, N] or None, edges float64
    [resolution + 1]; writes out_values[:, level] of [n, L, resolution, C] and out_alpha[:, level] of [n, L, resolution]."""
    global VIS_LAUNCHES
    f64 = _vis_f64(sdist, "vis_resample_rays sdist")
    n, N, Cn = values.shape
    if _vis_f64(values, "vis_resample_rays values") != f64 or (weights is not None and _vis_f64(weights, "vis_resample_rays weights") != f64):
        raise ValueError("vis_resample_rays: sdist, values and weights must be of one type")
    if tuple(sdist.shape) != (n, N + 1) or (weights is not None and tuple(weights.shape) != (n, N)):
        raise ValueError("vis_resample_rays: sdist must be [n, N + 1] and weights [n, N] for values [n, N, C]")
    res = edges.numel() - 1
    L = out_values.shape[1]
    if not (edges.is_cuda and edges.dtype == torch.float64 and edges.is_contiguous() and tuple(out_values.shape) == (n, L, res, Cn)
            and tuple(out_alpha.shape) == (n, L, res) and out_values.dtype == torch.float64 and out_alpha.dtype == torch.float64
            and out_values.is_contiguous() and out_alpha.is_contiguous() and 0 <= level < L):
        raise ValueError("vis_resample_rays: edges [resolution + 1] and the outputs [n, L, resolution(, C)] must be dense float64")
    check(lib().refnerf_vis_resample_rays(ptr(sdist), ptr(values), ptr(weights), f64, n, N, Cn, ptr(edges), res, int(bool(accumulate)),
                                          VIS_OPS[value_op], L, C.c_void_p(out_values.data_ptr() + level * res * Cn * 8),
                                          C.c_void_p(out_alpha.data_ptr() + level * res * 8), stream_ptr()))
    VIS_LAUNCHES += 1


def vis_ray_panel(lines_values, lines_alpha, rep, bg_color, alpha_max=None):
    """refnerf_vis_ray_panel: (panel [rows, resolution, C], alpha [rows, resolution]) in float64 from the lines
    [n, L, resolution, C] / [n, L, resolution]; rep = 0 keeps the lines of the first n - 1 rays untiled."""
    global VIS_LAUNCHES
    n, L, res, Cn = lines_values.shape
    rows = n * (L * rep + 1) - 1 if rep > 0 else (n - 1) * L
    vis = torch.empty((rows, res, Cn), dtype=torch.float64, device=lines_values.device)
    alpha = torch.empty((rows, res), dtype=torch.float64, device=lines_values.device)
    if alpha_max is not None and not (alpha_max.is_cuda and alpha_max.dtype == torch.float64 and alpha_max.numel() == 1):
        raise ValueError("vis_ray_panel: alpha_max must be a float64 device scalar")
    check(lib().refnerf_vis_ray_panel(ptr(lines_values), ptr(lines_alpha), n, L, res, Cn, int(rep), float(bg_color), ptr(alpha_max),
                                      ptr(vis), ptr(alpha), stream_ptr()))
    VIS_LAUNCHES += 1
    return vis, alpha


def set_timing(enable: bool):
    lib().refnerf_set_timing(int(enable))


def get_timing(family: int = TIMER_FORWARD):       # REFNERF_TIMER_*
    """(total ms, launches) of the kernels of one family launched since set_timing(True)."""
    ms, n = C.c_double(0), C.c_int64(0)
    check(lib().refnerf_get_timing_family(family, C.byref(ms), C.byref(n)))
    return ms.value, n.value

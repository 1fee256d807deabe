"""CPU: the ctypes binding is read from include/refnerf_hip.h (refnerf_pl_amd._abi); the C compiler is the witness of the layouts."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import refnerf_pl_amd  # noqa: F401
from refnerf_pl_amd import _abi, _hip, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof of every parsed struct, offsetof and size of every parsed field, as gcc -std=c99 lays the header out."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this host")
    lines = []
    for s, cls in _abi.structs.items():
        lines.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s} *)0)->{f}));' for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text('#include <stdio.h>\n#include "refnerf_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe])
    said = {k: tuple(int(x) for x in v) for k, *v in (l.split() for l in subprocess.check_output([exe], text=True).splitlines())}
    mine = {}
    for s, cls in _abi.structs.items():
        mine[s] = (C.sizeof(cls),)
        mine.update({f"{s}.{f}": (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_})
    assert len(_abi.structs) == 16 and mine == said
    assert mine["refnerf_level_cfg"] == (100,) and mine["refnerf_level_out"] == (184,)
    assert mine["refnerf_train_batch_args"] == (240,) and mine["refnerf_train_batch_args.rays"] == (136, 72)
    assert mine["refnerf_vis_panels_args"] == (336,) and mine["refnerf_vis_cmap_args"] == (128,)
    assert mine["refnerf_vis_panels_args.d_normals"][1] == 4 * 8 and mine["refnerf_vis_cmap_args.null_color"][1] == 3 * 8
    # the public names are the parsed classes, and the name tuples _hip keeps are those structs' fields
    assert _hip.LevelCfg is _abi.structs["refnerf_level_cfg"] and _hip.TrainBatchArgs is _abi.structs["refnerf_train_batch_args"]
    assert _hip.OUT_FIELDS == tuple(n for n, _ in _hip.LevelOut._fields_)
    assert _hip.OUT_EXTRA_FIELDS == tuple(n for n, _ in _hip.LevelOutExtra._fields_)
    assert tuple("d_" + n for n in _hip.RAY_FIELDS) == tuple(n for n, _ in _hip.ImageRaysOut._fields_)
    panels = {n for n, _ in _hip.VisPanelsArgs._fields_}
    assert set(_hip.VIS_PANEL_INPUTS + _hip.VIS_PANEL_INPUTS_2 + _hip.VIS_PANEL_OUTPUTS + _hip.VIS_PANEL_OUTPUTS_2) < panels


def test_prototypes_are_bound_as_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "refnerf_hip.h")).read()
    assert len(_abi.prototypes) == len(set(re.findall(r"\b(refnerf_[a-z_0-9]+)\s*\(", hdr))) == 61
    lib = _hip.lib()
    for name, (restype, argtypes) in _abi.prototypes.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    restype, args = _abi.prototypes["refnerf_image_rays"]
    assert restype is C.c_int and len(args) == 15 and args[9] is C.c_float and args[10] is C.c_float and args[11] is C.c_int64
    assert args[8] is C.POINTER(_hip.LensDistortion) and args[13] is C.POINTER(_hip.ImageRaysOut) and args[14] is C.c_void_p
    assert _abi.prototypes["refnerf_packed_weights_bytes"] == (C.c_size_t, [C.c_int])
    assert _abi.prototypes["refnerf_last_error"] == (C.c_char_p, [])
    assert _abi.prototypes["refnerf_level_cfg_default"] == (None, [C.POINTER(_hip.LevelCfg)])
    assert _abi.prototypes["refnerf_get_timing_family"] == (C.c_int, [C.c_int, C.c_void_p, C.c_void_p])      # host pointers: void * too


def test_constants_come_from_the_header():
    assert _hip.ABI_VERSION == 11 and _hip.NUM_PARAMS == layout.NUM_PARAMS and _hip.NUM_PARAMS_EXT == _hip.NUM_PARAMS + 2 * 6 * 256 * 96
    assert _hip.RAYDIST == {None: 0, "piecewise": 1, "reciprocal": 2, "log": 3, "exp": 4, "sqrt": 5, "square": 6}
    assert _hip.SRGB_MODES == {"none": 0, "linear": 1, "norm_linear": 2, "srgb": 3, "norm_srgb": 4}
    assert _hip.CONSISTENCY_TYPES == {"mse": 0, "avg_mse": 1, "var": 2}
    assert _hip.PENALTIES == {"mse": 0, "charb": 1}
    assert _hip.VIS_CURVES == {"none": 0, "neg_log": 1, "log": 2}
    assert _hip.VIS_OPS == {"none": 0, "clip01": 1, "sqrt": 2}
    assert len(_abi.constants) == 59 and all(k.startswith("REFNERF_") for k in _abi.constants)
    for name, value in _abi.constants.items():
        assert getattr(_hip, name[len("REFNERF_"):]) == value, name
    assert (_hip.PREC_F16X2, _hip.IMAGE_F16X2_TRAIN, _hip.ACT_SQ, _hip.WGRAD_F16, _hip.DIRENC_POSENC, _hip.PROJ_SPHERICAL, _hip.PREP_RAW,
            _hip.TIMER_DATASET, _hip.VIS_MAX_PS, _hip.VIS_MAX_NORMALS, _hip.EINVAL) == (3, 4, 3, 2, 1, 1, 3, 4, 8, 4, -1)


MINIATURE = """
/* a comment with a ; and a { in it */
#ifndef MINI_H
#define MINI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define MINI_N 2
#define MINI_M (MINI_N + 1)
enum { MINI_A, MINI_B = 5, MINI_C };
typedef struct mini_inner { int32_t a; double b; } mini_inner;
typedef struct mini_outer {
  int32_t n, m;             /* a comma declarator */
  mini_inner in;            /* by value */
  const mini_inner *link;   /* a struct pointer */
  float pair[MINI_N];
  const void *d_x, *d_y[MINI_M];
} mini_outer;
size_t mini_bytes(const mini_outer *o, int64_t n);
void mini_reset(void);
const char *mini_name(int32_t which, const float *d_in, float *d_out);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_a_miniature_header():
    constants, structs, prototypes = _abi.parse(MINIATURE)
    assert constants == {"MINI_N": 2, "MINI_M": 3, "MINI_A": 0, "MINI_B": 5, "MINI_C": 6}
    inner, outer = structs["mini_inner"], structs["mini_outer"]
    assert list(structs) == ["mini_inner", "mini_outer"] and C.sizeof(inner) == 16
    # n 0, m 4, in 8 (8-aligned, 16 bytes), link 24, pair 32 (2 floats), d_x 40, d_y 48 (3 pointers): 72 bytes
    assert [(n, getattr(outer, n).offset, getattr(outer, n).size) for n, _ in outer._fields_] == [
        ("n", 0, 4), ("m", 4, 4), ("in", 8, 16), ("link", 24, 8), ("pair", 32, 8), ("d_x", 40, 8), ("d_y", 48, 24)]
    assert C.sizeof(outer) == 72
    fields = dict(outer._fields_)
    assert fields["in"] is inner and fields["link"] is C.POINTER(inner) and fields["pair"] is C.c_float * 2 and fields["d_y"] is C.c_void_p * 3
    assert prototypes == {"mini_bytes": (C.c_size_t, [C.POINTER(outer), C.c_int64]), "mini_reset": (None, []),
                          "mini_name": (C.c_char_p, [C.c_int32, C.c_void_p, C.c_void_p])}


@pytest.mark.parametrize("text,names", [
    ("typedef struct s { uint8_t x; } s;", "uint8_t"),                                   # an unknown type
    ("int f(const other_t *p);", "other_t"),                                             # ... also behind a pointer
    ("typedef struct s { int32_t n; void (*done)(int32_t); } s;", "(*done)(int32_t)"),   # a function pointer member
    ("typedef struct s { union { int32_t i; float f; } u; } s;", "union"),               # a union
    ("typedef union u { int32_t i; float f; } u;", "union"),
    ("typedef struct s { int32_t flag : 1; } s;", "flag : 1"),                           # a bit-field
    ("typedef struct s { int32_t n; float x[n]; } s;", "'n'"),                           # an array bound that is no constant
    ("int f(int32_t, float *d_out);", "int32_t"),                                        # an unnamed parameter
    ("int f(const float *);", "const float *"),
    ("int f(double ps[3]);", "ps[3]"),                                                   # an array parameter
    ("int f(int32_t n)", "int f(int32_t n)"),                                            # a declaration that does not end
    ("#define REFNERF_X 1.5", "1.5"),                                                    # not an integer
    ("#define REFNERF_X (REFNERF_Y + 1)", "REFNERF_Y"),                                  # names a later / missing constant
    ("#pragma pack(1)", "#pragma pack(1)"),
    ("typedef int32_t refnerf_index;", "typedef int32_t refnerf_index"),
    ("extern int refnerf_flag;", "extern int refnerf_flag"),
])
def test_parser_refuses_what_it_does_not_understand(text, names):
    with pytest.raises(_abi.HeaderError, match=re.escape(names)):
        _abi.parse("#include <stdint.h>\nint before(void);\n" + text + "\n")


def test_missing_header_is_named(tmp_path):
    with pytest.raises(_hip.HipLibraryError, match=re.escape(str(tmp_path / "nope.h"))):
        _abi.load(str(tmp_path / "nope.h"))


def test_tensor_argument_check():
    """_hip._arg on CPU tensors (no library call): a conforming tensor fails on the device kind alone; each other fault is
    named next to it; the exception type is the caller's."""
    good = torch.zeros(4, 3)
    with pytest.raises(ValueError, match=r"^x is not on a HIP device$"):
        _hip._arg(good, "x", shape=(4, 3), numel=12)
    for kw, t, fault in ((dict(), good.double(), "is torch.float64, not torch.float32"),
                         (dict(dtype=torch.int64), good, "is torch.float32, not torch.int64"),
                         (dict(shape=(3, 4)), good, "has shape (4, 3), not (3, 4)"),
                         (dict(shape=(4,)), good, "has shape (4, 3), not (4,)"),
                         (dict(numel=1), good, "has 12 elements, not 1"),
                         (dict(shape=(3, 4)), good.t(), "is not contiguous"),
                         (dict(), good[:, :2], "is not contiguous")):
        for exc in (ValueError, AssertionError):
            with pytest.raises(exc, match=re.escape(fault)) as e:
                _hip._arg(t, "x", exc=exc, **kw)
            assert str(e.value).startswith("x ") and "is not on a HIP device" in str(e.value)
    assert not isinstance(ValueError("x"), AssertionError)
    with pytest.raises(AssertionError):
        _hip._arg(good, "x", exc=AssertionError)
    assert _hip._arg(None, "x", optional=True) is None and _hip._arg(None, "x", optional=True, empty_null=True, shape=(2,)) is None
    for exc in (ValueError, AssertionError):
        with pytest.raises(exc, match="x: a tensor is required, not NoneType"):
            _hip._arg(None, "x", exc=exc)
        with pytest.raises(exc, match="a tensor is required, not list"):
            _hip._arg([1.0], "x", optional=True, exc=exc)
    # the empty-tensor option is decided after the checks: an empty tensor of the wrong shape or kind of device is still refused
    with pytest.raises(ValueError, match=re.escape("has shape (0, 3), not (0, 4), is not on a HIP device")):
        _hip._arg(torch.zeros(0, 3), "x", shape=(0, 4), empty_null=True)
    with pytest.raises(ValueError, match="^x is not on a HIP device$"):
        _hip._arg(torch.zeros(0, 3), "x", shape=(0, 3), empty_null=True)

    class Resident(torch.Tensor):      # a CPU tensor that answers is_cuda as a device tensor does: what the helper returns
        is_cuda = property(lambda self: True)
    here = good.as_subclass(Resident)
    assert _hip._arg(here, "x", shape=(4, 3), numel=12, device=torch.device("cpu")) == good.data_ptr() != 0
    assert _hip._arg(here, "x", empty_null=True) == good.data_ptr()
    assert _hip._arg(torch.zeros(0, 3).as_subclass(Resident), "x", shape=(0, 3), empty_null=True) is None
    assert _hip._arg(torch.zeros(0, 3).as_subclass(Resident), "x", shape=(0, 3)) is not None
    with pytest.raises(ValueError, match="^x is on cpu, not cuda:0$"):
        _hip._arg(here, "x", device=torch.device("cuda:0"))
    with pytest.raises(ValueError, match=re.escape("x has shape (4, 3), not (4,)") + "$"):
        _hip._arg(here, "x", shape=(4,))

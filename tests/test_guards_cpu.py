"""CPU: the guarded allocator of tests/guards.py against fake "kernels" written in ATen.  Each planted error -- a write
past the end, before the start, a whole row past the end, an element left unwritten -- must be reported, in float32,
float64 and int32 outputs, and a correct kernel must pass: this is how the checker of tests/test_guard_bands.py proves
that it would fail on a subtly wrong kernel without any GPU run designed to go wrong.  Also the coverage gate: every
entry of include/refnerf_hip.h is in the guard test's case table or in its exemption dict."""
import re

import pytest
import torch

import guards
from guards import Arena, guarded


def _flat_with_zones(arena, t):
    """(the whole buffer as a flat tensor of t's dtype, index of t's first element in it): what a stray store sees"""
    r = arena._record_of(t)
    assert r.lead % t.element_size() == 0
    return r.buf.view(t.dtype), r.lead // t.element_size()


def _kernel(arena, out, first=0, stop=None, skip=None):
    """The fake kernel: writes elements [first, stop) of `out` by flat index relative to its start -- outside [0, numel)
    lands wherever the buffer has memory there, as a device store would."""
    flat, base = _flat_with_zones(arena, out)
    n = out.numel()
    stop = n if stop is None else stop
    vals = torch.arange(first, stop).to(out.dtype)
    if skip is not None:
        keep = torch.arange(first, stop) != skip
        idx = (base + torch.arange(first, stop))[keep]
        flat[idx] = vals[keep]
    else:
        flat[base + first:base + stop] = vals


DTYPES = [torch.float32, torch.float64, torch.int32]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 3), (1,), (37, 129)])
def test_correct_kernel_passes(dtype, shape):
    a = Arena()
    out = a.alloc(shape, dtype, name="out")
    assert out.is_contiguous() and tuple(out.shape) == shape and out.data_ptr() % 512 == a._record_of(out).buf.data_ptr() % 512
    _kernel(a, out)
    a.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_one_past_the_end_is_reported(dtype):
    a = Arena()
    out = a.alloc((5, 3), dtype, name="out")
    _kernel(a, out, stop=16)
    size = out.element_size()
    with pytest.raises(AssertionError, match=rf"out: trailing red zone overwritten, \d+ bytes changed, bytes 0 \.\. {size - 1} past"):
        a.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_one_before_the_start_is_reported(dtype):
    a = Arena()
    out = a.alloc((5, 3), dtype, name="out")
    _kernel(a, out, first=-1)
    size = out.element_size()
    with pytest.raises(AssertionError, match=rf"out: leading red zone overwritten, \d+ bytes changed, bytes -{size} \.\. -1 before"):
        a.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_one_row_past_the_end_is_reported(dtype):
    a = Arena()
    out = a.alloc((5, 3), dtype, name="out")
    _kernel(a, out, stop=18)
    with pytest.raises(AssertionError, match=rf"trailing red zone overwritten.*bytes 0 \.\. {3 * out.element_size() - 1} past"):
        a.check()


def test_far_rows_of_a_wide_tensor_stay_inside_the_zone():
    """8 rows of the leading dimension fit the red zone even where that exceeds 4 KiB and the tensor's own size"""
    a = Arena()
    out = a.alloc((2, 4000), torch.float32, name="wide")
    assert a._record_of(out).zone >= 8 * 4000 * 4 and a._record_of(out).zone % 512 == 0
    _kernel(a, out, stop=2 * 4000 + 7 * 4000 + 1)
    with pytest.raises(AssertionError, match=rf"wide: trailing red zone overwritten.*bytes 0 \.\. {(7 * 4000 + 1) * 4 - 1} past"):
        a.check()
    assert guards.zone_bytes((1 << 20, 64), 4) == guards.MAX_ZONE and guards.zone_bytes((1,), 4) == guards.MIN_ZONE


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_interior_element_is_reported(dtype):
    a = Arena()
    out = a.alloc((5, 3), dtype, name="out")
    _kernel(a, out, skip=7)
    words = out.element_size() // 4
    with pytest.raises(AssertionError, match=rf"out: {words} 32-bit words never written, first at flat index 7 "):
        a.check()


def test_red_zones_only_registration_and_inputs():
    a = Arena(float_zone=float("nan"))
    acc = a.alloc((4, 3), torch.float32, fill=0.0, name="grads", reason="refnerf_hip.h: ACCUMULATES into d_param_grads")
    assert float(acc.abs().sum()) == 0.0
    src = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    x = a.put(src, name="x")
    idx = a.put(torch.tensor([2, 0], dtype=torch.int32), name="idx", int_zone=1)
    assert torch.equal(x, src)
    flat, base = _flat_with_zones(a, x)
    assert torch.isnan(flat[base - 1]) and torch.isnan(flat[base + 6])
    flat, base = _flat_with_zones(a, idx)
    assert int(flat[base - 1]) == 1 and int(flat[base + 2]) == 1
    a.check()                           # nothing of an accumulated output has to be written
    out = a.alloc((3,), torch.float32, name="opt")
    a.loose(out, "refnerf_hip.h: optional output")
    a.check()
    x[1, 1] = 9.0                       # an entry that writes into its input
    with pytest.raises(AssertionError, match=r"x: input modified, \d bytes changed, first at byte 1[6-9], last at 19"):
        a.check()


def test_guarded_routes_the_named_module_only():
    import types

    def call():
        return torch.empty((3, 2)), torch.zeros(4, dtype=torch.int32), torch.full((2,), 7.0), torch.empty(16, dtype=torch.uint8)
    # the same function as a member of another module: guarded() tells callers apart by their module's name
    wrapper = types.FunctionType(call.__code__, {"__name__": "fake_wrappers", "torch": torch}, "call")
    a = Arena()
    before = torch.empty
    with guarded(a, modules=("fake_wrappers",)):
        e, z, f, ws = wrapper()
        mine = torch.empty(3)           # this module is not routed
    assert torch.empty is before
    assert a.owns(e) and a.owns(z) and a.owns(f) and a.owns(ws) and not a.owns(mine)
    assert int(z.abs().sum()) == 0 and float(f.sum()) == 14.0
    with pytest.raises(AssertionError, match=r"call:\d+: 6 32-bit words never written, first at flat index 0"):
        a.check()                       # the torch.empty output is held to "fully written", zeros / full / bytes are not
    e.fill_(1.0)
    a.check()


def test_every_abi_entry_is_guarded_or_exempt():
    """The coverage gate: a new entry of the header cannot arrive unguarded."""
    from refnerf_pl_amd import _abi
    import test_guard_bands as guard_cases      # (importing it touches no device)
    covered = set()
    for case in guard_cases.CASES:
        covered.update(case.entries)
    names = set(_abi.prototypes)
    assert not (covered | set(guard_cases.EXEMPT)) - names, "the case table names entries the header does not have"
    assert not covered & set(guard_cases.EXEMPT), "an entry is both guarded and exempt"
    for name, reason in guard_cases.EXEMPT.items():
        assert reason and re.search(r"_bytes(_basis)?$|_default$|abi_version|device_ok|last_error|level_image|activations_format|timing", name), name
    uncovered = names - covered - set(guard_cases.EXEMPT)
    assert uncovered == set(), f"entries without a guard-band case or an exemption: {sorted(uncovered)}"

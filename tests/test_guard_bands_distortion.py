"""The two entries of include/refnerf_distortion.h under guard bands (tests/guards.py), exactly as tests/test_guard_bands.py
holds every launching entry of include/refnerf_hip.h: per case one plain call and two guarded calls on the same inputs;
  (a) Arena.check(): no red-zone byte changed, no input changed, every output element written;
  (b) the guarded outputs are bit-equal to the plain call's: results do not depend on where buffers live;
  (c) the guarded outputs with the float inputs' red zones all zero and all NaN are bit-equal: no stray read reaches a result.
The allocators, the Case record and the driver are test_guard_bands's own (importing that module touches no device).  The new
header has a coverage gate of its own here, on the CPU: refnerf_hip.h's gate (tests/test_guards_cpu.py) reads only that header."""
import os

import pytest

import distortion_cases as DC
import test_guard_bands as GB
from refnerf_pl_amd import _hip

SHAPES = [(1, 1), (5, 65), (9, 512)]        # (R, N): the minimum; R and N off the block and the lane trips; the largest N
CASES = []
EXEMPT = {}                                 # both entries launch


def _distortion(R, N, backward):
    def fn(G):
        t, w = DC.rows("random", R, N, 31)
        args = (G.f(GB.T(t), name="t"), G.f(GB.T(w), name="w"))
        if backward:
            return dict(grad_w=_hip.distortion_backward(*args, G.f(GB.T(GB.f32([0.7])), name="g")))
        return dict(ray_loss=_hip.distortion_forward(*args))
    return fn


for _R, _N in SHAPES:
    CASES.append(GB.Case(f"distortion_forward-{_R}x{_N}", ["refnerf_distortion_forward"], _distortion(_R, _N, False)))
    CASES.append(GB.Case(f"distortion_backward-{_R}x{_N}", ["refnerf_distortion_backward"], _distortion(_R, _N, True)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_guard_bands_distortion(case):
    _hip.require_device()
    try:
        GB._run_case(case)
    except (_hip.HipLibraryError, RuntimeError) as e:
        if isinstance(e, _hip.HipLibraryError) or "HIP error" in str(e) or "hip error" in str(e):
            pytest.exit(f"{case.id}: the HIP runtime reported an error; nothing more is started on this device: {e}", returncode=3)
        raise


def test_every_entry_of_the_distortion_header_is_guarded():
    """The coverage gate of include/refnerf_distortion.h: a new entry of this header cannot arrive unguarded."""
    from refnerf_pl_amd import _abi
    header = os.path.join(os.path.dirname(__file__), "..", "include", "refnerf_distortion.h")
    names = set(_abi.load(header)[2])
    covered = set()
    for case in CASES:
        covered.update(case.entries)
    assert len(names) == 2
    assert not (covered | set(EXEMPT)) - names, "the case table names entries the header does not have"
    assert names - covered - set(EXEMPT) == set(), f"entries without a guard-band case: {sorted(names - covered)}"
    assert not covered & set(GB.EXEMPT) and not names & set(_abi.prototypes)

"""The launching entry of include/refnerf_raycast.h under guard bands (tests/guards.py), exactly as
tests/test_guard_bands_tsdf.py holds the entries of include/refnerf_tsdf.h: per case one plain call and two guarded calls on
the same inputs;
  (a) Arena.check(): no red-zone byte changed, no input changed, every output element written -- the miss paths (off the
      box, no bracket, an 8 x 8 tile that hangs over the image) are what this catches;
  (b) the guarded outputs are bit-equal to the plain call's: results do not depend on where buffers live;
  (c) the guarded outputs with the float inputs' red zones all zero and all NaN are bit-equal: no corner read past the grid
      reaches a result.
The allocators, the Case record and the driver are test_guard_bands's own (importing that module touches no device).  The
header has a coverage gate of its own here, on the CPU."""
import os

import pytest

import raycast_cases as RC
import test_guard_bands as GB
from refnerf_pl_amd import _hip

# (fixture of raycast_cases: grid, view W x H): the single cell; image sides off the 8 x 8 tile; nx one over a 64-lane trip
SHAPES = ["cell-5x4", "9x6x5-13x11", "65x3x2-40x24"]
CASES = []
EXEMPT = {}


def _raycast(name, colour):
    def fn(G):
        c = RC.case(name)
        grid = _hip.tsdf_grid(c["dims"], c["origin"], c["h"], 4 * c["h"])
        tsdf, weight = G.f(GB.T(c["tsdf"]), name="tsdf"), G.f(GB.T(c["weight"]), name="weight")
        rgb = G.f(GB.T(c["rgb"]), name="rgb") if colour else None
        p2c, c2w = G.f(GB.T(c["pixtocam"]), name="pixtocam"), G.f(GB.T(c["camtoworld"][None]), name="camtoworlds")
        depth, normals, view_rgb, acc = _hip.tsdf_raycast(grid, tsdf, weight, rgb, p2c, c2w, 0, *c["size"], 0.0, 1.0, 0.5, 4)
        return dict(depth=depth, normals=normals, acc=acc, **(dict(rgb=view_rgb) if colour else {}))
    return fn


for _name in SHAPES:
    CASES.append(GB.Case(f"tsdf_raycast-{_name}", ["refnerf_tsdf_raycast"], _raycast(_name, True)))
    CASES.append(GB.Case(f"tsdf_raycast-plain-{_name}", ["refnerf_tsdf_raycast"], _raycast(_name, False)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_guard_bands_raycast(case):
    _hip.require_device()
    try:
        GB._run_case(case)
    except (_hip.HipLibraryError, RuntimeError) as e:
        if isinstance(e, _hip.HipLibraryError) or "HIP error" in str(e) or "hip error" in str(e):
            pytest.exit(f"{case.id}: the HIP runtime reported an error; nothing more is started on this device: {e}", returncode=3)
        raise


def test_every_entry_of_the_raycast_header_is_guarded():
    """The coverage gate of include/refnerf_raycast.h: a new entry of this header cannot arrive unguarded."""
    from refnerf_pl_amd import _abi
    include = os.path.join(os.path.dirname(__file__), "..", "include")
    names = set(_abi.load(os.path.join(include, "refnerf_raycast.h"))[2])
    covered = set()
    for case in CASES:
        covered.update(case.entries)
    assert len(names) == 1
    assert not (covered | set(EXEMPT)) - names, "the case table names entries the header does not have"
    assert names - covered - set(EXEMPT) == set(), f"entries without a guard-band case: {sorted(names - covered)}"
    assert not covered & set(GB.EXEMPT) and not names & set(_abi.prototypes)
    assert not names & set(_abi.load(os.path.join(include, "refnerf_tsdf.h"))[2])

"""The launching entries of include/refnerf_tsdf.h under guard bands (tests/guards.py), exactly as tests/test_guard_bands.py
holds every launching entry of include/refnerf_hip.h: per case one plain call and two guarded calls on the same inputs;
  (a) Arena.check(): no red-zone byte changed, no input changed, every output element written;
  (b) the guarded outputs are bit-equal to the plain call's: results do not depend on where buffers live;
  (c) the guarded outputs with the float inputs' red zones all zero and all NaN are bit-equal: no stray read reaches a result.
The allocators, the Case record and the driver are test_guard_bands's own (importing that module touches no device).  The
volume arrays of refnerf_tsdf_integrate are updated in place and skipped voxels are not written (the header says so): they are
`inout` tensors, red zones only.  The header has a coverage gate of its own here, on the CPU."""
import os

import pytest

import test_guard_bands as GB
import tsdf_cases as TC
from refnerf_pl_amd import _hip

# (grid, view W x H): the minimum grid; distinct dimensions off every trip; nx one over a 64-lane trip
SHAPES = [((2, 2, 2), (5, 4)), ((9, 6, 5), (13, 11)), ((65, 3, 2), (40, 24))]
CASES = []
EXEMPT = {"refnerf_tsdf_mesh_workspace_bytes": "size query"}
IN_PLACE = "include/refnerf_tsdf.h, refnerf_tsdf_integrate: the volume is updated in place, a skipped voxel is not written"


def _integrate(dims, size, colour):
    def fn(G):
        S = TC.scene(dims, size)
        grid = _hip.tsdf_grid(dims, S["origin"], S["h"], S["trunc"])
        tsdf, weight, rgb = (G.inout(GB.T(a), IN_PLACE, name=n) for a, n in zip(TC.sentinel_state(dims), ("tsdf", "weight", "rgb")))
        c2w = G.f(GB.T(GB.f32([v["camtoworld"] for v in S["views"]])), name="camtoworlds")
        for n, view in enumerate(S["views"]):
            _hip.tsdf_integrate(grid, tsdf, weight, rgb if colour else None, G.f(GB.T(view["pixtocam"]), name="pixtocam"), c2w, n,
                                G.f(GB.T(view["depth"]), name="depth"), G.f(GB.T(view["acc"]), name="acc") if colour else None, 0.5,
                                G.f(GB.T(view["rgb"]), name="view_rgb") if colour else None, 1.5, 0.0)
        return dict(tsdf=tsdf, weight=weight, **(dict(rgb=rgb) if colour else {}))
    return fn


def _mesh(dims, emit):
    def fn(G):
        grid = _hip.tsdf_grid(dims, (0.1, -0.2, 0.3), 0.125, 0.5)
        tsdf, weight, rgb = TC.random_volume(dims, seed=sum(dims))
        tsdf, weight, rgb = G.f(GB.T(tsdf), name="tsdf"), G.f(GB.T(weight), name="weight"), G.f(GB.T(rgb), name="rgb")
        workspace, counts = _hip.tsdf_mesh_count(grid, tsdf, weight, 0.05, 1.0)
        N = dims[0] * dims[1] * dims[2]
        used = 9 * N + 8 * ((N + 255) // 256)              # the bytes the entry defines; the rest pads the size to 16
        if not emit:
            return dict(counts=counts, workspace=workspace[:used])
        n_vertices, n_triangles = counts.cpu().tolist()
        assert n_vertices > 0 and n_triangles > 0
        vertices, colors, triangles = _hip.tsdf_mesh_emit(grid, tsdf, rgb, 0.05, workspace, n_vertices, n_triangles)
        return dict(vertices=vertices, colors=colors, triangles=triangles)
    return fn


for _dims, _size in SHAPES:
    _id = "%dx%dx%d" % _dims
    CASES.append(GB.Case(f"tsdf_integrate-{_id}", ["refnerf_tsdf_integrate"], _integrate(_dims, _size, True)))
    CASES.append(GB.Case(f"tsdf_integrate-plain-{_id}", ["refnerf_tsdf_integrate"], _integrate(_dims, _size, False)))
    CASES.append(GB.Case(f"tsdf_mesh_count-{_id}", ["refnerf_tsdf_mesh_count"], _mesh(_dims, False)))
    CASES.append(GB.Case(f"tsdf_mesh_emit-{_id}", ["refnerf_tsdf_mesh_count", "refnerf_tsdf_mesh_emit"], _mesh(_dims, True)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_guard_bands_tsdf(case):
    _hip.require_device()
    try:
        GB._run_case(case)
    except (_hip.HipLibraryError, RuntimeError) as e:
        if isinstance(e, _hip.HipLibraryError) or "HIP error" in str(e) or "hip error" in str(e):
            pytest.exit(f"{case.id}: the HIP runtime reported an error; nothing more is started on this device: {e}", returncode=3)
        raise


def test_every_entry_of_the_tsdf_header_is_guarded():
    """The coverage gate of include/refnerf_tsdf.h: a new entry of this header cannot arrive unguarded."""
    from refnerf_pl_amd import _abi
    header = os.path.join(os.path.dirname(__file__), "..", "include", "refnerf_tsdf.h")
    names = set(_abi.load(header)[2])
    covered = set()
    for case in CASES:
        covered.update(case.entries)
    assert len(names) == 4
    assert not (covered | set(EXEMPT)) - names, "the case table names entries the header does not have"
    assert names - covered - set(EXEMPT) == set(), f"entries without a guard-band case: {sorted(names - covered)}"
    assert not covered & set(GB.EXEMPT) and not names & set(_abi.prototypes)

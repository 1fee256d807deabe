"""Geometry export: TSDF fusion and marching tetrahedra (include/refnerf_tsdf.h, csrc/refnerf_tsdf.h) and their interface
refnerf_pl_amd.geometry.

Truth is the header's own definition restated in float64 numpy (tsdf_cases.integrate_mirror) and as plain loops
(tsdf_cases.extract_mirror).  Every line of the definition is an IEEE operation in double on float32 inputs, rounded once at
the store, so the comparison is bit equality throughout: no tolerance, no excluded voxels.  On the CPU the mirrors are
checked against geometry (planes, the sphere's surface and volume) and topology; on the GPU the kernels against the mirrors.

Sphere fixture (12 x 11 x 10, h = 1/8, r = 0.45): 726 vertices, 2172 edges, 1448 triangles; the surface error bound is
delta = 3 h^2 / (8 (r - sqrt(3) h)) = 0.0251 (linear interpolation of a distance function along an edge of length at most
sqrt(3) h), the volume between the balls of radius r - delta - s and r + delta, s = 3 h^2 / (8 (r - delta)) the chord sagitta."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import refnerf_pl_amd  # noqa: F401
import tsdf_cases as TC
from refnerf_pl_amd import _abi, _hip, geometry

DEV = "cuda:0"
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "refnerf_tsdf.h")
ENTRIES = ["refnerf_tsdf_integrate", "refnerf_tsdf_mesh_workspace_bytes", "refnerf_tsdf_mesh_count", "refnerf_tsdf_mesh_emit"]
EPS32 = float(np.finfo(np.float32).eps)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} values differ, first at flat index {bad[0]}: " \
                          f"{got.reshape(-1)[bad[0]]!r} vs {want.reshape(-1)[bad[0]]!r}"


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_header_parses_and_is_disjoint_from_the_main_header():
    constants, structs, prototypes = _abi.load(HEADER)
    assert sorted(prototypes) == sorted(ENTRIES) and not constants and list(structs) == ["refnerf_tsdf_grid"]
    assert not set(prototypes) & set(_abi.prototypes) and not set(structs) & set(_abi.structs)
    grid = C.POINTER(structs["refnerf_tsdf_grid"])
    p, i32, f = C.c_void_p, C.c_int32, C.c_float
    assert prototypes["refnerf_tsdf_integrate"] == (C.c_int, [grid, p, p, p, p, p, i32, i32, i32, i32, p, p, f, p, f, f, p])
    assert prototypes["refnerf_tsdf_mesh_workspace_bytes"] == (C.c_size_t, [grid])
    assert prototypes["refnerf_tsdf_mesh_count"] == (C.c_int, [grid, p, p, f, f, p, C.c_size_t, p, p])
    assert prototypes["refnerf_tsdf_mesh_emit"] == (C.c_int, [grid, p, p, f, p, C.c_size_t, C.c_int64, C.c_int64, p, p, p, p])
    fields = [(n, t) for n, t in structs["refnerf_tsdf_grid"]._fields_]
    assert [n for n, _ in fields] == ["nx", "ny", "nz", "origin", "voxel_size", "trunc"] and C.sizeof(structs["refnerf_tsdf_grid"]) == 32
    assert _hip.TSDF_HEADER == os.path.normpath(HEADER) and _hip.TsdfGrid._fields_ == structs["refnerf_tsdf_grid"]._fields_
    assert _abi.constants["REFNERF_ABI_VERSION"] == 11          # the main header is untouched


def test_plane_exactness():
    """A fronto-parallel plane: the projective sdf is the Euclidean one, and every updated voxel holds
    clamp((D0 - z) / trunc) within one float32 rounding of a double value (the bar is 2 eps32)."""
    dims, h, trunc, D0 = (9, 6, 5), 0.125, 0.2, 2.0
    origin = (-0.5, -0.3, -0.25)
    c2w = TC.look_at((0.0, 0.0, 2.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))          # looks straight down -z: z-depth = 2 - P.z
    assert np.array_equal(c2w[:, :3], np.eye(3, dtype=np.float32))
    depth = np.full((24, 40), D0, np.float32)
    state = TC.sentinel_state(dims)
    tsdf, weight, _, ok = TC.integrate_mirror(dims, origin, h, trunc, state[0], state[1], None, TC.pixtocam(40, 24, 30.0, skew=0.0), c2w, depth)
    zdepth = 2.0 - (np.float64(np.float32(origin[2])) + np.arange(dims[2]) * np.float64(np.float32(h)))
    want = np.clip((np.float64(np.float32(D0)) - zdepth) / np.float64(np.float32(trunc)), None, 1.0)[:, None, None] * np.ones(tsdf.shape)
    assert ok.sum() > 100 and (~ok).sum() > 0                       # the far slab is cut by -trunc
    assert np.array_equal(ok, want >= -1.0) and (want[ok] == 1.0).any()        # every voxel is in the image; the near slab clamps
    err = np.abs(tsdf.astype(np.float64) - want)[ok]
    print("plane: worst |tsdf - exact| =", err.max(), "bar", 2 * EPS32)
    assert err.max() <= 2 * EPS32
    assert np.all(tsdf[~ok] == TC.SENTINEL["tsdf"]) and np.all(weight[ok] == 1) and np.all(weight[~ok] == 0)
    # and the module's restatement (device='cpu') is the mirror, bit for bit
    vol = geometry.TSDFVolume(origin, np.asarray(origin) + (np.asarray(dims) - 1) * h, voxel_size=h, trunc=trunc, color=False, device="cpu")
    assert vol.dims == dims
    vol.tsdf.fill_(TC.SENTINEL["tsdf"])
    vol.integrate(depth, TC.pixtocam(40, 24, 30.0, skew=0.0), c2w)
    assert_bit_equal(vol.tsdf.numpy(), tsdf, "geometry cpu tsdf")
    assert_bit_equal(vol.weight.numpy(), weight, "geometry cpu weight")


@functools.lru_cache(maxsize=None)
def mirror_mesh(name):
    """(dims, origin, h, tsdf, weight, rgb, iso, min_weight, (vertices, triangles, colours)) of the extraction fixtures"""
    if name == "fused":
        S, (tsdf, weight, rgb) = TC.fused_volume()
        dims, origin, h = S["dims"], S["origin"], S["h"]
    elif name == "empty":
        dims, origin, h = (9, 6, 5), (0.0, 0.0, 0.0), 0.125
        tsdf, weight, rgb = np.ones((5, 6, 9), np.float32), np.zeros((5, 6, 9), np.float32), np.zeros((5, 6, 9, 3), np.float32)
    else:
        dims, origin, h, tsdf, weight, rgb = TC.sphere_volume(quantum=0.25 if name == "degenerate" else None, unobserved=name == "unobserved")
    return dims, origin, h, tsdf, weight, rgb, 0.0, 1.0, TC.extract_mirror(dims, origin, h, tsdf, weight, rgb, 0.0, 1.0)


def check_closed(vertices, triangles, counts=None):
    top = TC.topology(vertices, triangles)
    assert top["once"] and not top["boundary"], "not a closed, consistently oriented manifold"
    assert top["used"] == top["V"] and top["V"] - top["E"] + top["F"] == 2, top
    assert np.isfinite(vertices).all()
    if counts:
        assert (top["V"], top["E"], top["F"]) == counts, top
    return top


def check_sphere(vertices, triangles):
    check_closed(vertices, triangles, (726, 2172, 1448))
    h, r = TC.SPHERE["h"], TC.SPHERE["r"]
    delta = 3 * h * h / (8 * (r - np.sqrt(3) * h))
    s = 3 * h * h / (8 * (r - delta))
    off = np.abs(np.linalg.norm(vertices.astype(np.float64) - np.asarray(TC.SPHERE["centre"]), axis=1) - r).max()
    vol = TC.signed_volume(vertices, triangles)
    ball = lambda rad: 4 / 3 * np.pi * rad ** 3       # noqa: E731
    print(f"sphere: worst distance to the surface {off:.4f} (bound {delta:.4f}); volume {vol:.4f} in [{ball(r - delta - s):.4f}, {ball(r + delta):.4f}]")
    assert off <= delta
    assert 0 < ball(r - delta - s) <= vol <= ball(r + delta)


def check_unobserved(vertices, triangles, dims, weight):
    """an open mesh: every boundary edge lies in a cell face shared with a cell that has an unobserved corner"""
    top = TC.topology(vertices, triangles)
    assert top["once"] and top["boundary"] and np.isfinite(vertices).all()
    h = TC.SPHERE["h"]
    nx, ny, nz = dims
    bad = np.zeros((nz - 1, ny - 1, nx - 1), bool)          # cells with an unobserved corner
    for m in range(8):
        bad |= weight[(m >> 2) & 1:nz - 1 + ((m >> 2) & 1), (m >> 1) & 1:ny - 1 + ((m >> 1) & 1), (m & 1):nx - 1 + (m & 1)] < 1
    for a, b in top["boundary"]:
        lo = np.minimum(vertices[a], vertices[b]).astype(np.float64) / h
        hi = np.maximum(vertices[a], vertices[b]).astype(np.float64) / h
        # the cells whose closed cube contains both ends
        rng = [range(max(int(np.ceil(hi[ax] - 1 - 1e-6)), 0), min(int(np.floor(lo[ax] + 1e-6)), n - 2) + 1) for ax, n in enumerate(dims)]
        touching = [(k, j, i) for i in rng[0] for j in rng[1] for k in rng[2]]
        assert touching and any(bad[c] for c in touching), ("a boundary edge away from every unobserved cell", vertices[a], vertices[b])


def test_sphere_mesh_is_closed_oriented_and_on_the_sphere():
    dims, origin, h, tsdf, weight, rgb, iso, mw, (v, f, c) = mirror_mesh("sphere")
    check_sphere(v, f)
    assert c.shape == v.shape and c.min() >= 0 and c.max() <= 1
    got = geometry.extract_mesh_host(dims, origin, h, tsdf, weight, rgb, iso, mw)
    for g, w, what in zip(got, (v, f, c), ("vertices", "triangles", "colours")):
        assert_bit_equal(g, w, "geometry.extract_mesh_host " + what)


def test_degenerate_values_keep_the_mesh_manifold():
    """tsdf rounded to multiples of 0.25: many corners equal iso exactly, many triangles have no area; the orientation is
    decided by the case, so the mesh stays closed, oriented and of Euler characteristic 2."""
    dims, origin, h, tsdf, weight, rgb, iso, mw, (v, f, c) = mirror_mesh("degenerate")
    assert (tsdf == 0).sum() > 50
    check_closed(v, f, (370, 1104, 736))
    assert TC.signed_volume(v, f) > 0 and np.isfinite(c).all()
    got = geometry.extract_mesh_host(dims, origin, h, tsdf, weight, rgb, iso, mw)
    for g, w, what in zip(got, (v, f, c), ("vertices", "triangles", "colours")):
        assert_bit_equal(g, w, "geometry.extract_mesh_host " + what)


def test_cells_with_an_unobserved_corner_emit_nothing():
    dims, origin, h, tsdf, weight, rgb, iso, mw, (v, f, c) = mirror_mesh("unobserved")
    full = mirror_mesh("sphere")[8]
    assert 0 < len(f) < len(full[1])
    check_unobserved(v, f, dims, weight)
    vol = geometry.TSDFVolume((0, 0, 0), (np.asarray(dims) - 1) * h, voxel_size=h, device="cpu")
    vol.tsdf.copy_(torch.from_numpy(tsdf)), vol.weight.copy_(torch.from_numpy(weight)), vol.rgb.copy_(torch.from_numpy(rgb))
    gv, gf, gc = vol.extract_mesh()
    assert_bit_equal(gv.numpy(), v, "vertices"), assert_bit_equal(gf.numpy(), f, "triangles"), assert_bit_equal(gc.numpy(), c, "colours")
    dims, *_, (v0, f0, c0) = mirror_mesh("empty")
    assert v0.shape == (0, 3) and f0.shape == (0, 3)


def test_fused_fixture_has_a_surface():
    S, (tsdf, weight, rgb) = TC.fused_volume()
    v, f, c = mirror_mesh("fused")[8]
    assert len(f) > 100 and weight.max() == 3 and (weight == 0).any() and np.isfinite(v).all()
    vol = geometry.TSDFVolume(S["origin"], np.asarray(S["origin"]) + (np.asarray(S["dims"]) - 1) * S["h"], voxel_size=S["h"], trunc=S["trunc"],
                              device="cpu")
    assert vol.dims == S["dims"]
    for view in S["views"]:
        vol.integrate(view["depth"], view["pixtocam"], view["camtoworld"], rgb=view["rgb"], acc=view["acc"])
    assert_bit_equal(vol.tsdf.numpy(), tsdf, "tsdf"), assert_bit_equal(vol.weight.numpy(), weight, "weight"), assert_bit_equal(vol.rgb.numpy(), rgb, "rgb")


def read_ply(path):
    """a minimal reader of what save_ply writes"""
    with open(path, "rb") as fp:
        data = fp.read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    colour = "property uchar red" in lines
    vt = np.dtype([("p", "<f4", (3,))] + ([("c", "u1", (3,))] if colour else []))
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(body) == nv * vt.itemsize + nf * ft.itemsize
    vert = np.frombuffer(body, vt, nv)
    face = np.frombuffer(body, ft, nf, offset=nv * vt.itemsize)
    assert np.all(face["n"] == 3)
    return vert["p"], face["v"], vert["c"] if colour else None


def test_save_ply_round_trips(tmp_path):
    v, f, c = mirror_mesh("sphere")[8]
    c = c.copy()
    c[0], c[1] = (np.nan, -0.5, 1.5), (0.5, 1.0, 0.999)
    geometry.save_ply(tmp_path / "m.ply", torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c))
    pv, pf, pc = read_ply(tmp_path / "m.ply")
    assert_bit_equal(pv, v, "vertices"), assert_bit_equal(pf, f, "faces")
    assert np.array_equal(pc, (np.clip(np.nan_to_num(c), 0, 1) * 255).astype(np.uint8))
    assert pc[0].tolist() == [0, 0, 255] and pc[1].tolist() == [127, 255, 254]
    geometry.save_ply(tmp_path / "n.ply", v, f)
    pv, pf, pc = read_ply(tmp_path / "n.ply")
    assert pc is None and np.array_equal(pv, v) and np.array_equal(pf, f)
    with pytest.raises(ValueError):
        geometry.save_ply(tmp_path / "bad.ply", v, f, c[:5])


def test_volume_arguments_and_refused_cameras():
    with pytest.raises(ValueError):
        geometry.TSDFVolume((0, 0, 0), (1, 1, 1), device="cpu")
    with pytest.raises(ValueError):
        geometry.TSDFVolume((0, 0, 0), (1, 1, 1), resolution=8, voxel_size=0.1, device="cpu")
    with pytest.raises(ValueError):
        geometry.TSDFVolume((0, 0, 0), (1, 0, 1), resolution=8, device="cpu")
    with pytest.raises(ValueError, match="2\\^31"):
        geometry.TSDFVolume((0, 0, 0), (1, 1, 1), resolution=700, device="cpu")
    vol = geometry.TSDFVolume((0, 0, 0), (1, 0.5, 0.25), resolution=9, device="cpu")
    assert vol.dims == (9, 5, 3) and vol.voxel_size == 0.125 and vol.trunc == 0.5 and tuple(vol.rgb.shape) == (3, 5, 9, 3)
    assert geometry.TSDFVolume((0, 0, 0), (1, 0.5, 0.25), resolution=(5, 4, 3), color=False, device="cpu").rgb is None
    p2c, c2w = TC.pixtocam(4, 4, 4.0), TC.look_at((0, 0, 3), (0, 0, 0), up=(0, 1, 0))[None]
    rendering = dict(distance_median=torch.full((4, 4), 2.9), acc=torch.ones(4, 4), rgb=torch.ones(4, 4, 3))
    with pytest.raises(ValueError, match="NDC"):
        vol.integrate_rendering(rendering, (p2c, c2w, None, p2c), 0)
    with pytest.raises(ValueError, match="distortion"):
        vol.integrate_rendering(rendering, (p2c, c2w, dict(k1=0.1), None), 0)

    class Pano:
        cameras, spherical = (p2c, c2w, None, None), True
    with pytest.raises(ValueError, match="spherical"):
        vol.integrate_rendering(rendering, Pano(), 0)
    bad = p2c.copy()
    bad[2] = (0, 1e-3, 1)
    with pytest.raises(ValueError, match="third row"):
        vol.integrate(torch.ones(4, 4), bad, c2w[0], rgb=torch.ones(4, 4, 3))
    with pytest.raises(ValueError, match="rgb"):
        vol.integrate(torch.ones(4, 4), p2c, c2w[0])
    vol.integrate_rendering(rendering, (p2c, c2w, None, None), 0)
    assert float(vol.weight.max()) == 1


# ----------------------------------------------------------------------------------------------------------------- GPU
def _hip_guard(fn, *a, **kw):
    """the pytest.exit pattern of the guard-band tests: after a HIP error nothing more is started on the device"""
    try:
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        return out
    except (_hip.HipLibraryError, RuntimeError) as e:
        if isinstance(e, _hip.HipLibraryError) or "HIP error" in str(e) or "hip error" in str(e):
            pytest.exit(f"the HIP runtime reported an error; nothing more is started on this device: {e}", returncode=3)
        raise


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


INTEGRATE_SHAPES = [((9, 6, 5), (13, 11)), ((33, 17, 9), (40, 24))]


@functools.lru_cache(maxsize=None)
def integrate_truth(dims, size, colour, use_acc, view_weight):
    """the mirror's state after one and after three sequential views; computed once, left unchanged"""
    S = TC.scene(dims, size)
    state = TC.sentinel_state(dims)
    state = (state[0], state[1], state[2] if colour else None)
    states, touched = [], None
    for view in S["views"]:
        *state, ok = TC.integrate_mirror(dims, S["origin"], S["h"], S["trunc"], *state, view["pixtocam"], view["camtoworld"], view["depth"],
                                         view["acc"] if use_acc else None, 0.5, view["rgb"] if colour else None, view_weight, 0.05)
        touched = ok if touched is None else touched | ok
        states.append((tuple(state), touched.copy()))
    return S, states


@pytest.mark.gpu
@pytest.mark.parametrize("colour,use_acc,view_weight", [(True, True, 1.0), (False, False, 1.0), (True, False, 0.375), (False, True, 2.5)],
                         ids=["rgb-acc", "plain", "rgb-w0.375", "acc-w2.5"])
@pytest.mark.parametrize("dims,size", INTEGRATE_SHAPES, ids=["9x6x5-13x11", "33x17x9-40x24"])
def test_hip_integrate_is_the_mirror_bit_for_bit(dims, size, colour, use_acc, view_weight):
    _hip.require_device()
    S, states = integrate_truth(dims, size, colour, use_acc, view_weight)
    grid = _hip.tsdf_grid(dims, S["origin"], S["h"], S["trunc"])
    tsdf, weight, rgb = (T(a) for a in TC.sentinel_state(dims))
    rgb = rgb if colour else None
    c2w = T(np.stack([v["camtoworld"] for v in S["views"]]))
    for n, view in enumerate(S["views"]):
        _hip_guard(_hip.tsdf_integrate, grid, tsdf, weight, rgb, T(view["pixtocam"]), c2w, n, T(view["depth"]),
                   T(view["acc"]) if use_acc else None, 0.5, T(view["rgb"]) if colour else None, view_weight, 0.05)
        if n in (0, 2):
            (want_tsdf, want_weight, want_rgb), touched = states[n]
            assert 0 < touched.sum() < touched.size                 # some voxels are behind the camera, off-image, or see holes
            assert_bit_equal(tsdf.cpu().numpy(), want_tsdf, f"tsdf after view {n}")
            assert_bit_equal(weight.cpu().numpy(), want_weight, f"weight after view {n}")
            assert np.all(want_tsdf[~touched] == TC.SENTINEL["tsdf"]) and np.all(want_weight[~touched] == 0)
            if colour:
                assert_bit_equal(rgb.cpu().numpy(), want_rgb, f"rgb after view {n}")
                assert np.all(want_rgb[~touched] == TC.SENTINEL["rgb"])
    # the fixture covers the branches: a view with voxels behind the camera, one with voxels off the image
    S0 = TC.scene(dims, size)
    assert len(S0["views"]) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "degenerate", "unobserved", "fused", "empty"])
def test_hip_extract_is_the_mirror_bit_for_bit(name):
    _hip.require_device()
    dims, origin, h, tsdf, weight, rgb, iso, mw, (v, f, c) = mirror_mesh(name)
    vol = geometry.TSDFVolume(origin, np.asarray(origin) + (np.asarray(dims) - 1) * h, voxel_size=h, device=DEV)
    assert vol.dims == dims
    vol.tsdf.copy_(T(tsdf)), vol.weight.copy_(T(weight)), vol.rgb.copy_(T(rgb))
    workspace, counts = _hip_guard(_hip.tsdf_mesh_count, vol.grid, vol.tsdf, vol.weight, iso, mw)
    assert counts.cpu().tolist() == [len(v), len(f)] and workspace.numel() == _hip.tsdf_mesh_workspace_bytes(vol.grid)
    gv, gf, gc = _hip_guard(vol.extract_mesh, iso, mw)
    gv, gf, gc = gv.cpu().numpy(), gf.cpu().numpy(), gc.cpu().numpy()
    assert_bit_equal(gv, v, "vertices"), assert_bit_equal(gf, f, "triangles"), assert_bit_equal(gc, c, "colours")
    if name == "sphere":
        check_sphere(gv, gf)
    elif name == "degenerate":
        check_closed(gv, gf, (370, 1104, 736))
    elif name == "unobserved":
        check_unobserved(gv, gf, dims, weight)
    elif name == "empty":
        assert gv.shape == (0, 3) and gf.shape == (0, 3)
    # without colour: the same vertices and triangles, no colour array
    vol.rgb = None
    gv2, gf2, gc2 = _hip_guard(vol.extract_mesh, iso, mw)
    assert gc2 is None and torch.equal(gv2.cpu(), torch.from_numpy(v)) and torch.equal(gf2.cpu(), torch.from_numpy(f))


@pytest.mark.gpu
def test_hip_volume_fuses_like_the_mirror():
    """TSDFVolume on the device, through integrate(): the fused fixture, bit for bit"""
    _hip.require_device()
    S, (tsdf, weight, rgb) = TC.fused_volume()
    vol = geometry.TSDFVolume(S["origin"], np.asarray(S["origin"]) + (np.asarray(S["dims"]) - 1) * S["h"], voxel_size=S["h"], trunc=S["trunc"],
                              device=DEV)
    for view in S["views"]:
        _hip_guard(vol.integrate, view["depth"], view["pixtocam"], view["camtoworld"], rgb=view["rgb"], acc=view["acc"])
    assert_bit_equal(vol.tsdf.cpu().numpy(), tsdf, "tsdf"), assert_bit_equal(vol.weight.cpu().numpy(), weight, "weight")
    assert_bit_equal(vol.rgb.cpu().numpy(), rgb, "rgb")


@pytest.mark.gpu
def test_hip_tsdf_argument_checks():
    _hip.require_device()
    lib = _hip.lib()
    EINVAL = _hip.EINVAL
    S = TC.scene((9, 6, 5), (13, 11))
    view = S["views"][0]
    good = _hip.tsdf_grid(S["dims"], S["origin"], S["h"], S["trunc"])
    tsdf, weight, rgb = (T(a) for a in TC.sentinel_state(S["dims"]))
    p2c, c2w, depth, acc, vrgb = T(view["pixtocam"]), T(view["camtoworld"][None]), T(view["depth"]), T(view["acc"]), T(view["rgb"])
    before = tsdf.clone()

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def integrate(grid=good, tsdf=tsdf, weight=weight, rgb=rgb, p2c=p2c, c2w=c2w, n_frames=1, frame=0, W=13, H=11, depth=depth, acc=acc,
                  vrgb=vrgb, w=1.0, z_min=0.0):
        return lib.refnerf_tsdf_integrate(C.byref(grid) if grid is not None else None, p(tsdf), p(weight), p(rgb), p(p2c), p(c2w), n_frames,
                                          frame, W, H, p(depth), p(acc), 0.5, p(vrgb), w, z_min, None)
    bad_row = view["pixtocam"].copy()
    bad_row[2] = (0, 0, 1.5)
    bad_grids = [_hip.tsdf_grid((1, 6, 5), S["origin"], S["h"], S["trunc"]), _hip.tsdf_grid((9, 6, 1), S["origin"], S["h"], S["trunc"]),
                 _hip.tsdf_grid((1024, 1024, 293), S["origin"], S["h"], S["trunc"]),          # 7 N = 2^31 + 3.1e6
                 _hip.tsdf_grid((65536, 65536, 2), S["origin"], S["h"], S["trunc"]),
                 _hip.tsdf_grid(S["dims"], S["origin"], S["h"], 0.0), _hip.tsdf_grid(S["dims"], S["origin"], S["h"], -1.0),
                 _hip.tsdf_grid(S["dims"], S["origin"], 0.0, S["trunc"]), _hip.tsdf_grid(S["dims"], S["origin"], S["h"], float("nan"))]
    refused = [integrate(grid=None), integrate(tsdf=None), integrate(weight=None), integrate(p2c=None), integrate(c2w=None),
               integrate(depth=None), integrate(rgb=None), integrate(vrgb=None), integrate(frame=1), integrate(frame=-1),
               integrate(n_frames=0), integrate(W=0), integrate(H=-3), integrate(w=0.0), integrate(w=float("nan")), integrate(z_min=-0.1),
               integrate(p2c=T(bad_row))] + [integrate(grid=g) for g in bad_grids]
    assert refused == [EINVAL] * len(refused), refused
    assert b"third row" in lib.refnerf_last_error() or b"grid" in lib.refnerf_last_error()
    assert 7 * 1024 * 1024 * 292 < 2 ** 31 <= 7 * 1024 * 1024 * 293
    assert _hip.tsdf_mesh_workspace_bytes(_hip.tsdf_grid((1024, 1024, 292), S["origin"], S["h"], S["trunc"])) > 0
    assert [_hip.tsdf_mesh_workspace_bytes(g) for g in bad_grids] == [0] * len(bad_grids)
    N = 9 * 6 * 5
    nbytes = _hip.tsdf_mesh_workspace_bytes(good)
    assert nbytes == (9 * N + 8 * ((N + 255) // 256) + 15) // 16 * 16
    ws, counts = torch.zeros(nbytes, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    verts, tris = torch.zeros((8, 3), device=DEV), torch.zeros((8, 3), dtype=torch.int32, device=DEV)

    def count(grid=good, tsdf=tsdf, weight=weight, iso=0.0, mw=1.0, ws=ws, nbytes=nbytes, counts=counts):
        return lib.refnerf_tsdf_mesh_count(C.byref(grid) if grid is not None else None, p(tsdf), p(weight), iso, mw, p(ws), nbytes, p(counts), None)

    def emit(grid=good, tsdf=tsdf, rgb=rgb, iso=0.0, ws=ws, nbytes=nbytes, V=8, Tn=8, verts=verts, vrgb=None, tris=tris):
        return lib.refnerf_tsdf_mesh_emit(C.byref(grid) if grid is not None else None, p(tsdf), p(rgb), iso, p(ws), nbytes, V, Tn, p(verts),
                                          p(vrgb), p(tris), None)
    refused = [count(grid=None), count(tsdf=None), count(weight=None), count(ws=None), count(counts=None), count(nbytes=nbytes - 1),
               count(nbytes=0), count(iso=float("nan")), count(grid=bad_grids[0]), count(grid=bad_grids[2]),
               emit(grid=None), emit(tsdf=None), emit(ws=None), emit(verts=None), emit(tris=None), emit(nbytes=nbytes - 16), emit(V=-1),
               emit(Tn=-1), emit(V=2 ** 31), emit(rgb=None, vrgb=verts), emit(grid=bad_grids[1]), emit(iso=float("inf"))]
    assert refused == [EINVAL] * len(refused), refused
    assert emit(V=0, Tn=0, verts=None, tris=None, tsdf=None, ws=None) == 0            # nothing to write: nothing is read, nothing launched
    torch.cuda.synchronize()
    assert torch.equal(tsdf, before) and not counts.any() and not verts.any()          # a refused call writes nothing
    # the wrappers raise ValueError before the library is reached
    with pytest.raises(ValueError):
        _hip.tsdf_integrate(good, tsdf.double(), weight, rgb, p2c, c2w, 0, depth, acc, 0.5, vrgb)
    with pytest.raises(ValueError):
        _hip.tsdf_integrate(good, tsdf, weight, rgb, p2c, c2w, 0, depth.t(), acc, 0.5, vrgb)
    with pytest.raises(ValueError):
        _hip.tsdf_integrate(good, tsdf, weight[:-1], rgb, p2c, c2w, 0, depth, acc, 0.5, vrgb)
    with pytest.raises(ValueError):
        _hip.tsdf_integrate(good, tsdf, weight, rgb, p2c, c2w, 0, depth, acc, 0.5, vrgb.cpu())
    with pytest.raises(ValueError, match="third row"):
        _hip.tsdf_integrate(good, tsdf, weight, rgb, T(bad_row), c2w, 0, depth, acc, 0.5, vrgb)
    with pytest.raises(ValueError):
        _hip.tsdf_mesh_count(good, tsdf, weight, workspace=ws[:-16])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fuse_views_on_the_fixture_scene(tmp_path):
    """Plumbing, not quality: the fixture Blender scene's test poses as 16 x 16 views, a model with synthetic weights,
    generate_ray_batch -> render_image -> integrate_rendering -> extract_mesh -> save_ply."""
    _hip.require_device()
    import importlib.util
    from helpers import GOLDEN, load_golden
    from refnerf_pl_amd import configs, datasets, models, synthetic
    spec = importlib.util.spec_from_file_location("make_golden_datasets", os.path.join(GOLDEN, "make_golden_datasets.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    z = load_golden("scene_datasets")
    blender = mk.write_scenes(z, str(tmp_path))[0]
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(os.path.dirname(GOLDEN), os.pardir, "configs", "refnerf_blender.gin")],
                                            ["Config.render_chunk_size = 128", "Model.num_prop_samples = 32", "Model.num_nerf_samples = 32"])
    cfg = configs.Config()
    dev = torch.device(DEV)
    model = models.construct_model(None, cfg).to(dev).eval()
    configs.clear_config()
    model.nerf_mlp.load_flat_params(synthetic.make_params(seed=0, bias_scale=0.05, sharpen=20.0))
    test = datasets.load_dataset("test", blender, cfg, device=dev)
    assert test.cameras[2] is None and test.cameras[3] is None
    from refnerf_pl_amd import camera_utils
    views = datasets.PathCameras(camera_utils.get_pixtocam(14.0, 16, 16), np.asarray(test.camtoworlds)[:2], 16, 16, cfg.near, cfg.far, device=dev)
    volume = geometry.TSDFVolume((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), resolution=24, device=dev)
    out = _hip_guard(geometry.fuse_views, lambda rays: model(rays, 1.0, True), views, cfg, volume, acc_threshold=0.0)
    assert out is volume and float(volume.weight.max()) >= 1 and bool(torch.isfinite(volume.tsdf).all())
    v, f, c = _hip_guard(volume.extract_mesh, min_weight=1.0)
    assert v.is_cuda and f.dtype == torch.int32 and c.shape == v.shape and f.shape[1] == 3
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(c).all())
    assert f.numel() == 0 or (int(f.min()) >= 0 and int(f.max()) < v.shape[0])
    geometry.save_ply(tmp_path / "mesh.ply", v, f, c)
    pv, pf, pc = read_ply(tmp_path / "mesh.ply")
    assert pv.shape == tuple(v.shape) and pf.shape == tuple(f.shape)
    # the dataset itself is a camera source too: one of its own 18 x 12 views
    geometry.fuse_views(lambda rays: model(rays, 1.0, True), test, cfg, volume, indices=[0], acc_threshold=0.0)
    torch.cuda.synchronize()

"""TSDF ray casting (include/refnerf_raycast.h, csrc/refnerf_raycast.h) and its interface in refnerf_pl_amd.geometry:
TSDFVolume.raycast / raycast_view, raycast_host, surface_metrics.

Truth is the header's definition as a plain loop in float64 (raycast_cases.raycast_mirror).  Every line of it is an IEEE
operation in double on float32 inputs, rounded once at the store, so the vectorised host path and the kernel are compared
with it bit for bit: no tolerance, no excluded pixels.  On the CPU the mirror itself is checked against geometry that does not
depend on the definition: a plane whose trilinear interpolant is exact, and the sphere fixture of tsdf_cases.

Bars.  Plane: the only error above double rounding is the one float32 rounding at the store, 2^-24 relative; the bar is 2^-23
(measured 4.2e-8).  Sphere (h = 1/8, r = 0.45): the trilinear error of a field is at most (h^2 / 8) * sum |d_ii f|, for the
distance to a sphere its Laplacian 2 / r, so the value is off by at most h^2 / (4 r); along a ray that divides by cos(theta),
at most 2 on the checked pixels (cos >= 0.5): h^2 / (2 r) = 0.0174; the bar is twice that, h^2 / r, because the trilinear
gradient is not exactly unit (measured 0.0138)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import refnerf_pl_amd  # noqa: F401
import raycast_cases as RC
import tsdf_cases as TC
from refnerf_pl_amd import _abi, _hip, geometry

DEV = "cuda:0"
INCLUDE = os.path.normpath(os.path.join(os.path.dirname(__file__), "..", "include"))
HEADER = os.path.join(INCLUDE, "refnerf_raycast.h")
NAMES = ("depth", "normals", "rgb", "acc")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} values differ, first at flat index {bad[0]}: " \
                          f"{got.reshape(-1)[bad[0]]!r} vs {want.reshape(-1)[bad[0]]!r}"


def assert_same_view(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert (g is None) == (w is None), (what, name)
        if w is not None:
            assert_bit_equal(g, w, f"{what}: {name}")


def host(c, colour=True, **kw):
    return geometry.raycast_host(c["dims"], c["origin"], c["h"], c["tsdf"], c["weight"], c["rgb"] if colour else None, c["pixtocam"],
                                 c["camtoworld"], *c["size"], **kw)


def check_rows(out):
    """misses are all-zero rows; hits have a positive finite depth and a unit (or zero) normal"""
    depth, normals, rgb, acc = out
    hit = acc == 1
    assert np.all((acc == 0) | hit)
    assert np.all(depth[~hit] == 0) and np.all(normals[~hit] == 0) and (rgb is None or np.all(rgb[~hit] == 0))
    assert np.all(np.isfinite(depth[hit]) & (depth[hit] > 0))
    norm = np.linalg.norm(normals[hit].astype(np.float64), axis=-1)
    assert np.all((np.abs(norm - 1) < 1e-6) | (norm == 0))
    assert rgb is None or (np.isfinite(rgb).all() and rgb.min() >= 0 and rgb.max() <= 1)


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_header_parses_through_its_quoted_include():
    constants, structs, prototypes = _abi.load(HEADER)
    assert list(prototypes) == ["refnerf_tsdf_raycast"] and not constants
    others = [_abi.load(os.path.join(INCLUDE, name))[2] for name in ("refnerf_hip.h", "refnerf_distortion.h", "refnerf_tsdf.h")]
    assert all(not set(prototypes) & set(o) for o in others)
    assert _hip.RAYCAST_HEADER == HEADER and _hip._raycast_prototypes == prototypes
    # the grid struct comes from the included header, and it is the class the other TSDF entries take
    assert list(structs) == ["refnerf_tsdf_grid"] and structs["refnerf_tsdf_grid"] is _hip.TsdfGrid
    grid, p, i32, f = C.POINTER(_hip.TsdfGrid), C.c_void_p, C.c_int32, C.c_float
    assert prototypes["refnerf_tsdf_raycast"] == (C.c_int, [grid, p, p, p, p, p, i32, i32, i32, i32, f, f, f, i32, f, f, p, p, p, p, p])
    # parse() opens no file: alone it does not know the struct, seeded it does, and returns the seeds with its own
    text = open(HEADER).read()
    with pytest.raises(_abi.HeaderError, match="refnerf_tsdf_grid"):
        _abi.parse(text)
    c2, s2, p2 = _abi.parse(text, structs={"refnerf_tsdf_grid": _hip.TsdfGrid}, constants={"SEED": 3})
    assert p2 == prototypes and s2 == {"refnerf_tsdf_grid": _hip.TsdfGrid} and c2 == {"SEED": 3}
    assert _abi.constants["REFNERF_ABI_VERSION"] == 11 and len(_abi.load(os.path.join(INCLUDE, "refnerf_tsdf.h"))[2]) == 4


def test_load_resolves_sibling_includes(tmp_path):
    (tmp_path / "base.h").write_text("#define BASE_N 2\ntypedef struct base_t { float v[BASE_N]; } base_t;\nint base_fn(const base_t *b);\n")
    (tmp_path / "user.h").write_text('#include <stdint.h>\n#include "base.h"\n#define USER_M (BASE_N + 1)\nint user_fn(const base_t *b, int32_t n);\n')
    constants, structs, prototypes = _abi.load(str(tmp_path / "user.h"))
    base = _abi.load(str(tmp_path / "base.h"))
    assert list(prototypes) == ["user_fn"] and constants == {"BASE_N": 2, "USER_M": 3}
    assert structs["base_t"] is base[1]["base_t"] and prototypes["user_fn"] == (C.c_int, [C.POINTER(base[1]["base_t"]), C.c_int32])
    (tmp_path / "lost.h").write_text('#include "nowhere.h"\nint f(void);\n')
    with pytest.raises(_hip.HipLibraryError, match="nowhere.h"):
        _abi.load(str(tmp_path / "lost.h"))
    (tmp_path / "loop.h").write_text('#include "loop.h"\nint f(void);\n')
    with pytest.raises(_abi.HeaderError, match="includes itself"):
        _abi.load(str(tmp_path / "loop.h"))


@pytest.mark.parametrize("name", list(RC.CASES))
def test_host_path_is_the_mirror_bit_for_bit(name):
    c = RC.case(name)
    hits = 0
    for colour, refine, step in RC.SWEEP:
        want = RC.truth(name, colour, refine, step)
        assert_same_view(host(c, colour, refine=refine, step=step), want, f"{name} colour={colour} refine={refine} step={step}")
        check_rows(want)
        hits += int(want[3].sum())
    assert hits > 0, "the fixture has no surface in view"
    if name in ("cell-5x4", "9x6x5-13x11", "65x3x2-40x24", "narrow", "zero-outside", "random-65x3"):
        assert (RC.truth(name)[3] == 0).any()                 # and it has misses


def test_plane_is_exact():
    """f = (2x + y + 2z - 3) / 4 is exact in float32 and linear, so its trilinear interpolant is the field: independent of
    the definition, every ray whose analytic hit lies more than a voxel inside the box hits at the analytic depth up to the
    float32 rounding of the store, with the normal (2, 1, 2) / 3."""
    P = RC.PLANE
    dims, origin, h, tsdf, weight, _ = RC.plane_volume()
    p2c, c2w = TC.pixtocam(*P["size"], P["focal"]), TC.look_at(P["eye"], P["target"])
    depth, normals, rgb, acc = geometry.raycast_host(dims, origin, h, tsdf, weight, None, p2c, c2w, *P["size"])
    assert rgb is None
    assert_same_view((depth, normals, None, acc), RC.raycast_mirror(dims, origin, h, tsdf, weight, None, p2c, c2w, *P["size"]), "plane")
    d, o = RC.ray_dirs(p2c, c2w, *P["size"])
    nv = np.asarray(P["normal"])
    ta = (P["offset"] - o @ nv) / (d @ nv)
    X = o + ta[..., None] * d
    lo, hi = RC._box(dims, origin, h)
    inside = ((X > lo + h) & (X < hi - h)).all(-1) & (ta > 0)
    assert inside.sum() >= 30 and acc[inside].all(), (int(inside.sum()), int(acc[inside].sum()))
    rel = (np.abs(depth.astype(np.float64) - ta) / ta)[inside].max()
    nerr = np.abs(normals[inside].astype(np.float64) - nv / 3).max()
    print(f"plane: {int(inside.sum())} of {inside.size} pixels checked, worst relative depth error {rel:.3g}, normal {nerr:.3g}; bar {2.0 ** -23:.3g}")
    assert rel <= 2.0 ** -23 and nerr <= 2.0 ** -23


def _sphere_analytic(c):
    d, o = RC.ray_dirs(c["pixtocam"], c["camtoworld"], *c["size"])
    ctr, r = np.asarray(TC.SPHERE["centre"]), TC.SPHERE["r"]
    oc = o - ctr
    A, B, Cq = (d * d).sum(-1), d @ oc, oc @ oc - r * r
    disc = B * B - A * Cq
    ta = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / A, np.nan)
    X = o + ta[..., None] * d
    cos = -((X - ctr) / r * d).sum(-1) / np.sqrt(A)
    return d, o, ta, X, cos, np.sqrt(A)


def test_sphere_depth_within_the_interpolation_bound():
    """on what geometry.raycast_host returns (and, bit-equal, on the mirror)"""
    c = RC.case("sphere")
    out = host(c)
    assert_same_view(out, RC.truth("sphere"), "sphere")
    depth, normals, rgb, acc = out
    d, o, ta, X, cos, length = _sphere_analytic(c)
    h, r, ctr = TC.SPHERE["h"], TC.SPHERE["r"], np.asarray(TC.SPHERE["centre"])
    sel = cos >= 0.5                                     # NaN where the ray misses the sphere: False
    assert sel.sum() >= 50 and acc[sel].all(), (int(sel.sum()), int(acc[sel].sum()))
    err = (np.abs(depth.astype(np.float64) - ta) * length)[sel].max()
    print(f"sphere: {int(sel.sum())} pixels with cos >= 0.5, all hit; worst world-space depth error {err:.4f}, h^2 / (2 r) = {h * h / (2 * r):.4f}, "
          f"bar h^2 / r = {h * h / r:.4f}")
    assert err <= h * h / r
    hit = acc > 0
    P = o + depth[hit].astype(np.float64)[:, None] * d[hit]
    assert ((normals[hit].astype(np.float64) * (P - ctr)).sum(-1) > 0).all()        # outward: towards free space
    assert rgb[hit].min() > 0


def test_semantics_of_the_march():
    S = TC.SPHERE
    # a camera inside the sphere sees only back faces: nothing
    inside = RC.sphere_case(eye=(0.72, 0.60, 0.65), focal=12.0)
    assert not host(inside)[3].any()
    # t_far < t_near is legal and misses everywhere; so does a t_near beyond the near surface: the far surface is a back face
    c = RC.case("sphere")
    assert RC.truth("sphere")[3].sum() > 50
    out = host(c, t_near=3.0, t_far=2.0)
    assert not out[3].any() and not out[0].any()
    centre_depth = float(np.linalg.norm(np.asarray(c["camtoworld"], np.float64)[:, 3] - np.asarray(S["centre"])))
    out = host(c, t_near=centre_depth)
    assert_same_view(out, RC.raycast_mirror(c["dims"], c["origin"], c["h"], c["tsdf"], c["weight"], c["rgb"], c["pixtocam"], c["camtoworld"],
                                            *c["size"], t_near=centre_depth), "t_near at the centre")
    assert not out[3].any()
    # ... and a t_far short of the sphere, while one just behind the near surface keeps the hits in front of it
    assert not host(c, t_far=centre_depth - S["r"] - 0.2)[3].any()
    near_half = host(c, t_far=centre_depth)
    assert 0 < near_half[3].sum() <= RC.truth("sphere")[3].sum() and np.all(near_half[0] <= np.float32(centre_depth))


def test_unobserved_cells_are_skipped_not_blocking():
    c = RC.case("unobserved")
    trace = {}
    depth, normals, rgb, acc = RC.raycast_mirror(c["dims"], c["origin"], c["h"], c["tsdf"], c["weight"], c["rgb"], c["pixtocam"], c["camtoworld"],
                                                 *c["size"], trace=trace)
    assert_same_view((depth, normals, rgb, acc), RC.truth("unobserved"), "trace changes nothing")
    full = RC.sphere_case(eye=(2.4, 1.9, 0.6))
    assert 0 < acc.sum() < host(full)[3].sum()
    # no hit point lies in a cell with an unobserved corner (a point on a cell face belongs to both cells: either may be clean)
    d, o = RC.ray_dirs(c["pixtocam"], c["camtoworld"], *c["size"])
    hit = acc > 0
    g = (o + depth[hit].astype(np.float64)[:, None] * d[hit] - np.asarray(c["origin"])) / c["h"]
    nx, ny, nz = c["dims"]
    for gi in g:
        clean = False
        for cell in {tuple(np.clip(np.floor(gi + s).astype(int), 0, (nx - 2, ny - 2, nz - 2))) for s in (-1e-5, 1e-5)}:
            i, j, k = cell
            clean |= bool((c["weight"][k:k + 2, j:j + 2, i:i + 2] >= 1).all())
        assert clean, gi
    # rays that crossed the unobserved block before they reached observed surface still hit it
    assert (hit & (trace["invalid"] > 0)).sum() >= 5


def test_zero_direction_components_and_values_on_the_iso():
    # d[a] == 0 with the origin inside the slab: the centre pixel looks straight down -z and hits the top of the sphere
    c = RC.case("zero-inside")
    d, o = RC.ray_dirs(c["pixtocam"], c["camtoworld"], *c["size"])
    assert d[3, 4, 0] == 0 and d[3, 4, 1] == 0 and d[3, 4, 2] == -1 and (d[:, 4, 0] == 0).all() and (d[3, :, 1] == 0).all()
    depth, normals, rgb, acc = RC.truth("zero-inside")
    S = TC.SPHERE
    assert acc[3, 4] == 1 and abs(float(depth[3, 4]) - (2.5 - S["centre"][2] - S["r"])) <= S["h"] ** 2 / S["r"]
    assert normals[3, 4, 2] > 0.99
    # ... and outside it: the whole centre column has d[0] == 0 and o[0] left of the box: it misses; other columns still hit
    c = RC.case("zero-outside")
    d, o = RC.ray_dirs(c["pixtocam"], c["camtoworld"], *c["size"])
    assert (d[:, 4, 0] == 0).all() and o[0] < c["origin"][0]
    acc = RC.truth("zero-outside")[3]
    assert not acc[:, 4].any() and acc.any()
    # a sample exactly on the iso value is outside: it opens a bracket with fa == 0, and without refinement t* is that sample
    c = RC.case("quantum")
    assert (c["tsdf"] == 0).sum() > 50
    trace = {}
    out = RC.raycast_mirror(c["dims"], c["origin"], c["h"], c["tsdf"], c["weight"], None, c["pixtocam"], c["camtoworld"], *c["size"], refine=0,
                            trace=trace)
    on_iso = (out[3] > 0) & (trace["fa"] == 0)
    assert on_iso.sum() >= 5 and np.array_equal(out[0][on_iso], trace["a"][on_iso].astype(np.float32))
    assert_same_view(out, RC.truth("quantum", False, 0, 0.5), "trace changes nothing")
    # an iso of its own moves the surface: the sphere of radius r + 0.1
    c = RC.case("sphere")
    out = host(c, iso=0.1)
    _, _, ta, _, cos, length = _sphere_analytic(c)
    sel = cos >= 0.5
    assert out[3][sel].all() and np.all((ta - out[0].astype(np.float64))[sel] * length[sel] > 0.05)


ROUND_TRIP_MEASURED = 0.021566391        # the worst |ray-cast depth - fused depth| of view 0, measured on the CPU mirror (h = 0.03125)


def test_round_trip_through_fusion():
    """fuse the 33 x 17 x 9 scene with the mirror of integrate, ray cast its view 0 through a cpu TSDFVolume holding the fused
    arrays: where the view's depth was fused and the ray hits, the two depths agree to well under a voxel.  The bound is a
    property of the fusion mirror (three views averaged into one field), not of the kernel: twice what the CPU measures."""
    S, (tsdf, weight, rgb) = TC.fused_volume()
    v = S["views"][0]
    vol = geometry.TSDFVolume(S["origin"], np.asarray(S["origin"]) + (np.asarray(S["dims"]) - 1) * S["h"], voxel_size=S["h"], trunc=S["trunc"],
                              device="cpu")
    assert vol.dims == S["dims"]
    vol.tsdf.copy_(torch.from_numpy(tsdf)), vol.weight.copy_(torch.from_numpy(weight)), vol.rgb.copy_(torch.from_numpy(rgb))
    view = vol.raycast(v["pixtocam"], v["camtoworld"], 40, 24)
    out = [view[k].numpy() for k in NAMES]
    assert_same_view(out, RC.truth("fused-view0"), "view 0 of the fused scene")
    depth, normals, col, acc = out
    D = v["depth"]
    with np.errstate(invalid="ignore"):
        both = np.isfinite(D) & (D > 0) & (v["acc"] >= 0.5) & (acc > 0)
    assert both.sum() >= 15
    err = np.abs(depth - D)[both].max()
    print(f"round trip: {int(both.sum())} pixels, worst |depth - fused depth| = {err:.9g} (recorded {ROUND_TRIP_MEASURED}), voxel {S['h']}")
    assert err <= 2 * ROUND_TRIP_MEASURED < S["h"] * 2
    # and the ray-cast depth is what integrate consumes: fusing it back updates voxels and leaves the volume finite
    before = vol.weight.clone()
    vol.integrate(view["depth"], v["pixtocam"], v["camtoworld"], rgb=view["rgb"], acc=view["acc"])
    assert bool((vol.weight > before).any()) and bool(torch.isfinite(vol.tsdf).all())


class SphereViews:
    """a synthetic dataset: two views of the sphere fixture with analytic normals, alphas and depths"""

    def __init__(self, device="cpu"):
        self.width, self.height, self.size = 40, 24, 2
        p2c = TC.pixtocam(40, 24, 30.0)
        c2w = np.stack([TC.look_at((2.4, 1.9, 2.2), TC.SPHERE["centre"]), TC.look_at((-1.2, 2.0, 1.5), TC.SPHERE["centre"])])
        self.cameras = (p2c, c2w, None, None)
        normals, alphas, self.renderings = [], [], []
        for m in c2w:
            _, _, ta, X, cos, _ = _sphere_analytic(dict(pixtocam=p2c, camtoworld=m, size=(40, 24)))
            seen = np.isfinite(ta)
            normals.append(np.where(seen[..., None], (X - np.asarray(TC.SPHERE["centre"])) / TC.SPHERE["r"], 0.0))
            alphas.append(seen.astype(np.float32))
            self.renderings.append(dict(acc=torch.from_numpy(alphas[-1]).to(device),
                                        distance_median=torch.from_numpy(np.nan_to_num(ta).astype(np.float32)).to(device)))
        self.normal_images = torch.from_numpy(np.stack(normals).astype(np.float32)).to(device)
        self.alphas = torch.from_numpy(np.stack(alphas)).to(device)


def sphere_volume_object(device, color=True):
    dims, origin, h, tsdf, weight, rgb = TC.sphere_volume()
    vol = geometry.TSDFVolume(origin, (np.asarray(dims) - 1) * h, voxel_size=h, color=color, device=device)
    assert vol.dims == dims
    vol.tsdf.copy_(torch.from_numpy(tsdf)), vol.weight.copy_(torch.from_numpy(weight))
    if color:
        vol.rgb.copy_(torch.from_numpy(rgb))
    return vol


def test_cpu_volume_raycast_views_and_metrics():
    c = RC.case("sphere")
    vol = sphere_volume_object("cpu")
    out = vol.raycast(c["pixtocam"], c["camtoworld"], 40, 24)
    assert sorted(out) == ["acc", "depth", "normals", "rgb"] and all(t.dtype == torch.float32 and t.device.type == "cpu" for t in out.values())
    assert_same_view([out[k].numpy() for k in NAMES], RC.truth("sphere"), "TSDFVolume.raycast")
    four = np.concatenate([c["camtoworld"], [[0, 0, 0, 1]]]).astype(np.float32)
    out = vol.raycast(torch.from_numpy(c["pixtocam"]), torch.from_numpy(four), 40, 24, refine=0, step=1.75)
    assert_same_view([out[k].numpy() for k in NAMES], RC.truth("sphere", True, 0, 1.75), "TSDFVolume.raycast, [4,4] pose")
    plain = sphere_volume_object("cpu", color=False).raycast(c["pixtocam"], c["camtoworld"], 40, 24)
    assert sorted(plain) == ["acc", "depth", "normals"] and torch.equal(plain["depth"], vol.raycast(c["pixtocam"], c["camtoworld"], 40, 24)["depth"])
    # views of a dataset, and of the reference's camera tuple
    data = SphereViews()
    view = vol.raycast_view(data, 0)
    assert_same_view([view[k].numpy() for k in NAMES], RC.truth("sphere"), "raycast_view(dataset)")
    tup = vol.raycast_view(data.cameras, 1, width=40, height=24)
    assert torch.equal(tup["depth"], vol.raycast_view(data, 1)["depth"]) and tup["acc"].sum() > 50
    assert tuple(vol.raycast_view(data, 1, width=13, height=11)["depth"].shape) == (11, 13)
    tensors = (torch.from_numpy(data.cameras[0]), torch.from_numpy(data.cameras[1]).double(), None, None)       # stacks as tensors
    assert torch.equal(vol.raycast_view(tensors, 1, width=40, height=24)["depth"], tup["depth"])
    with pytest.raises(ValueError, match="width= and height="):
        vol.raycast_view(data.cameras, 0)
    # the scores
    m = geometry.surface_metrics(vol, data, renderings=data.renderings)
    assert sorted(m) == ["coverage", "depth_l1", "normals_mae", "views"] and sorted(m["views"]) == [0, 1]
    for idx in (0, 1):
        v = vol.raycast_view(data, idx)
        acc, n, gt = v["acc"].double().numpy(), v["normals"].double().numpy(), data.normal_images[idx].double().numpy()
        w = acc * data.alphas[idx].double().numpy()
        eps = float(np.finfo(np.float32).eps)
        mae = (w * np.arccos(np.clip((n * gt).sum(-1), -1 + eps, 1 - eps))).sum() / w.sum() * 180 / np.pi
        both = (acc >= 0.5) & (data.alphas[idx].numpy() >= 0.5)
        l1 = np.abs(v["depth"].double().numpy() - data.renderings[idx]["distance_median"].double().numpy())[both].mean()
        got = m["views"][idx]
        assert abs(got["normals_mae"] - mae) <= 1e-9 * mae and abs(got["depth_l1"] - l1) <= 1e-12 * l1 and got["coverage"] == acc.mean()
        assert 0 < got["normals_mae"] < 30 and 0 < got["depth_l1"] < TC.SPHERE["h"] and 0 < got["coverage"] < 1
    for k in ("coverage", "depth_l1", "normals_mae"):
        assert m[k] == np.mean([m["views"][i][k] for i in (0, 1)])
    only = geometry.surface_metrics(vol, data, indices=[1], step=1.0)
    assert sorted(only) == ["coverage", "normals_mae", "views"] and list(only["views"]) == [1]
    bare = geometry.surface_metrics(vol, bare_dataset(data))
    assert sorted(bare) == ["coverage", "views"]


def bare_dataset(data):
    class Bare:
        cameras, width, height, size = data.cameras, data.width, data.height, data.size
    return Bare()


def test_cpu_volume_refuses_bad_arguments_and_cameras():
    c = RC.case("sphere")
    vol = sphere_volume_object("cpu")
    p2c, c2w = c["pixtocam"], c["camtoworld"]
    for kw in (dict(step=0.0), dict(step=1 / 128), dict(step=65.0), dict(step=float("nan")), dict(refine=-1), dict(refine=33), dict(refine=1.5),
               dict(near=-0.1), dict(near=float("nan")), dict(far=float("nan")), dict(iso=float("inf")), dict(min_weight=float("nan"))):
        with pytest.raises(ValueError, match="TSDFVolume.raycast"):
            vol.raycast(p2c, c2w, 40, 24, **kw)
    for args in ((p2c[:2], c2w, 40, 24), (p2c, c2w[:2], 40, 24), (p2c, c2w[:, :3], 40, 24), (p2c, c2w, 0, 24), (p2c, c2w, 40, -1), (p2c, c2w, 40.5, 24)):
        with pytest.raises(ValueError, match="TSDFVolume.raycast"):
            vol.raycast(*args)
    assert vol.raycast(p2c, c2w, 40, 24, step=64.0, refine=32, far=float("inf"))["acc"].shape == (24, 40)
    poses = c2w[None]
    with pytest.raises(ValueError, match="NDC"):
        vol.raycast_view((p2c, poses, None, p2c), 0, width=40, height=24)
    with pytest.raises(ValueError, match="distortion"):
        vol.raycast_view((p2c, poses, dict(k1=0.1), None), 0, width=40, height=24)

    class Pano:
        cameras, spherical, width, height = (p2c, poses, None, None), True, 40, 24
    with pytest.raises(ValueError, match="spherical"):
        vol.raycast_view(Pano(), 0)
    with pytest.raises(ValueError, match="cameras"):
        vol.raycast_view((p2c, poses), 0, width=40, height=24)


def test_surface_panels_are_written(tmp_path):
    from PIL import Image
    vol, data = sphere_volume_object("cpu"), SphereViews()
    written = geometry.write_surface_views(vol, data, str(tmp_path / "panels"), indices=[1])
    assert [os.path.basename(p) for p in written] == ["surface_normals_001.png", "surface_depth_001.png"]
    assert sorted(os.listdir(tmp_path / "panels")) == ["surface_depth_001.png", "surface_normals_001.png"]
    view = vol.raycast_view(data, 1)
    hit = view["acc"].numpy() > 0
    normals, panel = np.array(Image.open(written[0])), np.array(Image.open(written[1]))
    assert normals.shape == (24, 40, 3) and panel.shape == (24, 40) and normals.dtype == panel.dtype == np.uint8
    assert not normals[~hit].any() and not panel[~hit].any() and panel[hit].max() == 255
    want = ((view["normals"].numpy() / 2 + 0.5) * 255).astype(np.uint8)
    assert np.array_equal(normals[hit], want[hit])
    nearest = np.unravel_index(np.where(hit, view["depth"].numpy(), np.inf).argmin(), hit.shape)
    assert panel[nearest] == 255                                   # near is bright


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


@functools.lru_cache(maxsize=None)
def three_poses():
    """the fused scene's three cameras as one camtoworlds stack: `inside-the-grid` is its frame 1, `narrow` its frame 2"""
    return np.stack([v["camtoworld"] for v in TC.fused_volume()[0]["views"]])


@pytest.mark.gpu
@pytest.mark.parametrize("colour,refine,step", RC.SWEEP, ids=[f"{'rgb' if c else 'plain'}-refine{r}-step{s}" for c, r, s in RC.SWEEP])
@pytest.mark.parametrize("name", list(RC.CASES))
def test_hip_raycast_is_the_mirror_bit_for_bit(name, colour, refine, step):
    _hip.require_device()
    c = RC.case(name)
    want = RC.truth(name, colour, refine, step)
    grid = _hip.tsdf_grid(c["dims"], c["origin"], c["h"], 4 * c["h"])
    frame = {"inside-the-grid": 1, "narrow": 2}.get(name, 0)
    poses = three_poses() if frame else c["camtoworld"][None]
    assert np.array_equal(poses[frame], c["camtoworld"])
    got = _hip_guard(_hip.tsdf_raycast, grid, T(c["tsdf"]), T(c["weight"]), T(c["rgb"]) if colour else None, T(c["pixtocam"]), T(poses), frame,
                     *c["size"], 0.0, 1.0, step, refine)
    assert_same_view([None if g is None else g.cpu().numpy() for g in got], want, name)


@pytest.mark.gpu
def test_hip_raycast_near_far_and_iso_are_the_mirror_bit_for_bit():
    _hip.require_device()
    c = RC.case("sphere")
    grid = _hip.tsdf_grid(c["dims"], c["origin"], c["h"], 4 * c["h"])
    dev = [T(c[k]) for k in ("tsdf", "weight", "rgb", "pixtocam")] + [T(c["camtoworld"][None])]
    for kw in (dict(t_near=3.0, t_far=2.0), dict(t_near=3.2), dict(t_far=3.2), dict(iso=0.1, min_weight=0.5), dict(t_near=float("inf"))):
        want = RC.truth("sphere", True, 4, 0.5, **kw)
        got = _hip_guard(_hip.tsdf_raycast, grid, *dev, 0, 40, 24, kw.get("iso", 0.0), kw.get("min_weight", 1.0), 0.5, 4, kw.get("t_near", 0.0),
                         kw.get("t_far", float("inf")))
        assert_same_view([g.cpu().numpy() for g in got], want, str(kw))


@pytest.mark.gpu
def test_hip_raycast_argument_checks():
    _hip.require_device()
    lib, EINVAL = _hip.lib(), _hip.EINVAL
    c = RC.case("9x6x5-13x11")
    good = _hip.tsdf_grid(c["dims"], c["origin"], c["h"], 0.5)
    tsdf, weight, rgb, p2c, c2w = T(c["tsdf"]), T(c["weight"]), T(c["rgb"]), T(c["pixtocam"]), T(c["camtoworld"][None])
    outs = [torch.full(s, -7.0, device=DEV) for s in ((11, 13), (11, 13, 3), (11, 13, 3), (11, 13))]
    nan, inf = float("nan"), float("inf")

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def cast(grid=good, tsdf=tsdf, weight=weight, rgb=rgb, p2c=p2c, c2w=c2w, n_frames=1, frame=0, W=13, H=11, iso=0.0, mw=1.0, step=0.5, refine=4,
             near=0.0, far=inf, depth=outs[0], normals=outs[1], vrgb=outs[2], acc=outs[3]):
        return lib.refnerf_tsdf_raycast(C.byref(grid) if grid is not None else None, p(tsdf), p(weight), p(rgb), p(p2c), p(c2w), n_frames, frame,
                                        W, H, iso, mw, step, refine, near, far, p(depth), p(normals), p(vrgb), p(acc), None)
    bad_grids = [_hip.tsdf_grid((1, 6, 5), c["origin"], c["h"], 0.5), _hip.tsdf_grid((1024, 1024, 293), c["origin"], c["h"], 0.5),
                 _hip.tsdf_grid(c["dims"], c["origin"], 0.0, 0.5), _hip.tsdf_grid(c["dims"], (nan, 0, 0), c["h"], 0.5)]
    calls = dict(grid_null=dict(grid=None), tsdf=dict(tsdf=None), weight=dict(weight=None), p2c=dict(p2c=None), c2w=dict(c2w=None),
                 depth=dict(depth=None), normals=dict(normals=None), acc=dict(acc=None), rgb_without=dict(rgb=None), W=dict(W=0), H=dict(H=-2),
                 H_grid=dict(H=16 * 65535 + 1), frame_high=dict(frame=1), frame_low=dict(frame=-1), n_frames=dict(n_frames=0), iso=dict(iso=nan),
                 mw=dict(mw=inf), step_nan=dict(step=nan), step_inf=dict(step=inf), step_low=dict(step=1 / 128), step_zero=dict(step=0.0),
                 step_high=dict(step=64.5), refine_low=dict(refine=-1), refine_high=dict(refine=33), near_neg=dict(near=-0.5),
                 near_nan=dict(near=nan), far_nan=dict(far=nan), **{f"grid{n}": dict(grid=g) for n, g in enumerate(bad_grids)})
    for what, kw in calls.items():
        assert cast(**kw) == EINVAL, what
        assert b"refnerf_tsdf_raycast" in lib.refnerf_last_error(), what
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)                            # a refused call launches nothing
    assert cast(step=1 / 64, refine=0) == 0 and cast(step=64.0, refine=32, near=5.0, far=1.0) == 0 and cast(rgb=None, vrgb=None) == 0
    assert cast(vrgb=None) == 0                                                  # colour in the volume, none asked for
    torch.cuda.synchronize()
    assert not any(bool((o == -7.0).any()) for o in (outs[0], outs[1], outs[3]))
    # the wrapper raises ValueError before the library is reached
    for bad in (dict(tsdf=tsdf.double()), dict(weight=weight[:-1]), dict(rgb=rgb.cpu()), dict(p2c=p2c[:2]), dict(c2w=c2w[0])):
        a = dict(tsdf=tsdf, weight=weight, rgb=rgb, p2c=p2c, c2w=c2w)
        a.update(bad)
        with pytest.raises(ValueError):
            _hip.tsdf_raycast(good, a["tsdf"], a["weight"], a["rgb"], a["p2c"], a["c2w"], 0, 13, 11)
    with pytest.raises(ValueError, match="step"):
        _hip.tsdf_raycast(good, tsdf, weight, rgb, p2c, c2w, 0, 13, 11, step=0.0)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_hip_volume_equals_the_cpu_volume():
    _hip.require_device()
    c = RC.case("sphere")
    cpu, dev = sphere_volume_object("cpu"), sphere_volume_object(DEV)
    for kw in (dict(), dict(step=1.75, refine=0, near=0.5, far=3.3, iso=0.05)):
        want = cpu.raycast(c["pixtocam"], c["camtoworld"], 40, 24, **kw)
        got = _hip_guard(dev.raycast, c["pixtocam"], c["camtoworld"], 40, 24, **kw)
        assert sorted(got) == sorted(want) and all(t.is_cuda for t in got.values())
        for k in want:
            assert_bit_equal(got[k].cpu().numpy(), want[k].numpy(), f"device volume {k} {kw}")
    plain = _hip_guard(sphere_volume_object(DEV, color=False).raycast, c["pixtocam"], c["camtoworld"], 40, 24)
    assert sorted(plain) == ["acc", "depth", "normals"] and torch.equal(plain["depth"].cpu(), cpu.raycast(c["pixtocam"], c["camtoworld"], 40, 24)["depth"])
    host_data, dev_data = SphereViews(), SphereViews(DEV)
    on_device = (T(host_data.cameras[0]), T(host_data.cameras[1]), None, None)            # camera stacks that live on the device
    view = _hip_guard(dev.raycast_view, on_device, 1, width=40, height=24)
    assert_bit_equal(view["depth"].cpu().numpy(), cpu.raycast_view(host_data, 1)["depth"].numpy(), "raycast_view of device cameras")
    want = geometry.surface_metrics(cpu, host_data, renderings=host_data.renderings)
    got = _hip_guard(geometry.surface_metrics, dev, dev_data, renderings=dev_data.renderings)
    flat = lambda m: {**{k: v for k, v in m.items() if k != "views"}, **{(i, k): v for i, r in m["views"].items() for k, v in r.items()}}   # noqa: E731
    want, got = flat(want), flat(got)
    assert want.keys() == got.keys()
    for k in want:
        print(k, got[k], want[k])
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])

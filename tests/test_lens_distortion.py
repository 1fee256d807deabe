"""Radial-tangential lens undistortion in the device ray generator (camera_utils.pixels_to_rays with
`distortion_params`, internal/camera_utils.py:409-493, 558-565) and in the training batcher.

Fixture: tests/golden/camera_distortion.npz (tests/golden/make_golden_lens.py), the reference's float64 output from
int64 pixels.  Bars: the ray generator's own, rtol=2e-6 / atol=2e-7 per element (test_hip_parity.py::
test_device_ray_generation), against the float64 reference.  `strong` runs in world space only: a float32 emulation of the
kernel reaches 1.11 of the bar on its NDC radii, every other case stays within 0.84.
"""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import refnerf_pl_amd  # noqa: F401
from helpers import load_golden

DEV = "cuda:0"
RTOL, ATOL = 2e-6, 2e-7
KEYS = ("origins", "directions", "viewdirs", "radii", "imageplane")
ZERO = dict(k1=0., k2=0., k3=0., k4=0., p1=0., p2=0.)


# ---------------------------------------------------------------- float64 restatement (reference semantics)

def undistort64(xd, yd, k1=0., k2=0., k3=0., k4=0., p1=0., p2=0., eps=1e-9, max_iterations=10):
    """camera_utils._radial_and_tangential_undistort + _compute_residual_and_jacobian (:409-493)."""
    x, y = xd.copy(), yd.copy()
    for _ in range(max_iterations):
        r = x * x + y * y
        d = 1.0 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        fx = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x) - xd
        fy = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y) - yd
        d_r = k1 + r * (2.0 * k2 + r * (3.0 * k3 + r * 4.0 * k4))
        d_x, d_y = 2.0 * x * d_r, 2.0 * y * d_r
        fx_x = d + d_x * x + 2.0 * p1 * y + 6.0 * p2 * x
        fx_y = d_y * x + 2.0 * p1 * x + 2.0 * p2 * y
        fy_x = d_x * y + 2.0 * p2 * y + 2.0 * p1 * x
        fy_y = d + d_y * y + 2.0 * p2 * x + 6.0 * p1 * y
        den = fy_x * fx_y - fx_x * fy_y
        ok = np.abs(den) > eps
        safe = np.where(ok, den, 1.0)
        x = x + np.where(ok, (fx * fy_y - fy * fx_y) / safe, 0.0)
        y = y + np.where(ok, (fy * fx_x - fx * fy_x) / safe, 0.0)
    return x, y


def rays64(px, py, pixtocams, camtoworlds, distortion, pixtocam_ndc=None):
    """camera_utils.pixels_to_rays (:502-614) with distortion_params and convert_to_ndc (:31-97), float64 from int64
    pixels (the float32 cameras are upcast, as in the reference).  pixtocams / camtoworlds: one camera or one per pixel."""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    pd = np.stack([np.stack([px + ox + .5, py + oy + .5, np.ones(px.shape)], -1) for ox, oy in ((0, 0), (1, 0), (0, 1))])
    cam = np.matmul(np.asarray(pixtocams, np.float64), pd[..., None])[..., 0]
    x, y = undistort64(cam[..., 0], cam[..., 1], **distortion)
    cam = np.stack([x, -y, -np.ones_like(x)], -1)                          # restack with ones, OpenCV -> OpenGL
    imageplane = cam[0, ..., :2]
    c2w = np.asarray(camtoworlds, np.float64)
    d, dx, dy = np.matmul(c2w[..., :3, :3], cam[..., None])[..., 0]
    origins = np.broadcast_to(np.asarray(camtoworlds)[..., :3, -1], d.shape)    # in the pose's dtype: the reference's
                                                                               # NDC shift adds `near` in float32
    viewdirs = d / np.linalg.norm(d, axis=-1, keepdims=True)
    if pixtocam_ndc is None:
        dxn, dyn = np.linalg.norm(dx - d, axis=-1), np.linalg.norm(dy - d, axis=-1)
    else:
        def to_ndc(o, v):
            t = -(1. + o[..., 2]) / v[..., 2]
            o = o + t[..., None] * v
            xm, ym = 1. / pixtocam_ndc[0, 2], 1. / pixtocam_ndc[1, 2]       # float32 scalars, as in the reference
            on = np.stack([xm * o[..., 0] / o[..., 2], ym * o[..., 1] / o[..., 2], -np.ones_like(o[..., 2])], -1)
            inf = np.stack([xm * v[..., 0] / v[..., 2], ym * v[..., 1] / v[..., 2], np.ones_like(o[..., 2])], -1)
            return on, inf - on
        o_dx, _ = to_ndc(origins, dx)
        o_dy, _ = to_ndc(origins, dy)
        origins, d = to_ndc(origins, d)
        dxn, dyn = np.linalg.norm(o_dx - origins, axis=-1), np.linalg.norm(o_dy - origins, axis=-1)
    radii = (0.5 * (dxn + dyn))[..., None] * 2 / np.sqrt(12)
    return np.asarray(origins, np.float64), d, viewdirs, radii, imageplane


def case_inputs(g, case):
    per = case + "_pixtocam_ndc"
    return (g[case + "_pix_x"], g[case + "_pix_y"], g[case + "_pixtocam"], g[case + "_camtoworld"],
            json.loads(str(g[case + "_distortion"])), g[per] if per in g.files else None)


def restated(g, case, distortion=None):
    px, py, p2c, c2w, dist, ndc = case_inputs(g, case)
    if case + "_cam_idx" in g.files:
        ci = g[case + "_cam_idx"][..., 0]
        p2c, c2w = p2c[ci], c2w[ci]
    return rays64(px, py, p2c, c2w, dist if distortion is None else distortion, ndc)


def assert_bars(got, want, tag):
    """The ray generator's bars per element, each field's worst ratio printed first."""
    for k, a, b in zip(KEYS, got, want):
        a = a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, np.float64)
        b = np.asarray(b, np.float64)
        assert a.shape == b.shape, (tag, k)
        ratio = float((np.abs(a - b) / (ATOL + RTOL * np.abs(b))).max())
        print(f"{tag} {k}: worst |err| / (atol + rtol |ref|) = {ratio:.3f}")
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, err_msg=f"{tag} {k}")


# ---------------------------------------------------------------- CPU

def test_restatement_reproduces_reference_fixture():
    g = load_golden("camera_distortion")
    assert len(g["cases"]) == 19
    for case in g["cases"]:
        case = str(case)
        for k, v in zip(KEYS, restated(g, case)):
            want = g[f"{case}_{k}"]
            assert want.dtype == np.float64 and v.shape == want.shape, (case, k)
            np.testing.assert_allclose(v, want, rtol=0, atol=1e-12, err_msg=f"{case} {k}")
        # distortion moves the rays far beyond the bars: a pinhole result cannot pass
        assert np.abs(restated(g, case, ZERO)[1] - g[case + "_directions"]).max() > 100 * ATOL, case


def test_batcher_keeps_distortion_on_cpu():
    from refnerf_pl_amd import datasets, utils
    g = load_golden("camera_distortion")
    p2c, c2w = g["llff_simple_radial_world_pixtocam"], g["llff_simple_radial_world_camtoworld"]
    imgs = np.random.default_rng(0).random((2, 12, 16, 3), dtype=np.float32)
    b = datasets.TrainRayBatcher(imgs, (p2c, np.stack([c2w, c2w]), {'k1': -0.08}, None), 2., 6., batch_size=32, device='cpu')
    assert b.cameras[2] == {'k1': -0.08}
    batch = b.next(cast_rays=False)
    assert isinstance(batch.rays, utils.Pixels) and tuple(batch.rgb.shape) == (32, 1, 1, 3)
    with pytest.raises(TypeError):
        datasets.TrainRayBatcher(imgs, (p2c, c2w, {'k1': -0.08, 'k5': 0.}, None), 2., 6., batch_size=32, device='cpu')


def test_unknown_distortion_key_and_fisheye_refused_on_cpu():
    from refnerf_pl_amd import camera_utils, utils
    g = load_golden("camera_distortion")
    px, py, p2c, c2w, _, _ = case_inputs(g, "llff_radial_world")
    with pytest.raises(TypeError):
        camera_utils.pixels_to_rays(px, py, p2c, c2w, distortion_params={'k9': 1.})
    n = px.shape[0]
    one = np.ones((n, 1), np.float32)
    pix = utils.Pixels(pix_x_int=px, pix_y_int=py, lossmult=one, near=one, far=one, cam_idx=np.zeros((n, 1), np.int32))
    with pytest.raises(TypeError):
        camera_utils.cast_ray_batch((p2c, c2w, {'k1': 0.1, 'k9': 1.}, None), pix)
    with pytest.raises(ValueError):
        camera_utils.pixels_to_rays(px, py, p2c, c2w, camtype=camera_utils.ProjectionType.FISHEYE)
    with pytest.raises(ValueError):
        camera_utils.pixels_to_rays(px, py, p2c, c2w, distortion_params={'k1': 0.1},
                                    camtype=camera_utils.ProjectionType.FISHEYE)
    # defaults are the reference's keyword defaults (:462-469)
    d = camera_utils.lens_distortion({'k2': 0.5})
    assert (d.k1, d.k2, d.k3, d.k4, d.p1, d.p2, d.eps, d.max_iterations) == (0., 0.5, 0., 0., 0., 0., 1e-9, 10)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def hip():
    from refnerf_pl_amd import _hip
    _hip.require_device()
    return _hip


@pytest.mark.gpu
def test_device_undistortion_matches_reference(hip):
    from refnerf_pl_amd import camera_utils, utils
    g = load_golden("camera_distortion")
    dev = torch.device(DEV)
    for case in map(str, g["cases"]):
        px, py, p2c, c2w, dist, ndc = case_inputs(g, case)
        want = [g[f"{case}_{k}"] for k in KEYS]
        if case.startswith("multi"):
            ci = g[case + "_cam_idx"]
            n = px.shape[0]
            one = np.ones((n, 1), np.float32)
            pix = utils.Pixels(pix_x_int=px, pix_y_int=py, lossmult=one, near=one, far=one, cam_idx=ci)
            rays = camera_utils.cast_ray_batch((p2c, c2w, dist, None), pix, device=dev)
            assert_bars([rays.origins, rays.directions, rays.viewdirs, rays.radii, rays.imageplane], want, case)
            per = camera_utils.pixels_to_rays(px, py, p2c[ci[:, 0]], c2w[ci[:, 0]], distortion_params=dist, device=dev)
            for a, b in zip(per, (rays.origins, rays.directions, rays.viewdirs, rays.radii, rays.imageplane)):
                assert torch.equal(a, b), case
            continue
        res = camera_utils.pixels_to_rays(px, py, p2c, c2w, distortion_params=dist, pixtocam_ndc=ndc, device=dev)
        assert_bars(res, want, case)
        n = px.shape[0]
        per = camera_utils.pixels_to_rays(px, py, np.tile(p2c, (n, 1, 1)), np.tile(c2w, (n, 1, 1)), distortion_params=dist,
                                          pixtocam_ndc=ndc, device=dev)
        for a, b in zip(res, per):
            assert torch.equal(a, b), case
        # no distortion: Newton leaves x as it is, so the distorted kernel reproduces the pinhole kernel bit for bit
        assert np.array_equal(p2c[2], [0., 0., 1.])
        pin = camera_utils.pixels_to_rays(px, py, p2c, c2w, pixtocam_ndc=ndc, device=dev)
        for off in (dict(ZERO), dict(dist, max_iterations=0)):
            z = camera_utils.pixels_to_rays(px, py, p2c, c2w, distortion_params=off, pixtocam_ndc=ndc, device=dev)
            for a, b in zip(z, pin):
                assert torch.equal(a, b), (case, off)
        assert not torch.equal(res[1], pin[1]), case


GATED = [(d, s) for d in ("simple_radial", "radial", "opencv", "k3k4", "strong") for s in ("world", "ndc")
         if (d, s) != ("strong", "ndc")]      # strong + NDC: not a gated case (module docstring)


@pytest.mark.gpu
@pytest.mark.parametrize("dname,space", GATED)
def test_device_undistortion_full_raster(hip, dname, space):
    """Every pixel of the 1008x756 LLFF camera against the float64 restatement (pinned to the reference above)."""
    from refnerf_pl_amd import camera_utils
    g = load_golden("camera_distortion")
    _, _, p2c, c2w, dist, ndc = case_inputs(g, f"llff_{dname}_{space}")
    w, h = 1008, 756
    px, py = camera_utils.pixel_coordinates(w, h, torch.device(DEV))
    res = camera_utils.pixels_to_rays(px, py, p2c, c2w, distortion_params=dist, pixtocam_ndc=ndc, device=torch.device(DEV))
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert_bars(res, rays64(xx, yy, p2c, c2w, dist, ndc), f"raster llff_{dname}_{space}")


@pytest.mark.gpu
@pytest.mark.parametrize("space", ["world", "ndc"])
def test_batcher_casts_distorted_rays_on_device(hip, space):
    from refnerf_pl_amd import camera_utils, datasets
    g = load_golden("camera_distortion")
    if space == "world":                  # three cameras sharing one dict
        case = "multi_opencv_world"
        p2c, c2w, ndc = g[case + "_pixtocam"], g[case + "_camtoworld"], None
    else:
        case = "llff_radial_ndc"
        p2c, c2w, ndc = g[case + "_pixtocam"], np.stack([g[case + "_camtoworld"]] * 3), g[case + "_pixtocam_ndc"]
    dist = json.loads(str(g[case + "_distortion"]))
    imgs = torch.rand((3, 756, 1008, 3), device=DEV)
    mk = lambda: datasets.TrainRayBatcher(imgs, (p2c, c2w, dist, ndc), 0., 1., batch_size=4096, seed=3, device=DEV)  # noqa: E731
    b1, b2 = mk(), mk()
    assert b1.cameras[2] == dist
    pixels = b1.next(cast_rays=False).rays
    rays = b2.next().rays
    again = camera_utils.cast_ray_batch(b1.cameras, pixels, device=torch.device(DEV))
    fields = ("origins", "directions", "viewdirs", "radii", "imageplane")
    for k in fields:
        assert torch.equal(getattr(rays, k), getattr(again, k)), k
    ci = pixels.cam_idx[..., 0].long().cpu().numpy()
    p2c_r = p2c[ci] if p2c.ndim == 3 else p2c
    want = rays64(pixels.pix_x_int.cpu().numpy(), pixels.pix_y_int.cpu().numpy(), p2c_r, c2w[ci], dist, ndc)
    assert_bars([getattr(rays, k) for k in fields], want, f"batcher {space}")
    assert len(np.unique(ci)) == 3


@pytest.mark.gpu
def test_c_entry_refuses_bad_distortion(hip):
    L = hip.lib()
    n = 8
    i32 = torch.zeros(n, dtype=torch.int32, device=DEV)
    p2c = torch.eye(3, device=DEV)
    c2w = torch.eye(3, 4, device=DEV)
    outs = [torch.empty((n, 3), device=DEV) for _ in range(3)] + [torch.empty(n, device=DEV), torch.empty((n, 2), device=DEV)]

    def call(dist):
        return L.refnerf_pixels_to_rays_distorted(hip.ptr(i32), hip.ptr(i32), hip.ptr(p2c), 0, hip.ptr(c2w), 0, None, n,
                                                  *[hip.ptr(t) for t in outs], dist, hip.stream_ptr())
    good = hip.LensDistortion(-0.08, 0., 0., 0., 0., 0., 1e-9, 10)
    assert call(C.byref(good)) == 0
    torch.cuda.synchronize()
    assert call(None) == -1                       # REFNERF_EINVAL
    for field, value in (("k1", math.nan), ("p2", math.inf), ("eps", math.nan), ("max_iterations", 65), ("max_iterations", -1)):
        bad = hip.LensDistortion(-0.08, 0., 0., 0., 0., 0., 1e-9, 10)
        setattr(bad, field, value)
        assert call(C.byref(bad)) == -1, field
    bad = hip.LensDistortion(-0.08, 0., 0., 0., 0., 0., 1e-9, 64)
    assert call(C.byref(bad)) == 0
    torch.cuda.synchronize()

"""refnerf_image_rays: all nine `Rays` fields of a frame (or of a flat pixel range of it) in one launch, from
(width, height, camera, pose) -- camera_utils.cast_image_rays / cast_spherical_rays, datasets.PathCameras and
models.render_path on the device.

Pinhole truth: the existing entries (refnerf_pixels_to_rays / _distorted) on pixel_coordinates(W, H) -- bit-equal, the
library being built with -ffp-contract=off.  Spherical truth: the reference's float64 cast_spherical_rays
(tests/golden/camera_paths.npz) at the ray generator's bars, rtol=2e-6 / atol=2e-7.

Shapes: (W, H) = (13, 7) and (67, 5); the second has 335 pixels -- more than one 256-thread block, rows coprime to the
wavefront.  The range 60 .. 270 of it starts mid-row, crosses row boundaries and the block boundary.
"""
import json
import os

import numpy as np
import pytest
import torch

import refnerf_pl_amd  # noqa: F401
from helpers import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 2e-6, 2e-7
RAY_KEYS = ("origins", "directions", "viewdirs", "radii", "imageplane")
ALL_KEYS = RAY_KEYS + ("lossmult", "near", "far", "cam_idx")
SIZES = ((13, 7), (67, 5))        # (W, H)
NEAR, FAR = 0.25, 7.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from refnerf_pl_amd import _hip
    _hip.require_device()
    return _hip


def three_pose_path(c2w):
    """The fixture's pose and two near it (a small rotation about z, a shifted position), float32 [3,3,4]."""
    out = []
    for k in range(3):
        a = 0.05 * k
        rz = np.array([[np.cos(a), -np.sin(a), 0.], [np.sin(a), np.cos(a), 0.], [0., 0., 1.]])
        out.append(np.concatenate([rz @ c2w[:, :3].astype(np.float64), c2w[:, 3:] + k * np.array([[0.03], [-0.02], [0.01]])], -1))
    return np.stack(out).astype(np.float32)


def mode_cameras(mode):
    """(pixtocam [3,3], camtoworlds [3,3,4], distortion dict | None, pixtocam_ndc | None): the reference's cameras tuple."""
    if mode == "opencv":
        g, tag = load_golden("camera_distortion"), "llff_opencv_world"
        return g[tag + "_pixtocam"], three_pose_path(g[tag + "_camtoworld"]), json.loads(str(g[tag + "_distortion"])), None
    g, tag = load_golden("camera"), "llff" if mode == "ndc" else "blender"
    return g[tag + "_pixtocam"], three_pose_path(g[tag + "_camtoworld"]), None, g[tag + "_pixtocam"] if mode == "ndc" else None


@pytest.fixture(scope="module")
def frames(hip):
    """cast_image_rays of frame 2 of the 3-pose path, and the existing entry on the same pixels with pose 2 alone; computed
    once per (mode, size) and shared, unchanged, by the tests below."""
    from refnerf_pl_amd import camera_utils
    dev, out = torch.device(DEV), {}
    for mode in ("world", "ndc", "opencv"):
        p2c, c2ws, dist, ndc = mode_cameras(mode)
        for (w, h) in SIZES:
            rays = camera_utils.cast_image_rays((p2c, c2ws, dist, ndc), 2, h, w, NEAR, FAR, device=dev)
            px, py = camera_utils.pixel_coordinates(w, h, dev)
            want = camera_utils.pixels_to_rays(px, py, p2c, c2ws[2], distortion_params=dist, pixtocam_ndc=ndc, device=dev)
            out[mode, w, h] = (rays, dict(zip(RAY_KEYS, want)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("mode", ["world", "ndc", "opencv"])
def test_pinhole_equals_the_existing_entry(hip, frames, mode, w, h):
    from refnerf_pl_amd import camera_utils
    rays, want = frames[mode, w, h]
    for k in RAY_KEYS:
        got = getattr(rays, k)
        assert got.shape == want[k].shape == (h, w, want[k].shape[-1]) and got.dtype == torch.float32, k
        assert torch.equal(got, want[k]), (mode, k, float((got - want[k]).abs().max()))
    assert rays.lossmult.shape == rays.near.shape == rays.far.shape == rays.cam_idx.shape == (h, w, 1)
    assert bool((rays.lossmult == 1).all()) and bool((rays.near == NEAR).all()) and bool((rays.far == FAR).all())
    assert rays.cam_idx.dtype == torch.int32 and bool((rays.cam_idx == 2).all())
    # frame 2 reads pose 2 of the path: a path that holds that pose alone gives the same rays, and pose 0 does not
    p2c, c2ws, dist, ndc = mode_cameras(mode)
    single = camera_utils.cast_image_rays((p2c, c2ws[2:], dist, ndc), 0, h, w, NEAR, FAR, device=torch.device(DEV))
    first = camera_utils.cast_image_rays((p2c, c2ws, dist, ndc), 0, h, w, NEAR, FAR, device=torch.device(DEV))
    for k in RAY_KEYS:
        assert torch.equal(getattr(single, k), getattr(rays, k)), k
    assert bool((single.cam_idx == 0).all()) and not torch.equal(first.directions, rays.directions)


@pytest.mark.parametrize("mode", ["world", "ndc", "opencv"])
def test_pixel_range(hip, frames, mode):
    from refnerf_pl_amd import camera_utils
    w, h = SIZES[1]
    full, _ = frames[mode, w, h]
    cams, dev = mode_cameras(mode), torch.device(DEV)
    part = camera_utils.cast_image_rays(cams, 2, h, w, NEAR, FAR, first=60, count=210, device=dev)
    last = camera_utils.cast_image_rays(cams, 2, h, w, NEAR, FAR, first=w * h - 1, count=1, device=dev)
    whole = camera_utils.cast_image_rays(cams, 2, h, w, NEAR, FAR, first=0, count=w * h, device=dev)
    for k in ALL_KEYS:
        flat = getattr(full, k).reshape(w * h, -1)
        assert getattr(part, k).shape == (210, flat.shape[1]) and torch.equal(getattr(part, k), flat[60:270]), k
        assert getattr(last, k).shape == (1, flat.shape[1]) and torch.equal(getattr(last, k), flat[-1:]), k
        assert getattr(whole, k).shape == flat.shape and torch.equal(getattr(whole, k), flat), k


@pytest.mark.parametrize("case", ["pano_6x8", "pano_9x37"])
def test_spherical_against_reference(hip, case):
    from refnerf_pl_amd import camera_utils
    g = load_golden("camera_paths")
    h, w = int(g[case + "_height"]), int(g[case + "_width"])
    c2w, near, far = g[case + "_camtoworld"], float(g[case + "_near"][0, 0, 0]), float(g[case + "_far"][0, 0, 0])
    rays = camera_utils.cast_spherical_rays(c2w, h, w, near, far, device=torch.device(DEV))
    for k in ALL_KEYS:
        got, want = getattr(rays, k).cpu().numpy(), g[f"{case}_{k}"]
        assert got.shape == want.shape, (k, got.shape, want.shape)
        print(f"{case} {k}: worst error / bar {(np.abs(got - want) / (ATOL + RTOL * np.abs(want))).max():.3f}")
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=f"{case} {k}")
    assert torch.equal(rays.viewdirs, rays.directions)
    assert bool((rays.imageplane == 0).all()) and bool((rays.cam_idx == 0).all()) and rays.cam_idx.dtype == torch.int32
    assert bool((rays.lossmult == 1).all()) and bool((rays.near == np.float32(near)).all()) and bool((rays.far == np.float32(far)).all())
    pole = rays.radii[0].cpu().numpy()                  # row 0: phi = 0, every node is the pole, dx = 0
    assert np.isfinite(pole).all() and (pole > 0).all()
    np.testing.assert_allclose(pole, g[case + "_radii"][0], rtol=RTOL, atol=ATOL)
    # through the cameras tuple: frame 1 of a path is its pose, cam_idx stays 0, and a range is rows of the frame
    path = np.stack([three_pose_path(c2w)[1], c2w])
    again = camera_utils.cast_image_rays((None, path, None, None), 1, h, w, near, far, spherical=True, device=torch.device(DEV))
    part = camera_utils.cast_image_rays((None, path, None, None), 1, h, w, near, far, spherical=True, first=w - 3, count=w + 5,
                                        device=torch.device(DEV))
    for k in ALL_KEYS:
        assert torch.equal(getattr(again, k), getattr(rays, k)), k
        assert torch.equal(getattr(part, k), getattr(rays, k).reshape(w * h, -1)[w - 3:2 * w + 2]), k


def test_errors_are_host_side(hip):
    """Every refusal is REFNERF_EINVAL from the entry's own checks -- ValueError here -- before anything is launched."""
    from refnerf_pl_amd import camera_utils
    dev = torch.device(DEV)
    p2c, c2ws, _, _ = mode_cameras("world")
    p2c_d, c2w_d = torch.as_tensor(p2c, device=dev), torch.as_tensor(c2ws, device=dev)
    w, h = 13, 7
    assert hip.image_rays(hip.PROJ_PINHOLE, w, h, p2c_d, c2w_d, 2, NEAR, FAR)["origins"].shape == (w * h, 3)
    for frame in (3, -1):
        with pytest.raises(ValueError, match="frame"):
            hip.image_rays(hip.PROJ_PINHOLE, w, h, p2c_d, c2w_d, frame, NEAR, FAR)
    for first, count in ((0, w * h + 1), (w * h - 1, 2), (w * h, 1), (-1, 2)):
        with pytest.raises(ValueError, match="outside the image"):
            hip.image_rays(hip.PROJ_PINHOLE, w, h, p2c_d, c2w_d, 0, NEAR, FAR, first=first, count=count)
    with pytest.raises(ValueError, match="positive"):
        hip.image_rays(hip.PROJ_PINHOLE, w, h, p2c_d, c2w_d, 0, NEAR, FAR, first=0, count=0)
    with pytest.raises(ValueError, match="positive"):
        hip.image_rays(hip.PROJ_PINHOLE, 0, h, p2c_d, c2w_d, 0, NEAR, FAR, first=0, count=1)
    with pytest.raises(ValueError, match="projection"):
        hip.image_rays(2, w, h, p2c_d, c2w_d, 0, NEAR, FAR)
    with pytest.raises(ValueError, match="null"):
        hip.image_rays(hip.PROJ_PINHOLE, w, h, None, c2w_d, 0, NEAR, FAR)
    with pytest.raises(ValueError, match="spherical"):
        hip.image_rays(hip.PROJ_SPHERICAL, w, h, None, c2w_d, 0, NEAR, FAR, pixtocam_ndc=p2c_d)
    with pytest.raises(ValueError, match="spherical"):
        hip.image_rays(hip.PROJ_SPHERICAL, w, h, None, c2w_d, 0, NEAR, FAR, distortion=camera_utils.lens_distortion(dict(k1=-.1)))
    with pytest.raises(ValueError, match="spherical"):
        camera_utils.cast_image_rays((p2c, c2ws, None, p2c), 0, h, w, NEAR, FAR, spherical=True, device=dev)
    with pytest.raises(ValueError, match="spherical"):
        camera_utils.cast_image_rays((p2c, c2ws, dict(k1=-.1), None), 0, h, w, NEAR, FAR, spherical=True, device=dev)
    # the distorted entry's own checks
    with pytest.raises(ValueError, match="max_iterations"):
        hip.image_rays(hip.PROJ_PINHOLE, w, h, p2c_d, c2w_d, 0, NEAR, FAR, distortion=hip.LensDistortion(0., 0., 0., 0., 0., 0., 1e-9, 65))
    with pytest.raises(ValueError, match="non-finite"):
        hip.image_rays(hip.PROJ_PINHOLE, w, h, p2c_d, c2w_d, 0, NEAR, FAR,
                       distortion=hip.LensDistortion(float("nan"), 0., 0., 0., 0., 0., 1e-9, 10))
    with pytest.raises(TypeError):
        camera_utils.cast_image_rays((p2c, c2ws, dict(k9=1.), None), 0, h, w, NEAR, FAR, device=dev)
    torch.cuda.synchronize()


def test_render_path_end_to_end(hip, tmp_path):
    """PathCameras.from_config (3-frame forward-facing spiral, 16 x 12, NDC) -> models.render_path -> artefacts; frame 1's
    rgb is bit-equal to render_image on cast_ray_batch rays of the same pose: the rays are bit-equal (above) and the
    eval kernels are deterministic."""
    from refnerf_pl_amd import camera_utils, configs, datasets, models, synthetic, utils
    dev = torch.device(DEV)
    g = load_golden("camera_paths")
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "refnerf_llff.gin")],
                                            ["Model.num_prop_samples = 64", "Model.num_nerf_samples = 64", "Config.forward_facing = True",
                                             "Config.render_path = True", "Config.render_path_frames = 3", "Config.render_chunk_size = 80"])
    cfg = configs.Config()
    model = models.construct_model(None, cfg).to(dev).eval()
    model.nerf_mlp.load_flat_params(synthetic.make_params(seed=0, bias_scale=0.05, sharpen=20.0))
    w, h = 16, 12
    cams = datasets.PathCameras.from_config(cfg, g["forward_poses"], g["forward_bounds"], focal=20., height=h, width=w,
                                            near=cfg.near, far=cfg.far, device=dev)
    assert cams.size == 3 and cams.cameras[3] is not None

    def render_fn(rays):
        return model(rays, 1.0, True)
    done = dict(models.render_path(render_fn, cams, cfg, out_dir=str(tmp_path)))
    assert sorted(done) == [0, 1, 2] and done[1]["rgb"].shape == (h, w, 3)
    names = ("color_{}.png", "diffuse_{}.png", "specular_{}.png", "normals_pred_{}.png", "rho_{}.png", "distance_mean_{}.tiff",
             "distance_median_{}.tiff", "acc_{}.tiff")
    assert sorted(os.listdir(tmp_path)) == sorted(n.format(f"{i:03d}") for n in names for i in range(3))

    px, py = camera_utils.pixel_coordinates(w, h, dev)

    def scalar(x, dtype=torch.float32):
        return torch.full((h, w, 1), x, dtype=dtype, device=dev)
    pixels = utils.Pixels(pix_x_int=px, pix_y_int=py, lossmult=scalar(1.), near=scalar(cfg.near), far=scalar(cfg.far),
                          cam_idx=scalar(1, torch.int32))
    rays = camera_utils.cast_ray_batch(cams.cameras, pixels, device=dev)
    mine = cams.generate_ray_batch(1).rays
    for k in ALL_KEYS:
        assert torch.equal(getattr(mine, k), getattr(rays, k)), k
    with torch.no_grad():
        want = models.render_image(render_fn, rays, cfg, verbose=False, device=dev)
    assert torch.isfinite(done[1]["rgb"]).all() and float(done[1]["rgb"].std()) > 0
    assert torch.equal(done[1]["rgb"], want["rgb"])
    assert not torch.equal(done[0]["rgb"], done[1]["rgb"])
    assert [b.rays.origins.shape for b in cams] == [(h, w, 3)] * 3          # iteration: one Batch per view

"""Render-path cameras on the host: the pose / path functions of camera_utils (internal/camera_utils.py:100-377), the
general stepfun.sample they need, datasets.PathCameras.from_config, a float64 emulation of the spherical ray kernel, and
the loop of models.render_path.  No device.

Fixture: tests/golden/camera_paths.npz (tests/golden/make_golden_paths.py): the reference's float64 outputs on a seeded
set of 12 inward-facing and one of 10 forward-facing poses.

Bars of the path functions.  They are the same float64 numpy / scipy operations on O(1) numbers as the reference's, so
the measured maximum absolute differences against the fixture (MEASURED below, printed by every test before it asserts) are all 0: the
restatements keep the reference's operation order and the same LAPACK / FITPACK routines see the same bits.  A measured
0 means "below one unit in the last place", so each bar is 10 units in the last place of the fixture's largest element
(10 * 2.2e-16 * max|want|, about 1e-14 here) -- ten times the resolution of the measurement -- and in no case above 1e-9:
anything larger is a formula difference, not rounding.
"""
import os

import numpy as np
import pytest
import torch

import refnerf_pl_amd  # noqa: F401
from helpers import load_golden
from refnerf_pl_amd import camera_utils, configs, datasets, models, stepfun, utils

RTOL, ATOL = 2e-6, 2e-7          # the ray generator's bars (test_hip_parity.py::test_device_ray_generation, test_lens_distortion.py)

# max |ours - reference| per function on the fixture's cases, as measured when the fixture was written
MEASURED = dict(
    recenter_poses=0., transform_poses_pca=0., focus_point_fn=0., generate_spiral_path=0., generate_ellipse_path=0.,
    generate_ellipse_path_wave=0., generate_interpolated_path=0., interpolate_1d=0., create_render_spline_path=0.,
    stepfun_sample=0., recentred_average_pose=9.1e-16, from_config_forward_facing=0., from_config_ellipse=0., from_config_spline=0.)


@pytest.fixture(scope="module")
def g():
    return load_golden("camera_paths")


def close(name, got, want):
    """Print the measured difference, then assert it at 10 x MEASURED[name] (floor: 10 ulp of the largest element; cap 1e-9)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (name, got.shape, want.shape, got.dtype)
    diff = float(np.abs(got - want).max())
    bar = min(max(10 * MEASURED[name], 10 * np.finfo(np.float64).eps * float(np.abs(want).max())), 1e-9)
    print(f"{name}: max abs diff {diff:.3e} (bar {bar:.3e})")
    assert diff <= bar, (name, diff, bar)


def spline_config(g, tmp_path, **kw):
    keyframes = tmp_path / "keyframes.txt"
    keyframes.write_text("\n".join(str(n) for n in g["spline_keyframes"]) + "\n")
    return configs.Config(render_spline_keyframes=str(keyframes), render_spline_n_interp=int(g["spline_n_interp"]),
                          render_spline_degree=int(g["spline_degree"]), render_spline_smoothness=float(g["spline_smoothness"]), **kw)


# ---------------------------------------------------------------- path functions against the reference

def test_constants_and_padding():
    assert (camera_utils.NEAR_STRETCH, camera_utils.FAR_STRETCH, camera_utils.FOCUS_DISTANCE) == (.9, 5., .75)
    p = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    padded = camera_utils.pad_poses(p)
    assert padded.shape == (2, 4, 4) and np.array_equal(padded[:, 3], np.tile([0, 0, 0, 1.], (2, 1)))
    assert np.array_equal(camera_utils.unpad_poses(padded), p)
    assert np.array_equal(camera_utils.normalize(np.array([3., 0., 4.])), [.6, 0., .8])
    m = camera_utils.viewmatrix(np.array([0., 0., 2.]), np.array([0., 1., 0.]), np.array([1., 2., 3.]))
    assert np.array_equal(m, np.concatenate([np.eye(3), [[1.], [2.], [3.]]], -1))


@pytest.mark.parametrize("name", ["inward", "forward"])
def test_pose_normalisation(g, name):
    poses = g[name + "_poses"]
    got, transform = camera_utils.recenter_poses(poses.copy())
    close("recenter_poses", got, g[name + "_recenter_poses"])
    close("recenter_poses", transform, g[name + "_recenter_transform"])
    close("recentred_average_pose", camera_utils.average_pose(got), np.eye(4)[:3])       # a property, not a fixture: the identity
    got, transform = camera_utils.transform_poses_pca(poses.copy())
    close("transform_poses_pca", got, g[name + "_pca_poses"])
    close("transform_poses_pca", transform, g[name + "_pca_transform"])
    close("focus_point_fn", camera_utils.focus_point_fn(poses), g[name + "_focus_point"])


def test_spiral_path(g):
    got = camera_utils.generate_spiral_path(g["forward_poses"], g["forward_bounds"], n_frames=8)
    close("generate_spiral_path", got, g["forward_spiral"])
    assert camera_utils.generate_spiral_path(g["forward_poses"], g["forward_bounds"]).shape == (120, 3, 4)


def test_ellipse_path(g):
    close("generate_ellipse_path", camera_utils.generate_ellipse_path(g["inward_poses"], n_frames=8), g["inward_ellipse"])
    got = camera_utils.generate_ellipse_path(g["inward_poses"], n_frames=8, const_speed=False, z_variation=.5, z_phase=.25)
    close("generate_ellipse_path_wave", got, g["inward_ellipse_wave"])


def test_spline_paths(g, tmp_path):
    close("generate_interpolated_path", camera_utils.generate_interpolated_path(g["inward_poses"], 3), g["inward_interpolated"])
    close("interpolate_1d", camera_utils.interpolate_1d(g["interp1d_x"], 3, 3, 0.), g["interp1d_out"])
    ret = camera_utils.create_render_spline_path(spline_config(g, tmp_path), [str(n) for n in g["spline_image_names"]],
                                                 g["inward_poses"])
    assert isinstance(ret, tuple) and len(ret) == 2
    assert np.array_equal(ret[0], g["spline_indices"])
    close("create_render_spline_path", ret[1], g["spline_poses"])


def test_stepfun_sample_float64(g):
    t, logits, n = torch.tensor(g["sample_t"]), torch.tensor(g["sample_logits"]), int(g["sample_n"])
    for key, center in (("sample_out", False), ("sample_out_center", True)):
        got = stepfun.sample(t, logits, n, deterministic_center=center)
        assert got.dtype == torch.float64
        close("stepfun_sample", got.numpy(), g[key])
    w = torch.softmax(logits, -1)
    cw = stepfun.integrate_weights(w)
    assert cw.dtype == torch.float64 and cw.shape == (2, 9) and bool((cw[:, 0] == 0).all()) and bool((cw[:, -1] == 1).all())
    assert stepfun.integrate_weights(w.float()).dtype == torch.float32
    u = torch.tensor([[0., .25, .999], [.5, .75, 1.]], dtype=torch.float64)
    want = np.stack([np.interp(u[i].numpy(), cw[i].numpy(), g["sample_t"][i]) for i in range(2)])
    np.testing.assert_allclose(stepfun.invert_cdf(u, t, logits).numpy(), want, rtol=0, atol=1e-15)
    np.testing.assert_allclose(stepfun.sorted_interp(u, cw, t).numpy(), want, rtol=0, atol=1e-15)


# ---------------------------------------------------------------- PathCameras.from_config

ARGS = dict(focal=20., height=12, width=16, near=0.1, far=3.)


def test_from_config_forward_facing(g):
    cfg = configs.Config(forward_facing=True, render_path=True, render_path_frames=8)
    poses, bounds = g["forward_poses"].copy(), g["forward_bounds"].copy()
    pc = datasets.PathCameras.from_config(cfg, poses, bounds, **ARGS)
    assert np.array_equal(poses, g["forward_poses"]) and np.array_equal(bounds, g["forward_bounds"])     # inputs untouched
    close("from_config_forward_facing", pc.camtoworlds, g["ff_spiral"])
    close("from_config_forward_facing", pc.colmap_to_world_transform, g["ff_transform"])
    close("from_config_forward_facing", pc.poses, g["ff_poses"])
    p2c = camera_utils.get_pixtocam(20., 16, 12)
    pixtocams, camtoworlds, distortion, ndc = pc.cameras
    assert np.array_equal(pixtocams, p2c) and np.array_equal(ndc, p2c) and distortion is None and camtoworlds is pc.camtoworlds
    assert (pc.size, len(pc), pc.height, pc.width, pc.near, pc.far, pc.spherical) == (8, 8, 12, 16, 0.1, 3., False)


def test_from_config_360(g, tmp_path):
    cfg = configs.Config(render_path=True, render_path_frames=8)
    pc = datasets.PathCameras.from_config(cfg, g["inward_poses"], np.array([0.01, 1.]), distortion_params=dict(k1=-.1), **ARGS)
    close("from_config_ellipse", pc.camtoworlds, g["pca_ellipse"])
    close("from_config_ellipse", pc.colmap_to_world_transform, g["inward_pca_transform"])
    assert pc.cameras[2] is None and pc.cameras[3] is None          # a path is rendered without lens distortion, no NDC here
    cfg = configs.Config(render_path=True, render_path_frames=8, z_variation=.5, z_phase=.25)
    wave = datasets.PathCameras.from_config(cfg, g["inward_poses"], np.array([0.01, 1.]), **ARGS).camtoworlds
    assert np.abs(wave[:, 2, 3]).max() > 1e-3 and np.abs(pc.camtoworlds[:, 2, 3]).max() == 0      # z_variation reaches the path

    cfg = spline_config(g, tmp_path, render_path=True)
    pc = datasets.PathCameras.from_config(cfg, g["inward_poses"], np.array([0.01, 1.]),
                                          image_names=[str(n) for n in g["spline_image_names"]], **ARGS)
    close("from_config_spline", pc.camtoworlds, g["pca_spline_poses"])
    assert np.array_equal(pc.spline_indices, g["pca_spline_indices"])


def test_from_config_render_overrides(g, tmp_path):
    path_file = tmp_path / "path.npy"
    custom = g["inward_ellipse_wave"][:5]
    np.save(path_file, custom)
    cfg = configs.Config(render_path=True, render_path_frames=8, render_path_file=str(path_file), render_resolution=(24, 10),
                         render_focal=33., render_camtype='perspective')
    pc = datasets.PathCameras.from_config(cfg, g["inward_poses"], np.array([0.01, 1.]), **ARGS)
    assert np.array_equal(pc.camtoworlds, custom) and pc.size == 5
    assert (pc.width, pc.height, pc.spherical) == (24, 10, False)
    assert np.array_equal(pc.cameras[0], camera_utils.get_pixtocam(33., 24, 10))
    close("from_config_ellipse", pc.colmap_to_world_transform, g["inward_pca_transform"])

    pano = datasets.PathCameras.from_config(configs.Config(render_path=True, render_path_frames=8, render_camtype='pano'),
                                            g["inward_poses"], np.array([0.01, 1.]), **ARGS)
    assert pano.spherical
    with pytest.raises(ValueError, match="PERSPECTIVE"):
        datasets.PathCameras.from_config(configs.Config(render_path=True, render_path_frames=8, render_camtype='fisheye'),
                                         g["inward_poses"], np.array([0.01, 1.]), **ARGS)
    with pytest.raises(ValueError):
        datasets.PathCameras.from_config(configs.Config(render_path=True, render_path_frames=8, render_camtype='orthographic'),
                                         g["inward_poses"], np.array([0.01, 1.]), **ARGS)


def test_from_config_test_views(g):
    """render_path = False: the given poses, unchanged, with their distortion."""
    dist = dict(k1=-.1, p2=1e-3)
    cfg = configs.Config(render_path=False, forward_facing=True, render_resolution=(24, 10), render_camtype='pano')
    pc = datasets.PathCameras.from_config(cfg, g["forward_poses"], g["forward_bounds"], distortion_params=dist, **ARGS)
    assert np.array_equal(pc.camtoworlds, g["forward_poses"]) and pc.cameras[2] == dist
    assert np.array_equal(pc.colmap_to_world_transform, np.eye(4))
    assert (pc.width, pc.height, pc.spherical) == (16, 12, False)              # the render_* fields apply to paths only
    assert np.array_equal(pc.cameras[3], camera_utils.get_pixtocam(20., 16, 12))
    with pytest.raises(TypeError):
        datasets.PathCameras.from_config(cfg, g["forward_poses"], g["forward_bounds"], distortion_params=dict(k9=1.), **ARGS)


# ---------------------------------------------------------------- the spherical kernel's arithmetic, emulated

def spherical_emulation(c2w32, height, width):
    """image_rays_kernel<true, .>: float64 from the float32 pose, rounded to float32 at the store.  Node (i, j) and its
    j + 1 / i + 1 neighbours, the last column / row reaching theta = 2 pi / phi = pi."""
    c2w = c2w32.astype(np.float64)
    j, i = np.meshgrid(np.arange(width), np.arange(height), indexing='xy')
    th = lambda jj: np.where(jj == width, 2 * np.pi, jj * (2 * np.pi / width))      # noqa: E731
    ph = lambda ii: np.where(ii == height, np.pi, ii * (np.pi / height))          # noqa: E731

    def direction(ii, jj):
        cam = np.stack([-np.sin(ph(ii)) * np.sin(th(jj)), np.cos(ph(ii)), np.sin(ph(ii)) * np.cos(th(jj))], -1)
        return (c2w[:, 0] * cam[..., 0:1] + c2w[:, 1] * cam[..., 1:2]) + c2w[:, 2] * cam[..., 2:3]
    d0, d1, d2 = direction(i, j), direction(i, j + 1), direction(i + 1, j)
    radii = (0.5 * (np.sqrt(((d1 - d0) ** 2).sum(-1)) + np.sqrt(((d2 - d0) ** 2).sum(-1)))) * 2.0 / np.sqrt(12.0)
    d32 = d0.astype(np.float32)
    return dict(origins=np.broadcast_to(c2w32[:, 3], d32.shape), directions=d32, viewdirs=d32,
                radii=radii.astype(np.float32)[..., None], imageplane=np.zeros(d32.shape[:2] + (2,), np.float32))


def test_spherical_emulation_reaches_the_bars(g):
    """The kernel's scheme (double arithmetic, float32 pose and stores) is within the ray generator's bars of the
    reference's float64 panorama on both sizes -- before a GPU is involved."""
    assert [str(c) for c in g["pano_cases"]] == ["pano_6x8", "pano_9x37"]
    for case in g["pano_cases"]:
        h, w = int(g[f"{case}_height"]), int(g[f"{case}_width"])
        emu = spherical_emulation(g[f"{case}_camtoworld"], h, w)
        for k, v in emu.items():
            want = g[f"{case}_{k}"]
            err = np.abs(v - want) / (ATOL + RTOL * np.abs(want))
            print(f"{case} {k}: worst error / bar {err.max():.3f}")
            np.testing.assert_allclose(v, want, rtol=RTOL, atol=ATOL, err_msg=f"{case} {k}")
        assert np.isfinite(emu["radii"][0]).all() and (emu["radii"][0] > 0).all()      # the pole row: dx = 0, dy is not
        assert np.array_equal(g[f"{case}_cam_idx"], np.zeros((h, w, 1))) and np.array_equal(g[f"{case}_lossmult"], np.ones((h, w, 1)))


# ---------------------------------------------------------------- models.render_path with a fake renderer

class FakeCameras:
    def __init__(self, size, height=3, width=4):
        self.size, self.height, self.width, self.cast = size, height, width, []

    def generate_ray_batch(self, idx):
        self.cast.append(idx)
        z = lambda n, dtype=torch.float32: torch.full((self.height, self.width, n), float(idx), dtype=dtype)   # noqa: E731
        pixel = torch.arange(self.height * self.width, dtype=torch.float32).reshape(self.height, self.width, 1)
        return utils.Batch(rays=utils.Rays(origins=z(3), directions=z(3), viewdirs=z(3), radii=z(1), imageplane=z(2), lossmult=z(1),
                                           near=z(1), far=pixel, cam_idx=z(1, torch.int32)))


def fake_render_fn(rays):
    """Constant images: every colour is the frame index (carried in the rays' `near`) / 16; `acc` is a ramp over the
    pixels (carried in `far`), since the roughness artefact is min-max normalised by it."""
    n = rays.origins.shape[0]
    v = rays.near[:, 0] / 16.
    one, three, acc = v.clone(), v[:, None].expand(n, 3).clone(), rays.far[:, 0] / 16.
    return [dict(rgb=three, diffuse=three, specular=three, normals_pred=three, acc=acc, distance_mean=one, distance_median=one,
                 roughness=one)], None


ARTEFACTS = ("color_{}.png", "diffuse_{}.png", "specular_{}.png", "normals_pred_{}.png", "rho_{}.png", "distance_mean_{}.tiff",
             "distance_median_{}.tiff", "acc_{}.tiff")


@pytest.fixture
def host_render(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)      # render_image synchronises; there is no device here


def test_render_path_names_and_padding(host_render, tmp_path):
    cfg = configs.Config(render_chunk_size=5)
    cams = FakeCameras(3)
    done = list(models.render_path(fake_render_fn, cams, cfg, out_dir=str(tmp_path)))
    assert [i for i, _ in done] == [0, 1, 2] and cams.cast == [0, 1, 2]
    for idx, rendering in done:
        assert rendering["rgb"].shape == (3, 4, 3) and bool((rendering["rgb"] == idx / 16.).all())
    assert sorted(os.listdir(tmp_path)) == sorted(a.format(f"{i:03d}") for a in ARTEFACTS for i in range(3))
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "color_002.png")), np.full((3, 4, 3), int(2 / 16. * 255), np.uint8))

    big = tmp_path / "big"                      # 12001 views: five digits
    cfg = configs.Config(render_chunk_size=64, render_num_jobs=6000, render_job_id=1)
    assert [i for i, _ in models.render_path(fake_render_fn, FakeCameras(12001), cfg, out_dir=str(big))] == [1, 6001]
    assert sorted(os.listdir(big)) == sorted(a.format(s) for a in ARTEFACTS for s in ("00001", "06001"))

    cams = FakeCameras(2)                       # without out_dir nothing is written
    assert [i for i, _ in models.render_path(fake_render_fn, cams, configs.Config(), out_dir=None)] == [0, 1]


def test_render_path_job_striding(host_render, tmp_path):
    seen = []
    for job in range(3):
        cfg = configs.Config(render_num_jobs=3, render_job_id=job)
        mine = [i for i, _ in models.render_path(fake_render_fn, FakeCameras(8), cfg, out_dir=str(tmp_path))]
        assert mine == list(range(job, 8, 3))
        seen += mine
    assert sorted(seen) == list(range(8))
    assert len(os.listdir(tmp_path)) == 8 * len(ARTEFACTS)


def test_render_path_skip_rule(host_render, tmp_path):
    """A view is skipped only when its own colour file and that of the job's next view both exist."""
    cfg = configs.Config(render_num_jobs=2, render_job_id=0)
    for i in (0, 2, 6):
        (tmp_path / f"color_{i:03d}.png").write_bytes(b"")
    cams = FakeCameras(9)
    gen = models.render_path(fake_render_fn, cams, cfg, out_dir=str(tmp_path))
    assert cams.cast == []                      # a generator: nothing runs before the first next()
    # 0: 000 and 002 exist -> skipped; 2: 004 is missing -> rendered; 4: rendered; 6: 008 is missing -> rendered; 8: rendered
    assert [i for i, _ in gen] == [2, 4, 6, 8] and cams.cast == [2, 4, 6, 8]
    assert (tmp_path / "color_000.png").read_bytes() == b"" and (tmp_path / "color_002.png").stat().st_size > 0
    # a second pass finds every file of the job: only the last view, whose successor does not exist, is rendered again
    assert [i for i, _ in models.render_path(fake_render_fn, FakeCameras(9), cfg, out_dir=str(tmp_path))] == [8]

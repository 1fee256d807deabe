"""The scene loaders (datasets.load_dataset / Blender / LLFF), the device image preparation (refnerf_prepare_images) and the
fused training batch (refnerf_train_batch).

Fixture: tests/golden/scene_datasets.npz (tests/golden/make_golden_datasets.py): two tiny scenes as raw arrays and what
the reference's `Blender` / `LLFF` loaded from them.  Every test rebuilds the scene folders in tmp_path (PNG and float
TIFF are lossless).

Bars.  Everything the loaders compute from pixels is compared with np.array_equal / torch.equal: the preparation is the
reference's float32 flow rounding for rounding, and the fused batch is the arithmetic of the existing ray kernels.  The
LLFF pose normalisation follows the reference's dtype flow and comes out equal too (no tolerance).  Only the debug-mode
batch against the reference's numpy rays has a tolerance: the ray generator's own bars, imported from
test_lens_distortion.py.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import refnerf_pl_amd  # noqa: F401
from helpers import GOLDEN, load_golden
from test_lens_distortion import ATOL, RTOL


def _load_generator():
    """tests/golden/make_golden_datasets.py as a module, without putting its folder on sys.path (importing it touches
    nothing; see its docstring): the scene writer and the case tables are shared with the fixture's generator."""
    spec = importlib.util.spec_from_file_location("make_golden_datasets", os.path.join(GOLDEN, "make_golden_datasets.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


mk = _load_generator()

DEV = "cuda:0"
RAY_FIELDS = mk.RAY_FIELDS
SIDE = ("rgb", "disps", "normals", "alphas")


@pytest.fixture(scope="module")
def z():
    return load_golden("scene_datasets")


@pytest.fixture
def scenes(z, tmp_path):
    return dict(zip(("blender", "llff"), mk.write_scenes(z, str(tmp_path))))


@pytest.fixture(scope="module")
def hip():
    from refnerf_pl_amd import _hip
    _hip.require_device()
    return _hip


def case_config(z, case, **more):
    from refnerf_pl_amd import configs
    entry = json.loads(str(z[case + "_config"]))
    cfg = configs.Config(dataset_loader=entry["loader"], render_path_frames=mk.FRAMES, **dict(entry["config"], **more))
    return entry["loader"], entry["split"], cfg


def load_case(z, scenes, case, device, **more):
    from refnerf_pl_amd import datasets
    loader, split, cfg = case_config(z, case, **more)
    return datasets.load_dataset(split, scenes[loader], cfg, device=device)


def host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def same(a, want, what):
    a, want = host(a), np.asarray(want)
    assert a.shape == want.shape and a.dtype == want.dtype, (what, a.shape, a.dtype, want.shape, want.dtype)
    assert np.array_equal(a, want), what


def check_loaded(z, ds, case):
    """Every attribute the fixture stores for `case`, equal."""
    for attr in ("images", "alphas", "normal_images", "disp_images"):
        key = f"{case}_{attr}"
        if attr == "images" and key not in z.files:       # LLFF: the rows of the raw stack the reference selected
            raw = z["llff_images_2" if ds.config.factor > 1 else "llff_images"]
            same(ds.images, raw[z[case + "_image_index"]].astype(np.float32) / 255., key)
        elif key in z.files:
            same(getattr(ds, attr), z[key], key)
        else:
            assert getattr(ds, attr) is None, key
    for attr in ("camtoworlds", "pixtocams"):
        same(getattr(ds, attr), z[f"{case}_{attr}"], f"{case}_{attr}")
    for attr in ("focal", "height", "width", "near", "far", "size"):
        assert getattr(ds, attr) == z[f"{case}_{attr}"], (case, attr)
    assert ds.cameras[0] is ds.pixtocams and ds.cameras[1] is ds.camtoworlds and ds.split == json.loads(str(z[case + "_config"]))["split"]
    if case.startswith("llff"):
        if case + "_pixtocam_ndc" in z.files:
            same(ds.pixtocam_ndc, z[case + "_pixtocam_ndc"], case + " ndc")
        else:
            assert ds.pixtocam_ndc is None
        assert ds.distortion_params == json.loads(str(z[case + "_distortion_params"]))
        same(ds.poses, z[case + "_poses"], case + " poses")
        same(ds.colmap_to_world_transform, z[case + "_colmap_to_world_transform"], case + " transform")


# ---------------------------------------------------------------- CPU: the host path

def test_host_path_equals_reference_blender(z, scenes):
    cases = [c for c in z["cases"] if c.startswith("blender")]
    assert len(cases) == len(mk.BLENDER_CASES)
    for case in cases:
        ds = load_case(z, scenes, case, "cpu")
        check_loaded(z, ds, case)
        assert ds.images.device.type == "cpu" and ds.distortion_params is None and ds.pixtocam_ndc is None


def test_host_path_equals_reference_llff(z, scenes):
    cases = [c for c in z["cases"] if c.startswith("llff")]
    assert len(cases) == len(mk.LLFF_CASES)
    for case in cases:
        check_loaded(z, load_case(z, scenes, case, "cpu"), case)
    # without poses_bounds.npy the reference's default bounds apply: same scene, forward facing, other scale
    os.remove(os.path.join(scenes["llff"], "poses_bounds.npy"))
    ds = load_case(z, scenes, "llff_ff_train", "cpu")
    assert not np.array_equal(ds.camtoworlds, z["llff_ff_train_camtoworlds"])
    from refnerf_pl_amd import camera_utils, datasets
    names, poses, _, _, _ = datasets.load_blender_posedata(scenes["llff"])
    poses = poses[np.argsort(names)]
    scale = 1. / (np.array([0.01, 1.]).min() * .75)           # a numpy scalar, as in the loader (datasets.py:646, 654)
    poses[:, :3, 3] *= scale
    assert np.array_equal(ds.colmap_to_world_transform, camera_utils.recenter_poses(poses)[1] @ np.diag([scale] * 3 + [1]))


def test_integer_block_sums_reproduce_the_float32_mean():
    """What licenses the integer-sum kernel: for every possible block sum, float32(sum) / factor^2 / 255 as the host path
    and the kernel compute it equals the reference expression, the float32 array's .mean() then / 255."""
    from refnerf_pl_amd import _hip, datasets
    for f in (2, 3, 4, 5):
        sums = np.arange(255 * f * f + 1)
        q, r = np.divmod(sums, f * f)
        blocks = (q[:, None] + (np.arange(f * f)[None, :] < r[:, None])).astype(np.uint8)     # [S, f*f], row s sums to s
        assert np.array_equal(blocks.sum(1, dtype=np.int64), sums)
        img = blocks.reshape(1, len(sums) * f, f, 1)                                              # one block per f rows
        want = np.stack([b.astype(np.float32).reshape(1, f, 1, f).mean((1, 3)) for b in blocks]).reshape(-1) / 255.
        assert want.dtype == np.float32
        got = datasets.prepare_images_host(img, _hip.PREP_SCALE, f)
        assert got.shape == (1, len(sums), 1, 1) and np.array_equal(got.reshape(-1), want), f
        assert np.array_equal((sums.astype(np.float32) / np.float32(f * f)) / np.float32(255.), want), f


def test_errors_are_raised_on_the_host(z, scenes):
    from refnerf_pl_amd import configs, datasets
    with pytest.raises(ValueError, match="does not evenly divide"):
        load_case(z, scenes, "blender_train", "cpu", factor=5)
    with pytest.raises(ValueError, match="does not evenly divide"):
        load_case(z, scenes, "blender_train", DEV, factor=5)            # decided before any device is touched
    with pytest.raises(ValueError, match="Image folder .*images_3 does not exist"):
        load_case(z, scenes, "llff_train", "cpu", factor=3)
    with pytest.raises(ValueError, match="render_path cannot be used for the blender dataset"):
        load_case(z, scenes, "blender_test", "cpu", render_path=True)
    with pytest.raises(ValueError, match="use_tiffs"):
        load_case(z, scenes, "blender_train", "cpu", use_tiffs=True)
    with pytest.raises(ValueError, match="Patch size 7\\^2 too large for per-process batch size 48"):
        load_case(z, scenes, "blender_train", "cpu", patch_size=7, batch_size=48)
    for name in ("tat_nerfpp", "tat_fvs", "dtu", "rffr"):
        with pytest.raises(ValueError, match=f"'{name}' is not built"):
            datasets.load_dataset("train", scenes["llff"], configs.Config(dataset_loader=name), device="cpu")
    with pytest.raises(ValueError, match="unknown dataset_loader"):
        datasets.load_dataset("train", scenes["llff"], configs.Config(dataset_loader="nope"), device="cpu")
    with pytest.raises(ValueError, match="DataSplit"):
        datasets.Blender("nope", scenes["blender"], configs.Config(), device="cpu")
    os.makedirs(os.path.join(scenes["llff"], "sparse", "0"))
    with pytest.raises(ValueError, match="pycolmap"):
        load_case(z, scenes, "llff_train", "cpu")


def test_llff_render_path_is_the_path_of_pathcameras(z, scenes):
    from refnerf_pl_amd import datasets
    for case in ("llff_test", "llff_ff_test"):
        ds = load_case(z, scenes, case, "cpu", render_path=True)
        _, _, cfg = case_config(z, case, render_path=True)
        names, poses, _, _, _ = datasets.load_blender_posedata(scenes["llff"])
        order = np.argsort(names)
        bounds = z["llff_poses_bounds"][:, -2:]
        want = datasets.PathCameras.from_config(cfg, poses[order], bounds, ds.focal, 12, 18, cfg.near, cfg.far,
                                                image_names=[names[i] for i in order])
        assert ds.size == mk.FRAMES == want.size and ds.distortion_params is None
        assert np.array_equal(ds.camtoworlds, want.camtoworlds) and np.array_equal(ds.pixtocams, want.pixtocams)
        assert (ds.pixtocam_ndc is None) == (case == "llff_test")
        # the dataset's own normalisation (float32 flow) and the path's (float64) are the same function on the same poses
        assert np.allclose(ds.poses, want.poses, rtol=0, atol=1e-5) and ds.poses.shape == (9, 3, 4)


def test_host_debug_batches_carry_the_reference_pixels(z, scenes):
    """`dataset_debug_mode` on the host, rays left as Pixels: the gathered colours (and disps / normals / alphas) are the
    reference batch's, and the pixels are its deterministic ones."""
    from refnerf_pl_amd import utils
    for case in z["batch_cases"]:
        ds = load_case(z, scenes, case, "cpu")
        batch = ds.next(cast_rays=False)
        assert isinstance(batch.rays, utils.Pixels)
        for k in SIDE:
            if f"{case}_{k}" in z.files:
                same(getattr(batch, k), z[f"{case}_{k}"], f"{case} {k}")
            else:
                assert getattr(batch, k) is None, (case, k)
        n = z[f"{case}_rgb"].shape[0]
        upper = ds.config.patch_size - 1
        assert np.array_equal(host(batch.rays.pix_x_int).reshape(-1), np.arange(n) % (18 - upper))
        assert np.array_equal(host(batch.rays.pix_y_int).reshape(-1), np.arange(n) // (18 - upper))
        assert len(ds) == ds.images.shape[0] * 12 * 18 // ds.config.batch_size


# ---------------------------------------------------------------- GPU: refnerf_prepare_images

def random_stack(rng, n, H, W, Cn):
    x = rng.integers(0, 256, (n, H, W, Cn), dtype=np.uint8)
    if Cn == 4:
        kind = rng.integers(0, 3, (n, H, W))
        x[..., 3] = np.where(kind == 0, 0, np.where(kind == 1, 255, x[..., 3]))
    return x


def prepared_equal(hip, src, op, factor, alpha=False):
    from refnerf_pl_amd import datasets
    want = datasets.prepare_images_host(src, op, factor, return_alpha=alpha)
    got = hip.prepare_images(torch.from_numpy(src).to(DEV), op, factor, return_alpha=alpha)
    for g, w in zip(got if alpha else (got,), want if alpha else (want,)):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape, (op, factor)
        assert torch.equal(g.cpu(), torch.from_numpy(np.ascontiguousarray(w))), (op, factor, src.shape)
    return got


@pytest.mark.gpu
def test_prepare_images_equals_the_host_path(hip):
    rng = np.random.default_rng(1)
    for Cn in (3, 4):
        src = random_stack(rng, 3, 12, 18, Cn)                       # 3 * 12 * 18 = 648 outputs at factor 1: a partial block
        for factor in (1, 2, 3):
            prepared_equal(hip, src, hip.PREP_SCALE, factor)
            prepared_equal(hip, src, hip.PREP_NORMALS, factor)
            prepared_equal(hip, src, hip.PREP_RAW, factor)
            if Cn == 4:
                prepared_equal(hip, src, hip.PREP_WHITE, factor)
                prepared_equal(hip, src, hip.PREP_WHITE, factor, alpha=True)
    prepared_equal(hip, random_stack(rng, 2, 12, 18, 1)[..., 0], hip.PREP_SCALE, 2)          # [n,H,W]: one channel
    big = random_stack(rng, 5, 36, 30, 4)                            # 5400 outputs: 21 blocks and a tail of 24
    prepared_equal(hip, big, hip.PREP_WHITE, 1, alpha=True)
    prepared_equal(hip, big, hip.PREP_SCALE, 1)
    # float32 sources: disparities on the 2^-10 grid (exact block sums), [n,H,W] and [n,H,W,3]
    disp = (rng.integers(0, 4096, (3, 12, 18)) / 1024.).astype(np.float32)
    for factor in (1, 2, 3):
        prepared_equal(hip, disp, hip.PREP_RAW, factor)
    prepared_equal(hip, (rng.integers(0, 4096, (3, 12, 18, 3)) / 1024.).astype(np.float32), hip.PREP_RAW, 3)


@pytest.mark.gpu
def test_prepare_images_makes_no_alignment_assumption(hip):
    """Sources that are non-zero-offset slices of a larger allocation: RGBA at byte offsets 1 and 3 (the byte path), 4 (the
    32-bit path), RGB at offset 1, float32 at element offset 1."""
    rng = np.random.default_rng(2)
    for Cn, offsets in ((4, (1, 3, 4)), (3, (1,))):
        src = random_stack(rng, 3, 12, 18, Cn)
        for off in offsets:
            buf = torch.zeros(src.size + 16, dtype=torch.uint8, device=DEV)
            view = buf[off:off + src.size].view(src.shape)
            view.copy_(torch.from_numpy(src))
            assert view.data_ptr() % 4 == off % 4 and view.is_contiguous()
            for factor in (1, 2):
                op = hip.PREP_WHITE if Cn == 4 else hip.PREP_SCALE
                assert torch.equal(hip.prepare_images(view, op, factor), hip.prepare_images(torch.from_numpy(src).to(DEV), op, factor))
    disp = (rng.integers(0, 4096, (2, 12, 18)) / 1024.).astype(np.float32)
    buf = torch.zeros(disp.size + 3, dtype=torch.float32, device=DEV)
    view = buf[1:1 + disp.size].view(disp.shape)
    view.copy_(torch.from_numpy(disp))
    assert torch.equal(hip.prepare_images(view, hip.PREP_RAW, 2), hip.prepare_images(torch.from_numpy(disp).to(DEV), hip.PREP_RAW, 2))


@pytest.mark.gpu
def test_prepare_images_refuses_on_the_host(hip):
    x = torch.zeros((2, 12, 18, 4), dtype=torch.uint8, device=DEV)
    for src, op, factor, alpha, msg in ((x, hip.PREP_SCALE, 5, False, "does not evenly divide"), (x, hip.PREP_SCALE, 0, False, "factor"),
                                        (x[..., :3].contiguous(), hip.PREP_WHITE, 1, False, "needs C = 4"),
                                        (x[..., 0].contiguous(), hip.PREP_NORMALS, 1, False, "needs C >= 3"),
                                        (x, hip.PREP_SCALE, 1, True, "d_alpha"), (x, 7, 1, False, "unknown operation"),
                                        (torch.zeros((1, 514, 514, 1), dtype=torch.uint8, device=DEV), hip.PREP_SCALE, 257, False, "above 256"),
                                        (x[..., :2].contiguous(), hip.PREP_SCALE, 1, False, "C must be 1, 3 or 4")):
        with pytest.raises(ValueError, match=msg):
            hip.prepare_images(src, op, factor, return_alpha=alpha)


@pytest.mark.gpu
def test_device_loaders_equal_the_reference(z, scenes, hip):
    """The loaders on the device against the fixture, attribute for attribute, and one launch per prepared stack."""
    for case in z["cases"]:
        torch.cuda.synchronize()
        hip.set_timing(True)
        ds = load_case(z, scenes, str(case), DEV)
        launches = sum(hip.get_timing(f)[1] for f in range(5))
        hip.set_timing(False)
        check_loaded(z, ds, str(case))
        assert ds.images.is_cuda
        metrics = "metrics" in str(case)
        assert launches == (3 if metrics else 1), (case, launches)


# ---------------------------------------------------------------- GPU: refnerf_train_batch

N_CAM, IH, IW = 3, 11, 13


def array_scene(rng, per_camera, ndc, distortion):
    """(images, disps, normals, alphas, cameras): n = 3 cameras, 11 x 13 images."""
    images = rng.random((N_CAM, IH, IW, 3), dtype=np.float32)
    disps, alphas = rng.random((N_CAM, IH, IW), dtype=np.float32), rng.random((N_CAM, IH, IW), dtype=np.float32)
    normals = rng.standard_normal((N_CAM, IH, IW, 3)).astype(np.float32)
    p2c = np.linalg.inv(np.array([[15.5, 0, 6.4], [0, 14.75, 5.6], [0, 0, 1.]]))
    if per_camera:
        p2c = np.stack([p2c @ np.diag([1 + .1 * k, 1 - .05 * k, 1.]) for k in range(N_CAM)])
    c2w = []
    for k in range(N_CAM):
        q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        c2w.append(np.concatenate([q, rng.normal(0, 2., (3, 1))], -1))
    p2c, c2w = p2c.astype(np.float32), np.stack(c2w).astype(np.float32)
    ndc_m = np.linalg.inv(np.array([[15.5, 0, 6.5], [0, 15.5, 5.5], [0, 0, 1.]])).astype(np.float32) if ndc else None
    dist = dict(k1=0.04, k2=-0.01, p1=0.002, p2=-0.001) if distortion else None
    return images, disps, normals, alphas, (p2c, c2w, dist, ndc_m)


def batches_equal(a, b, what):
    for k in RAY_FIELDS:
        x, y = getattr(a.rays, k), getattr(b.rays, k)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, k)
    assert a.rgb.shape == b.rgb.shape and torch.equal(a.rgb, b.rgb), what


@pytest.mark.gpu
@pytest.mark.parametrize("batch_size,patch_size", [(333, 3), (37, 1)])      # 37 patches either way; 333 rays = a block and a tail
def test_train_batch_equals_the_step_by_step_batcher(hip, batch_size, patch_size):
    from refnerf_pl_amd import configs, datasets
    rng = np.random.default_rng(3)
    for batching in ("all_images", "single_image"):
        for per_camera in (False, True):
            for ndc in (False, True):
                for distortion in (False, True):
                    for debug in (False, True):
                        what = (batching, per_camera, ndc, distortion, debug)
                        images, disps, normals, alphas, cams = array_scene(rng, per_camera, ndc, distortion)
                        cfg = configs.Config(batch_size=batch_size, patch_size=patch_size, batching=batching, near=.3, far=5.5,
                                             dataset_debug_mode=debug)
                        ds = datasets.ArrayScene(cfg, images, cams, disp_images=disps, normal_images=normals, alphas=alphas,
                                                 device=DEV, seed=11, rank=2)
                        ref = datasets.TrainRayBatcher(images, cams, .3, 5.5, batch_size, patch_size, batching, seed=11, rank=2,
                                                       device=DEV, debug_mode=debug)
                        for _ in range(2):                                   # the generators stay in step
                            got, want = ds.next(), ref.next()
                            batches_equal(got, want, what)
                        pixels = datasets.TrainRayBatcher(images, cams, .3, 5.5, batch_size, patch_size, batching, seed=11, rank=2,
                                                          device=DEV, debug_mode=debug).sample_pixels()
                        first = datasets.ArrayScene(cfg, images, cams, disp_images=disps, normal_images=normals, alphas=alphas,
                                                    device=DEV, seed=11, rank=2).next()
                        cam, y, x = pixels.cam_idx[..., 0].long(), pixels.pix_y_int.long(), pixels.pix_x_int.long()
                        for name, stack in (("disps", disps), ("normals", normals), ("alphas", alphas)):
                            assert torch.equal(getattr(first, name), torch.from_numpy(stack).to(DEV)[cam, y, x]), (what, name)
                        n_rays = (batch_size // patch_size ** 2) * (1 if debug else patch_size ** 2)
                        assert first.rgb.numel() == 3 * n_rays


@pytest.mark.gpu
def test_train_batch_binding_border_patches(hip):
    """Hand-placed origins (0, 0) and (W - ps, H - ps): the corner patches, against refnerf_pixels_to_rays on the expanded
    pixels with per-ray cameras and stack[cam, y, x]; int32 and int64 indices agree."""
    rng = np.random.default_rng(4)
    ps = 3
    images, disps, normals, alphas, (p2c, c2w, _, _) = array_scene(rng, True, False, False)
    dev = dict(device=DEV)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    px0 = torch.tensor([0, IW - ps, 5, 0], dtype=torch.int32, **dev)
    py0 = torch.tensor([0, IH - ps, 4, IH - ps], dtype=torch.int32, **dev)
    cam = torch.tensor([0, 2, 1, 2], dtype=torch.int32, **dev)
    rays, got = hip.train_batch(px0, py0, cam, ps, t(images), t(p2c), t(c2w), 2., 6., disps=t(disps), normals=t(normals), alphas=t(alphas))
    d = torch.arange(ps, **dev)
    x = (px0.long().reshape(-1, 1, 1) + d.reshape(1, 1, -1)).expand(-1, ps, ps)
    y = (py0.long().reshape(-1, 1, 1) + d.reshape(1, -1, 1)).expand(-1, ps, ps)
    c = cam.long().reshape(-1, 1, 1).expand(-1, ps, ps)
    assert int(x.max()) == IW - 1 and int(y.max()) == IH - 1 and int(x.min()) == 0 and int(y.min()) == 0
    want = hip.pixels_to_rays(x.reshape(-1), y.reshape(-1), t(p2c)[c.reshape(-1)], t(c2w)[c.reshape(-1)])
    for k, w in zip(("origins", "directions", "viewdirs", "radii", "imageplane"), want):
        assert torch.equal(rays[k].reshape(w.shape), w), k
    assert torch.equal(rays["cam_idx"][..., 0], c.int()) and rays["cam_idx"].dtype == torch.int32
    assert float(rays["lossmult"].min()) == 1. == float(rays["lossmult"].max()) and tuple(rays["near"].shape) == (4, ps, ps, 1)
    assert torch.equal(rays["near"], torch.full_like(rays["near"], 2.)) and torch.equal(rays["far"], torch.full_like(rays["far"], 6.))
    for name, stack in (("rgb", images), ("disps", disps), ("normals", normals), ("alphas", alphas)):
        assert torch.equal(got[name], t(stack)[c, y, x]), name
    rays64, got64 = hip.train_batch(px0.long(), py0.long(), cam.long(), ps, t(images), t(p2c), t(c2w), 2., 6., disps=t(disps),
                                    normals=t(normals), alphas=t(alphas))
    assert all(torch.equal(rays[k], rays64[k]) for k in rays) and all(torch.equal(got[k], got64[k]) for k in got)
    one = hip.train_batch(px0, py0, cam[1:2].contiguous(), ps, t(images), t(p2c), t(c2w), 2., 6.)[0]       # 'single_image'
    assert torch.equal(one["cam_idx"], torch.full_like(one["cam_idx"], 2)) and torch.equal(one["origins"][1], rays["origins"][1])
    with pytest.raises(ValueError, match="patch_size larger than the image"):
        hip.train_batch(px0, py0, cam, IH + 1, t(images), t(p2c), t(c2w), 2., 6.)


@pytest.mark.gpu
def test_debug_batch_against_the_reference(z, scenes, hip):
    """The stored `dataset_debug_mode` training batches of the reference (rays cast by its numpy path) against one fused
    launch, at the ray generator's bars; the gathered pixels are equal."""
    for case in z["batch_cases"]:
        ds = load_case(z, scenes, str(case), DEV)
        batch = ds.next()
        for k in RAY_FIELDS:
            got, want = host(getattr(batch.rays, k)), z[f"{case}_{k}"]
            assert got.shape == want.shape, (case, k, got.shape, want.shape)
            err = np.abs(got - want) / (ATOL + RTOL * np.abs(want))
            print(f"MEASURED {case} {k}: max |diff| / (atol + rtol |ref|) = {err.max():.3f}")
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=f"{case} {k}")
        for k in SIDE:
            if f"{case}_{k}" in z.files:
                same(getattr(batch, k), z[f"{case}_{k}"], f"{case} {k}")
            else:
                assert getattr(batch, k) is None


@pytest.mark.gpu
def test_one_launch_per_training_batch_and_whole_views(z, scenes, hip):
    ds = load_case(z, scenes, "blender_train_metrics", DEV, batch_size=64)
    ds.next()                                                            # warm-up: the cameras' upload
    torch.cuda.synchronize()
    hip.set_timing(True)
    batch = ds.next()
    launches = [hip.get_timing(f)[1] for f in range(5)]
    hip.set_timing(False)
    assert launches == [0, 0, 0, 0, 1] and tuple(batch.rays.origins.shape) == (64, 1, 1, 3) and tuple(batch.disps.shape) == (64, 1, 1)
    # val / test: whole views round-robin, as views of the resident stacks; debug mode pins view 0 for val
    test = load_case(z, scenes, "blender_test_metrics_f2", DEV)
    seen = [test.next() for _ in range(4)]
    assert [int(b.rays.cam_idx[0, 0, 0]) for b in seen] == [0, 1, 2, 0] and tuple(seen[0].rays.origins.shape) == (6, 9, 3)
    assert seen[1].rgb.data_ptr() == test.images[1].data_ptr() and seen[1].normals.data_ptr() == test.normal_images[1].data_ptr()
    assert seen[2].disps.data_ptr() == test.disp_images[2].data_ptr() and seen[2].alphas.data_ptr() == test.alphas[2].data_ptr()
    from refnerf_pl_amd import camera_utils
    want = camera_utils.cast_image_rays(test.cameras, 1, 6, 9, test.near, test.far, device=torch.device(DEV))
    assert all(torch.equal(getattr(seen[1].rays, k), getattr(want, k)) for k in RAY_FIELDS)
    _, _, cfg = case_config(z, "llff_ff_test", dataset_debug_mode=True)
    from refnerf_pl_amd import datasets
    val = datasets.LLFF("val", scenes["llff"], cfg, device=DEV)
    assert [int(val.next().rays.cam_idx[0, 0, 0]) for _ in range(3)] == [0, 0, 0] and val.size == 2


@pytest.mark.gpu
def test_end_to_end_train_and_test_on_the_blender_scene(z, scenes, hip):
    """The Batch the loaders make is the one the rest of the library consumes: three training steps' losses, and a test view
    through render_image into evaluate_test_image with the disparity and normal metrics on."""
    from refnerf_pl_amd import configs, datasets, image, models, synthetic, train_utils
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(os.path.dirname(GOLDEN), os.pardir, "configs", "refnerf_blender.gin")],
                                            ["Config.batch_size = 64", "Config.compute_disp_metrics = True",
                                             "Config.compute_normal_metrics = True", "Config.render_chunk_size = 216"])
    cfg = configs.Config()
    assert cfg.dataset_loader == "blender"
    dev = torch.device(DEV)
    model = models.construct_model(None, cfg).to(dev)
    configs.clear_config()
    model.nerf_mlp.load_flat_params(synthetic.make_params(seed=0, bias_scale=0.05, sharpen=20.0))
    train = datasets.load_dataset("train", scenes["blender"], cfg, device=dev)
    for step in range(3):
        batch = train.next()
        total, terms, _, _ = train_utils.training_losses(model, batch, batch.rays, cfg, global_step=step + 1)
        assert torch.isfinite(total) and "data" in terms, (step, total)
    test = datasets.load_dataset("test", scenes["blender"], cfg, device=dev)
    batch = test.next()
    model.eval()
    with torch.no_grad():
        rendering = models.render_image(lambda r: model(r, 1.0, True), batch.rays, cfg, verbose=False, device=dev)
    metric, metric_cc, rgb_cc = image.evaluate_test_image(rendering, batch, cfg)
    # in eval mode the model renders the predicted normals only (as the reference does)
    assert {"psnr", "ssim", "disparity_mean_mse", "disparity_median_mse", "normals_pred_mae"} <= set(metric) and tuple(rgb_cc.shape) == (12, 18, 3)
    assert all(bool(torch.isfinite(v)) for v in list(metric.values()) + list(metric_cc.values())), (metric, metric_cc)

"""Scene datasets, on the device: the loaders, the render-path cameras and the training batches in front of the hot path
(second half).

`load_dataset(split, data_dir, config)` is the reference's entry (internal/datasets.py:44-54) for `Blender` and `LLFF`
(:519-708): `SceneDataset` holds what `BaseDataset` holds after `_load_renderings`.  The files are decoded with PIL into
one uint8 stack, uploaded once, and turned into the float32 arrays the reference builds in numpy -- block mean by
`Config.factor`, `/ 255`, white background, normal decoding -- by one launch of refnerf_prepare_images per stack, bit
for bit; the images then live on the device.  `next()` follows `_next_fn` by split: a training batch is the three
`torch.randint` draws of `TrainRayBatcher.sample_pixels` and ONE launch of refnerf_train_batch, which indexes the
camera, casts the nine `Rays` fields and gathers rgb / disps / normals / alphas; val / test views are one launch of
refnerf_image_rays plus views of the resident stacks.  With `device='cpu'` the preparation runs in numpy (the same
operations in the same order) and the batches through the ATen steps of `TrainRayBatcher`, so the loaders work on a host
without a GPU; only casting rays needs one.  Not built: the COLMAP pose reader (`sparse/0`, needs pycolmap), the
loaders 'tat_nerfpp', 'tat_fvs', 'dtu', 'rffr', and `use_tiffs`.

`TrainRayBatcher` mirrors `Dataset._next_train` / `Dataset._make_ray_batch` (:395-485) on caller-held images, step by
step in ATen, for perspective cameras (optionally with lens distortion) with `Config.cast_rays_in_train_step` semantics
(configs.py:80): a batch is `batch_size // patch_size**2` random pixel patches drawn from all images ('all_images') or
from one random image ('single_image'); the colours are gathered and the rays cast (`camera_utils.cast_ray_batch` ->
`refnerf_pixels_to_rays`, or `refnerf_pixels_to_rays_distorted` when the cameras carry a distortion dict) on the device, so
a training step moves no per-ray data over PCIe.  `PathCameras` is the render-path / test views of
`BaseDataset` (:311-336, 487-498) with the pose normalisation and path generation of `LLFF._load_renderings` (:639-681),
whole frames cast in one launch each.

Random numbers: a `torch.Generator` on the device, seeded per rank (`seed + rank`): the reference draws from the global
`numpy.random` state, which every DDP rank and DataLoader worker inherits identically -- not
reproduced on purpose.
"""
import json
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _hip, camera_utils, utils


def normalize_poses(config, poses, bounds, image_names=None):
    """The pose branch of `LLFF._load_renderings` (datasets.py:649-679), on `poses` [n,3,4] / `bounds` as the loader read
    them, in the dtypes given (the loader passes the float32 poses of the JSON, `PathCameras.from_config` float64);
    `poses[:, :3, 3]` and `bounds` are scaled in place, as there.  forward_facing: positions and bounds scaled by
    1 / (0.75 * bounds.min()), `recenter_poses`, the spiral path; otherwise `transform_poses_pca` and the ellipse path
    (`z_variation`, `z_phase`) or the spline path through `render_spline_keyframes` (which needs `image_names`).
    Returns (poses, colmap_to_world_transform, render_poses, spline_indices | None)."""
    spline_indices = None
    if config.forward_facing:
        scale = 1. / (bounds.min() * .75)
        poses[:, :3, 3] *= scale
        bounds *= scale
        poses, transform = camera_utils.recenter_poses(poses)
        transform = transform @ np.diag([scale] * 3 + [1])
        render_poses = camera_utils.generate_spiral_path(poses, bounds, n_frames=config.render_path_frames)
    else:
        poses, transform = camera_utils.transform_poses_pca(poses)
        if config.render_spline_keyframes is not None:
            spline_indices, render_poses = camera_utils.create_render_spline_path(config, image_names, poses)
        else:
            render_poses = camera_utils.generate_ellipse_path(poses, n_frames=config.render_path_frames,
                                                              z_variation=config.z_variation, z_phase=config.z_phase)
    return poses, transform, render_poses, spline_indices


class PathCameras:
    """The render / test half of the reference's `BaseDataset` (datasets.py:311-336, 487-498): a list of views that
    `generate_ray_batch(idx)` turns into whole-image `Rays` on the device, one launch per frame
    (`camera_utils.cast_image_rays` -> refnerf_image_rays).  The pose path goes to the device once, at the first batch;
    building the object touches no device, so paths can be generated and inspected on a host without one.

    `.cameras` is the reference's tuple (pixtocams, camtoworlds, distortion_params, pixtocam_ndc) as host arrays,
    `.camtoworlds` the [size,3,4] float64 path, `.colmap_to_world_transform` the [4,4] normalisation `from_config`
    applied (identity when it applied none)."""

    def __init__(self, pixtocams, camtoworlds, height: int, width: int, near: float, far: float, distortion_params=None,
                 pixtocam_ndc=None, spherical: bool = False, colmap_to_world_transform=None,
                 device: Optional[torch.device] = None):
        if distortion_params is not None:
            camera_utils.lens_distortion(distortion_params)       # unknown keys raise TypeError here, not at the first frame
            distortion_params = dict(distortion_params)
        self.pixtocams = np.asarray(pixtocams, np.float32)
        self.camtoworlds = np.asarray(camtoworlds)[..., :3, :4]
        if self.camtoworlds.ndim != 3:
            raise ValueError(f'camtoworlds must be [n, 3, 4], got {np.asarray(camtoworlds).shape}')
        self.distortion_params, self.pixtocam_ndc = distortion_params, pixtocam_ndc
        self.height, self.width, self.near, self.far = int(height), int(width), float(near), float(far)
        self.spherical = bool(spherical)
        self.colmap_to_world_transform = np.eye(4) if colmap_to_world_transform is None else colmap_to_world_transform
        self.poses = self.spline_indices = None
        self.device = device
        self._device_cameras = None

    @classmethod
    def from_config(cls, config, poses, bounds, focal, height, width, near, far, image_names=None, distortion_params=None,
                    device: Optional[torch.device] = None):
        """The pose branch of `LLFF._load_renderings` (datasets.py:639-681) followed by the `render_path` block of
        `BaseDataset.__init__` (:311-336), in that order, on `poses` [n,3,4] / `bounds` as the loader read them:

        forward_facing: positions and bounds scaled by 1 / (0.75 * bounds.min()), `recenter_poses`, the spiral path of
        `render_path_frames` frames, and `pixtocam_ndc` = the pinhole inverse intrinsics; otherwise `transform_poses_pca`
        and the ellipse path (`z_variation`, `z_phase`), or the spline path through `render_spline_keyframes` (which
        needs `image_names`).  Then `render_path_file` replaces the path, `render_resolution` / `render_focal` the
        camera, `render_camtype` the projection ('pano': spherical; 'perspective'; 'fisheye' raises ValueError as
        `camera_utils.pixels_to_rays` does), and the path is rendered without lens distortion.

        With `config.render_path = False` the given poses are served unchanged, with `distortion_params`: the test
        views, which the caller passes in the frame the model was trained in."""
        poses = np.array(poses, np.float64)[..., :3, :4]
        bounds = np.array(bounds, np.float64)
        pixtocams = camera_utils.get_pixtocam(focal, width, height)
        ndc = pixtocams if config.forward_facing else None
        if not config.render_path:
            return cls(pixtocams, poses, height, width, near, far, distortion_params=distortion_params, pixtocam_ndc=ndc,
                       device=device)
        poses, transform, render_poses, spline_indices = normalize_poses(config, poses, bounds, image_names)
        if config.render_path_file is not None:
            with open(config.render_path_file, 'rb') as fp:
                render_poses = np.load(fp)
        if config.render_resolution is not None:
            width, height = config.render_resolution
        if config.render_focal is not None:
            focal = config.render_focal
        spherical = False
        if config.render_camtype is not None:
            if config.render_camtype == 'pano':
                spherical = True
            elif camera_utils.ProjectionType(config.render_camtype) != camera_utils.ProjectionType.PERSPECTIVE:
                raise ValueError("only ProjectionType.PERSPECTIVE cameras are generated on the device")
        self = cls(camera_utils.get_pixtocam(focal, width, height), render_poses, height, width, near, far,
                   distortion_params=None, pixtocam_ndc=ndc, spherical=spherical, colmap_to_world_transform=transform,
                   device=device)
        self.poses, self.spline_indices = poses, spline_indices
        return self

    @property
    def cameras(self):
        return (self.pixtocams, self.camtoworlds, self.distortion_params, self.pixtocam_ndc)

    @property
    def size(self) -> int:
        return self.camtoworlds.shape[0]

    def __len__(self):
        return self.size

    def generate_ray_batch(self, cam_idx: int, first: int = 0, count: Optional[int] = None) -> utils.Batch:
        """All rays of view `cam_idx` ([H, W, .]; the flat pixel range [first, first + count) as [count, .] when given),
        cast on the device (datasets.py:487-498)."""
        if not 0 <= cam_idx < self.size:
            raise IndexError(f'view {cam_idx} outside [0, {self.size})')
        if self._device_cameras is None:                   # the one upload of the path
            dev = torch.device('cuda') if self.device is None else torch.device(self.device)
            f32 = dict(dtype=torch.float32, device=dev)
            self._device_cameras = (torch.as_tensor(self.pixtocams, **f32), torch.as_tensor(self.camtoworlds, **f32).contiguous(),
                                    None if self.pixtocam_ndc is None else torch.as_tensor(np.asarray(self.pixtocam_ndc), **f32))
        p2c, c2w, ndc = self._device_cameras
        cameras = (p2c, c2w, None, None) if self.spherical else (p2c, c2w, self.distortion_params, ndc)
        rays = camera_utils.cast_image_rays(cameras, cam_idx, self.height, self.width, self.near, self.far,
                                            spherical=self.spherical, first=first, count=count, device=c2w.device)
        return utils.Batch(rays=rays)

    def __iter__(self):
        return (self.generate_ray_batch(i) for i in range(self.size))


class TrainRayBatcher:
    """images [n, H, W, C] (device or host, float), cameras = (pixtocams [n,3,3] | [3,3], camtoworlds [n,3,4],
    distortion_params dict | None, pixtocam_ndc | None) -- the tuple `Dataset.cameras` holds in the reference
    (datasets.py:607-621); the distortion dict is shared by all cameras and applied on the device."""

    def __init__(self, images, cameras: Sequence, near: float, far: float, batch_size: int, patch_size: int = 1,
                 batching: str = 'all_images', seed: int = 0, rank: int = 0, device: Optional[torch.device] = None,
                 debug_mode: bool = False):
        if batching not in ('all_images', 'single_image'):
            raise ValueError(f'Unknown batching method {batching}')
        self.device = torch.device('cuda') if device is None else torch.device(device)
        self.images = torch.as_tensor(np.asarray(images) if not torch.is_tensor(images) else images, dtype=torch.float32).to(self.device)
        self.n_examples, self.height, self.width = self.images.shape[:3]
        pixtocams, camtoworlds, distortion, ndc = cameras
        if distortion is not None:
            camera_utils.lens_distortion(distortion)       # unknown keys raise TypeError here, not at the first batch
            distortion = dict(distortion)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.cameras = (torch.as_tensor(np.asarray(pixtocams), **f32), torch.as_tensor(np.asarray(camtoworlds), **f32)[..., :3, :4],
                        distortion, None if ndc is None else torch.as_tensor(np.asarray(ndc), **f32))
        self.near, self.far = float(near), float(far)
        self.batch_size, self.patch_size, self.batching, self.debug_mode = int(batch_size), int(patch_size), batching, debug_mode
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed) + int(rank))

    def sample_pixels(self) -> utils.Pixels:
        """datasets.py:449-485: pixel patches + camera indices of one batch, shape [num_patches, patch, patch]."""
        num_patches = self.batch_size // self.patch_size ** 2
        upper = self.patch_size - 1
        dev = self.device
        if self.debug_mode:
            xs = torch.arange(0, self.width - upper, device=dev)
            ys = torch.arange(0, self.height - upper, device=dev)
            gx, gy = torch.meshgrid(xs, ys, indexing='xy')
            px = gx.reshape(-1)[:num_patches].reshape(-1, 1, 1)
            py = gy.reshape(-1)[:num_patches].reshape(-1, 1, 1)
            cam = torch.zeros((num_patches, 1, 1), dtype=torch.int64, device=dev)
        else:
            px = torch.randint(0, self.width - upper, (num_patches, 1, 1), generator=self.gen, device=dev)
            py = torch.randint(0, self.height - upper, (num_patches, 1, 1), generator=self.gen, device=dev)
            if self.batching == 'all_images':
                cam = torch.randint(0, self.n_examples, (num_patches, 1, 1), generator=self.gen, device=dev)
            else:
                cam = torch.randint(0, self.n_examples, (1,), generator=self.gen, device=dev).reshape(1, 1, 1)
        if not self.debug_mode:                            # the reference adds the patch offsets in the random branch only (datasets.py:459-476)
            d = torch.arange(self.patch_size, device=dev)
            px = px + d.reshape(1, 1, -1)                  # patch offsets (camera_utils.pixel_coordinates)
            py = py + d.reshape(1, -1, 1)
        px, py, cam = torch.broadcast_tensors(px, py, cam)
        shape = tuple(px.shape)

        def scalar(x):
            return torch.full(shape + (1,), x, dtype=torch.float32, device=dev)
        return utils.Pixels(pix_x_int=px.to(torch.int32).contiguous(), pix_y_int=py.to(torch.int32).contiguous(), lossmult=scalar(1.),
                            near=scalar(self.near), far=scalar(self.far), cam_idx=cam.to(torch.int32)[..., None].contiguous())

    def next(self, cast_rays: bool = True) -> utils.Batch:
        """One training batch: `Batch(rays=Rays | Pixels, rgb=[..., C])`, all on the device."""
        pixels = self.sample_pixels()
        cam, py, px = pixels.cam_idx[..., 0].long(), pixels.pix_y_int.long(), pixels.pix_x_int.long()
        rgb = self.images[cam, py, px]
        rays = camera_utils.cast_ray_batch(self.cameras, pixels, device=self.device) if cast_rays else pixels
        return utils.Batch(rays=rays, rgb=rgb)

    __next__ = next

    def __iter__(self):
        return self


# ------------------------------------------------------------------------------------------------
# The scene loaders (datasets.py:44-54, 155-189, 519-708).

UNBUILT_LOADERS = ('tat_nerfpp', 'tat_fvs', 'dtu', 'rffr')
SPLITS = ('train', 'val', 'test')


def load_blender_posedata(data_dir, split=None):
    """Poses and intrinsics of a `transforms.json` file, as used in Blender / NGP datasets (datasets.py:155-189):
    (names, poses [n,4,4] float32, pixtocam [3,3] float64, distortion_params | None, camtype).  Frames whose file does
    not exist are skipped, as there."""
    suffix = '' if split is None else f'_{split}'
    with open(os.path.join(data_dir, f'transforms{suffix}.json'), 'r') as fp:
        meta = json.load(fp)
    names, poses = [], []
    for frame in meta['frames']:
        if os.path.exists(os.path.join(data_dir, frame['file_path'])):
            names.append(frame['file_path'].split('/')[-1])
            poses.append(np.array(frame['transform_matrix'], dtype=np.float32))
    poses = np.stack(poses, axis=0)
    w, h = meta['w'], meta['h']
    cx = meta['cx'] if 'cx' in meta else w / 2.
    cy = meta['cy'] if 'cy' in meta else h / 2.
    fx = meta['fl_x'] if 'fl_x' in meta else 0.5 * w / np.tan(0.5 * float(meta['camera_angle_x']))
    fy = meta['fl_y'] if 'fl_y' in meta else 0.5 * h / np.tan(0.5 * float(meta['camera_angle_y']))
    pixtocam = np.linalg.inv(camera_utils.intrinsic_matrix(fx, fy, cx, cy))
    coeffs = ['k1', 'k2', 'p1', 'p2']
    params = {c: (meta[c] if c in meta else 0.) for c in coeffs} if any(c in meta for c in coeffs) else None
    return names, poses, pixtocam, params, camera_utils.ProjectionType.PERSPECTIVE


def read_image_stack(paths) -> np.ndarray:
    """The files decoded with PIL (`utils.load_img`'s decoder) into one stack [n,H,W(,C)]: uint8 as stored where every
    file decodes to uint8 (the PNGs), float32 otherwise (the disparity TIFFs), which is what `load_img` casts to."""
    from PIL import Image
    frames = []
    for pth in paths:
        with open(pth, 'rb') as f:
            frames.append(np.array(Image.open(f)))
    if any(f.shape != frames[0].shape for f in frames):
        raise ValueError(f'images of different shapes in one stack: {paths[0]} ...')
    if not all(f.dtype == np.uint8 for f in frames):
        frames = [f.astype(np.float32) for f in frames]
    return np.stack(frames, axis=0)


def prepare_images_host(src, op: int, factor: int = 1, return_alpha: bool = False):
    """refnerf_prepare_images in numpy float32, in the reference's operation order: `image.downsample` (a block mean:
    float32(sum) / float32(factor^2); uint8 blocks are summed as integers, which is numpy's float32 sum exactly while
    factor^2 * 255 < 2^24; float32 images go through the reference's own `reshape(...).mean((1, 3))`, image by image),
    then `/ 255.` (PREP_SCALE), that and `rgb * alpha + (1. - alpha)` (PREP_WHITE), `[..., :3] * 2. / 255. - 1.`
    (PREP_NORMALS) or nothing (PREP_RAW).  numpy arrays in and out."""
    src = np.asarray(src)
    f = int(factor)
    n, H, W = src.shape[:3]
    if f < 1 or H % f or W % f:
        raise ValueError(f'Downsampling factor {f} does not evenly divide image shape {(H, W)}')
    if f > 256:
        raise ValueError(f'Downsampling factor {f} above 256: a block sum of factor^2 bytes must stay below 2^24')
    if src.dtype == np.uint8:
        if f > 1:
            sums = src.reshape((n, H // f, f, W // f, f) + src.shape[3:]).sum((2, 4), dtype=np.uint32)
            mean = sums.astype(np.float32) / np.float32(f * f)
        else:
            mean = src.astype(np.float32)
    else:
        mean = src.astype(np.float32)
        if f > 1:
            mean = np.stack([im.reshape((H // f, f, W // f, f) + im.shape[2:]).mean((1, 3)) for im in mean], axis=0)
    alpha = None
    if op == _hip.PREP_RAW:
        out = mean
    elif op == _hip.PREP_SCALE:
        out = mean / 255.
    elif op == _hip.PREP_NORMALS:
        if mean.ndim != 4 or mean.shape[3] < 3:
            raise ValueError('PREP_NORMALS needs at least 3 channels')
        out = mean[..., :3] * 2. / 255. - 1.
    elif op == _hip.PREP_WHITE:
        if mean.ndim != 4 or mean.shape[3] != 4:
            raise ValueError('PREP_WHITE needs RGBA images')
        v = mean / 255.
        rgb, a = v[..., :3], v[..., -1:]
        out = rgb * a + (1. - a)
        alpha = v[..., -1]
    else:
        raise ValueError(f'unknown operation {op}')
    assert out.dtype == np.float32
    return (out, alpha) if return_alpha else out


def prepare_images(src, op: int, factor: int = 1, return_alpha: bool = False, device=None):
    """A decoded stack (numpy, uint8 or float32) -> the prepared float32 stack as a tensor on `device`: uploaded as it
    was decoded and prepared there in one launch (refnerf_prepare_images), or, for the host, `prepare_images_host`."""
    device = torch.device('cuda') if device is None else torch.device(device)
    f = int(factor)
    if f < 1 or src.shape[1] % f or src.shape[2] % f:       # the reference's error (image.py:76-78), before any upload
        raise ValueError(f'Downsampling factor {f} does not evenly divide image shape {tuple(src.shape[1:3])}')
    if device.type == 'cpu':
        res = prepare_images_host(src, op, f, return_alpha)
        return tuple(torch.from_numpy(np.ascontiguousarray(r)) for r in res) if return_alpha else torch.from_numpy(np.ascontiguousarray(res))
    return _hip.prepare_images(torch.from_numpy(np.ascontiguousarray(src)).to(device), op, f, return_alpha)


class SceneDataset:
    """The loaded state of the reference's `BaseDataset` (datasets.py:208-516) and its batches.

    Set by the subclass's `_load_renderings`: `images` [n,H,W,3], `disp_images` [n,H,W], `normal_images` [n,H,W,3],
    `alphas` [n,H,W] (float32 tensors on `device`, or None), `camtoworlds`, `pixtocams`, `pixtocam_ndc`, `poses`,
    `colmap_to_world_transform` (host numpy arrays, the reference's dtypes), `distortion_params`, `height`, `width`,
    `focal`; from the config `near`, `far`, `split`; `size` views, `cameras` the reference's tuple.

    `next()` is `_next_fn`: a random (or, in `dataset_debug_mode`, the deterministic) training batch for 'train', the next
    whole view for 'val' / 'test'.  `seed` / `rank` seed the per-rank device generator of the training pixels."""

    def __init__(self, split: str, data_dir: str, config, device: Optional[torch.device] = None, seed: int = 0, rank: int = 0):
        self.config = config
        self._patch_size = max(int(config.patch_size), 1)
        self._batch_size = int(config.batch_size)
        if self._patch_size ** 2 > self._batch_size:
            raise ValueError(f'Patch size {self._patch_size}^2 too large for per-process batch size {self._batch_size}')
        if config.batching not in ('all_images', 'single_image'):
            raise ValueError(f'{config.batching!r} is not a valid BatchingMethod')
        if split not in SPLITS:
            raise ValueError(f'{split!r} is not a valid DataSplit')
        self._batching = config.batching
        self._load_disps, self._load_normals = bool(config.compute_disp_metrics), bool(config.compute_normal_metrics)
        self._val_camera_idx = self._test_camera_idx = 0
        self._cast_rays_in_train_step = bool(config.cast_rays_in_train_step)
        self._debug_mode = bool(config.dataset_debug_mode)
        self.device = torch.device('cuda') if device is None else torch.device(device)
        self.split, self.data_dir = split, data_dir
        self.near, self.far = config.near, config.far
        self.render_path = bool(config.render_path)
        self.distortion_params = self.disp_images = self.normal_images = self.alphas = self.poses = self.pixtocam_ndc = None
        self.camtype = camera_utils.ProjectionType.PERSPECTIVE
        self.colmap_to_world_transform = np.eye(4)
        self.images = self.camtoworlds = self.pixtocams = self.height = self.width = self.focal = None
        self._path = None                                  # the PathCameras of a render path (LLFF)

        self._load_renderings(config)

        if self.distortion_params is not None:
            camera_utils.lens_distortion(self.distortion_params)   # unknown keys raise TypeError here, not at the first batch
        self._n_examples = self.camtoworlds.shape[0]
        self.cameras = (self.pixtocams, self.camtoworlds, self.distortion_params, self.pixtocam_ndc)
        self._device_cameras = self._debug_origins = None
        self._batcher = None
        if self.split == 'train' and self.images is not None and not self.render_path:
            # the yardstick's sampler, and its generator: the fused batch draws from it what `sample_pixels` draws
            self._batcher = TrainRayBatcher(self.images, self.cameras, self.near, self.far, self._batch_size, self._patch_size,
                                            self._batching, seed=seed, rank=rank, device=self.device, debug_mode=self._debug_mode)

    def _load_renderings(self, config):
        raise NotImplementedError

    @property
    def size(self) -> int:
        return self._n_examples

    def __len__(self):
        """datasets.py:196-202: the batches of one pass over the training pixels, or the number of views."""
        if self.split == 'train':
            n, h, w = self.images.shape[:3]
            return (n * h * w // self._batch_size) * getattr(self.config, 'num_gpus', 1)
        return self._n_examples

    def _cameras_on_device(self):
        """(pixtocams, camtoworlds [n,3,4], pixtocam_ndc | None, LensDistortion | None): the one upload of the cameras."""
        if self._device_cameras is None:
            dev = self.device if self.device.type != 'cpu' else torch.device('cuda')
            f32 = dict(dtype=torch.float32, device=dev)
            self._device_cameras = (
                torch.as_tensor(np.asarray(self.pixtocams), **f32).contiguous(),
                torch.as_tensor(np.asarray(self.camtoworlds), **f32)[..., :3, :4].contiguous(),
                None if self.pixtocam_ndc is None else torch.as_tensor(np.asarray(self.pixtocam_ndc), **f32).contiguous(),
                None if self.distortion_params is None else camera_utils.lens_distortion(self.distortion_params))
        return self._device_cameras

    def _side_stacks(self):
        """The optional stacks a batch carries (datasets.py:442-446), cut to the views `images` kept."""
        n = self.images.shape[0]
        return dict(disps=self.disp_images[:n] if self._load_disps else None,
                    normals=self.normal_images[:n] if self._load_normals else None,
                    alphas=self.alphas[:n] if self._load_normals else None)

    def _patch_origins(self):
        """[P] x, y and [P] | [1] camera indices of the batch's patches and the patch size the kernel expands: the draws of
        `TrainRayBatcher.sample_pixels`, from its generator, in its order; in debug mode its deterministic pixels, which
        the reference does not expand into patches (datasets.py:458-464)."""
        num_patches = self._batch_size // self._patch_size ** 2
        upper = self._patch_size - 1
        dev = self.device
        if self._debug_mode:
            if self._debug_origins is None:
                gx, gy = torch.meshgrid(torch.arange(0, self.width - upper, device=dev),
                                        torch.arange(0, self.height - upper, device=dev), indexing='xy')
                px, py = gx.reshape(-1)[:num_patches].contiguous(), gy.reshape(-1)[:num_patches].contiguous()
                self._debug_origins = (px, py, torch.zeros_like(px))
            return self._debug_origins + (1,)
        gen = self._batcher.gen
        px = torch.randint(0, self.width - upper, (num_patches, 1, 1), generator=gen, device=dev)
        py = torch.randint(0, self.height - upper, (num_patches, 1, 1), generator=gen, device=dev)
        cam = torch.randint(0, self._n_examples, (num_patches, 1, 1) if self._batching == 'all_images' else (1,),
                            generator=gen, device=dev)
        return px.reshape(-1), py.reshape(-1), cam.reshape(-1), self._patch_size

    def _next_train(self, cast_rays: Optional[bool] = None) -> utils.Batch:
        """One training batch (datasets.py:449-485): `Batch(rays, rgb[, disps, normals, alphas])`, shaped
        [num_patches, patch, patch, .]; with `cast_rays=False` (the default under `Config.cast_rays_in_train_step`) the
        rays are the `Pixels`, to be cast in the training step."""
        if self._batcher is None:
            raise ValueError('training batches need the images of a train split (not a render path)')
        if cast_rays is None:
            cast_rays = not self._cast_rays_in_train_step
        side = self._side_stacks()
        if not cast_rays or self.device.type == 'cpu':     # the ATen steps of the yardstick
            pixels = self._batcher.sample_pixels()
            cam, py, px = pixels.cam_idx[..., 0].long(), pixels.pix_y_int.long(), pixels.pix_x_int.long()
            rays = camera_utils.cast_ray_batch(self._batcher.cameras, pixels) if cast_rays else pixels
            return utils.Batch(rays=rays, rgb=self.images[cam, py, px],
                               **{k: None if v is None else v[cam, py, px] for k, v in side.items()})
        px0, py0, cam, ps = self._patch_origins()
        p2c, c2w, ndc, dist = self._cameras_on_device()
        rays, got = _hip.train_batch(px0, py0, cam, ps, self.images, p2c, c2w, self.near, self.far, pixtocam_ndc=ndc,
                                     distortion=dist, **side)
        return utils.Batch(rays=utils.Rays(**rays), **got)

    def generate_ray_batch(self, cam_idx: int) -> utils.Batch:
        """All rays of view `cam_idx`, cast in one launch, with views (no copies) of the resident stacks
        (datasets.py:487-498)."""
        if self._path is not None:
            return self._path.generate_ray_batch(cam_idx)
        if not 0 <= cam_idx < self.size:
            raise IndexError(f'view {cam_idx} outside [0, {self.size})')
        p2c, c2w, ndc, _ = self._cameras_on_device()
        rays = camera_utils.cast_image_rays((p2c, c2w, self.distortion_params, ndc), cam_idx, self.height, self.width,
                                            self.near, self.far, device=c2w.device)
        batch = utils.Batch(rays=rays)
        if not self.render_path:
            batch.rgb = self.images[cam_idx]
        if self._load_disps:
            batch.disps = self.disp_images[cam_idx]
        if self._load_normals:
            batch.normals, batch.alphas = self.normal_images[cam_idx], self.alphas[cam_idx]
        return batch

    def _next_val(self) -> utils.Batch:
        """datasets.py:500-509: the next view; `dataset_debug_mode` pins view 0."""
        if self._debug_mode:
            cam_idx = self._val_camera_idx = 0
        else:
            cam_idx = self._val_camera_idx
            self._val_camera_idx = (self._val_camera_idx + 1) % self._n_examples
        return self.generate_ray_batch(cam_idx)

    def _next_test(self) -> utils.Batch:
        """datasets.py:511-516"""
        cam_idx = self._test_camera_idx
        self._test_camera_idx = (self._test_camera_idx + 1) % self._n_examples
        return self.generate_ray_batch(cam_idx)

    def next(self, cast_rays: Optional[bool] = None) -> utils.Batch:
        if self.split == 'train':
            return self._next_train(cast_rays)
        return self._next_val() if self.split == 'val' else self._next_test()

    def __next__(self):
        return self.next()

    def __iter__(self):
        return self

    def __getitem__(self, index):
        return self.next()


class ArrayScene(SceneDataset):
    """A `SceneDataset` over images and cameras the caller already holds -- what `TrainRayBatcher` takes: `images`
    [n,H,W,3] (device or host, float) and the reference's cameras tuple (pixtocams [3,3] | [n,3,3], camtoworlds, distortion
    dict | None, pixtocam_ndc | None); optional `disp_images` [n,H,W], `normal_images` [n,H,W,3], `alphas` [n,H,W], which
    the batches then carry whatever the config's metric switches say."""

    def __init__(self, config, images, cameras: Sequence, split: str = 'train', disp_images=None, normal_images=None,
                 alphas=None, device: Optional[torch.device] = None, seed: int = 0, rank: int = 0):
        if (normal_images is None) != (alphas is None):
            raise ValueError('normal_images and alphas come together (datasets.py:444-446)')
        self._arrays = (images, cameras, disp_images, normal_images, alphas)
        super().__init__(split, None, config, device=device, seed=seed, rank=rank)

    def _load_renderings(self, config):
        images, cameras, disps, normals, alphas = self._arrays
        del self._arrays

        def resident(x):
            if x is None:
                return None
            return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x, dtype=torch.float32).to(self.device).contiguous()
        self.images, self.disp_images, self.normal_images, self.alphas = (resident(x) for x in (images, disps, normals, alphas))
        self._load_disps, self._load_normals = disps is not None, normals is not None
        pixtocams, camtoworlds, self.distortion_params, self.pixtocam_ndc = cameras
        host = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)   # noqa: E731
        self.pixtocams, self.camtoworlds = host(pixtocams), host(camtoworlds)
        if self.pixtocam_ndc is not None:
            self.pixtocam_ndc = host(self.pixtocam_ndc)
        self.height, self.width = self.images.shape[1:3]
        self.focal = 1. / self.pixtocams.reshape(-1, 3, 3)[0, 0, 0]


class Blender(SceneDataset):
    """`nerf_synthetic`-style scenes (datasets.py:519-581): `transforms_<split>.json`, RGBA PNGs composited on white,
    optional `_disp.tiff` / `_normal.png` per frame."""

    def _load_renderings(self, config):
        if config.render_path:
            raise ValueError('render_path cannot be used for the blender dataset.')
        if config.use_tiffs:
            raise ValueError('use_tiffs (linear-light TIFF channels) is not built; see INTEGRATION.md')
        with open(os.path.join(self.data_dir, f'transforms_{self.split}.json'), 'r') as fp:
            meta = json.load(fp)
        prefixes = [os.path.join(self.data_dir, frame['file_path']) for frame in meta['frames']]
        factor = config.factor if config.factor > 1 else 1
        rgba = read_image_stack([p + '.png' for p in prefixes])
        if rgba.ndim != 4 or rgba.shape[3] != 4:
            raise ValueError(f'the blender loader needs RGBA images, got shape {rgba.shape[1:]}')
        self.images, alphas = prepare_images(rgba, _hip.PREP_WHITE, factor, return_alpha=True, device=self.device)
        if self._load_disps:
            self.disp_images = prepare_images(read_image_stack([p + '_disp.tiff' for p in prefixes]), _hip.PREP_RAW, factor,
                                              device=self.device)
        if self._load_normals:
            self.normal_images = prepare_images(read_image_stack([p + '_normal.png' for p in prefixes]), _hip.PREP_NORMALS,
                                                factor, device=self.device)
            self.alphas = alphas
        self.camtoworlds = np.stack([np.array(frame['transform_matrix'], dtype=np.float32) for frame in meta['frames']], axis=0)
        if self.split == 'train' and config.n_input_views > 0:
            self.images = self.images[:config.n_input_views]
            self.camtoworlds = self.camtoworlds[:config.n_input_views]
        self.height, self.width = self.images.shape[1:3]
        self.focal = .5 * self.width / np.tan(.5 * float(meta['camera_angle_x']))
        # the reference's get_pixtocam (camera_utils.py:393-399) stays float64; the device sees its float32 rounding
        self.pixtocams = np.linalg.inv(camera_utils.intrinsic_matrix(self.focal, self.focal, self.width * .5, self.height * .5))


class LLFF(SceneDataset):
    """LLFF / real forward-facing and 360 scenes with `transforms.json` poses (datasets.py:584-708)."""

    def _load_renderings(self, config):
        image_dir_suffix, factor = '', 1
        if config.factor > 1:
            image_dir_suffix, factor = f'_{config.factor}', config.factor
        if os.path.exists(os.path.join(self.data_dir, 'sparse/0/')):
            raise ValueError(f"{os.path.join(self.data_dir, 'sparse/0')}: COLMAP reconstructions need pycolmap, which is not "
                             "built; export the poses to transforms.json (see INTEGRATION.md)")
        image_names, poses, pixtocam, distortion_params, camtype = load_blender_posedata(self.data_dir)
        if config.load_alphabetical:
            inds = np.argsort(image_names)
            image_names = [image_names[i] for i in inds]
            poses = poses[inds]
        pixtocam = pixtocam @ np.diag([factor, factor, 1.])
        self.pixtocams = pixtocam.astype(np.float32)
        self.focal = 1. / self.pixtocams[0, 0]
        self.distortion_params, self.camtype = distortion_params, camtype

        colmap_image_dir = os.path.join(self.data_dir, 'images')
        image_dir = os.path.join(self.data_dir, 'images' + image_dir_suffix)
        for d in [image_dir, colmap_image_dir]:
            if not os.path.exists(d):
                raise ValueError(f'Image folder {d} does not exist.')
        # downsampled images may have other names than the ones the poses name: map between the two sorted lists
        colmap_to_image = dict(zip(sorted(os.listdir(colmap_image_dir)), sorted(os.listdir(image_dir))))
        image_paths = [os.path.join(image_dir, colmap_to_image[f]) for f in image_names]

        posefile = os.path.join(self.data_dir, 'poses_bounds.npy')
        if os.path.exists(posefile):
            with open(posefile, 'rb') as fp:
                bounds = np.load(fp)[:, -2:]
        else:
            bounds = np.array([0.01, 1.])
        if config.forward_facing:
            self.pixtocam_ndc = self.pixtocams.reshape(-1, 3, 3)[0]
        raw = (poses.copy(), bounds.copy()) if config.render_path else None   # normalize_poses scales in place
        poses, self.colmap_to_world_transform, self.render_poses, spline_indices = normalize_poses(config, poses, bounds, image_names)
        if spline_indices is not None:
            self.spline_indices = spline_indices
        self.poses = poses

        all_indices = np.arange(len(image_paths))
        train_indices = all_indices if config.llff_use_all_images_for_training else all_indices[all_indices % config.llffhold != 0]
        held_out = all_indices[all_indices % config.llffhold == 0]
        indices = {'val': held_out, 'test': held_out, 'train': train_indices}[self.split]
        if self.split == 'train' and config.n_input_views > 0:
            n_input_views = min(config.n_input_views, len(indices))
            indices = indices[[round(i) for i in np.linspace(0, len(indices) - 1, n_input_views)]]
        # only the views of the split are decoded and uploaded; the reference loads all and indexes (:696-704)
        self.images = prepare_images(read_image_stack([image_paths[i] for i in indices]), _hip.PREP_SCALE, 1, device=self.device)
        self.height, self.width = self.images.shape[1:3]
        self.camtoworlds = poses[indices]
        if config.render_path:
            # the `render_path` block of BaseDataset.__init__ (:311-336) lives in PathCameras.from_config, which normalises
            # the loaded poses in float64 through the same normalize_poses; the dataset serves that path's views
            self._path = PathCameras.from_config(config, raw[0], raw[1], self.focal, self.height, self.width, self.near, self.far,
                                                 image_names=image_names,
                                                 device=None if self.device.type == 'cpu' else self.device)
            self.camtoworlds, self.pixtocams = self._path.camtoworlds, self._path.pixtocams
            self.height, self.width = self._path.height, self._path.width
            self.distortion_params, self.pixtocam_ndc = None, self._path.pixtocam_ndc


def load_dataset(split, data_dir, config, device=None, **kwargs) -> SceneDataset:
    """A split of a scene, by the loader `config.dataset_loader` names (datasets.py:44-54)."""
    loaders = {'blender': Blender, 'llff': LLFF}
    if config.dataset_loader in UNBUILT_LOADERS:
        raise ValueError(f"dataset_loader {config.dataset_loader!r} is not built: only {sorted(loaders)} are (see INTEGRATION.md)")
    if config.dataset_loader not in loaders:
        raise ValueError(f"unknown dataset_loader {config.dataset_loader!r}")
    return loaders[config.dataset_loader](split, data_dir, config, device=device, **kwargs)

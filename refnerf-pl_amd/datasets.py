"""The random-ray training batcher in front of the hot path, on the device (second half).

Mirrors `Dataset._next_train` / `Dataset._make_ray_batch` of the reference's internal/datasets.py (:395-485) for
perspective cameras (optionally with lens distortion) with `Config.cast_rays_in_train_step` semantics (configs.py:80): a
batch is `batch_size // patch_size**2` random pixel patches drawn from all images ('all_images') or from one random image
('single_image'); the colours are gathered and the rays cast (`camera_utils.cast_ray_batch` -> `refnerf_pixels_to_rays`,
or `refnerf_pixels_to_rays_distorted` when the cameras carry a distortion dict) on the device, so
a training step moves no per-ray data over PCIe.  `PathCameras` is the other half: the render-path / test views of
`BaseDataset` (:311-336, 487-498) with the pose normalisation and path generation of `LLFF._load_renderings` (:639-681),
whole frames cast in one launch each.  The file loaders (COLMAP / LLFF images) stay out of scope.

Random numbers: a `torch.Generator` on the device, seeded per rank (`seed + rank`): the reference draws from the global
`numpy.random` state, which every DDP rank and DataLoader worker inherits identically -- not
reproduced on purpose.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import camera_utils, utils


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

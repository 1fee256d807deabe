"""Ray generation in front of the hot path, on the device.

Mirrors the call surface of the reference's internal/camera_utils.py for the part
the Ref-NeRF configs use: `pixels_to_rays` (:502-614), `cast_ray_batch` (:617-670),
`cast_pinhole_rays` (:673-697), `pixel_coordinates` / `get_pixtocam` (:380-406).
Perspective cameras, with or without radial-tangential lens distortion
(`distortion_params`, :409-493 and :558-565); the NDC conversion (:31-97) is
included.  The arithmetic runs in one HIP kernel (refnerf_pixels_to_rays, or
refnerf_pixels_to_rays_distorted): pixel indices in, the `Rays` fields out, so
whole-image rendering neither casts rays with numpy on the host nor copies
64 B/ray over PCIe.

A whole frame needs no pixel indices at all: `cast_image_rays` / `cast_spherical_rays` (:700-746) write the nine
`Rays` fields of a frame, or of a flat pixel range of it, in one launch of refnerf_image_rays from (width, height,
camera, pose).  The poses themselves come from the host-side path functions of the same reference file (:100-377:
spiral, ellipse and spline paths, pose recentring), restated here in numpy float64.
"""
import enum
import operator
import os

import numpy as np
import torch

from . import _hip, utils


class ProjectionType(enum.Enum):
    """camera_utils.py:493-496"""
    PERSPECTIVE = 'perspective'
    FISHEYE = 'fisheye'


# ------------------------------------------------------------------------------------------------
# Poses and render paths (camera_utils.py:100-377): host side, numpy float64, O(frames) numbers.

def pad_poses(p):
    """[..., 3, 4] poses -> [..., 4, 4] with the homogeneous row (0, 0, 0, 1) (camera_utils.py:100-103)."""
    bottom = np.broadcast_to([0, 0, 0, 1.], p[..., :1, :4].shape)
    return np.concatenate([p[..., :3, :4], bottom], axis=-2)


def unpad_poses(p):
    """Drop the homogeneous row again (camera_utils.py:106-108)."""
    return p[..., :3, :4]


def recenter_poses(poses):
    """Express the poses in the frame of their average pose: (poses [n,3,4], transform [4,4]) (camera_utils.py:111-116)."""
    transform = np.linalg.inv(pad_poses(average_pose(poses)))
    return unpad_poses(transform @ pad_poses(poses)), transform


def average_pose(poses):
    """The look-at pose of the mean position, mean z axis and mean up vector (camera_utils.py:119-125)."""
    return viewmatrix(poses[:, :3, 2].mean(0), poses[:, :3, 1].mean(0), poses[:, :3, 3].mean(0))


def viewmatrix(lookdir, up, position):
    """Look-at camera-to-world matrix [3,4] (camera_utils.py:128-135)."""
    z = normalize(lookdir)
    x = normalize(np.cross(up, z))
    y = normalize(np.cross(z, x))
    return np.stack([x, y, z, position], axis=1)


def normalize(x):
    """camera_utils.py:138-140"""
    return x / np.linalg.norm(x)


def focus_point_fn(poses):
    """The point nearest, in least squares, to all the cameras' focal axes (camera_utils.py:143-149)."""
    directions, origins = poses[:, :3, 2:3], poses[:, :3, 3:4]
    m = np.eye(3) - directions * np.transpose(directions, [0, 2, 1])
    mt_m = np.transpose(m, [0, 2, 1]) @ m
    return np.linalg.inv(mt_m.mean(0)) @ (mt_m @ origins).mean(0)[:, 0]


# generate_spiral_path (camera_utils.py:152-155)
NEAR_STRETCH = .9      # push the near bound forward
FAR_STRETCH = 5.       # push the far bound back
FOCUS_DISTANCE = .75   # weight of the far bound in the focus depth


def generate_spiral_path(poses, bounds, n_frames=120, n_rots=2, zrate=.5):
    """Forward-facing spiral around the average pose, every camera looking at (0, 0, -focus depth) of that pose;
    the focus depth is a disparity-space mean of the stretched bounds, the spiral radii the 90th percentile of the
    camera positions (camera_utils.py:158-188).  Returns [n_frames, 3, 4]."""
    near_bound = bounds.min() * NEAR_STRETCH
    far_bound = bounds.max() * FAR_STRETCH
    focal = 1 / (((1 - FOCUS_DISTANCE) / near_bound + FOCUS_DISTANCE / far_bound))
    radii = np.concatenate([np.percentile(np.abs(poses[:, :3, 3]), 90, 0), [1.]])
    cam2world = average_pose(poses)
    up = poses[:, :3, 1].mean(0)
    lookat = cam2world @ [0, 0, -focal, 1.]
    path = []
    for theta in np.linspace(0., 2. * np.pi * n_rots, n_frames, endpoint=False):
        position = cam2world @ (radii * [np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.])
        path.append(viewmatrix(position - lookat, up, position))
    return np.stack(path, axis=0)


def transform_poses_pca(poses):
    """Rotate the poses so the principal axes of the camera positions lie on x, y, z (largest first), flip so that the
    mean camera's y axis points up in z, and scale the positions into [-1, 1]^3 (camera_utils.py:191-227).
    Returns (poses [n,3,4], transform [4,4])."""
    t = poses[:, :3, 3]
    t_mean = t.mean(axis=0)
    t = t - t_mean
    eigval, eigvec = np.linalg.eig(t.T @ t)
    rot = eigvec[:, np.argsort(eigval)[::-1]].T
    if np.linalg.det(rot) < 0:
        rot = np.diag(np.array([1, 1, -1])) @ rot
    transform = np.concatenate([rot, rot @ -t_mean[:, None]], -1)
    recentered = unpad_poses(transform @ pad_poses(poses))
    transform = np.concatenate([transform, np.eye(4)[3:]], axis=0)
    if recentered.mean(axis=0)[2, 1] < 0:
        recentered = np.diag(np.array([1, -1, -1])) @ recentered
        transform = np.diag(np.array([1, -1, -1, 1])) @ transform
    scale_factor = 1. / np.max(np.abs(recentered[:, :3, 3]))
    recentered[:, :3, 3] *= scale_factor
    transform = np.diag(np.array([scale_factor] * 3 + [1])) @ transform
    return recentered, transform


def generate_ellipse_path(poses, n_frames=120, const_speed=True, z_variation=0., z_phase=0.):
    """Inward-facing ellipse in the z = 0 plane, symmetric in xy about the cameras' focus point, with axes from the
    90th percentile of the camera offsets and an optional height wave between the 10th / 90th height percentiles;
    `const_speed` resamples the angles by arc length with stepfun.sample (camera_utils.py:230-278)."""
    center = focus_point_fn(poses)
    offset = np.array([center[0], center[1], 0])
    sc = np.percentile(np.abs(poses[:, :3, 3] - offset), 90, axis=0)
    low, high = -sc + offset, sc + offset
    z_low = np.percentile((poses[:, :3, 3]), 10, axis=0)
    z_high = np.percentile((poses[:, :3, 3]), 90, axis=0)

    def get_positions(theta):
        return np.stack([low[0] + (high - low)[0] * (np.cos(theta) * .5 + .5),
                         low[1] + (high - low)[1] * (np.sin(theta) * .5 + .5),
                         z_variation * (z_low[2] + (z_high - z_low)[2] * (np.cos(theta + 2 * np.pi * z_phase) * .5 + .5))], -1)

    theta = np.linspace(0, 2. * np.pi, n_frames + 1, endpoint=True)
    positions = get_positions(theta)
    if const_speed:
        from . import stepfun
        lengths = np.linalg.norm(positions[1:] - positions[:-1], axis=-1)
        theta = stepfun.sample(torch.tensor(theta), torch.log(torch.tensor(lengths)), n_frames + 1).numpy()
        positions = get_positions(theta)
    positions = positions[:-1]                             # the last one repeats the first

    avg_up = poses[:, :3, 1].mean(0)
    avg_up = avg_up / np.linalg.norm(avg_up)
    ind_up = np.argmax(np.abs(avg_up))
    up = np.eye(3)[ind_up] * np.sign(avg_up[ind_up])       # the axis closest to the mean up vector
    return np.stack([viewmatrix(p - center, up, p) for p in positions])


def generate_interpolated_path(poses, n_interp, spline_degree=5, smoothness=.03, rot_weight=.1):
    """Smoothing B-spline through keyframe poses [n,3,4], fitted to (position, look-at point, up point) triples with
    the two points `rot_weight` away from the position; n_interp * (n - 1) poses back (camera_utils.py:281-328)."""
    import scipy.interpolate
    pos = poses[:, :3, -1]
    points = np.stack([pos, pos - rot_weight * poses[:, :3, 2], pos + rot_weight * poses[:, :3, 1]], 1)
    n = n_interp * (points.shape[0] - 1)
    sh = points.shape
    k = min(spline_degree, sh[0] - 1)
    tck, _ = scipy.interpolate.splprep(np.reshape(points, (sh[0], -1)).T, k=k, s=smoothness)
    new_points = np.array(scipy.interpolate.splev(np.linspace(0, 1, n, endpoint=False), tck))
    new_points = np.reshape(new_points.T, (n, sh[1], sh[2]))
    return np.array([viewmatrix(p - l, u - p, p) for p, l, u in new_points])


def interpolate_1d(x, n_interp, spline_degree, smoothness):
    """A 1-d signal resampled n_interp times finer through a smoothing spline (camera_utils.py:331-340)."""
    import scipy.interpolate
    tck = scipy.interpolate.splrep(np.linspace(0, 1, len(x), endpoint=True), x, s=smoothness, k=spline_degree)
    return scipy.interpolate.splev(np.linspace(0, 1, n_interp * (len(x) - 1), endpoint=False), tck)


def create_render_spline_path(config, image_names, poses):
    """The spline path through the poses whose image names `config.render_spline_keyframes` lists (a directory of
    images, or a text file with one name per line): (spline_indices, render_poses) (camera_utils.py:343-377)."""
    if os.path.isdir(config.render_spline_keyframes):
        keyframe_names = sorted(os.listdir(config.render_spline_keyframes))
    else:
        with open(config.render_spline_keyframes, 'rb') as fp:
            keyframe_names = fp.read().decode('utf-8').splitlines()
    spline_indices = np.array([i for i, n in enumerate(image_names) if n in keyframe_names])
    render_poses = generate_interpolated_path(poses[spline_indices], n_interp=config.render_spline_n_interp,
                                              spline_degree=config.render_spline_degree,
                                              smoothness=config.render_spline_smoothness, rot_weight=.1)
    return spline_indices, render_poses


def intrinsic_matrix(fx, fy, cx, cy):
    """camera_utils.py:379-386"""
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.]])


def get_pixtocam(focal, width, height):
    """Inverse intrinsic matrix for a perfect pinhole camera (camera_utils.py:389-393)."""
    return np.linalg.inv(intrinsic_matrix(focal, focal, width * .5, height * .5)).astype(np.float32)


def pixel_coordinates(width, height, device):
    """Tuple of the x and y integer coordinates for a grid of pixels (camera_utils.py:396-400)."""
    y, x = torch.meshgrid(torch.arange(height, dtype=torch.int32, device=device),
                          torch.arange(width, dtype=torch.int32, device=device), indexing='ij')
    return x, y


def _dev(x, device, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x, dtype=dtype).to(device)


# the keyword parameters of camera_utils._radial_and_tangential_undistort and their defaults (:462-469)
DISTORTION_DEFAULTS = dict(k1=0., k2=0., k3=0., k4=0., p1=0., p2=0., eps=1e-9, max_iterations=10)


def lens_distortion(distortion_params) -> _hip.LensDistortion:
    """A `distortion_params` dict (shared by all cameras) -> refnerf_lens_distortion.  Missing keys take the reference's
    defaults; an unknown key raises TypeError, as the reference's `**distortion_params` call does."""
    unknown = [k for k in distortion_params if k not in DISTORTION_DEFAULTS]
    if unknown:
        raise TypeError(f"_radial_and_tangential_undistort() got an unexpected keyword argument {unknown[0]!r}")
    p = {**DISTORTION_DEFAULTS, **distortion_params}
    return _hip.LensDistortion(*(float(p[k]) for k in ("k1", "k2", "k3", "k4", "p1", "p2", "eps")),
                               operator.index(p["max_iterations"]))


def pixels_to_rays(pix_x_int, pix_y_int, pixtocams, camtoworlds, distortion_params=None, pixtocam_ndc=None,
                   camtype=ProjectionType.PERSPECTIVE, xnp=torch, device=None):
    """camera_utils.pixels_to_rays: returns (origins, directions, viewdirs [SH,3], radii [SH,1],
    imageplane [SH,2]) as device tensors.  `pixtocams` / `camtoworlds` are one camera ([3,3] / [3,4])
    or one per pixel (SH + [3,3] / SH + [3,4]); `distortion_params` is None or one dict for all of them."""
    del xnp
    dist = None if distortion_params is None else lens_distortion(distortion_params)
    if camtype != ProjectionType.PERSPECTIVE:
        raise ValueError("only ProjectionType.PERSPECTIVE cameras are generated on the device")
    if device is None:
        device = pix_x_int.device if torch.is_tensor(pix_x_int) and pix_x_int.is_cuda else torch.device("cuda")
    px = _dev(pix_x_int, device, torch.int32)
    py = _dev(pix_y_int, device, torch.int32)
    sh = tuple(px.shape)
    p2c = _dev(pixtocams, device)
    c2w = _dev(camtoworlds, device)[..., :3, :4]
    if p2c.dim() > 2:
        p2c = torch.broadcast_to(p2c, sh + (3, 3)).reshape(-1, 3, 3)
    if c2w.dim() > 2:
        c2w = torch.broadcast_to(c2w, sh + (3, 4)).reshape(-1, 3, 4)
    ndc = None if pixtocam_ndc is None else _dev(pixtocam_ndc, device)
    o, d, v, r, ip = _hip.pixels_to_rays(px, py, p2c, c2w, ndc, distortion=dist)
    return o.reshape(sh + (3,)), d.reshape(sh + (3,)), v.reshape(sh + (3,)), r.reshape(sh + (1,)), ip.reshape(sh + (2,))


def cast_ray_batch(cameras, pixels, camtype=ProjectionType.PERSPECTIVE, xnp=torch, device=None) -> utils.Rays:
    """Maps from input cameras and Pixel batch to output Ray batch (camera_utils.py:617-670)."""
    pixtocams, camtoworlds, distortion_params, pixtocam_ndc = cameras
    cam_idx = torch.as_tensor(np.asarray(pixels.cam_idx) if not torch.is_tensor(pixels.cam_idx) else pixels.cam_idx)[..., 0].long()

    def batch_index(arr):
        arr = torch.as_tensor(np.asarray(arr) if not torch.is_tensor(arr) else arr)
        return arr if arr.dim() == 2 else arr[cam_idx.to(arr.device)]
    o, d, v, r, ip = pixels_to_rays(pixels.pix_x_int, pixels.pix_y_int, batch_index(pixtocams), batch_index(camtoworlds),
                                    distortion_params=distortion_params, pixtocam_ndc=pixtocam_ndc, camtype=camtype,
                                    xnp=xnp, device=device)
    dev = o.device
    return utils.Rays(origins=o, directions=d, viewdirs=v, radii=r, imageplane=ip,
                      lossmult=_dev(pixels.lossmult, dev), near=_dev(pixels.near, dev), far=_dev(pixels.far, dev),
                      cam_idx=_dev(pixels.cam_idx, dev, torch.int32))


def _image_rays(projection, p2c, c2w, frame, height, width, near, far, ndc, dist, first, count) -> utils.Rays:
    whole = first == 0 and count is None
    res = _hip.image_rays(projection, width, height, p2c, c2w, frame, near, far, pixtocam_ndc=ndc, distortion=dist,
                          first=first, count=count)
    if whole:
        res = {k: v.reshape(height, width, v.shape[-1]) for k, v in res.items()}
    return utils.Rays(**res)


def cast_spherical_rays(camtoworld, height, width, near, far, xnp=torch, device=None) -> utils.Rays:
    """Equirectangular panorama ray batch for a whole image, shape [H, W, .] (camera_utils.py:700-746): one launch of
    refnerf_image_rays, nothing but the pose uploaded."""
    del xnp
    device = torch.device("cuda") if device is None else device
    c2w = _dev(camtoworld, device)[..., :3, :4].reshape(1, 3, 4).contiguous()
    return _image_rays(_hip.PROJ_SPHERICAL, None, c2w, 0, int(height), int(width), near, far, None, None, 0, None)


def cast_image_rays(cameras, cam_idx, height, width, near, far, spherical=False, first=0, count=None, device=None) -> utils.Rays:
    """All rays of view `cam_idx` of `cameras`, cast on the device in one launch: the device form of
    Dataset.generate_ray_batch (datasets.py:487-498).  `cameras` is the reference's tuple (pixtocams [3,3] | [n,3,3],
    camtoworlds [n,3,4], distortion_params dict | None, pixtocam_ndc | None); arrays already on the device as float32
    are used in place (PathCameras uploads its path once).  Returns Rays shaped [H, W, .]; with `first` / `count`, the
    rays of the flat row-major pixel range [first, first + count) shaped [count, .] -- a rank of a sharded render
    casts only its own.  `spherical`: the panorama of cast_spherical_rays at that pose (no distortion, no NDC)."""
    pixtocams, camtoworlds, distortion_params, pixtocam_ndc = cameras
    if device is None:
        device = camtoworlds.device if torch.is_tensor(camtoworlds) and camtoworlds.is_cuda else torch.device("cuda")
    cam_idx = operator.index(cam_idx)
    c2w = _dev(camtoworlds, device)[..., :3, :4]
    c2w = c2w.reshape((-1, 3, 4)).contiguous()
    dist = None if distortion_params is None else lens_distortion(distortion_params)
    ndc = None if pixtocam_ndc is None else _dev(pixtocam_ndc, device).contiguous()
    p2c = None
    if not spherical:
        p2c = _dev(pixtocams, device)
        p2c = (p2c if p2c.dim() == 2 else p2c[cam_idx]).contiguous()
    return _image_rays(_hip.PROJ_SPHERICAL if spherical else _hip.PROJ_PINHOLE, p2c, c2w, cam_idx, int(height), int(width),
                       near, far, ndc, dist, int(first), count)


def cast_pinhole_rays(camtoworld, height, width, focal, near, far, xnp=torch, device=None) -> utils.Rays:
    """Pinhole camera ray batch for a whole image (camera_utils.py:673-697)."""
    device = torch.device("cuda") if device is None else device
    pix_x_int, pix_y_int = pixel_coordinates(width, height, device)
    o, d, v, r, ip = pixels_to_rays(pix_x_int, pix_y_int, get_pixtocam(focal, width, height), camtoworld, xnp=xnp, device=device)

    def broadcast_scalar(x, dtype=torch.float32):
        return torch.full(tuple(pix_x_int.shape) + (1,), x, dtype=dtype, device=device)
    return utils.Rays(origins=o, directions=d, viewdirs=v, radii=r, imageplane=ip, lossmult=broadcast_scalar(1.),
                      near=broadcast_scalar(float(near)), far=broadcast_scalar(float(far)),
                      cam_idx=broadcast_scalar(0, torch.int32))

#!/usr/bin/env python3
"""Capture what the upstream reference's scene loaders load (build container only).

Run:  python tests/golden/make_golden_datasets.py
Needs the reference checkout (see _ref_harness.py), which is imported at run time only.  Writes
tests/golden/scene_datasets.npz: two tiny seeded scenes as raw arrays and JSON text, and, for a list of configurations,
the attributes of the reference's `Blender` / `LLFF` objects (internal/datasets.py:519-708) on those scenes.  Arrays and
strings of settings only; no reference source travels.  `write_scenes` rebuilds the scene folders from the fixture (PNG
and float TIFF are lossless); tests/test_scene_datasets.py imports it, which is why importing this file touches nothing.

Layout
  blender_json_<split> (str)       transforms_<split>.json, <split> = train (5 frames), test (3 frames)
  blender_rgba_<split> [n,12,18,4] uint8, blender_normal_<split> [n,12,18,4] uint8, blender_disp_<split> [n,12,18] float32
                                   <frame>.png, <frame>_normal.png, <frame>_disp.tiff; alpha includes 0 and 255, the
                                   disparities are multiples of 2^-10 in [0, 4) (block sums exact in float32)
  llff_json (str)                  transforms.json: 9 frames in shuffled order, fl_x, fl_y, cx, cy, k1, p1
  llff_names / llff_images [9,12,18,3] uint8      images/<name>, sorted by name
  llff_names_2 / llff_images_2 [9,6,9,3] uint8    images_2/<name>: other names, matched through the sorted lists
  llff_poses_bounds [9,17]         poses_bounds.npy
  cases (str[])                    per case <case>_config: JSON of {"loader", "split", "config": Config overrides} and the
                                   reference's attributes <case>_<attr>: images, alphas, normal_images, disp_images (where
                                   set), camtoworlds, pixtocams, focal, height, width, near, far, size; LLFF also
                                   pixtocam_ndc (where set), distortion_params (JSON), poses, colmap_to_world_transform and
                                   image_index (the rows of llff_images[_2] that `images` holds, in order)
  batch_cases (str[])              per case <case>_config as above (dataset_debug_mode on) and one training batch, rays
                                   cast by the reference's numpy path: <case>_<Rays field>, _rgb and _disps / _normals /
                                   _alphas where the configuration loads them
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

import numpy as np  # noqa: E402

RAY_FIELDS = ("origins", "directions", "viewdirs", "radii", "imageplane", "lossmult", "near", "far", "cam_idx")
H, W = 12, 18
FRAMES = 4          # render_path_frames: the reference builds a render path in every LLFF load

BLENDER_CASES = [
    ("blender_train", "train", {}),
    ("blender_test", "test", {}),
    ("blender_train_f2", "train", {"factor": 2}),
    ("blender_test_f2", "test", {"factor": 2}),
    ("blender_train_f3", "train", {"factor": 3}),
    ("blender_test_f3", "test", {"factor": 3}),
    ("blender_train_metrics", "train", {"compute_disp_metrics": True, "compute_normal_metrics": True}),
    ("blender_test_metrics_f2", "test", {"factor": 2, "compute_disp_metrics": True, "compute_normal_metrics": True}),
    ("blender_test_metrics_f3", "test", {"factor": 3, "compute_disp_metrics": True, "compute_normal_metrics": True}),
    ("blender_train_views3", "train", {"n_input_views": 3}),
]
LLFF_CASES = [
    ("llff_train", "train", {}),
    ("llff_test", "test", {}),
    ("llff_ff_train", "train", {"forward_facing": True}),
    ("llff_ff_test", "test", {"forward_facing": True}),
    ("llff_f2_train", "train", {"factor": 2}),
    ("llff_ff_f2_test", "test", {"factor": 2, "forward_facing": True}),
    ("llff_unsorted_train", "train", {"load_alphabetical": False}),
    ("llff_unsorted_ff_test", "test", {"load_alphabetical": False, "forward_facing": True}),
    ("llff_views3_train", "train", {"n_input_views": 3}),
    ("llff_all_train", "train", {"llff_use_all_images_for_training": True}),
    ("llff_hold3_test", "val", {"llffhold": 3}),
]
BATCH_CASES = [
    ("batch_blender_p1", "blender", {"batch_size": 40, "patch_size": 1, "compute_disp_metrics": True, "compute_normal_metrics": True}),
    ("batch_blender_p3", "blender", {"batch_size": 40, "patch_size": 3}),
    ("batch_llff_ff_p1", "llff", {"batch_size": 25, "patch_size": 1, "forward_facing": True, "near": 0., "far": 1.}),
    ("batch_llff_p3", "llff", {"batch_size": 30, "patch_size": 3, "near": .2, "far": 1e6}),
]


def look_at(position, target, up):
    z = position - target
    z = z / np.linalg.norm(z)
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z, position], axis=1)


def pose44(p34):
    return np.concatenate([p34, [[0., 0., 0., 1.]]], 0)


def make_scenes(rng):
    """The two seeded scenes as the arrays and JSON text the fixture stores."""
    z = {}
    for split, n in (("train", 5), ("test", 3)):
        rgba = rng.integers(0, 256, (n, H, W, 4), dtype=np.uint8)
        kind = rng.integers(0, 3, (n, H, W))
        rgba[..., 3] = np.where(kind == 0, 0, np.where(kind == 1, 255, rgba[..., 3]))
        rgba[0, 0, 0] = (0, 0, 0, 0)                 # every value class: the extremes of colour and alpha together
        rgba[0, 0, 1] = (255, 255, 255, 255)
        rgba[0, 0, 2] = (255, 0, 255, 1)
        rgba[0, 0, 3] = (1, 254, 0, 254)
        normal = rng.integers(0, 256, (n, H, W, 4), dtype=np.uint8)
        normal[0, 0, :2, :3] = ((0, 255, 128), (127, 1, 254))
        disp = (rng.integers(0, 4096, (n, H, W)) / 1024.).astype(np.float32)
        frames = []
        for k in range(n):
            a = 2 * np.pi * k / n + rng.normal(0, .1)
            pos = 4. * np.array([np.cos(a) * .8, np.sin(a) * .8, .6]) + rng.normal(0, .05, 3)
            frames.append({"file_path": f"./{split}/r_{k}", "rotation": 0.012566370614359171,
                           "transform_matrix": pose44(look_at(pos, np.zeros(3), np.array([0., 0., 1.]))).tolist()})
        z[f"blender_json_{split}"] = json.dumps({"camera_angle_x": 0.6911112070083618, "frames": frames}, indent=1)
        z[f"blender_rgba_{split}"], z[f"blender_normal_{split}"], z[f"blender_disp_{split}"] = rgba, normal, disp

    n = 9
    names = [f"view_{k:02d}.png" for k in range(n)]                 # sorted
    names_2 = [f"small_{k:02d}.png" for k in range(n)]
    images = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    images[0, 0, :2] = ((0, 255, 1), (254, 128, 127))
    images_2 = rng.integers(0, 256, (n, H // 2, W // 2, 3), dtype=np.uint8)
    frames = []
    for k in range(n):
        pos = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1., 1.), rng.normal(0, .3)])
        c2w = look_at(pos, np.array([.1, -.05, -6.]) + rng.normal(0, .2, 3), np.array([.02, 1., .03]))
        frames.append({"file_path": f"images/{names[k]}", "transform_matrix": pose44(c2w).tolist()})
    order = rng.permutation(n)
    assert list(order) != sorted(order)
    meta = {"w": W, "h": H, "fl_x": 21.5, "fl_y": 20.75, "cx": 9.25, "cy": 5.5, "k1": 0.03, "p1": -0.002,
            "frames": [frames[i] for i in order]}
    z["llff_json"] = json.dumps(meta, indent=1)
    z["llff_names"], z["llff_images"] = np.array(names), images
    z["llff_names_2"], z["llff_images_2"] = np.array(names_2), images_2
    bounds = np.stack([rng.uniform(2., 3., n), rng.uniform(20., 40., n)], -1)
    z["llff_poses_bounds"] = np.concatenate([rng.normal(size=(n, 15)), bounds], -1)
    return z


def write_scenes(z, root):
    """Rebuild the two scene folders from the fixture's arrays: (blender_dir, llff_dir)."""
    from PIL import Image
    blender, llff = os.path.join(root, "blender_scene"), os.path.join(root, "llff_scene")
    for split in ("train", "test"):
        os.makedirs(os.path.join(blender, split))
        with open(os.path.join(blender, f"transforms_{split}.json"), "w") as fh:
            fh.write(str(z[f"blender_json_{split}"]))
        for k, frame in enumerate(json.loads(str(z[f"blender_json_{split}"]))["frames"]):
            prefix = os.path.join(blender, frame["file_path"])
            Image.fromarray(np.asarray(z[f"blender_rgba_{split}"][k]), "RGBA").save(prefix + ".png")
            Image.fromarray(np.asarray(z[f"blender_normal_{split}"][k]), "RGBA").save(prefix + "_normal.png")
            Image.fromarray(np.asarray(z[f"blender_disp_{split}"][k], np.float32), "F").save(prefix + "_disp.tiff")
    for folder, names, images in (("images", z["llff_names"], z["llff_images"]), ("images_2", z["llff_names_2"], z["llff_images_2"])):
        os.makedirs(os.path.join(llff, folder))
        for name, img in zip(names, images):
            Image.fromarray(np.asarray(img), "RGB").save(os.path.join(llff, folder, str(name)))
    with open(os.path.join(llff, "transforms.json"), "w") as fh:
        fh.write(str(z["llff_json"]))
    np.save(os.path.join(llff, "poses_bounds.npy"), np.asarray(z["llff_poses_bounds"]))
    return blender, llff


def main():
    sys.path.insert(0, HERE)
    import _ref_harness
    _ref_harness.install()
    from internal import configs, datasets

    z = make_scenes(np.random.default_rng(20241020))
    out = dict(z)
    with tempfile.TemporaryDirectory() as tmp:
        dirs = dict(zip(("blender", "llff"), write_scenes(z, tmp)))
        ref = {"blender": datasets.Blender, "llff": datasets.LLFF}

        def load(loader, split, overrides):
            cfg = configs.Config(dataset_loader=loader, render_path_frames=FRAMES, **overrides)
            return ref[loader](split, dirs[loader], cfg)

        cases = []
        for loader, table in (("blender", BLENDER_CASES), ("llff", LLFF_CASES)):
            for case, split, overrides in table:
                ds = load(loader, split, overrides)
                out[case + "_config"] = json.dumps({"loader": loader, "split": split, "config": overrides})
                for attr in ("images", "alphas", "normal_images", "disp_images"):
                    if getattr(ds, attr) is not None:
                        assert getattr(ds, attr).dtype == np.float32, (case, attr)
                        out[f"{case}_{attr}"] = getattr(ds, attr)
                for attr in ("camtoworlds", "pixtocams", "focal", "height", "width", "near", "far", "size"):
                    out[f"{case}_{attr}"] = np.asarray(getattr(ds, attr))
                if loader == "llff":
                    if ds.pixtocam_ndc is not None:
                        out[case + "_pixtocam_ndc"] = ds.pixtocam_ndc
                    out[case + "_distortion_params"] = json.dumps(ds.distortion_params)
                    out[case + "_poses"], out[case + "_colmap_to_world_transform"] = ds.poses, ds.colmap_to_world_transform
                    full = (z["llff_images_2"] if overrides.get("factor", 0) > 1 else z["llff_images"]).astype(np.float32) / 255.
                    index = [[i for i in range(len(full)) if np.array_equal(full[i], im)] for im in ds.images]
                    assert all(len(i) == 1 for i in index), case
                    out[case + "_image_index"] = np.array([i[0] for i in index])
                    del out[case + "_images"]          # llff_images[_2][image_index] / 255 says it all (asserted above)
                cases.append(case)
        out["cases"] = np.array(cases)

        batch_cases = []
        for case, loader, overrides in BATCH_CASES:
            ds = load(loader, "train", dict(overrides, dataset_debug_mode=True))
            out[case + "_config"] = json.dumps({"loader": loader, "split": "train", "config": dict(overrides, dataset_debug_mode=True)})
            batch = next(ds)
            for k in RAY_FIELDS:
                out[f"{case}_{k}"] = np.asarray(getattr(batch.rays, k))
            for k in ("rgb", "disps", "normals", "alphas"):
                if getattr(batch, k) is not None:
                    out[f"{case}_{k}"] = np.asarray(getattr(batch, k))
            batch_cases.append(case)
        out["batch_cases"] = np.array(batch_cases)

    for k, v in out.items():
        assert np.asarray(v).dtype.kind in "fiuU", (k, np.asarray(v).dtype)
    path = os.path.join(HERE, "scene_datasets.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()

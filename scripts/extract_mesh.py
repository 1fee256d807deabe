"""A trained model to a mesh: render the views of a scene, fuse their depth maps into a TSDF volume and write the
iso-surface as a binary PLY (refnerf_pl_amd.geometry; include/refnerf_tsdf.h):
    python scripts/extract_mesh.py --gin_configs configs/refnerf_blender.gin --ckpt model.ckpt --data_dir scene/ --out mesh.ply
--ckpt is a checkpoint of the reference's Lightning system (utils.load_reference_checkpoint); without it the model keeps its
initial weights (a plumbing run).  The views are those of --split, pinhole and undistorted (NDC, lens distortion and
panoramas raise).  --aabb is the box the volume covers, in the frame the model was trained in.
--surface_metrics ray casts the fused volume back into the same views (include/refnerf_raycast.h) and prints
geometry.surface_metrics: the angular error of the surface's normals against the split's ground-truth normals (where the
scene has them), the L1 distance of its depth to the rendered --depth_key, the coverage.  --surface_dir DIR writes the normal
and depth panels of those views."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gin_configs", nargs="+", required=True)
    ap.add_argument("--gin_bindings", nargs="*", default=[])
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--data_dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--split", default="test")
    ap.add_argument("--aabb", type=float, nargs=6, default=[-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--resolution", type=int, default=256, help="voxels along the longest side of the box")
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance in world units (default: 4 voxels)")
    ap.add_argument("--depth_key", default="distance_median", choices=["distance_median", "distance_mean"])
    ap.add_argument("--acc_threshold", type=float, default=0.5)
    ap.add_argument("--min_weight", type=float, default=1.0, help="a cell needs this much weight on all eight corners")
    ap.add_argument("--max_views", type=int, default=None)
    ap.add_argument("--no_color", action="store_true")
    ap.add_argument("--surface_metrics", action="store_true", help="print the scores of the ray-cast surface for the fused split")
    ap.add_argument("--surface_dir", default=None, help="write surface_normals_ / surface_depth_ panels of the ray-cast views here")
    args = ap.parse_args(argv)

    import torch

    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import _hip, configs, datasets, geometry, models, utils
    _hip.require_device()
    dev = torch.device("cuda:0")
    configs.clear_config()
    configs.parse_config_files_and_bindings(args.gin_configs, args.gin_bindings)
    cfg = configs.Config()
    model = models.construct_model(None, cfg).to(dev).eval()
    configs.clear_config()
    if args.ckpt:
        missing, unexpected = utils.load_reference_checkpoint(model, args.ckpt)
        assert not missing and not unexpected, (missing, unexpected)
    views = datasets.load_dataset(args.split, args.data_dir, cfg, device=dev)
    volume = geometry.TSDFVolume(args.aabb[:3], args.aabb[3:], resolution=args.resolution, trunc=args.trunc, color=not args.no_color, device=dev)
    indices = range(views.size if args.max_views is None else min(views.size, args.max_views))
    renderings = {} if args.surface_metrics else None
    geometry.fuse_views(lambda rays: model(rays, 1.0, True), views, cfg, volume, indices=indices, depth_key=args.depth_key,
                        keep=renderings, acc_threshold=args.acc_threshold)
    vertices, faces, colors = volume.extract_mesh(min_weight=args.min_weight)
    geometry.save_ply(args.out, vertices, faces, colors)
    print(f"{args.out}: {vertices.shape[0]} vertices, {faces.shape[0]} triangles from {len(indices)} views "
          f"({volume.dims[0]} x {volume.dims[1]} x {volume.dims[2]} voxels of {volume.voxel_size:g})")
    cast = dict(min_weight=args.min_weight)
    if args.surface_metrics:
        scores = geometry.surface_metrics(volume, views, indices=indices, renderings=renderings, depth_key=args.depth_key, **cast)
        print(json.dumps(scores))
    if args.surface_dir:
        written = geometry.write_surface_views(volume, views, args.surface_dir, indices=indices, **cast)
        print(f"{args.surface_dir}: {len(written)} files")
    return 0


if __name__ == "__main__":
    sys.exit(main())

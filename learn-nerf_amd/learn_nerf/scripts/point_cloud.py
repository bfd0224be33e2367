"""
Coloured mesh from the RGB-D views that render_new_dataset.py writes: the reference's Go command point_cloud/main.go
with its flags in this package's spelling and its defaults.  The views NNNNN.json / NNNNN.png / NNNNN_depth.png of
`data_dir` are back-projected into a point cloud, thinned to --max_points (at random, or the densest with
--sort_density), and the union of the balls of radius --thickness about the points is meshed on a grid of spacing
--delta; every vertex takes the colour of its nearest point (HIP, learn_nerf/point_cloud.py).  Deliberate differences:
per-vertex colours in .obj ('v x y z r g b') or binary .ply instead of a zipped material OBJ, a linearly interpolated
surface on a grid padded by thickness + delta, a stable density sort and a seeded shuffle (--seed), and the additive
flags --batch_size and --cloud_path.
"""
import argparse
import os
import sys

import torch

from learn_nerf.point_cloud import extract, read_dataset, subsample, write_colored_obj, write_ply


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--max_depth", type=float, default=10.0, help="maximum depth value corresponding to white pixel")
    parser.add_argument("--thickness", type=float, default=0.02, help="radius of each point")
    parser.add_argument("--delta", type=float, default=0.02, help="marching cubes delta")
    parser.add_argument("--max_points", type=int, default=50000, help="maximum points to sample")
    parser.add_argument("--sort_density", action="store_true", help="remove lowest density samples first")
    parser.add_argument("--sort_density_k", type=int, default=5, help="neighbor to use for density estimate")
    parser.add_argument("--seed", type=int, default=0, help="(additive) seed of the shuffle without --sort_density")
    parser.add_argument("--batch_size", type=int, default=1 << 22, help="(additive) grid points per field batch")
    parser.add_argument("--cloud_path", type=str, default=None, help="(additive) write the kept points to this .ply")
    parser.add_argument("data_dir", type=str, help="data directory")
    parser.add_argument("output_path", type=str, help="output mesh, .obj or .ply")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.output_path.endswith((".obj", ".ply")):
        parser.error(f"output_path must end in .obj or .ply: {args.output_path!r}")
    if args.cloud_path is not None and not args.cloud_path.endswith(".ply"):
        parser.error(f"--cloud_path must end in .ply: {args.cloud_path!r}")
    if args.max_points < 1 or args.batch_size < 1 or not 1 <= args.sort_density_k <= 32:
        parser.error("--max_points and --batch_size must be positive and --sort_density_k in [1, 32]")
    if not (args.thickness > 0 and args.delta > 0 and args.max_depth > 0):
        parser.error("--thickness, --delta and --max_depth must be positive")

    if not os.path.exists(os.path.join(args.data_dir, "00000.json")):
        sys.exit(f"no views: {args.data_dir!r} has no 00000.json")

    print("Computing points...", flush=True)
    device = torch.device("cuda", torch.cuda.current_device())
    points, colors, views = read_dataset(args.data_dir, args.max_depth, device)
    total = points.shape[0]
    if total == 0:
        sys.exit(f"no points: every depth pixel of the {views} views in {args.data_dir!r} is 0xffff (nothing was hit)")
    if total > args.max_points:
        print(f"Found {total} points. Reducing to {args.max_points}...", flush=True)
        points, colors = subsample(points, colors, args.max_points, args.sort_density, args.sort_density_k, args.seed)
    else:
        print(f"Using all {total} points.", flush=True)
    if args.cloud_path is not None:
        write_ply(args.cloud_path, points.cpu().numpy(), colors.cpu().numpy())

    print("Creating mesh...", flush=True)
    try:
        verts, faces, vertex_colors = extract(points, colors, args.thickness, args.delta, args.batch_size)
    except ValueError as err:  # the field's point budget
        sys.exit(str(err))

    print("Saving mesh...", flush=True)
    if args.output_path.endswith(".obj"):
        write_colored_obj(args.output_path, verts, faces, vertex_colors)
    else:
        write_ply(args.output_path, verts, vertex_colors, faces)


if __name__ == "__main__":
    main()

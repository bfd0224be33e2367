"""
Coloured single-surface mesh from the RGB-D views that render_new_dataset.py writes, by TSDF fusion (additive; no
counterpart in the reference).  The views NNNNN.json / NNNNN.png / NNNNN_depth.png of `data_dir` are fused into a
--resolution^3 grid over the bounding box of --metadata_json (the copy render_new_dataset.py leaves in data_dir), and
marching cubes at signed distance 0 gives the surface, coloured per vertex from the views that saw it (HIP,
learn_nerf/tsdf.py).  Output: .obj ('v x y z r g b') or binary .ply, in the dataset's own frame.  Space that no view
saw in front of a surface is solid by default (--unseen inside), which closes holes; with few views this can leave a
blob where a region is occluded in one view and outside every other: add views or --keep_largest 1.
--target_faces / --simplify_grid simplify the coloured mesh by quadric vertex clustering (learn_nerf/simplify.py): a
vertex of the result has the mean 8-bit colour of the corners it replaces.  Without them nothing changes.
"""
import argparse
import os
import sys

import numpy as np
import torch

from learn_nerf.dataset import ModelMetadata
from learn_nerf.point_cloud import _rgb8, write_colored_obj, write_ply
from learn_nerf.tsdf import TsdfVolume, read_rgbd_views


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--resolution", type=int, default=256, help="grid points along each axis of the bounding box")
    parser.add_argument("--truncation", type=float, default=3.0, help="truncation distance in grid steps")
    parser.add_argument("--max_depth", type=float, default=10.0, help="maximum depth value corresponding to white pixel")
    parser.add_argument("--no_carve", action="store_true", help="do not treat pixels that hit nothing as free space")
    parser.add_argument("--unseen", choices=("inside", "outside"), default="inside",
                        help="what a voxel is that was only ever seen behind a surface")
    parser.add_argument("--min_component", type=int, default=1,
                        help="drop connected components of the inside set with fewer grid points than this")
    parser.add_argument("--keep_largest", type=int, default=None,
                        help="keep only this many of the largest connected components")
    parser.add_argument("--connectivity", type=int, default=26, choices=(6, 26),
                        help="grid points are joined through faces (6) or faces, edges and corners (26)")
    parser.add_argument("--target_faces", type=int, default=None, help="simplify the mesh to at most this many faces")
    parser.add_argument("--simplify_grid", type=int, default=None,
                        help="simplify the mesh on a grid of this many cells along its longest axis")
    parser.add_argument("--metadata_json", type=str, default=None, help="bounding box; default data_dir/metadata.json")
    parser.add_argument("data_dir", type=str, help="data directory")
    parser.add_argument("output_path", type=str, help="output mesh, .obj or .ply")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.output_path.endswith((".obj", ".ply")):
        sys.exit(f"output_path must end in .obj or .ply: {args.output_path!r}")
    if args.resolution < 2:
        sys.exit("--resolution must be at least 2")
    if not (args.truncation > 0 and args.max_depth > 0):
        sys.exit("--truncation and --max_depth must be positive")
    if args.min_component < 1 or (args.keep_largest is not None and args.keep_largest < 1):
        sys.exit("--min_component and --keep_largest must be at least 1")
    if args.target_faces is not None and args.simplify_grid is not None:
        sys.exit("give --target_faces or --simplify_grid, not both")
    if any(v is not None and v < 1 for v in (args.target_faces, args.simplify_grid)):
        sys.exit("--target_faces and --simplify_grid must be at least 1")
    if not os.path.exists(os.path.join(args.data_dir, "00000.json")):
        sys.exit(f"no views: {args.data_dir!r} has no 00000.json")
    metadata_path = args.metadata_json or os.path.join(args.data_dir, "metadata.json")
    if not os.path.exists(metadata_path):
        sys.exit(f"no metadata: {metadata_path!r} does not exist (pass --metadata_json)")
    metadata = ModelMetadata.from_json(metadata_path)

    cameras, depths, colors = read_rgbd_views(args.data_dir)
    print(f"Fusing {len(cameras)} views...", flush=True)
    device = torch.device("cuda", torch.cuda.current_device())
    volume = TsdfVolume(metadata.bbox_min, metadata.bbox_max, args.resolution, truncation_voxels=args.truncation,
                        max_depth=args.max_depth, carve=not args.no_carve, device=device)
    volume.integrate(cameras, depths, colors)
    filtering = args.min_component != 1 or args.keep_largest is not None
    verts, faces, vertex_colors, info = volume.extract(unseen=args.unseen, min_component=args.min_component,
                                                       keep_largest=args.keep_largest, connectivity=args.connectivity)
    print(f"voxels: observed={info['observed']} unseen_inside={info['unseen_inside']} "
          f"unseen_outside={info['unseen_outside']}", flush=True)
    if filtering:
        print(f"components: kept {info['kept']} of {info['components']}, removed {info['removed']} points", flush=True)
    if len(faces) == 0:
        sys.exit(f"no surface: the signed distance changes sign nowhere in the box ({info['observed']} observed voxels); "
                 "check --max_depth and the bounding box")
    print(f"vertices={len(verts)} faces={len(faces)} uncoloured={info['uncoloured']}", flush=True)
    if args.target_faces is not None or args.simplify_grid is not None:
        from learn_nerf.simplify import format_info, simplify

        try:
            simple = simplify(verts, faces, _rgb8(vertex_colors), target_faces=args.target_faces,
                              grid=args.simplify_grid, device=device)
        except ValueError as err:
            sys.exit(f"no surface after simplification: {err}")
        print("simplified: " + " ".join(format_info(simple.info)), flush=True)
        verts, faces = simple.verts.cpu().numpy(), simple.faces.cpu().numpy()
        vertex_colors = (simple.colors.cpu().numpy().astype(np.float64) / 255).astype(np.float32)

    print("Saving mesh...", flush=True)
    if args.output_path.endswith(".obj"):
        write_colored_obj(args.output_path, verts, faces, vertex_colors)
    else:
        write_ply(args.output_path, verts, vertex_colors, faces)


if __name__ == "__main__":
    main()

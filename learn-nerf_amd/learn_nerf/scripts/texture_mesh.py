"""
Bake a texture for a triangle mesh from the views of a dataset (additive; no counterpart in the reference):
`mesh data_dir output.obj`.  mesh is a .stl, .obj or .ply file in the dataset's world coordinates (marching_cubes.py
--world_coords, tsdf_mesh.py and point_cloud.py write such meshes); data_dir is a dataset directory as eval_nerf.py
reads it.  Every triangle gets a right-angled patch of a texture atlas, and every texel the weighted mean colour of the
views that see its surface point (learn_nerf/texture.py; HIP).  Writes output.obj with `vt` records, output.mtl and
output.png.  --target_faces simplifies the mesh first (learn_nerf/simplify.py), which is what makes the patches large
enough to hold detail.

stdout: one key=value line each for faces, texture_size (the size used, at most --texture_size), cell, views, offset,
texels_used, seen, filled, unseen, degenerate_faces, and with --check `reprojection_psnr=<repr> <image_path>` per view
and `reprojection_psnr_mean=<repr>`: the mesh is rendered with its texture from every view and compared with the image.
"""
import argparse
import math
import sys

import numpy as np
import torch

from learn_nerf.mesh_metrics import read_mesh
from learn_nerf.raycast import TriangleMesh
from learn_nerf.texture import TextureAtlas, bake_views, read_views, reprojection_psnr, write_textured_obj


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--texture_size", type=int, default=2048, help="largest side of the square texture")
    parser.add_argument("--max_angle", type=float, default=80.0,
                        help="largest angle, in degrees, between a texel's normal and the direction to a view")
    parser.add_argument("--angle_power", type=int, default=2, help="a view's weight is cos(angle)^power")
    parser.add_argument("--offset", type=float, default=None,
                        help="start of the visibility ray off the surface (default: 1e-3 of the mesh's diagonal)")
    parser.add_argument("--fill_passes", type=int, default=8,
                        help="passes that give unseen texels the colour of seen neighbours of their patch")
    parser.add_argument("--unseen_color", type=int, nargs=3, default=(128, 128, 128), metavar=("R", "G", "B"),
                        help="colour of the texels that stay unseen")
    parser.add_argument("--target_faces", type=int, default=None, help="simplify the mesh to at most this many faces first")
    parser.add_argument("--max_views", type=int, default=None, help="use only the first N views of the dataset")
    parser.add_argument("--check", action="store_true", help="print the reprojection PSNR of every view and the mean")
    parser.add_argument("mesh", type=str, help="input mesh, .stl, .obj or .ply, in world coordinates")
    parser.add_argument("data_dir", type=str, help="a dataset directory")
    parser.add_argument("output", type=str, help="output .obj; the .mtl and .png go beside it")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.output.lower().endswith(".obj"):
        sys.exit(f"{args.output!r}: expected a .obj file")
    if args.texture_size < 1:
        sys.exit("--texture_size must be positive")
    if not 0 < args.max_angle <= 90:
        sys.exit("--max_angle must lie in (0, 90] degrees")
    if not 0 <= args.angle_power <= 64:
        sys.exit("--angle_power must lie in [0, 64]")
    if args.offset is not None and not (args.offset >= 0 and math.isfinite(args.offset)):
        sys.exit("--offset must be finite and not negative")
    if args.fill_passes < 0:
        sys.exit("--fill_passes must not be negative")
    if not all(0 <= c <= 255 for c in args.unseen_color):
        sys.exit("--unseen_color must be three integers in [0, 255]")
    if args.target_faces is not None and args.target_faces < 1:
        sys.exit("--target_faces must be positive")
    if args.max_views is not None and args.max_views < 1:
        sys.exit("--max_views must be positive")
    try:
        tris = read_mesh(args.mesh)
        cameras, images, paths = read_views(args.data_dir, args.max_views)
    except (ValueError, OSError) as err:
        sys.exit(str(err))
    if not cameras:
        sys.exit(f"{args.data_dir}: no views")
    device = torch.device("cuda", torch.cuda.current_device())
    try:
        if args.target_faces is not None:
            from learn_nerf.simplify import simplify

            small = simplify(tris, target_faces=args.target_faces, device=device)
            tris = small.verts[small.faces.long()].cpu().numpy()
        tris_dev = torch.from_numpy(np.ascontiguousarray(tris, dtype=np.float32)).to(device)
        atlas = TextureAtlas(tris_dev, args.texture_size)
        mesh = TriangleMesh(tris_dev)
    except ValueError as err:
        sys.exit(str(err))
    print(f"faces={atlas.F}")
    print(f"texture_size={atlas.S}")
    print(f"cell={atlas.c}")
    print(f"views={len(cameras)}", flush=True)
    texture, info = bake_views(atlas, mesh, cameras, images, max_angle=math.radians(args.max_angle),
                               power=args.angle_power, offset=args.offset, fill_passes=args.fill_passes,
                               unseen_color=tuple(args.unseen_color))
    for key in ("texels_used", "seen", "filled", "unseen", "degenerate_faces"):
        print(f"{key}={info[key]}")
    write_textured_obj(args.output, tris, atlas, texture)
    if args.check:
        per_view, mean = reprojection_psnr(atlas, mesh, texture, cameras, images)
        for value, path in zip(per_view, paths):
            print(f"reprojection_psnr={value!r} {path}")
        print(f"reprojection_psnr_mean={mean!r}")


if __name__ == "__main__":
    main()

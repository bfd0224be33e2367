"""
Simplify a triangle mesh by vertex clustering with quadric error metrics (additive; no counterpart in the reference):
`input output`, each a .stl, .obj or .ply file, and exactly one of --cell_size (the edge of the cubic cells), --grid
(cells along the longest axis of the bounding box) and --target_faces (the finest such grid that leaves at most that
many faces).  Every occupied cell becomes one vertex, placed by the quadrics of the cell's triangles (--placement
quadric, which keeps corners and creases) or at the mean of its corners (--placement mean); HIP,
learn_nerf/simplify.py.  The vertex colours of a .ply input are carried into a .ply or .obj output as the mean colour
of each cell's corners.  Prints one key=value line per item of the result's info.
"""
import argparse
import sys

import numpy as np
import torch

from learn_nerf.mesh import write_obj, write_stl
from learn_nerf.mesh_metrics import _read_obj, read_ply
from learn_nerf.point_cloud import write_colored_obj, write_ply
from learn_nerf.raycast import read_stl
from learn_nerf.simplify import PLACEMENTS, format_info, simplify

EXTENSIONS = (".stl", ".obj", ".ply")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--cell_size", type=float, default=None, help="edge of the cubic cells")
    parser.add_argument("--grid", type=int, default=None, help="cells along the longest axis of the bounding box")
    parser.add_argument("--target_faces", type=int, default=None, help="at most this many faces")
    parser.add_argument("--placement", choices=PLACEMENTS, default="quadric", help="where a cell's vertex goes")
    parser.add_argument("input", type=str, help="input mesh, .stl, .obj or .ply")
    parser.add_argument("output", type=str, help="output mesh, .stl, .obj or .ply")
    return parser


def read_indexed(path: str):
    """(triangles [F, 3, 3] or verts [V, 3], faces [F, 3] or None, colours uint8 [V, 3] or None) of a mesh file."""
    lower = path.lower()
    if lower.endswith(".stl"):
        return read_stl(path), None, None
    if lower.endswith(".obj"):
        verts, faces = _read_obj(path)
        colors = None
    else:
        verts, colors, faces = read_ply(path)
    if len(faces) == 0:
        raise ValueError(f"{path}: the mesh holds no triangles")
    if faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError(f"{path}: a face names a vertex outside [0, {len(verts)})")
    return verts, faces, colors


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    for path in (args.input, args.output):
        if not path.lower().endswith(EXTENSIONS):
            sys.exit(f"{path!r}: expected a .stl, .obj or .ply file")
    if sum(v is not None for v in (args.cell_size, args.grid, args.target_faces)) != 1:
        sys.exit("give exactly one of --cell_size, --grid and --target_faces")
    try:
        verts, faces, colors = read_indexed(args.input)
        device = torch.device("cuda", torch.cuda.current_device())
        out = simplify(verts, faces, colors, cell_size=args.cell_size, grid=args.grid,
                       target_faces=args.target_faces, placement=args.placement, device=device)
    except (ValueError, OSError) as err:
        sys.exit(str(err))
    for line in format_info(out.info):
        print(line)
    v, f = out.verts.cpu().numpy(), out.faces.cpu().numpy()
    rgb = None if out.colors is None else (out.colors.cpu().numpy().astype(np.float64) / 255).astype(np.float32)
    lower = args.output.lower()
    if lower.endswith(".stl"):
        write_stl(args.output, v, f)
    elif lower.endswith(".ply"):
        write_ply(args.output, v, rgb, f)
    elif rgb is not None:
        write_colored_obj(args.output, v, f, rgb)
    else:
        write_obj(args.output, v, f)


if __name__ == "__main__":
    main()

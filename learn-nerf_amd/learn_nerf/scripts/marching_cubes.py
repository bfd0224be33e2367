"""
Mesh export with the command line of the reference's scripts/marching_cubes.py: flags, positional
`metadata_json output_obj`, the fine model's occupancy 1 - exp(-sigma) on a resolution^3 grid inside the scene's
bounding box, marching cubes at --threshold (HIP, learn_nerf/mesh.py), OBJ or STL by the output's extension.
Deliberate differences: a binary STL writer that works (the reference's cannot run), outward-wound faces, an error for
an output extension other than .obj / .stl and for a grid where no occupancy exceeds the threshold, and one additive
flag, --world_coords.  Additive as well: --min_component / --keep_largest / --connectivity remove floaters, the connected
components of {occupancy > threshold} that are small or not among the largest (learn_nerf/components.py), before the
surface is extracted; without them nothing changes.  --target_faces / --simplify_grid simplify the extracted mesh by
quadric vertex clustering (learn_nerf/simplify.py) before the frame transform; without them nothing changes either.
"""
import argparse
import sys

import torch

from learn_nerf.dataset import ModelMetadata
from learn_nerf.mesh import extract_mesh, reference_frame, world_frame, write_obj, write_stl
from learn_nerf.scripts.train_nerf import add_model_args, create_model
from learn_nerf.train import load_params

WRITERS = {".obj": write_obj, ".stl": write_stl}


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--batch_size", type=int, default=1024, help="rays per batch")
    parser.add_argument("--resolution", type=int, default=32, help="steps along each direction")
    parser.add_argument("--threshold", type=float, default=0.9, help="occupancy level of the surface")
    parser.add_argument("--model_path", type=str, default="nerf.pkl", help="checkpoint written by train_nerf.py")
    add_model_args(parser)
    parser.add_argument("--world_coords", action="store_true",
                        help="(additive) write scene coordinates instead of the reference's centred, x/z-swapped frame")
    parser.add_argument("--min_component", type=int, default=1,
                        help="(additive) drop connected components of the inside set with fewer grid points than this")
    parser.add_argument("--keep_largest", type=int, default=None,
                        help="(additive) keep only this many of the largest connected components")
    parser.add_argument("--connectivity", type=int, default=26, choices=(6, 26),
                        help="(additive) grid points are joined through faces (6) or faces, edges and corners (26)")
    parser.add_argument("--target_faces", type=int, default=None,
                        help="(additive) simplify the mesh to at most this many faces")
    parser.add_argument("--simplify_grid", type=int, default=None,
                        help="(additive) simplify the mesh on a grid of this many cells along its longest axis")
    parser.add_argument("metadata_json", type=str)
    parser.add_argument("output_obj", type=str, help="output mesh, .obj or .stl")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    ext = next((e for e in WRITERS if args.output_obj.endswith(e)), None)
    if ext is None:
        parser.error(f"output_obj must end in .obj or .stl: {args.output_obj!r}")
    if args.resolution < 2 or args.batch_size < 1:
        parser.error("--resolution must be at least 2 and --batch_size positive")
    if args.min_component < 1 or (args.keep_largest is not None and args.keep_largest < 1):
        parser.error("--min_component and --keep_largest must be at least 1")
    if args.target_faces is not None and args.simplify_grid is not None:
        parser.error("give --target_faces or --simplify_grid, not both")
    if any(v is not None and v < 1 for v in (args.target_faces, args.simplify_grid)):
        parser.error("--target_faces and --simplify_grid must be at least 1")

    print("loading metadata...")
    metadata = ModelMetadata.from_json(args.metadata_json)

    print("loading model...")
    device = torch.device("cuda", torch.cuda.current_device())
    coarse, fine, _ = create_model(args, metadata)
    params = load_params(args.model_path, coarse, fine, device)["fine"]

    print("computing densities...")
    box = (metadata.bbox_min, metadata.bbox_max, args.resolution)
    found = {}
    verts, faces, largest = extract_mesh(fine, params, *box, args.batch_size, args.threshold,
                                         min_component=args.min_component, keep_largest=args.keep_largest,
                                         connectivity=args.connectivity, info=found)
    if found:  # a filter is active
        print(f"components: kept {found['kept']} of {found['components']}, removed {found['removed']} points")
        if found["components"] and not found["kept"]:
            sys.exit(f"no surface: the filter removed all {found['components']} components")
    if faces.shape[0] == 0:
        sys.exit(f"no surface: no occupancy exceeds the threshold {args.threshold} (largest occupancy {largest:.6g})")
    if args.target_faces is not None or args.simplify_grid is not None:
        from learn_nerf.simplify import format_info, simplify

        try:
            simple = simplify(verts, faces, target_faces=args.target_faces, grid=args.simplify_grid)
        except ValueError as err:
            sys.exit(f"no surface after simplification: {err}")
        print("simplified: " + " ".join(format_info(simple.info)))
        verts, faces = simple.verts, simple.faces
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    if args.world_coords:
        verts = world_frame(verts, *box)
    else:
        verts, faces = reference_frame(verts, faces, *box)
    WRITERS[ext](args.output_obj, verts, faces)


if __name__ == "__main__":
    main()

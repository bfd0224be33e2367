"""
Dataset from an .stl: the reference's Go command simple_dataset/ with its flags in this package's spelling and its
defaults.  The mesh is normalised (box centred on 0, largest coordinate 1), lit by --num_lights random point lights and
ray-cast in HIP (learn_nerf/raycast.py) from --images random cameras, or with --rotate from cameras circling
--rotation_axis; NNNN.png (RGBA), NNNN.json {origin, x, y, z, x_fov, y_fov} and metadata.json {min, max} are what
load_dataset reads.  Deliberate differences: --fov is converted from degrees once (the Go random-camera path converts
it twice and renders at about 1 degree), random numbers come from np.random.RandomState(--seed) (lights first, then one
direction per random camera), the shading, camera frame and camera distance are the ones fixed in learn_nerf/raycast.py
(model3d's are not in the reference), and the progress line says "image" where the Go program says "imade".
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from learn_nerf import raycast


def _vector(text: str):
    parts = text.split(",")
    if len(parts) != 3:
        raise argparse.ArgumentTypeError(f"expected 'x,y,z', got {text!r}")
    try:
        return tuple(float(p) for p in parts)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected 'x,y,z', got {text!r}") from None


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--fov", type=float, default=60.0, help="field of view in degrees")
    parser.add_argument("--resolution", type=int, default=800, help="side length of images to render")
    parser.add_argument("--images", type=int, default=100, help="number of images to render")
    parser.add_argument("--num_lights", type=int, default=5, help="number of lights to put into the scene")
    parser.add_argument("--light_brightness", type=float, default=0.5, help="brightness of lights")
    parser.add_argument("--seed", type=int, default=0, help="seed of the random lights and cameras")
    parser.add_argument("--no_images", action="store_true", help="only save json files, not renderings")
    parser.add_argument("--rotate", action="store_true", help="render a rotating view rather than random views")
    parser.add_argument("--color", type=_vector, default=(0.8, 0.8, 0.0), help="color of the model, as 'r,g,b'")
    parser.add_argument("--rotation_axis", type=_vector, default=(0.0, 0.0, 1.0), help="axis of rotation for --rotate")
    parser.add_argument("--rotation_offset", type=_vector, default=(0.0, -1.0, 0.0),
                        help="initial offset from center for --rotate")
    parser.add_argument("input_stl", type=str, help="input .stl, binary or ASCII")
    parser.add_argument("output_dir", type=str, help="output directory")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.resolution < 2 or args.images < 1 or args.num_lights < 0:
        parser.error("--resolution must be at least 2, --images at least 1 and --num_lights at least 0")
    if not 0 < args.fov < 180:
        parser.error("--fov must lie in (0, 180) degrees")
    fov = math.radians(args.fov)

    print(f"Creating output directory: {args.output_dir}...", flush=True)
    if os.path.exists(args.output_dir) and not os.path.isdir(args.output_dir):
        sys.exit(f"output directory already exists: {args.output_dir}")

    print("Loading model...", flush=True)
    try:
        tris = raycast.normalize(raycast.read_stl(args.input_stl))
        if args.rotate:
            raycast.rotating_directions(args.rotation_axis, args.rotation_offset, 1)
    except (OSError, ValueError) as err:
        sys.exit(str(err))
    lo, hi = tris.min(axis=(0, 1)).astype(np.float64), tris.max(axis=(0, 1)).astype(np.float64)
    mesh = None
    if not args.no_images:
        from PIL import Image

        mesh = raycast.TriangleMesh(torch.from_numpy(tris).to(torch.device("cuda", torch.cuda.current_device())))
    os.makedirs(args.output_dir, exist_ok=True)

    print("Writing metadata...", flush=True)
    with open(os.path.join(args.output_dir, "metadata.json"), "w") as f:
        json.dump({"min": lo.tolist(), "max": hi.tolist()}, f)

    print("Creating random lights...", flush=True)
    rs = np.random.RandomState(args.seed)
    lights = raycast.random_lights(rs, lo, hi, args.num_lights, args.light_brightness)
    cameras = None
    if args.rotate:
        cameras = raycast.rotating_cameras(lo, hi, fov, args.rotation_axis, args.rotation_offset, args.images)

    for i in range(args.images):
        print(f"Rendering image {i + 1}/{args.images}...", flush=True)
        camera = cameras[i] if cameras is not None else raycast.random_camera(rs, lo, hi, fov)
        if mesh is not None:
            rgba = mesh.render(camera, args.resolution, args.resolution, lights, args.color)
            Image.fromarray(rgba.cpu().numpy(), "RGBA").save(os.path.join(args.output_dir, f"{i:04d}.png"))
        with open(os.path.join(args.output_dir, f"{i:04d}.json"), "w") as f:
            json.dump(raycast.camera_json(camera), f)


if __name__ == "__main__":
    main()

"""
Run a NeRF model with K-fold cross-validation to find the frames which have the highest validation loss; these might
be samples in the dataset with incorrect camera poses.  The command line of the reference's scripts/cv_nerf.py (same
flags, defaults and output lines: one "{loss} {image_path}" per held-out view), driving learn_nerf.diagnostics: the
validation loss of a view is summed in fp64 in a fixed order on the GPU, so two runs with one seed print the same
digits.  Extra, additive flag: --error_map_dir.  Single process only.
"""
import argparse
import os
import sys

from learn_nerf.dataset import load_dataset
from learn_nerf.diagnostics import cross_validate, error_map_image
from learn_nerf.scripts.train_nerf import add_model_args


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--lr", type=float, default=1e-4)
    parser.add_argument("--batch_size", type=int, default=4096, help="rays per batch")
    parser.add_argument("--folds", type=int, default=10, help="number of training runs to perform")
    parser.add_argument("--coarse_samples", type=int, default=64, help="samples per coarse ray")
    parser.add_argument("--fine_samples", type=int, default=128,
                        help="samples per fine ray (not including coarse samples)")
    parser.add_argument("--train_iters", type=int, default=1500)
    parser.add_argument("--error_map_dir", type=str, default=None,
                        help="(additive) write one 8-bit PNG per held-out view: sqrt(squared error / 3) / 2 per pixel")
    add_model_args(parser)
    parser.add_argument("data_dir", type=str)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.folds < 1 or args.batch_size < 1 or args.train_iters < 0:
        sys.exit("--folds and --batch_size must be positive and --train_iters non-negative")
    from tqdm.auto import tqdm

    print("loading dataset...", flush=True)
    data = load_dataset(args.data_dir)
    maps = None
    if args.error_map_dir is not None:
        from PIL import Image

        os.makedirs(args.error_map_dir, exist_ok=True)
        maps = {}

    def say(message):
        print(message, flush=True)

    for _, results in cross_validate(args, data, say=say, progress=lambda it: tqdm(it, file=sys.stderr),
                                     error_maps=maps):
        for loss, image_path in results:
            print(loss, image_path, flush=True)
        if maps is not None:
            for image_path, ray_err in maps.items():
                name = os.path.splitext(os.path.basename(image_path))[0] + ".png"
                Image.fromarray(error_map_image(ray_err), "L").save(os.path.join(args.error_map_dir, name))
            maps.clear()


if __name__ == "__main__":
    main()

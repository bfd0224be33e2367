"""
Measure the image quality of a checkpoint on a dataset: PSNR and SSIM of every view (additive: the reference has no
such command).  Each view of data_dir is rendered at its own size with the fine model and compared with its image as
[0, 1] pictures (learn_nerf.metrics): PSNR = -10 log10(mse); SSIM as the NeRF papers report it — 11 x 11 Gaussian
window, sigma 1.5, valid region, C1 = 0.01^2, C2 = 0.03^2, mean over pixels and channels, i.e.
skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1,
channel_axis=-1).  Both are reduced in fp64 in a fixed order on the GPU, so two runs with one seed print the same digits.

stdout: one line `psnr=<repr> ssim=<repr> mse=<repr> <image_path>` per view in dataset order, then
`mean: psnr=<repr> ssim=<repr> views=<n>` — the mean PSNR is the mean of the per-view PSNRs, the literature's
convention.  Progress messages go to stderr.  --output_dir receives <stem>.png (the render) and <stem>_ssim.png (the
channel mean of the SSIM map as an 8-bit grey image) per view.  Single process only.
"""
import argparse
import contextlib
import math
import os
import sys

from learn_nerf.dataset import load_dataset
from learn_nerf.metrics import evaluate_views, ssim_map_image
from learn_nerf.scripts.render_nerf import RENDER_FLAGS, RenderSession, quantise
from learn_nerf.scripts.train_nerf import add_model_args

_SHARED = ("--batch_size", "--coarse_samples", "--fine_samples", "--model_path", "--occupancy_grid",
           "--occupancy_threshold", "--occupancy_dilate", "--occupancy_min_component", "--occupancy_keep_largest",
           "--occupancy_connectivity")  # as in render_nerf.py: type, default and meaning


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--seed", type=int, default=0)
    for flag, typ, default, text in RENDER_FLAGS:
        if flag in _SHARED:
            parser.add_argument(flag, type=typ, default=default, help=text)
    parser.add_argument("--output_dir", type=str, default=None,
                        help="write <stem>.png (render) and <stem>_ssim.png (SSIM map) per view")
    add_model_args(parser)
    parser.add_argument("data_dir", type=str, help="a dataset directory; its metadata.json gives the scene box")
    return parser


def format_view(result) -> str:
    return f"psnr={result['psnr']!r} ssim={result['ssim']!r} mse={result['mse']!r} {result['image_path']}"


def format_mean(results) -> str:
    count = len(results)
    psnr = math.fsum(r["psnr"] for r in results) / count
    ssim = math.fsum(r["ssim"] for r in results) / count
    return f"mean: psnr={psnr!r} ssim={ssim!r} views={count}"


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch_size < 1:
        sys.exit("--batch_size must be positive")
    data = load_dataset(args.data_dir)
    if not data.views:
        sys.exit(f"{args.data_dir}: no views")
    args.metadata_json = os.path.join(args.data_dir, "metadata.json")
    with contextlib.redirect_stdout(sys.stderr):  # the session's progress lines
        session = RenderSession(args)
    keep = args.output_dir is not None
    renders, maps = ([], []) if keep else (None, None)
    results = list(evaluate_views(session.key, session.renderer, data, args.batch_size, renders=renders,
                                  ssim_maps=maps))
    for result in results:
        print(format_view(result), flush=True)
    print(format_mean(results), flush=True)
    if keep:
        from PIL import Image

        os.makedirs(args.output_dir, exist_ok=True)
        for result, colors, ssim_map in zip(results, renders, maps):
            stem = os.path.splitext(os.path.basename(result["image_path"]))[0]
            Image.fromarray(quantise(colors.cpu().numpy())).save(os.path.join(args.output_dir, stem + ".png"))
            Image.fromarray(ssim_map_image(ssim_map), "L").save(os.path.join(args.output_dir, stem + "_ssim.png"))


if __name__ == "__main__":
    main()

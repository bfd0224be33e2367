"""
Compute (min, max, mean) of the pixels for rays shooting outside of a scene's bounding box to make sure the bounding
box actually covers everything: anything but the background colour means the box of metadata.json cuts the object.
The command line and the three output lines of the reference's scripts/check_bbox.py; the per-pixel work runs on the
GPU (learn_nerf.diagnostics.bbox_miss_stats, lnrf_view_miss_stats).  When no ray misses the box — the reference
divides by zero there — it prints "every ray hits the bounding box" and exits 0.
"""
import argparse

import torch

from learn_nerf.dataset import load_dataset
from learn_nerf.diagnostics import bbox_miss_stats


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("data_dir")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    from tqdm.auto import tqdm

    dataset = load_dataset(args.data_dir)
    device = torch.device("cuda", torch.cuda.current_device())
    stats = bbox_miss_stats(dataset, device, progress=tqdm)
    if stats["count"] == 0:
        print("every ray hits the bounding box")
        return
    print("min color", stats["min"].tolist())
    print("max color", stats["max"].tolist())
    print("mean color", stats["mean"].tolist())


if __name__ == "__main__":
    main()

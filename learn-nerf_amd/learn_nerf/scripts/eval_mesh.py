"""
Measure the geometry of a mesh against a reference mesh (additive: the reference project has no such command): accuracy,
completeness, Chamfer distance, precision / recall / F-score at distance thresholds, Hausdorff distance and normal
consistency, as learn_nerf/mesh_metrics.py defines them.  Both meshes (.stl, .obj or .ply) are sampled in proportion to
area and every sample is taken to the other mesh by an exact point-to-triangle query on the GPU; the sums are fp64 in a
fixed order, so two runs with one seed print the same digits.
No alignment is estimated (no ICP) and nothing is culled by visibility: both meshes must be in one frame.
Hidden interior surfaces of the reference count against completeness.

--normalize_reference applies the transform scripts/stl_dataset.py applies to its STL before rendering (box centred,
largest coordinate scaled to 1), so a mesh extracted in world coordinates from a model trained on such a dataset
(marching_cubes.py --world_coords) is compared with the STL in the frame it was trained in.

stdout: `samples=`, `pred_triangles=`, `ref_triangles=`, the counts of zero-area triangles that are never sampled and
of samples left out of the normal consistency, `threshold=` per threshold, then one `key=value` line per metric (the
per-threshold ones as `precision[<tau>]=`).
"""
import argparse
import math
import os
import sys

import numpy as np

DEFAULT_THRESHOLD_FRACTION = 0.01  # of the reference box's diagonal


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--samples", type=int, default=1_000_000, help="surface samples per mesh")
    parser.add_argument("--threshold", type=float, action="append", default=None,
                        help="distance threshold of precision / recall / F-score; repeatable (at most 8); default: "
                             "1 %% of the diagonal of the reference's box")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--normalize_reference", action="store_true",
                        help="centre and scale the reference as stl_dataset.py does before rendering")
    parser.add_argument("--per_sample_dir", type=str, default=None,
                        help="write pred_samples.ply and ref_samples.ply: the samples coloured by distance, blue at 0 "
                             "to red at the first threshold and beyond")
    parser.add_argument("predicted", type=str, help="the mesh to judge (.stl, .obj, .ply)")
    parser.add_argument("reference", type=str, help="the ground truth (.stl, .obj, .ply)")
    return parser


def distance_colors(distance: np.ndarray, scale: float) -> np.ndarray:
    t = np.clip(distance.astype(np.float64) / scale, 0.0, 1.0) if scale > 0 else (distance > 0).astype(np.float64)
    return np.stack([t, np.zeros_like(t), 1.0 - t], axis=1)


def format_lines(result) -> list:
    lines = [f"accuracy={result.accuracy!r}", f"completeness={result.completeness!r}", f"chamfer={result.chamfer!r}",
             f"chamfer_l2={result.chamfer_l2!r}"]
    for k, tau in enumerate(result.thresholds):
        lines += [f"precision[{tau!r}]={result.precision[k]!r}", f"recall[{tau!r}]={result.recall[k]!r}",
                  f"f_score[{tau!r}]={result.f_score[k]!r}"]
    return lines + [f"hausdorff={result.hausdorff!r}", f"normal_consistency={result.normal_consistency!r}"]


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.samples < 1:
        sys.exit("--samples must be positive")
    if args.threshold is not None and (len(args.threshold) > 8 or
                                       not all(t >= 0 and math.isfinite(t) for t in args.threshold)):
        sys.exit("--threshold: at most 8 values, each finite and not negative")
    from learn_nerf.mesh_metrics import compare_meshes, read_mesh
    from learn_nerf.point_cloud import write_ply
    from learn_nerf.raycast import normalize

    try:
        pred, ref = read_mesh(args.predicted), read_mesh(args.reference)
        if args.normalize_reference:
            ref = normalize(ref)
    except (OSError, ValueError) as err:
        sys.exit(str(err))
    thresholds = args.threshold
    if thresholds is None:
        flat = ref.reshape(-1, 3).astype(np.float64)
        thresholds = [DEFAULT_THRESHOLD_FRACTION * float(np.linalg.norm(flat.max(axis=0) - flat.min(axis=0)))]
    try:
        result = compare_meshes(pred, ref, samples=args.samples, thresholds=thresholds, seed=args.seed)
    except ValueError as err:
        sys.exit(str(err))
    print(f"samples={result.samples}")
    print(f"pred_triangles={len(pred)}")
    print(f"ref_triangles={len(ref)}")
    print(f"pred_degenerate_triangles_skipped={result.degenerate_triangles[0]}")
    print(f"ref_degenerate_triangles_skipped={result.degenerate_triangles[1]}")
    print(f"normal_samples_skipped={result.normals_skipped}")
    for tau in result.thresholds:
        print(f"threshold={tau!r}")
    for line in format_lines(result):
        print(line, flush=True)
    if args.per_sample_dir is not None:
        os.makedirs(args.per_sample_dir, exist_ok=True)
        for side in ("pred", "ref"):
            points = result.per_sample[side + "_points"].cpu().numpy()
            distance = result.per_sample[side + "_distance"].cpu().numpy()
            write_ply(os.path.join(args.per_sample_dir, side + "_samples.ply"), points,
                      distance_colors(distance, result.thresholds[0]))


if __name__ == "__main__":
    main()

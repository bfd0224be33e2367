"""
Times of the point-cloud export's passes on the GPU, as one JSON line (device events around synchronised work, after a
warm-up; median of --repeats), each with the compulsory bytes of the pass:
  * the search structure over n surface-distributed points (a bumpy unit sphere with a little noise): lnrf_pc_cell_ids
    alone, and PointGrid as a whole (cell ids, the stable sort, the gather and cell_start);
  * knn_dist2 at k = 5 over 1 M and over 26 M such points (the -sort-density pass at the default 100 views of 512^2),
    queries in cell order;
  * the distance field at the default thickness = delta = 0.02 on 50,000 points, and the colour lookup of the mesh's
    vertices;
  * scipy's cKDTree.query(k=5, workers=16) on the same 1 M points as the CPU comparison, when scipy is importable.
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times (pc_cell_ids_kernel, pc_knn_kernel,
pc_nearest_kernel).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learn-nerf_amd"))

from learn_nerf.mesh import marching_cubes  # noqa: E402
from learn_nerf.point_cloud import PointGrid, point_field  # noqa: E402


def timed(fn, repeats):
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def surface_points(n: int, seed: int) -> torch.Tensor:
    """n points on a bumpy unit sphere, 0.002 of radial noise (what back-projected depth images look like)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.randn(n, 3, device="cuda", generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    radius = 1 + 0.08 * torch.sin(9 * d[:, 0]) * torch.sin(7 * d[:, 1]) * torch.sin(8 * d[:, 2])
    radius = radius + 0.002 * torch.randn(n, device="cuda", generator=gen)
    return (d * radius[:, None]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 26_000_000])
    ap.add_argument("--field_points", type=int, default=50_000)
    ap.add_argument("--cpu_points", type=int, default=1_000_000, help="0 skips the cKDTree comparison")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {}

    PointGrid(surface_points(10_000, 0)).knn_dist2(surface_points(1_000, 1), 5)  # warm-up: code objects
    for n in args.sizes:
        points = surface_points(n, 2)
        grid = PointGrid(points)
        cells = math.prod(grid.dims)
        tag = f"{n / 1e6:g}M"
        out[f"grid_{tag}"] = dict(dims=grid.dims, h=float(grid.h),
                                  occupied_cells=int((grid.cell_start[1:] > grid.cell_start[:-1]).sum()))
        out[f"cell_ids_{tag}_ms"] = timed(lambda: grid.cell_ids(points), args.repeats)
        out[f"cell_ids_{tag}_min_bytes"] = n * (12 + 4)
        out[f"point_grid_{tag}_ms"] = timed(lambda: PointGrid(points), args.repeats)
        # ids written, sorted (keys and indices read and written once at the least), points gathered, cell_start
        out[f"point_grid_{tag}_min_bytes"] = n * (12 + 4) + n * (4 + 8) * 2 + n * (12 + 12 + 4) + 4 * cells
        out[f"knn5_{tag}_ms"] = timed(lambda: grid.knn_dist2(grid.sorted_points, 5, sort=False), args.repeats)
        out[f"knn5_{tag}_min_bytes"] = n * (12 + 12 + 4) + 4 * cells  # queries, points, result, cell_start
        del grid, points

    points = surface_points(args.field_points, 3)
    thickness = delta = 0.02
    volume, origin, dims = point_field(points, thickness, delta)
    out["field_dims"] = dims
    out["field_ms"] = timed(lambda: point_field(points, thickness, delta), args.repeats)
    out["field_min_bytes"] = math.prod(dims) * 4 + args.field_points * 16  # the volume written, the cloud read
    grid = PointGrid(points)
    verts, faces = marching_cubes(volume, 0.0)
    world = torch.from_numpy((origin + verts.cpu().numpy().astype(np.float64) * delta).astype(np.float32)).cuda()
    out["mesh_vertices"], out["mesh_faces"] = verts.shape[0], faces.shape[0]
    out["color_lookup_ms"] = timed(lambda: grid.nearest(world), args.repeats)
    out["color_lookup_min_bytes"] = verts.shape[0] * (12 + 8) + args.field_points * 16

    if args.cpu_points:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            out["ckdtree"] = "scipy not importable"
        else:
            cloud = surface_points(args.cpu_points, 2).cpu().numpy()
            t0 = time.perf_counter()
            tree = cKDTree(cloud)
            t1 = time.perf_counter()
            dist, _ = tree.query(cloud, k=5, workers=16)
            t2 = time.perf_counter()
            out[f"ckdtree_build_{args.cpu_points / 1e6:g}M_ms"] = (t1 - t0) * 1e3
            out[f"ckdtree_query_k5_workers16_{args.cpu_points / 1e6:g}M_ms"] = (t2 - t1) * 1e3
            # the same answer up to float64 vs float32 rounding
            got = PointGrid(torch.from_numpy(cloud).cuda()).knn_dist2(torch.from_numpy(cloud).cuda(), 5).cpu().numpy()
            out["ckdtree_max_rel_diff"] = float(np.max(np.abs(np.sqrt(got) - dist[:, 4]) / dist[:, 4]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

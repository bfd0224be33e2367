"""
Time of every pass of the mesh simplifier on the GPU (DESIGN.md section 5 "Mesh simplification"): the marching-cubes
mesh of a sphere of radius 0.4 * --resolution grid steps, simplified on grids of --grids cells along the longest axis.
Each pass on its own with device events (median, min, max of seven after two warm-up calls) and the bytes it has to
move, computed from the shapes: keys, sort, segments, the fold in its three launch shapes, placement, survivor count,
the faces (torch), flipped; then one whole simplify() and one target_faces search in host wall time ending in a device
synchronise.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learn-nerf_amd"))

from learn_nerf import ops  # noqa: E402
from learn_nerf import simplify as M  # noqa: E402
from learn_nerf.mesh import marching_cubes  # noqa: E402


def sphere_mesh(res: int, device) -> torch.Tensor:
    ax = torch.arange(res, device=device, dtype=torch.float32) - (res - 1) / 2
    dist = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    verts, faces = marching_cubes((0.4 * res - dist).contiguous(), 0.0)
    return verts[faces.long()].contiguous()


def timed(call, repeats=7):
    call()
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        out = call()
        end.record()
        torch.cuda.synchronize()
        times.append(begin.elapsed_time(end) * 1e3)
    return out, (float(np.median(times)), min(times), max(times))


def report(name, times, nbytes=None):
    rate = "" if nbytes is None else f"  {nbytes / 1e6:.1f} MB -> {nbytes / times[0] / 1e3:.0f} GB/s"
    print(f"  {name}: median {times[0]:.1f} us, min {times[1]:.1f}, max {times[2]:.1f}{rate}", flush=True)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--resolution", type=int, default=512)
    parser.add_argument("--grids", type=int, nargs="+", default=[256, 128, 16])
    args = parser.parse_args(argv)
    device = torch.device("cuda", 0)
    tris = sphere_mesh(args.resolution, device)
    n_tris, pts = tris.shape[0], tris.view(-1, 3)
    lo, hi = pts.amin(0).cpu().numpy(), pts.amax(0).cpu().numpy()
    for cells_along in args.grids:
        h, inv_h, dims = M.choose_grid(lo, hi, cells=cells_along)
        grid = ops.simp_grid(lo, inv_h, dims)
        keys, t_keys = timed(lambda: ops.simp_cell_keys(grid, pts))
        (sorted_keys, order), t_sort = timed(lambda: torch.sort(keys, stable=True))

        def segments():
            cells, lengths = torch.unique_consecutive(sorted_keys, return_counts=True)
            start = torch.zeros(cells.numel() + 1, dtype=torch.int32, device=device)
            start[1:] = torch.cumsum(lengths, 0)
            return cells, lengths, start

        (cells, lengths, seg_start), t_seg = timed(segments)
        n_cells, order32 = cells.numel(), order.to(torch.int32)
        print(f"resolution={args.resolution} faces={n_tris} grid={cells_along} cells={n_cells} "
              f"mean segment={3 * n_tris / n_cells:.1f} longest={int(lengths.max())}", flush=True)
        report("keys", t_keys, 3 * n_tris * (12 + 4))
        report("sort (torch)", t_sort)
        report("segments (torch)", t_seg)
        fold_bytes = 3 * n_tris * (4 + 36 + 12) + n_cells * (4 + 4 + 13 * 8)  # order, triangle, its keys; start, outputs
        for shape in ("auto", "groups", "waves"):
            (counts, sums, _), t = timed(lambda: ops.simp_accumulate(tris, keys, order32, seg_start, None, shape))
            report(f"fold {shape}", t, fold_bytes)
        (cell_verts, _, _), t = timed(lambda: ops.simp_place(grid, h, cells, counts, sums, None, "quadric"))
        report("place", t, n_cells * (4 + 4 + 13 * 8 + 12 + 1))
        count = torch.zeros(1, dtype=torch.int64, device=device)
        _, t = timed(lambda: ops.simp_count_faces_(grid, tris, count))
        report("count_faces", t, n_tris * 36)

        def faces_pass():
            src, face_keys, _ = M.surviving_faces(keys)
            used = torch.unique(face_keys)
            slot = torch.searchsorted(cells.long(), used)
            faces = torch.searchsorted(used, face_keys.reshape(-1)).reshape(-1, 3).to(torch.int32).contiguous()
            return src.to(torch.int32), faces, cell_verts[slot].contiguous()

        (src, faces, verts), t = timed(faces_pass)
        report("faces (torch)", t)
        _, t = timed(lambda: ops.simp_flipped(tris, src, faces, verts))
        report("flipped", t, faces.shape[0] * (4 + 12 + 36 + 36))
        torch.cuda.synchronize()
        start = time.perf_counter()
        out = M.simplify(tris, grid=cells_along)
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - start)
        print(f"  simplify(): {wall:.2f} ms  " + " ".join(M.format_info(out.info)), flush=True)
    torch.cuda.synchronize()
    start = time.perf_counter()
    out = M.simplify(tris, target_faces=n_tris // 10)
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - start)
    print(f"target_faces={n_tris // 10}: {wall:.2f} ms  " + " ".join(M.format_info(out.info)), flush=True)


if __name__ == "__main__":
    main()

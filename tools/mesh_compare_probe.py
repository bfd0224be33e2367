"""
Time of one mesh comparison on the GPU (DESIGN.md section 4 "Mesh comparison"): compare_meshes at --samples per side
between two icospheres of 20 * 4^--subdivisions triangles (radii 1.01 and 1), in host wall time around work that ends
in a device synchronise, one warm-up call first; then its parts on their own with device events (median, min, max of
five): building a TriangleMesh, sample_surface, and nearest for one direction.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learn-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raycast_reference as R  # noqa: E402
from learn_nerf.mesh_metrics import compare_meshes  # noqa: E402
from learn_nerf.raycast import TriangleMesh  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--samples", type=int, default=1_000_000)
    parser.add_argument("--subdivisions", type=int, default=8)
    parser.add_argument("--repeats", type=int, default=3)
    args = parser.parse_args(argv)
    pred = torch.from_numpy(R.icosphere(args.subdivisions, radius=1.01)).cuda()
    ref = torch.from_numpy(R.icosphere(args.subdivisions, radius=1.0)).cuda()
    print(f"triangles={pred.shape[0]} samples={args.samples}", flush=True)
    for rep in range(args.repeats + 1):
        torch.cuda.synchronize()
        start = time.perf_counter()
        result = compare_meshes(pred, ref, samples=args.samples, thresholds=(0.02,), seed=0)
        torch.cuda.synchronize()
        label = "warm-up" if rep == 0 else f"run {rep}"
        print(f"{label}: compare_meshes {time.perf_counter() - start:.4f} s  accuracy={result.accuracy!r} "
              f"completeness={result.completeness!r} hausdorff={result.hausdorff!r}", flush=True)
    mesh_pred, mesh_ref = TriangleMesh(pred), TriangleMesh(ref)
    points, _ = mesh_pred.sample_surface(args.samples, 0)
    parts = (("build", lambda: TriangleMesh(ref)), ("sample_surface", lambda: mesh_pred.sample_surface(args.samples, 0)),
             ("nearest", lambda: mesh_ref.nearest(points)))
    for name, call in parts:
        call()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            call()
            end.record()
            torch.cuda.synchronize()
            times.append(begin.elapsed_time(end))
        print(f"{name}: median {float(np.median(times)):.3f} ms, min {min(times):.3f}, max {max(times):.3f}", flush=True)


if __name__ == "__main__":
    main()

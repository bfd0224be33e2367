"""
Times of the STL dataset producer's passes on the GPU, as one JSON line (device events around synchronised work, after
a warm-up; median of --repeats):
  * TriangleMesh as a whole (Morton codes, the stable sort, the gather, the bounds) and lnrf_rt_fit's share, and closest
    and occluded in rays per second over one 800^2 view from a fitted camera, on the 12-triangle cube, on an icosphere
    of 20,480 triangles and on one of 1,310,720;
  * the NumPy brute force of tests/raycast_reference.py on the cube over the same view, for scale;
  * one run at the command's defaults (--views 100 of 800^2, 5 lights) on the 20,480-triangle icosphere, split into
    trace (closest), shade (the float64 shading and its 5 shadow-ray passes) and PNG encoding, in host wall time around
    synchronised work.
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times (rt_morton_kernel, rt_fit_leaves_kernel,
rt_fit_level_kernel, rt_closest_kernel, rt_occluded_kernel).
"""
import argparse
import io
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learn-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raycast_reference as R  # noqa: E402
from learn_nerf import _lib as L  # noqa: E402
from learn_nerf import raycast  # noqa: E402


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


def fitted_view(tris, fov, seed):
    lo, hi = tris.min(axis=(0, 1)), tris.max(axis=(0, 1))
    return raycast.random_camera(np.random.RandomState(seed), lo, hi, fov)


def main():
    import ctypes

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=800)
    ap.add_argument("--subdivisions", type=int, nargs="+", default=[5, 8])
    ap.add_argument("--views", type=int, default=100, help="views of the default run; 0 skips it")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    fov = math.radians(60.0)
    size = args.resolution
    out = {"rays": size * size}

    meshes = {"cube12": raycast.normalize(R.cube(0.5))}
    for s in args.subdivisions:
        meshes[f"icosphere{20 * 4 ** s}"] = R.icosphere(s)
    warm = raycast.TriangleMesh(torch.from_numpy(meshes["cube12"]).cuda())
    warm.render(fitted_view(meshes["cube12"], fov, 0), 16, 16, [[0.0, 0.0, 1000.0, 0.5]], (0.8, 0.8, 0.0))

    for tag, tris_np in meshes.items():
        tris = torch.from_numpy(tris_np).cuda()
        mesh = raycast.TriangleMesh(tris)
        rays = fitted_view(tris_np, fov, 1).bare_rays(size, size, device="cuda")
        t, idx = mesh.closest(rays)
        out[f"{tag}_hit_fraction"] = float((idx >= 0).float().mean())
        out[f"{tag}_build_ms"] = timed(lambda: raycast.TriangleMesh(tris), args.repeats)
        out[f"{tag}_fit_ms"] = timed(lambda: L.check(L.lib().lnrf_rt_fit(
            ctypes.byref(mesh.bvh), L.ptr(mesh.sorted_tris), L.ptr(mesh.nodes), L.stream())), args.repeats)
        t_out, id_out = torch.empty_like(t), torch.empty_like(idx)
        occ_out = torch.empty(rays.shape[0], dtype=torch.uint8, device="cuda")
        lib, bvh = L.lib(), ctypes.byref(mesh.bvh)
        ms = timed(lambda: lib.lnrf_rt_closest(bvh, L.ptr(mesh.sorted_tris), L.ptr(mesh.order, torch.int32),
                                               L.ptr(mesh.nodes), L.ptr(rays), None, rays.shape[0], L.ptr(t_out),
                                               L.ptr(id_out, torch.int32), L.stream()), args.repeats)
        out[f"{tag}_closest_ms"], out[f"{tag}_closest_Mrays_s"] = ms, rays.shape[0] / ms / 1e3
        ms = timed(lambda: lib.lnrf_rt_occluded(bvh, L.ptr(mesh.sorted_tris), L.ptr(mesh.nodes), L.ptr(rays), None,
                                                rays.shape[0], L.ptr(occ_out, torch.uint8), L.stream()), args.repeats)
        out[f"{tag}_occluded_ms"], out[f"{tag}_occluded_Mrays_s"] = ms, rays.shape[0] / ms / 1e3
        if tag == "cube12":
            host_rays = rays.cpu().numpy()
            t0 = time.perf_counter()
            ref_t, ref_id, _ = R.brute_force(tris_np, host_rays, chunk=1 << 16)
            out["cube12_numpy_brute_force_ms"] = (time.perf_counter() - t0) * 1e3
            out["cube12_equals_numpy"] = bool(np.array_equal(ref_id, idx.cpu().numpy())
                                              and np.array_equal(ref_t, t.cpu().numpy()))
        del mesh, tris, rays

    if args.views:
        from PIL import Image

        tag = f"icosphere{20 * 4 ** args.subdivisions[0]}"
        tris_np = meshes[tag]
        mesh = raycast.TriangleMesh(torch.from_numpy(tris_np).cuda())
        lo, hi = tris_np.min(axis=(0, 1)), tris_np.max(axis=(0, 1))
        rs = np.random.RandomState(0)
        lights = raycast.random_lights(rs, lo, hi, 5, 0.5)
        trace = shade = png = 0.0
        for _ in range(args.views):
            view = raycast.random_camera(rs, lo, hi, fov)
            rays = view.bare_rays(size, size, device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t, idx = mesh.closest(rays)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rgba = mesh.shade(rays, t, idx, lights, (0.8, 0.8, 0.0)).view(size, size, 4).cpu().numpy()
            t2 = time.perf_counter()
            Image.fromarray(rgba, "RGBA").save(io.BytesIO(), format="PNG")
            t3 = time.perf_counter()
            trace, shade, png = trace + (t1 - t0), shade + (t2 - t1), png + (t3 - t2)
        out[f"default_run_{tag}_{args.views}views"] = dict(trace_s=trace, shade_s=shade, png_s=png)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

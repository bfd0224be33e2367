"""
Times of the TSDF export's passes beside their byte floors, one JSON line per resolution, appended to --out:

  python tools/tsdf_probe.py [--resolutions 256 512] [--views 100] [--size 512] [--repeats 7] [--out profiles/tsdf_probe.jsonl]

The scene is synthetic and seeded by nothing: a sphere of radius 0.6 in the box [-1, 1]^3 seen by `views` pinhole cameras
of `size`^2 pixels on a Fibonacci spiral of radius 4.  Timed, each after one warm-up call, `repeats` times, median and
[min, max] reported: lnrf_tsdf_integrate over all views in one launch (inputs already on the device; device events),
TsdfVolume.integrate end to end (packing, upload and launch; host clock around a synchronise), lnrf_tsdf_volume,
marching cubes (count, read-back, emit; host clock around a synchronise) and lnrf_tsdf_vertex_colors.

floor_us is bytes / HBM_BYTES_PER_S with the bytes a pass must move once per the shapes: integrate reads and writes the
25 bytes of state per voxel and reads the 5 bytes per pixel of the launch's images; volume reads 9 bytes per voxel and
writes 4 per padded point; marching cubes reads the padded volume in both passes and writes vertices and faces; the
colour pass reads and writes 12 bytes per vertex and gathers two 16-byte state entries.  The integration is arithmetic
per voxel and view, not traffic: valu_floor_us is voxels * views * OPS_PER_UPDATE lane-operations over the chip's
fp32 vector issue rate, with OPS_PER_UPDATE counted from the kernel's ISA.  These are measurements, not gates.
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

from learn_nerf.dataset import CameraView  # noqa: E402
from learn_nerf.mesh import marching_cubes  # noqa: E402
from learn_nerf.tsdf import TsdfVolume  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # achievable HBM rate of an MI355X (8 TB/s peak)
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9  # 256 CUs x 4 SIMDs x 32 lanes at 2.4 GHz: one fp32 vector operation per lane and clock
OPS_PER_UPDATE = 128  # vector instructions per voxel and view on the longest path (a hit with a colour; 4 divisions)
RADIUS, CAMERA_RADIUS, FOV, MAX_DEPTH = 0.6, 4.0, 0.6, 10.0


def fibonacci_cameras(n):
    cams = []
    for i in range(n):
        h = 1 - 2 * (i + 0.5) / n
        phi = i * math.pi * (3 - math.sqrt(5))
        z = np.array([math.sqrt(1 - h * h) * math.cos(phi), math.sqrt(1 - h * h) * math.sin(phi), h])
        x = np.array([z[1], -z[0], 0.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
        x = x - z * (x @ z)
        x /= np.linalg.norm(x)
        cams.append(CameraView(camera_direction=tuple(z), camera_origin=tuple(-z * CAMERA_RADIUS), x_axis=tuple(x),
                               y_axis=tuple(np.cross(z, x)), x_fov=FOV, y_fov=FOV))
    return cams


def render(cam, size):
    u = np.linspace(-1, 1, size) * math.tan(FOV / 2)
    d = (np.asarray(cam.camera_direction) + u[None, :, None] * np.asarray(cam.x_axis)
         + u[:, None, None] * np.asarray(cam.y_axis)).reshape(-1, 3)
    o = np.asarray(cam.camera_origin)
    a, b = (d * d).sum(1), d @ o
    disc = b * b - a * (o @ o - RADIUS ** 2)
    hit = disc > 0
    t = (-b - np.sqrt(np.where(hit, disc, 0.0))) / a
    depth = np.where(hit, np.floor(t * (d @ np.asarray(cam.camera_direction)) / MAX_DEPTH * 65535), 0xFFFF)
    normal = (o + d * t[:, None]) / RADIUS
    color = np.where(hit[:, None], np.rint((normal * 0.5 + 0.5) * 255), 0)
    return depth.astype(np.uint16).reshape(size, size), color.astype(np.uint8).reshape(size, size, 3)


def timed_events(fn, repeats):
    fn()  # warm-up: code object, allocator
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def timed_host(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def report(out, name, times, nbytes):
    times = sorted(times)
    median = times[len(times) // 2]
    out[f"{name}_us"] = round(median, 1)
    out[f"{name}_us_min_max"] = [round(times[0], 1), round(times[-1], 1)]
    if nbytes is not None:
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        out[f"{name}_bytes"] = int(nbytes)
        out[f"{name}_floor_us"] = round(floor, 1)
        out[f"{name}_over_floor"] = round(median / floor, 2)


def measure(resolution, cameras, depths, colors, repeats):
    vol = TsdfVolume((-1, -1, -1), (1, 1, 1), resolution, max_depth=MAX_DEPTH, device="cuda")
    n, padded = resolution ** 3, (resolution + 2) ** 3
    pixels = sum(d.size for d in depths)
    out = dict(resolution=resolution, views=len(cameras), pixels_per_view=depths[0].size, repeats=repeats)
    # the mesh comes from a single fusion; the timed launches that follow add the same views again
    vol.integrate(cameras, depths, colors)
    volume = vol.volume()
    verts, faces = marching_cubes(volume, 0.0)
    out.update(vertices=verts.shape[0], faces=faces.shape[0], uncoloured=vol.vertex_colors(verts)[1])
    report(out, "volume", timed_events(vol.volume, repeats), 9 * n + 4 * padded)
    report(out, "marching_cubes", timed_host(lambda: marching_cubes(volume, 0.0), repeats),
           2 * 4 * padded + 12 * (verts.shape[0] + faces.shape[0]))
    report(out, "vertex_colors", timed_events(lambda: vol.vertex_colors(verts), repeats), (24 + 32) * verts.shape[0])
    uploaded = vol.upload(cameras, depths, colors)
    report(out, "integrate", timed_events(lambda: vol.integrate_uploaded(*uploaded), repeats), 50 * n + 5 * pixels)
    valu_floor = n * len(cameras) * OPS_PER_UPDATE / LANE_OPS_PER_S * 1e6
    out["integrate_valu_floor_us"] = round(valu_floor, 1)
    out["integrate_over_valu_floor"] = round(out["integrate_us"] / valu_floor, 2)
    out["integrate_ns_per_voxel_view"] = round(out["integrate_us"] * 1e3 / (n * len(cameras)), 5)
    del uploaded
    report(out, "integrate_with_upload", timed_host(lambda: vol.integrate(cameras, depths, colors), max(3, repeats // 2)),
           None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "tsdf_probe.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_probe needs a GPU")
    torch.cuda.set_device(0)
    cameras = fibonacci_cameras(args.views)
    images = [render(c, args.size) for c in cameras]
    depths, colors = [i[0] for i in images], [i[1] for i in images]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for resolution in args.resolutions:
        line = json.dumps(measure(resolution, cameras, depths, colors, args.repeats))
        print(line, flush=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

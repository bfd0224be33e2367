"""
Times of a texture bake beside their floors, one JSON line per mesh, appended to --out:

  python tools/texture_probe.py [--subdivisions 5 6] [--views 100] [--size 512] [--texture_size 2048] [--repeats 5]
                                [--out profiles/texture_probe.jsonl]

The scene is the one of tools/tsdf_probe.py: a sphere of radius 0.6 seen by `views` pinhole cameras of `size`^2 pixels on
a Fibonacci spiral of radius 4, coloured by its normal on a transparent background; the mesh is the icosphere of
20 * 4^subdivisions faces.  Timed, each after one warm-up call, `repeats` times, median and [min, max] reported:
lnrf_tex_bake_views over all views in one launch (inputs already on the device; device events), lnrf_tex_resolve, one
lnrf_tex_fill pass, bake_views end to end (packing, upload, launches, fill; host clock around a synchronise).  Then
reprojection_psnr over the views.

Floors.  traversals = the (texel, view) pairs that pass the facing, footprint and alpha tests and so start a walk of the
tree, counted by restating those tests with torch in fp32 (not bit-pinned: a pair on a threshold may differ).  The bake
is arithmetic and dependent loads, not traffic, so it gets two floors: bake_floor_us (bytes: 32 per texel of state, 4
per pixel once) and bake_valu_floor_us = (live texels * views * OPS_CULL + traversals * OPS_ROOT) lane-operations over
the chip's fp32 vector issue rate: every pair pays the facing test, and every started walk tests at least the root
node.  A walk that goes deeper does more; the floor does not know how much.  These are measurements, not gates.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_nerf.raycast import TriangleMesh  # noqa: E402
from learn_nerf.texture import TextureAtlas, TextureBake, bake_views, fill, pack_views, reprojection_psnr  # noqa: E402
from tsdf_probe import RADIUS, fibonacci_cameras, render, report, timed_events, timed_host  # noqa: E402

LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
OPS_CULL = 24  # v = o - p, |v|, l = v / |v|, n . l and the compare: the least a (texel, view) pair costs
OPS_ROOT = 36  # one node test: six plane distances, their products, the interval's min / max chain


def icosphere(subdivisions, radius):
    p = (1 + math.sqrt(5)) / 2
    verts = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
             (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
             (8, 6, 7), (9, 8, 1)]
    tris = np.asarray(verts, np.float64)[np.asarray(faces)]
    for _ in range(subdivisions):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        tris = np.concatenate([np.stack(t, axis=1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    tris = tris / np.linalg.norm(tris, axis=2, keepdims=True) * radius
    return tris.astype(np.float32)


def count_traversals(atlas, bake, views, images_dev, sizes):
    """(live texels, traversals): the culling tests of csrc/tex_geom.h "Bake" restated with torch in fp32."""
    face, p, n, _ = atlas.texels()
    live = (face >= 0) & (n.abs().sum(-1) > 0)
    p, n = p[live], n[live]
    total = 0
    for view, image, (width, height) in zip(views, images_dev, sizes):
        origin = torch.from_numpy(view["origin"].copy()).to(p)
        inv = torch.from_numpy(view["inv"].copy()).to(p).view(3, 3)
        v = origin - p
        l = v / v.norm(dim=-1, keepdim=True)
        ok = (n * l).sum(-1) > bake.cos_max
        d = (p - origin) @ inv.T
        xf = (d[:, 0] / d[:, 2] + 1) * 0.5 * (width - 1)
        yf = (d[:, 1] / d[:, 2] + 1) * 0.5 * (height - 1)
        ok &= (d[:, 2] > 0) & (xf >= 0) & (xf <= width - 1) & (yf >= 0) & (yf <= height - 1)
        x0, y0 = xf.floor().clamp(0, width - 1).long(), yf.floor().clamp(0, height - 1).long()
        x1, y1 = (x0 + (xf > x0)).clamp(max=width - 1), (y0 + (yf > y0)).clamp(max=height - 1)
        alpha = image[:, :, 3]
        ok &= (alpha[y0, x0] >= 128) & (alpha[y0, x1] >= 128) & (alpha[y1, x0] >= 128) & (alpha[y1, x1] >= 128)
        total += int(ok.sum())
    return int(live.sum()), total


def measure(subdivisions, cameras, images, texture_size, repeats):
    tris = torch.from_numpy(icosphere(subdivisions, RADIUS)).cuda()
    atlas, mesh = TextureAtlas(tris, texture_size), TriangleMesh(tris)
    out = dict(faces=atlas.F, texture_size=atlas.S, cell=atlas.c, views=len(cameras),
               pixels_per_view=images[0].shape[0] * images[0].shape[1], repeats=repeats)
    bake = TextureBake(atlas, mesh)
    uploaded = bake.upload(cameras, images)
    sizes = [(im.shape[1], im.shape[0]) for im in images]
    live, traversals = count_traversals(atlas, bake, pack_views(cameras, sizes), [torch.from_numpy(i).cuda() for i in images],
                                        sizes)
    n, pixels = atlas.S * atlas.S, sum(w * h for w, h in sizes)
    out.update(texels=n, texels_live=live, traversals=traversals,
               traversals_per_live_texel=round(traversals / live, 3))
    report(out, "bake", timed_events(lambda: bake.add_uploaded(*uploaded), repeats), 32 * n + 4 * pixels)
    valu_floor = (live * len(cameras) * OPS_CULL + traversals * OPS_ROOT) / LANE_OPS_PER_S * 1e6
    out["bake_valu_floor_us"] = round(valu_floor, 1)
    out["bake_over_valu_floor"] = round(out["bake_us"] / valu_floor, 2)
    out["bake_ns_per_traversal"] = round(out["bake_us"] * 1e3 / traversals, 4)
    del uploaded
    report(out, "resolve", timed_events(bake.resolve, repeats), (16 + 4) * n)
    rgb, seen = bake.resolve()
    report(out, "fill_pass", timed_events(lambda: fill(atlas, rgb, seen, 1), repeats), 2 * 4 * n)
    report(out, "bake_views_end_to_end", timed_host(lambda: bake_views(atlas, mesh, cameras, images, verbose=False),
                                                   max(3, repeats // 2)), None)
    texture, info = bake_views(atlas, mesh, cameras, images, verbose=False)
    out.update({k: info[k] for k in ("texels_used", "seen", "filled", "unseen", "degenerate_faces")})
    t0 = time.perf_counter()
    per_view, mean = reprojection_psnr(atlas, mesh, texture, cameras, images)
    torch.cuda.synchronize()
    out.update(reprojection_psnr_mean=round(mean, 3), reprojection_psnr_min=round(min(per_view), 3),
               reprojection_psnr_max=round(max(per_view), 3), reprojection_psnr_s=round(time.perf_counter() - t0, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivisions", type=int, nargs="+", default=[5, 6])
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--texture_size", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "texture_probe.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_probe needs a GPU")
    torch.cuda.set_device(0)
    cameras = fibonacci_cameras(args.views)
    images = []
    for cam in cameras:
        depth, color = render(cam, args.size)
        alpha = np.where(depth == 0xFFFF, 0, 255).astype(np.uint8)
        images.append(np.ascontiguousarray(np.concatenate([color, alpha[:, :, None]], axis=2)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for subdivisions in args.subdivisions:
        line = json.dumps(measure(subdivisions, cameras, images, args.texture_size, args.repeats))
        print(line, flush=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

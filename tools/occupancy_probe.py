"""
Measurements of the occupancy grid on the synthetic cube scene (scripts/make_cube_dataset.py's analytic ray-caster,
trained as tests/test_gpu_psnr_parity.py trains it), one JSON line per run:

  train CKPT             train the scene from one seed (bf16 kernels, the annealed schedule of the PSNR test), save CKPT
  diff CKPT              render one 64x64 view with --occupancy_grid 64 and without, same seed, the CLI's default sample
                         counts: largest absolute difference of the fine RGB (float, and in 8-bit steps), and for scale
                         the same difference between two seeds of the renderer without a grid
  speed CKPT --grid R --batch_size B
                         HIP-event median of rendering one 256x256 view through RenderSession at 64 + 128 samples, with
                         R = 0 (no grid) or a grid, the live-ray fraction and the one-off cost of building the grid.
                         Run every configuration in a process of its own.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learn-nerf_amd"))

from learn_nerf.dataset import CameraView  # noqa: E402
from learn_nerf.rng import Key  # noqa: E402
from learn_nerf.scripts import make_cube_dataset as mk  # noqa: E402
from learn_nerf.scripts import render_nerf  # noqa: E402

FOV, RADIUS = math.radians(40.0), 2.5
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
SCHEDULE = ((900, 5e-4), (500, 1e-4), (300, 2e-5))


def camera(seed):
    origin, x, y, z = mk.random_camera(np.random.default_rng(seed), RADIUS)
    return CameraView(camera_direction=tuple(z), camera_origin=tuple(origin), x_axis=tuple(x), y_axis=tuple(y),
                      x_fov=FOV, y_fov=FOV), (origin, x, y, z)


def train(path):
    from learn_nerf.model import NeRFModel
    from learn_nerf.train import TrainLoop

    size, rows = 32, []
    for seed in range(24):
        view, (origin, x, y, z) = camera(seed)
        rgba = mk.render_cube(origin, x, y, z, FOV, size).astype(np.float64)
        rgb = np.round(rgba[..., :3] * (rgba[..., 3:] / 255)).astype(np.uint8)
        col = rgb.reshape(-1, 1, 3).astype(np.float32) / 127.5 - 1
        rows.append(np.concatenate([view.bare_rays(size, size).numpy(), col], axis=1).astype(np.float32))
    rays = torch.from_numpy(np.concatenate(rows)).cuda()
    loop = TrainLoop(NeRFModel(), NeRFModel(), init_rng=5, lr=SCHEDULE[0][1], coarse_ts=16, fine_ts=32)
    step = loop.step_fn(BMIN, BMAX)
    gen = torch.Generator().manual_seed(104)
    i, log = 0, {}
    for n_steps, lr in SCHEDULE:
        loop.lr = lr
        for _ in range(n_steps):
            idx = torch.randint(0, rays.shape[0], (512,), generator=gen)
            log = step(Key(i), rays[idx.cuda()].contiguous())
            i += 1
    loop.save(path)
    return dict(mode="train", steps=i, fine_loss=float(log["fine"]))


def session(ckpt, grid, batch_size, size, meta_dir):
    meta = os.path.join(meta_dir, "metadata.json")
    with open(meta, "w") as handle:
        json.dump({"min": list(BMIN), "max": list(BMAX)}, handle)
    flags = ["--seed", "0", "--batch_size", str(batch_size), "--width", str(size), "--height", str(size),
             "--model_path", ckpt, "--occupancy_grid", str(grid), meta]
    return render_nerf.RenderSession(render_nerf.argparser().parse_args(flags))


def diff(ckpt, meta_dir):
    view, _ = camera(1000)
    images = []
    for grid, seed in ((0, 0), (64, 0), (0, 1)):  # the third: the same renderer under other sampling noise
        s = session(ckpt, grid, 1024, 64, meta_dir)
        rays = view.bare_rays(64, 64, device=s.device)
        key, pieces = Key(seed), []
        for start in range(0, rays.shape[0], 1024):
            key, slice_key = key.split(2)
            pieces.append(s.render_fn(slice_key, rays[start:start + 1024].contiguous()))
        images.append(torch.cat(pieces).cpu())
        if grid:
            fraction = s.renderer.occupancy.occupied_fraction
    delta = (images[0] - images[1]).abs()
    noise = (images[0] - images[2]).abs()
    steps = np.abs(render_nerf.quantise(images[0].numpy()).astype(int) - render_nerf.quantise(images[1].numpy()))
    return dict(mode="diff", size=64, grid=64, occupied_fraction=fraction, max_abs_rgb=float(delta.max()),
                mean_abs_rgb=float(delta.mean()), max_8bit_steps=int(steps.max()),
                pixels_differing_8bit=int((steps.max(axis=-1) > 0).sum()),
                no_grid_seed0_vs_seed1_max_abs_rgb=float(noise.max()),
                no_grid_seed0_vs_seed1_mean_abs_rgb=float(noise.mean()))


def events(fn, repeats):
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


def speed(ckpt, grid, batch_size, repeats, meta_dir):
    from learn_nerf.occupancy import OccupancyGrid

    view, _ = camera(1000)
    s = session(ckpt, grid, batch_size, 256, meta_dir)
    out = dict(mode="speed", size=256, grid=grid, batch_size=batch_size, samples="64+128", repeats=repeats)

    def render():
        s.images.clear()
        s.render_view(view)

    render()  # warm-up: code objects, weight packing, allocator
    out["view_ms"] = events(render, repeats)
    if grid:
        out["grid_build_ms"] = events(lambda: OccupancyGrid.from_renderer(s.renderer, grid), 3)
        out["occupied_fraction"] = s.renderer.occupancy.occupied_fraction
        rays = view.bare_rays(256, 256, device=s.device)
        t_min, t_max, mask = s.renderer.t_range(rays)
        live = s.renderer.occupancy.clip(rays, t_min, t_max, mask)[2]
        out["box_ray_fraction"] = float(mask.float().mean())
        out["live_ray_fraction"] = float(live.float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("train", "diff", "speed"))
    ap.add_argument("ckpt")
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    meta_dir = os.path.dirname(os.path.abspath(args.ckpt))
    if args.mode == "train":
        out = train(args.ckpt)
    elif args.mode == "diff":
        out = diff(args.ckpt, meta_dir)
    else:
        out = speed(args.ckpt, args.grid, args.batch_size, args.repeats, meta_dir)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

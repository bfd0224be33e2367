"""
Time of lnrf_distortion (ops.distortion, loss + gradient accumulated into g_density) beside lnrf_composite_bwd_det
(ops.composite_bwd, no aux channels) on the same rays, one JSON line per shape:

  python tools/distortion_probe.py [--rays 4096] [--samples 64 192] [--repeats 10] [--calls 50]

Each timed window is `calls` back-to-back launches of one of the two between a pair of device events (a single launch of
a few microseconds would measure the event pair); the two alternate window by window, after a warm-up of both, and the
figure is the median window over `repeats`, divided by `calls`.  bytes_* are what each call must move per the shapes
(ts, density and a read-modify-write of g_density, against ts, density, rgb and writes of g_density and g_rgb); the rows
are re-read from cache by the later sweeps, which is not counted.  These are measurements, not gates.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learn-nerf_amd"))

from learn_nerf import ops  # noqa: E402


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # microseconds per call


def measure(n, t, repeats, calls):
    gen = torch.Generator().manual_seed(t)
    t_min = (2.0 + torch.rand(n, generator=gen)).cuda()
    t_max = t_min + 1.0 + torch.rand(n, generator=gen).cuda()
    u = torch.rand(n, t, generator=gen).cuda()
    ts = ops.stratified(t_min, t_max, t, u=u)
    mask = torch.ones(n, dtype=torch.uint8, device="cuda")
    dens = (torch.rand(n, t, generator=gen) * 4).cuda()
    rgb = (torch.rand(n, t, 3, generator=gen) * 2 - 1).cuda()
    bg = torch.tensor([-0.5, 0.1, 0.7], device="cuda")
    g_out = (torch.rand(n, 3, generator=gen) - 0.5).cuda()
    g_bg = torch.zeros(3, device="cuda")
    gd = torch.zeros(n, t, device="cuda")

    def distortion():
        ops.distortion(ts, t_min, t_max, mask, dens, g_density=gd, grad_scale=0.01 / n)

    def distortion_loss_only():
        ops.distortion(ts, t_min, t_max, mask, dens)

    def composite_bwd():
        ops.composite_bwd(ts, t_min, t_max, mask, dens, rgb, bg, g_bg, g_out=g_out)

    fns = dict(distortion=distortion, distortion_loss_only=distortion_loss_only, composite_bwd=composite_bwd)
    for fn in fns.values():  # warm-up: code objects, allocator, workspace lease
        window(fn, calls)
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(window(fn, calls))
    out = dict(rays=n, samples=t, repeats=repeats, calls_per_window=calls)
    for k, v in times.items():
        v = sorted(v)
        out[f"{k}_us"] = round(v[len(v) // 2], 2)
        out[f"{k}_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
    out["bytes_distortion"] = 4 * (n * t * 4 + 3 * n)
    out["bytes_composite_bwd"] = 4 * (n * t * (2 + 3 + 1 + 3) + 6 * n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 192])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distortion_probe needs a GPU")
    torch.cuda.set_device(0)
    for t in args.samples:
        print(json.dumps(measure(args.rays, t, args.repeats, args.calls)), flush=True)


if __name__ == "__main__":
    main()

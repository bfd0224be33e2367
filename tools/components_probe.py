"""
Measurements of the connected-component labelling (learn_nerf/components.py), one JSON line per case:

  serpentine             the (33, 33, 33) serpentine of tests/components_reference.py: cells and merge rounds
  analytic R             the inside set {cos x + cos y + cos z > 2.7} of the analytic scene of tests/mesh_reference.py on
                         R^3 points of the box (-1.5, -1.5, -1.5) .. (6.0, 1.5, 1.5) (one whole blob and one cut by the box
                         face), evaluated with torch in float32 rather than through the model: foreground fraction,
                         components, merge rounds and the HIP-event median of label_components, of component_sizes and
                         of the whole keep_components(keep_largest=1), read-backs included
  random R P             a random mask of density P on R^3 cells (the tangled case), the same figures at connectivity 6

These are measurements, not gates.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "learn-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from learn_nerf import components  # noqa: E402


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


def measure(mask, connectivity, repeats):
    labels, rounds = components.label_components(mask, connectivity)  # warm-up: code objects, allocator
    sizes = components.component_sizes(labels)
    out = dict(shape=list(mask.shape), connectivity=connectivity, repeats=repeats,
               foreground_fraction=float(mask.float().mean()), components=int(sizes.count_nonzero()),
               largest=int(sizes.max()), rounds=rounds)
    out["label_ms"] = events(lambda: components.label_components(mask, connectivity), repeats)
    out["sizes_ms"] = events(lambda: components.component_sizes(labels), repeats)
    out["keep_largest_1_ms"] = events(lambda: components.keep_components(mask, keep_largest=1,
                                                                         connectivity=connectivity), repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("serpentine", "analytic", "random"))
    ap.add_argument("resolution", type=int, nargs="?", default=33)
    ap.add_argument("density", type=float, nargs="?", default=0.31)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.mode == "serpentine":
        import components_reference as C

        mask = torch.from_numpy(C.serpentine(33)).cuda()
        out = dict(mode="serpentine", cells=int(mask.sum()))
        for connectivity in (6, 26):
            out[f"rounds_{connectivity}"] = components.label_components(mask, connectivity)[1]
        out["max_rounds"] = components.L.lib().lnrf_cc_max_rounds()
    elif args.mode == "analytic":
        r = args.resolution
        axes = [torch.from_numpy(np.linspace(lo, hi, r).astype(np.float32)).cuda()
                for lo, hi in zip((-1.5, -1.5, -1.5), (6.0, 1.5, 1.5))]
        field = torch.cos(axes[0])[:, None, None] + torch.cos(axes[1])[None, :, None] + torch.cos(axes[2])[None, None, :]
        mask = (field > 2.7).to(torch.uint8)
        del field
        out = dict(mode="analytic", **measure(mask, 26, args.repeats))
    else:
        r = args.resolution
        gen = torch.Generator(device="cuda").manual_seed(0)
        mask = (torch.rand((r, r, r), device="cuda", generator=gen) < args.density).to(torch.uint8)
        out = dict(mode="random", density=args.density, **measure(mask, 6, args.repeats))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

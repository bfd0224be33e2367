"""
Helper of tests/test_gpu_nerf_backward_edges.py: the FIRST layer-stationary and the first two-launch NeRF backward of a
fresh process, at the case the parent builds (first_call_case: m = 70000, the model and inputs of nerf_grad_helpers),
written as .npy files for the parent to compare bit for bit.  argv: out_dir
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "learn-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out_dir = sys.argv[1]
    import numpy as np
    import torch

    from test_gpu_nerf_backward_edges import first_call_case, run_single

    torch.cuda.set_device(0)
    model, flat, inp = first_call_case()
    for kind in ("ls", "split"):  # the process's first call of each kind
        dens, rgb, grad, status = run_single(model, flat, inp, kind)
        for name, t in (("density", dens), ("rgb", rgb), ("gradient", grad)):
            np.save(os.path.join(out_dir, f"{kind}_{name}.npy"), t.cpu().numpy())
        if kind == "ls":
            np.save(os.path.join(out_dir, "ls_status.npy"), np.array(status, dtype=np.int64))
    print(f"first calls written: ls status {status}")


if __name__ == "__main__":
    main()

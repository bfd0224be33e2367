"""
Helpers shared by the NeRFModel gradient tests (test_gpu_nerf_mlp.py, test_gpu_nerf_backward_edges.py): random points,
a model with perturbed biases, the float64 autograd oracle of the gradient and the per-Dense-layer relative error.
A plain module, not a test file: importing it collects nothing.
"""
import torch

from oracle import model as OM


def make_points(m, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(m, 3, generator=gen) * 2 - 1).float()
    d = torch.randn(m, 3, generator=gen)
    d = (d / d.norm(dim=-1, keepdim=True)).float()
    return x, d, gen


def make_model(precision, seed=1, bias_scale=0.1, render_precision="bf16x3"):
    from learn_nerf.model import NeRFModel

    model = NeRFModel(precision=precision, render_precision=render_precision)
    params = model.init(dict(params=seed))["params"]
    flat = model.flat(params)
    # Flax initialises biases to zero; perturb them so that bias handling is exercised
    gen = torch.Generator().manual_seed(seed + 100)
    noise = torch.zeros(flat.numel())
    off = 0
    for fi, fo in model.layer_dims():
        off += fi * fo
        noise[off:off + fo] = torch.randn(fo, generator=gen) * bias_scale
        off += fo
    flat.add_(noise.cuda())
    return model, params, flat


def oracle_grads(flat64, x, d, g_dens, g_rgb, operand_round=None):
    p = flat64.clone().requires_grad_(True)
    dens, rgb, _ = OM.nerf_mlp(p, x.double(), d.double(), operand_round=operand_round)
    loss = (dens[:, 0] * g_dens.double()).sum() + (rgb * g_rgb.double()).sum()
    (g,) = torch.autograd.grad(loss, p)
    return g


def per_layer_rel_err(model, got, ref):
    out, off = [], 0
    for i, (fi, fo) in enumerate(model.layer_dims()):
        for name, n in (("kernel", fi * fo), ("bias", fo)):
            a, b = got[off:off + n], ref[off:off + n]
            out.append((f"Dense_{i}.{name}", ((a - b).norm() / (b.norm() + 1e-30)).item(), b.norm().item()))
            off += n
    return out

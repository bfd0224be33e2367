"""
Shared pieces of the whole-step tests (test_gpu_train_step.py, test_gpu_train_step_paths.py): the ray batch, the Philox
uniforms and the density-penalty key that TrainLoop derives from a step key, the oracle step (oracle/train.py losses +
autograd, with the optional density penalty of train.py:153-163), optax.adam on the oracle's side, and the per-slice /
per-layer comparison of a flat gradient.  Everything here runs on the CPU; only the TrainLoop handed in lives on the GPU.
"""
import math

import torch

from oracle import instant_ngp as ON
from oracle import model as OM
from oracle import philox
from oracle import ref_nerf as ORF
from oracle import train as OT

F64 = torch.float64
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


# ---------------------------------------------------------------- inputs
def make_batch(n, seed=0, away=False):
    """[n,3,3] (origin on the radius-4 sphere, unit direction, target rgb in [-1,1]).  Nine rays in ten aim at the box;
    the first n // 10 get a random direction (most of them miss) or, with away=True, point away from it (all miss)."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=gen)
    o = 4 * o / o.norm(dim=-1, keepdim=True)
    d = -o + (torch.rand(n, 3, generator=gen) - 0.5) * 0.6
    d[: n // 10] = torch.randn(n // 10, 3, generator=gen)
    if away:
        d[: n // 10] = o[: n // 10] + 0.3 * d[: n // 10]
    d = d / d.norm(dim=-1, keepdim=True)
    c = torch.rand(n, 3, generator=gen) * 2 - 1
    return torch.stack([o, d, c], 1).float().contiguous()


def boost_density(loop):
    """Random-init NeRF predicts softplus(~0): scale the density head so alpha spans (0,1)."""
    for name in ("coarse", "fine"):
        p = loop.state.params[name]
        p["Dense_9"]["kernel"].mul_(6.0)
        p["Dense_9"]["bias"].add_(1.5)


def add_bias_noise_(loop, seed=4, scale=0.1):
    """Flax initialises biases to zero, which hides a misplaced or dropped bias: give every bias leaf of both models
    N(0, scale^2) values."""
    gen = torch.Generator().manual_seed(seed)
    for model, sl in zip((loop.coarse, loop.fine), loop._slices(loop.flat)[:2]):
        for _, leaf, lo, hi in leaf_ranges(model):
            if leaf == "bias":
                sl[lo:hi] += (torch.randn(hi - lo, generator=gen) * scale).to(sl.device)
    loop._params_changed()


def step_keys(key_seed):
    """(coarse sampling key, fine sampling key, density-penalty key) of a step key, as TrainLoop splits it
    (train.py:137, render.py:55)."""
    from learn_nerf.rng import Key, split

    render_key, density_key = split(Key(key_seed), 2)
    ck, fk = split(render_key, 2)
    return ck, fk, density_key


def uniforms_for(key_seed, n, tc, tf):
    """The stratified / fine-sampling uniforms the kernels draw for this step key (oracle/philox.py)."""
    ck, fk, _ = step_keys(key_seed)
    uc = torch.from_numpy(philox.ray_uniforms(ck.seed, 0, 0, n, tc))
    uf = torch.from_numpy(philox.ray_uniforms(fk.seed, 1, 0, n, tf))
    return uc, uf


def split_flat(loop, flat=None):
    c, f, bg = loop._slices(loop.flat if flat is None else flat)
    return c.cpu().double(), f.cpu().double(), bg.cpu().double()


# ---------------------------------------------------------------- oracle
def model_fn_factory(model, operand_round=None):
    """make_fn(flat) -> fn(x, d) -> (density, rgb, aux): the oracle restatement of `model` over a flat parameter vector."""
    from learn_nerf.instant_ngp import InstantNGPModel
    from learn_nerf.model import NeRFModel
    from learn_nerf.ref_nerf import RefNERFModel

    if type(model) is NeRFModel:
        kw = dict(input_layers=model.input_layers, mid_layers=model.mid_layers, hidden_dim=model.hidden_dim,
                  color_layer_dim=model.color_layer_dim, x_freqs=model.x_freqs, d_freqs=model.d_freqs)
        return lambda fl: OM.make_nerf_fn(fl, operand_round, **kw)
    if type(model) is RefNERFModel:
        kw = dict(sh_degree=model.sh_degree, input_layers=model.input_layers, mid_layers=model.mid_layers,
                  hidden_dim=model.hidden_dim, color_layer_dim=model.color_layer_dim, x_freqs=model.x_freqs)
        return lambda fl: (lambda x, d: ORF.ref_nerf_model(fl, x, d, operand_round=operand_round, **kw))
    if type(model) is InstantNGPModel:
        return lambda fl: (lambda x, d: ON.ngp_model(fl, x, d, model.table_sizes, model.grid_sizes, model.bbox_min,
                                                     model.bbox_max, operand_round=operand_round))
    raise TypeError(type(model))


def oracle_step(make_c, make_f, params, batch, tc, tf, uc, uf, dtype=F64, bmin=BMIN, bmax=BMAX, loss_weights=None,
                penalty=None, want_grad=True):
    """
    TrainLoop.losses + jax.grad (train.py:85-165) for parameters (coarse_flat, fine_flat, background) in `dtype`.
    penalty = (lambda, coords[B,3], dirs[B,3]) adds lambda * mean(density) of the fine, then of the coarse model at those
    points (train.py:153-163) through OT.losses' extra_penalty hook and logs fine_density / coarse_density.
    Returns dict(total, log, grads, penalty_grads, hit, mean_density): grads of the total as three tensors; penalty_grads
    the part of the two model slices' gradient that comes from the penalty term alone (None without a penalty); hit the
    number of rays that meet the box and mean_density the mean fine-pass density (is the scene degenerate?).
    """
    p = [t.detach().to(dtype).clone().requires_grad_(want_grad) for t in params]
    fns = dict(coarse=make_c(p[0]), fine=make_f(p[1]))
    pen_terms = {}

    def extra_penalty(total, loss_dict):
        lam, coords, dirs = penalty
        for name in ("fine", "coarse"):  # train.py:153-163: the same density_key, hence the same points, for both
            dens = fns[name](coords.to(dtype), dirs.to(dtype))[0].mean()
            loss_dict[f"{name}_density"] = dens
            pen_terms[name] = lam * dens
            total = total + pen_terms[name]
        return total, loss_dict

    total, loss_dict, out = OT.losses(fns["coarse"], fns["fine"], p[2], torch.tensor(bmin, dtype=dtype),
                                      torch.tensor(bmax, dtype=dtype), batch.to(dtype), tc, tf, uc.to(dtype),
                                      uf.to(dtype), loss_weights=loss_weights,
                                      extra_penalty=extra_penalty if penalty is not None else None)
    res = dict(total=total.detach(), log={k: v.detach() for k, v in loss_dict.items()}, grads=None, penalty_grads=None,
               hit=int(out["coarse_ts"].mask.sum()),
               mean_density=float(out["fine"]["densities"].detach().mean()))
    if want_grad:
        if penalty is not None:
            res["penalty_grads"] = (torch.autograd.grad(pen_terms["coarse"], p[0], retain_graph=True)[0].detach(),
                                    torch.autograd.grad(pen_terms["fine"], p[1], retain_graph=True)[0].detach())
        grads = tuple(g.detach() for g in torch.autograd.grad(total, p))
        res["grads"] = grads
        res["log"]["grad_norm"] = OT.tree_norm(*grads)
        res["log"]["param_norm"] = OT.tree_norm(*[t.detach() for t in p])
    return res


def oracle_adam(params, grads, opt, step, lr, b1=0.9, b2=0.999, eps=1e-7):
    """optax.adam (train.py:59) over the three leaves in float64.  opt = dict(m=[3 tensors], v=[...]) or None."""
    params = [t.double() for t in params]
    if opt is None:
        opt = dict(m=[torch.zeros_like(t) for t in params], v=[torch.zeros_like(t) for t in params])
    new_p, new_m, new_v = [], [], []
    for t, g, m, v in zip(params, grads, opt["m"], opt["v"]):
        p2, m2, v2 = OT.adam_update(t, g.double(), m, v, step, lr, b1, b2, eps)
        new_p.append(p2)
        new_m.append(m2)
        new_v.append(v2)
    return new_p, dict(m=new_m, v=new_v)


# ---------------------------------------------------------------- comparison
def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def leaf_ranges(model):
    """(module, leaf, start, stop) of every parameter leaf of `model` in its flat vector."""
    out, off = [], 0
    for module, leaf, shape in model.param_spec():
        n = int(math.prod(shape))
        out.append((module, leaf, off, off + n))
        off += n
    return out


def per_layer_rel(model, got, ref):
    """[(module/leaf, relative L2 error)] of one model's flat gradient, leaf by leaf."""
    return [(f"{module}/{leaf}", ((got[lo:hi].double() - ref[lo:hi].double()).norm()
                                  / (ref[lo:hi].double().norm() + 1e-30)).item())
            for module, leaf, lo, hi in leaf_ranges(model)]


def compare_gradient(loop, ref_grads, gtol, label=""):
    """loop.grad against the oracle's (coarse, fine, background) gradients: relative L2 below gtol for the coarse and for
    the fine slice separately (one bad slice cannot hide in the other's norm), the three background entries on their own
    (3 of ~10^6 entries are invisible in any whole-vector norm).  Prints the per-slice and per-leaf errors and returns
    {"coarse": rel, "fine": rel, "background": max abs}."""
    got = split_flat(loop, loop.grad)
    res = {}
    for name, model, g, r in (("coarse", loop.coarse, got[0], ref_grads[0]), ("fine", loop.fine, got[1], ref_grads[1])):
        r = r.reshape(-1).double()
        res[name] = rel_l2(g, r)
        layers = per_layer_rel(model, g, r)
        print(f"{label} {name}: grad rel L2 err {res[name]:.2e} (|ref| {r.norm().item():.3e}); per leaf: "
              + " ".join(f"{k}={v:.1e}" for k, v in layers))
    bg_ref = ref_grads[2].reshape(-1).double()
    res["background"] = (got[2] - bg_ref).abs().max().item()
    print(f"{label} background grad {got[2].tolist()} / oracle {bg_ref.tolist()}")
    for name in ("coarse", "fine"):
        assert res[name] < gtol, (label, name, res[name])
    assert torch.allclose(got[2], bg_ref, rtol=gtol, atol=1e-6), (label, got[2], bg_ref)
    return res

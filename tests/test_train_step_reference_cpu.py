"""
The whole-step test helpers (tests/train_step_reference.py) checked against oracle/train.py on a small NeRF, CPU only:
the oracle step without a penalty is OT.nerf_train_step, the penalty adds exactly lambda * grad(mean density) to each model
slice and nothing to the background, and the batch maker aims the rays it says it aims.
"""
import torch

import train_step_reference as R
from oracle import model as OM
from oracle import train as OT

F64 = torch.float64
KW = dict(input_layers=2, mid_layers=2, hidden_dim=16, color_layer_dim=8, x_freqs=3, d_freqs=2)
N, TC, TF = 20, 5, 7


def _setup():
    dims = OM.nerf_layer_dims(**KW)
    gen = torch.Generator().manual_seed(1)
    flats = [OM.lecun_normal_init(dims, gen, dtype=F64) for _ in range(2)]
    for fl in flats:
        fl += 0.05 * torch.randn(fl.shape, generator=gen, dtype=F64)
    bg = torch.tensor([0.2, -0.4, 0.9], dtype=F64)
    batch = R.make_batch(N, seed=2, away=True)
    uc = torch.rand(N, TC, generator=gen, dtype=F64)
    uf = torch.rand(N, TF, generator=gen, dtype=F64)
    make = lambda fl: OM.make_nerf_fn(fl, **KW)
    return make, (flats[0], flats[1], bg), batch, uc, uf, gen


def test_batch_maker():
    a = R.make_batch(40, seed=3)
    b = R.make_batch(40, seed=3, away=True)
    assert a.shape == (40, 3, 3) and a.dtype == torch.float32
    assert torch.equal(a[4:], b[4:]) and torch.equal(a[:, 0], b[:, 0]) and not torch.equal(a[:4, 1], b[:4, 1])
    assert torch.allclose(a[:, 1].norm(dim=-1), torch.ones(40), atol=1e-6)
    assert bool(((b[:4, 0] * b[:4, 1]).sum(-1) > 0).all())  # pointing away from the origin, hence from the box
    assert bool(((b[4:, 0] * b[4:, 1]).sum(-1) < 0).all())


def test_oracle_step_without_penalty_is_nerf_train_step():
    make, params, batch, uc, uf, _ = _setup()
    res = R.oracle_step(make, make, params, batch, TC, TF, uc, uf)
    assert res["hit"] == N - N // 10 and res["penalty_grads"] is None
    new_p, opt, log, grads = OT.nerf_train_step(make, *params, None, 1, 1e-3, torch.tensor(R.BMIN, dtype=F64),
                                                torch.tensor(R.BMAX, dtype=F64), batch.double(), TC, TF, uc, uf)
    for a, b in zip(res["grads"], grads):
        assert torch.equal(a, b)
    assert set(res["log"]) == set(log) and all(torch.equal(res["log"][k], log[k]) for k in log)
    mine_p, mine_opt = R.oracle_adam(params, res["grads"], None, 1, 1e-3)
    for a, b in zip(mine_p + mine_opt["m"] + mine_opt["v"], list(new_p) + opt["m"] + opt["v"]):
        assert torch.equal(a, b)


def test_oracle_penalty_adds_lambda_times_the_density_gradient_to_both_models():
    make, params, batch, uc, uf, gen = _setup()
    coords = torch.rand(13, 3, generator=gen) * 2 - 1
    dirs = torch.randn(13, 3, generator=gen)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    lam = 0.7
    plain = R.oracle_step(make, make, params, batch, TC, TF, uc, uf)
    pen = R.oracle_step(make, make, params, batch, TC, TF, uc, uf, penalty=(lam, coords, dirs))
    assert set(pen["log"]) - set(plain["log"]) == {"coarse_density", "fine_density"}
    for i, name in enumerate(("coarse", "fine")):
        fl = params[i].clone().requires_grad_(True)
        mean = make(fl)(coords.double(), dirs.double())[0].mean()
        (g,) = torch.autograd.grad(mean, fl)
        assert abs(float(pen["log"][f"{name}_density"]) - float(mean.detach())) < 1e-12
        assert torch.allclose(pen["penalty_grads"][i], lam * g, rtol=1e-12, atol=1e-15)
        assert torch.allclose(pen["grads"][i], plain["grads"][i] + lam * g, rtol=1e-10, atol=1e-14)
        assert g.norm() > 0
    assert torch.equal(pen["grads"][2], plain["grads"][2])
    want = plain["total"] + lam * (pen["log"]["coarse_density"] + pen["log"]["fine_density"])
    assert abs(float(pen["total"]) - float(want)) < 1e-12


def test_per_layer_and_slice_helpers():
    from learn_nerf.model import NeRFModel

    model = NeRFModel(precision="fp32", **KW)
    ranges = R.leaf_ranges(model)
    assert ranges[0][2] == 0 and ranges[-1][3] == model.num_params()
    assert all(a[3] == b[2] for a, b in zip(ranges, ranges[1:]))
    ref = torch.randn(model.num_params(), dtype=F64)
    got = ref.clone()
    lo, hi = ranges[3][2], ranges[3][3]
    got[lo:hi] *= 1.5
    errs = dict(R.per_layer_rel(model, got, ref))
    bad = f"{ranges[3][0]}/{ranges[3][1]}"
    assert abs(errs[bad] - 0.5) < 1e-12 and all(v == 0 for k, v in errs.items() if k != bad)

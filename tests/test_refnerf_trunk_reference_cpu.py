"""
CPU checks of tests/refnerf_trunk_reference.py, the float64 reference and the rules test_gpu_refnerf_trunk.py applies to the
fused Ref-NeRF trunk, normal pass and their two backwards.  No GPU involved.

  composition   the stage formulas composed without rounding are torch autograd on a float64 model (oracle/ref_nerf.py's
                spatial block) with the same weights: n_raw = grad of -spatial_out[:, 0], the first-order gradient, and the
                second-order weight gradient (create_graph=True, grad of sum u . n_raw), to 1e-9 relative.  This is what pins
                WHICH (tbar, c) pair feeds which dW; the stage checks take that pairing as given.
  recurrence    a numpy float32 emulation of the doubling chain of emb_bwd_tile, seeded with float32 sin / cos, stays inside the
                derived eps of every pair at every test input
  emulator      a numpy emulation of the kernel arithmetic (bf16 RNE, fp32 accumulation, the float32 recurrence) passes every
                rule at every size of the GPU test
  mutations     each way the kernels could be subtly wrong is rejected by at least one rule
  cap           the float32 CPU result stays inside the cap at every rounded stage, the cap is smaller than the allowance
                region it guards, and a result that takes the other neighbour wherever the allowance permits is rejected by it
  inputs        every hidden layer has 10 % .. 90 % of its ReLU bits set, |n_raw| > 1e-3 on >= 90 % of the rows
"""
import functools

import numpy as np
import pytest
import torch

import nerf_dump_decode as D
import refnerf_trunk_reference as T


@pytest.fixture(scope="module", autouse=True)
def _host_lib():
    try:
        D.load_host_lib()
    except FileNotFoundError as e:
        pytest.skip(str(e))


def wide(g, ld=276, fill=float("nan")):
    out = torch.full((g.shape[0], ld), fill, dtype=torch.float32)
    out[:, :g.shape[1]] = g
    return out


@functools.lru_cache(maxsize=None)
def emulated(m, variant=None, mut=None):
    x = T.make_x(m)
    g, u = T.make_upstream(m, None if variant is None else T.keep_mask(variant, m))
    gw = wide(g, fill=0.5 if mut else float("nan"))
    return x, gw, u, T.emulate(x, gw, u, T.weights(), mut)


def all_cases():
    multi, full = T.multi_sizes()
    return [(m, None) for m in T.MS] + [(multi, v) for v in T.MULTI_MASKS] + [(full, "every-tile")]


def test_multi_workgroup_sizes_follow_the_production_lists():
    multi, full = T.multi_sizes()
    assert multi % 32 == 27 and full % 32 == 27 and multi < full
    for which in (T.LIST_TRUNK, T.LIST_NORMAL):
        blocks, per = T.fold_blocks(which, multi)
        assert min(blocks) >= 2 and min(per) >= 2 and -(-multi // 32) >= 2 * max(per), (blocks, per)
    blocks, _ = T.fold_blocks(T.LIST_NORMAL, full)
    assert blocks[:8] == [28] * 8 and T.fold_blocks(T.LIST_NORMAL, full - 32)[0][0] < 28, blocks
    for m in (multi, full):
        for v in T.MULTI_MASKS:
            keep = T.keep_mask(v, m)
            tiles = set((np.flatnonzero(keep) // 32).tolist())
            assert ((m - 1) // 32 in tiles) == (v != "first-tiles")
            if v == "every-tile":
                assert len(tiles) == -(-m // 32)
    print(f"[trunk-cpu] multi-workgroup m = {multi}, full width m = {full}")


def test_stage_formulas_compose_to_float64_autograd(monkeypatch):
    import oracle.ref_nerf as O

    monkeypatch.setattr(O, "ref_nerf_base", lambda spatial, directional, x, d, sh: spatial)
    m = 97
    p = T.params().double().clone().requires_grad_(True)
    block = O.ref_nerf_model(p, None, None)
    x = T.make_x(m).double().requires_grad_(True)
    g, u = T.make_upstream(m)
    g, u = g.double(), u.double()
    out = block(x)
    (n_raw,) = torch.autograd.grad(-out[:, 0].sum(), x, create_graph=True)
    (first,) = torch.autograd.grad((out * g).sum(), p, retain_graph=True)
    (second,) = torch.autograd.grad((n_raw * u).sum(), p)
    offs = D.dense_offsets()[:9]
    pn = p.detach().numpy()
    w_list = [pn[wo:bo].reshape(fi, fo) for wo, bo, fi, fo in offs]
    b_list = [pn[bo:bo + fo] for wo, bo, fi, fo in offs]
    spatial, nr, d1, d2 = T.compose_float64(x.detach().numpy(), w_list, b_list, g.numpy(), u.numpy())

    def rel(a, b):
        return np.linalg.norm(a - b) / np.linalg.norm(b)

    assert rel(spatial, out.detach().numpy()) < 1e-12
    assert rel(nr, n_raw.detach().numpy()) < 1e-9
    first, second = first.numpy(), second.numpy()
    for l, (wo, bo, fi, fo) in enumerate(offs):
        assert rel(d1[l][0].reshape(-1), first[wo:bo]) < 1e-9 and rel(d1[l][1], first[bo:bo + fo]) < 1e-9, f"first order, Dense_{l}"
        assert rel(d2[l].reshape(-1), second[wo:bo]) < 1e-9, f"second order, Dense_{l}"
        assert not second[bo:bo + fo].any(), f"second order: the bias of Dense_{l} has a gradient"
    end = offs[8][1] + T.HID
    assert not first[end:].any() and not second[end:].any()


def test_doublings_follow_the_lane_layout():
    d = T.doublings()
    assert d[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
    assert d[1].tolist() == [0, 1, 2, 3, 4, 5, 0, 1, 2, 3]
    assert d[2].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 5]
    eps = T.eps_chain()
    assert eps[0] == np.sqrt(2.0) * 2e-7 and (np.diff(eps) > eps[:-1]).all() and eps[7] < 2.0 ** 7 * 5e-7


@pytest.mark.parametrize("m,variant", all_cases(), ids=lambda v: str(v))
def test_float32_recurrence_stays_inside_eps(m, variant):
    x = T.make_x(m)
    s, co = T.emulate_recurrence(x)
    ang, _ = T.angles(x)
    err = np.hypot(s.astype(np.float64) - np.sin(ang), co.astype(np.float64) - np.cos(ang))
    ratio = (err / T.eps_pairs()[None]).max(0)
    print(f"[trunk-cpu] m={m}: float32 recurrence, largest error over eps per doubling count " +
          " ".join(f"{k}:{ratio[T.doublings() == k].max():.3f}" for k in range(8)))
    assert ratio.max() < 1.0


@pytest.mark.parametrize("m,variant", all_cases(), ids=lambda v: str(v))
def test_emulation_passes_every_rule(m, variant):
    x, g, u, r = emulated(m, variant)
    what = f"(numpy emulation, m={m}, {variant})"
    stats = T.check_all(r, x, g, u, T.weights(), what)
    twice = dict(r, grads=2.0 * r["grads"], grads2=2.0 * r["grads2"])
    T.check_trunk_bwd(twice, g, T.weights(), what, scale=2.0, skip_chain=True)
    T.check_normal_bwd(dict(twice, grads=twice["grads2"]), x, u, T.weights(), what, scale=2.0, skip_chain=True)
    ratios = {k: v for k, v in stats.items() if isinstance(v, float)}
    need = {k: v["need"] for k, v in stats.items() if isinstance(v, dict)}
    by_f = T.n_raw_by_frequency(r["n_raw"], x, r["c"][0], r["c"][5], T.weights())
    print(f"[trunk-cpu] m={m} {variant}: largest error-to-bound ratio {max(ratios.values()):.3f} "
          f"({max(ratios, key=ratios.get)}), n_raw {ratios['n_raw']:.3f}, largest needed part of delta {max(need.values()):.3f} "
          f"({max(need, key=need.get)}); n_raw error over the bound's share of frequency f: " + " ".join(f"{v:.2f}" for v in by_f))
    assert max(ratios.values()) < 1.0 and max(need.values()) < 1.0
    # (d) the float32 CPU result is inside the cap (asserted by the rules above) and the cap is not vacuous: wherever the
    # allowance region of a Dense stage holds more than the 8 free elements, the cap admits fewer elements than it holds
    if m >= 1000:
        for k, v in stats.items():
            n = m * T.HID
            if isinstance(v, dict) and not k.endswith(("x_emb", "ubar_e")) and v["allow"] * n > 8:
                assert 10 * v["cpu"] * n + 8 < v["allow"] * n, f"{k}: cap {10 * v['cpu'] * n + 8:.0f} elements, allowance {v['allow'] * n:.0f}"


MUT_MS = [33, 1000]
CAUGHT_BY = {"mask l+1": "c6", "mask l-1": "c", "x_emb rows of Dense_5 dropped": "n_raw", "seed +e_0": "c_8",
             "no coordinate advance": "n_raw", "2^f dropped": "n_raw", "sin / cos swapped": "n_raw",
             "tangent chain from the bias": "tbar0", "dW_l from c_{l-1}": "dW", "truncation": "x_emb",
             "dy8 from columns 4..259": "dy8"}


@pytest.mark.parametrize("m", MUT_MS)
@pytest.mark.parametrize("mut", T.MUTATIONS)
def test_rejects_a_mutated_kernel(mut, m):
    x, g, u, r = emulated(m, None, mut)
    with pytest.raises(AssertionError, match=CAUGHT_BY[mut]):
        T.check_all(r, x, g, u, T.weights(), f"mutation: {mut}")


def test_the_cap_rejects_the_other_neighbour_inside_the_allowance():
    m = 2053
    x, g, u, r = emulated(m)
    w = T.weights()
    ins = T.fwd_inputs(r["x_emb"], r["h"])
    ref = ins[3] @ w.w[3] + w.b[3]
    delta = D.dot_delta(256, np.abs(ins[3]) @ np.abs(w.w[3]) + np.abs(w.b[3]))
    f = lambda v: np.maximum(v, 0.0)
    lo, hi, mid = D.bf16_rne(f(ref - delta)), D.bf16_rne(f(ref + delta)), D.bf16_rne(f(ref))
    other = np.where(mid == lo, hi, lo)
    assert (other != mid).sum() > 100
    D.check_rounded(other, ref, delta, relu=True, what="inside the allowance")  # the allowance alone lets it through
    bad = dict(r, h=[v if l != 3 else other for l, v in enumerate(r["h"])], mask=[v if l != 3 else other > 0 for l, v in enumerate(r["mask"])])
    with pytest.raises(AssertionError, match="cap"):
        T.check_forward(bad, x, w, "the other neighbour wherever the allowance permits")


@pytest.mark.parametrize("m", [1000, 2053])
def test_input_conditions(m):
    x, g, u, r = emulated(m)
    for l in range(8):
        share = r["mask"][l].mean()
        assert 0.1 <= share <= 0.9, f"h{l}: {share:.3f} of the ReLU bits set"
    big = (np.abs(r["n_raw"]) > 1e-3).all(1).mean()
    assert big >= 0.9, f"|n_raw| > 1e-3 on {big:.3f} of the rows"
    assert all(np.abs(v).max() > 0 for v in r["c"] + r["dy"] + r["tbar"])
    print(f"[trunk-cpu] m={m}: ReLU shares " + " ".join(f"{r['mask'][l].mean():.2f}" for l in range(8)) + f", |n_raw| > 1e-3 on {big:.3f}")

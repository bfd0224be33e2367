"""
CPU checks of tests/refnerf_dir_reference.py, the float64 reference and the rules test_gpu_refnerf_dir.py applies to the fused
Ref-NeRF directional block.  No GPU involved.

  composition   the float64 stages composed are the oracle's directional block (oracle/ref_nerf.py) on the same rounded
                operands
  the bounds    the torch.float32 CPU emulation of every stage passes every rule on exactly the inputs and sizes of the GPU
                test (a correct implementation stays inside each bound and cap); the largest error-to-bound ratios are printed
  mutations     each way the kernels could be subtly wrong is rejected by the rule that guards that stage
"""
import functools

import numpy as np
import pytest
import torch

import nerf_dump_decode as D
import refnerf_dir_reference as R


@pytest.fixture(scope="module", autouse=True)
def _host_lib():
    try:
        D.load_host_lib()
    except FileNotFoundError as e:
        pytest.skip(str(e))


@functools.lru_cache(maxsize=None)
def weights():
    return R.Weights(R.make_params())


@functools.lru_cache(maxsize=None)
def emulated(m, variant=None):
    x, large = R.make_dir_in(m)
    g = R.make_g_dir_out(m, None if variant is None else R.multi_mask(variant, m))
    return x, g, R.emulate(x, g, weights()), large


def test_stages_compose_to_the_oracle(monkeypatch):
    import oracle.ref_nerf as O

    monkeypatch.setattr(O, "ref_nerf_base", lambda spatial, directional, x, d, sh: directional)
    flat = R.make_params()
    block = O.ref_nerf_model(flat.double(), None, None, operand_round=lambda t: torch.from_numpy(D.bf16_rne(t.numpy())))
    x, _ = R.make_dir_in(257)
    want = block(x.double()).numpy()
    w = weights()
    xin = R.stage_xin(x)[0]
    h9 = D.bf16_rne(np.maximum(R.stage_h9(xin, w)[0], 0.0))
    got, s, _ = R.stage_dir_out(h9, w)
    assert want.shape == got.shape == (257, 3) and np.abs(got - want).max() <= 1e-13 * s.max()
    # and the float64 gradients of the composition are the stages of the backward (autograd on the same rounded operands)
    g = R.make_g_dir_out(257)
    dy10 = R.stage_dy10(g)[0]
    w9, w10 = (torch.from_numpy(a).requires_grad_(True) for a in (w.w9, w.w10))
    b9, b10 = (torch.from_numpy(a).requires_grad_(True) for a in (w.b9, w.b10))
    xt = torch.from_numpy(xin).requires_grad_(True)
    pre = xt @ w9 + b9
    h = torch.relu(pre)
    assert ((h > 0).numpy() == (h9 > 0)).all()  # rounding to bf16 moves no positive value to zero
    out = torch.from_numpy(h9) @ w10 + b10  # Dense_10 sees the ROUNDED h9
    out.backward(torch.from_numpy(dy10))
    dy9_exact = R.stage_dy9(dy10, h9 > 0, w)[0]
    dy9 = D.bf16_rne(dy9_exact)
    ref = R.stage_wgrads(xin, h9, dy9, dy10)
    assert np.abs(ref["dW10"][0] - w10.grad.numpy()).max() < 1e-12 and np.abs(ref["db10"][0] - b10.grad.numpy()).max() < 1e-12
    # Dense_9's gradients take the rounded dy9: feed it through pre
    (gx, gw, gb) = torch.autograd.grad(pre, (xt, w9, b9), torch.from_numpy(dy9))
    assert np.abs(ref["dW9"][0] - gw.numpy()).max() < 1e-11 and np.abs(ref["db9"][0] - gb.numpy()).max() < 1e-11
    assert np.abs(R.stage_g_dir_in(dy9, w)[0] - gx.numpy()).max() < 1e-11


CASES = [(m, None) for m in R.MS] + [(R.MULTI_M, v) for v in R.MULTI_MASKS] + [(R.FULL_WIDTH_M, "every-tile")]


@pytest.mark.parametrize("m,variant", CASES, ids=lambda v: str(v))
def test_emulation_stays_inside_every_bound(m, variant):
    x, g, r, _ = emulated(m, variant)
    w = weights()
    what = f"(CPU fp32 emulation, m={m}, {variant})"
    n_active = R.n_active_of(g)
    assert n_active <= R.MAX_ACTIVE
    fw = R.check_forward(r, x, w, what)
    bw = R.check_backward(r, g, w, n_active, what)
    for ld in R.LDS_ALL:
        got = R.check_g_dir_in_buffer(R.g_dir_in_buffer(r["g_dir_in"], ld, m + 3), m, ld, what)
        assert (got == r["g_dir_in"]).all()
    twice = dict(r, **{k: 2.0 * r[k] for k in R.grad_ranges()})  # a second accumulating call (doubling is exact)
    R.check_backward(twice, g, w, n_active, what, scale=2.0, skip_chain=True)
    ratios = {k: v for k, v in {**fw, **bw}.items() if isinstance(v, float)}
    print(f"[dir-cpu] m={m} {variant}: {n_active} active; error-to-bound ratios " +
          " ".join(f"{k} {v:.3f}" for k, v in ratios.items()) +
          f"; h9 needed {fw['h9']['need']:.3f} dy9 needed {bw['dy9']['need']:.3f}")
    assert max(ratios.values()) < 1.0 and fw["h9"]["need"] < 1.0 and bw["dy9"]["need"] < 1.0
    blocks, per = R.fold_rows(m)
    if m == R.FULL_WIDTH_M:  # the cap of one workgroup per 6 tiles no longer binds
        assert blocks == R.fold_rows(4 * m)[0] and blocks[0] > R.fold_rows(R.MULTI_M)[0][0]
    if m >= R.MULTI_M:  # several workgroups per problem, several tiles per workgroup, a ragged last tile
        assert min(blocks) > 1 and min(per) >= 2 and m % 32 != 0
        tiles = np.unique(np.flatnonzero((g != 0).any(1).numpy()) // 32)
        assert ((m - 1) // 32 in tiles) == (variant != "first-tiles")


@pytest.mark.parametrize("m", R.SPLIT_MS)
def test_split_emulation_stays_inside_the_derived_bound(m):
    x, large = R.make_dir_in(m)
    w = weights()
    ratio, worst = R.check_split(R.emulate_split(x, w), x, w, large, f"(CPU fp32 emulation of the split arithmetic, m={m})")
    print(f"[dir-cpu] split m={m}: largest error-to-bound ratio {ratio:.4f}, largest error on the realistic rows {worst:.2e}")
    assert ratio < 1.0
    # plain bf16 operands (no lo halves) are far outside it
    plain = R.emulate(x, R.make_g_dir_out(m), w)["dir_out"]
    with pytest.raises(AssertionError):
        R.check_split(plain, x, w, large, "plain bf16 operands")


# ---- mutations ------------------------------------------------------------------------------------------------------------
def neighbour(v, step=1):
    return float(D._bf16_of_key(D._bf16_key(np.array([v])) + step)[0])


def clear_of_boundaries(ref, delta, relu):
    f = (lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v)
    return D.bf16_rne(f(ref - delta)) == D.bf16_rne(f(ref + delta))


MUT_MS = [33, 2053, R.MULTI_M]


def case(m):
    x, g, r, _ = emulated(m, "every-tile" if m == R.MULTI_M else None)
    return x, g, {k: np.array(v, copy=True) for k, v in r.items()}, weights(), R.n_active_of(g)


@pytest.mark.parametrize("m", MUT_MS)
def test_rejects_a_wrong_bf16_neighbour(m):
    x, g, r, w, n = case(m)
    ref, s, _ = R.stage_h9(r["xin"], w)
    ev, ft = (int(v) for v in np.argwhere(clear_of_boundaries(ref, D.dot_delta(R.K9, s), True) & (r["h9"] > 0))[11])
    r["h9"][ev, ft] = neighbour(r["h9"][ev, ft])
    with pytest.raises(AssertionError, match=f"(?s)h9 .*evaluation {ev} feature {ft}"):
        R.check_forward(r, x, w, "one h9 element one bf16 step off")
    x, g, r, w, n = case(m)
    r["xin"][m // 2, 100] = neighbour(r["xin"][m // 2, 100], -1)
    with pytest.raises(AssertionError, match="xin"):
        R.check_forward(r, x, w, "one xin element one bf16 step off")
    x, g, r, w, n = case(m)
    ref, s, _ = R.stage_dy9(r["dy10"], r["mask9"], w)
    ev, ft = (int(v) for v in np.argwhere(clear_of_boundaries(ref, D.dot_delta(R.K10T, s), False) & (r["dy9"] != 0))[5])
    r["dy9"][ev, ft] = neighbour(r["dy9"][ev, ft])
    with pytest.raises(AssertionError, match=f"(?s)dy9 .*evaluation {ev} feature {ft}"):
        R.check_backward(r, g, w, n, "one dy9 element one bf16 step off")
    # truncation instead of round-to-nearest-even in the register conversion: the tie rows alone give it away
    x, g, r, w, n = case(m)
    r["xin"] = D.bf16_trunc(x[:, :R.DIR_IN].double().numpy())
    with pytest.raises(AssertionError, match="xin"):
        R.check_forward(r, x, w, "truncated xin")


@pytest.mark.parametrize("m", MUT_MS)
def test_rejects_swapped_tail_features(m):
    x, g, r, w, n = case(m)
    r["xin"][:, [256, 272]] = r["xin"][:, [272, 256]]
    with pytest.raises(AssertionError, match="xin"):
        R.check_forward(r, x, w, "features 256 and 272 swapped")
    # a kernel that swaps them consistently in its dump AND its weights rows is caught one stage on
    x, g, r, w, n = case(m)
    sw = x.clone()
    sw[:, [256, 272]] = sw[:, [272, 256]]
    r2 = R.emulate(sw, g, w)
    r["h9"] = r2["h9"]
    with pytest.raises(AssertionError, match="h9"):
        R.check_forward(r, x, w, "Dense_9 contracted features 256 and 272 swapped")


@pytest.mark.parametrize("m", MUT_MS)
def test_rejects_a_dropped_scalar_tail(m):
    """input row 272 of W9 dropped = the scalar tail load of feature 272 missing from the contraction"""
    x, g, r, w, n = case(m)
    flat = R.make_params()
    w9 = R.offsets()[0]
    flat[w9 + 272 * R.HID:w9 + 273 * R.HID] = 0.0
    r["h9"] = R.emulate(x, g, R.Weights(flat))["h9"]
    with pytest.raises(AssertionError, match="h9"):
        R.check_forward(r, x, w, "W9 row 272 dropped")


@pytest.mark.parametrize("m", MUT_MS)
def test_rejects_a_dropped_evaluation_and_a_dropped_tile(m):
    x, g, r, w, n = case(m)
    ev = int(np.flatnonzero((g != 0).all(1).numpy())[-1])
    r["dW9"] = r["dW9"] - np.outer(r["xin"][ev], r["dy9"][ev])
    with pytest.raises(AssertionError, match="dW9"):
        R.check_backward(r, g, w, n, f"evaluation {ev} dropped from dW9")
    x, g, r, w, n = case(m)
    tile = ((m - 1) // 32) // 2
    r["db10"] = r["db10"] - r["dy10"][32 * tile:32 * tile + 32].sum(0)
    assert np.abs(r["dy10"][32 * tile:32 * tile + 32]).sum() > 0
    with pytest.raises(AssertionError, match="db10"):
        R.check_backward(r, g, w, n, f"tile {tile} dropped from db10")
    # an entry whose reference is exactly zero must be exactly zero
    x, g, r, w, n = case(m)
    g0 = g.clone()
    g0[:, 1] = 0.0
    r0 = R.emulate(x, g0, w)
    r0["dW10"][5, 1] = 1e-30
    with pytest.raises(AssertionError, match="dW10"):
        R.check_backward(r0, g0, w, n, "non-zero where the reference is exactly zero")


@pytest.mark.parametrize("m", MUT_MS)
def test_rejects_a_flipped_mask_bit_and_a_written_pad_column(m):
    x, g, r, w, n = case(m)
    r["mask9"][m - 1, 77] ^= True
    with pytest.raises(AssertionError, match="mask9"):
        R.check_forward(r, x, w, "one mask bit flipped")
    x, g, r, w, n = case(m)
    for ld in R.LDS_ALL:
        buf = R.g_dir_in_buffer(r["g_dir_in"], ld, m + 2)
        R.check_g_dir_in_buffer(buf, m, ld, "clean")
        bad = buf.copy()
        bad[m // 2, 273] = np.float32(1e-20).view(np.uint32)
        with pytest.raises(AssertionError, match="columns 273"):
            R.check_g_dir_in_buffer(bad, m, ld, "non-zero in column 273")
        if ld > R.WRITTEN_COLS:
            bad = buf.copy()
            bad[0, R.WRITTEN_COLS] = 0
            with pytest.raises(AssertionError, match="beyond column 288"):
                R.check_g_dir_in_buffer(bad, m, ld, "column 288 written")
        bad = buf.copy()
        bad[m, 0] = 0
        with pytest.raises(AssertionError, match="rows from"):
            R.check_g_dir_in_buffer(bad, m, ld, "row m written")

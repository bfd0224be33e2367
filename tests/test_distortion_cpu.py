"""
tests/distortion_reference.py checked on the CPU: the two float64 references agree, known answers, the float32 emulation
of distortion_kernel stays inside the derived bound on every case, and each of a set of mutations of the emulation breaks
the bound on some case (so the bound, loose as a worst case is, still tells a wrong kernel from a right one).
"""
import math

import numpy as np
import pytest
import torch

import distortion_reference as DR
import rays_edge_cases as RC

F32, F64 = torch.float32, torch.float64
CASES = DR.all_cases()


def one_ray(ts, t_min, t_max, dens, mask=True) -> RC.QuadCase:
    ts = torch.tensor([ts], dtype=F64).to(F32)
    n, t = ts.shape
    return RC.QuadCase(ts, torch.tensor([t_min], dtype=F64).to(F32), torch.tensor([t_max], dtype=F64).to(F32),
                       torch.tensor([mask]), torch.tensor([dens], dtype=F64).to(F32), torch.zeros(n, t, 3),
                       torch.zeros(n, t, 0), torch.zeros(3), torch.zeros(n, 3), ())


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_the_two_float64_references_agree(name):
    case = dict(CASES)[name]()
    l_bf, g_bf = DR.brute_force(case)
    l_st, g_st = DR.stage_formulas(case)
    dl, dg = (l_bf - l_st).abs().max().item(), (g_bf - g_st).abs().max().item()
    print(f"{name}: O(T^2) autograd vs O(T) stages: loss {dl:.1e}, gradient {dg:.1e}; largest loss {l_bf.max().item():.4f}")
    assert torch.isfinite(l_bf).all() and torch.isfinite(g_bf).all()
    assert dl <= 1e-12 and dg <= 1e-12
    miss = ~DR.Stages(case).valid
    assert (l_bf[miss] == 0).all() and (g_bf[miss] == 0).all()
    if name.startswith("T") or name in ("clustered", "repeated", "zero_range"):
        assert case.n == DR.N_RAYS and miss[list(DR.MISS_ROWS)].all()
        assert l_bf[~miss].min().item() > 0


def test_case_table_covers_what_it_claims():
    names = [c[0] for c in CASES]
    assert names[:8] == [f"T{t}" for t in (1, 2, 63, 64, 65, 128, 129, 192)]
    assert {"opaque", "empty", "late", "clustered", "repeated", "zero_range"} <= set(names)
    c = DR.clustered_case()
    span = (c.ts[:, DR.CLUSTER_HI - 1] - c.ts[:, DR.CLUSTER_LO]) / (c.t_max - c.t_min)
    assert DR.CLUSTER_HI - DR.CLUSTER_LO == 128 and c.t == 192 and (span <= 0.01).all()
    assert (c.ts[:, 1:] >= c.ts[:, :-1]).all()
    share = DR.Stages(c).w[:, DR.CLUSTER_LO:DR.CLUSTER_HI].sum(1)[1]
    assert share.item() > 0.05, "the cluster must hold a visible share of the weight"
    rep = DR.repeated_case()
    assert (DR.Stages(rep).delta == 0).any(1).all() and (rep.ts[:, 1:] >= rep.ts[:, :-1]).all()
    z = DR.zero_range_case()
    st = DR.Stages(z)
    assert z.mask[list(DR.ZERO_RANGE_ROWS)].all() and not st.valid[list(DR.ZERO_RANGE_ROWS)].any()


def test_known_answers():
    # sigma = 0: no weight, no loss
    empty = RC.empty_case()
    assert (DR.brute_force(empty)[0] == 0).all() and (DR.stage_formulas(empty)[0] == 0).all()
    # T = 1: one bin over the whole range, m = 1/2, d = 1: L = w^2 / 3 with w = 1 - exp(-sigma r)
    case = one_ray([2.7], 2.0, 3.5, [1.3])
    w = 1 - math.exp(-float(case.dens[0, 0]) * 1.5)
    for fn in (DR.brute_force, DR.stage_formulas):
        assert abs(fn(case)[0].item() - w * w / 3) < 1e-15
    # two bins of weight 1/2 each: ts (0.25, 0.75) in [0, 1] -> m = (0.25, 0.75), d = (0.5, 0.5); sigma_0 = 2 ln 2 gives
    # w_0 = 1/2, an opaque second bin takes the rest: L = 2 (1/2)(1/2)(1/2) + (1/3)(1/4 + 1/4)(1/2) = 1/3
    case = one_ray([0.25, 0.75], 0.0, 1.0, [0.0, RC.OPAQUE_DENSITY])
    case.dens = torch.tensor([[2 * math.log(2.0), RC.OPAQUE_DENSITY]], dtype=F64)  # exact sigma_0: float64 on purpose
    for fn in (DR.brute_force, DR.stage_formulas):
        assert abs(fn(case)[0].item() - 1.0 / 3.0) < 1e-15
    # a masked ray and a ray of zero range have no loss and no gradient
    for case in (one_ray([2.7, 2.9], 2.0, 3.5, [1.3, 2.0], mask=False), one_ray([2.0, 2.0], 2.0, 2.0, [1.3, 2.0])):
        for fn in (DR.brute_force, DR.stage_formulas):
            loss, grad = fn(case)
            assert loss.item() == 0 and (grad == 0).all()


def test_opaque_sample_ends_the_ray():
    """A ray opaque at sample k: w_k = exp(-A_{k-1}), nothing behind it:
    L = L(bins before k) + 2 w_k sum_{j<k} w_j (m_k - m_j) + w_k^2 d_k / 3; for k = 0 that is d_0 / 3."""
    case = RC.opaque_case()
    s = DR.Stages(case)
    loss, grad = DR.brute_force(case)
    for row, k in enumerate(RC.OPAQUE_AT):
        w, m, d = s.w[row], s.m[row], s.d[row]
        assert w[k].item() == math.exp(-s.A_prev[row, k].item()) and (w[k + 1:] == 0).all()
        before = sum(w[i] * w[j] * abs(m[i] - m[j]) for i in range(k) for j in range(k)) + (w[:k] ** 2 * d[:k]).sum() / 3
        want = before + 2 * w[k] * (w[:k] * (m[k] - m[:k])).sum() + w[k] ** 2 * d[k] / 3
        assert abs(loss[row].item() - float(want)) < 1e-14, (row, k)
        assert (grad[row, k + 1:] == 0).all()
    assert RC.OPAQUE_AT[0] == 0 and abs(loss[0].item() - s.d[0, 0].item() / 3) < 1e-15


def _excess(case, mutate=None):
    """(largest |emulation - float64| / bound over the loss, over the gradient); inf where the bound is 0 and missed."""
    l_ref, g_ref = DR.stage_formulas(case)
    l_b, g_b = DR.error_bound(case)
    l_em, g_em = DR.emulate(case, mutate)
    assert np.isfinite(l_em).all() and np.isfinite(g_em).all()
    out = []
    for got, ref, bound in ((l_em, l_ref, l_b), (g_em, g_ref, g_b)):
        err = (torch.from_numpy(got).double() - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # 0 / 0 is inside, x / 0 is outside
        out.append((ratio.max().item(), err.max().item(), bound.max().item()))
    return out


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_emulation_stays_inside_the_bound(name):
    case = dict(CASES)[name]()
    (lr, le, lb), (gr, ge, gb) = _excess(case)
    print(f"{name}: float32 emulation vs float64: loss |d| {le:.2e} (largest bound {lb:.2e}, worst ratio {lr:.3f}); "
          f"gradient |d| {ge:.2e} (largest bound {gb:.2e}, worst ratio {gr:.3f})")
    assert lr <= 1.0 and gr <= 1.0
    l_em, g_em = DR.emulate(case)
    miss = ~DR.Stages(case).valid.numpy()
    assert (l_em[miss] == 0).all() and (g_em[miss] == 0).all()


@pytest.mark.parametrize("mutation", DR.MUTATIONS)
def test_mutations_break_the_bound(mutation):
    broken = []
    for name, make in CASES:
        (lr, _, _), (gr, _, _) = _excess(make(), mutation)
        if lr > 1.0 or gr > 1.0:
            broken.append((name, round(min(lr, 1e9), 1), round(min(gr, 1e9), 1)))
    print(f"{mutation}: outside the bound on {broken}")
    assert broken, mutation

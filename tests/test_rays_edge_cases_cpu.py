"""
The case tables of tests/rays_edge_cases.py are well posed (no GPU): the float32 and float64 oracles agree on every
degenerate ray, the quadrature references are finite, and the sizes that tests/test_gpu_rays_edges.py relies on (LDS
bytes, Philox counter words, fold trips) are what its comments claim.  This keeps the GPU tests from being vacuous.
"""
import numpy as np
import pytest
import torch

import rays_edge_cases as RC
from oracle import philox
from oracle import render as OR

F32, F64 = torch.float32, torch.float64


def test_degenerate_rays_float32_and_float64_oracles_agree():
    rays = RC.degenerate_rays()
    lo32, hi32, m32 = RC.oracle_t_range(rays, F32)
    lo64, hi64, m64 = RC.oracle_t_range(rays, F64)
    for i, (_, _, note) in enumerate(RC.DEGENERATE_RAYS):
        assert bool(m32[i]) == bool(m64[i]), (i, note)
    hit = m64
    assert torch.allclose(lo32[hit].double(), lo64[hit], rtol=1e-5, atol=1e-6)
    assert torch.allclose(hi32[hit].double(), hi64[hit], rtol=1e-5, atol=1e-6)
    # misses carry the null range in both
    assert (lo64[~hit] == 0).all() and (hi64[~hit] == RC.MIN_T_RANGE).all()
    assert (lo32[~hit] == 0).all() and (hi32[~hit] == np.float32(RC.MIN_T_RANGE)).all()
    assert torch.isfinite(lo64).all() and torch.isfinite(hi64).all()
    assert torch.isfinite(lo32).all() and torch.isfinite(hi32).all()


def test_degenerate_rays_cover_every_kind():
    rays = RC.degenerate_rays()
    lo, hi, mask = RC.oracle_t_range(rays, F64)
    assert len(RC.DEGENERATE_RAYS) >= 12
    assert mask.any() and (~mask).any()
    assert (mask & (lo == 0)).any(), "no hit that starts at t = 0"
    clamped = mask & ((hi - lo - RC.MIN_T_RANGE).abs() < 1e-12)
    assert clamped.any(), "no hit whose t_max is t_min + min_t_range"
    nan_rows = RC.nan_intermediate_rows(rays)
    assert nan_rows.any(), "no row with a 0/0 slab quotient in float32"
    assert not mask[nan_rows].any(), "the 0/0 rows are misses in the reference"
    # den == 0 without 0/0: an infinite quotient on a ray that still hits
    r = rays.to(F32)
    den = r[:, 1] + torch.tensor(RC.EPSILON, dtype=F32)
    assert ((den == 0).any(1) & mask).any()
    # the tiled table keeps whole copies in order and ends in a ragged tail of two workgroups of 256 threads
    tiled = RC.degenerate_rays(257)
    assert tiled.shape == (257, 2, 3) and torch.equal(tiled[: rays.shape[0]], rays)
    assert torch.equal(tiled[rays.shape[0]], rays[0])


@pytest.mark.parametrize("name,build", RC.all_quad_cases(), ids=[n for n, _ in RC.all_quad_cases()])
def test_quadrature_references_are_finite(name, build):
    case = build()
    ref = RC.quad_reference(case)
    for x in ref.tensors():
        assert torch.isfinite(x).all(), name
    assert case.ts.dtype == F32 and (case.ts[:, 1:] >= case.ts[:, :-1]).all()
    assert (case.ts >= case.t_min[:, None]).all() and (case.ts <= case.t_max[:, None]).all()
    assert len(case.gw) == case.n_aux and len(set(case.gw)) == case.n_aux


def test_opaque_builder_saturates_float32():
    case = RC.opaque_case()
    assert (case.n, case.t) == (8, 70)
    at = torch.tensor(RC.OPAQUE_AT)
    assert 0 in RC.OPAQUE_AT and case.t - 1 in RC.OPAQUE_AT and 63 in RC.OPAQUE_AT and 64 in RC.OPAQUE_AT
    a = (case.dens * case.samples(F32).deltas())[torch.arange(case.n), at]
    assert torch.isfinite(a).all() and (torch.exp(-a) == 0.0).all()
    probs = RC.quad_reference(case).probs
    for r, k in enumerate(RC.OPAQUE_AT):
        assert (probs[r, k + 1:] == 0).all()


def test_empty_and_late_builders():
    ref = RC.quad_reference(RC.empty_case())
    assert (ref.probs[:, :-1] == 0).all() and (ref.probs[:, -1] == 1).all()
    assert torch.equal(ref.outputs, torch.tensor(RC.BACKGROUND, dtype=F32).double().expand(8, 3))
    late = RC.late_case()
    assert (late.n, late.t) == (8, 70)
    assert (late.dens[:, :64] == 0).all() and (late.dens[:, 64:] > 0).all()


def test_missed_and_fold_builders():
    case = RC.missed_case()
    assert (case.n, case.t, case.n_aux) == (9, 65, 2)
    assert (~case.mask).nonzero().flatten().tolist() == [0, 4, 8]
    ref = RC.quad_reference(case)
    # a missed ray hands its whole upstream gradient to the background
    only_missed = case.g_out.double()[~case.mask].sum(0)
    hits = (ref.probs[:, -1:] * case.g_out.double())[case.mask].sum(0)
    assert torch.allclose(ref.g_background, only_missed + hits, rtol=1e-12, atol=1e-15)
    allm = RC.all_missed_case()
    assert not allm.mask.any()
    assert torch.allclose(RC.quad_reference(allm).g_background, allm.g_out.double().sum(0), rtol=1e-12, atol=1e-15)
    for n in RC.FOLD_NS:
        fold = RC.fold_case(n)
        assert (fold.n + 3) // 4 > 256, "the fold loop must take a second trip"
        assert fold.mask.any() and (~fold.mask).any()
        g = fold.g_out.abs()
        assert g.min() < 3e-3 and g.max() > 0.3 and (fold.g_out > 0).any() and (fold.g_out < 0).any()
        # dropping the rows of any one trip of the fold loop moves g_background by far more than the tolerance
        fref = RC.quad_reference(fold)
        shares = RC.fold_trip_shares(fold, fref)
        assert shares.shape[0] == (n + 1023) // 1024 >= 2
        assert torch.allclose(shares.sum(0), fref.g_background, rtol=1e-12, atol=1e-14)
        assert (shares.abs() > 100 * (2e-6 + 1e-4 * fref.g_background.abs())).all(), shares
    assert (RC.FOLD_NS[0] + 3) // 4 == 258 and RC.FOLD_NS[1] == 2049


def test_philox_offset_reaches_the_high_counter_word():
    n, count, off = 6, 7, 2 ** 33
    assert ((off * count) >> 2) >> 32 != 0
    assert (((off + n) * count - 1) >> 2) >> 32 != 0
    hi = philox.ray_uniforms(0x1234ABCD5678, 3, off, n, count)
    lo = philox.ray_uniforms(0x1234ABCD5678, 3, 0, n, count)
    assert hi.shape == lo.shape == (n, count)
    assert not np.array_equal(hi, lo)
    assert (hi >= 0).all() and (hi <= np.float32(RC.U_MAX)).all()
    assert np.float32(RC.U_MAX) < 1.0 and np.float32(RC.U_MAX) == np.float32((2 ** 24 - 1) * 2.0 ** -24)


def test_fine_sample_lds_sizes():
    """bytes = 16 * (3*tc + tf + 2): 4 waves per workgroup, each xs[tc+1], ys[tc+1], comb[tc+tf] floats."""
    tc = RC.FINE_LDS_TC
    assert [RC.fine_sample_lds_bytes(tc, tf) for tf in RC.FINE_LDS_TFS] == [65536, 65552, 163840]
    assert RC.fine_sample_lds_bytes(tc, RC.FINE_LDS_TF_TOO_LARGE) > 163840
    assert RC.fine_sample_lds_bytes(1, 1) == 4 * 4 * (2 * 2 + 1 + 1)


@pytest.mark.parametrize("uf", [None, 0.0, RC.U_MAX])
def test_fine_cdf_check_accepts_the_float32_oracle(uf):
    """The criterion is attainable: float32 arithmetic of the oracle's own formulas passes it on the cases the GPU test
    uses (so a failure there is the kernel's), and samples moved by 1e-3 of the span do not."""
    case = RC.fine_case(5, 64, 131, seed=3, uf=uf)
    s32 = OR.RaySamples(case.t_min, case.t_max, torch.ones(case.ts.shape[0], dtype=torch.bool), case.ts)
    new32 = s32.fine_sampling(131, case.uf, case.dens, combine=False).ts
    RC.fine_cdf_check(new32, case.samples64(), case.dens, case.uf)
    bad = new32 - 1e-3 * (case.t_max - case.t_min)[:, None]
    with pytest.raises(AssertionError):
        RC.fine_cdf_check(bad, case.samples64(), case.dens, case.uf)


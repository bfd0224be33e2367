"""
The per-ray kernels (csrc/rays.hip, csrc/ray_geom.h) at their edges, against the float64 oracle: degenerate rays of
the slab test, chunk seams and extreme counts of the quadrature, opaque / empty rays, missed rays of the backward on
poisoned outputs, the background fold past 256 partial rows, lnrf_bin_edges, lnrf_fine_sample from its smallest sizes
to its LDS limit, and Philox counters past 2^32.

Cases and references: tests/rays_edge_cases.py (checked on the CPU by tests/test_rays_edge_cases_cpu.py).  Tolerances
are those of the matching assertion in tests/test_gpu_rays.py; the float32 oracle (the same formulas in torch float32)
meets every one of them on these cases with its worst figure, probs of the `late` family, at 1.4e-6 of the 2e-6 allowed.
"""
import ctypes

import numpy as np
import pytest
import torch

import rays_edge_cases as RC
from gpu_poison import poisoned
from oracle import philox

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ERR_ARG = -1


def g(x):
    return None if x is None else x.cuda()


def cpu64(x):
    return x.cpu().double()


class Dev:
    """A QuadCase on the GPU (mask as the uint8 flags the kernels read)."""

    def __init__(self, case):
        self.case = case
        self.ts, self.t_min, self.t_max = g(case.ts), g(case.t_min), g(case.t_max)
        self.mask = g(case.mask.to(torch.uint8))
        self.dens, self.rgb, self.bg, self.tgt = g(case.dens), g(case.rgb), g(case.bg), g(case.tgt)
        self.aux = g(case.aux) if case.n_aux else None
        self.g_out = g(case.g_out)

    def fwd(self):
        from learn_nerf import ops

        return ops.composite_fwd(None, self.ts, self.t_min, self.t_max, self.mask, self.dens, self.rgb, self.bg,
                                 aux=self.aux, want_coords=False)

    def probs(self):
        from learn_nerf import ops

        return ops.termination_probs(self.ts, self.t_min, self.t_max, self.dens)

    def bwd(self, g_bg, outputs=None):
        """The wrapper's backward: explicit upstream gradient if the case has one, else the fused MSE gradient."""
        from learn_nerf import ops

        kw = dict(aux=self.aux, g_aux_w=list(self.case.gw))
        if self.case.g_out is not None:
            kw["g_out"] = self.g_out
        else:
            kw.update(outputs=outputs, targets=self.tgt, out_scale=self.case.out_scale)
        return ops.composite_bwd(self.ts, self.t_min, self.t_max, self.mask, self.dens, self.rgb, self.bg, g_bg, **kw)


def assert_forward(d: Dev, ref):
    probs = d.probs()
    outputs, alphas, _, aux_sum = d.fwd()
    for x in (probs, outputs, alphas) + ((aux_sum,) if d.case.n_aux else ()):
        assert torch.isfinite(x).all()
    assert torch.allclose(cpu64(probs), ref.probs, atol=2e-6)
    assert torch.allclose(cpu64(outputs), ref.outputs, atol=5e-6)
    assert torch.allclose(cpu64(alphas), ref.alphas, atol=5e-6)
    if d.case.n_aux:
        assert torch.allclose(cpu64(aux_sum), ref.aux_sum, atol=5e-6)
    return probs, outputs, alphas


def assert_backward(d: Dev, ref, outputs=None):
    g_bg = torch.zeros(3, device="cuda")
    gd, gc, ga = d.bwd(g_bg, outputs)
    for x in (gd, gc, g_bg) + ((ga,) if d.case.n_aux else ()):
        assert torch.isfinite(x).all()
    assert torch.allclose(cpu64(gd), ref.g_density, atol=2e-6, rtol=1e-4)
    assert torch.allclose(cpu64(gc), ref.g_rgb, atol=2e-7, rtol=1e-4)
    assert torch.allclose(cpu64(g_bg), ref.g_background, atol=2e-6, rtol=1e-4)
    if d.case.n_aux:
        assert torch.allclose(cpu64(ga), ref.g_aux, atol=2e-7, rtol=1e-4)
    return gd, gc, ga, g_bg


# ---------------------------------------------------------------------------------------------------------------------
# slab test

@pytest.mark.parametrize("rows", [None, 257])
@pytest.mark.parametrize("layout", ["rays", "batch"])
def test_slab_on_degenerate_rays(rows, layout):
    """ops.ray_aabb_stratified on DEGENERATE_RAYS (and the table tiled to 257 rows: two workgroups, ragged tail), with
    count 0 and count 3, through the [N,2,3] and the [N,3,3] training-batch stride."""
    from learn_nerf import ops

    rays = RC.degenerate_rays(rows)
    n = rays.shape[0]
    gen = torch.Generator().manual_seed(5)
    u = torch.rand(n, 3, generator=gen).to(F32)
    s = RC.oracle_samples(rays, 3, u)
    assert s.mask.any() and (~s.mask).any()
    arg = rays if layout == "rays" else torch.cat([rays, torch.rand(n, 1, 3, generator=gen)], 1).contiguous()
    null_hi = torch.tensor(RC.MIN_T_RANGE, dtype=F32)
    for count in (0, 3):
        t_min, t_max, mask, ts = ops.ray_aabb_stratified(g(arg), RC.BBOX_MIN, RC.BBOX_MAX, count,
                                                         u=g(u) if count else None, min_t_range=RC.MIN_T_RANGE,
                                                         epsilon=RC.EPSILON)
        t_min, t_max, mask, ts = t_min.cpu(), t_max.cpu(), mask.cpu(), ts.cpu()
        wrong = (mask.bool() != s.mask).nonzero().flatten().tolist()
        assert not wrong, [(i, RC.DEGENERATE_RAYS[i % len(RC.DEGENERATE_RAYS)][2]) for i in wrong]
        assert ((mask == 0) | (mask == 1)).all()
        for x in (t_min, t_max, ts):
            assert torch.isfinite(x).all()
        hit = s.mask
        assert torch.allclose(t_min[hit].double(), s.t_min[hit], rtol=1e-5, atol=1e-6)
        assert torch.allclose(t_max[hit].double(), s.t_max[hit], rtol=1e-5, atol=1e-6)
        assert (t_min[~hit] == 0).all()
        assert (t_max[~hit] == null_hi).all()
        assert ts.shape == (n, count)
        if count:
            assert torch.allclose(ts.double(), s.ts, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# bin edges

@pytest.mark.parametrize("n,t", [(1, 1), (3, 2), (5, 65), (300, 7)])
def test_bin_edges(n, t):
    from learn_nerf import _lib as L
    from learn_nerf import ops

    case = RC.quad_case(n, t, 0, seed=40 + t)
    s = case.samples(F64)
    ts, t_min, t_max = g(case.ts), g(case.t_min), g(case.t_max)
    starts, ends = ops.bin_edges(ts, t_min, t_max)
    assert torch.allclose(cpu64(starts), s.starts(), atol=1e-6, rtol=0)
    assert torch.allclose(cpu64(ends), s.ends(), atol=1e-6, rtol=0)
    assert torch.equal(starts[:, 0], t_min)
    assert torch.equal(ends[:, -1], t_max)
    assert torch.equal(ends[:, :-1], starts[:, 1:])
    # NULL starts or NULL ends through the C ABI: the other buffer is still filled, bit for bit as above
    for which in ("starts", "ends"):
        out = torch.full((n, t), 7.0, device="cuda")
        rc = L.lib().lnrf_bin_edges(L.ptr(ts), L.ptr(t_min), L.ptr(t_max), n, t,
                                    L.ptr(out) if which == "starts" else None,
                                    L.ptr(out) if which == "ends" else None, L.stream())
        assert rc == 0, L.lib().lnrf_last_error()
        assert torch.equal(out, starts if which == "starts" else ends), which


# ---------------------------------------------------------------------------------------------------------------------
# quadrature seams and counts

@pytest.mark.parametrize("t", RC.SEAM_FWD_TS)
def test_forward_at_chunk_seams(t):
    case = RC.quad_case(5, t, 2, seed=t)
    assert_forward(Dev(case), RC.quad_reference(case))


@pytest.mark.parametrize("n,t,n_aux", RC.SEAM_BWD)
def test_backward_at_chunk_seams_and_counts(n, t, n_aux):
    """composite_bwd against float64 autograd of the MSE loss (+ weighted aux sums), as
    test_composite_bwd_matches_autograd: T = 1 (one sample is the first and the last bin), T just past a 64-lane
    chunk, n_aux 3 and 4 (kMaxAux) with distinct weights."""
    case = RC.quad_case(n, t, n_aux, seed=n + t)
    d = Dev(case)
    ref = RC.quad_reference(case)
    _, outputs, _ = assert_forward(d, ref)
    gd, gc, _, _ = assert_backward(d, ref, outputs)
    # explicit upstream gradient path gives the same answer
    from learn_nerf import ops

    g_out = (case.out_scale * (outputs - d.tgt)).contiguous()
    gd2, gc2, _ = ops.composite_bwd(d.ts, d.t_min, d.t_max, d.mask, d.dens, d.rgb, d.bg, torch.zeros(3, device="cuda"),
                                    g_out=g_out, aux=d.aux, g_aux_w=list(case.gw))
    assert torch.equal(gd, gd2) and torch.equal(gc, gc2)


def abi_bwd(d: Dev, n_aux, aux, gw, gd, gc, ga, g_bg, scratch_ptr, scratch_bytes):
    """lnrf_composite_bwd_det with an explicit upstream gradient and caller-owned outputs -> return code."""
    from learn_nerf import _lib as L

    return L.lib().lnrf_composite_bwd_det(
        L.ptr(d.ts), L.ptr(d.t_min), L.ptr(d.t_max), L.ptr(d.mask, torch.uint8), L.ptr(d.dens), L.ptr(d.rgb),
        L.ptr(aux), n_aux, L.ptr(d.bg), d.case.n, d.case.t, L.ptr(d.g_out), None, None, 0, 0.0, gw, L.ptr(gd),
        L.ptr(gc), L.ptr(ga), L.ptr(g_bg), scratch_ptr, scratch_bytes, L.stream())


def last_error() -> str:
    from learn_nerf import _lib as L

    return (L.lib().lnrf_last_error() or b"").decode()


def test_five_aux_channels_are_rejected_before_any_launch():
    from learn_nerf import _lib as L

    n, t = 4, 6
    case = RC.quad_case(n, t, 4, seed=50, g_out=True)
    d = Dev(case)
    aux5 = torch.rand(n, t, 5, device="cuda")
    fill = 7.0
    outputs, alphas = torch.full((n, 3), fill, device="cuda"), torch.full((n,), fill, device="cuda")
    aux_sum = torch.full((n, 5), fill, device="cuda")
    rc = L.lib().lnrf_composite_fwd(None, 6, L.ptr(d.ts), L.ptr(d.t_min), L.ptr(d.t_max), L.ptr(d.mask, torch.uint8),
                                    L.ptr(d.dens), L.ptr(d.rgb), L.ptr(aux5), 5, L.ptr(d.bg), n, t, L.ptr(outputs),
                                    L.ptr(alphas), None, L.ptr(aux_sum), None, 0, None, L.stream())
    assert rc == ERR_ARG and "bad aux" in last_error()
    gd, gc = torch.full((n, t), fill, device="cuda"), torch.full((n, t, 3), fill, device="cuda")
    ga, g_bg = torch.full((n, t, 5), fill, device="cuda"), torch.full((3,), fill, device="cuda")
    nbytes = L.lib().lnrf_composite_bwd_scratch_bytes(n)
    scratch = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    gw = (L.c_float * 8)(0.3, 0.05, -0.2, 0.11, 0.4, 0.0, 0.0, 0.0)
    rc = abi_bwd(d, 5, aux5, gw, gd, gc, ga, g_bg, L.ptr(scratch, torch.uint8), nbytes)
    assert rc == ERR_ARG and "bad aux" in last_error()
    torch.cuda.synchronize()
    for x in (outputs, alphas, aux_sum, gd, gc, ga, g_bg):
        assert (x == fill).all()
    assert (scratch == 0x5A).all()


# ---------------------------------------------------------------------------------------------------------------------
# opaque, empty and partly saturated rays

@pytest.mark.parametrize("family", sorted(RC.FAMILIES))
def test_saturated_and_empty_rays(family):
    """Forward, termination_probs and backward of the three families (n = 8, T = 70), existing tolerances.  These are
    the cancellation-prone ends of rest = F - pw_incl in the backward."""
    case = RC.FAMILIES[family]()
    d = Dev(case)
    ref = RC.quad_reference(case)
    probs, outputs, alphas = assert_forward(d, ref)
    gd, gc, ga, _ = assert_backward(d, ref, outputs)
    t = case.t
    if family == "empty":
        assert torch.equal(outputs.cpu(), case.bg.expand(case.n, 3))
        assert (alphas == 0).all()
        assert (probs[:, t] == 1).all() and (probs[:, :t] == 0).all()
    if family == "opaque":
        assert (probs[:, t] == 0).all() and (alphas == 1).all()
        for r, k in enumerate(RC.OPAQUE_AT):
            assert (probs[r, k + 1:] == 0).all(), (r, k)
            assert (gc[r, k + 1:] == 0).all() and (ga[r, k + 1:] == 0).all(), (r, k)
    if family == "late":
        assert (probs[:, :64] == 0).all() and (gc[:, :64] == 0).all() and (ga[:, :64] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# missed rays in the backward

def poison_word(pattern: int) -> int:
    return int(np.array([pattern] * 4, dtype=np.uint8).view(np.int32)[0])


@pytest.mark.parametrize("pattern", [0x41, 0xFF])
@pytest.mark.parametrize("which", ["mixed", "all_missed"])
def test_backward_writes_zeros_for_missed_rays(which, pattern):
    """The C ABI on gradient arrays and a scratch block that start as poison: rows of masked rays are exactly 0 (stored,
    not left over), no poisoned word survives, g_background = sum of g over misses + p_bg * g over hits."""
    from learn_nerf import _lib as L

    case = RC.missed_case() if which == "mixed" else RC.all_missed_case()
    d = Dev(case)
    ref = RC.quad_reference(case)
    n, t, n_aux = case.n, case.t, case.n_aux
    nbytes = L.lib().lnrf_composite_bwd_scratch_bytes(n)
    with poisoned(pattern):
        gd = torch.empty((n, t), dtype=F32, device="cuda")
        gc = torch.empty((n, t, 3), dtype=F32, device="cuda")
        ga = torch.empty((n, t, n_aux), dtype=F32, device="cuda")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    word = poison_word(pattern)
    for x in (gd, gc, ga):
        assert (x.view(torch.int32) == word).all(), "the fill did not happen"
        assert not (x == 0).any()
    assert (scratch == pattern).all()
    g_bg = torch.zeros(3, device="cuda")
    gw = (L.c_float * 4)(*case.gw, 0.0, 0.0)
    rc = abi_bwd(d, n_aux, d.aux, gw, gd, gc, ga, g_bg, L.ptr(scratch, torch.uint8), nbytes)
    assert rc == 0, last_error()
    miss = ~case.mask
    for x in (gd, gc, ga):
        assert (x.view(torch.int32) != word).all(), "a poisoned word survived"
        assert torch.isfinite(x).all()
        assert (x.cpu()[miss] == 0).all()
    assert torch.allclose(cpu64(gd), ref.g_density, atol=2e-6, rtol=1e-4)
    assert torch.allclose(cpu64(gc), ref.g_rgb, atol=2e-7, rtol=1e-4)
    assert torch.allclose(cpu64(ga), ref.g_aux, atol=2e-7, rtol=1e-4)
    assert torch.allclose(cpu64(g_bg), ref.g_background, atol=2e-6, rtol=1e-4)
    if which == "all_missed":
        assert (gd == 0).all() and (gc == 0).all() and (ga == 0).all()
        assert torch.allclose(cpu64(g_bg), case.g_out.double().sum(0), atol=2e-6, rtol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# background fold beyond 256 partial rows

@pytest.mark.parametrize("n", RC.FOLD_NS)
def test_background_fold_beyond_256_rows(n):
    """258 and 513 workgroups: the fold's loop over b += 256 takes a second and a third trip.  Rays are mixed hit / miss
    with per-ray gradients of mixed sign over three decades, so a dropped row shows."""
    from learn_nerf import _lib as L

    case = RC.fold_case(n)
    d = Dev(case)
    ref = RC.quad_reference(case)
    _, _, _, g_bg = assert_backward(d, ref)
    # every trip's rows carry a share of the sum far above that tolerance (rays_edge_cases.fold_trip_shares, asserted
    # in test_rays_edge_cases_cpu.py)
    g_bg2 = torch.zeros(3, device="cuda")
    d.bwd(g_bg2)
    assert torch.equal(g_bg, g_bg2), "the fold is not bit-reproducible"
    pre = torch.tensor([1.0, 2.0, 3.0], device="cuda")
    g_bg3 = pre.clone()
    d.bwd(g_bg3)
    assert torch.equal(g_bg3, pre + g_bg), "the fold must accumulate into g_background"

    # scratch size and alignment at the C ABI
    nbytes = L.lib().lnrf_composite_bwd_scratch_bytes(n)
    assert nbytes == ((n + 3) // 4) * 16 + 16
    t = case.t
    gd, gc = torch.empty((n, t), device="cuda"), torch.empty((n, t, 3), device="cuda")
    buf = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    exact = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    gw = (L.c_float * 4)(0.0, 0.0, 0.0, 0.0)
    g_bg4 = torch.zeros(3, device="cuda")
    assert abi_bwd(d, 0, None, gw, gd, gc, None, g_bg4, L.ptr(exact, torch.uint8), nbytes) == 0, last_error()
    assert torch.equal(g_bg4, g_bg)
    fill = 7.0
    gd.fill_(fill)
    g_bg5 = torch.full((3,), fill, device="cuda")
    assert abi_bwd(d, 0, None, gw, gd, gc, None, g_bg5, L.ptr(exact, torch.uint8), nbytes - 1) == ERR_ARG
    assert "scratch" in last_error()
    assert abi_bwd(d, 0, None, gw, gd, gc, None, g_bg5, L.c_void_p(buf.data_ptr() + 4), nbytes) == ERR_ARG
    assert "scratch" in last_error()
    assert (gd == fill).all() and (g_bg5 == fill).all()


# ---------------------------------------------------------------------------------------------------------------------
# fine sampling

def run_fine(case, tf, **kw):
    from learn_nerf import ops

    ts, t_min, t_max, dens = g(case.ts), g(case.t_min), g(case.t_max), g(case.dens)
    out = ops.fine_sample(ts, t_min, t_max, dens, tf, u=g(case.uf), **kw)
    new_only = ops.fine_sample(ts, t_min, t_max, dens, tf, u=g(case.uf), combine=False, **kw)
    assert out.shape == (case.ts.shape[0], case.ts.shape[1] + tf) and new_only.shape == (case.ts.shape[0], tf)
    # combine == exact sort of [coarse ts, new ts] (render.py:253-255): bit-exact check
    assert torch.equal(out, torch.sort(torch.cat([ts, new_only], 1), 1).values)
    return out.cpu(), new_only.cpu()


@pytest.mark.parametrize("n,tc,tf", [(1, 1, 1), (3, 1, 5), (5, 2, 1)])
def test_fine_sample_smallest_sizes(n, tc, tf):
    case = RC.fine_case(n, tc, tf, seed=tc + tf)
    out, new_only = run_fine(case, tf)
    s = case.samples64()
    ref = s.fine_sampling(tf, case.uf.double(), case.dens.double(), combine=False).ts
    assert torch.allclose(new_only.double(), ref, atol=2e-5, rtol=0)
    ref_all = s.fine_sampling(tf, case.uf.double(), case.dens.double(), combine=True).ts
    assert torch.allclose(out.double(), ref_all, atol=2e-5, rtol=0)


@pytest.mark.parametrize("uf", [0.0, RC.U_MAX])
def test_fine_sample_extreme_uniforms(uf):
    """Every uniform 0, and every uniform 1 - 2^-24 (the largest Philox returns): x sits on a stratum's edge."""
    n, tc, tf = 5, 64, 131
    case = RC.fine_case(n, tc, tf, seed=3, uf=uf)
    out, new_only = run_fine(case, tf)
    assert (new_only >= case.t_min[:, None]).all() and (new_only <= case.t_max[:, None]).all()
    assert (new_only[:, 1:] >= new_only[:, :-1]).all() and (out[:, 1:] >= out[:, :-1]).all()
    RC.fine_cdf_check(new_only, case.samples64(), case.dens, case.uf)


@pytest.mark.parametrize("tf", RC.FINE_LDS_TFS)
def test_fine_sample_up_to_the_lds_limit(tf):
    """Dynamic LDS of 65 536 B, 65 552 B and 163 840 B (the largest lnrf_fine_sample accepts), both combine modes; at
    65 552 B also shuffled coarse ts, so the rank-count fallback runs past 64 KB."""
    tc = RC.FINE_LDS_TC
    assert RC.fine_sample_lds_bytes(tc, tf) in (65536, 65552, 163840)
    case = RC.fine_case(5, tc, tf, seed=7)
    out, new_only = run_fine(case, tf)
    assert (out[:, 1:] >= out[:, :-1]).all()
    RC.fine_cdf_check(new_only, case.samples64(), case.dens, case.uf)
    if tf == 3903:
        shuffled = RC.fine_case(2, tc, tf, seed=8, shuffle=True)
        assert not (shuffled.ts[:, 1:] >= shuffled.ts[:, :-1]).all()
        out2, _ = run_fine(shuffled, tf)
        assert (out2[:, 1:] >= out2[:, :-1]).all()


def test_fine_sample_past_the_lds_limit_is_an_argument_error():
    from learn_nerf import _lib as L

    tc, tf = RC.FINE_LDS_TC, RC.FINE_LDS_TF_TOO_LARGE
    case = RC.fine_case(5, tc, tf, seed=9)
    ts, t_min, t_max, dens, uf = g(case.ts), g(case.t_min), g(case.t_max), g(case.dens), g(case.uf)
    for combine in (0, 1):
        out = torch.full((5, tf + (tc if combine else 0)), 7.0, device="cuda")
        rc = L.lib().lnrf_fine_sample(L.ptr(ts), L.ptr(t_min), L.ptr(t_max), L.ptr(dens), 5, tc, tf, 1e-8, combine,
                                      L.ptr(uf), 0, 1, 0, L.ptr(out), L.stream())
        assert rc == ERR_ARG, (rc, last_error())
        assert "too large for LDS" in last_error()
        torch.cuda.synchronize()
        assert (out == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# Philox counters past 2^32

def test_philox_high_counter_word():
    """ray_offset = 2^33 with count 7 puts (ray_offset + n) * count + i past 2^34, so the counter's high word is 3: the
    kernels' Philox must equal the oracle's bit for bit there, in all three kernels that draw."""
    from learn_nerf import ops

    n, count, off, seed, stream = 6, 7, 2 ** 33, 0x1234ABCD5678, 3
    assert ((off * count) >> 2) >> 32 != 0
    rays = g(RC.degenerate_rays()[[0, 3, 5, 9, 11, 13]].contiguous())
    u_hi = g(torch.from_numpy(philox.ray_uniforms(seed, stream, off, n, count)))
    a = ops.ray_aabb_stratified(rays, RC.BBOX_MIN, RC.BBOX_MAX, count, u=u_hi)
    assert a[2].all(), "these rows are hits"
    b = ops.ray_aabb_stratified(rays, RC.BBOX_MIN, RC.BBOX_MAX, count, seed=seed, stream_id=stream, ray_offset=off)
    assert torch.equal(a[3], b[3])
    assert torch.equal(ops.stratified(a[0], a[1], count, seed=seed, stream_id=stream, ray_offset=off), a[3])
    zero = ops.ray_aabb_stratified(rays, RC.BBOX_MIN, RC.BBOX_MAX, count, seed=seed, stream_id=stream, ray_offset=0)
    assert not torch.equal(zero[3], b[3])
    assert not torch.equal(ops.stratified(a[0], a[1], count, seed=seed, stream_id=stream, ray_offset=0), a[3])

    case = RC.fine_case(n, 5, count, seed=4)
    ts, t_min, t_max, dens = g(case.ts), g(case.t_min), g(case.t_max), g(case.dens)
    uf = g(torch.from_numpy(philox.ray_uniforms(seed, 1, off, n, count)))
    want = ops.fine_sample(ts, t_min, t_max, dens, count, u=uf)
    assert torch.equal(ops.fine_sample(ts, t_min, t_max, dens, count, seed=seed, stream_id=1, ray_offset=off), want)
    assert not torch.equal(ops.fine_sample(ts, t_min, t_max, dens, count, seed=seed, stream_id=1, ray_offset=0), want)

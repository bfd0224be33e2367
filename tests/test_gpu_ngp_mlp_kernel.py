"""
The fused InstantNGP MLP kernels (csrc/ngp_mlp.hip) through the C ABI against the float64 emulation of
ngp_mlp_reference.py, on rounding-safe inputs.

lnrf_ngp_mlp_bwd writes no dump, so its stages cannot be recomputed from its own intermediates.  Instead the inputs are chosen
so that, for the evaluations that carry an upstream gradient, no fp32 accumulation error can move any bf16 value inside
the kernel (every margin of the emulation exceeds its delta; sparse Dense_0..3, see the reference module).  g_enc_t, dW_l
and db_l then differ from float64 by ONE fp32 accumulation:

  g_enc_t           per element (K + 2) 2^-23 |dy0| |W0|^T, K = non-zero products + 4 k-steps; exactly 0 elsewhere
  dW_l, db_l        per entry (n_nonzero + n_rows + 2) 2^-23 |X|^T |dy|: n_nonzero evaluations carry a gradient (<= ~4000, so
                    the bound stays below one dropped evaluation, and far below one dropped group), n_rows partial rows and
                    slice sums are folded by the reduce launch; an exact-zero reference must be exactly 0
  level_absmax      bit-equal to max |g_enc_t| over each level's two rows
  density, rgb      safe evaluations: propagated delta + EXP / TANH allowance (measured, see below); others 2e-3

Every call runs on synthetic enc_t (no hash grid), a scratch of 0xFF bytes, outputs that are views into larger buffers with
sentinel words on both sides, and three backward calls: into zeros (-> the added vector `tot`), into a random prefill P
(must be fp32(P + tot) bit for bit, the words in front of dense_offset untouched) and once more on top (fp32(g1 + tot)).

Shapes: single group per workgroup m in {1, 31, 33, 255, 257, 2053} x enc_dim {2, 16, 18, 32}; multi-group m = 256 (2 CUs
+ 3) - 5 (workgroups of the persistent backward loop over 2 or 3 groups, ragged last tile) x enc_dim {16, 32} x three masks
of the upstream gradient: first round only, later rounds only, 7 evaluations of every group.  Also: one call against
2048-evaluation chunks with dense weights (position independence), lnrf_ngp_mlp_fwd_split against the exact model, and
the forward of the unsafe evaluations (2e-3 gate, and tightly under an admissible rounding of their near-boundary points).

The allowance for __expf / tanhf cannot be derived from the project: it is 4 x the largest error beyond the propagated
delta measured on the MI355X over all cases of this file (density 5.4e-8 relative, rgb none: the tanh error stays inside
the accumulation bound of its argument), at least 4 fp32 ulp (a correctly rounded routine already has half an ulp), and
never above 1e-5, the value the safety margins of dy4 and dy1 assume.  Both come out at 2.4e-7.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ngp_mlp_reference as R
from test_gpu_nerf_backward_edges import device_tag

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel words on either side of every output
SENTINEL = 0x7FC5A5A5  # a NaN pattern no kernel produces
MEASURED_EXP_EXCESS, MEASURED_TANH_EXCESS = 5.5e-8, 0.0  # largest error beyond the propagated delta, MI355X, all cases here
ULP4 = 4 * 2.0 ** -24
EXP_ALLOWANCE = min(max(4 * MEASURED_EXP_EXCESS, ULP4), R.LIBM_ALLOWANCE)
TANH_ALLOWANCE = min(max(4 * MEASURED_TANH_EXCESS, ULP4), R.LIBM_ALLOWANCE)
MAX_ACTIVE = 4000
CHUNK = 2048


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def guarded(n):
    """-> (buffer with sentinels, fp32 view of n words between them)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def assert_guards(buf, n, what):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), f"{what}: words outside the output were written"


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


class Kernels:
    """one parameter vector packed for one encoding width; every call goes through the C ABI"""

    def __init__(self, lf, dense_offset, flat):
        from learn_nerf import _lib as L
        self.L, self.lib, self.lf, self.off = L, L.lib(), lf, dense_offset
        self.desc = L.NgpMlpDesc(lf, R.HIDDEN, R.DENSITY_DIM, 1, 2, R.D_FREQS, dense_offset)
        self.n_flat = dense_offset + R.dense_params(lf)
        assert flat.shape == (self.n_flat,)
        self.flat = dev(flat)
        self.tag = f"enc_dim={lf} dense_offset={dense_offset} {device_tag()}"

    def _pack(self, split):
        L, lib, by = self.L, self.lib, ctypes.byref(self.desc)
        n = lib.lnrf_ngp_mlp_packed_split_bytes(by) if split else lib.lnrf_ngp_mlp_packed_bytes(by)
        packed = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
        fn = lib.lnrf_ngp_mlp_pack_split if split else lib.lnrf_ngp_mlp_pack
        L.check(fn(by, L.ptr(self.flat), L.ptr(packed, torch.uint8), L.stream()), "ngp_mlp_pack")
        return packed

    def forward(self, enc_t, d, split=False):
        """lnrf_ngp_mlp_fwd / _fwd_split -> density [m], rgb [m, 3] (numpy); outputs are guarded views"""
        L, lib = self.L, self.lib
        m = enc_t.shape[1]
        packed = self._pack(split)
        dbuf, dens = guarded(m)
        rbuf, rgb = guarded(3 * m)
        fn, name = (lib.lnrf_ngp_mlp_fwd_split, "lnrf_ngp_mlp_fwd_split") if split else (lib.lnrf_ngp_mlp_fwd, "lnrf_ngp_mlp_fwd")
        L.check(fn(ctypes.byref(self.desc), L.ptr(packed, torch.uint8), L.ptr(enc_t), L.ptr(d), m, L.ptr(dens), L.ptr(rgb),
                   L.stream()), name)
        torch.cuda.synchronize()
        assert_guards(dbuf, m, f"{name} density m={m} {self.tag}")
        assert_guards(rbuf, 3 * m, f"{name} rgb m={m} {self.tag}")
        return dens.cpu().numpy(), rgb.cpu().numpy().reshape(m, 3)

    def backward(self, enc_t, d, gd, gc, grads_in):
        """lnrf_ngp_mlp_bwd into a guarded copy of `grads_in` (fp32 numpy, whole vector) with a 0xFF scratch
        -> g_enc_t [lf, m], level_absmax [lf // 2], grads (numpy)"""
        L, lib, lf = self.L, self.lib, self.lf
        m = enc_t.shape[1]
        what = f"lnrf_ngp_mlp_bwd m={m} {self.tag}"
        packed = self._pack(False)
        scratch = torch.full((lib.lnrf_ngp_mlp_scratch_bytes(ctypes.byref(self.desc), m),), 0xFF, dtype=torch.uint8, device="cuda")
        gbuf, g_enc = guarded(lf * m)
        wbuf, grads = guarded(self.n_flat)
        grads.copy_(dev(grads_in))
        lmax = torch.zeros(lf // 2, device="cuda")
        L.check(lib.lnrf_ngp_mlp_bwd(ctypes.byref(self.desc), L.ptr(packed, torch.uint8), L.ptr(enc_t), L.ptr(d), L.ptr(gd),
                                     L.ptr(gc), m, L.ptr(scratch, torch.uint8), L.ptr(g_enc), L.ptr(lmax), L.ptr(grads),
                                     L.stream()), "lnrf_ngp_mlp_bwd")
        torch.cuda.synchronize()
        assert_guards(gbuf, lf * m, f"{what} g_enc_t (rows >= enc_dim do not exist)")
        assert_guards(wbuf, self.n_flat, f"{what} grads")
        out = grads.cpu().numpy()
        assert np.array_equal(out[:self.off].view(np.uint32), np.asarray(grads_in, np.float32)[:self.off].view(np.uint32)), \
            f"{what}: words in front of dense_offset changed"
        return g_enc.cpu().numpy().reshape(lf, m), lmax.cpu().numpy(), out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def three_backwards(k, enc_t, d, gd, gc, seed, what):
    """backward into zeros, into a random prefill, and once more on top.  -> g_enc_t, level_absmax, tot (Dense part), g1 (Dense
    part, prefilled call).  Asserts: g1 == fp32(P + tot) and g2 == fp32(g1 + tot) bit for bit (the backward is deterministic
    and accumulates), g_enc_t and level_absmax identical in all three."""
    zeros = np.zeros(k.n_flat, np.float32)
    prefill = np.random.default_rng(seed).standard_normal(k.n_flat).astype(np.float32)
    g0, l0, tot = k.backward(enc_t, d, gd, gc, zeros)
    g1, l1, a1 = k.backward(enc_t, d, gd, gc, prefill)
    g2, l2, a2 = k.backward(enc_t, d, gd, gc, a1)
    assert np.array_equal(bits(g0), bits(g1)) and np.array_equal(bits(g0), bits(g2)), f"{what}: g_enc_t differs between calls"
    assert np.array_equal(bits(l0), bits(l1)) and np.array_equal(bits(l0), bits(l2)), f"{what}: level_absmax differs between calls"
    assert np.isfinite(tot).all(), f"{what}: non-finite Dense gradient (a word of the 0xFF scratch was folded?)"
    for name, got, base in (("prefilled", a1, prefill), ("second", a2, a1)):
        want = base[k.off:] + tot[k.off:]  # one correctly rounded fp32 addition, as the reduce launch's +=
        diff = np.flatnonzero(bits(got[k.off:]) != bits(want))
        assert diff.size == 0, (f"{what}: the {name} call did not add the vector of the first call bit for bit at {diff.size} "
                                f"Dense entries, first {diff[:8]}")
    return g0, l0, tot[k.off:], a1[k.off:]


STATS = {}


def report(case, ratios, x_d, x_y, safe_share, n_active):
    STATS[case] = (ratios, x_d, x_y)
    worst = {k: round(v, 4) for k, v in ratios.items()}
    print(f"[ngp-mlp] {case}: safe share {safe_share:.3f}, {n_active} evaluations with gradient; forward excess over the "
          f"propagated delta: density {x_d:.3e} rgb {x_y:.3e}; error-to-bound ratios {worst}")


def run_tight(lf, m, dense_offset, flat, enc_t, d, em, safe, active, gd, gc, case, seed):
    k = Kernels(lf, dense_offset, flat)
    n_wg = R.n_workgroups(m, cu_count())
    what = f"{case} ({k.tag}, {n_wg} workgroups)"
    enc_dev, d_dev = dev(enc_t), dev(d)
    dens, rgb = k.forward(enc_dev, d_dev)
    x_d, x_y = R.check_forward_safe(em, dens, rgb, EXP_ALLOWANCE, TANH_ALLOWANCE, f"lnrf_ngp_mlp_fwd {what}")
    g_enc, lmax, tot, g1 = three_backwards(k, enc_dev, d_dev, dev(gd), dev(gc), seed, f"lnrf_ngp_mlp_bwd {what}")
    ratios = R.check_backward(em, active, n_wg, g_enc, lmax, tot, f"lnrf_ngp_mlp_bwd {what}")
    prefill = np.random.default_rng(seed).standard_normal(k.n_flat).astype(np.float32)[dense_offset:]
    R.check_backward(em, active, n_wg, g_enc, lmax, g1.astype(np.float64) - prefill, f"lnrf_ngp_mlp_bwd (got - prefill) {what}",
                     final_add_of=g1)
    report(case, ratios, x_d, x_y, safe.mean(), int(active.sum()))
    return g_enc, lmax


SINGLE = [c for c in R.gpu_cases(1) if c[1] in R.SINGLE_GROUP_M]


@pytest.mark.parametrize("case", SINGLE, ids=lambda c: f"enc{c[0]}-m{c[1]}-off{c[2]}")
def test_single_group_per_workgroup(case):
    lf, m, off, seed = case
    assert R.groups_of(m) <= cu_count() and m <= MAX_ACTIVE
    flat, enc_t, d, gd, gc, fw, safe = R.safe_share_inputs(lf, m, off, seed)
    assert safe.mean() >= R.SAFE_SHARE_MIN
    em, safe, active, gd, gc = R.safe_problem(flat, off, enc_t, d, gd, gc, fw=fw, safe=safe)
    run_tight(lf, m, off, flat, enc_t, d, em, safe, active, gd, gc, f"single-group enc_dim={lf} m={m}", seed)


@pytest.mark.parametrize("case", SINGLE, ids=lambda c: f"enc{c[0]}-m{c[1]}-off{c[2]}")
def test_forward_of_unsafe_evaluations_single_group(case):
    """the evaluations outside the tight check keep the end-to-end gate: 2e-3 against the emulation"""
    lf, m, off, seed = case
    flat, enc_t, d, gd, gc, fw, safe = R.safe_share_inputs(lf, m, off, seed)
    k = Kernels(lf, off, flat)
    dens, rgb = k.forward(dev(enc_t), dev(d))
    R.check_forward_unsafe(fw, dens, rgb, f"lnrf_ngp_mlp_fwd single-group m={m} {k.tag}")


@functools.lru_cache(maxsize=None)
def multi_inputs(lf):
    (case,) = [c for c in R.gpu_cases(cu_count()) if c[0] == lf and c[1] == R.multi_group_m(cu_count())]
    return case, R.safe_share_inputs(*case)


def choose(cand, n, rng):
    idx = np.flatnonzero(cand)
    out = np.zeros(cand.size, bool)
    out[idx if idx.size <= n else rng.choice(idx, n, replace=False)] = True
    return out


def upstream_mask(variant, safe, n_wg, rng):
    """which safe evaluations keep their upstream gradient (at most about MAX_ACTIVE)"""
    m = safe.size
    ev = np.arange(m)
    group = ev // R.EVALS_PER_GROUP
    ragged = ev >= m - m % R.EVALS_PER_TILE
    if variant == "first-round":
        return choose(safe & (group < n_wg), MAX_ACTIVE, rng)
    if variant == "later-rounds":  # every safe evaluation of the third round and of the ragged tile, the rest at random
        must = safe & ((group >= 2 * n_wg) | ragged)
        return must | choose(safe & (group >= n_wg) & ~must, MAX_ACTIVE - int(must.sum()), rng)
    assert variant == "every-group"
    key = np.where(safe, rng.random(m), np.inf)
    keep = safe & ragged
    for g in range(int(group.max()) + 1):
        lo, hi = g * R.EVALS_PER_GROUP, min((g + 1) * R.EVALS_PER_GROUP, m)
        pick = lo + np.argsort(key[lo:hi])[:7]
        keep[pick[np.isfinite(key[pick])]] = True
    return keep


@pytest.mark.parametrize("variant", ["first-round", "later-rounds", "every-group"])
@pytest.mark.parametrize("lf", R.MULTI_ENC_DIMS)
def test_multi_group_persistent_loop(lf, variant):
    cus = cu_count()
    (_, m, off, seed), (flat, enc_t, d, gd, gc, fw, safe) = multi_inputs(lf)
    n_wg = R.n_workgroups(m, cus)
    per_wg = {len(range(w, R.groups_of(m), n_wg)) for w in range(n_wg)}
    assert per_wg == {2, 3} and m % R.EVALS_PER_TILE != 0, f"{cus} CUs: workgroups take {per_wg} groups"
    assert safe.mean() >= R.SAFE_SHARE_MIN
    keep = upstream_mask(variant, safe, n_wg, np.random.default_rng(seed + 1))
    em, safe, active, gd, gc = R.safe_problem(flat, off, enc_t, d, gd, gc, keep=keep, fw=fw, safe=safe)
    rounds = np.arange(m) // R.EVALS_PER_GROUP // n_wg
    present = set(np.unique(rounds[active]).tolist())
    assert present == {"first-round": {0}, "later-rounds": {1, 2}, "every-group": {0, 1, 2}}[variant]
    assert 0 < active.sum() <= MAX_ACTIVE + 300 and active[m - m % R.EVALS_PER_TILE:].any() == (variant != "first-round")
    g_enc, lmax = run_tight(lf, m, off, flat, enc_t, d, em, safe, active, gd, gc,
                            f"multi-group {variant} enc_dim={lf} m={m}", seed)
    if variant == "later-rounds":  # every level's maximum comes from a later round here
        assert (lmax > 0).all() and (rounds[np.abs(g_enc).reshape(lf // 2, 2, m).max(1).argmax(1)] >= 1).all()


@pytest.mark.parametrize("lf", R.MULTI_ENC_DIMS)
def test_forward_of_unsafe_evaluations_multi_group(lf):
    """The evaluations outside the tight check against the end-to-end gate, 2e-3 against the emulation, at the multi-group m
    (about a quarter of the 131835 evaluations).  A correct kernel can meet it because the input generator redraws every
    evaluation on which one admissible rounding of a near-boundary point would move density or rgb by more than 1e-3
    (ngp_mlp_reference.flip_hazard: about 1 % of the raw draws, decided from the emulation alone)."""
    (_, m, off, seed), (flat, enc_t, d, gd, gc, fw, safe) = multi_inputs(lf)
    k = Kernels(lf, off, flat)
    dens, rgb = k.forward(dev(enc_t), dev(d))
    n = R.check_forward_unsafe(fw, dens, rgb, f"lnrf_ngp_mlp_fwd multi-group m={m} {k.tag}")
    print(f"[ngp-mlp] multi-group enc_dim={lf} m={m}: {n} forward-unsafe evaluations within 2e-3")


@pytest.mark.parametrize("lf", R.MULTI_ENC_DIMS)
def test_unsafe_evaluations_follow_an_admissible_rounding(lf):
    """The unsafe evaluations, tightly: every forward-unsafe evaluation of the multi-group m meets the
    TIGHT bound of the safe ones against the emulation under one of the admissible roundings of its near-boundary points."""
    (_, m, off, seed), (flat, enc_t, d, gd, gc, fw, safe) = multi_inputs(lf)
    k = Kernels(lf, off, flat)
    dens, rgb = k.forward(dev(enc_t), dev(d))
    n, n_other, n_many = R.check_forward_admissible(fw, flat, off, enc_t, d, dens, rgb, EXP_ALLOWANCE, TANH_ALLOWANCE,
                                                    f"lnrf_ngp_mlp_fwd multi-group m={m} {k.tag}")
    print(f"[ngp-mlp] multi-group enc_dim={lf} m={m}: {n} forward-unsafe evaluations, {n_other} took another admissible "
          f"rounding than the emulation, {n_many} with more than 4 near-boundary points not enumerated")
    assert n_many <= n // 100


@pytest.mark.parametrize("lf", R.MULTI_ENC_DIMS)
def test_position_independence_with_dense_weights(lf):
    """Dense Flax-initialised weights (the general numerics the sparse weights do not cover): one call at the multi-group m
    against calls on consecutive chunks of 2048 evaluations (a multiple of 256: every evaluation keeps its wave and lane)."""
    cus = cu_count()
    m, off = R.multi_group_m(cus), R.DENSE_OFFSETS[1]
    flat = R.flax_params(lf, off, seed=11 * lf)
    enc_t, d, gd, gc = R.inputs(lf, m, seed=11 * lf + 1)
    k = Kernels(lf, off, flat)
    what = f"position independence m={m} {k.tag}"
    zeros = np.zeros(k.n_flat, np.float32)
    dens, rgb = k.forward(dev(enc_t), dev(d))
    g_enc, lmax, big = k.backward(dev(enc_t), dev(d), dev(gd), dev(gc), zeros)
    csum, cmax, n_chunks = np.zeros(k.n_flat), np.zeros(lf // 2, np.float32), 0
    for lo in range(0, m, CHUNK):
        hi = min(lo + CHUNK, m)
        e, dd = dev(enc_t[:, lo:hi]), dev(d[lo:hi])
        cd, cr = k.forward(e, dd)
        cg, cl, cw = k.backward(e, dd, dev(gd[lo:hi]), dev(gc[lo:hi]), zeros)
        for name, a, b in (("density", dens[lo:hi], cd), ("rgb", rgb[lo:hi], cr), ("g_enc_t", g_enc[:, lo:hi], cg)):
            diff = np.flatnonzero((bits(a) != bits(b)).reshape(-1))
            assert diff.size == 0, f"{what}: {name} of evaluations {lo}..{hi} differs from the chunk call at {diff.size} words"
        csum += cw
        cmax = np.maximum(cmax, cl)
        n_chunks += 1
    assert np.array_equal(bits(lmax), bits(cmax)), f"{what}: level_absmax {lmax} != maximum of the chunks {cmax}"
    em = R.emulate(flat, off, enc_t, d, gd, gc, margins=False)
    n_wg = R.n_workgroups(m, cus)
    pos = off
    for l, (dw, sw, db, sb) in enumerate(R.wgrad_reference(em)):
        n_add = m + n_chunks + R.n_rows(l, n_wg) + R.n_rows(l, R.n_workgroups(CHUNK, cus))
        for kind, s in (("kernel", sw), ("bias", sb)):
            ratio = R.check_accumulated(big[pos:pos + s.size].reshape(s.shape), csum[pos:pos + s.size].reshape(s.shape), n_add,
                                        s * (1 + 2.0 ** -6), what=f"{what}: Dense_{l} {kind} gradient, one call against the chunks")
            print(f"[ngp-mlp] position independence enc_dim={lf} Dense_{l}/{kind}: error-to-bound ratio {ratio:.2e}")
            pos += s.size


@pytest.mark.parametrize("m", [33, 2053])
@pytest.mark.parametrize("lf", [2, 16, 18])
def test_split_forward_against_the_exact_model(lf, m):
    """lnrf_ngp_mlp_pack_split + _fwd_split with dense weights against the exact float64 model at the project's 5e-5 gates"""
    off = R.DENSE_OFFSETS[(lf + m) % 3]
    flat = R.flax_params(lf, off, seed=13 * lf + m, bias_std=0.1)
    enc_t, d, _, _ = R.inputs(lf, m, seed=13 * lf + m + 1)
    k = Kernels(lf, off, flat)
    dens, rgb = k.forward(dev(enc_t), dev(d), split=True)
    ex = R.forward(flat, off, enc_t, d, rnd=lambda v: np.asarray(v, np.float64), margins=False)
    e_rgb = np.abs(rgb.astype(np.float64) - ex["rgb"]).max()
    e_den = (np.abs(dens.astype(np.float64) - ex["density"]) / (1e-3 + ex["density"])).max()
    print(f"[ngp-mlp] lnrf_ngp_mlp_fwd_split enc_dim={lf} m={m}: rgb {e_rgb:.2e}, density rel {e_den:.2e}")
    assert e_rgb < 5e-5 and e_den < 5e-5, f"lnrf_ngp_mlp_fwd_split m={m} {k.tag}: rgb {e_rgb:.3e} density {e_den:.3e}"

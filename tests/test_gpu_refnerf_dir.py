"""
The fused Ref-NeRF directional block (csrc/refnerf_fused.hip: Dense_9 273 -> 128 relu, Dense_10 128 -> 3) through the C ABI,
stage by stage in float64: lnrf_refnerf_dir_fwd, lnrf_refnerf_dir_bwd, lnrf_refnerf_dir_fwd_split.

The forward leaves every activation in dsave, the backward every gradient in the front of its scratch
(nerf_dump_decode.dir_layouts()), so each stage is recomputed from the KERNEL'S OWN decoded operands by
refnerf_dir_reference.py (rules and derivations there; test_refnerf_dir_reference_cpu.py shows that a correct
implementation stays inside every bound and that each mutation is rejected):

  xin, dy10          bit-equal to bf16_rne of the fp32 input (ties to even, -0.0 kept); pad k-slots, the second dy10 slot and the
                     rows of invalid evaluations exactly zero
  h9, dy9            check_rounded with delta = dot_delta(K, sum |a||b| (+ |bias|)), K = 288 / 16, + the cap; mask9 == h9 > 0
  dir_out, g_dir_in  check_accumulated, K = 128
  dW9, db9, dW10, db10   check_accumulated, n_add = evaluations with a non-zero upstream gradient + the slabs the fold adds;
                     an exact-zero reference entry must be exactly 0
  g_dir_in columns   273 .. min(ld, 288) - 1 hold 0, nothing at or beyond column 288 and no row >= m is written (lnrf.h)

Every call: 0xFF-filled blobs, dsave and scratch; dir_in with NaN in columns 273 .. ld - 1; outputs are views inside
sentinel-filled buffers.  Three backward calls (into zeros -> tot, into a random prefill P -> fp32(P + tot) bit for bit, once
more on top); every gradient word outside the Dense_9 / Dense_10 ranges bit-untouched; everything bit-identical across ld.

Sizes: m in {1, 31, 33, 1000, 2053} x ld in {276, 292}, ld in {280, 320} at m = 33; weight gradients over several
workgroups at m = 32 (2 200 + 3) - 5 = 12891.  At that m the launch caps a problem at one workgroup per 6 tiles
(nerf_wgrad.h), so Dense_9 runs on 68 workgroups of 6 tiles and Dense_10 on 56 of 8 (the last five own none); the masks of
the upstream gradient take the first / the last tile of every workgroup's range, or seven evaluations of every tile.
Once more at m = 32 (6 200 + 3) - 5 = 38491, the smallest size of that form at which the cap no longer binds and the fold
runs over every workgroup the two problems ask for (three evaluations of every tile carry a gradient).

Split forward: the bound derived in refnerf_dir_reference.py on every row; the model-level 2e-4 absolute gate on every row
but the edge rows of magnitude 1e4 (an absolute gate made for inputs of the model's scale says nothing about those).
Figures measured on an MI355X are recorded in DESIGN.md (Ref-NeRF path); they are not gates.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nerf_dump_decode as D
import refnerf_dir_reference as R
from test_gpu_nerf_backward_edges import device_tag

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel words on either side of every output (256 bytes: the views stay 16-byte aligned)
SENTINEL = R.SENTINEL
EXTRA_ROWS = 2  # sentinel rows behind row m - 1 of g_dir_in


def guarded(n):
    """-> (int32 buffer of sentinels, fp32 view of the n words between the guards — sentinels too until written)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def assert_guards(buf, n, what):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), f"{what}: words outside the output were written"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ff_bytes(n):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")


class Kernels:
    def __init__(self):
        from learn_nerf import _lib as L
        self.L, self.lib = L, L.lib()
        self.flat_cpu = R.make_params()
        self.flat = self.flat_cpu.cuda()
        self.w = R.Weights(self.flat_cpu)
        self.n = self.flat.numel()
        self.packed = ff_bytes(self.lib.lnrf_refnerf_trunk_packed_bytes())
        L.check(self.lib.lnrf_refnerf_trunk_pack(L.ptr(self.flat), L.ptr(self.packed, torch.uint8), L.stream()), "trunk_pack")
        self.packed3 = ff_bytes(self.lib.lnrf_refnerf_render_packed_bytes())
        L.check(self.lib.lnrf_refnerf_render_pack(L.ptr(self.flat), L.ptr(self.packed3, torch.uint8), L.stream()), "render_pack")
        torch.cuda.synchronize()

    def forward(self, x, ld, split=False):
        """x [m, 273] fp32 (CPU) -> dir_out [m, 3] (numpy), dsave (CPU uint8; None for the split kernel)"""
        L, lib = self.L, self.lib
        m = x.shape[0]
        name = "lnrf_refnerf_dir_fwd_split" if split else "lnrf_refnerf_dir_fwd"
        what = f"{name} m={m} ld={ld} {device_tag()}"
        dir_in = R.strided(x, ld).cuda()
        obuf, out = guarded(3 * m)
        if split:
            dsave = None
            rc = lib.lnrf_refnerf_dir_fwd_split(L.ptr(self.packed3, torch.uint8), L.ptr(dir_in), ld, m, L.ptr(out), L.stream())
        else:
            dsave = ff_bytes(lib.lnrf_refnerf_dir_save_bytes(m))
            rc = lib.lnrf_refnerf_dir_fwd(L.ptr(self.packed, torch.uint8), L.ptr(dir_in), ld, m, L.ptr(dsave, torch.uint8),
                                          L.ptr(out), L.stream())
        L.check(rc, name)
        torch.cuda.synchronize()
        assert_guards(obuf, 3 * m, f"{what} dir_out (rows >= m do not exist)")
        res = out.cpu().numpy().reshape(m, 3)
        assert np.isfinite(res).all(), f"{what}: dir_out is not finite (a NaN pad column or an unwritten word was read)"
        return res, dsave

    def backward(self, dsave, g, ld, grads_in):
        """-> raw words of g_dir_in [m + EXTRA_ROWS, ld], the gradient vector (numpy), the gradient dump (CPU uint8)"""
        L, lib = self.L, self.lib
        m = g.shape[0]
        what = f"lnrf_refnerf_dir_bwd m={m} ld={ld} {device_tag()}"
        scratch = ff_bytes(lib.lnrf_refnerf_dir_scratch_bytes(m))
        ibuf, g_in = guarded((m + EXTRA_ROWS) * ld)
        wbuf, grads = guarded(self.n)
        grads.copy_(torch.from_numpy(np.ascontiguousarray(grads_in, dtype=np.float32)).cuda())
        gd = g.cuda()
        L.check(lib.lnrf_refnerf_dir_bwd(L.ptr(self.packed, torch.uint8), L.ptr(dsave, torch.uint8), L.ptr(gd), m,
                                         L.ptr(scratch, torch.uint8), L.ptr(g_in), ld, L.ptr(grads), L.stream()),
                "lnrf_refnerf_dir_bwd")
        torch.cuda.synchronize()
        assert_guards(ibuf, (m + EXTRA_ROWS) * ld, f"{what} g_dir_in")
        assert_guards(wbuf, self.n, f"{what} grads")
        raw = g_in.view(torch.int32).cpu().numpy().view(np.uint32).reshape(m + EXTRA_ROWS, ld)
        return raw, grads.cpu().numpy(), scratch[:D.dir_grad_dump_bytes(m)].cpu()


@functools.lru_cache(maxsize=None)
def kernels():
    return Kernels()


class Run:
    pass


@functools.lru_cache(maxsize=None)
def run(m, ld, variant=None):
    """forward, three backward calls and their decoded dumps for one size; computed once and shared, unchanged, by the tests"""
    k = kernels()
    r = Run()
    r.m, r.ld, r.k = m, ld, k
    r.x, r.large = R.make_dir_in(m)
    r.g = R.make_g_dir_out(m, None if variant is None else R.multi_mask(variant, m))
    r.dir_out, dsave = k.forward(r.x, ld)
    r.dsave_raw = dsave.cpu()
    rng = np.random.default_rng(m + ld)
    r.prefill = rng.standard_normal(k.n).astype(np.float32)
    r.gin0, r.tot, r.dump_raw = k.backward(dsave, r.g, ld, np.zeros(k.n, np.float32))
    r.gin1, r.g1, r.dump1 = k.backward(dsave, r.g, ld, r.prefill)
    r.gin2, r.g2, r.dump2 = k.backward(dsave, r.g, ld, r.g1)
    r.save, r.grad = D.decode_dir_save(r.dsave_raw, m), D.decode_dir_grad(r.dump_raw, m)
    r.res = {"xin": r.save["xin"].numpy(), "h9": r.save["h9"].numpy(), "mask9": r.save["mask9"].numpy(),
             "dir_out": r.dir_out.astype(np.float64), "dy10": r.grad["dy10"].numpy(), "dy9": r.grad["dy9"].numpy()}
    return r


def tag(entry, r):
    return f"({entry}, m={r.m}, ld={r.ld}, {device_tag()})"


def show(r, variant, stats):
    for stage, v in stats.items():
        if isinstance(v, dict):
            print(f"[dir-stage] m={r.m:5d} ld={r.ld} {variant or '-':11s} {stage:8s} allowance share {v['allow']:.3e}  mismatch share "
                  f"{v['diff']:.3e}  CPU fp32 flip share {v['cpu']:.3e}  largest needed part of delta {v['need']:.2e}")
        else:
            print(f"[dir-stage] m={r.m:5d} ld={r.ld} {variant or '-':11s} {stage:8s} largest error-to-bound ratio {v:.4f}")


CASES = [(m, ld) for m in R.MS for ld in R.LDS_MAIN] + [(R.M_OTHER_LD, ld) for ld in R.LDS_ALL if ld not in R.LDS_MAIN]


def forward_checks(r, variant=None):
    what = tag("lnrf_refnerf_dir_fwd", r)
    s = r.save
    stats = R.check_forward(r.res, r.x, r.k.w, what)
    assert not s["pad_slots"]["xin"].numpy().any(), f"xin {what}: the k-slots of inputs 273..287 are not zero"
    assert not s["pad"]["xin"].numpy().any(), f"xin {what}: rows of invalid evaluations {r.m}.. are not zero"
    assert np.isfinite(s["pad"]["h9"].numpy()).all(), f"h9 {what}: rows of invalid evaluations are not finite"
    assert (s["pad"]["mask9"].numpy() == (s["pad"]["h9"].numpy() > 0)).all(), f"mask9 {what}: pad evaluations"
    assert not s["mask9_high"].numpy().any(), f"mask9 {what}: the 64 unused bits per lane are not zero"
    assert not s["zero_slots"], what
    show(r, variant, stats)


def backward_checks(r, variant=None):
    what = tag("lnrf_refnerf_dir_bwd", r)
    k, g = r.k, r.grad
    res = dict(r.res)
    res["g_dir_in"] = R.check_g_dir_in_buffer(r.gin0, r.m, r.ld, what)
    for name, (a, b, shape) in R.grad_ranges().items():
        res[name] = r.tot[a:b].astype(np.float64).reshape(shape)
    n_active = R.n_active_of(r.g)
    assert n_active <= R.MAX_ACTIVE
    stats = R.check_backward(res, r.g, k.w, n_active, what)
    assert not g["pad_slots"]["dy10"].numpy().any(), f"dy10 {what}: its unused k-slots or its second slot are not zero"
    assert all(not v.numpy().any() for v in g["pad"].values()), f"{what}: the pad evaluations {r.m}.. hold non-zero gradients"
    assert not g["zero_slots"], what
    show(r, variant, stats)
    # accumulation: bit for bit on top of a prefill, and once more; nothing outside the four ranges moves
    lo = R.grad_ranges()["dW9"][0]
    assert R.grad_ranges()["db10"][1] == k.n
    assert not r.tot[:lo].any(), f"{what}: gradient words in front of Dense_9 were written (call into zeros)"
    assert np.isfinite(r.tot).all(), f"{what}: non-finite gradient (a word of the 0xFF scratch was folded?)"
    for name, got, base in (("prefilled", r.g1, r.prefill), ("second", r.g2, r.g1)):
        assert np.array_equal(bits(got[:lo]), bits(base[:lo])), f"{what}: the {name} call changed words in front of Dense_9"
        diff = np.flatnonzero(bits(got[lo:]) != bits(base[lo:] + r.tot[lo:]))
        assert diff.size == 0, (f"{what}: the {name} call did not add the vector of the first call bit for bit at {diff.size} "
                                f"entries, first {lo + diff[:8]}")
    for name, a, b in (("g_dir_in", r.gin0, r.gin1), ("g_dir_in", r.gin0, r.gin2), ("gradient dump", r.dump_raw.numpy(), r.dump1.numpy()),
                       ("gradient dump", r.dump_raw.numpy(), r.dump2.numpy())):
        assert np.array_equal(a, b), f"{what}: {name} differs between two calls on the same inputs"
    if n_active:
        assert np.abs(r.tot[lo:]).max() > 0 and np.abs(res["g_dir_in"]).max() > 0
    return res, n_active


@pytest.mark.parametrize("m,ld", CASES)
def test_forward_stage_by_stage(m, ld):
    forward_checks(run(m, ld))


@pytest.mark.parametrize("m,ld", CASES)
def test_backward_stage_by_stage(m, ld):
    backward_checks(run(m, ld))


@pytest.mark.parametrize("m", R.MS)
def test_bit_identical_across_ld(m):
    """the NaN columns 273 .. ld - 1 of dir_in are never read and ld moves no result"""
    lds = R.LDS_ALL if m == R.M_OTHER_LD else R.LDS_MAIN
    a = run(m, lds[0])
    for ld in lds[1:]:
        b = run(m, ld)
        what = f"(m={m}, ld={ld} vs ld={lds[0]}, {device_tag()})"
        assert np.array_equal(bits(a.dir_out), bits(b.dir_out)), f"dir_out differs {what}"
        assert torch.equal(a.dsave_raw, b.dsave_raw), f"dsave differs {what}"
        assert torch.equal(a.dump_raw, b.dump_raw), f"gradient dump differs {what}"
        assert np.array_equal(a.gin0[:m, :R.DIR_IN], b.gin0[:m, :R.DIR_IN]), f"g_dir_in differs {what}"
        assert np.array_equal(bits(a.tot), bits(b.tot)), f"weight gradients differ {what}"


@pytest.mark.parametrize("variant", R.MULTI_MASKS)
def test_weight_gradients_over_several_workgroups(variant):
    m = R.MULTI_M
    blocks, per = R.fold_rows(m)
    assert min(blocks) > 1 and min(per) >= 2 and m % 32 != 0, (blocks, per)
    r = run(m, R.LDS_MAIN[0], variant)
    forward_checks(r, variant)
    backward_checks(r, variant)
    tiles = set((np.flatnonzero((r.g != 0).any(1).numpy()) // 32).tolist())
    assert ((m - 1) // 32 in tiles) == (variant != "first-tiles")


def test_weight_gradients_at_the_full_width_of_the_launch():
    """m = 32 (6 200 + 3) - 5 = 38491: the cap of one workgroup per 6 tiles no longer binds, Dense_9 and Dense_10 get every
    workgroup they ask for (the trailing ones of Dense_9 own no tile) and the fold adds that many slabs; three evaluations
    of every tile carry an upstream gradient"""
    m = R.FULL_WIDTH_M
    blocks, per = R.fold_rows(m)
    assert blocks == R.fold_rows(4 * m)[0] and blocks[0] > R.fold_rows(R.MULTI_M)[0][0], blocks
    r = run(m, R.LDS_MAIN[0], "every-tile")
    forward_checks(r, "every-tile")
    backward_checks(r, "every-tile")


@pytest.mark.parametrize("m", R.SPLIT_MS)
def test_split_forward_against_the_exact_model(m):
    k = kernels()
    x, large = R.make_dir_in(m)
    outs = []
    for ld in R.LDS_MAIN:
        got, _ = k.forward(x, ld, split=True)
        ratio, worst = R.check_split(got, x, k.w, large, f"(lnrf_refnerf_dir_fwd_split, m={m}, ld={ld}, {device_tag()})")
        outs.append(got)
    print(f"[dir-stage] m={m:5d} split      dir_out  largest error-to-bound ratio {ratio:.5f}  largest error on the realistic rows "
          f"{worst:.2e}")
    assert np.array_equal(bits(outs[0]), bits(outs[1])), f"lnrf_refnerf_dir_fwd_split m={m}: dir_out differs between ld values"


def test_arguments():
    """m = 0 is LNRF_OK and writes nothing; a bad ld, a misaligned row pointer and null pointers are rejected with a negative
    code and a message before any launch: every buffer keeps its fill"""
    k = kernels()
    L, lib = k.L, k.lib
    m, ld = 5, 276
    dir_in = torch.full((m * 320 + 4,), 0.5, device="cuda")
    g_out = torch.full((m * 3,), 0.25, device="cuda")
    dsave = ff_bytes(lib.lnrf_refnerf_dir_save_bytes(m))
    scratch = ff_bytes(lib.lnrf_refnerf_dir_scratch_bytes(m))
    obuf, out = guarded(3 * m)
    ibuf, g_in = guarded(m * 320 + 4)
    wbuf, grads = guarded(k.n)
    P, P3 = L.ptr(k.packed, torch.uint8), L.ptr(k.packed3, torch.uint8)
    st = L.stream()

    def off4(t):
        return ctypes.c_void_p(t.data_ptr() + 4)

    def fwd(packed=P, x=L.ptr(dir_in), ld_=ld, m_=m, save=L.ptr(dsave, torch.uint8), o=L.ptr(out)):
        return lib.lnrf_refnerf_dir_fwd(packed, x, ld_, m_, save, o, st)

    def split(packed=P3, x=L.ptr(dir_in), ld_=ld, m_=m, o=L.ptr(out)):
        return lib.lnrf_refnerf_dir_fwd_split(packed, x, ld_, m_, o, st)

    def bwd(packed=P, save=L.ptr(dsave, torch.uint8), g=L.ptr(g_out), m_=m, sc=L.ptr(scratch, torch.uint8), gi=L.ptr(g_in), ld_=ld,
            gr=L.ptr(grads)):
        return lib.lnrf_refnerf_dir_bwd(packed, save, g, m_, sc, gi, ld_, gr, st)

    def untouched(what):
        torch.cuda.synchronize()
        assert (dsave == 0xFF).all() and (scratch == 0xFF).all(), f"{what}: dsave / scratch written"
        for buf in (obuf, ibuf, wbuf):
            assert (buf == SENTINEL).all(), f"{what}: an output was written"

    for name, fn in (("lnrf_refnerf_dir_fwd", fwd), ("lnrf_refnerf_dir_fwd_split", split), ("lnrf_refnerf_dir_bwd", bwd)):
        assert fn(m_=0) == 0, f"{name}: m = 0 must return LNRF_OK"
        untouched(f"{name} m=0")
    bad = [(f"{n} ld={v}", f, dict(ld_=v)) for n, f in (("dir_fwd", fwd), ("dir_fwd_split", split), ("dir_bwd", bwd))
           for v in (272, 275, 278)]
    bad += [("dir_fwd dir_in + 4 bytes", fwd, dict(x=off4(dir_in))), ("dir_fwd_split dir_in + 4 bytes", split, dict(x=off4(dir_in))),
            ("dir_bwd g_dir_in + 4 bytes", bwd, dict(gi=off4(g_in)))]
    bad += [(f"dir_fwd null {a}", fwd, {a: None}) for a in ("packed", "x", "save", "o")]
    bad += [(f"dir_fwd_split null {a}", split, {a: None}) for a in ("packed", "x", "o")]
    bad += [(f"dir_bwd null {a}", bwd, {a: None}) for a in ("packed", "save", "g", "sc", "gi", "gr")]
    bad += [("dir_fwd m=-1", fwd, dict(m_=-1)), ("dir_bwd m=-1", bwd, dict(m_=-1))]
    for what, fn, kw in bad:
        rc = fn(**kw)
        msg = lib.lnrf_last_error()
        assert rc < 0 and msg, f"lnrf_refnerf_{what}: returned {rc}, message {msg!r}"
        untouched(f"lnrf_refnerf_{what}")
    # and the same buffers are accepted once the argument is right (the rejections above were about the argument)
    assert fwd() == 0 and split() == 0
    torch.cuda.synchronize()

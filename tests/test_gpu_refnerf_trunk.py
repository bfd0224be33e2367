"""
The fused Ref-NeRF trunk (csrc/refnerf_fused.hip: Dense_0..8), its normal pass and their two backwards through the C ABI,
stage by stage in float64: lnrf_refnerf_trunk_fwd, lnrf_refnerf_normal_pass, lnrf_refnerf_trunk_bwd, lnrf_refnerf_normal_bwd,
lnrf_refnerf_trunk_bwd_scratch_bytes.

The forward leaves x_emb, h0..h7 and the ReLU masks in the save (NeRFModel's save layout), the normal pass its chain states
c_8..c_0 in cdump and the first-order backward dy8..dy0 in the front of its scratch (both the gradient-dump layout), the
second-order backward ubar_e and tbar_0..7 in its scratch (the save layout again).  nerf_dump_decode.py reads all four, so
every stage is recomputed from the KERNEL'S OWN decoded operands by refnerf_trunk_reference.py (rules and derivations there;
test_refnerf_trunk_reference_cpu.py shows that a correct implementation passes them and that each mutation is rejected).

Every call: 0xFF-filled blob, save, cdump and scratches; spatial_out, n_raw and the gradient vector are views inside
sentinel-filled buffers; g_spatial has NaN in columns 256 .. ld - 1.  Three calls of each backward (into zeros -> tot, into a
random prefill P -> fp32(P + tot) bit for bit, once more on top); lnrf_refnerf_trunk_bwd leaves Dense_9.. bit-untouched,
lnrf_refnerf_normal_bwd every bias word too; the dumps are identical between calls; everything is bit-identical across ld.

Sizes: m in {1, 31, 33, 1000, 2053} x ld in {256, 276}; the first-order backward once more at the pipeline edges of the
layer-stationary kernel (33, 32P-5, 32(P+8)-31, 96P+1, P = pipelines of the device); the weight gradients of both production
lists over several workgroups at the two sizes refnerf_trunk_reference.multi_sizes() derives from the lists, with an upstream
that is non-zero on few evaluations per tile.  Figures measured on an MI355X are recorded in DESIGN.md (Ref-NeRF path); they
are not gates.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nerf_dump_decode as D
import refnerf_trunk_reference as T
from test_gpu_nerf_backward_edges import SIZES, device_tag, pipelines

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel words on either side of every output (256 bytes: the views stay 16-byte aligned)
SENTINEL = T.SENTINEL
EXTRA_ROWS = 2  # sentinel rows behind row m - 1 of spatial_out and n_raw
HID = T.HID


def guarded(n):
    """-> (int32 buffer of sentinels, fp32 view of the n words between the guards — sentinels too until written)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def assert_guards(buf, n, what):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all(), f"{what}: words outside the output were written"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def raw_words(view):
    return view.view(torch.int32).cpu().numpy().view(np.uint32)


def ff_bytes(n):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")


def strided_nan(g, ld):
    out = torch.full((g.shape[0], ld), float("nan"), dtype=torch.float32)
    out[:, :g.shape[1]] = g
    return out


class Kernels:
    def __init__(self):
        from learn_nerf import _lib as L
        self.L, self.lib = L, L.lib()
        self.shape = L.NerfShape(5, 4, 256, 128, 10, 4)  # the trunk's buffers have NeRFModel's layout
        self.flat_cpu = T.params()
        self.flat = self.flat_cpu.cuda()
        self.w = T.weights()
        self.n = self.flat.numel()
        self.packed = ff_bytes(self.lib.lnrf_refnerf_trunk_packed_bytes())
        L.check(self.lib.lnrf_refnerf_trunk_pack(L.ptr(self.flat), L.ptr(self.packed, torch.uint8), L.stream()), "trunk_pack")
        torch.cuda.synchronize()

    def P(self):
        return self.L.ptr(self.packed, torch.uint8)

    def save_bytes(self, m):
        return self.lib.lnrf_nerf_save_bytes(ctypes.byref(self.shape), m)

    def cdump_bytes(self, m):
        return self.lib.lnrf_nerf_bwd_scratch_bytes(ctypes.byref(self.shape), m)

    def forward(self, x, ld):
        """-> save (GPU uint8), raw words of spatial_out [m + EXTRA_ROWS, ld]"""
        L, lib = self.L, self.lib
        m = x.shape[0]
        save = ff_bytes(self.save_bytes(m))
        n = (m + EXTRA_ROWS) * ld
        obuf, out = guarded(n)
        xg = x.cuda()
        L.check(lib.lnrf_refnerf_trunk_fwd(self.P(), L.ptr(xg), m, L.ptr(save, torch.uint8), L.ptr(out), ld, L.stream()),
                "lnrf_refnerf_trunk_fwd")
        torch.cuda.synchronize()
        assert_guards(obuf, n, f"lnrf_refnerf_trunk_fwd m={m} ld={ld} {device_tag()} spatial_out")
        return save, raw_words(out).reshape(m + EXTRA_ROWS, ld)

    def normal_pass(self, save, x):
        """-> cdump (GPU uint8, dump + slab region), raw words of n_raw [m + EXTRA_ROWS, 3]"""
        L, lib = self.L, self.lib
        m = x.shape[0]
        cdump = ff_bytes(self.cdump_bytes(m))
        n = (m + EXTRA_ROWS) * 3
        nbuf, nraw = guarded(n)
        xg = x.cuda()
        L.check(lib.lnrf_refnerf_normal_pass(self.P(), L.ptr(save, torch.uint8), L.ptr(xg), m, L.ptr(cdump, torch.uint8), L.ptr(nraw),
                                             L.stream()), "lnrf_refnerf_normal_pass")
        torch.cuda.synchronize()
        assert_guards(nbuf, n, f"lnrf_refnerf_normal_pass m={m} {device_tag()} n_raw")
        return cdump, raw_words(nraw).reshape(m + EXTRA_ROWS, 3)

    def _grads(self, grads_in):
        wbuf, grads = guarded(self.n)
        grads.copy_(torch.from_numpy(np.ascontiguousarray(grads_in, dtype=np.float32)).cuda())
        return wbuf, grads

    def trunk_bwd(self, save, g, ld, grads_in):
        """-> gradient vector (numpy), the first-order dump (CPU uint8), the LS status word"""
        L, lib = self.L, self.lib
        m = g.shape[0]
        nbytes = lib.lnrf_refnerf_trunk_bwd_scratch_bytes(m)
        assert nbytes == lib.lnrf_nerf_bwd_ls_scratch_bytes(ctypes.byref(self.shape), m)
        scratch = ff_bytes(nbytes)
        wbuf, grads = self._grads(grads_in)
        gd = strided_nan(g, ld).cuda()
        L.check(lib.lnrf_refnerf_trunk_bwd(self.P(), L.ptr(save, torch.uint8), L.ptr(gd), ld, m, L.ptr(scratch, torch.uint8),
                                           L.ptr(grads), L.stream()), "lnrf_refnerf_trunk_bwd")
        torch.cuda.synchronize()
        assert_guards(wbuf, self.n, f"lnrf_refnerf_trunk_bwd m={m} ld={ld} {device_tag()} grads")
        off = lib.lnrf_nerf_bwd_ls_status_offset(ctypes.byref(self.shape), m)
        status = int(scratch[off:off + 4].cpu().numpy().view(np.uint32)[0])
        return grads.cpu().numpy(), scratch[:D.grad_dump_bytes(m)].cpu(), status

    def normal_bwd(self, save, cdump, x, u, grads_in):
        """-> gradient vector (numpy), the tangent dump (CPU uint8)"""
        L, lib = self.L, self.lib
        m = x.shape[0]
        scratch = ff_bytes(self.save_bytes(m))
        wbuf, grads = self._grads(grads_in)
        xg, ug = x.cuda(), u.cuda()
        L.check(lib.lnrf_refnerf_normal_bwd(self.P(), L.ptr(save, torch.uint8), L.ptr(cdump, torch.uint8), L.ptr(xg), L.ptr(ug), m,
                                            L.ptr(scratch, torch.uint8), L.ptr(grads), L.stream()), "lnrf_refnerf_normal_bwd")
        torch.cuda.synchronize()
        assert_guards(wbuf, self.n, f"lnrf_refnerf_normal_bwd m={m} {device_tag()} grads")
        return grads.cpu().numpy(), scratch.cpu()


@functools.lru_cache(maxsize=None)
def kernels():
    return Kernels()


class Run:
    pass


def _np_list(ts):
    return [t.numpy() for t in ts]


@functools.lru_cache(maxsize=None)
def run(m, ld, variant=None):
    """forward, normal pass, three calls of each backward and their decoded dumps for one size; computed once and shared,
    unchanged, by the tests"""
    k = kernels()
    r = Run()
    r.m, r.ld, r.k, r.variant = m, ld, k, variant
    r.x = T.make_x(m)
    r.g, r.u = T.make_upstream(m, None if variant is None else T.keep_mask(variant, m))
    save, r.spatial_raw = k.forward(r.x, ld)
    r.save_raw = save.cpu()
    cdump, r.nraw_raw = k.normal_pass(save, r.x)
    nd = D.grad_dump_bytes(m)
    r.cdump_raw = cdump[:nd].cpu()
    rng = np.random.default_rng(m + ld)
    r.prefill = rng.standard_normal(k.n).astype(np.float32)
    zeros = np.zeros(k.n, np.float32)
    r.tot1, r.dump1, r.status = k.trunk_bwd(save, r.g, ld, zeros)
    r.g1a, r.dump1a, st_a = k.trunk_bwd(save, r.g, ld, r.prefill)
    r.g1b, r.dump1b, st_b = k.trunk_bwd(save, r.g, ld, r.g1a)
    r.statuses = (r.status, st_a, st_b)
    r.tot2, r.tdump = k.normal_bwd(save, cdump, r.x, r.u, zeros)
    r.g2a, r.tdump_a = k.normal_bwd(save, cdump, r.x, r.u, r.prefill)
    r.g2b, r.tdump_b = k.normal_bwd(save, cdump, r.x, r.u, r.g2a)
    r.cdump_after = cdump[:nd].cpu()
    r.save_after = save.cpu()
    r.save = D.decode_save(r.save_raw, m)
    r.cd = D.decode_grad(r.cdump_raw, m)
    r.gd = D.decode_grad(r.dump1, m)
    r.td = D.decode_save(r.tdump, m, hidden_masks=False)
    r.res = {"x_emb": r.save["x_emb"].numpy(), "h": _np_list(r.save["h"]), "mask": _np_list(r.save["mask"]),
             "spatial_out": r.spatial_raw[:m, :HID].view(np.float32).astype(np.float64),
             "c": _np_list(r.cd["dy"]), "n_raw": r.nraw_raw[:m].view(np.float32).astype(np.float64),
             "dy": _np_list(r.gd["dy"]), "ubar": r.td["x_emb"].numpy(), "tbar": _np_list(r.td["h"])}
    return r


def tag(entry, r):
    return f"({entry}, m={r.m}, ld={r.ld}, {r.variant}, {device_tag()})"


def show(r, stats):
    for stage, v in stats.items():
        if isinstance(v, dict):
            print(f"[trunk-stage] m={r.m:5d} ld={r.ld} {r.variant or '-':11s} {stage:11s} allowance share {v['allow']:.3e}  mismatch share "
                  f"{v['diff']:.3e}  CPU fp32 flip share {v['cpu']:.3e}  largest needed part of delta {v['need']:.2e}")
        else:
            print(f"[trunk-stage] m={r.m:5d} ld={r.ld} {r.variant or '-':11s} {stage:11s} largest error-to-bound ratio {v:.4f}")


def unowned_slots_keep_their_fill(raw, what):
    """z, d_emb, h10 and mask10 of a buffer in the save layout: every byte still 0xFF"""
    lay, _ = D.layouts()
    blocks = raw.numpy().reshape(-1, lay.n_slots, lay.frag_bytes)
    slots = [lay.tensors[n].slot0 + i for n in ("z", "d_emb", "h10") for i in range(lay.tensors[n].nks)] + [lay.masks["mask10"].slot]
    for s in slots:
        assert (blocks[:, s] == 0xFF).all(), f"{what}: slot {s} (not the trunk's) was written"


def forward_checks(r):
    what = tag("lnrf_refnerf_trunk_fwd", r)
    m, ld, s = r.m, r.ld, r.save
    assert (r.spatial_raw[m:] == SENTINEL).all(), f"spatial_out {what}: rows from {m} on were written"
    assert (r.spatial_raw[:m, HID:] == SENTINEL).all(), f"spatial_out {what}: columns from 256 on were written"
    assert np.isfinite(r.res["spatial_out"]).all(), f"spatial_out {what}: not finite (an unwritten word?)"
    stats = T.check_forward(r.res, r.x, r.k.w, what)
    assert not s["pad_slots"]["x_emb"].numpy().any(), f"x_emb {what}: its unused k-slots are not zero"
    for name in ["x_emb"] + [f"h{l}" for l in range(8)]:
        assert np.isfinite(s["pad"][name].numpy()).all(), f"{name} {what}: pad evaluations are not finite"
    for l in range(8):
        assert (s["pad"][f"mask{l}"].numpy() == (s["pad"][f"h{l}"].numpy() > 0)).all(), f"mask{l} {what}: pad evaluations"
    unowned_slots_keep_their_fill(r.save_raw, f"save {what}")
    assert torch.equal(r.save_raw, r.save_after), f"{what}: a later call wrote into the save"
    show(r, stats)


def normal_checks(r):
    what = tag("lnrf_refnerf_normal_pass", r)
    m = r.m
    assert (r.nraw_raw[m:] == SENTINEL).all(), f"n_raw {what}: rows from {m} on were written"
    stats = T.check_normal(r.res, r.x, r.k.w, what)
    for l in range(9):
        v = r.cd["pad"][f"dy{l}"].numpy()
        assert not v.any(), f"c_{l} {what}: the pad evaluations {m}.. hold {int((v != 0).sum())} non-zero values"
    assert torch.equal(r.cdump_raw, r.cdump_after), f"{what}: lnrf_refnerf_normal_bwd changed the chain-state dump"
    show(r, stats)
    by_f = T.n_raw_by_frequency(r.res["n_raw"], r.x, r.res["c"][0], r.res["c"][5], r.k.w)
    print(f"[trunk-stage] m={m:5d} ld={r.ld} {r.variant or '-':11s} n_raw error over the bound's share of frequency 0..9: " +
          " ".join(f"{v:.3f}" for v in by_f))


def accumulation_checks(what, k, tot, g_a, g_b, prefill, untouched):
    """the call into zeros left `tot`; the later calls add it bit for bit; the words of `untouched` (bool mask) never move"""
    assert np.isfinite(tot).all(), f"{what}: non-finite gradient (a word of a 0xFF scratch was folded?)"
    assert not bits(tot)[untouched].any(), f"{what}: words outside the kernel's ranges were written (call into zeros)"
    for name, got, base in (("prefilled", g_a, prefill), ("second", g_b, g_a)):
        assert np.array_equal(bits(got)[untouched], bits(base)[untouched]), f"{what}: the {name} call changed words it does not own"
        diff = np.flatnonzero(bits(got) != bits(base + tot))
        assert diff.size == 0, (f"{what}: the {name} call did not add the vector of the first call bit for bit at {diff.size} "
                                f"entries, first {diff[:8]}")


def trunk_bwd_checks(r):
    what = tag("lnrf_refnerf_trunk_bwd", r)
    k = r.k
    assert r.statuses == (0, 0, 0), f"LS status words {r.statuses} {what}"
    stats = T.check_trunk_bwd(dict(r.res, grads=r.tot1), strided_nan(r.g, r.ld), k.w, what)
    for l in range(9):
        v = r.gd["pad"][f"dy{l}"].numpy()
        assert not v.any(), f"dy{l} {what}: the pad evaluations {r.m}.. hold {int((v != 0).sum())} non-zero gradients"
    untouched = np.zeros(k.n, bool)
    untouched[k.w.end:] = True
    accumulation_checks(what, k, r.tot1, r.g1a, r.g1b, r.prefill, untouched)
    for other in (r.dump1a, r.dump1b):
        assert torch.equal(r.dump1, other), f"{what}: the gradient dump differs between two calls on the same inputs"
    if T.n_active_of(r.g):
        assert np.abs(r.tot1[:k.w.end]).max() > 0
    show(r, {f"1:{k_}": v for k_, v in stats.items()})


def normal_bwd_checks(r):
    what = tag("lnrf_refnerf_normal_bwd", r)
    k, td = r.k, r.td
    stats = T.check_normal_bwd(dict(r.res, grads=r.tot2), r.x, r.u, k.w, what)
    assert not td["pad_slots"]["x_emb"].numpy().any(), f"ubar_e {what}: its unused k-slots are not zero"
    for name in ["x_emb"] + [f"h{l}" for l in range(8)]:
        v = td["pad"][name].numpy()
        assert not v.any(), f"tangent dump {name} {what}: the pad evaluations {r.m}.. hold non-zero values"
    unowned_slots_keep_their_fill(r.tdump, f"tangent dump {what}")
    untouched = np.ones(k.n, bool)
    for wo, bo, fi, fo in k.w.offs:
        untouched[wo:bo] = False
    accumulation_checks(what, k, r.tot2, r.g2a, r.g2b, r.prefill, untouched)
    for other in (r.tdump_a, r.tdump_b):
        assert torch.equal(r.tdump, other), f"{what}: the tangent dump differs between two calls on the same inputs"
    if T.n_active_of(r.u):
        assert np.abs(r.tot2).max() > 0
    show(r, {f"2:{k_}": v for k_, v in stats.items()})


CASES = [(m, ld) for m in T.MS for ld in T.LDS]


@pytest.mark.parametrize("m,ld", CASES)
def test_forward_stage_by_stage(m, ld):
    forward_checks(run(m, ld))


@pytest.mark.parametrize("m,ld", CASES)
def test_normal_pass_stage_by_stage(m, ld):
    normal_checks(run(m, ld))


@pytest.mark.parametrize("m,ld", CASES)
def test_trunk_backward_stage_by_stage(m, ld):
    trunk_bwd_checks(run(m, ld))


@pytest.mark.parametrize("m,ld", CASES)
def test_normal_backward_stage_by_stage(m, ld):
    normal_bwd_checks(run(m, ld))


@pytest.mark.parametrize("m", T.MS)
def test_bit_identical_across_ld(m):
    """ld moves no result and the NaN columns 256 .. ld - 1 of g_spatial are never read"""
    a, b = run(m, T.LDS[0]), run(m, T.LDS[1])
    what = f"(m={m}, ld={b.ld} vs ld={a.ld}, {device_tag()})"
    assert np.array_equal(a.spatial_raw[:m, :HID], b.spatial_raw[:m, :HID]), f"spatial_out differs {what}"
    assert np.array_equal(a.nraw_raw, b.nraw_raw), f"n_raw differs {what}"
    for name in ("save_raw", "cdump_raw", "dump1", "tdump"):
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{name} differs {what}"
    assert np.array_equal(bits(a.tot1), bits(b.tot1)) and np.array_equal(bits(a.tot2), bits(b.tot2)), f"weight gradients differ {what}"


@pytest.mark.parametrize("size", T.LS_SIZES)
def test_trunk_backward_at_the_pipeline_edges(size):
    """the layer-stationary pipeline behind lnrf_refnerf_trunk_bwd at the tile counts where a pipeline gets no tile, one, two and
    one, four and three (test_gpu_nerf_backward_edges.py)"""
    m = SIZES[size](pipelines())
    assert m <= T.MAX_ACTIVE
    r = run(m, T.LDS[1])
    trunk_bwd_checks(r)
    forward_checks(r)


@pytest.mark.parametrize("variant", T.MULTI_MASKS)
def test_weight_gradients_over_several_workgroups(variant):
    m, _ = T.multi_sizes()
    for which in (T.LIST_TRUNK, T.LIST_NORMAL):
        blocks, per = T.fold_blocks(which, m)
        assert min(blocks) >= 2 and min(per) >= 2 and m % 32 != 0, (blocks, per)
    r = run(m, T.LDS[1], variant)
    forward_checks(r)
    normal_checks(r)
    trunk_bwd_checks(r)
    normal_bwd_checks(r)
    tiles = set((np.flatnonzero((r.u != 0).any(1).numpy()) // 32).tolist())
    assert ((m - 1) // 32 in tiles) == (variant != "first-tiles")


def test_weight_gradients_at_the_full_width_of_the_launch():
    """the smallest m = 32 k - 5 at which the cap of one workgroup per 6 tiles no longer binds for the 28-workgroup hidden
    problems of lnrf_refnerf_normal_bwd; a few evaluations of every tile carry an upstream gradient"""
    _, m = T.multi_sizes()
    assert T.fold_blocks(T.LIST_NORMAL, m)[0][:8] == [28] * 8
    r = run(m, T.LDS[1], "every-tile")
    forward_checks(r)
    normal_checks(r)
    trunk_bwd_checks(r)
    normal_bwd_checks(r)


def test_arguments():
    """m = 0 is LNRF_OK and writes nothing; a bad ld, a misaligned row pointer, null pointers and m = -1 are rejected with a
    negative code and a message before any launch: every buffer keeps its fill"""
    k = kernels()
    L, lib = k.L, k.lib
    m, ld = 5, 276
    x = torch.full((m * 3,), 0.5, device="cuda")
    u = torch.full((m * 3,), 0.25, device="cuda")
    g = torch.full((m * 320 + 4,), 0.25, device="cuda")
    save, cdump = ff_bytes(k.save_bytes(m)), ff_bytes(k.cdump_bytes(m))
    scratch, tscratch = ff_bytes(lib.lnrf_refnerf_trunk_bwd_scratch_bytes(m)), ff_bytes(k.save_bytes(m))
    obuf, out = guarded(m * 320 + 4)
    nbuf, nraw = guarded(m * 3)
    wbuf, grads = guarded(k.n)
    u8 = lambda t: L.ptr(t, torch.uint8)
    st = L.stream()

    def off4(t):
        return ctypes.c_void_p(t.data_ptr() + 4)

    def fwd(packed=k.P(), x_=L.ptr(x), m_=m, save_=u8(save), o=L.ptr(out), ld_=ld):
        return lib.lnrf_refnerf_trunk_fwd(packed, x_, m_, save_, o, ld_, st)

    def nrm(packed=k.P(), save_=u8(save), x_=L.ptr(x), m_=m, cd=u8(cdump), o=L.ptr(nraw)):
        return lib.lnrf_refnerf_normal_pass(packed, save_, x_, m_, cd, o, st)

    def bwd(packed=k.P(), save_=u8(save), g_=L.ptr(g), ld_=ld, m_=m, sc=u8(scratch), gr=L.ptr(grads)):
        return lib.lnrf_refnerf_trunk_bwd(packed, save_, g_, ld_, m_, sc, gr, st)

    def nbw(packed=k.P(), save_=u8(save), cd=u8(cdump), x_=L.ptr(x), u_=L.ptr(u), m_=m, sc=u8(tscratch), gr=L.ptr(grads)):
        return lib.lnrf_refnerf_normal_bwd(packed, save_, cd, x_, u_, m_, sc, gr, st)

    def untouched(what):
        torch.cuda.synchronize()
        for name, t in (("save", save), ("cdump", cdump), ("scratch", scratch), ("tangent scratch", tscratch)):
            assert (t == 0xFF).all(), f"{what}: {name} written"
        for buf in (obuf, nbuf, wbuf):
            assert (buf == SENTINEL).all(), f"{what}: an output was written"

    fns = (("trunk_fwd", fwd), ("normal_pass", nrm), ("trunk_bwd", bwd), ("normal_bwd", nbw))
    for name, fn in fns:
        assert fn(m_=0) == 0, f"lnrf_refnerf_{name}: m = 0 must return LNRF_OK"
        untouched(f"lnrf_refnerf_{name} m=0")
    bad = [(f"{n} ld={v}", f, dict(ld_=v)) for n, f in (("trunk_fwd", fwd), ("trunk_bwd", bwd)) for v in (252, 255, 258)]
    bad += [("trunk_fwd spatial_out + 4 bytes", fwd, dict(o=off4(out))), ("trunk_bwd g_spatial + 4 bytes", bwd, dict(g_=off4(g)))]
    bad += [(f"trunk_fwd null {a}", fwd, {a: None}) for a in ("packed", "x_", "save_", "o")]
    bad += [(f"normal_pass null {a}", nrm, {a: None}) for a in ("packed", "save_", "x_", "cd", "o")]
    bad += [(f"trunk_bwd null {a}", bwd, {a: None}) for a in ("packed", "save_", "g_", "sc", "gr")]
    bad += [(f"normal_bwd null {a}", nbw, {a: None}) for a in ("packed", "save_", "cd", "x_", "u_", "sc", "gr")]
    bad += [(f"{n} m=-1", f, dict(m_=-1)) for n, f in fns]
    for what, fn, kw in bad:
        rc = fn(**kw)
        msg = lib.lnrf_last_error()
        assert rc < 0 and msg, f"lnrf_refnerf_{what}: returned {rc}, message {msg!r}"
        untouched(f"lnrf_refnerf_{what}")
    assert lib.lnrf_refnerf_trunk_bwd_scratch_bytes(-1) == -1
    # and the same buffers are accepted once the argument is right (the rejections above were about the argument)
    assert fwd() == 0 and nrm() == 0
    torch.cuda.synchronize()

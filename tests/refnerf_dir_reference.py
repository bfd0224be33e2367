"""
Float64 reference of RefNERFModel's directional block (ref_nerf.py:100-107: Dense_9 273 -> 128 relu, Dense_10 128 -> 3), stage
by stage, for lnrf_refnerf_dir_fwd / _dir_bwd / _dir_fwd_split (csrc/refnerf_fused.hip).  A plain module: importing it
collects nothing.  Shared by test_refnerf_dir_reference_cpu.py (the rules on a CPU fp32 emulation and on its mutations) and
test_gpu_refnerf_dir.py (the same rules on the kernels), so both run exactly the same inputs, sizes and bounds.

Every stage function takes the operands the kernel saw (decoded from its own dumps) and returns
(float64 reference, the same contraction with absolute values, the torch.float32 result of the same operands):

  xin       bf16_rne(dir_in[:, :273])                       bit-equal
  h9        relu(xin bf16(W9) + b9), K = 288 (15 pad rows)  check_rounded(relu) + cap
  dir_out   h9 bf16(W10) + b10, K = 128                     check_accumulated
  dy10      bf16_rne(g_dir_out)                             bit-equal
  dy9       mask9 o (dy10 bf16(W10)^T), K = 16              check_rounded + cap, masked-off exactly 0
  g_dir_in  dy9 bf16(W9)^T, K = 128                         check_accumulated; columns 273 .. min(ld, 288) - 1 exactly 0
  dW9 = xin^T dy9, db9 = sum dy9, dW10 = h9^T dy10, db10 = sum dy10
                                                            check_accumulated, n_add = evaluations with a non-zero upstream
                                                            gradient + the slabs the fold adds (lnrf_host_wgrad_list)

The split path (lnrf_refnerf_dir_fwd_split) against the EXACT float64 model of the fp32 operands.  Its bound, derived from
the arithmetic of split_store / acc_to_frag_split / chain_layer_split (fused_chain.h), not measured:

  * every fp32 operand v is carried as hi = bf16(v), lo = bf16(v - hi); v - hi is exact in fp32, so |v - hi - lo| <=
    2^-9 |v - hi| <= 2^-18 |v|.  The bound uses the coarser E = 2^-16 per operand.
  * a product is formed as w_lo x_hi + w_hi x_lo + w_hi x_hi = (w_hi + w_lo)(x_hi + x_lo) - w_lo x_lo.  The first term is
    w x (1 + a)(1 + b), |a|, |b| <= E; the dropped w_lo x_lo is at most 2^-9 |w| 2^-9 |x|.  Per product:
    |w||x| (2 E + E^2 + 2^-18) =: |w||x| P.
  * the three bf16 products of a k-step are exact in fp32 and go into ONE fp32 accumulator that starts from the bias: 3 x 18
    k-steps of 16 = 864 terms in layer 1, 3 x 8 x 16 = 384 in layer 2, each at most (1 + 2^-8)^2 |w||x|:
    (K + 2) 2^-23 ((1 + 2^-8)^2 S + |b|), S = sum |w||x|, as dot_delta.
  * layer 1:  e1 = P S1 + 866 2^-23 (1.01 S1 + |b9|), S1 = |x| |W9|;  the ReLU is 1-Lipschitz, so |h - h_exact| <= e1.
  * layer 2 splits the fp32 h again and contracts it with W10:  |out - out_exact| <= e1 |W10| (layer 1's error carried
    through) + P S2 + 386 2^-23 (1.01 S2 + |b10|), S2 = (|h_exact| + e1) |W10|.

emulate_split() repeats that arithmetic in torch.float32 on the CPU; it must stay inside the bound (CPU test).
"""
import ctypes

import numpy as np
import torch

import nerf_dump_decode as D

DIR_IN, HID = D.DIR_IN, D.DIR_HIDDEN
K9 = 16 * (-(-DIR_IN // 16))  # 288: the 18 k-steps of Dense_9, 15 zero rows included
K10, K10T, K9T = HID, 16, HID  # Dense_10; Dense_10^T (one k-step, 3 real k-slots); Dense_9^T

MS = [1, 31, 33, 1000, 2053]
LDS_ALL = [276, 280, 292, 320]
LDS_MAIN = [276, 292]
M_OTHER_LD = 33
SPLIT_MS = [1, 33, 2053]
MAX_ACTIVE = 4000
MULTI_M = 32 * (2 * 200 + 3) - 5
MULTI_MASKS = ["first-tiles", "last-tiles", "every-tile"]
# At MULTI_M the launch caps both problems at one workgroup per 6 tiles (nerf_wgrad.h).  The smallest size of the same form
# at which Dense_9 gets every workgroup it asks for, so that the fold runs over the full width of the launch:
FULL_WIDTH_M = 32 * (6 * 200 + 3) - 5
WRITTEN_COLS = 288  # lnrf.h: g_dir_in columns 273 .. min(ld, 288) - 1 receive 0, nothing at or beyond 288 is touched


def host():
    lib = D.load_host_lib()
    lib.lnrf_host_wgrad_list.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    return lib


def offsets():
    """(W9, B9, W10, B10, parameter count) of a RefNERFModel vector of default widths, from the host layout library"""
    lib = host()
    w9, b9, w10, b10 = (lib.lnrf_host_wgrad_const(i) for i in (4, 5, 6, 7))
    assert b9 - w9 == DIR_IN * HID and w10 - b9 == HID and b10 - w10 == HID * 3
    return w9, b9, w10, b10, b10 + 3


def fold_rows(m):
    """slabs the fold of lnrf_refnerf_dir_bwd's weight-gradient launch adds per problem (Dense_9, Dense_10), and the tiles a
    workgroup of each owns, from the production problem list"""
    lib = host()
    n_tiles = D.padded_tiles(m)
    out = np.zeros(6 * 13, np.int32)
    assert lib.lnrf_host_wgrad_list(4, n_tiles, out.ctypes.data) == 2
    blocks = [int(out[1]), int(out[7])]
    return blocks, [-(-n_tiles // b) for b in blocks]


# ---- parameters and inputs ------------------------------------------------------------------------------------------------
def make_params(seed=7):
    """A full RefNERFModel vector: Dense_9 / Dense_10 dense N(0, 1 / sqrt(fan_in)) with random non-zero biases, everything
    else random, so that a pack walk that reads the wrong region shows"""
    w9, b9, w10, b10, n = offsets()
    gen = torch.Generator().manual_seed(seed)
    flat = torch.randn(n, generator=gen) * 0.3
    flat[w9:b9] = torch.randn(DIR_IN * HID, generator=gen) / DIR_IN ** 0.5
    flat[b9:w10] = torch.randn(HID, generator=gen) * 0.1 + 0.01
    flat[w10:b10] = torch.randn(HID * 3, generator=gen) / HID ** 0.5
    flat[b10:n] = torch.tensor([0.3, -0.2, 0.1])
    return flat.float().contiguous()


class Weights:
    """Dense_9 / Dense_10 of a vector: fp32 as float64 (the split path's operands), bf16 as float64 and as fp32 (the bf16
    path's operand and the CPU fp32 product), fp32 biases"""

    def __init__(self, flat):
        w9, b9, w10, b10, n = offsets()
        f = flat.detach().cpu().float()
        assert f.numel() == n
        self.w9_32, self.w10_32 = f[w9:b9].view(DIR_IN, HID), f[w10:b10].view(HID, 3)
        self.b9_32, self.b10_32 = f[b9:w10].clone(), f[b10:n].clone()
        self.w9, self.w10 = self.w9_32.bfloat16().double().numpy(), self.w10_32.bfloat16().double().numpy()
        self.w9_f, self.w10_f = self.w9_32.bfloat16().float(), self.w10_32.bfloat16().float()
        self.b9, self.b10 = self.b9_32.double().numpy(), self.b10_32.double().numpy()


def tie(n, e=0, sign=1.0):
    """exactly midway between the bf16 numbers (128 + n) 2^(e-7) and (128 + n + 1) 2^(e-7): the lower neighbour is even
    iff n is even, so round-to-nearest-even goes down for even n and up for odd n"""
    return sign * (128 + n + 0.5) / 128 * 2.0 ** e


def edge_rows(gen):
    """the edge rows of dir_in [8, 273]"""
    rows = realistic_rows(8, gen)
    t = rows[0]  # ties with an even and with an odd lower neighbour, both signs, the scalar-tail feature and its neighbour
    t[0], t[1], t[2], t[3] = tie(0), tie(1), tie(2, -3, -1.0), tie(3, -3, -1.0)
    t[4], t[5], t[255], t[256] = tie(126, 2), tie(127, 2), tie(77, -1), tie(78, -1)
    t[270], t[271], t[272] = tie(5, -2, -1.0), tie(10, -1), tie(11, -1, -1.0)
    rows[1] = 0.0
    rows[1, 1::2] = -0.0
    sgn = torch.where(torch.rand(DIR_IN, generator=gen) < 0.5, -1.0, 1.0)
    mag = 1.0 + torch.rand(DIR_IN, generator=gen)
    rows[2] = 1e4 * sgn * mag
    rows[3] = 1e-4 * sgn * mag
    rows[4] = 0.0
    rows[4, 272] = -0.8125
    rows[5] = 0.0
    rows[5, 271] = 0.71875
    rows[6] = 0.0  # the scalar tail and its neighbour apart from everything else, not bf16 numbers
    rows[6, 272], rows[6, 256] = 0.3331, -0.9173
    rows[7, 256:] = 0.0  # the trunk columns alone
    return rows


N_LARGE_ROWS = (2,)  # edge rows of magnitude 1e4: outside the model-level absolute gate of the split path


def realistic_rows(m, gen):
    """[spatial_out (256) ~ N(0, 1) | IDE (16) and -d.n in [-1, 1]]"""
    x = torch.randn(m, DIR_IN, generator=gen)
    x[:, 256:] = torch.rand(m, DIR_IN - 256, generator=gen) * 2 - 1
    return x


def make_dir_in(m):
    """dir_in[m, 273] fp32 (the same for every ld): realistic rows, the edge rows at the front and, from m = 64 on, once
    more at the end (the ragged last tile).  -> (values, indices of the 1e4-magnitude rows)"""
    gen = torch.Generator().manual_seed(1000 + m)
    x = realistic_rows(m, gen)
    e = edge_rows(gen)
    n = min(m, e.shape[0])
    x[:n] = e[:n]
    large = [i for i in N_LARGE_ROWS if i < n]
    if m >= 64:
        x[m - e.shape[0]:] = e
        large += [m - e.shape[0] + i for i in N_LARGE_ROWS]
    x = x.float().contiguous()
    assert torch.isfinite(x).all() and ((x == 0) | (x.abs() > 1e-30)).all()  # normal numbers only
    return x, large


def strided(x, ld, fill=float("nan")):
    """x[m, 273] inside rows of ld floats; columns 273 .. ld - 1 hold `fill`"""
    out = torch.full((x.shape[0], ld), fill, dtype=torch.float32)
    out[:, :x.shape[1]] = x
    return out


def make_g_dir_out(m, keep=None):
    """upstream gradient [m, 3]; zero outside `keep`"""
    gen = torch.Generator().manual_seed(2000 + m)
    g = torch.randn(m, 3, generator=gen).float()
    if m > 2:
        g[1, 1] = 0.0
        g[2] = torch.tensor([tie(1), -tie(2), tie(4, -5)])
    if keep is not None:
        g = g * torch.from_numpy(np.asarray(keep)).float()[:, None]
    return g.contiguous()


def multi_mask(variant, m):
    """which evaluations carry an upstream gradient at the multi-workgroup sizes (at most MAX_ACTIVE): the first / the last
    tile of every workgroup's range of either weight-gradient problem (the ragged last tile with the last ones), or seven
    evaluations of every tile (fewer where seven per tile would exceed MAX_ACTIVE)"""
    _, per = fold_rows(m)
    ev = np.arange(m)
    t = ev // 32
    last_tile = (m - 1) // 32
    if variant == "first-tiles":
        keep = ((t % per[0] == 0) | (t % per[1] == 0)) & (t != last_tile)
    elif variant == "last-tiles":
        keep = (t % per[0] == per[0] - 1) | (t % per[1] == per[1] - 1) | (t == last_tile)
    else:
        assert variant == "every-tile"
        rng = np.random.default_rng(5)
        keep = np.zeros(m, bool)
        per_tile = min(7, MAX_ACTIVE // (last_tile + 1))
        for tile in range(last_tile + 1):
            lo, hi = 32 * tile, min(32 * tile + 32, m)
            keep[lo + rng.permutation(hi - lo)[:per_tile]] = True
    assert 0 < keep.sum() <= MAX_ACTIVE, keep.sum()
    return keep


# ---- the stages -------------------------------------------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


def stage_xin(dir_in):
    x = dir_in[:, :DIR_IN]
    return D.bf16_rne(x.double().numpy()), None, x.bfloat16().double().numpy()


def stage_h9(xin, w):
    """pre-activation of Dense_9 (check_rounded applies the ReLU)"""
    return xin @ w.w9 + w.b9, np.abs(xin) @ np.abs(w.w9) + np.abs(w.b9), (_f32(xin) @ w.w9_f + w.b9_32).double().numpy()


def stage_dir_out(h9, w):
    return h9 @ w.w10 + w.b10, np.abs(h9) @ np.abs(w.w10) + np.abs(w.b10), (_f32(h9) @ w.w10_f + w.b10_32).double().numpy()


def stage_dy10(g_dir_out):
    return D.bf16_rne(g_dir_out.double().numpy()), None, g_dir_out.bfloat16().double().numpy()


def stage_dy9(dy10, mask9, w):
    k = np.asarray(mask9, np.float64)
    return (k * (dy10 @ w.w10.T), k * (np.abs(dy10) @ np.abs(w.w10).T),
            (_f32(dy10) @ w.w10_f.T).double().numpy() * k)


def stage_g_dir_in(dy9, w):
    return dy9 @ w.w9.T, np.abs(dy9) @ np.abs(w.w9).T, (_f32(dy9) @ w.w9_f.T).double().numpy()


def stage_wgrads(xin, h9, dy9, dy10):
    """{name: (ref, abs, cpu fp32)} of dW9 [273,128], db9 [128], dW10 [128,3], db10 [3]"""
    out = {}
    for name, x, dy in (("9", xin, dy9), ("10", h9, dy10)):
        out["dW" + name] = (x.T @ dy, np.abs(x).T @ np.abs(dy), (_f32(x).T @ _f32(dy)).double().numpy())
        out["db" + name] = (dy.sum(0), np.abs(dy).sum(0), _f32(dy).sum(0).double().numpy())
    return out


def grad_ranges():
    w9, b9, w10, b10, n = offsets()
    return {"dW9": (w9, b9, (DIR_IN, HID)), "db9": (b9, w10, (HID,)), "dW10": (w10, b10, (HID, 3)), "db10": (b10, n, (3,))}


def emulate(dir_in, g_dir_out, w):
    """the bf16 path in torch.float32 on the CPU: what a correct implementation computes, up to the order of its fp32 sums.
    -> dict of float64 numpy: xin, h9, mask9, dir_out, dy10, dy9, g_dir_in [m, 273], dW9, db9, dW10, db10"""
    r = {}
    r["xin"] = stage_xin(dir_in)[2]
    r["h9"] = D.bf16_rne(np.maximum(stage_h9(r["xin"], w)[2], 0.0))
    r["mask9"] = r["h9"] > 0
    r["dir_out"] = stage_dir_out(r["h9"], w)[2]
    r["dy10"] = stage_dy10(g_dir_out)[2]
    r["dy9"] = D.bf16_rne(stage_dy9(r["dy10"], r["mask9"], w)[2])
    r["g_dir_in"] = stage_g_dir_in(r["dy9"], w)[2]
    for name, (_, _, cpu) in stage_wgrads(r["xin"], r["h9"], r["dy9"], r["dy10"]).items():
        r[name] = cpu
    return r


# ---- the rules on one result (the kernel's decoded dumps, or the emulation) --------------------------------------------------
def _rounded(stats, stage, what, got, ref, delta, cpu, relu=False):
    f = (lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v)
    cpu_share = float((D.bf16_rne(f(cpu)) != D.bf16_rne(f(ref))).mean())
    n_allow, n_diff = D.check_rounded(got, ref, delta, relu=relu, what=f"{stage} {what}")
    need = D.needed_share_of_delta(got, ref, delta, relu=relu)
    stats[stage] = dict(allow=n_allow / got.size, diff=n_diff / got.size, cpu=cpu_share, need=need)
    D.check_cap(n_diff, got.size, cpu_share, what=f"{stage} {what}")


def check_forward(r, dir_in, w, what):
    """xin, h9, mask9, dir_out of one result from ITS OWN xin and h9 -> {stage: figures}"""
    stats = {}
    ref, _, _ = stage_xin(dir_in)
    bad = D.f64_to_bf16_bits(r["xin"]) != D.f64_to_bf16_bits(ref)
    assert not bad.any(), (f"xin {what}: {int(bad.sum())} elements are not bf16_rne(dir_in) bit for bit, first (evaluation, "
                           f"feature, got, want) {[(int(e), int(f), float(r['xin'][e, f]), float(ref[e, f])) for e, f in np.argwhere(bad)[:8]]}")
    ref, s, cpu = stage_h9(r["xin"], w)
    _rounded(stats, "h9", what, r["h9"], ref, D.dot_delta(K9, s), cpu, relu=True)
    bad = np.asarray(r["mask9"], bool) != (r["h9"] > 0)
    assert not bad.any(), f"mask9 {what}: {int(bad.sum())} bits differ from h9 > 0, first (evaluation, feature) {np.argwhere(bad)[:8].tolist()}"
    ref, s, _ = stage_dir_out(r["h9"], w)
    stats["dir_out"] = D.check_accumulated(r["dir_out"], ref, K10, s, what=f"dir_out {what}")
    return stats


def check_backward(r, g_dir_out, w, n_active, what, scale=1.0, skip_chain=False):
    """dy10, dy9, g_dir_in and the four gradients of one result from ITS OWN xin, h9, mask9, dy10, dy9.  `scale`: the gradient
    entries hold `scale` times the sum (a second accumulating call); n_add = scale n_active + the slabs the fold adds."""
    stats = {}
    m = r["xin"].shape[0]
    if not skip_chain:
        ref, _, _ = stage_dy10(g_dir_out)
        bad = D.f64_to_bf16_bits(r["dy10"]) != D.f64_to_bf16_bits(ref)
        assert not bad.any(), f"dy10 {what}: {int(bad.sum())} elements are not bf16_rne(g_dir_out), first {np.argwhere(bad)[:8].tolist()}"
        ref, s, cpu = stage_dy9(r["dy10"], r["mask9"], w)
        off = ~np.asarray(r["mask9"], bool)
        assert not (r["dy9"][off] != 0).any(), f"dy9 {what}: {int((r['dy9'][off] != 0).sum())} masked-off elements are not zero"
        _rounded(stats, "dy9", what, r["dy9"], ref, D.dot_delta(K10T, s), cpu)
        ref, s, _ = stage_g_dir_in(r["dy9"], w)
        stats["g_dir_in"] = D.check_accumulated(r["g_dir_in"], ref, K9T, s, what=f"g_dir_in {what}")
    blocks, _ = fold_rows(m)
    rows = {"dW9": blocks[0], "db9": blocks[0], "dW10": blocks[1], "db10": blocks[1]}
    for name, (ref, s, _) in stage_wgrads(r["xin"], r["h9"], r["dy9"], r["dy10"]).items():
        n_add = int(scale) * (n_active + rows[name])
        stats[name] = D.check_accumulated(r[name], scale * ref, n_add, scale * s, what=f"{name} x{scale:g} {what}")
    return stats


SENTINEL = 0x7FC5A5A5  # a NaN pattern no kernel produces


def g_dir_in_buffer(g_dir_in, ld, rows):
    """what a correct lnrf_refnerf_dir_bwd leaves in a sentinel-filled g_dir_in of `rows` rows of ld floats (uint32 bits)"""
    m = g_dir_in.shape[0]
    buf = np.full((rows, ld), SENTINEL, np.uint32)
    buf[:m, :min(ld, WRITTEN_COLS)] = 0
    buf[:m, :DIR_IN] = np.asarray(g_dir_in, np.float32).view(np.uint32)
    return buf


def check_g_dir_in_buffer(bits, m, ld, what):
    """The write contract of g_dir_in (include/lnrf.h) on the raw words [rows, ld] of a sentinel-filled buffer: columns
    273 .. min(ld, 288) - 1 of the m rows hold 0, every column from min(ld, 288) on and every row from m on is untouched.
    -> g_dir_in[m, 273] as float64"""
    bits = np.asarray(bits, np.uint32).reshape(-1, ld)
    hi = min(ld, WRITTEN_COLS)
    tail = bits[:m, DIR_IN:hi].view(np.float32)
    bad = tail != 0  # a NaN (the sentinel left in place) counts as non-zero
    assert not bad.any(), (f"g_dir_in {what}: columns {DIR_IN}..{hi - 1} must receive 0; {int(bad.sum())} words do not, first "
                           f"(evaluation, column, value) "
                           f"{[(int(e), DIR_IN + int(c), float(tail[e, c])) for e, c in np.argwhere(bad)[:8]]}")
    beyond = bits[:m, hi:] != SENTINEL
    assert not beyond.any(), (f"g_dir_in {what}: {int(beyond.sum())} words at or beyond column {hi} were written, first "
                              f"(evaluation, column) {[(int(e), hi + int(c)) for e, c in np.argwhere(beyond)[:8]]}")
    assert (bits[m:] == SENTINEL).all(), f"g_dir_in {what}: rows from {m} on were written"
    out = bits[:m, :DIR_IN].view(np.float32).astype(np.float64)
    assert np.isfinite(out).all(), f"g_dir_in {what}: non-finite values (an unwritten word?)"
    return out


def n_active_of(g_dir_out):
    return int((g_dir_out != 0).any(1).sum())


# ---- split path ---------------------------------------------------------------------------------------------------------------
E_OP = 2.0 ** -16
P_PROD = 2 * E_OP + E_OP * E_OP + 2.0 ** -18


def split_exact(dir_in, w):
    """the exact model of the fp32 operands in float64 -> (dir_out [m, 3], its bound per element)"""
    x = dir_in[:, :DIR_IN].double().numpy()
    w9, w10 = w.w9_32.double().numpy(), w.w10_32.double().numpy()
    pre = x @ w9 + w.b9
    s1 = np.abs(x) @ np.abs(w9)
    e1 = P_PROD * s1 + (3 * K9 + 2) * D.U23 * (1.01 * s1 + np.abs(w.b9))
    h = np.maximum(pre, 0.0)
    out = h @ w10 + w.b10
    s2 = (h + e1) @ np.abs(w10)
    bound = e1 @ np.abs(w10) + P_PROD * s2 + (3 * K10 + 2) * D.U23 * (1.01 * s2 + np.abs(w.b10))
    return out, bound


def _split(v):
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def emulate_split(dir_in, w):
    """fp32 emulation of refnerf_dir_fwd_split_kernel: per k-step of 16 features lo.hi, hi.lo, hi.hi into one fp32 accumulator
    that starts from the bias; h9 is split again"""
    def layer(x, wt, b, k_steps):
        k = 16 * k_steps
        xp = torch.zeros(x.shape[0], k)
        xp[:, :x.shape[1]] = x
        wp = torch.zeros(k, wt.shape[1])
        wp[:wt.shape[0]] = wt
        (xh, xl), (wh, wl) = _split(xp), _split(wp)
        acc = b[None, :].repeat(x.shape[0], 1)
        for ks in range(k_steps):
            c = slice(16 * ks, 16 * ks + 16)
            acc = acc + xh[:, c] @ wl[c]
            acc = acc + xl[:, c] @ wh[c]
            acc = acc + xh[:, c] @ wh[c]
        return acc

    h = torch.relu(layer(dir_in[:, :DIR_IN].float(), w.w9_32, w.b9_32, K9 // 16))
    return layer(h, w.w10_32, w.b10_32, K10 // 16).double().numpy()


def check_split(got, dir_in, w, large_rows, what):
    """-> (largest error-to-bound ratio, largest absolute error on the realistic rows)"""
    ref, bound = split_exact(dir_in, w)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bad = err > bound
    assert not bad.any(), (f"dir_out {what}: {int(bad.sum())} of {got.size} elements outside the derived split bound; worst "
                           f"(evaluation, channel, got, ref, bound) "
                           f"{[(int(e), int(c), float(got[e, c]), float(ref[e, c]), float(bound[e, c])) for e, c in np.argwhere(bad)[:8]]}")
    real = np.ones(got.shape[0], bool)
    real[list(large_rows)] = False
    worst = float(err[real].max()) if real.any() else 0.0
    assert worst < 2e-4, f"dir_out {what}: {worst:.3e} off the exact model on the realistic rows (model-level gate 2e-4)"
    return float((err / bound).max()), worst

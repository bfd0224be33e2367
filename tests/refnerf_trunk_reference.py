"""
Float64 reference of RefNERFModel's trunk (ref_nerf.py:92-99: Dense_0..8) and of everything that differentiates through it,
stage by stage, for lnrf_refnerf_trunk_fwd / _normal_pass / _trunk_bwd / _normal_bwd (csrc/refnerf_fused.hip).  A plain module:
importing it collects nothing.  Shared by test_refnerf_trunk_reference_cpu.py (the rules on a numpy emulation of the kernel
arithmetic and on its mutations) and test_gpu_refnerf_trunk.py (the same rules on the kernels).

Every stage is recomputed from the operands the kernel saw (decoded from its own dumps): bf16 weights as float64, fp32
biases.  K = contraction length with its pad k-steps: 64 (Dense_0), 320 (Dense_5 on [h4 | x_emb]), 256 otherwise.

  trunk forward (save, nerf_dump_decode.decode_save)
    x_emb        check_rounded, delta 2e-7 (the pinned accuracy of sincos_pe on |x| <= 1, 2^f <= 512)
    h0..h7       check_rounded(relu) + cap, delta = dot_delta(K, sum |a||W| + |b|); mask_l == h_l > 0
    spatial_out  check_accumulated from h7, K = 256, fp32 bias
  normal pass (chain-state dump in the gradient-dump layout, dy[l] = c_l)
    c_8          bit-equal to -e_0
    c_7..c_0     c_l = bf16(mask_l o (c_{l+1} W_{l+1}[:256]^T)): check_rounded + cap, K = 256, no bias, the SAVED masks
    n_raw[a]     sum_f 2^f (cos(2^f x_a) e_sin[a, f] - sin(2^f x_a) e_cos[a, f]),  e = c_0 W_0^T + c_5 W_5[256:316]^T in fp32
  trunk backward (gradient dump at the front of its scratch)
    dy8          bit-equal to bf16_rne(g_spatial[:, :256])
    dy7..dy0     check_rounded + cap with mask = h_l > 0 (what the layer-stationary pipeline gates with), K = 256
    dW_l, db_l   check_accumulated, reference in_l^T dy_l / sum dy_l from the decoded save and dump
  normal backward (tangent dump in the save layout: x_emb slots = ubar_e, h slots = tbar_l)
    ubar_e       bf16(2^f cos(2^f x) u_a), bf16(-2^f sin(2^f x) u_a): check_rounded, delta = 2^f |u_a| 2e-7 + 2 fp32 ulp
    tbar_0..7    bf16(mask_l o (in_l W_l)), inputs and K as in the forward (Dense_5 on [tbar_4 | ubar_e]), no bias
    dW_l         l = 1..8: tbar_{l-1}^T c_l; Dense_0: ubar_e^T c_0; rows 256.. of Dense_5: ubar_e^T c_5

n_add of the accumulated gradients: evaluations with a non-zero upstream row (a zero row of g_spatial / u gives exact-zero
dy / tbar rows, which add nothing) + the slabs the fold adds: the workgroups of the problem in the production list
(lnrf_host_wgrad_list) for nerf_wgrad_kernel, LS_SLABS = 128 for Dense_1..8 of the layer-stationary pipeline (at most 64
pipelines, each folded once per stage and once in the reduce; the figure of the NeRFModel gate).

The bound of n_raw, derived from emb_bwd_tile (csrc/refnerf_fused.hip), per pair (a, f) and summed over f:
  1. accumulation   e_sin, e_cos are two fp32 accumulators each (one per X layer) of K = 256 exact products:
                    |e - e_exact| <= dot_delta(256, S_0) + dot_delta(256, S_5) =: d, S = sum |c||W|; |cos|, |sin| <= 1, so
                    2^f (d_sin + d_cos).
  2. trig           the kernel holds (s, co) with an error vector v = (s - sin, co - cos).  sincos_pe is within 2e-7 per
                    component, so |v|_2 <= sqrt(2) 2e-7 =: eps_0 for the pairs that come from a call.  Angle doubling
                    (s, co) -> (2 s co, co^2 - s^2) is the complex square z -> z^2 of z = co + i s: (z + v)^2 - z^2 =
                    2 z v + v^2, |z| = 1, so the carried error is at most 2 eps + eps^2; the fp32 evaluation adds one
                    rounding of 2 s co (<= 2^-24 |2 s co|) and up to three of co co - s s (<= 2^-24 (co^2 + s^2 + |co^2 -
                    s^2|) <= 2 2^-24 |z|^2), together at most sqrt(1 + 4) 2^-24 |z + v|^2 <= 3 2^-24 (1 + eps)^2:
                        eps_{i+1} = 2 eps_i + eps_i^2 + 3 2^-24 (1 + eps_i)^2.
                    |co e_sin - s e_cos - (cos e_sin - sin e_cos)| = |(e_sin, -e_cos) . (v_co, v_s)| <= (|e_sin| + |e_cos|) eps.
                    A lane owns the eight pairs pg = 10 a + f of base = 8 (pg // 8): one sincos_pe at its first pair, one at
                    frequency 0 of the next coordinate, doubling in between, so pair pg has seen
                        doublings(pg) = pg - base if pg // 10 == base // 10 else f            (at most 7).
  3. summation      a coordinate receives 20 non-zero terms (10 pairs x 2 X layers; the other adds are + 0.0, exact), each
                    formed with at most two roundings (co e_sin, and the subtraction or its fma; 2^f is exact) and added
                    into one fp32 sum, the two lane halves joined by one more add: (20 + 2 + 2) 2^-23 sum |term|.
|e| in 2 and 3 is taken as |e_0| + |e_5| + d (the fp32 accumulators of the two X layers, bounded from the float64 ones).
test_refnerf_trunk_reference_cpu.py shows that a numpy float32 emulation of the recurrence, seeded with float32 sin / cos,
stays inside eps_i at every test input.
"""
import functools

import numpy as np
import torch

import nerf_dump_decode as D
import refnerf_dir_reference as R
from nerf_grad_helpers import make_points
from test_gpu_nerf_stagewise import embedding

HID, FREQS = D.HIDDEN, 10
K_OF = {0: 64, 5: 320}  # contraction lengths with their pad k-steps; every other layer 256
MS = [1, 31, 33, 1000, 2053]
LDS = [256, 276]
LS_SIZES = ["33", "32P-5", "32(P+8)-31", "96P+1"]
MAX_ACTIVE = 4000
LS_SLABS = 128
SINCOS_TOL = 2e-7
MULTI_MASKS = R.MULTI_MASKS
SENTINEL = R.SENTINEL
LIST_TRUNK, LIST_NORMAL = 2, 3  # `which` of lnrf_host_wgrad_list (csrc/layout_host.cpp)


def k_of(l):
    return K_OF.get(l, 256)


# ---- parameters ---------------------------------------------------------------------------------------------------------------
class Weights:
    """Dense_0..8 of a RefNERFModel vector (the NeRFModel trunk layout): per layer bf16(kernel) as float64 [in, out] and as
    torch.float32, the fp32 bias as float64 and as torch.float32"""

    def __init__(self, flat):
        f = flat.detach().cpu().float()
        self.offs = D.dense_offsets()[:9]
        assert self.offs[8][1] + HID == R.offsets()[0], "Dense_9 does not follow Dense_8"
        self.n = f.numel()
        self.w, self.w_f, self.b, self.b_f = [], [], [], []
        for wo, bo, fi, fo in self.offs:
            wb = f[wo:bo].view(fi, fo).bfloat16()
            self.w.append(wb.double().numpy())
            self.w_f.append(wb.float())
            self.b.append(f[bo:bo + fo].double().numpy())
            self.b_f.append(f[bo:bo + fo].clone())
        self.end = self.offs[8][1] + HID  # first word behind Dense_8


@functools.lru_cache(maxsize=None)
def params():
    return R.make_params()


@functools.lru_cache(maxsize=None)
def weights():
    return Weights(params())


def fold_blocks(which, m):
    """workgroups (= slabs the fold adds) and tiles per workgroup of every problem of a production weight-gradient list"""
    lib = R.host()
    n_tiles = D.padded_tiles(m)
    out = np.zeros(6 * 13, np.int32)
    n = lib.lnrf_host_wgrad_list(which, n_tiles, out.ctypes.data)
    assert n == (1 if which == LIST_TRUNK else 9), n
    blocks = [int(out[6 * i + 1]) for i in range(n)]
    return blocks, [-(-n_tiles // b) for b in blocks]


def multi_sizes():
    """(the smallest m = 32 k - 5 at which every problem of both lists runs on >= 2 workgroups of >= 2 tiles, the smallest at
    which the cap of one workgroup per 6 tiles no longer binds for the 28-workgroup hidden problems), from the lists"""
    def first(cond):
        k = 1
        while not cond(32 * k - 5):
            k += 1
        return 32 * k - 5

    def several(m):  # ... of REAL tiles: the pad tiles of a dump padded to whole workgroups do not count
        real = -(-m // 32)
        return all(min(b) >= 2 and min(p) >= 2 and real >= 2 * max(p)
                   for b, p in (fold_blocks(LIST_TRUNK, m), fold_blocks(LIST_NORMAL, m)))

    def uncapped(m):
        return fold_blocks(LIST_NORMAL, m)[0][:8] == fold_blocks(LIST_NORMAL, 64 * m)[0][:8]

    return first(several), first(uncapped)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
ONE_BELOW = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
EDGE_ROWS = [[0.0, 1.0, -1.0], [ONE_BELOW, -ONE_BELOW, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -1.0, -1.0],
             [-ONE_BELOW, ONE_BELOW, ONE_BELOW]]


def make_x(m):
    """points in [-1, 1]^3 (make_points), the edge rows (exactly 0, +-1, one fp32 ulp below 1) at the front and, from m = 64 on,
    once more at the end (the ragged last tile)"""
    x, _, _ = make_points(m, seed=4000 + m)
    e = torch.tensor(EDGE_ROWS, dtype=torch.float32)
    n = min(m, e.shape[0])
    x[:n] = e[:n]
    if m >= 64:
        x[m - e.shape[0]:] = e
    assert x.dtype == torch.float32 and x.abs().max() <= 1.0
    return x.contiguous()


def keep_mask(variant, m):
    """which evaluations carry an upstream gradient at the multi-workgroup sizes (at most MAX_ACTIVE): the first / the last tile
    of every workgroup's range of every problem of both lists (the ragged last tile with the last ones), or a few evaluations
    of every tile"""
    pers = sorted(set(fold_blocks(LIST_TRUNK, m)[1] + fold_blocks(LIST_NORMAL, m)[1]))
    ev = np.arange(m)
    t = ev // 32
    last_tile = (m - 1) // 32
    keep = np.zeros(m, bool)
    if variant == "first-tiles":
        for per in pers:
            keep |= t % per == 0
        keep &= t != last_tile
    elif variant == "last-tiles":
        for per in pers:
            keep |= t % per == per - 1
        keep |= t == last_tile
    else:
        assert variant == "every-tile"
        rng = np.random.default_rng(5)
        per_tile = max(1, min(7, MAX_ACTIVE // (last_tile + 1)))
        for tile in range(last_tile + 1):
            lo, hi = 32 * tile, min(32 * tile + 32, m)
            keep[lo + rng.permutation(hi - lo)[:per_tile]] = True
    assert 0 < keep.sum() <= MAX_ACTIVE, keep.sum()
    return keep


def make_upstream(m, keep=None):
    """g_spatial[m, 256] and u[m, 3] (fp32); zero rows outside `keep`; a few bf16 ties and zeros in g_spatial"""
    gen = torch.Generator().manual_seed(5000 + m)
    g = torch.randn(m, HID, generator=gen).float()
    u = torch.randn(m, 3, generator=gen).float()
    g[0, 0], g[0, 1], g[0, 2], g[0, 255] = R.tie(0), R.tie(1), -R.tie(2, -3), R.tie(5, 2)
    g[0, 3] = 0.0
    if keep is not None:
        k = torch.from_numpy(np.asarray(keep)).float()[:, None]
        g, u = g * k, u * k
    return g.contiguous(), u.contiguous()


def n_active_of(t):
    return int((t != 0).any(1).sum())


# ---- the embedding and its Jacobian ----------------------------------------------------------------------------------------------
def angles(x32):
    """fp32 arguments 2^f x (exact) as float64 [m, 3, F], and 2^f"""
    scale = 2.0 ** np.arange(FREQS)
    return x32.double().numpy()[:, :, None] * scale[None, None, :], scale


def doublings():
    """how many angle doublings pair pg = 10 a + f has seen in emb_bwd_tile, [3, F], from the lane layout"""
    d = np.zeros((3, FREQS), np.int64)
    for pg in range(3 * FREQS):
        base, a, f = 8 * (pg // 8), pg // FREQS, pg % FREQS
        d[a, f] = pg - base if a == base // FREQS else f
    return d


def eps_chain(n=8):
    """eps_0 .. eps_{n-1} of the doubling recurrence (module docstring)"""
    eps = [np.sqrt(2.0) * SINCOS_TOL]
    for _ in range(n - 1):
        e = eps[-1]
        eps.append(2 * e + e * e + 3 * 2.0 ** -24 * (1 + e) ** 2)
    return np.array(eps)


def eps_pairs():
    return eps_chain()[doublings()]  # [3, F]


def emulate_recurrence(x32, advance=True):
    """numpy float32 emulation of emb_bwd_tile's (s, co) per pair: float32 sin / cos at a lane's first pair and at frequency 0
    of the next coordinate, doubling in float32 in between -> s, co [m, 3, F] float32.  advance=False: the coordinate is not
    advanced at a chain restart (the mutation)."""
    x = x32.numpy().astype(np.float32)
    s_out = np.zeros((x.shape[0], 3, FREQS), np.float32)
    c_out = np.zeros_like(s_out)
    two = np.float32(2.0)
    for base in range(0, 3 * FREQS, 8):
        a0, f0 = base // FREQS, base % FREQS
        ang = x[:, a0] * np.float32(2.0 ** f0)
        s, co = np.sin(ang), np.cos(ang)
        for pg in range(base, min(base + 8, 3 * FREQS)):
            a, f = pg // FREQS, pg % FREQS
            if pg > base:
                if f == 0:
                    xa = x[:, a if advance else a0]
                    s, co = np.sin(xa), np.cos(xa)
                else:
                    s, co = two * s * co, co * co - s * s
            s_out[:, a, f], c_out[:, a, f] = s, co
    return s_out, c_out


def sin_cos_features(e):
    """[m, 60] in the embedding's feature order [coordinate][sin f0.. | cos f0..] -> sin part, cos part [m, 3, F]"""
    e = np.asarray(e).reshape(e.shape[0], 3, 2, FREQS)
    return e[:, :, 0], e[:, :, 1]


def stage_n_raw(x32, c0, c5, w):
    """-> (float64 n_raw [m, 3], bound [m, 3], per-frequency terms and bounds [m, 3, F] for the record)"""
    w0, w5x = w.w[0], w.w[5][HID:]
    e0, e5 = c0 @ w0.T, c5 @ w5x.T
    d = D.dot_delta(256, np.abs(c0) @ np.abs(w0).T) + D.dot_delta(256, np.abs(c5) @ np.abs(w5x).T)
    es, ec = sin_cos_features(e0 + e5)
    ds, dc = sin_cos_features(d)
    a_s, a_c = (p + q + r for p, q, r in zip(sin_cos_features(np.abs(e0)), sin_cos_features(np.abs(e5)), (ds, dc)))
    ang, scale = angles(x32)
    term = scale * (np.cos(ang) * es - np.sin(ang) * ec)
    mag = scale * (a_s + a_c)
    bound_f = scale * (ds + dc) + mag * eps_pairs()[None]
    bound = bound_f.sum(-1) + (20 + 2 + 2) * D.U23 * mag.sum(-1)
    return term.sum(-1), bound, term, bound_f + (20 + 2 + 2) * D.U23 * mag


def stage_ubar(x32, u32):
    """-> (float64 ubar_e [m, 60], delta, the float32 result) in the embedding's feature order"""
    ang, scale = angles(x32)
    u = u32.double().numpy()[:, :, None]
    ref = np.stack([scale * np.cos(ang) * u, -scale * np.sin(ang) * u], 2)  # [m, 3, 2, F]
    ulp = np.where(ref == 0, 0.0, np.ldexp(1.0, np.maximum(np.frexp(np.abs(ref))[1] - 1, -126) - 23))  # u_a = 0: exactly 0
    delta = np.broadcast_to((scale * np.abs(u) * SINCOS_TOL)[:, :, None, :], ref.shape) + 2 * ulp
    a32 = ang.astype(np.float32)
    sc32, u32n = scale.astype(np.float32), u32.numpy()[:, :, None].astype(np.float32)
    cpu = np.stack([sc32 * np.cos(a32) * u32n, -sc32 * np.sin(a32) * u32n], 2)
    m = x32.shape[0]
    return ref.reshape(m, -1), delta.reshape(m, -1), cpu.astype(np.float64).reshape(m, -1)


# ---- the rules ------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


def rounded(stats, stage, what, got, ref, delta, cpu, relu=False):
    R._rounded(stats, stage, what, got, ref, delta, cpu, relu=relu)


def dense_rule(stats, stage, what, got, inp, w64, w32, k, b64=None, b32=None, relu=False, mask=None):
    """one Dense stage from decoded operands (test_gpu_nerf_stagewise.dense_stage on numpy operands): ref = inp bf16(W) (+ b),
    masked by `mask` where given; check_rounded with delta = dot_delta(k, sum |inp||W| (+ |b|)) + the cap"""
    ref, s = inp @ w64, np.abs(inp) @ np.abs(w64)
    cpu = _f32(inp) @ w32
    if b64 is not None:
        ref, s, cpu = ref + b64, s + np.abs(b64), cpu + b32
    cpu = cpu.double().numpy()
    delta = D.dot_delta(k, s)
    if mask is not None:
        mk = np.asarray(mask, np.float64)
        ref, delta, cpu = ref * mk, delta * mk, cpu * mk
    rounded(stats, stage, what, got, ref, delta, cpu, relu=relu)


def fwd_inputs(x_emb, h):
    return [x_emb] + [h[l] for l in range(4)] + [np.concatenate([h[4], x_emb], 1)] + [h[5], h[6]]


def check_forward(r, x32, w, what):
    """r: x_emb [m, 60], h [8][m, 256], mask [8][m, 256], spatial_out [m, 256] -> {stage: figures}"""
    stats = {}
    ref, cpu = embedding(x32, FREQS)
    rounded(stats, "x_emb", what, r["x_emb"], ref.numpy(), np.full(ref.shape, SINCOS_TOL), cpu.numpy())
    ins = fwd_inputs(r["x_emb"], r["h"])
    for l in range(8):
        dense_rule(stats, f"h{l}", what, r["h"][l], ins[l], w.w[l], w.w_f[l], k_of(l), w.b[l], w.b_f[l], relu=True)
        bad = np.asarray(r["mask"][l], bool) != (r["h"][l] > 0)
        assert not bad.any(), (f"mask{l} {what}: {int(bad.sum())} bits differ from h{l} > 0, first (evaluation, feature) "
                               f"{np.argwhere(bad)[:8].tolist()}")
    h7 = r["h"][7]
    stats["spatial_out"] = D.check_accumulated(r["spatial_out"], h7 @ w.w[8] + w.b[8], 256, np.abs(h7) @ np.abs(w.w[8]) + np.abs(w.b[8]),
                                               what=f"spatial_out {what}")
    return stats


def check_normal(r, x32, w, what):
    """r: c [9][m, 256] (the chain-state dump), mask [8] (THE SAVE'S), n_raw [m, 3] -> {stage: figures}"""
    stats = {}
    c = r["c"]
    seed = np.zeros_like(c[8])
    seed[:, 0] = -1.0
    bad = (c[8] != seed) | (np.signbit(c[8]) != np.signbit(seed))
    assert not bad.any(), f"c_8 {what}: {int(bad.sum())} elements differ from -e_0, first (evaluation, feature) {np.argwhere(bad)[:8].tolist()}"
    for l in range(7, -1, -1):
        wt = np.ascontiguousarray(w.w[l + 1][:HID].T)
        dense_rule(stats, f"c{l}", what, c[l], c[l + 1], wt, w.w_f[l + 1][:HID].T.contiguous(), 256, mask=r["mask"][l])
    ref, bound, _, _ = stage_n_raw(x32, c[0], c[5], w)
    got = np.asarray(r["n_raw"], np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), f"n_raw {what}"
    err = np.abs(got - ref)
    bad = err > bound
    assert not bad.any(), (f"n_raw {what}: {int(bad.sum())} of {got.size} elements outside the derived bound; worst (evaluation, "
                           f"coordinate, got, ref, bound) "
                           f"{[(int(e), int(a), float(got[e, a]), float(ref[e, a]), float(bound[e, a])) for e, a in np.argwhere(bad)[:8]]}")
    nz = bound > 0
    stats["n_raw"] = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    assert not (got[~nz] != 0).any(), f"n_raw {what}: non-zero where the reference and its bound are exactly zero"
    return stats


def n_raw_by_frequency(n_raw, x32, c0, c5, w):
    """record only: the device leaves no per-frequency partial sums, so the whole error of an element is set against the part
    of its bound that frequency f contributes -> [F] largest |got - ref| / bound_f"""
    ref, _, _, bound_f = stage_n_raw(x32, c0, c5, w)
    err = np.abs(np.asarray(n_raw, np.float64) - ref)[:, :, None]
    nz = bound_f > 0
    return np.where(nz, err / np.where(nz, bound_f, 1.0), 0.0).max((0, 1))


def check_dy8(dy8, g_spatial, what):
    ref = D.bf16_rne(g_spatial[:, :HID].double().numpy())
    bad = D.f64_to_bf16_bits(dy8) != D.f64_to_bf16_bits(ref)
    assert not bad.any(), (f"dy8 {what}: {int(bad.sum())} elements are not bf16_rne(g_spatial[:, :256]) bit for bit, first "
                           f"(evaluation, feature, got, want) "
                           f"{[(int(e), int(f), float(dy8[e, f]), float(ref[e, f])) for e, f in np.argwhere(bad)[:8]]}")


def trunk_wgrad_reference(x_emb, h, dy, n):
    """float64 dW_l = in_l^T dy_l, db_l = sum dy_l of Dense_0..8 from decoded operands -> reference vector, the same with
    absolute values, how often each word was covered (as test_gpu_nerf_stagewise.wgrad_reference)"""
    ins = fwd_inputs(x_emb, h) + [h[7]]
    ref, ab, cover = (np.zeros(n) for _ in range(3))
    for (wo, bo, fi, fo), xin, d in zip(D.dense_offsets()[:9], ins, dy):
        assert xin.shape[1] == fi and d.shape[1] == fo
        ref[wo:bo], ab[wo:bo] = (xin.T @ d).reshape(-1), (np.abs(xin).T @ np.abs(d)).reshape(-1)
        ref[bo:bo + fo], ab[bo:bo + fo] = d.sum(0), np.abs(d).sum(0)
        cover[wo:bo + fo] += 1
    return ref, ab, cover


def normal_wgrad_reference(ubar, tbar, c, n):
    """float64 second-order kernel gradients: dW_l = tbar_{l-1}^T c_l (l = 1..8), Dense_0 = ubar_e^T c_0, rows 256.. of Dense_5 =
    ubar_e^T c_5; no bias words -> reference vector, absolute values, cover"""
    ins = fwd_inputs(ubar, tbar) + [tbar[7]]
    ref, ab, cover = (np.zeros(n) for _ in range(3))
    for (wo, bo, fi, fo), xin, d in zip(D.dense_offsets()[:9], ins, c):
        ref[wo:bo], ab[wo:bo] = (xin.T @ d).reshape(-1), (np.abs(xin).T @ np.abs(d)).reshape(-1)
        cover[wo:bo] += 1
    return ref, ab, cover


def _wgrad_ranges():
    """{name: (first word, end, n_cols, which fold adds its slabs)}: Dense_0 and rows 256.. of Dense_5 are the merged x_emb
    problem, everything else a hidden problem"""
    out = {}
    for l, (wo, bo, fi, fo) in enumerate(D.dense_offsets()[:9]):
        if l == 0:
            out["dW0"], out["db0"] = (wo, bo, fo, "x"), (bo, bo + fo, fo, "x")
        else:
            out[f"dW{l}"] = (wo, wo + HID * fo, fo, l)
            if l == 5:
                out["dW5x"] = (wo + HID * fo, bo, fo, "x")
            out[f"db{l}"] = (bo, bo + fo, fo, l)
    return out


def check_wgrads(stats, got, ref, ab, n_add_of, what, scale=1.0, biases=True):
    for name, (a, b, fo, kind) in _wgrad_ranges().items():
        if name.startswith("db") and not biases:
            continue
        stats[name] = D.check_accumulated(np.asarray(got[a:b], np.float64).reshape(-1, fo), scale * ref[a:b].reshape(-1, fo),
                                          int(scale) * n_add_of(kind), scale * ab[a:b].reshape(-1, fo),
                                          what=f"{name} x{scale:g} {what}")


def check_trunk_bwd(r, g_spatial, w, what, scale=1.0, skip_chain=False):
    """r: x_emb, h [8] (the save), dy [9] (the first-order dump), grads (the vector after the call into zeros, or `scale` times
    it) -> {stage: figures}"""
    stats = {}
    dy, m = r["dy"], r["x_emb"].shape[0]
    if not skip_chain:
        check_dy8(dy[8], g_spatial, what)
        for l in range(7, -1, -1):
            wt = np.ascontiguousarray(w.w[l + 1][:HID].T)
            dense_rule(stats, f"dy{l}", what, dy[l], dy[l + 1], wt, w.w_f[l + 1][:HID].T.contiguous(), 256, mask=r["h"][l] > 0)
    ref, ab, cover = trunk_wgrad_reference(r["x_emb"], r["h"], dy, w.n)
    assert (cover[:w.end] == 1).all() and not cover[w.end:].any(), f"{what}: Dense_0..8 not covered exactly once"
    n_active = n_active_of(g_spatial[:, :HID])
    assert n_active <= MAX_ACTIVE
    blocks = fold_blocks(LIST_TRUNK, m)[0]
    check_wgrads(stats, r["grads"], ref, ab, lambda kind: n_active + (blocks[0] if kind == "x" else LS_SLABS), what, scale)
    return stats


def check_normal_bwd(r, x32, u32, w, what, scale=1.0, skip_chain=False):
    """r: ubar [m, 60], tbar [8] (the tangent dump), mask [8] (the save), c [9] (the chain-state dump), grads"""
    stats = {}
    m = r["ubar"].shape[0]
    if not skip_chain:
        ref, delta, cpu = stage_ubar(x32, u32)
        rounded(stats, "ubar_e", what, r["ubar"], ref, delta, cpu)
        ins = fwd_inputs(r["ubar"], r["tbar"])
        for l in range(8):
            dense_rule(stats, f"tbar{l}", what, r["tbar"][l], ins[l], w.w[l], w.w_f[l], k_of(l), mask=r["mask"][l])
    ref, ab, cover = normal_wgrad_reference(r["ubar"], r["tbar"], r["c"], w.n)
    n_active = n_active_of(u32)
    assert n_active <= MAX_ACTIVE
    blocks = fold_blocks(LIST_NORMAL, m)[0]
    check_wgrads(stats, r["grads"], ref, ab, lambda kind: n_active + (blocks[8] if kind == "x" else blocks[kind - 1]), what, scale,
                 biases=False)
    return stats


# ---- numpy emulation of the kernel arithmetic ---------------------------------------------------------------------------------
def _mm32(a, b32):
    return (_f32(a) @ b32).double().numpy()


def emulate(x32, g_spatial, u32, w, mut=None):
    """bf16 RNE, fp32 accumulation, the doubling recurrence in float32: what a correct implementation computes, up to the order
    of its fp32 sums.  `mut`: one of MUTATIONS (a subtly wrong kernel).  -> dict: x_emb, h, mask, spatial_out, c, n_raw,
    n_terms [m, 3, F], dy, grads (first order), ubar, tbar, grads2 (second order)"""
    rne = D.bf16_trunc if mut == "truncation" else D.bf16_rne
    r = {}
    m = x32.shape[0]
    r["x_emb"] = rne(embedding(x32, FREQS)[1].numpy())
    h = []
    for l in range(8):
        inp = r["x_emb"] if l == 0 else np.concatenate([h[4], r["x_emb"]], 1) if l == 5 else h[l - 1]
        h.append(rne(np.maximum((_f32(inp) @ w.w_f[l] + w.b_f[l]).double().numpy(), 0.0)))
    r["h"], r["mask"] = h, [v > 0 for v in h]
    r["spatial_out"] = (_f32(h[7]) @ w.w_f[8] + w.b_f[8]).double().numpy()
    # normal pass
    c = [None] * 9
    c[8] = np.zeros((m, HID))
    c[8][:, 0] = 1.0 if mut == "seed +e_0" else -1.0
    for l in range(7, -1, -1):
        ml = l + 1 if mut == "mask l+1" and l < 7 else l - 1 if mut == "mask l-1" and l > 0 else l
        c[l] = rne(r["mask"][ml] * _mm32(c[l + 1], w.w_f[l + 1][:HID].T.contiguous()))
    r["c"] = c
    e0 = _f32(c[0]) @ w.w_f[0].T.contiguous()
    e5 = _f32(c[5]) @ w.w_f[5][HID:].T.contiguous()
    s, co = emulate_recurrence(x32, advance=mut != "no coordinate advance")
    sc = (2.0 ** np.arange(FREQS)).astype(np.float32)
    if mut == "2^f dropped":
        sc = np.ones_like(sc)
    terms = np.zeros((m, 3, FREQS), np.float32)
    for e in ([e0] if mut == "x_emb rows of Dense_5 dropped" else [e5, e0]):
        es, ec = sin_cos_features(e.numpy())
        terms = terms + (sc * (s * es - co * ec) if mut == "sin / cos swapped" else sc * (co * es - s * ec))
    r["n_terms"] = terms.astype(np.float64)
    acc = np.zeros((m, 3), np.float32)
    for f in range(FREQS):
        acc = acc + terms[:, :, f]
    r["n_raw"] = acc.astype(np.float64)
    # first-order backward
    cols = slice(4, 4 + HID) if mut == "dy8 from columns 4..259" else slice(0, HID)
    dy = [None] * 9
    dy[8] = rne(g_spatial[:, cols].double().numpy())
    for l in range(7, -1, -1):
        dy[l] = rne((h[l] > 0) * _mm32(dy[l + 1], w.w_f[l + 1][:HID].T.contiguous()))
    r["dy"] = dy
    grads = np.zeros(w.n)
    ins = fwd_inputs(r["x_emb"], h) + [h[7]]
    for (wo, bo, fi, fo), xin, d in zip(w.offs, ins, dy):
        grads[wo:bo] = (_f32(xin).T @ _f32(d)).double().numpy().reshape(-1)
        grads[bo:bo + fo] = _f32(d).sum(0).double().numpy()
    r["grads"] = grads
    # second-order backward
    r["ubar"] = rne(stage_ubar(x32, u32)[2])
    tbar = []
    for l in range(8):
        inp = r["ubar"] if l == 0 else np.concatenate([tbar[4], r["ubar"]], 1) if l == 5 else tbar[l - 1]
        pre = _mm32(inp, w.w_f[l])
        if mut == "tangent chain from the bias":
            pre = (_f32(inp) @ w.w_f[l] + w.b_f[l]).double().numpy()
        tbar.append(rne(r["mask"][l] * pre))
    r["tbar"] = tbar
    grads2 = np.zeros(w.n)
    ins = fwd_inputs(r["ubar"], tbar) + [tbar[7]]
    for l, ((wo, bo, fi, fo), xin) in enumerate(zip(w.offs, ins)):
        d = c[l - 1] if mut == "dW_l from c_{l-1}" and l > 0 else c[l]
        grads2[wo:bo] = (_f32(xin).T @ _f32(d)).double().numpy().reshape(-1)
    r["grads2"] = grads2
    return r


MUTATIONS = ["mask l+1", "mask l-1", "x_emb rows of Dense_5 dropped", "seed +e_0", "no coordinate advance", "2^f dropped",
             "sin / cos swapped", "tangent chain from the bias", "dW_l from c_{l-1}", "truncation", "dy8 from columns 4..259"]


def check_all(r, x32, g_spatial, u32, w, what):
    """every rule on one result (an emulation's, or a device run's) -> {stage: figures}"""
    stats = check_forward(r, x32, w, what)
    stats.update(check_normal(r, x32, w, what))
    stats.update({f"1:{k}": v for k, v in check_trunk_bwd(r, g_spatial, w, what).items()})
    stats.update({f"2:{k}": v for k, v in check_normal_bwd(dict(r, grads=r["grads2"]), x32, u32, w, what).items()})
    return stats


# ---- float64 composition (what the stage formulas mean, unrounded) ---------------------------------------------------------------
def compose_float64(x64, w_list, b_list, g_spatial, u):
    """The stage formulas above composed WITHOUT any rounding, on float64 kernels [in, out] and biases: -> spatial_out, n_raw,
    first-order gradients [(dW_l, db_l)], second-order kernel gradients [dW_l] (numpy float64)"""
    m = x64.shape[0]
    scale = 2.0 ** np.arange(FREQS)
    ang = x64[:, :, None] * scale
    x_emb = np.concatenate([np.sin(ang), np.cos(ang)], -1).reshape(m, -1)
    h, mask = [], []
    for l in range(8):
        inp = x_emb if l == 0 else np.concatenate([h[4], x_emb], 1) if l == 5 else h[l - 1]
        h.append(np.maximum(inp @ w_list[l] + b_list[l], 0.0))
        mask.append(h[-1] > 0)
    spatial = h[7] @ w_list[8] + b_list[8]
    c = [None] * 9
    c[8] = np.zeros((m, HID))
    c[8][:, 0] = -1.0
    for l in range(7, -1, -1):
        c[l] = mask[l] * (c[l + 1] @ w_list[l + 1][:HID].T)
    es, ec = sin_cos_features(c[0] @ w_list[0].T + c[5] @ w_list[5][HID:].T)
    n_raw = (scale * (np.cos(ang) * es - np.sin(ang) * ec)).sum(-1)
    dy = [None] * 9
    dy[8] = g_spatial
    for l in range(7, -1, -1):
        dy[l] = mask[l] * (dy[l + 1] @ w_list[l + 1][:HID].T)
    ins = fwd_inputs(x_emb, h) + [h[7]]
    first = [(xin.T @ d, d.sum(0)) for xin, d in zip(ins, dy)]
    ubar = np.stack([scale * np.cos(ang) * u[:, :, None], -scale * np.sin(ang) * u[:, :, None]], 2).reshape(m, -1)
    tbar = []
    for l in range(8):
        inp = ubar if l == 0 else np.concatenate([tbar[4], ubar], 1) if l == 5 else tbar[l - 1]
        tbar.append(mask[l] * (inp @ w_list[l]))
    second = [xin.T @ d for xin, d in zip(fwd_inputs(ubar, tbar) + [tbar[7]], c)]
    return spatial, n_raw, first, second

"""
Float64 emulation of the fused InstantNGP MLP kernels (csrc/ngp_mlp.hip), the margins that make an evaluation
"rounding-safe", the checker of the kernels' outputs, and a CPU fp32 simulation of those outputs for the checker's own
tests.  A plain module (numpy / torch on the CPU only): importing it collects nothing.

The kernels write no dump, so a stage cannot be recomputed from its own inputs as test_gpu_nerf_stagewise.py does.
Instead the emulation restates every point where ngp_mlp_kernel rounds to bf16, carries with each the admissible error
`delta` of the fp32 value that is rounded there and its `margin` (the distance to the nearest point where the rounded
value changes), and calls an evaluation SAFE when every margin exceeds its delta.  For a safe evaluation no fp32
accumulation error can move an internal bf16 value: every bf16 operand inside the kernel equals the emulation's bit for
bit, and the outputs differ from float64 by one fp32 accumulation with a worst-case bound.

Rounding points (line numbers of csrc/ngp_mlp.hip):
  W_l -> bf16            ngp_pack_kernel :602, forward and transposed stream alike (ngp_layout.h :84-113); exact input
  enc -> bf16            :188; exact input, delta 0
  d_emb = bf16(sin / cos(2^f d))   :216-232, feature e = 8 coord + 4 is_cos + freq; delta 4e-7 = twice the measured bound of
                         sincos_pe (fast_math.h :3-4); the argument 2^f d is exact in fp32
  h0, c1, c2 = bf16(relu(acc))     relu_frags :38-41 at :273-274, :283-290, :292-293
  o16 = bf16(acc1)       :278; the logit is the fp32 acc1[0], unrounded (:279); density = __expf(logit) :281
  y = tanhf(acc4)        :298-300
  dy4 = bf16(g_rgb (1 - y^2))      :314-316
  dy3 = bf16(mask(c2 != 0) W4 dy4), dy2 likewise with c1      masked_by :49-60 at :328-329, :338-339
  dy1 = bf16(W2[24:40] dy2 + e0 g_density density)            :318, :350-355
  dy0 = bf16(mask(h0 != 0) W1 dy1) :363-364
  g_enc = W0 dy0, fp32   :373-383
  dW_l = X_l^T dy_l, db_l = sum dy_l in fp32 (wgrad_layer :239-268, flush :413-440, ngp_wparts_reduce_kernel :81-105) with
  X_0 = bf16(enc), X_1 = h0, X_2 = [d_emb, o16], X_3 = c1, X_4 = c2.

delta of a Dense stage: (K + 2) 2^-23 (sum |a||b| + |bias|), K = number of non-zero products + number of k-steps of the
stage (ngp_fwd_nk / ngp_bwd_nk): products of bf16 values are exact in fp32 and adding an exact zero rounds nothing.

delta of dy4 = g (1 - y^2), y = tanhf(acc4):  |acc4 - a4| <= d4 (the Dense rule) and |tanh'| <= 1 give
  |dy| = |y_kernel - tanh(a4)| <= d4 + LIBM_ALLOWANCE;
  fp32 y*y, 1 - y*y and the product with g each round once (2^-24 relative, operands <= 1), so
  delta = |g| ((2 |y| + dy) dy + 3 2^-24) + 2^-24 |g (1 - y^2)|.
delta of dy1[0] = acc + g_density density:  the logit has error d1 (its Dense rule), so density = __expf(logit) has
  relative error expm1(d1) + LIBM_ALLOWANCE; the product with g_density and the sum each round once:
  delta = delta_acc + |g_density| density (expm1(d1) + LIBM_ALLOWANCE + 2^-24) + 2^-24 |value|.
LIBM_ALLOWANCE = 1e-5 is the cap the GPU test enforces on the measured error of __expf (relative) and tanhf (absolute).
"""
import concurrent.futures
import ctypes

import numpy as np
import torch

import nerf_dump_decode as D
from nerf_dump_decode import U23, bf16_rne, bf16_trunc, check_accumulated, dot_delta  # noqa: F401 (bf16_trunc: tests)
from oracle.instant_ngp import ngp_spec

LAYERS = 5
D_FREQS, DEMB, DENSITY_DIM, HIDDEN = 4, 24, 16, 64
DEMB_DELTA = 4e-7
LIBM_ALLOWANCE = 1e-5
U24 = 2.0 ** -24
EVALS_PER_GROUP, EVALS_PER_TILE, REDUCE_SLICES = 256, 32, 8


# ---- tables of ngp_layout.h ------------------------------------------------------------------------------------------
def dense_dims(lf):
    """[(fan_in, fan_out)] of Dense_0..4 for an encoding of lf features (oracle.instant_ngp.ngp_spec)"""
    return ngp_spec([0] * lf, [2] * lf, feature_dim=1)[1]


def dense_params(lf):
    return sum(i * o + o for i, o in dense_dims(lf))


def offsets(lf, dense_offset):
    """[(kernel offset, bias offset, fan_in, fan_out)] of Dense_0..4 (ngp_offsets)"""
    out, off = [], dense_offset
    for fi, fo in dense_dims(lf):
        out.append((off, off + fi * fo, fi, fo))
        off += fi * fo + fo
    return out


def ne_of(lf):  # ngp_ne
    return 1 if lf <= 16 else 2


def fwd_nk(l, lf):  # ngp_fwd_nk
    return ne_of(lf) if l == 0 else (3 if l == 2 else 4)


BWD_NK = {4: 1, 3: 4, 2: 4, 1: 1, 0: 4}  # ngp_bwd_nk(4 - l): k-steps of the transposed stage that applies Dense_l^T
WGRAD_PARTS = {3: 1, 2: 1, 1: 2, 4: 2, 0: 2}  # ngp_wgrad_kparts: k-parts of Dense_l's rows in the partial-sum buffer


def host_parts():
    """WGRAD_PARTS as the host build of ngp_layout.h states it (lnrf_host_ngp_parts_plan)"""
    lib = D.load_host_lib()
    out = (ctypes.c_int32 * 20)()
    assert lib.lnrf_host_ngp_parts_plan(16, out) == dense_params(16)
    return {out[4 * i]: out[4 * i + 3] for i in range(LAYERS)}


def n_workgroups(m, cus):
    """grid of the persistent backward (lnrf_ngp_mlp_bwd): min(groups, CUs, 512)"""
    return min(groups_of(m), cus, 512)


def groups_of(m):
    return -(-m // EVALS_PER_GROUP)


def n_rows(layer, n_wg):
    """partial rows and slice sums the reduce launch folds into one gradient entry of Dense_layer"""
    return n_wg * WGRAD_PARTS[layer] + REDUCE_SLICES


# ---- parameters and inputs -------------------------------------------------------------------------------------------
def sparse_params(lf, dense_offset, seed, fan=4):
    """Flat fp32 vector for the tight tests: Dense_0..3 have `fan` non-zero kernel entries per output column at random
    rows, N(0, 1) 1.5 / 2 as general fp32 (the pack's rounding is exercised); Dense_4 is dense lecun-normal (its forward
    accumulator is never rounded to bf16, its transpose contracts 3 terms); biases N(0, 0.1); random words in front."""
    rng = np.random.default_rng(seed)
    flat = rng.standard_normal(dense_offset + dense_params(lf)).astype(np.float32)
    for l, (w, b, fi, fo) in enumerate(offsets(lf, dense_offset)):
        if l < 4:
            k = np.zeros((fi, fo), np.float32)
            for col in range(fo):
                rows = rng.choice(fi, size=min(fan, fi), replace=False)
                k[rows, col] = (rng.standard_normal(rows.size) * 0.75).astype(np.float32)
        else:
            k = (rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(np.float32)
        flat[w:b] = k.reshape(-1)
        flat[b:b + fo] = (rng.standard_normal(fo) * 0.1).astype(np.float32)
    return flat


def flax_params(lf, dense_offset, seed, bias_std=0.0):
    """dense Flax-initialised weights (lecun-normal kernels, zero or N(0, bias_std) biases): the general numerics"""
    rng = np.random.default_rng(seed)
    flat = rng.standard_normal(dense_offset + dense_params(lf)).astype(np.float32)
    for w, b, fi, fo in offsets(lf, dense_offset):
        flat[w:b] = (rng.standard_normal(fi * fo) / np.sqrt(fi)).astype(np.float32)
        flat[b:b + fo] = (rng.standard_normal(fo) * bias_std).astype(np.float32)
    return flat


def inputs(lf, m, seed):
    """enc_t [lf][m] U(-1, 1), unit d [m][3], upstream gradients N(0, 1): fp32"""
    rng = np.random.default_rng(seed)
    enc_t = rng.uniform(-1, 1, (lf, m)).astype(np.float32)
    d = rng.standard_normal((m, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return enc_t, d, rng.standard_normal(m).astype(np.float32), rng.standard_normal((m, 3)).astype(np.float32)


# ---- margins ---------------------------------------------------------------------------------------------------------
def round_margin(v):
    """-> (bf16_rne(v), distance from v to the nearest midpoint between bf16 neighbours) in one pass.  With |v| = f 2^e,
    f in [0.5, 1), the bf16 quantum of v's binade is q = 2^(e - 8) (2^-133 for subnormals) and bf16_rne(|v|) = n q.  The
    neighbour above n q is q away (2 q if the rounding reached the next binade, n = 256), the one below q (q / 2 if n q is
    the binade's lower end, n = 128, and the binade below is not subnormal)."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    _, e = np.frexp(a)
    q = np.ldexp(1.0, np.maximum(e - 8, -133))
    n = np.rint(a / q)
    ra = n * q
    up = np.where(n == 256, 2 * q, q)
    dn = np.where((n == 128) & (e - 9 >= -133), q / 2, q)
    return np.copysign(ra, v), np.minimum(ra + up / 2 - a, a - (ra - dn / 2))


def margin(v, relu=False):
    """distance from v to the nearest point where bf16_rne(relu?(v)) changes: the midpoints between bf16 neighbours, and
    0 after a ReLU (below 0 the value is pinned to 0, so only 0 itself counts there)"""
    v = np.asarray(v, dtype=np.float64)
    mid = round_margin(v)[1]
    return np.where(v <= 0, -v, np.minimum(mid, v)) if relu else mid


def _dense(x, w, bias, k_steps, want_delta=True):
    """-> value, delta of x @ w (+ bias): K = non-zero products + k-steps"""
    val = x @ w
    if bias is not None:
        val = val + bias
    if not want_delta:
        return val, None
    s = np.abs(x) @ np.abs(w)
    if bias is not None:
        s = s + np.abs(bias)
    nnz = (x != 0).astype(np.float64) @ (w != 0).astype(np.float64)
    return val, dot_delta(nnz + k_steps, s)


def demb_arg(d):
    """[m, 24] arguments 2^f d in the kernel's feature order e = 8 coord + 4 is_cos + freq, and the is_cos mask"""
    d = np.asarray(d, dtype=np.float64)
    arg = d[:, :, None, None] * (2.0 ** np.arange(D_FREQS))[None, None, None, :] * np.ones((1, 1, 2, 1))
    is_cos = np.broadcast_to(np.array([False, True])[None, None, :, None], arg.shape)
    return arg.reshape(d.shape[0], DEMB), is_cos.reshape(d.shape[0], DEMB)


class _Points:
    """the rounding points of one pass: name -> (value before rounding, delta, margin, behind a ReLU?)"""

    def __init__(self, rnd, margins, force=None):
        self.rnd, self.margins, self.pts, self.force = rnd, margins, {}, force or {}

    def _forced(self, name, r):
        f = self.force.get(name)
        return r if f is None else np.where(np.isnan(f), r, f)

    def add(self, name, v, delta, relu=False, on=None):
        """-> the rounded tensor.  `on`: ReLU mask of a dy tensor; a masked-out element is an exact 0 with nothing to flip"""
        if on is not None:
            v = np.where(on, v, 0.0)
        f = np.maximum(v, 0.0) if relu else v
        if not self.margins:
            return self._forced(name, self.rnd(f))
        r, mg = round_margin(v)
        if relu:
            mg = np.where(v <= 0, -v, np.minimum(mg, v))
        if on is not None:
            delta, mg = np.where(on, delta, 0.0), np.where(on, mg, np.inf)
        self.pts[name] = (v, delta, mg, relu)
        if self.rnd is not bf16_rne:
            return self._forced(name, self.rnd(f))
        return self._forced(name, np.maximum(r, 0.0) if relu else r)

    def safe(self, m):
        ok = np.ones(m, bool)
        for v, delta, mg, _ in self.pts.values():
            ok &= (mg > delta).reshape(m, -1).all(1)
        return ok


def forward(flat, dense_offset, enc_t, d, rnd=bf16_rne, margins=True, force=None):
    """float64 emulation of the forward.  `rnd` rounds what the kernel keeps in bf16 (identity = the exact model).
    `force`: {rounding point: array of its shape, NaN = as computed, else the rounded value to carry on with}.
    -> dict: the rounded tensors X_l, bf16 weights W, the fp32 outputs' references with their deltas, the rounding points
    ("points") and `safe` [m] (every forward margin exceeds its delta)"""
    flat = np.asarray(flat, dtype=np.float64)
    enc = np.asarray(enc_t, dtype=np.float64).T  # [m, lf]
    m, lf = enc.shape
    W, B = [], []
    for w, b, fi, fo in offsets(lf, dense_offset):
        W.append(rnd(flat[w:b].reshape(fi, fo)))
        B.append(flat[b:b + fo])
    p = _Points(rnd, margins, force)
    x0 = rnd(enc)
    a0, d0 = _dense(x0, W[0], B[0], fwd_nk(0, lf))
    h0 = p.add("h0", a0, d0, relu=True)
    a1, d1 = _dense(h0, W[1], B[1], fwd_nk(1, lf))
    o16 = p.add("o16", a1, d1)
    arg, is_cos = demb_arg(d)
    e_pre = np.where(is_cos, np.cos(arg), np.sin(arg))
    demb = p.add("d_emb", e_pre, np.full(e_pre.shape, DEMB_DELTA))
    x2 = np.concatenate([demb, o16], 1)
    a2, d2 = _dense(x2, W[2], B[2], fwd_nk(2, lf))
    c1 = p.add("c1", a2, d2, relu=True)
    a3, d3 = _dense(c1, W[3], B[3], fwd_nk(3, lf))
    c2 = p.add("c2", a3, d3, relu=True)
    a4, d4 = _dense(c2, W[4], B[4], fwd_nk(4, lf))
    return {"m": m, "lf": lf, "rnd": rnd, "points": p.pts, "safe": p.safe(m), "W": W, "B": B, "X": [x0, h0, x2, c1, c2],
            "logit": a1[:, 0], "logit_delta": d1[:, 0], "density": np.exp(a1[:, 0]), "a4": a4, "a4_delta": d4,
            "rgb": np.tanh(a4)}


def backward(fw, g_density, g_rgb, dy_rnd=None, margins=True):
    """float64 emulation of the backward on top of forward(): -> a copy of `fw` with DY = [dy0..dy4], g_enc and its delta, the
    backward's rounding points merged in and `safe` over all points (forward's only if margins=False)"""
    rnd = fw["rnd"] if dy_rnd is None else dy_rnd
    gd, gc = np.asarray(g_density, dtype=np.float64), np.asarray(g_rgb, dtype=np.float64)
    W, (x0, h0, x2, c1, c2), y, m = fw["W"], fw["X"], fw["rgb"], fw["m"]
    p = _Points(rnd, margins)
    v4 = gc * (1 - y * y)
    ey = fw["a4_delta"] + LIBM_ALLOWANCE
    dy4 = p.add("dy4", v4, np.abs(gc) * ((2 * np.abs(y) + ey) * ey + 3 * U24) + U24 * np.abs(v4))
    t, dt = _dense(dy4, W[4].T, None, BWD_NK[4], margins)
    dy3 = p.add("dy3", t, dt, on=c2 != 0)
    t, dt = _dense(dy3, W[3].T, None, BWD_NK[3], margins)
    dy2 = p.add("dy2", t, dt, on=c1 != 0)
    t, dt = _dense(dy2, W[2][DEMB:].T, None, BWD_NK[2], margins)
    gl = gd * fw["density"]
    t = t.copy()
    t[:, 0] += gl
    if margins:
        dt = dt.copy()
        dt[:, 0] += np.abs(gl) * (np.expm1(fw["logit_delta"]) + LIBM_ALLOWANCE + U24) + U24 * np.abs(t[:, 0])
    dy1 = p.add("dy1", t, dt)
    t, dt = _dense(dy1, W[1].T, None, BWD_NK[1], margins)
    dy0 = p.add("dy0", t, dt, on=h0 != 0)
    g_enc = dy0 @ W[0].T
    em = dict(fw)
    em.update(points={**fw["points"], **p.pts}, safe=fw["safe"] & p.safe(m) if margins else fw["safe"],
              DY=[dy0, dy1, dy2, dy3, dy4], g_enc=g_enc)
    return em


def emulate(flat, dense_offset, enc_t, d, g_density, g_rgb, rnd=bf16_rne, dy_rnd=None, margins=True):
    """forward() + backward(): the whole float64 emulation"""
    return backward(forward(flat, dense_offset, enc_t, d, rnd, margins), g_density, g_rgb, dy_rnd, margins)


def wgrad_reference(em, sel=None):
    """float64 dW_l = X_l^T dy_l, db_l = sum dy_l over the evaluations `sel` (default all) and the same contractions of
    absolute values -> [(dW, |dW|, db, |db|)] per layer"""
    out = []
    for x, dy in zip(em["X"], em["DY"]):
        if sel is not None:
            x, dy = x[sel], dy[sel]
        out.append((x.T @ dy, np.abs(x).T @ np.abs(dy), dy.sum(0), np.abs(dy).sum(0)))
    return out


def dense_vector(per_layer, lf, which=0):
    """layer-wise (dW, .., db, ..) tuples -> flat Dense gradient vector (kernel then bias per layer); which = 0 values, 1 abs"""
    return np.concatenate([np.concatenate([t[which].reshape(-1), t[2 + which]]) for t in per_layer])


def safe_problem(flat, dense_offset, enc_t, d, g_density, g_rgb, keep=None, fw=None, safe=None):
    """The tight-test problem: safety from the emulation of the given inputs, upstream gradients zeroed on every unsafe
    evaluation (and outside `keep`, a bool mask or a function safe -> bool mask), emulation of the masked problem (its `safe`
    is the forward's: the forward of an evaluation without upstream gradient is still checked).  `fw`, `safe`: forward() and the safety
    of the same inputs, if the caller has them.
    -> (emulation of the masked problem, safe, active, masked g_density, masked g_rgb)"""
    fw = forward(flat, dense_offset, enc_t, d) if fw is None else fw
    safe = backward(fw, g_density, g_rgb)["safe"] if safe is None else safe
    active = safe.copy()
    if keep is not None:
        active &= keep(safe) if callable(keep) else keep
    gd = np.where(active, g_density, 0).astype(np.float32)
    gc = np.where(active[:, None], g_rgb, 0).astype(np.float32)
    # evaluations are independent columns: zeroing other evaluations' gradients moves no value of an active one
    em = backward(fw, gd, gc, margins=False)
    assert all((dy[~active] == 0).all() for dy in em["DY"])
    return em, safe, active, gd, gc


SAFE_SHARE_MIN = 0.20
DENSE_OFFSETS = [0, 6, 2 * 4096]
SINGLE_GROUP_M = [1, 31, 33, 255, 257, 2053]
ENC_DIMS = [2, 16, 18, 32]  # the smallest even width, NE = 1 full, NE = 2 with two real features in the second k-step, NE = 2 full
MULTI_ENC_DIMS = [16, 32]


def multi_group_m(cus):
    """G = 2 CUs + 3 groups: workgroups of the persistent backward take 2 or 3 groups, the last tile is ragged"""
    return EVALS_PER_GROUP * (2 * cus + 3) - 5


def gpu_cases(cus):
    """(lf, m, dense_offset, seed) of every tight case test_gpu_ngp_mlp_kernel.py runs on a device with `cus` CUs"""
    cases = []
    for i, lf in enumerate(ENC_DIMS):
        for j, m in enumerate(SINGLE_GROUP_M):
            cases.append((lf, m, DENSE_OFFSETS[(i + j) % 3], 100 * lf + j))
    for lf in MULTI_ENC_DIMS:
        cases.append((lf, multi_group_m(cus), DENSE_OFFSETS[lf // 16], 7 * lf))
    return cases


FWD_POINTS = ("h0", "o16", "d_emb", "c1", "c2")
HAZARD_SPREAD = 1e-3  # half the 2e-3 gate of the unsafe evaluations; the other half is left to fp32 error (about 1e-6)
HAZARD_POINTS = 4


def flip_hazard(fw, flat, dense_offset, enc_t, d):
    """Which evaluations could miss the 2e-3 forward gate with a CORRECT kernel -> bool [m].  At a forward rounding point
    whose margin is within its delta the fp32 accumulator may land on either side, so the kernel may carry on with the other
    admissible neighbour bf16_rne(relu?(v -+ delta)).  An unsafe evaluation is a hazard if, for one of the 2^k roundings of
    its k near-boundary points, density or rgb of the emulation moves by more than HAZARD_SPREAD (density as
    |x - ref| / (1 + ref), the gate's measure), or a further point comes within delta of a boundary, or k > HAZARD_POINTS.
    Everything here is the emulation's; no kernel output enters."""
    hazard = np.zeros(fw["m"], bool)
    un = np.flatnonzero(~fw["safe"])
    if un.size == 0:
        return hazard
    near, alts, cols, c0 = [], [], {}, 0
    for name in FWD_POINTS:
        v, dl, mg, relu = fw["points"][name]
        v, dl, mg = v[un], dl[un], mg[un]
        f = (lambda t: np.maximum(t, 0.0)) if relu else (lambda t: t)
        here, lo, hi = bf16_rne(f(v)), bf16_rne(f(v - dl)), bf16_rne(f(v + dl))
        near.append(~(mg > dl))
        alts.append(np.where(lo == here, hi, lo))
        cols[name] = slice(c0, c0 + v.shape[1])
        c0 += v.shape[1]
    near, alts = np.concatenate(near, 1), np.concatenate(alts, 1)
    rank = np.clip(np.cumsum(near, 1) - 1, 0, 31)  # index of a near-boundary point among its evaluation's
    k = near.sum(1)
    hz = k > HAZARD_POINTS
    enc_t, d = np.asarray(enc_t), np.asarray(d)
    for combo in range(1, 2 ** HAZARD_POINTS):
        rows = np.flatnonzero((k >= combo.bit_length()) & ~hz)
        if rows.size == 0:
            continue
        flip = near[rows] & ((np.right_shift(combo, rank[rows]) & 1) == 1)
        force = {name: np.where(flip[:, sl], alts[rows][:, sl], np.nan) for name, sl in cols.items()}
        alt = forward(flat, dense_offset, enc_t[:, un[rows]], d[un[rows]], force=force)
        more = np.zeros(rows.size, bool)
        for name, sl in cols.items():
            _, dl2, mg2, _ = alt["points"][name]
            more |= (~(mg2 > dl2) & ~near[rows][:, sl]).any(1)
        ref = fw["density"][un[rows]]
        e_d = np.abs(alt["density"] - ref) / (1 + ref)
        e_y = np.abs(alt["rgb"] - fw["rgb"][un[rows]]).max(1)
        hz[rows] |= more | (e_d > HAZARD_SPREAD) | (e_y > HAZARD_SPREAD)
    hazard[un] = hz
    return hazard


def _merge(fw, sub, idx):
    """rows idx of forward() dict fw <- forward() of those evaluations alone"""
    for key in ("safe", "logit", "logit_delta", "density", "a4", "a4_delta", "rgb"):
        fw[key][idx] = sub[key]
    for a, b in zip(fw["X"], sub["X"]):
        a[idx] = b
    for name, (v, dl, mg, _) in fw["points"].items():
        sv, sdl, smg, _ = sub["points"][name]
        v[idx], dl[idx], mg[idx] = sv, sdl, smg


def _concat(fws):
    """forward() dicts of consecutive blocks of evaluations -> one"""
    out = dict(fws[0])
    out["m"] = sum(f["m"] for f in fws)
    for key in ("safe", "logit", "logit_delta", "density", "a4", "a4_delta", "rgb"):
        out[key] = np.concatenate([f[key] for f in fws])
    out["X"] = [np.concatenate([f["X"][l] for f in fws]) for l in range(LAYERS)]
    out["points"] = {name: tuple(np.concatenate([f["points"][name][i] for f in fws]) for i in range(3)) + (pt[3],)
                     for name, pt in fws[0]["points"].items()}
    return out


GEN_BLOCK = 8192


def safe_share_inputs(lf, m, dense_offset, seed):
    """Parameters and inputs of a tight case, chosen from the emulation alone, before any kernel runs:
      * an evaluation that is a flip_hazard — a correct kernel could miss the 2e-3 gate of the unsafe evaluations on it,
        because one admissible rounding moves its output by more than 1e-3 — gets fresh enc / d draws until it is none
        (evaluations are independent columns; about 1 % of them are redrawn; the others stay, unsafe ones included);
      * at least SAFE_SHARE_MIN of the evaluations are safe.  A handful of evaluations can miss the share by chance (m = 1
        has one evaluation), so the seed is advanced until the draw reaches it.
    -> flat, enc_t, d, g_density, g_rgb (unmasked), forward(), safe"""
    for attempt in range(64):
        flat = sparse_params(lf, dense_offset, seed + 1000 * attempt)
        enc_t, d, gd, gc = inputs(lf, m, seed + 1000 * attempt + 1)

        def block(lo):  # evaluations are independent: blocks of GEN_BLOCK run side by side (numpy releases the GIL)
            hi = min(lo + GEN_BLOCK, m)
            rng = np.random.default_rng([seed + 1000 * attempt + 2, lo])
            e, dd = enc_t[:, lo:hi].copy(), d[lo:hi].copy()
            fw = forward(flat, dense_offset, e, dd)
            idx, sub = np.arange(hi - lo), fw
            for _ in range(64):
                hz = flip_hazard(sub, flat, dense_offset, e[:, idx], dd[idx])
                if not hz.any():
                    break
                idx = idx[hz]
                e[:, idx], dd[idx] = inputs(lf, idx.size, int(rng.integers(1 << 31)))[:2]
                sub = forward(flat, dense_offset, e[:, idx], dd[idx])
                _merge(fw, sub, idx)
            else:
                raise AssertionError(f"flip hazards remain after 64 redraws at lf={lf} m={m}")
            return e, dd, fw, backward(fw, gd[lo:hi], gc[lo:hi])["safe"]

        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            parts = list(pool.map(block, range(0, m, GEN_BLOCK)))
        enc_t = np.concatenate([p[0] for p in parts], 1)
        d = np.concatenate([p[1] for p in parts])
        fw, safe = _concat([p[2] for p in parts]), np.concatenate([p[3] for p in parts])
        if safe.mean() >= SAFE_SHARE_MIN:
            return flat, enc_t, d, gd, gc, fw, safe
    raise AssertionError(f"no seed gives {SAFE_SHARE_MIN:.0%} safe evaluations at lf={lf} m={m}")


# ---- the checker -----------------------------------------------------------------------------------------------------
def _owner(ev, n_wg):
    g = int(ev) // EVALS_PER_GROUP
    return f"evaluation {int(ev)} (group {g}, round {g // n_wg}, workgroup {g % n_wg})"


def _acc_elementwise(got, ref, k, s, what):
    """check_accumulated with a per-element n_add = k: the bound (k + 2) 2^-23 s is handed over as (kmax + 2) 2^-23 s'"""
    kmax = float(np.max(k)) if np.size(k) else 0.0
    return check_accumulated(got, ref, kmax, s * (k + 2) / (kmax + 2), what=what)


def check_forward(em, density, rgb, allow_density, allow_rgb, what, unsafe_tol=2e-3):
    """check_forward_safe + check_forward_unsafe -> (largest density excess over the propagated delta, rgb excess)"""
    out = check_forward_safe(em, density, rgb, allow_density, allow_rgb, what)
    check_forward_unsafe(em, density, rgb, what, unsafe_tol)
    return out


def _fwd_errors(em, density, rgb, what):
    dens, y = np.asarray(density, np.float64).reshape(-1), np.asarray(rgb, np.float64).reshape(-1, 3)
    assert dens.shape == (em["m"],) and np.isfinite(dens).all() and np.isfinite(y).all(), f"{what}: non-finite forward output"
    return dens, np.abs(dens - em["density"]) / em["density"], np.abs(y - em["rgb"])


def check_forward_safe(em, density, rgb, allow_density, allow_rgb, what):
    """Evaluations whose forward is safe: density against exp(a1[0]) relative, rgb against tanh(a4) absolute, bound =
    propagated delta + allowance (for the exp / tanh routine).
    -> (largest density error beyond the propagated delta, the same for rgb; 0 if none)"""
    safe = em["safe"]
    _, e_d, e_y = _fwd_errors(em, density, rgb, what)
    p_d, p_y = np.expm1(em["logit_delta"]), em["a4_delta"]  # exp: relative error of the value; |tanh'| <= 1
    x_d = float(np.max((e_d - p_d)[safe], initial=0.0))
    x_y = float(np.max((e_y - p_y)[safe], initial=0.0))
    bad = safe & ((e_d > p_d + allow_density) | (e_y > p_y + allow_rgb).any(1))
    assert not bad.any(), (f"{what}: forward of {int(bad.sum())} safe evaluations beyond propagated delta + {allow_density:g} "
                           f"(density) / {allow_rgb:g} (rgb); first {np.flatnonzero(bad)[:8]}; largest excess density "
                           f"{x_d:.3e} rgb {x_y:.3e}")
    return x_d, x_y


def check_forward_unsafe(em, density, rgb, what, tol=2e-3):
    """Evaluations whose forward is not safe: the end-to-end gate of test_gpu_instant_ngp.py against the emulation,
    |rgb - ref| < tol and |density - ref| / (1 + ref) < tol.  A failure lists, per offending evaluation, the rounding points
    whose margin is within delta (where the kernel may legitimately round the other way).  -> number of unsafe evaluations"""
    unsafe = ~em["safe"]
    dens, _, e_y = _fwd_errors(em, density, rgb, what)
    e_d = np.abs(dens - em["density"]) / (1 + em["density"])
    loose = unsafe & ((e_d > tol) | (e_y > tol).any(1))
    if loose.any():
        rows = []
        for ev in np.flatnonzero(loose)[np.argsort(-np.maximum(e_d, e_y.max(1))[loose])][:8]:
            near = [f"{name}[{j}] = {v[ev, j]:.7g} margin {mg[ev, j]:.2e} delta {dl[ev, j]:.2e}"
                    for name, (v, dl, mg, _) in em["points"].items() if name in ("h0", "o16", "d_emb", "c1", "c2")
                    for j in np.flatnonzero(~(mg[ev] > dl[ev]))]
            rows.append(f"    evaluation {int(ev)}: density error {e_d[ev]:.3e} rgb error {e_y[ev].max():.3e}; " + "; ".join(near))
        raise AssertionError(f"{what}: forward of {int(loose.sum())} of {int(unsafe.sum())} unsafe evaluations beyond {tol:g} "
                             f"(largest density error {e_d[loose].max():.3e}, rgb {e_y[loose].max():.3e}); worst:\n" + "\n".join(rows))
    return int(unsafe.sum())


def check_forward_admissible(fw, flat, dense_offset, enc_t, d, density, rgb, allow_density, allow_rgb, what, max_points=4):
    """Unsafe evaluations, tightly: an evaluation whose forward has rounding points within delta of a boundary may round
    those either way, so its density / rgb must meet the bound of check_forward_safe against the emulation for ONE of the
    2^k admissible roundings of its k near-boundary points (the other neighbour is bf16_rne(relu?(v -+ delta))).
    Evaluations with more than `max_points` such points are not enumerated.
    -> (unsafe evaluations, of them not matching the plain emulation, not enumerated)"""
    unsafe = np.flatnonzero(~fw["safe"])
    dens, e_d, e_y = _fwd_errors(fw, density, rgb, what)
    y = np.asarray(rgb, np.float64).reshape(-1, 3)

    def within(em, ev, rows):
        ed = np.abs(dens[ev] - em["density"][rows]) / em["density"][rows]
        ey = np.abs(y[ev] - em["rgb"][rows])
        return (ed <= np.expm1(em["logit_delta"][rows]) + allow_density) & (ey <= em["a4_delta"][rows] + allow_rgb).all(1)

    off = unsafe[~within(fw, unsafe, unsafe)]  # the kernel took another admissible rounding somewhere (or is wrong)
    near = {}  # evaluation -> [(point, element, the other admissible rounded value)]
    for name in FWD_POINTS:
        v, dl, mg, relu = fw["points"][name]
        f = (lambda t: np.maximum(t, 0.0)) if relu else (lambda t: t)
        for i, ev in enumerate(off):
            for j in np.flatnonzero(~(mg[ev] > dl[ev])):
                here, lo, hi = bf16_rne(f(v[ev, j])), bf16_rne(f(v[ev, j] - dl[ev, j])), bf16_rne(f(v[ev, j] + dl[ev, j]))
                near.setdefault(i, []).append((name, j, hi if lo == here else lo))
    many = np.array([len(near.get(i, [])) > max_points for i in range(off.size)], bool)
    todo = np.flatnonzero(~many)
    matched = np.zeros(off.size, bool)
    sub_enc, sub_d = np.asarray(enc_t)[:, off[todo]], np.asarray(d)[off[todo]]
    for combo in range(1, 2 ** max_points):
        force = {name: np.full((todo.size,) + fw["points"][name][0].shape[1:], np.nan) for name in FWD_POINTS}
        for row, i in enumerate(todo):
            for t, (name, j, alt) in enumerate(near.get(i, [])):
                if combo >> t & 1:
                    force[name][row, j] = alt
        alt_fw = forward(flat, dense_offset, sub_enc, sub_d, force=force)
        matched[todo] |= within(alt_fw, off[todo], np.arange(todo.size))
    bad = np.flatnonzero(~matched & ~many)
    assert bad.size == 0, (f"{what}: {bad.size} unsafe evaluations match the emulation under NO admissible rounding of their "
                           f"near-boundary points, first {off[bad][:8]} (density error {e_d[off[bad]][:4]}, rgb "
                           f"{e_y[off[bad]].max(1)[:4]} against the plain emulation)")
    return unsafe.size, off.size, int(many.sum())


def check_backward(em, active, n_wg, g_enc_t, level_absmax, dense_grad, what, final_add_of=None):
    """The backward's outputs against the emulation of a safe problem.
      g_enc_t [lf][m]      active evaluations: check_accumulated per element against dy0 W0^T; all others exactly 0
      level_absmax [lf/2]  bit-equal to max |g_enc_t| over each level's two rows
      dense_grad           what the call added to the Dense block: every dW_l / db_l entry within
                           (n_active + n_rows + 2) 2^-23 |X|^T|dy|; an exact-zero reference must be exactly 0.
                           `final_add_of` = the fp32 vector the call left there when it was prefilled: the `+=` into a
                           non-zero word rounds once more, 2^-24 |result|, which is added to the bound.
    -> {layer name: largest error-to-bound ratio}"""
    m, lf = em["m"], em["lf"]
    g = np.asarray(g_enc_t, np.float64)
    assert g.shape == (lf, m) and np.isfinite(g).all(), f"{what}: g_enc_t shape / finiteness"
    off = ~active
    if off.any():
        nz = np.flatnonzero((g[:, off] != 0).any(0))
        assert nz.size == 0, (f"{what}: g_enc_t is not exactly 0 on {nz.size} evaluations without upstream gradient, first "
                              f"{[_owner(e, n_wg) for e in np.flatnonzero(off)[nz[:4]]]}")
    ratios = {}
    k = (em["DY"][0] != 0).astype(np.float64) @ (em["W"][0].T != 0).astype(np.float64) + BWD_NK[0]
    s = np.abs(em["DY"][0]) @ np.abs(em["W"][0].T)
    try:
        ratios["g_enc_t"] = _acc_elementwise(g.T[active], em["g_enc"][active], k[active], s[active], what=f"{what}: g_enc_t")
    except AssertionError as e:
        err = np.abs(g.T - em["g_enc"]) - (k + 2) * U23 * s
        worst = np.argsort(-err.max(1))[:4]
        raise AssertionError(f"{e}\n  owners of the worst: {[_owner(w, n_wg) for w in worst]} (element rows index the ACTIVE "
                             f"evaluations)") from None
    lm = np.asarray(level_absmax, np.float32)
    want = np.abs(np.asarray(g_enc_t, np.float32)[:2 * (lf // 2)]).reshape(lf // 2, 2 * m).max(1)
    if not np.array_equal(lm.view(np.uint32), want.view(np.uint32)):
        lv = int(np.flatnonzero(lm.view(np.uint32) != want.view(np.uint32))[0])
        ev = int(np.abs(np.asarray(g_enc_t, np.float32)[2 * lv:2 * lv + 2]).max(0).argmax())
        raise AssertionError(f"{what}: level_absmax {lm.tolist()} != max |g_enc_t| {want.tolist()}; level {lv}'s maximum is at "
                             f"{_owner(ev, n_wg)}")
    n_active = int(active.sum())
    ref = wgrad_reference(em, active)
    dg = np.asarray(dense_grad, np.float64)
    assert dg.shape == (dense_params(lf),), f"{what}: Dense gradient size"
    extra = None if final_add_of is None else np.abs(np.asarray(final_add_of, np.float64)) * U24
    pos = 0
    for l, (dw, sw, db, sb) in enumerate(ref):
        n_add = n_active + n_rows(l, n_wg)
        for kind, r, sa in (("kernel", dw, sw), ("bias", db, sb)):
            got = dg[pos:pos + r.size].reshape(r.shape)
            sa2 = sa if extra is None else sa + extra[pos:pos + r.size].reshape(r.shape) / ((n_add + 2) * U23)
            try:
                ratios[f"Dense_{l}/{kind}"] = check_accumulated(got, r, n_add, sa2, what=f"{what}: Dense_{l} {kind} gradient")
            except AssertionError as e:
                raise AssertionError(f"{e}\n  {_round_shares(em, active, n_wg, l, kind, got - r)}") from None
            pos += r.size
    return ratios


def _round_shares(em, active, n_wg, l, kind, err):
    """what each round of the persistent loop contributes to the worst entry (a lost round shows as err = -share)"""
    i = np.unravel_index(np.abs(err).argmax(), err.shape)
    rounds = np.arange(em["m"]) // EVALS_PER_GROUP // n_wg
    x, dy = em["X"][l], em["DY"][l]
    txt = []
    for r in range(int(rounds.max()) + 1):
        sel = active & (rounds == r)
        c = (x[sel, i[0]] * dy[sel, i[1]]).sum() if kind == "kernel" else dy[sel, i[0]].sum()
        txt.append(f"round {r}: {c:.6e}")
    return f"worst entry {tuple(int(v) for v in i)} error {err[i]:.6e}; reference contributions by round: " + ", ".join(txt)


# ---- CPU fp32 simulation of the kernels' outputs (for the checker's tests) -------------------------------------------------
def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))


def _bf(t):
    return t.bfloat16().float()


def _bf_trunc(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def simulate(flat, dense_offset, enc_t, d, g_density, g_rgb, n_wg, mutation=None, pick=None):
    """torch.float32 restatement of lnrf_ngp_mlp_fwd + _bwd: the same roundings stored in fp32, dW summed per (workgroup,
    k-part) row as kNgpWgrad prescribes (workgroup = group mod n_wg, k-part = the wave's share of the group) and folded as
    ngp_wparts_reduce_kernel does.  `mutation` names one deliberate defect; `pick` = (evaluation, ...) it applies to.
    -> dict(density, rgb, g_enc_t, level_absmax, dense_grad)"""
    enc = _t32(enc_t).t().contiguous()
    m, lf = enc.shape
    flat32 = _t32(flat)
    W, B = [], []
    for w, b, fi, fo in offsets(lf, dense_offset):
        W.append(_bf(flat32[w:b].view(fi, fo)))
        B.append(flat32[b:b + fo])
    rdy = _bf_trunc if mutation == "dy_trunc" else _bf
    x0 = _bf(enc)
    a0 = x0 @ W[0] + B[0]
    h0 = _bf(torch.relu(a0))
    a1 = h0 @ W[1] + B[1]
    o16 = _bf(a1)
    dens = torch.exp(a1[:, 0])
    arg, is_cos = demb_arg(_t32(d).numpy())
    arg32 = _t32(arg)  # exact: 2^f d
    demb = _bf(torch.where(torch.from_numpy(np.ascontiguousarray(is_cos)), torch.cos(arg32), torch.sin(arg32)))
    x2 = torch.cat([demb, o16], 1)
    a2 = x2 @ W[2] + B[2]
    c1 = _bf(torch.relu(a2))
    a3 = c1 @ W[3] + B[3]
    c2 = _bf(torch.relu(a3))
    y = torch.tanh(c2 @ W[4] + B[4])
    gd, gc = _t32(g_density), _t32(g_rgb)
    dy4 = rdy(gc * (1.0 - y * y))
    mask2 = (c2 != 0)
    if mutation == "relu_sign":  # the mask of one element whose bf16 activation is 0 read from somewhere else
        mask2 = mask2.clone()
        assert c2[pick[0], pick[1]] == 0
        mask2[pick[0], pick[1]] = True
    dy3 = rdy((dy4 @ W[4].t()) * mask2)
    dy2 = rdy((dy3 @ W[3].t()) * (c1 != 0))
    t = dy2 @ W[2][DEMB:].t()
    t[:, 0] += gd * dens
    dy1 = rdy(t)
    dy0 = rdy((dy1 @ W[1].t()) * (h0 != 0))
    g_enc_t = (dy0 @ W[0].t()).t().contiguous()
    if mutation == "genc_swap":
        g_enc_t[[0, 1]] = g_enc_t[[1, 0]]
    ev = torch.arange(m)
    group, wave = ev // EVALS_PER_GROUP, (ev % EVALS_PER_GROUP) // EVALS_PER_TILE
    wg = group % n_wg
    n_groups = int(group.max()) + 1
    last_group_of_wg = torch.tensor([max(g for g in range(n_groups) if g % n_wg == w) for w in range(min(n_wg, n_groups))])
    in_last = group == last_group_of_wg[wg]
    lmax_src = g_enc_t.abs()[:2 * (lf // 2)]
    if mutation == "lmax_last_group":
        lmax_src = lmax_src * in_last
    level_absmax = lmax_src.reshape(lf // 2, 2 * m).max(1).values
    keep = torch.ones(m, dtype=torch.bool)
    if mutation == "wacc_zeroed":
        keep = in_last
    elif mutation == "drop_eval":
        keep[pick[0]] = False
    elif mutation == "drop_ragged_tile":
        keep[m - m % EVALS_PER_TILE:] = False
    grad = torch.zeros(dense_params(lf), dtype=torch.float32)
    pos = 0
    for l, (x, dy) in enumerate(zip([x0, h0, x2, c1, c2], [dy0, dy1, dy2, dy3, dy4])):
        parts = WGRAD_PARTS[l]
        part = wave // (8 // parts)
        rows_w, rows_b = [], []
        for w in range(n_wg):
            for q in range(parts):
                sel = keep & (wg == w) & (part == q)
                if mutation == "row_not_folded" and l == 1 and w == n_wg - 1 and q == 1:
                    sel = torch.zeros_like(sel)
                selb = sel & ((ev % 16) // 4 % 2 == 1) if mutation == "db_one_half" else sel  # k slots of lane half 1
                rows_w.append(x[sel].t() @ dy[sel])
                rows_b.append(dy[selb].sum(0))
        for rows, n in ((rows_w, x.shape[1] * dy.shape[1]), (rows_b, dy.shape[1])):
            tot = torch.zeros(n)
            for sl in range(REDUCE_SLICES):
                acc = torch.zeros(n)
                for w in range(n_wg * sl // REDUCE_SLICES, n_wg * (sl + 1) // REDUCE_SLICES):
                    for q in range(parts):
                        acc = acc + rows[w * parts + q].reshape(-1)
                tot = tot + acc
            grad[pos:pos + n] = tot
            pos += n
    return {"density": dens.numpy(), "rgb": y.numpy(), "g_enc_t": g_enc_t.numpy(), "level_absmax": level_absmax.numpy(),
            "dense_grad": grad.numpy()}

"""
GPU parity of every dispatch path of the generic dense GEMM (csrc/dense.hip) against the float64 product of the same
operands, with a derived error bound and guard zones around every operand and output.

Reference and bound.  The reference is the float64 product; under bf16 both operands are first rounded with .bfloat16()
(round-to-nearest-even, as include/lnrf.h states; bf16 x bf16 products are exact in fp32).  For any order of an fp32
summation of R exact products, split into nsplit partial sums that are added afterwards (in order or by atomics),

    |C - C_ref| <= (R + nsplit + 2) u (|A| |B|)_ij + u |C_ref|,        u = 2^-23,

u = 2^-23 (faithful rounding) so that nothing is assumed about the MFMA's internal order.  What is added to the result
afterwards rounds once more: u |c_old| for mode 1 and for the fixed-order fold, nsplit u |c_old| for the nsplit atomic
adds of mode 2 (each rounds a running sum that contains c_old), u |gb_old| for the bias gradient; mode 2 and the bias
gradient also run from C = 0 / gb = 0, where the bound is the formula above alone.  Mode 0 with an activation: act_bound.
Operands are drawn from randn: no subnormals.

Guard zones.  Every operand and output is a strided view into a larger allocation of the test's own: at least 132 rows
in front of and behind the matrix, at least 136 floats between the end of a row and the start of the next, NaN in operand
buffers (rows / columns just past I, J, R, the padding between rows, the floats in front of an offset pointer, the
skipped elements of an operand with element stride 2), a sentinel bit pattern in output buffers.  After the call no
operand word and no output word outside I x J has changed and the result holds no NaN.  A tile-sized over-read or
over-write of a wrong guard therefore stays inside memory the test owns.

Epilogue functions: through a K = 1, w = [[1]] GEMM the pre-activation is exactly the input.  Allowed error on the grid
+-{0, 1e-8, 1e-4, 0.5, 5, 17, 40, 88, 89, 104, 200}: 4 x the error of torch's float32 CPU evaluation of the same function
on the same grid against float64 (in ulps of the float32 result) + 1 ulp, applied per grid point (_allowed).  Measured on
an MI355X, worst over the grid, torch float32 on the CPU | the kernels, in ulps: relu 0 | 0, softplus 0.51 | 0.51,
tanh 0 | 0, exp 0 | 0, sigmoid 1.6e6 | 1.6e6 (both return 0 at x = -88 and -89, where the result is subnormal; 0 | 0 at
every other point); derivatives from outputs: relu 0 | 0, softplus 0.69 | 0.69, tanh 566 | 0 (1 - y y next to y = 1: the
kernel's is a single fma), exp 0 | 0, sigmoid 0.52 | 0.52; sinusoidal_emb 0.60 | 0.99 ulps of 1.  The tests print both
figures on every run.
"""
import numpy as np
import pytest
import torch

import gpu_poison
from test_dense_plan import ALL_PATHS, PATH_TABLE, Case, case_strides, gemm_plan, host_lib, make_case, path_of

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -23
SENTINEL = 0x3A83126F  # 1.0000000475e-3: a store, an add of anything above 1e-10 or a NaN changes it
GUARD_ROWS = 132
PREC = {0: "fp32", 1: "bf16"}

def _bits(t):
    return t.view(torch.int32)


class Guarded:
    """An [outer, inner] matrix (row stride ld, element stride es) inside a flat buffer filled with `fill`."""

    def __init__(self, outer, inner, ld, es=1, off=0, fill=float("nan"), guard_rows=GUARD_ROWS):
        assert ld >= (inner - 1) * es + 1 and 0 <= off < 4
        self.start = (guard_rows * ld + 8 + 3) // 4 * 4 + off
        n = self.start + (outer + guard_rows) * ld + 8
        if isinstance(fill, int):
            self.flat = torch.full((n,), fill, dtype=torch.int32, device="cuda").view(torch.float32)
        else:
            self.flat = torch.full((n,), fill, dtype=torch.float32, device="cuda")
        self.view = self.flat.as_strided((outer, inner), (ld, es), self.start)
        self.ptr = self.flat[self.start:]  # what the kernel gets: the pointer of element (0, 0)
        self.low = self.ptr.data_ptr() & 15
        self.snap = None

    def set(self, values):
        self.view.copy_(values.to(torch.float32).cuda())
        self.snap = _bits(self.flat).clone()
        return self

    def unchanged(self):
        return torch.equal(_bits(self.flat), self.snap)

    def take(self, fill):
        """The matrix; what is left of the buffer afterwards must be `fill` everywhere."""
        out = self.view.clone()
        _bits(self.flat).as_strided(self.view.shape, self.view.stride(), self.start).fill_(fill)
        return out, bool((_bits(self.flat) == fill).all())


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _rounded(t, bf16):
    return t.bfloat16().double() if bf16 else t.double()


def gemm_bound(a64, b64, ref, r_depth, nsplit, c_old=None, c_old_adds=1):
    """The bound of the module docstring (a64, b64: the float64 operands the kernel multiplies)."""
    bound = (r_depth + nsplit + 2) * U * (a64.abs() @ b64.abs()) + U * ref.abs()
    if c_old is not None:
        bound = bound + c_old_adds * U * c_old.abs()
    return bound


def _worst(got, ref, bound):
    """max |got - ref| / bound (0 / 0 = 0)"""
    err = (got.double().cpu() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


def act_lipschitz(name, lo, hi):
    """max |act'| over [lo, hi] (float64 tensors)"""
    near0 = torch.where((lo <= 0) & (hi >= 0), torch.zeros_like(lo), torch.minimum(lo.abs(), hi.abs()))
    if name == "softplus":
        return torch.sigmoid(hi)
    if name == "tanh":
        return 1 - torch.tanh(near0) ** 2
    if name == "exp":
        return torch.exp(hi)
    if name == "sigmoid":
        return torch.sigmoid(near0) * (1 - torch.sigmoid(near0))
    return torch.ones_like(lo)  # relu


def act_bound(name, pre, pre_bound):
    """Mode 0 with an activation: the kernel applies its float32 act to a pre-activation within pre_bound of `pre`, so
    |y - act(pre)| <= allowance(act) + L pre_bound: L = max |act'| over [pre - pre_bound, pre + pre_bound], and the
    allowance of the epilogue tests (_allowed: 4 x the error of torch's float32 evaluation at the float32-rounded
    pre-activation + 1 ulp) in ulps of the largest result the interval admits (act is monotone)."""
    fn = ACTS[name][1]
    lip = act_lipschitz(name, pre - pre_bound, pre + pre_bound)
    p32 = pre.float()
    ulps = _allowed(_ulps_off(fn(p32), fn(p32.double())))
    top = torch.maximum(fn(pre - pre_bound).abs(), fn(pre + pre_bound).abs())
    return ulps * _ulp(top.float()) + lip * pre_bound


def run_gemm(c: Case, mode, splits=0, det=False, seed=0, hits=None, bias=False, act=None, results=None, zero_c=False,
             scale=1.0):
    """One ops.gemm call on guarded operands.  mode as lnrf_gemm_f32; det: the fixed-order form of mode 2; act: a key
    of ACTS (mode 0); results: a list that receives the raw result; zero_c: C starts as zeros; scale: factor on A.
    Returns (problems, worst error / bound)."""
    from learn_nerf import ops

    I, J, R = c.I, c.J, c.R
    gen = torch.Generator().manual_seed(1000 * seed + I + 7 * J + 13 * R)
    a_val, b_val = _randn(gen, I, R) * scale, _randn(gen, R, J)
    A = (Guarded(R, I, c.lda, off=c.a_off).set(a_val.T) if c.a_lay == "i" else
         Guarded(I, R, c.lda, 2 if c.a_lay == "s" else 1, c.a_off).set(a_val))
    B = (Guarded(J, R, c.ldb, off=c.b_off).set(b_val.T) if c.b_lay == "r" else
         Guarded(R, J, c.ldb, 2 if c.b_lay == "s" else 1, c.b_off).set(b_val))
    ldc = J if det else J + 136
    C = Guarded(I, J, ldc, fill=SENTINEL)
    c_old = _randn(gen, I, J) * (0.0 if zero_c else 1.0) if (mode != 0 or det) else None
    if c_old is not None:
        C.view.copy_(c_old.cuda())
    bias_v = _randn(gen, J) if bias else None
    plan = gemm_plan(*case_strides(c), I, J, R, A.low, B.low, bool(c.bf16), 3 if det else mode, splits)
    assert A.low == (4 * c.a_off) & 15 and B.low == (4 * c.b_off) & 15
    if hits is not None:
        hits.add((path_of(plan), "det" if det else mode))
        hits.add(c.name)
    with ops.dense_precision(PREC[c.bf16]):
        ops.gemm(A.ptr, *case_strides(c)[:2], B.ptr, *case_strides(c)[2:], C.ptr, ldc, I, J, R,
                 bias=None if bias_v is None else bias_v.cuda(), act=0 if act is None else ACTS[act][0], mode=2 if det else mode, splits=splits)
    torch.cuda.synchronize()
    got, guards_ok = C.take(SENTINEL)
    if results is not None:
        results.append(got)
    a64, b64 = _rounded(a_val, c.bf16), _rounded(b_val, c.bf16)
    ref = a64 @ b64
    if bias_v is not None:
        ref = ref + bias_v.double()
    if c_old is not None:
        ref = ref + c_old.double()
    bound = gemm_bound(a64, b64, ref, R, plan.nsplit, None if c_old is None else c_old.double(),
                       plan.nsplit if (mode == 2 and not det) else 1)
    if act is not None:
        bound = act_bound(act, ref, bound)
        ref = ACTS[act][1](ref)
    worst = _worst(got, ref, bound)
    problems = []
    tag = f"{c.name} I={I} J={J} R={R} mode={'det' if det else mode} splits={splits} -> {path_of(plan)} nsplit={plan.nsplit}"
    if not A.unchanged() or not B.unchanged():
        problems.append(f"{tag}: an operand buffer was written")
    if not guards_ok:
        problems.append(f"{tag}: a word of C outside I x J was written")
    if torch.isnan(got).any():
        problems.append(f"{tag}: NaN in the result (a guard word of an operand was read and used)")
    elif worst > 1.0:
        problems.append(f"{tag}: error / bound = {worst:.3g}")
    return problems, worst


def _report(name, problems, worst):
    print(f"{name}: worst error / bound {worst:.3g}")
    assert not problems, "\n".join(problems)


# ---- the path table -------------------------------------------------------------------------------------------------
def test_every_dispatch_path_matches_float64():
    """Every row of the path table (16 big instantiations, the generic kernel, the twelve fall-through neighbours, both
    precisions) in modes 0 (with bias), 1, 2 (atomics, splits = 2) and the fixed-order form; the host plan is asked
    which kernel each call takes, and at the end every path, every row and every mode has been hit."""
    assert host_lib() is not None, "liblnrf_layout_host.so not built"
    hits, problems, worst = set(), [], 0.0
    for c in PATH_TABLE:
        for mode, det in ((0, False), (1, False), (2, False), (2, True)):
            p, w = run_gemm(c, mode, splits=0 if det or mode != 2 else 2, det=det, hits=hits, bias=(mode == 0))
            problems += p
            worst = max(worst, w)
    for path in ALL_PATHS:
        for mode in (0, 1, 2, "det"):
            assert (path, mode) in hits, f"path {path} never ran in mode {mode}"
    assert all(c.name in hits for c in PATH_TABLE) and sum(c.name.startswith("nb-") for c in PATH_TABLE) == 24
    _report("path table", problems, worst)


@pytest.mark.parametrize("bf16", [0, 1])
def test_big_kernel_tile_and_chunk_edges(bf16):
    """I in {64, 132} (132: two row tiles, the second holding 4 rows), J in {64, 68, 132}, R in {32, 36, 68} (one chunk, a
    chunk plus a 4-deep tail, several chunks, at KC 16 and 32), in the three operand layouts of the dense entry points;
    R = 37 where neither operand is contiguous in r."""
    problems, worst = [], 0.0
    for I in (64, 132):
        for J in (64, 68, 132):
            for R in (32, 36, 68):
                for a_lay, b_lay, mode, det in (("r", "j", 0, False), ("r", "r", 1, False), ("i", "j", 2, True)):
                    c = make_case(f"edges-{a_lay}{b_lay}", I, J, R, a_lay, b_lay, bf16, None)
                    hits = set()
                    p, w = run_gemm(c, mode, det=det, hits=hits, bias=(mode == 0), seed=1)
                    assert any(h[0][0] == "big" for h in hits if isinstance(h, tuple))
                    problems += p
                    worst = max(worst, w)
    for b_off in (0, 3):
        for mode, det, splits in ((0, False, 0), (1, False, 0), (2, False, 2), (2, True, 0)):
            c = make_case("edges-R37", 132, 68, 37, "i", "j", bf16, None, b_off=b_off)
            hits = set()
            p, w = run_gemm(c, mode, splits=splits, det=det, hits=hits, seed=2)
            assert (("big", bf16, 0, 0, int(b_off == 0)), "det" if det else mode) in hits
            problems += p
            worst = max(worst, w)
    _report("big kernel edges", problems, worst)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("b_off", [0, 1])
def test_atomic_splits_given_by_the_caller(bf16, b_off):
    """Mode 2 with caller-given splits in {2, 5} and more splits than there are chunks (R = 68: 5 chunks of 16, 3 of 32),
    added into a random C and into C = 0."""
    problems, worst = [], 0.0
    for a_lay, b_lay in (("i", "j"), ("r", "r")):
        for splits in (2, 5, 1000):
            c = make_case(f"atomic-{a_lay}{b_lay}", 132, 68, 68, a_lay, b_lay, bf16, None, b_off=b_off)
            hits = set()
            for zero_c in (False, True):  # C = 0: the bound has no c_old term
                p, w = run_gemm(c, 2, splits=splits, hits=hits, seed=3, zero_c=zero_c)
                problems += p
                worst = max(worst, w)
            assert (("big", bf16, int(a_lay == "r"), int(b_lay == "r"), int(b_off == 0)), 2) in hits
    _report("atomic splits", problems, worst)


@pytest.mark.parametrize("bf16", [0, 1])
def test_generic_kernel_shapes_and_strides(bf16):
    """(I, J, R) = (1, 1, 1), (65, 65, 17), (64, 64, 16), (3, 130, 33) in all four modes; every operand layout,
    including operands where neither stride is 1."""
    problems, worst = [], 0.0
    for I, J, R in ((1, 1, 1), (65, 65, 17), (64, 64, 16), (3, 130, 33)):
        for a_lay, b_lay in (("r", "j"), ("i", "r"), ("s", "s"), ("r", "s"), ("s", "r")):
            for mode, det, splits in ((0, False, 0), (1, False, 0), (2, False, 3), (2, True, 0)):
                c = make_case(f"generic-{a_lay}{b_lay}", I, J, R, a_lay, b_lay, bf16, None, a_off=1 if a_lay == "s" else 0)
                hits = set()
                p, w = run_gemm(c, mode, splits=splits, det=det, hits=hits, bias=(mode == 0), seed=4)
                assert (("generic", bf16), "det" if det else mode) in hits
                problems += p
                worst = max(worst, w)
    _report("generic kernel", problems, worst)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("I", [8064, 8192, 8196])
def test_xcd_tile_order(bf16, I):
    """ni = 63 (plain order), 64 (grouped) and 65 (grouped, grid padded to 72 row tiles): every tile is computed once and
    the padding blocks touch nothing."""
    problems, worst = [], 0.0
    for J in (64, 132):
        for mode in (0, 1):
            c = make_case("tile-order", I, J, 32, "r", "j", bf16, None)
            plan = gemm_plan(*case_strides(c), I, J, 32, 0, 0, bool(bf16), mode, 0)
            ni, nj = (I + 127) // 128, (J + 127) // 128
            assert plan.big and plan.gx == (ni if ni < 64 else (ni + 7) // 8 * 8) * nj
            p, w = run_gemm(c, mode, seed=5, bias=(mode == 0))
            problems += p
            worst = max(worst, w)
    _report("tile order", problems, worst)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("name", ["relu", "softplus", "tanh", "exp", "sigmoid"])
def test_activation_on_a_real_gemm(bf16, name):
    """Mode 0 with bias and each activation on one big case (132 x 68 x 36: the epilogue of gemm_big_kernel) and one
    generic case (65 x 65 x 17), pre-activations of order 1: bound = act_bound of the GEMM bound."""
    problems, worst = [], 0.0
    for c in (make_case("act-big", 132, 68, 36, "r", "j", bf16, None), make_case("act-generic", 65, 65, 17, "r", "j", bf16, None)):
        hits = set()
        p, w = run_gemm(c, 0, bias=True, act=name, seed=6, hits=hits, scale=c.R ** -0.5)
        assert ((("big", bf16, 1, 0, 1) if c.I == 132 else ("generic", bf16)), 0) in hits
        problems += p
        worst = max(worst, w)
    _report(f"{name} on a real GEMM", problems, worst)


# ---- split reductions through the entry points ----------------------------------------------------------------------
def _wgrad_case(m, k, n, bf16, gen, gw_off):
    """x and gy as column slices of wider NaN-filled buffers, gw and gb as views at float offset 64 + gw_off / 5 floats
    behind gw of a flat sentinel-filled vector."""
    x_val, gy_val = _randn(gen, m, k), _randn(gen, m, n)
    X = Guarded(m, k, k + 136 + (m == 513)).set(x_val)  # row strides: multiples of 4 (big kernel if k, n >= 64) but for
    GY = Guarded(m, n, n + 136 + (m == 512)).set(gy_val)  # one m each
    flat = torch.full((64 + gw_off + k * n + 5 + n + 64,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    gw = flat[64 + gw_off:64 + gw_off + k * n].view(k, n)
    gb = flat[64 + gw_off + k * n + 5:64 + gw_off + k * n + 5 + n]
    return x_val, gy_val, X, GY, flat, gw, gb


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("k,n", [(64, 64), (316, 68), (60, 3), (1, 1)])
def test_weight_and_bias_gradient_split_reduction(bf16, k, n):
    """dense_bwd_weight and bias_grad at m on both sides of the 256-row split granule and of the 512-row bias block:
    parity, bit-equality of two runs, and bit-equality under poisoned workspaces (leases dense_wgrad)."""
    from learn_nerf import ops

    problems, worst, worst_b = [], 0.0, 0.0
    for m in (1, 255, 256, 257, 512, 513, 1100):
        gen = torch.Generator().manual_seed(m * 31 + k)
        gw_off = 1 + 2 * (m % 2)  # odd float offsets 1 and 3
        x_val, gy_val, X, GY, flat, gw, gb = _wgrad_case(m, k, n, bf16, gen, gw_off)
        gw_old, gb_old = _randn(gen, k, n), _randn(gen, n)
        plan = gemm_plan(1, X.view.stride(0), GY.view.stride(0), 1, k, n, m, X.low, GY.low, bool(bf16), 3, 0)

        def run(with_x=True):
            gw.copy_(gw_old.cuda())
            gb.copy_(gb_old.cuda())
            with ops.dense_precision(PREC[bf16]):
                if with_x:
                    ops.dense_bwd_weight(X.view, GY.view, gw, gb)
                else:
                    ops.bias_grad(GY.view, gb)
            torch.cuda.synchronize()
            return gw.clone(), gb.clone()

        w1, b1 = run()
        w2, b2 = run()
        _, b3 = run(with_x=False)
        gb.zero_()  # into gb = 0: (m + 2) u sum |gy| alone
        with ops.dense_precision(PREC[bf16]):
            ops.bias_grad(GY.view, gb)
        torch.cuda.synchronize()
        wb0 = _worst(gb.clone(), gy_val.double().sum(0), (m + 2) * U * gy_val.double().abs().sum(0))
        tag = f"m={m} k={k} n={n} {PREC[bf16]} nsplit={plan.nsplit} big={plan.big}"
        if not (torch.equal(_bits(w1), _bits(w2)) and torch.equal(_bits(b1), _bits(b2)) and torch.equal(_bits(b1), _bits(b3))):
            problems.append(f"{tag}: two runs differ")
        for pattern in gpu_poison.PATTERNS:
            with gpu_poison.poisoned(pattern) as rec:
                wp, bp = run()
                _, bp2 = run(with_x=False)
            assert "dense_wgrad" in rec.poisoned_purposes
            if not (torch.equal(_bits(w1), _bits(wp)) and torch.equal(_bits(b1), _bits(bp)) and torch.equal(_bits(b1), _bits(bp2))):
                problems.append(f"{tag}: result changes under workspace poison {pattern:#04x}")
        if not (X.unchanged() and GY.unchanged()):
            problems.append(f"{tag}: an operand buffer was written")
        rest = _bits(flat).clone()
        rest[64 + gw_off:64 + gw_off + k * n] = SENTINEL
        rest[64 + gw_off + k * n + 5:64 + gw_off + k * n + 5 + n] = SENTINEL
        if not bool((rest == SENTINEL).all()):
            problems.append(f"{tag}: a word next to gw / gb was written")
        x64, gy64 = _rounded(x_val, bf16), _rounded(gy_val, bf16)
        ref_w = x64.T @ gy64 + gw_old.double()
        bound_w = gemm_bound(x64.T, gy64, ref_w, m, plan.nsplit, gw_old.double())
        ref_b = gy_val.double().sum(0) + gb_old.double()  # the bias gradient sums gy as it is (fp32) in both precisions
        bound_b = (m + 2) * U * gy_val.double().abs().sum(0) + U * gb_old.double().abs()  # + the add into gb (as mode 1)
        ww, wb = _worst(w1, ref_w, bound_w), _worst(b1, ref_b, bound_b)
        if torch.isnan(w1).any() or torch.isnan(b1).any():
            problems.append(f"{tag}: NaN in the result")
        elif ww > 1 or wb > 1 or not wb0 <= 1:
            problems.append(f"{tag}: error / bound gw {ww:.3g} gb {wb:.3g} gb from zero {wb0:.3g}")
        worst, worst_b = max(worst, ww), max(worst_b, wb, wb0)
    print(f"bias gradient: worst error / bound {worst_b:.3g}")
    _report("weight gradient", problems, worst)


@pytest.mark.parametrize("bf16", [0, 1])
def test_fixed_order_gemm_under_poisoned_workspace(bf16):
    """ops.gemm mode 2 with the choice of splits left open (lnrf_gemm_f32_det, lease gemm_det): two runs and the three
    poison patterns give the same bits; R = 1100 splits 5 ways on the 64 x 64 tile."""
    c = make_case("det-poison", 64, 64, 1100, "i", "j", bf16, None)
    assert gemm_plan(*case_strides(c), 64, 64, 1100, 0, 0, bool(bf16), 3, 0).nsplit > 1
    p0, w0 = run_gemm(c, 2, det=True, seed=7)
    runs = []
    run_gemm(c, 2, det=True, seed=7, results=runs)
    for pattern in gpu_poison.PATTERNS:
        with gpu_poison.poisoned(pattern) as rec:
            run_gemm(c, 2, det=True, seed=7, results=runs)
        assert "gemm_det" in rec.poisoned_purposes
    assert len(runs) == 4 and all(torch.equal(_bits(runs[0]), _bits(r)) for r in runs[1:])
    # split partials (nsplit = 5) from the instantiations with A or B contiguous in r, B aligned or not
    for a_lay, b_lay, b_off in (("r", "r", 0), ("r", "r", 3), ("r", "j", 0), ("r", "j", 1), ("i", "r", 0), ("i", "r", 2)):
        c = make_case(f"det-{a_lay}{b_lay}", 132, 68, 1100, a_lay, b_lay, bf16, None, b_off=b_off)
        hits, two = set(), []
        p, w = run_gemm(c, 2, det=True, seed=8, hits=hits, results=two)
        run_gemm(c, 2, det=True, seed=8, results=two)
        assert (("big", bf16, int(a_lay == "r"), int(b_lay == "r"), int(b_off == 0)), "det") in hits
        assert gemm_plan(*case_strides(c), 132, 68, 1100, 0, 4 * b_off, bool(bf16), 3, 0).nsplit == 5
        assert torch.equal(_bits(two[0]), _bits(two[1]))
        p0, w0 = p0 + p, max(w0, w)
    _report("fixed-order gemm", p0, w0)


# ---- the gate -------------------------------------------------------------------------------------------------------
def _gate_derivative(y64, act):
    return (y64 > 0).double() if act == 1 else 1 - y64 * y64


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("m,k,n,g", [(132, 132, 64, 70), (132, 64, 64, 1), (65, 132, 17, 70), (65, 64, 17, 1)])
def test_gated_input_gradient(bf16, m, k, n, g):
    """dense_bwd_input(gate=) with n_gated < k cutting through a 32-column wave tile, on both kernels (n = 64: big, n = 17:
    generic), plain and accumulating, gate activations ReLU (with exact zeros) and tanh, against the float64 product
    times the float64 derivative.  The kernel multiplies the rounded sum by gm = act'(y) evaluated in fp32 (exact for
    ReLU, 1 - y y within 2u for tanh) and rounds the product: |sum| 2u + u |sum gm| on top of |gm| x the GEMM bound."""
    from learn_nerf import _lib as L
    from learn_nerf import ops

    problems, worst = [], 0.0
    gen = torch.Generator().manual_seed(m + k + g)
    for act in (L.ACT_RELU, L.ACT_TANH):
        for accumulate in (False, True):
            gy_val, w_val = _randn(gen, m, n), _randn(gen, k, n)
            y_val = torch.relu(_randn(gen, m, g)) if act == L.ACT_RELU else torch.tanh(_randn(gen, m, g))
            GY = Guarded(m, n, n + 136).set(gy_val)
            W = Guarded(k, n, n, guard_rows=GUARD_ROWS * 3).set(w_val)  # contiguous weight, NaN rows around it
            Y = Guarded(m, g, g + 139).set(y_val)
            GX = Guarded(m, k, k + 136, fill=SENTINEL)
            c_old = _randn(gen, m, k)
            GX.view.copy_(c_old.cuda())
            plan = gemm_plan(GY.view.stride(0), 1, 1, n, m, k, n, GY.low, W.low, bool(bf16), 1 if accumulate else 0, 1)
            assert plan.big == int(n == 64)
            with ops.dense_precision(PREC[bf16]):
                ops.dense_bwd_input(GY.view, W.view, out=GX.view, accumulate=accumulate, gate=Y.view, gate_act=act)
            torch.cuda.synchronize()
            got, guards_ok = GX.take(SENTINEL)
            a64, b64 = _rounded(gy_val, bf16), _rounded(w_val, bf16).T
            prod = a64 @ b64
            gm = torch.ones(m, k, dtype=F64)
            gm[:, :g] = _gate_derivative(y_val.double(), act)
            ref = prod * gm + (c_old.double() if accumulate else 0)
            bound = gm.abs() * gemm_bound(a64, b64, prod, n, 1) + prod.abs() * (2 * U if act == L.ACT_TANH else 0) \
                + U * (prod * gm).abs() + U * ref.abs() + (U * c_old.double().abs() if accumulate else 0)
            w = _worst(got, ref, bound)
            tag = f"m={m} k={k} n={n} g={g} act={act} accumulate={accumulate} {PREC[bf16]}"
            if not (GY.unchanged() and W.unchanged() and Y.unchanged()):
                problems.append(f"{tag}: an operand buffer was written")
            if not guards_ok:
                problems.append(f"{tag}: a word of gx outside m x k was written")
            if torch.isnan(got).any():
                problems.append(f"{tag}: NaN in the result")
            elif w > 1:
                problems.append(f"{tag}: error / bound = {w:.3g}")
            if act == L.ACT_RELU:  # exact zeros where the gate is closed, none elsewhere by accident
                closed = torch.zeros(m, k, dtype=torch.bool)
                closed[:, :g] = y_val == 0
                if not accumulate and not bool((got.cpu()[closed] == 0).all()):
                    problems.append(f"{tag}: a closed ReLU gate let a value through")
            worst = max(worst, w)
    _report("gated input gradient", problems, worst)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("m,k,n", [(132, 36, 68), (65, 17, 33)])
def test_gated_forward_into_a_column_slice(bf16, m, k, n):
    """dense_fwd(gate=) (tanh gate over all n columns) writing out = cat[:, de_w:], a column slice of a concatenation
    buffer: the columns in front of it and the padding behind keep their bits."""
    from learn_nerf import _lib as L
    from learn_nerf import ops

    gen = torch.Generator().manual_seed(m + n)
    de_w = 27
    x_val, w_val, b_val = _randn(gen, m, k), _randn(gen, k, n), _randn(gen, n)
    y_val = torch.tanh(_randn(gen, m, n))
    X = Guarded(m, k, k + 136).set(x_val)
    W = Guarded(k, n, n, guard_rows=GUARD_ROWS * 3).set(w_val)
    Y = Guarded(m, n, n + 137).set(y_val)
    CAT = Guarded(m, de_w + n, de_w + n + 136, fill=SENTINEL)
    out = CAT.view[:, de_w:]
    with ops.dense_precision(PREC[bf16]):
        ops.dense_fwd(X.view, W.view, b_val.cuda(), L.ACT_NONE, out=out, gate=Y.view, gate_act=L.ACT_TANH)
    torch.cuda.synchronize()
    got = out.clone()
    _bits(out).fill_(SENTINEL)
    assert bool((_bits(CAT.flat) == SENTINEL).all()), "a word outside the column slice was written"
    assert X.unchanged() and W.unchanged() and Y.unchanged()
    a64, b64 = _rounded(x_val, bf16), _rounded(w_val, bf16)
    pre = a64 @ b64 + b_val.double()
    gm = _gate_derivative(y_val.double(), L.ACT_TANH)
    ref = pre * gm
    bound = gm.abs() * gemm_bound(a64, b64, pre, k, 1) + pre.abs() * 2 * U + U * ref.abs()
    assert not torch.isnan(got).any()
    _report("gated forward", [], _worst(got, ref, bound))
    assert _worst(got, ref, bound) <= 1


# ---- weights as the models pass them --------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_weights_inside_a_flat_parameter_vector(bf16, off):
    """w = a slice of one flat fp32 vector at float offsets 0..3 (B_ALIGNED false for 1..3), forward and input gradient on
    the big kernel, and the row slice W[:hd] of a taller matrix (the rows behind it are NaN here)."""
    from learn_nerf import ops

    m, k, n, hd = 132, 36, 68, 32
    gen = torch.Generator().manual_seed(off)
    x_val, w_val, gy_val = _randn(gen, m, k), _randn(gen, k, n), _randn(gen, m, n)
    flat = torch.full((4096 + off + k * n + 4096,), float("nan"), device="cuda")
    w = flat[4096 + off:4096 + off + k * n].view(k, n)
    w.copy_(w_val.cuda())
    snap = _bits(flat).clone()
    assert (w.data_ptr() & 15) == 4 * off
    X, GY = Guarded(m, k, k + 136).set(x_val), Guarded(m, n, n + 136).set(gy_val)
    problems, worst = [], 0.0
    for rows in (k, hd):
        Yb, GXb = Guarded(m, n, n + 136, fill=SENTINEL), Guarded(m, rows, rows + 136, fill=SENTINEL)
        fwd = gemm_plan(X.view.stride(0), 1, n, 1, m, n, rows, X.low, 4 * off, bool(bf16), 0, 1)
        bwd = gemm_plan(GY.view.stride(0), 1, 1, n, m, rows, n, GY.low, 4 * off, bool(bf16), 0, 1)
        assert path_of(fwd) == ("big", bf16, 1, 0, int(off == 0))
        assert path_of(bwd) == (("big", bf16, 1, 1, int(off == 0)) if rows >= 64 else ("generic", bf16))
        with ops.dense_precision(PREC[bf16]):
            ops.dense_fwd(X.view[:, :rows], w[:rows], None, 0, out=Yb.view)
            ops.dense_bwd_input(GY.view, w[:rows], out=GXb.view)
        torch.cuda.synchronize()
        y, ok_y = Yb.take(SENTINEL)
        gx, ok_gx = GXb.take(SENTINEL)
        x64, w64, gy64 = _rounded(x_val[:, :rows], bf16), _rounded(w_val[:rows], bf16), _rounded(gy_val, bf16)
        wy = _worst(y, x64 @ w64, gemm_bound(x64, w64, x64 @ w64, rows, 1))
        wg = _worst(gx, gy64 @ w64.T, gemm_bound(gy64, w64.T, gy64 @ w64.T, n, 1))
        tag = f"off={off} rows={rows} {PREC[bf16]}"
        if not (ok_y and ok_gx and X.unchanged() and GY.unchanged() and torch.equal(_bits(flat), snap)):
            problems.append(f"{tag}: a guard word changed")
        if torch.isnan(y).any() or torch.isnan(gx).any():
            problems.append(f"{tag}: NaN in the result")
        elif wy > 1 or wg > 1:
            problems.append(f"{tag}: error / bound fwd {wy:.3g} bwd {wg:.3g}")
        worst = max(worst, wy, wg)
    _report("flat-vector weights", problems, worst)


@pytest.mark.parametrize("bf16", [0, 1])
def test_input_gradient_big_kernel_with_unaligned_weight(bf16):
    """dense_bwd_input with k >= 64 (B contiguous in r) and w at float offsets 0..3: the instantiations <.., true, true, *>
    as the entry point reaches them."""
    from learn_nerf import ops

    m, k, n = 68, 132, 36
    problems, worst = [], 0.0
    for off in (0, 1, 2, 3):
        gen = torch.Generator().manual_seed(10 + off)
        w_val, gy_val = _randn(gen, k, n), _randn(gen, m, n)
        flat = torch.full((8192 + off + k * n + 8192,), float("nan"), device="cuda")
        w = flat[8192 + off:8192 + off + k * n].view(k, n)
        w.copy_(w_val.cuda())
        GY, GX = Guarded(m, n, n + 136).set(gy_val), Guarded(m, k, k + 136, fill=SENTINEL)
        plan = gemm_plan(GY.view.stride(0), 1, 1, n, m, k, n, GY.low, 4 * off, bool(bf16), 0, 1)
        assert path_of(plan) == ("big", bf16, 1, 1, int(off == 0))
        with ops.dense_precision(PREC[bf16]):
            ops.dense_bwd_input(GY.view, w, out=GX.view)
        torch.cuda.synchronize()
        gx, ok = GX.take(SENTINEL)
        gy64, w64 = _rounded(gy_val, bf16), _rounded(w_val, bf16)
        wg = _worst(gx, gy64 @ w64.T, gemm_bound(gy64, w64.T, gy64 @ w64.T, n, 1))
        if not ok or not GY.unchanged() or torch.isnan(gx).any() or wg > 1:
            problems.append(f"off={off}: guards {ok} nan {bool(torch.isnan(gx).any())} error / bound {wg:.3g}")
        worst = max(worst, wg)
    _report("unaligned weight, input gradient", problems, worst)


# ---- epilogue functions ---------------------------------------------------------------------------------------------
_GRID = [0.0, 1e-8, 1e-4, 0.5, 5.0, 17.0, 40.0, 88.0, 89.0, 104.0, 200.0]
ACTS = {"relu": (1, torch.relu), "softplus": (2, torch.nn.functional.softplus), "tanh": (3, torch.tanh),
        "exp": (4, torch.exp), "sigmoid": (5, torch.sigmoid)}


def _grid():
    g = torch.tensor(_GRID, dtype=torch.float32)
    return torch.cat([g, -g])


def _ulp(ref32):
    """spacing of float32 at ref32 (towards larger magnitude; the smallest subnormal at 0)"""
    a = torch.where(torch.isfinite(ref32), ref32.abs(), torch.zeros_like(ref32)).numpy()
    return torch.from_numpy((np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64))


def _ulps_off(got32, ref64):
    """error in ulps of the float32-rounded reference; equal infinities and exact hits count 0, a wrong infinity inf"""
    ref32 = ref64.float()
    err = (got32.double() - ref64).abs()
    same = got32 == ref32
    fin = torch.isfinite(ref32) & torch.isfinite(got32)
    out = torch.full_like(ref64, float("inf"))
    out[same] = 0.0
    sel = fin & ~same
    out[sel] = err[sel] / _ulp(ref32)[sel]
    return out


def _allowed(e32):
    """Per grid point, from torch's float32 error e32 (ulps) on the grid: 4 x that + 1 ulp, where "that" is the error
    at the point itself (cancellation, a subnormal result flushed to zero) or else the worst error on the grid, but no
    more than the 0.5 ulp of a correctly rounded evaluation: never more than 4 x the worst error on the grid + 1."""
    return 4 * torch.maximum(e32, torch.full_like(e32, min(0.5, float(e32.max())))) + 1


def _report_ulps(what, e32, off, allowed):
    normal = e32 <= 0.5
    print(f"{what}: torch float32 CPU {float(e32.max()):.2f} ulp, kernel {float(off.max()):.2f} ulp; where torch is "
          f"within 0.5 ulp: kernel {float(off[normal].max()):.2f} ulp, allowed {float(allowed[normal].max()):.2f}")


@pytest.mark.parametrize("name", list(ACTS))
def test_epilogue_activation_on_the_grid(name):
    """act(x) through a K = 1, w = [[1]] GEMM (generic kernel, mode 0), so the pre-activation is exactly x: overflow gives
    the inf of the float64 result rounded to float32, saturated sigmoid / tanh / softplus are exact."""
    from learn_nerf import ops

    act, fn = ACTS[name]
    x = _grid()
    X = Guarded(x.numel(), 1, 140).set(x[:, None])
    Y = Guarded(x.numel(), 1, 140, fill=SENTINEL)
    ops.dense_fwd(X.view, torch.ones(1, 1, device="cuda"), None, act, out=Y.view)
    torch.cuda.synchronize()
    got, ok = Y.take(SENTINEL)
    got = got.cpu()[:, 0]
    ref64 = fn(x.double())
    ref32 = ref64.float()
    e32 = _ulps_off(fn(x), ref64)
    allowed = _allowed(e32)
    off = _ulps_off(got, ref64)
    _report_ulps(name, e32, off, allowed)
    assert ok and X.unchanged()
    assert torch.equal(torch.isinf(got), torch.isinf(ref32)) and not torch.isnan(got).any()
    sat = {"sigmoid": (ref32 == 0) | (ref32 == 1), "tanh": ref32.abs() == 1, "softplus": (ref32 == 0) | (ref32 == x),
           "relu": torch.ones_like(x, dtype=torch.bool), "exp": torch.isinf(ref32) | (ref32 == 0) | (ref32 == 1)}[name]
    assert torch.equal(got[sat], ref32[sat]), f"{name}: saturated values differ: {got[sat]} vs {ref32[sat]}"
    assert bool((off <= allowed).all()), f"{name}: {off} ulp at {x}, allowed {allowed}"


@pytest.mark.parametrize("name", list(ACTS))
def test_activation_derivatives_from_outputs(name):
    """act_bwd_ and the gate derivative on the outputs the grid produces (y = 0, y = 1, y = inf for exp): g' = g * act'(y)
    with g = 1 (act_bwd_) and through a K = 1 gated GEMM whose product is exactly 1."""
    from learn_nerf import ops

    act, fn = ACTS[name]
    x = _grid()
    y = fn(x.double()).float()  # the outputs a correct forward produces
    y64 = y.double()
    deriv = {"relu": lambda v: (v > 0).double(), "softplus": lambda v: -torch.expm1(-v), "tanh": lambda v: 1 - v * v,
             "exp": lambda v: v, "sigmoid": lambda v: v * (1 - v)}[name]
    ref64 = deriv(y64)
    e32 = _ulps_off(deriv(y).float(), ref64)
    allowed = _allowed(e32)
    Yb = Guarded(y.numel(), 1, 140).set(y[:, None])
    G = Guarded(y.numel(), 1, 140, fill=SENTINEL)
    G.view.fill_(1.0)
    ops.act_bwd_(G.view, Yb.view, act)
    ones = Guarded(y.numel(), 1, 140).set(torch.ones(y.numel(), 1))
    GX = Guarded(y.numel(), 1, 140, fill=SENTINEL)
    ops.dense_bwd_input(ones.view, torch.ones(1, 1, device="cuda"), out=GX.view, gate=Yb.view, gate_act=act)
    torch.cuda.synchronize()
    for what, buf in (("act_bwd_", G), ("gate", GX)):
        got, ok = buf.take(SENTINEL)
        got = got.cpu()[:, 0]
        off = _ulps_off(got, ref64)
        _report_ulps(f"{name} {what}", e32, off, allowed)
        assert ok and Yb.unchanged() and not torch.isnan(got).any()
        assert bool((off <= allowed).all()), f"{name} {what}: {off} ulp for y = {y}, allowed {allowed}"


@pytest.mark.parametrize("dims,freqs", [(1, 1), (4, 1), (1, 16), (4, 16)])
def test_sinusoidal_emb(dims, freqs):
    """lnrf_sinusoidal_emb with a strided x, col_off > 0 and guard columns, against float64 sin / cos of the exactly
    representable 2^f x; allowance as for the epilogue functions, per element in ulps of the result (_allowed)."""
    from learn_nerf import ops

    m, col_off = 67, 5
    gen = torch.Generator().manual_seed(dims + freqs)
    x = torch.rand(m, dims, generator=gen) * 2 - 1
    x[0] = 0.0
    x[1] = 1.0
    X = Guarded(m, dims, dims + 139).set(x)
    width = dims * 2 * freqs
    O = Guarded(m, col_off + width, col_off + width + 137, fill=SENTINEL)
    ops.sinusoidal_emb_into(X.view, freqs, O.view, col_off=col_off)
    torch.cuda.synchronize()
    got = O.view[:, col_off:].clone()
    _bits(O.view[:, col_off:]).fill_(SENTINEL)
    assert bool((_bits(O.flat) == SENTINEL).all()) and X.unchanged()
    scale = 2.0 ** torch.arange(freqs, dtype=F64)
    arg = x.double()[:, :, None] * scale  # exact in fp32 as well
    assert torch.equal(arg, (x[:, :, None] * scale.float()).double())
    ref = torch.cat([torch.sin(arg), torch.cos(arg)], -1).reshape(m, width)
    t32 = torch.cat([torch.sin(arg.float()), torch.cos(arg.float())], -1).reshape(m, width)
    e32 = _ulps_off(t32, ref)
    allowed = _allowed(e32)
    off = _ulps_off(got.cpu(), ref)
    _report_ulps(f"sinusoidal_emb dims={dims} freqs={freqs}", e32.flatten(), off.flatten(), allowed.flatten())
    assert not torch.isnan(got).any()
    assert bool((off <= allowed).all()), f"worst {float((off / allowed).max()):.3g} x the allowance"

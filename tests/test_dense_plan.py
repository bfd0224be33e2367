"""
CPU check of the dispatch plan of the generic dense GEMM (csrc/dense_plan.h, compiled for the host into
liblnrf_layout_host.so): the function launch_gemm launches from, the split counts the scratch blocks are sized for, and the
blockIdx -> tile map of gemm_big_kernel.  No GPU involved.

PATH_TABLE is the list of operand descriptions the GPU parity test (test_gpu_gemm_paths.py) drives: all 16
gemm_big_kernel instantiations, the generic kernel in both precisions, and for each of the conditions of the big-path
predicate the nearest neighbour that fails only that condition.
"""
import collections
import ctypes
import itertools
import os

import numpy as np
import pytest

from test_nerf_layout import HOST_LIB

PLAN_FIELDS = ("launch", "big", "bf16", "a_fast_r", "b_fast_r", "b_aligned", "kc", "nsplit", "lda", "ldb", "per", "gx",
               "gy", "gz", "asked")
Plan = collections.namedtuple("Plan", PLAN_FIELDS)

_LIB = None


def host_lib():
    """The host library with the dense-plan entry points typed; None if it has not been built."""
    global _LIB
    if _LIB is None and os.path.exists(HOST_LIB):
        lib = ctypes.CDLL(HOST_LIB)
        i64, i32, u32 = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32
        lib.lnrf_host_gemm_plan.argtypes = [i64, i64, i64, i64, i64, i32, i64, u32, u32, i32, i32, i32, ctypes.c_void_p]
        lib.lnrf_host_gemm_plan.restype = None
        lib.lnrf_host_gemm_tile.argtypes = [i64, i32, u32, i64, ctypes.c_void_p]
        lib.lnrf_host_gemm_tile.restype = None
        lib.lnrf_host_dense_bwd_weight_scratch_bytes.argtypes = [i64, i32, i32]
        lib.lnrf_host_dense_bwd_weight_scratch_bytes.restype = i64
        lib.lnrf_host_gemm_det_scratch_bytes.argtypes = [i64, i32, i64]
        lib.lnrf_host_gemm_det_scratch_bytes.restype = i64
        _LIB = lib
    return _LIB


_OUT = np.zeros(len(PLAN_FIELDS), np.int64)


def gemm_plan(sa_i, sa_r, sb_r, sb_j, I, J, R, a_low=0, b_low=0, bf16=False, mode=0, splits=0) -> Plan:
    """gemm_plan of dense_plan.h; a_low / b_low = low 4 bits of the operand addresses, mode 3 = split partials."""
    host_lib().lnrf_host_gemm_plan(sa_i, sa_r, sb_r, sb_j, I, J, R, a_low, b_low, int(bf16), mode, splits, _OUT.ctypes.data)
    return Plan(*(int(v) for v in _OUT))


def path_of(p: Plan):
    """("big", bf16, a_fast_r, b_fast_r, b_aligned) or ("generic", bf16): the kernel instantiation a plan launches."""
    return ("big", p.bf16, p.a_fast_r, p.b_fast_r, p.b_aligned) if p.big else ("generic", p.bf16)


@pytest.fixture(scope="module")
def H():
    if host_lib() is None:
        pytest.skip("liblnrf_layout_host.so not built (run __graft_entry__.build())")
    return host_lib()


# ---- the path table -----------------------------------------------------------------------------------------------
# One operand description: extents, the layout of A ("r": contiguous in r, "i": contiguous in i, "s": neither, element
# stride 2 along r) and of B ("j": contiguous in j, "r": contiguous in r, "s": neither, element stride 2 along j), the
# leading dimensions (stride of the other dimension), the float offsets of the two pointers from a 16-byte boundary,
# the precision, and the kernel it has to take.  The leading dimensions leave room for the guard zones of the GPU test
# (a full tile plus a float4 beyond the extent).
Case = collections.namedtuple("Case", "name I J R a_lay b_lay lda ldb a_off b_off bf16 expect why")
GUARD_PAD = 136


def _ld(extent, elem_stride=1, extra=0):
    return (extent * elem_stride + GUARD_PAD + 3) // 4 * 4 + extra


def make_case(name, I, J, R, a_lay, b_lay, bf16, expect, why="", lda_extra=0, ldb_extra=0, a_off=0, b_off=0):
    lda = _ld(R, 2 if a_lay == "s" else 1, lda_extra) if a_lay in "rs" else _ld(I, 1, lda_extra)
    ldb = _ld(J, 2 if b_lay == "s" else 1, ldb_extra) if b_lay in "js" else _ld(R, 1, ldb_extra)
    return Case(name, I, J, R, a_lay, b_lay, lda, ldb, a_off, b_off, int(bf16), expect, why)


def case_strides(c: Case):
    """(sa_i, sa_r, sb_r, sb_j) of lnrf_gemm_f32 for a case."""
    sa = {"r": (c.lda, 1), "i": (1, c.lda), "s": (c.lda, 2)}[c.a_lay]
    sb = {"j": (c.ldb, 1), "r": (1, c.ldb), "s": (c.ldb, 2)}[c.b_lay]
    return sa + sb


def case_plan(c: Case, mode=0, splits=0, a_low=None, b_low=None) -> Plan:
    a_low = (4 * c.a_off) & 15 if a_low is None else a_low
    b_low = (4 * c.b_off) & 15 if b_low is None else b_low
    return gemm_plan(*case_strides(c), c.I, c.J, c.R, a_low, b_low, bool(c.bf16), mode, splits)


def _path_table():
    rows = []
    # the 16 instantiations; I, J ragged against the 128-tile, R = one chunk + a 4-deep tail at either chunk depth
    for bf16, a_lay, b_lay, b_off in itertools.product((0, 1), "ri", "rj", (0, 1)):
        rows.append(make_case(f"big-{'bf16' if bf16 else 'fp32'}-a{a_lay}-b{b_lay}-{'unal' if b_off else 'al'}", 132, 68, 36,
                              a_lay, b_lay, bf16, ("big", bf16, int(a_lay == "r"), int(b_lay == "r"), int(b_off == 0)),
                              b_off=b_off))
    for bf16 in (0, 1):
        g = ("generic", bf16)
        p = "bf16" if bf16 else "fp32"
        rows += [
            make_case(f"generic-{p}", 65, 65, 17, "r", "j", bf16, g, "small and ragged"),
            # nearest neighbours of the big path: each fails exactly one condition of the predicate
            make_case(f"nb-{p}-I63", 63, 64, 32, "r", "r", bf16, g, "I >= 64"),
            make_case(f"nb-{p}-J63", 64, 63, 32, "r", "r", bf16, g, "J >= 64"),
            make_case(f"nb-{p}-R28", 64, 64, 28, "r", "j", bf16, g, "R >= 32"),
            make_case(f"nb-{p}-lda", 64, 64, 32, "r", "j", bf16, g, "lda % 4 == 0", lda_extra=1),
            make_case(f"nb-{p}-ldb", 64, 64, 32, "r", "j", bf16, g, "ldb % 4 == 0", ldb_extra=1),
            make_case(f"nb-{p}-a-off1", 64, 64, 32, "r", "j", bf16, g, "a 16-byte aligned", a_off=1),
            make_case(f"nb-{p}-I66-ai", 66, 64, 32, "i", "j", bf16, g, "I % 4 == 0 with A contiguous in i"),
            make_case(f"nb-{p}-J66-bj", 64, 66, 32, "r", "j", bf16, g, "J % 4 == 0 with B contiguous in j"),
            make_case(f"nb-{p}-R34-ar", 64, 64, 34, "r", "j", bf16, g, "R % 4 == 0 with A contiguous in r"),
            make_case(f"nb-{p}-R34-ai-br", 64, 64, 34, "i", "r", bf16, g, "R % 4 == 0 with B contiguous in r"),
            make_case(f"nb-{p}-a-strided", 64, 64, 32, "s", "j", bf16, g, "A contiguous in one dimension"),
            make_case(f"nb-{p}-b-strided", 64, 64, 32, "r", "s", bf16, g, "B contiguous in one dimension"),
        ]
    return tuple(rows)


PATH_TABLE = _path_table()
ALL_PATHS = frozenset([("big",) + f for f in itertools.product((0, 1), repeat=4)] + [("generic", 0), ("generic", 1)])
SPLITS = (0, 1, 2, 3, 7, 64, 512, 1000)


def test_path_table_takes_the_expected_kernels(H):
    assert {c.expect for c in PATH_TABLE} == ALL_PATHS  # 16 big instantiations + the generic kernel twice
    assert len({c.name for c in PATH_TABLE}) == len(PATH_TABLE)
    for c in PATH_TABLE:
        p = case_plan(c)
        assert path_of(p) == c.expect, (c, p)
        if p.big:
            assert (p.lda, p.ldb, p.kc) == (c.lda, c.ldb, 32 if c.bf16 else 16)


def test_neighbours_fail_exactly_one_condition(H):
    """Undoing the one thing a neighbour has wrong puts it on the big path: nothing else keeps it off."""
    fix = {
        "I >= 64": dict(I=64), "J >= 64": dict(J=64), "R >= 32": dict(R=32),
        "a 16-byte aligned": dict(a_off=0), "I % 4 == 0 with A contiguous in i": dict(I=68),
        "J % 4 == 0 with B contiguous in j": dict(J=68), "R % 4 == 0 with A contiguous in r": dict(R=36),
        "R % 4 == 0 with B contiguous in r": dict(R=36), "A contiguous in one dimension": dict(a_lay="r"),
        "B contiguous in one dimension": dict(b_lay="j"),
    }
    seen = set()
    for c in PATH_TABLE:
        if not c.name.startswith("nb-"):
            continue
        seen.add(c.why)
        if c.why == "lda % 4 == 0":
            fixed = c._replace(lda=c.lda - 1)
        elif c.why == "ldb % 4 == 0":
            fixed = c._replace(ldb=c.ldb - 1)
        else:
            fixed = c._replace(**fix[c.why])
        assert not case_plan(c).big and case_plan(fixed).big, c
    assert len(seen) == 12


def _check_split_plan(p: Plan, R, asked):
    per, ns = p.per, p.nsplit
    assert p.launch and ns >= 1 and per >= 1 and (p.gz == ns)
    # the ranges [z per, min((z + 1) per, R)) for z < nsplit: contiguous by construction, so they partition [0, R) iff
    # the last one reaches R, and none is empty iff the last one starts below R
    assert ns * per >= R and (ns - 1) * per < R, (p, R)
    assert per % p.kc == 0, (p, R)
    if p.big:
        assert per % 4 == 0 and p.kc == (32 if p.bf16 else 16)
    else:
        assert p.kc == 16
    assert ns <= max(asked, 1), (p, R, asked)


def test_split_plans_partition_the_reduction(H):
    """R in 1..700 x requested splits x precision x kernel, as atomics (mode 2) and as split partials (mode 3)."""
    n = 0
    for R in range(1, 701):
        for bf16 in (False, True):
            for big in (False, True):
                # weight-gradient layout (A contiguous in i, B in j): no condition on R but R >= 32
                I, J = (64, 64) if big else (8, 8)
                for mode in (2, 3):
                    for s in SPLITS:
                        p = gemm_plan(1, I, J, 1, I, J, R, 0, 0, bf16, mode, s)
                        assert p.big == int(big and R >= 32) and p.bf16 == int(bf16)
                        _check_split_plan(p, R, p.asked if s <= 0 else s)
                        n += 1
                for mode in (0, 1):  # never split
                    p = gemm_plan(1, I, J, 1, I, J, R, 0, 0, bf16, mode, 7)
                    assert p.nsplit == 1 and p.per >= R and p.per % p.kc == 0
    assert n == 700 * 2 * 2 * 2 * len(SPLITS)


@pytest.mark.parametrize("bf16", [False, True])
def test_splits_fit_the_scratch_they_are_sized_for(H, bf16):
    """The split partials (mode 3) of lnrf_dense_bwd_weight_det and lnrf_gemm_f32_det go to a scratch block sized by the
    *_scratch_bytes functions from the extents alone; the plan (which also sees strides and alignment) must never launch
    more splits than that."""
    depths = list(range(1, 701)) + [1100, 4096, 65_537, 131_072, 1_000_003]
    for (k, n_), m in itertools.product([(64, 64), (316, 68), (60, 3), (1, 1), (256, 256), (8, 8)], depths):
        bias_parts = (m + 511) // 512 * n_
        nbytes = H.lnrf_host_dense_bwd_weight_scratch_bytes(m, k, n_)
        sized = ((nbytes - 256) // 4 - bias_parts) // (k * n_)
        assert ((nbytes - 256) // 4 - bias_parts) % (k * n_) == 0 and 1 <= sized <= 512
        for ldx, ldgy, a_low, b_low in [(k, n_, 0, 0), (k + 4, n_ + 4, 0, 4), (k + 1, n_ + 3, 4, 12)]:
            p = gemm_plan(1, ldx, ldgy, 1, k, n_, m, a_low, b_low, bf16, 3, 0)  # x^T gy as launch_gemm gets it
            _check_split_plan(p, m, sized)
        nbytes = H.lnrf_host_gemm_det_scratch_bytes(k, n_, m)
        sized = (nbytes - 256) // 4 // (k * n_)
        assert 1 <= sized <= 512
        for sa, sb in [((m, 1), (n_, 1)), ((1, k), (1, m)), ((m + 1, 1), (n_, 1))]:
            _check_split_plan(gemm_plan(*sa, *sb, k, n_, m, 0, 0, bf16, 3, 0), m, sized)
    assert H.lnrf_host_dense_bwd_weight_scratch_bytes(1000, 0, 5) == 256 + 4 * 2 * 5  # bias only


def test_tile_map_covers_every_tile_once(H):
    """ni in 1..200 (plain order below 64 row tiles, XCD-grouped from 64 on, grid padded to a multiple of 8), nj in 1..5."""
    for ni, nj in itertools.product(range(1, 201), range(1, 6)):
        I, J = ni * 128 - 4, nj * 128 - 60  # ragged last tiles
        p = gemm_plan(32, 1, J, 1, I, J, 32)
        assert p.big and p.gy == 1
        assert p.gx == (ni if ni < 64 else (ni + 7) // 8 * 8) * nj
        tiles = np.zeros((p.gx, 2), np.int64)
        H.lnrf_host_gemm_tile(I, J, 0, p.gx, tiles.ctypes.data)
        it, jt = tiles[:, 0], tiles[:, 1]
        assert it.min() >= 0 and jt.min() >= 0
        real = (it < ni) & (jt < nj)
        count = np.zeros((ni, nj), np.int64)
        np.add.at(count, (it[real], jt[real]), 1)
        assert (count == 1).all(), (ni, nj)
        # the padding blocks leave at the kernel's `i0 >= I || jt >= nj`
        assert ((it[~real] * 128 >= I) | (jt[~real] >= nj)).all()
        assert real.sum() == ni * nj

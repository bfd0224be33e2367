"""
CPU check of the hash grid's host arithmetic (csrc/hashgrid_plan.h, compiled for the host into liblnrf_layout_host.so):
the cell geometry the kernels share (corner indices, trilinear weights and their derivatives) against the oracle, the
XCD plan of the gather and the bucket plan of the scatter walked through the decodes the kernels read them with, and the
layout of the scatter's scratch block.  No GPU involved.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_nerf_layout import HOST_LIB

from learn_nerf import _lib as L
from oracle import instant_ngp as ON

# the level set of test_gpu_per_sample_kernels.py: dense and hashed levels, tables that are no power of two
GRIDS = [4, 16, 20, 24, 48, 64]
TABLES = [4096, 4096, 8000, 5000, 12289, 16384]
U = 2.0 ** -24  # unit roundoff of fp32

i32, i64, u32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p
_LIB = None


@pytest.fixture(scope="module")
def H():
    global _LIB
    if not os.path.exists(HOST_LIB):
        pytest.skip("liblnrf_layout_host.so not built (run __graft_entry__.build())")
    if _LIB is None:
        lib = ctypes.CDLL(HOST_LIB)
        lib.lnrf_host_hashgrid_corners.argtypes = [vp, i32, vp, vp, vp, vp]
        lib.lnrf_host_hashgrid_corners.restype = None
        lib.lnrf_host_hashgrid_xcd_plan.argtypes = [vp, vp, i32, i64, vp, vp]
        lib.lnrf_host_hashgrid_xcd_plan.restype = i64
        lib.lnrf_host_hashgrid_bucket_plan.argtypes = [vp, i64, vp, vp]
        lib.lnrf_host_hashgrid_bucket_plan.restype = i32
        lib.lnrf_host_hashgrid_reduce_work.argtypes = [vp, i64, i32, i64, i64, vp]
        lib.lnrf_host_hashgrid_reduce_work.restype = None
        _LIB = lib
    return _LIB


def make_desc(grids, tables, smooth=False, bmin=(0.0, 0.0, 0.0), bmax=(1.0, 1.0, 1.0)):
    """The descriptor MultiresHashTableEncoding.desc() builds, without the model around it."""
    d = L.HashGridDesc()
    d.n_levels, d.feature_dim, d.smooth = len(grids), 2, int(smooth)
    for a in range(3):
        d.bbox_min[a], d.bbox_max[a] = bmin[a], bmax[a]
    off = 0
    for l, (g, t) in enumerate(zip(grids, tables)):
        rows, hashed = ON.level_rows(g, t)
        d.grid_size[l], d.table_size[l], d.table_offset[l], d.hashed[l] = g, rows, off, int(hashed)
        off += 2 * rows
    return d


# ---- geometry -----------------------------------------------------------------------------------------------------

def lattice_points():
    """Points k / 1024 of the unit box: (G - 1) k / 1024 and 0.5 + (G - 2) k / 1024 have at most 17 significant bits for
    G <= 64, so the cell coordinate, its floor and the fraction c (a multiple of 2^-10) are exact in fp32.  With them:
    points on every face, corners of the box, and points outside it on one, two and three axes (clamped: exact too)."""
    gen = torch.Generator().manual_seed(17)
    x = torch.randint(0, 1025, (200, 3), generator=gen).double() / 1024.0
    extra = torch.tensor([[0.0, 0.5, 0.25], [0.5, 1.0, 0.25], [0.25, 0.5, 0.0], [1.0, 0.125, 0.5], [0.0, 0.0, 0.0],
                          [1.0, 1.0, 1.0], [0.0, 1.0, 0.5], [-0.25, 0.5, 0.75], [0.5, 1.5, 0.75], [0.5, 0.25, -3.0],
                          [2.0, -1.0, 0.5], [-8.0, 9.0, 1.25], [1.0, 2.0, 0.0]], dtype=torch.float64)
    return torch.cat([x, extra])


def geometry64(x, g, smooth):
    """float64: floored cell [m,3], fraction c [m,3] (after the smoothstep) and d c / d x [m,3] of the unit box."""
    frac = torch.clamp(x, 0, 1)
    scale = g - 2 if smooth else g - 1
    fi = 0.5 + scale * frac if smooth else scale * frac
    fl = torch.clamp(torch.floor(fi), max=g - 2)
    c = fi - fl
    dc = torch.full_like(c, float(scale))
    if smooth:
        dc = dc * 6 * c * (1 - c)
        c = c * c * (3 - 2 * c)
    inside = (x > 0) & (x < 1)
    return fl.to(torch.int64), c, torch.where(inside, dc, torch.zeros_like(dc))


@pytest.mark.parametrize("smooth", [False, True])
def test_corners_match_the_oracle(H, smooth):
    """Indices exactly, weights and weight derivatives within a bound counted from the fp32 roundings of locate and
    corner_weight / corner_weight_grad (u = 2^-24; the inputs are exact, see lattice_points; the host build may fuse a
    multiply-add, which only removes a rounding):
      factor f = c or 1 - c.  plain: c exact, 1 - c at most one rounding of a value <= 1: |df| <= 1 u.
        smooth: c*c (u), 3 - 2c in [1, 3] (2 u), their product <= 1 (3 u + 2 u + u = 6 u), 1 - c (u): |df| <= 7 u.
      weight = f f f <= 1: two products, |dw| <= 3 |df| + 2 u, one more u for the second-order terms and the reference.
      slope S: plain (G - 1) / extent, one rounding of the extent and one of the division: |dS| <= 2 u S_max with
        S_max = G - 1.  smooth: (G - 2) / extent times 6 c (1 - c) <= 1.5: 6c (u of <= 6), (1 - c) (u), product
        (6 u + 6 u + 1.5 u), times the slope (2 u + u of the result): |dS| <= (13.5 + 4.5) u (G - 2) = 12 u S_max with
        S_max = 1.5 (G - 2).
      derivative = +-S f f: |d| <= (dS / S_max + 2 |df| + 2) u S_max, one more u S_max as above."""
    df = 7 if smooth else 1
    tol_w = (3 * df + 2 + 1) * U
    ds = 12 if smooth else 2
    x = lattice_points()
    desc = make_desc(GRIDS, TABLES, smooth)
    xf = x.float().contiguous()
    assert torch.equal(xf.double(), x)
    m = x.shape[0]
    xn = xf.numpy()
    on_or_out = ~((x > 0) & (x < 1))  # [m,3]: on a face or outside along that axis
    assert on_or_out.any(dim=0).all() and (~on_or_out).any()
    for level, (g, t) in enumerate(zip(GRIDS, TABLES)):
        rows, hashed = ON.level_rows(g, t)
        base, c, dc = geometry64(x, g, smooth)
        s_max = 1.5 * (g - 2) if smooth else float(g - 1)
        tol_dw = (ds + 2 * df + 2 + 1) * U * s_max
        idx, w, dw = np.zeros((m, 8), np.uint32), np.zeros((m, 8), np.float32), np.zeros((m, 8, 3), np.float32)
        for n in range(m):
            H.lnrf_host_hashgrid_corners(ctypes.byref(desc), level, xn[n].ctypes.data, idx[n].ctypes.data,
                                         w[n].ctypes.data, dw[n].ctypes.data)
        idx, w, dw = (torch.from_numpy(v.astype(np.float64 if v.dtype == np.float32 else np.int64)) for v in (idx, w, dw))
        for corner in range(8):
            off = torch.tensor([corner >> 2, (corner >> 1) & 1, corner & 1])  # xo outermost
            coords = base + off
            want = (ON.hash_table_lookup_index(coords, rows) if hashed
                    else coords[:, 0] + g * (coords[:, 1] + g * coords[:, 2]))
            assert torch.equal(idx[:, corner], want), (level, corner)
            f = torch.where(off == 1, c, 1 - c)  # [m,3]
            err = (w[:, corner] - f.prod(dim=1)).abs().max().item()
            assert err <= tol_w, (level, corner, err / U)
            for a in range(3):
                want_d = torch.where(off[a] == 1, dc[:, a], -dc[:, a]) * f[:, (a + 1) % 3] * f[:, (a + 2) % 3]
                err = (dw[:, corner, a] - want_d).abs().max().item()
                assert err <= tol_dw, (level, corner, a, err / (U * s_max))
                assert (dw[:, corner, a][on_or_out[:, a]] == 0.0).all(), "on a face or outside: exactly zero"


# ---- plans --------------------------------------------------------------------------------------------------------
# 1, 6, 16 and 32 levels; costs of the gather mixed: dense (12), hashed with <= 4, <= 32 and more cells per entry
LEVEL_SETS = {
    1: ([64], [2 ** 14]),
    6: (GRIDS, TABLES),
    16: ([2 ** (4 + i // 2) for i in range(16)], [2 ** 19] * 16),
    32: ([4 + 13 * i for i in range(32)], [2 ** (12 + (5 * i) % 9) for i in range(32)]),
}


def test_level_sets_mix_the_costs():
    for n, (grids, tables) in LEVEL_SETS.items():
        if n == 1:
            continue
        kinds = set()
        for g, t in zip(grids, tables):
            rows, hashed = ON.level_rows(g, t)
            cells = g ** 3 / rows
            kinds.add(0 if not hashed else 1 if cells <= 4 else 2 if cells <= 32 else 3)
        assert len(kinds) >= 3, (n, kinds)


@pytest.mark.parametrize("n_levels", sorted(LEVEL_SETS))
@pytest.mark.parametrize("m", [1, 255, 256, 257, 4095, 65536, 786432])
def test_xcd_plan_covers_every_chunk_once(H, n_levels, m):
    desc = make_desc(*LEVEL_SETS[n_levels])
    levels = np.arange(n_levels, dtype=np.int32)[::-1].copy() if n_levels == 6 else np.arange(n_levels, dtype=np.int32)
    plan = np.zeros(9 + 3 * (32 + 8), np.int32)
    grid = H.lnrf_host_hashgrid_xcd_plan(ctypes.byref(desc), levels.ctypes.data, n_levels, m, plan.ctypes.data, None)
    assert grid > 0 and grid % 8 == 0
    work = np.zeros((grid, 2), np.int64)
    assert H.lnrf_host_hashgrid_xcd_plan(ctypes.byref(desc), levels.ctypes.data, n_levels, m, None,
                                         work.ctypes.data) == grid
    chunks = (m + 255) // 256
    first_seg = plan[:9]
    segs = plan[9:9 + 3 * first_seg[8]].reshape(-1, 3)  # level, first chunk, chunks
    assert (np.diff(first_seg) >= 0).all() and first_seg[0] == 0
    slots = [int(segs[first_seg[x]:first_seg[x + 1], 2].sum()) for x in range(8)]
    assert grid == 8 * max(slots)
    order = {int(l): i for i, l in enumerate(levels)}  # position of a level in the list = order of the sweep
    keys = []
    for x in range(8):
        wx = work[x::8]
        valid = wx[:, 0] >= 0
        assert int(valid.sum()) == slots[x]
        assert valid[:slots[x]].all(), "the blocks of an XCD without work come last"
        lv, m0 = wx[valid, 0], wx[valid, 1]
        assert (m0 % 256 == 0).all() and (m0 < m).all()
        k = np.array([order[int(l)] for l in lv], np.int64) * chunks + m0 // 256
        assert (np.diff(k) == 1).all(), "an XCD sweeps its piece of the line in order"
        # ... and through the segments of the plan, one after the other
        want = np.concatenate([order[int(s[0])] * chunks + s[1] + np.arange(s[2])
                               for s in segs[first_seg[x]:first_seg[x + 1]]] or [np.zeros(0, np.int64)])
        assert np.array_equal(k, want)
        keys.append(k)
    keys = np.sort(np.concatenate(keys))
    assert np.array_equal(keys, np.arange(n_levels * chunks)), "every (level, chunk) exactly once"


def bucket_plan(H, desc, m):
    levels = np.zeros((32, 7), np.int64)
    scratch = np.zeros(5, np.int64)
    n = H.lnrf_host_hashgrid_bucket_plan(ctypes.byref(desc), m, levels.ctypes.data, scratch.ctypes.data)
    return levels[:n], scratch


@pytest.mark.parametrize("n_levels", sorted(LEVEL_SETS))
@pytest.mark.parametrize("m", [1, 2047, 2048, 2049, 20000, 786432])
def test_bucket_plan_and_scratch(H, n_levels, m):
    desc = make_desc(*LEVEL_SETS[n_levels])
    levels, scratch = bucket_plan(H, desc, m)
    cursor_bytes, level_max_off, tuple_off, total, n_wg = (int(v) for v in scratch)
    rows = [desc.table_size[l] for l in range(n_levels)]
    bucketed = [l for l in range(n_levels) if (rows[l] + 4095) // 4096 <= 256]
    assert [int(v) for v in levels[:, 0]] == bucketed
    wg, regions, cursors = 0, [], []
    for li, row in enumerate(levels):
        level, slices, split, wg_off, t_off, c_off, cap = (int(v) for v in row)
        assert slices == (rows[level] + 4095) // 4096 and 1 <= split <= 64
        assert wg_off == wg
        assert 1 <= cap <= 8 * m
        wg += slices * split
        regions.append((tuple_off + 12 * t_off, tuple_off + 12 * (t_off + slices * cap)))
        cursors.append((4 * c_off, 4 * (c_off + slices)))
        # the reduce workgroups of the level, for buckets holding 0, 1, cap and cap + 1 tuples
        for count in (0, 1, cap, cap + 1):
            out = np.zeros((slices * split, 6), np.int64)
            H.lnrf_host_hashgrid_reduce_work(ctypes.byref(desc), m, wg_off, slices * split, count, out.ctypes.data)
            assert (out[:, 0] == li).all() and (out[:, 1] == level).all()
            key = out[:, 2] * split + out[:, 3]
            assert np.array_equal(key, np.arange(slices * split)), "every (bucket, part) once, parts of a bucket together"
            assert (out[:, 3] < split).all() and (out[:, 2] < slices).all()
            lo, hi = out[:, 4].reshape(slices, split), out[:, 5].reshape(slices, split)
            assert (lo[:, 0] == 0).all() and (hi[:, -1] == min(count, cap)).all()
            assert (lo[:, 1:] == hi[:, :-1]).all() and (lo <= hi).all()
    assert wg == n_wg
    # cursors, level maxima (32 unsigned) and tuple regions: disjoint, in this order, inside the block
    for (a0, a1), (b0, b1) in zip(cursors, cursors[1:]):
        assert a1 <= b0
    assert (cursors[-1][1] if cursors else 0) <= level_max_off and level_max_off + 4 * 32 <= cursor_bytes
    assert cursor_bytes % 256 == 0 and tuple_off >= cursor_bytes
    for (a0, a1), (b0, b1) in zip(regions, regions[1:]):
        assert a0 < a1 <= b0
    assert all(tuple_off <= a0 and a1 <= total for a0, a1 in regions)


@pytest.mark.parametrize("n_levels", sorted(LEVEL_SETS))
def test_scratch_total_is_what_the_abi_reports(H, n_levels):
    if not os.path.exists(L.library_path()):
        pytest.skip("liblnrf.so not built (run __graft_entry__.build())")
    desc = make_desc(*LEVEL_SETS[n_levels])
    for m in (1, 2047, 2048, 2049, 20000, 786432):
        total = int(bucket_plan(H, desc, m)[1][3])
        assert L.lib().lnrf_hashgrid_bwd_scratch_bytes(ctypes.byref(desc), m) == total


def test_reduce_work_names_the_level(H):
    """Entry li of the plan and the level it stands for travel together: a level too large to bucket shifts them."""
    grids, tables = [16, 512, 32], [2 ** 21, 2 ** 21, 2 ** 21]  # 512^3 hashed into 2^21 rows: 512 slices, not bucketed
    desc = make_desc(grids, tables)
    levels, scratch = bucket_plan(H, desc, 5000)
    assert [int(v) for v in levels[:, 0]] == [0, 2]
    out = np.zeros((int(scratch[4]), 6), np.int64)
    H.lnrf_host_hashgrid_reduce_work(ctypes.byref(desc), 5000, 0, int(scratch[4]), 7, out.ctypes.data)
    assert sorted({(int(a), int(b)) for a, b in out[:, :2]}) == [(0, 0), (1, 2)]

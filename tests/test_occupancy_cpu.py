"""
The NumPy float32 restatement of the occupancy-grid kernels (tests/occupancy_reference.py) against float64 brute force,
without a GPU: the build against the cell-by-cell definition, the clip against 4096 float64 points per ray (zero
exceptions allowed), its defining properties, and the brute-force checkers against seeded mutations of the restatement
(the pattern of test_refnerf_dir_reference_cpu.py: a checker that accepts a broken restatement checks nothing).
"""
import numpy as np
import pytest

import occupancy_reference as R

F = np.float32
BMIN, BMAX = np.asarray(R.BOX_MIN, F), np.asarray(R.BOX_MAX, F)


def corner_densities(res: int, seed: int, special: bool = True):
    """(res + 1)^3 densities, about 10 % above the threshold 1.0, with a NaN and a +inf corner."""
    rng = np.random.default_rng(seed)
    sigma = (rng.random((res + 1) ** 3) * 1.1).astype(F)
    sigma[sigma > 1.0] += F(1.0)
    if special:
        sigma[rng.integers(0, sigma.size)] = np.nan
        sigma[rng.integers(0, sigma.size)] = np.inf
    return sigma


@pytest.mark.parametrize("res", [1, 2, 5, 33])
@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_build_equals_the_float64_definition(res, dilate):
    sigma = corner_densities(res, seed=res)
    bits, count = R.build(sigma, res, 1.0, dilate)
    occ = R.build_f64(sigma, res, 1.0, dilate)
    assert bits.dtype == np.uint32 and bits.shape == ((res ** 3 + 31) // 32,)
    flat = occ.reshape(-1)
    for idx in range(res ** 3):  # the bit layout, spelled out
        assert (int(bits[idx >> 5]) >> (idx & 31)) & 1 == int(flat[idx]), idx
    tail = res ** 3 & 31
    assert tail == 0 or int(bits[-1]) >> tail == 0, "unused bits of the last word must be zero"
    assert count == int(occ.sum()) == R.popcount(bits)
    assert np.array_equal(R.unpack_bits(bits, res), occ)


@pytest.mark.parametrize("res", [1, 2, 5, 33])
def test_build_zero_threshold_is_a_full_grid_and_nan_inf_occupy(res):
    sigma = corner_densities(res, seed=7)
    bits, count = R.build(sigma, res, 0.0, 0)
    assert count == res ** 3 and R.unpack_bits(bits, res).all()
    lone = np.zeros((res + 1) ** 3, F)
    for value in (np.nan, np.inf):
        lone[:] = 0
        lone[0] = value  # corner (0, 0, 0) belongs to cell (0, 0, 0) alone
        occ = R.unpack_bits(R.build(lone, res, 1.0, 0)[0], res)
        assert occ[0, 0, 0] and occ.sum() == 1


def clipped(res, kind, n=4113, mutate=None, seed=0):
    rays = R.make_rays(n, res, seed=res + seed)
    t_min, t_max, mask = R.box_range(rays, BMIN, BMAX)
    occ = R.make_grid(kind, res, seed=1 + seed)
    lo, hi, out = R.clip(rays, BMIN, BMAX, res, R.pack_bits(occ), t_min, t_max, mask, mutate=mutate)
    return rays, occ, (t_min, t_max, mask), (lo, hi, out)


@pytest.mark.parametrize("res", [1, 4, 33])
@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_clip_is_conservative_with_zero_exceptions(res, kind):
    """Several hundred rays (the hand-made ones included), 4096 float64 points each: every point of an occupied cell
    that stands 1e-4 of a cell off the faces lies in the clipped range.  The stand-off only removes points whose cell
    fp32 cannot decide; the pad of occ_geom.h is what the restatement uses."""
    n = 400
    rays, occ, (t_min, t_max, mask), (lo, hi, out) = clipped(res, kind, n=n)
    assert R.conservativeness_violations(rays, BMIN, BMAX, res, occ, t_min, t_max, mask, lo, hi, out) == 0
    live = out != 0
    assert (lo[live] >= t_min[live]).all() and (hi[live] <= t_max[live]).all() and (lo[live] < hi[live]).all()
    assert (out <= mask).all()
    assert (lo[~live] == 0).all() and (hi[~live] == F(1e-3)).all()  # the null range of ray_t_range


@pytest.mark.parametrize("res", [1, 4, 33])
def test_full_grid_returns_its_inputs_and_empty_grid_kills_every_ray(res):
    rays, _, (t_min, t_max, mask), (lo, hi, out) = clipped(res, "full")
    assert mask.sum() > 100 and (mask == 0).sum() > 100  # both kinds of ray are present
    assert np.array_equal(lo.view(np.uint32), t_min.view(np.uint32))
    assert np.array_equal(hi.view(np.uint32), t_max.view(np.uint32))
    assert np.array_equal(out, mask)
    _, _, _, (lo, hi, out) = clipped(res, "empty")
    assert not out.any() and (lo == 0).all() and (hi == F(1e-3)).all()


def test_clip_actually_clips():
    """A single occupied cell: most rays are culled and the survivors' ranges shrink to about one cell."""
    res = 33
    _, _, (t_min, t_max, mask), (lo, hi, out) = clipped(res, "single")
    live = out != 0
    assert 0 < live.sum() < 0.05 * mask.sum()
    diagonal = float(np.linalg.norm((BMAX - BMIN) / res))
    assert ((hi - lo)[live] <= diagonal + 2e-3).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4113])
def test_compaction_is_ascending_and_complete(n):
    rng = np.random.default_rng(n)
    for mask in (np.zeros(n, np.uint8), np.ones(n, np.uint8), (rng.random(n) < 0.3).astype(np.uint8) * 7):
        idx, count = R.compact(mask)
        assert idx.dtype == np.int32 and count == int((mask != 0).sum()) == idx.size
        assert (np.diff(idx) > 0).all() and (mask[idx] != 0).all()
        rest = np.ones(n, bool)
        rest[idx] = False
        assert (mask[rest] == 0).all()


# ------------------------------------------------------------------------------------------------ mutations
def violations(res, kind, mutate, rays=None):
    if rays is None:
        rays, occ, (t_min, t_max, mask), (lo, hi, out) = clipped(res, kind, n=400, mutate=mutate)
    else:
        occ = R.make_grid(kind, res, seed=1) if isinstance(kind, str) else kind
        t_min, t_max, mask = R.box_range(rays, BMIN, BMAX)
        lo, hi, out = R.clip(rays, BMIN, BMAX, res, R.pack_bits(occ), t_min, t_max, mask, mutate=mutate)
    return R.conservativeness_violations(rays, BMIN, BMAX, res, occ, t_min, t_max, mask, lo, hi, out)


def test_checker_rejects_zero_pad_with_a_shrunken_t_last():
    assert violations(33, "random5", None) == 0
    assert violations(33, "random5", "pad0_shrunk_last") > 0


def test_checker_rejects_a_dropped_tie_break_on_a_corner_ray():
    """A ray along the cell diagonal through the lattice points ties on all three axes at every step.  Without the
    tie-break the walk leaves the diagonal and never sees the occupied cells on it."""
    res = 4
    h = (BMAX - BMIN) / F(res)
    corner = (BMIN + F(2) * h).astype(F)
    rays = np.zeros((1, 2, 3), F)
    rays[0, 0] = corner - F(4) * h
    rays[0, 1] = (h.astype(np.float64) / np.linalg.norm(h.astype(np.float64))).astype(F)
    occ = np.zeros((res, res, res), bool)
    occ[1, 1, 1] = occ[2, 2, 2] = True
    assert violations(res, occ, None, rays=rays) == 0
    t_min, t_max, mask = R.box_range(rays, BMIN, BMAX)
    assert R.clip(rays, BMIN, BMAX, res, R.pack_bits(occ), t_min, t_max, mask)[2][0] == 1
    assert violations(res, occ, "no_tie_break", rays=rays) > 0


def test_checker_rejects_an_off_by_one_positive_plane_index():
    assert violations(4, "shell", None) == 0
    assert violations(4, "shell", "plane_off_by_one") > 0


def test_checker_rejects_a_forgotten_dilation():
    res = 5
    sigma = corner_densities(res, seed=3, special=False)
    good, _ = R.build(sigma, res, 1.0, 1)
    assert np.array_equal(R.unpack_bits(good, res), R.build_f64(sigma, res, 1.0, 1))
    bad, _ = R.build(sigma, res, 1.0, 1, mutate="no_dilate")
    assert not np.array_equal(R.unpack_bits(bad, res), R.build_f64(sigma, res, 1.0, 1))

"""
The NumPy restatement of the connected-component kernels (tests/components_reference.py) against hand-written answers
and scipy.ndimage.label, the property checker of the GPU tests against seeded mutations, and the facts about the test
volumes that the GPU tests lean on.  No GPU.
"""
import numpy as np
import pytest

import components_reference as C


def test_hand_written_answers():
    m = np.zeros((2, 3, 4), np.uint8)
    m[0, 0, 0] = m[0, 0, 1] = 1          # cells 0, 1
    m[0, 1, 2] = 1                       # cell 6: diagonal to cell 1 in the (j, k) plane
    m[1, 2, 3] = 1                       # cell 23: a corner away from cell 6
    m[1, 2, 0] = 1                       # cell 20: alone at both connectivities
    lab6, lab26 = C.label(m, 6), C.label(m, 26)
    want6 = np.full(24, -1, np.int32)
    want6[[0, 1, 6, 23, 20]] = [0, 0, 6, 23, 20]
    want26 = np.full(24, -1, np.int32)
    want26[[0, 1, 6, 23, 20]] = [0, 0, 0, 0, 20]
    assert np.array_equal(lab6.reshape(-1), want6) and np.array_equal(lab26.reshape(-1), want26)
    s6, s26 = C.sizes(lab6).reshape(-1), C.sizes(lab26).reshape(-1)
    assert s6.sum() == s26.sum() == 5 and s6[0] == 2 and s6[6] == s6[23] == s6[20] == 1
    assert s26[0] == 4 and s26[20] == 1 and np.count_nonzero(s26) == 2
    assert C.ranked(s26) == [(0, 4), (20, 1)]
    assert C.keep(lab26, C.sizes(lab26), min_cells=2).reshape(-1).nonzero()[0].tolist() == [0, 1, 6, 23]
    assert C.keep(lab6, C.sizes(lab6), keep_largest=2).reshape(-1).nonzero()[0].tolist() == [0, 1, 6]  # tie: 6 < 20 < 23
    assert C.keep(lab6, C.sizes(lab6), min_cells=3).sum() == 0
    for shape in ((1, 1, 1), (3, 1, 2)):
        assert (C.label(np.zeros(shape, np.uint8)) == -1).all()
        full = C.label(np.ones(shape, np.uint8), 6)
        assert (full == 0).all() and C.sizes(full).reshape(-1)[0] == full.size


@pytest.mark.parametrize("connectivity", [6, 26])
def test_reference_against_scipy(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    cases = [C.random_mask((9, 8, 7), p, seed) for p in (0.1, 0.31, 0.6) for seed in (0, 1)]
    cases += [C.checkerboard(), C.two_blocks("corner"), C.two_blocks("edge"), C.runs(), C.serpentine(9)]
    for mask in cases:
        theirs, count = ndimage.label(mask, structure=structure)
        ours = C.label(mask, connectivity)
        roots = np.unique(ours[ours >= 0])
        assert len(roots) == count
        # scipy numbers the components 1.. in raster order of first appearance: the rank of our smallest-index labels
        rank = np.searchsorted(roots, ours) + 1
        assert np.array_equal(np.where(ours >= 0, rank, 0), theirs)
        C.check(mask, connectivity, ours, C.sizes(ours))


@pytest.mark.parametrize("mutation", [m for m in C.MUTATIONS if m != "tie_to_higher_label"])
def test_checker_rejects_seeded_mutations(mutation):
    for mask in (C.two_blocks("corner"), C.random_mask((9, 8, 7), 0.31, 3)):
        good = C.reference(mask, 26)
        C.check(mask, 26, *good)
        bad = C.reference(mask, 26, mutate=mutation)
        assert not (np.array_equal(bad[0], good[0]) and np.array_equal(bad[1], good[1])), "the mutation changed nothing"
        with pytest.raises(AssertionError):
            C.check(mask, 26, *bad)


def test_tie_broken_towards_the_higher_label_is_rejected():
    mask = C.tie_mask()
    lab = C.label(mask, 26)
    size = C.sizes(lab)
    assert C.ranked(size) == [(0, 4), (110, 4), (220, 2), (204, 1)]
    good = C.keep(lab, size, keep_largest=1)
    bad = C.keep(lab, size, keep_largest=1, mutate="tie_to_higher_label")
    assert good.reshape(-1).nonzero()[0].tolist() == [0, 1, 2, 3]
    assert bad.reshape(-1).nonzero()[0].tolist() == [110, 111, 112, 113] and not np.array_equal(good, bad)


def test_serpentine_is_one_long_path_with_its_minimum_at_an_end():
    mask = C.serpentine(33)
    cells = int(mask.sum())
    assert cells > 4000
    lab = C.label(mask, 6)
    assert set(np.unique(lab).tolist()) == {-1, 0}, "one 6-connected component"
    # a path: two ends with one neighbour, every other cell with two; cell 0 is an end
    fg = np.pad(mask.astype(bool), 1)
    degree = sum(np.roll(fg, shift, axis) for axis in range(3) for shift in (-1, 1))[1:-1, 1:-1, 1:-1]
    degree = np.where(mask != 0, degree, 0)
    assert (degree == 1).sum() == 2 and (degree == 2).sum() == cells - 2
    assert mask[0, 0, 0] and degree[0, 0, 0] == 1
    # it enters every second layer and every second row
    assert mask[::2, ::2, :].all() and mask[1::2].sum() == 16 and mask[::2, 1::2].sum() == 17 * 16


def test_generators():
    board = C.checkerboard()
    assert (C.sizes(C.label(board, 6)).max() == 1) and len(np.unique(C.label(board, 26))) == 2
    for touch, at6, at26 in (("corner", 2, 1), ("edge", 2, 1)):
        m = C.two_blocks(touch)
        assert np.count_nonzero(C.sizes(C.label(m, 6))) == at6 and np.count_nonzero(C.sizes(C.label(m, 26))) == at26
    assert C.runs().shape == (1, 1, 70) and np.count_nonzero(C.sizes(C.label(C.runs(), 26))) == 11
    vol = C.blobs_volume()
    inside = vol > 0.5
    s26, s6 = C.sizes(C.label(inside, 26)), C.sizes(C.label(inside, 6))
    assert np.count_nonzero(s26) == 3 and np.count_nonzero(s6) == 4  # the corner blob is its own component at 6 only
    assert sorted(s6[s6 > 0].tolist())[:3] == [1, 8, 8] and s26.max() == s6.max() + 8

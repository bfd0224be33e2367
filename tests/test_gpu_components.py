"""
lnrf_cc_* on the GPU (csrc/components.hip, learn_nerf/components.py) against the NumPy restatement
tests/components_reference.py: labels, sizes and keep masks compared with torch.equal, on volumes small enough to run
in moments and shaped to cross waves, tiles and workgroups in every way the kernels distinguish.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import components_reference as C

pytestmark = pytest.mark.gpu
T = C.TILE


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_and_compare(mask, connectivity, check=True):
    """Labels and sizes of `mask` through learn_nerf.components equal the restatement's; -> (labels, sizes, rounds)."""
    from learn_nerf import components

    labels, rounds = components.label_components(gpu(mask), connectivity)
    sizes = components.component_sizes(labels)
    want = C.label(mask, connectivity)
    assert labels.dtype == torch.int32 and labels.shape == mask.shape and sizes.dtype == torch.int32
    assert torch.equal(labels.cpu(), torch.from_numpy(want)), f"labels differ, shape {mask.shape} at {connectivity}"
    assert torch.equal(sizes.cpu(), torch.from_numpy(C.sizes(want)))
    if check:
        C.check(mask, connectivity, labels.cpu().numpy(), sizes.cpu().numpy())
    assert 1 <= rounds <= components.L.lib().lnrf_cc_max_rounds()
    return labels, sizes, rounds


@pytest.mark.parametrize("connectivity", [6, 26])
def test_smallest_volumes(connectivity):
    from learn_nerf import components

    for value in (0, 1):
        labels, sizes, _ = run_and_compare(np.full((1, 1, 1), value, np.uint8), connectivity)
        assert labels.item() == value - 1 and sizes.item() == value
    run_and_compare(C.runs(70), connectivity)
    labels, _, rounds = run_and_compare(np.zeros((9, 8, 7), np.uint8), connectivity)
    assert (labels == -1).all() and rounds == 1, "an empty mask is not an error"
    labels, sizes, _ = run_and_compare(np.ones((9, 8, 7), np.uint8), connectivity)
    assert (labels == 0).all() and sizes.reshape(-1)[0].item() == 9 * 8 * 7
    keep, info = components.keep_components(gpu(np.zeros((3, 2, 1), np.uint8)), connectivity=connectivity)
    assert not keep.any() and (info["components"], info["kept"], info["removed"]) == (0, 0, 0)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_all_256_masks_of_2x2x2(connectivity):
    """Each mask is a volume of its own: packed into one volume, the blocks would need gaps and lose the box faces."""
    from learn_nerf import components

    for bits in range(256):
        mask = np.array([(bits >> c) & 1 for c in range(8)], np.uint8).reshape(2, 2, 2)
        labels, _ = components.label_components(gpu(mask), connectivity)
        assert torch.equal(labels.cpu(), torch.from_numpy(C.label(mask, connectivity))), bits


def test_checkerboard_and_touching_blocks():
    board = C.checkerboard((9, 10, 11))
    labels, sizes, _ = run_and_compare(board, 6)
    assert sizes.max().item() == 1
    labels, sizes, _ = run_and_compare(board, 26)
    assert sizes.reshape(-1)[0].item() == int(board.sum()) and sizes.count_nonzero().item() == 1
    for touch in ("corner", "edge"):
        block = C.two_blocks(touch)
        assert run_and_compare(block, 6)[1].count_nonzero().item() == 2
        assert run_and_compare(block, 26)[1].count_nonzero().item() == 1


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape", [(T + 1, T + 1, T + 1), (2 * T - 1, T, 1), (5, 7, 9)])
def test_components_straddle_tiles(shape, connectivity):
    for seed in (0, 1):
        run_and_compare(C.random_mask(shape, 0.5, seed), connectivity)


def test_serpentine_converges_in_few_rounds():
    """One component thousands of cells long whose smallest index is at one end (tests/test_components_cpu.py): a
    propagation bounded by the diameter needs thousands of rounds, the cap is 64."""
    mask = C.serpentine(33)
    for connectivity in (6, 26):
        labels, sizes, rounds = run_and_compare(mask, connectivity, check=False)
        print(f"serpentine (33, 33, 33), {int(mask.sum())} cells, connectivity {connectivity}: {rounds} rounds")
        assert sizes.reshape(-1)[0].item() == int(mask.sum())
        assert rounds < 64


@pytest.mark.parametrize("connectivity,p", [(6, 0.31), (26, 0.10), (6, 0.6), (26, 0.6)])
def test_percolation_thresholds(connectivity, p):
    for seed in (0, 1, 2):
        run_and_compare(C.random_mask((33, 31, 29), p, seed), connectivity)


def test_many_workgroups_twice_in_one_process():
    from learn_nerf import components

    mask = C.random_mask((130, 66, 34), 0.31, 0)
    first, _, rounds = run_and_compare(mask, 6, check=False)
    second, again = components.label_components(gpu(mask), 6)
    assert torch.equal(first, second)
    print(f"(130, 66, 34) at p = 0.31, connectivity 6: {rounds} and {again} rounds")


def test_raw_abi_on_a_poisoned_scratch():
    """The C entry points themselves, the scratch block and every output filled with 0xFF bytes beforehand."""
    from learn_nerf import _lib as L

    lib = L.lib()
    mask = C.random_mask((T + 1, 2 * T - 1, 11), 0.12, 5)  # 28 components at 26
    nx, ny, nz = mask.shape
    n = mask.size
    want = C.label(mask, 26)
    nbytes = lib.lnrf_cc_scratch_bytes(nx, ny, nz)
    assert nbytes >= 4 * n
    dev_mask = gpu(mask)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")  # 0xFF bytes
    sizes, changed = labels.clone(), labels[:1].clone()
    keep = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    L.check(lib.lnrf_cc_local(L.ptr(dev_mask, torch.uint8), nx, ny, nz, 26, L.ptr(labels, torch.int32),
                              L.ptr(scratch, torch.uint8), nbytes, L.stream()))
    for round_index in range(lib.lnrf_cc_max_rounds()):
        L.check(lib.lnrf_cc_merge_round(nx, ny, nz, 26, round_index, L.ptr(labels, torch.int32),
                                        L.ptr(changed, torch.int32), L.ptr(scratch, torch.uint8), nbytes, L.stream()))
        if changed.item() == 0:
            break
    else:
        raise AssertionError("no fixed point below the cap")
    assert torch.equal(labels.cpu().view(mask.shape), torch.from_numpy(want))
    L.check(lib.lnrf_cc_sizes(L.ptr(labels, torch.int32), n, L.ptr(sizes, torch.int32), L.stream()))
    assert torch.equal(sizes.cpu().view(mask.shape), torch.from_numpy(C.sizes(want)))
    order = C.ranked(C.sizes(want))
    cut_label, cut_size = order[1]
    L.check(lib.lnrf_cc_keep(L.ptr(labels, torch.int32), L.ptr(sizes, torch.int32), n, 2, cut_size, cut_label,
                             L.ptr(keep, torch.uint8), L.stream()))
    assert torch.equal(keep.cpu().view(mask.shape), torch.from_numpy(C.keep(want, C.sizes(want), 2, 2)))
    # the call for the round after the last allowed one launches nothing and says why
    rc = lib.lnrf_cc_merge_round(nx, ny, nz, 26, lib.lnrf_cc_max_rounds(), L.ptr(labels, torch.int32),
                                 L.ptr(changed, torch.int32), L.ptr(scratch, torch.uint8), nbytes, L.stream())
    assert rc == L.ERR_UNSUPPORTED and b"no fixed point" in lib.lnrf_last_error()


def test_keep_components():
    from learn_nerf import components

    cases = [(C.tie_mask(), 26), (C.random_mask((9, 10, 11), 0.2, 7), 6), (C.random_mask((9, 10, 11), 0.12, 8), 26)]
    for mask, connectivity in cases:
        lab = C.label(mask, connectivity)
        size = C.sizes(lab)
        count, largest = int(np.count_nonzero(size)), int(size.max())
        assert count >= 4
        for min_cells, keep_largest in itertools.product((1, 2, largest + 1), (None, 1, 2, count + 3)):
            keep, info = components.keep_components(gpu(mask), min_cells=min_cells, keep_largest=keep_largest,
                                                    connectivity=connectivity)
            want = C.keep(lab, size, min_cells, keep_largest)
            assert keep.dtype == torch.uint8
            assert torch.equal(keep.cpu(), torch.from_numpy(want)), (min_cells, keep_largest)
            kept_roots = np.unique(lab[want != 0])
            assert info["components"] == count and info["kept"] == len(kept_roots)
            assert info["removed"] == int((mask != 0).sum() - want.sum()) and info["rounds"] >= 1
    # the tie: two components of 4 cells, the one with the lower label wins
    keep, info = components.keep_components(gpu(C.tie_mask()), keep_largest=1)
    assert keep.reshape(-1).nonzero().reshape(-1).tolist() == [0, 1, 2, 3] and info["kept"] == 1
    # a bool mask is a mask
    keep_b, _ = components.keep_components(gpu(C.tie_mask()).bool(), keep_largest=1)
    assert torch.equal(keep, keep_b)


def test_errors():
    from learn_nerf import _lib as L
    from learn_nerf import components

    lib = L.lib()
    mask = gpu(np.ones((2, 2, 2), np.uint8))
    with pytest.raises(ValueError, match="connectivity"):
        components.label_components(mask, 8)
    with pytest.raises(ValueError, match="dimension"):
        components.label_components(torch.zeros((2, 0, 2), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="min_cells"):
        components.keep_components(mask, min_cells=0)
    with pytest.raises(ValueError, match="keep_largest"):
        components.keep_components(mask, keep_largest=0)
    labels = torch.empty(8, dtype=torch.int32, device="cuda")
    scratch = torch.empty(32, dtype=torch.uint8, device="cuda")
    args = (L.ptr(labels, torch.int32), L.ptr(scratch, torch.uint8), 32, L.stream())
    assert lib.lnrf_cc_local(L.ptr(mask, torch.uint8), 2, 2, 2, 8, *args) == -1
    assert b"connectivity" in lib.lnrf_last_error()
    assert lib.lnrf_cc_local(L.ptr(mask, torch.uint8), 2, 0, 2, 26, *args) == -1
    assert lib.lnrf_cc_keep(L.ptr(labels, torch.int32), L.ptr(labels, torch.int32), 8, 0, 0, -1,
                            L.ptr(scratch, torch.uint8), L.stream()) == -1
    assert b"min_cells" in lib.lnrf_last_error()
    # more than INT32_MAX cells, sizes only: refused before any pointer is looked at, so nothing is launched
    assert lib.lnrf_cc_scratch_bytes(2048, 1024, 1024) == -1
    assert lib.lnrf_cc_local(None, 2048, 1024, 1024, 26, None, None, 0, None) == L.ERR_UNSUPPORTED
    assert b"INT32_MAX" in lib.lnrf_last_error()
    assert lib.lnrf_cc_merge_round(2048, 1024, 1024, 26, 0, None, None, None, 0, None) == L.ERR_UNSUPPORTED
    assert lib.lnrf_cc_sizes(None, 2 ** 31, None, None) == L.ERR_UNSUPPORTED
    assert ctypes.c_int64(lib.lnrf_cc_scratch_bytes(1290, 1290, 1290)).value == 4 * 1290 ** 3  # just below the limit

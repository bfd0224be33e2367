"""
Workspace poisoning for GPU tests (a plain module that tests import; not a conftest).

    with poisoned(0x41, models=(model,)) as rec:
        ...  # every leased workspace block and every float / uint8 torch.empty on the GPU starts as 0x41414141...
    rec.purposes  # the lease purposes handed out inside the block

Workspace blocks (learn_nerf/_ws.py) and the caching allocator hand a call memory that the previous call wrote, so a
kernel that reads a word its own call never wrote returns a stale value that is usually plausible and often the same
from call to call.  Filling that memory with a pattern first turns such a read into a visible difference: 0x41 is 12.08
in fp32 and 12.06 in bf16 (a stale value ADDED into a result), 0xFF is NaN in both (a stale value MULTIPLIED into a
result, even by zero), 0x00 is what a fresh allocation often holds.  A correct call gives the same bits under all three.

Safety: no poisoned word may ever become an address.  Integer dtypes of 16 bits and wider are never poisoned, and
neither is a lease purpose whose block holds indices (UNPOISONED_PURPOSES).  Every other purpose the package leases was
checked for index content and is listed in POISONED_PURPOSES with the reason a stale word there can only be a wrong
number; a purpose that is in neither table (a new or renamed one) is left alone until it has been reviewed
(test_abi_and_host.py::test_poison_helper_reviews_every_lease_purpose keeps the tables in step with the package's
lease calls).  A block is allocated with the torch.empty patch suspended, so an unpoisoned purpose stays unpoisoned on
its first lease too.  uint8 tensors from torch.empty are the packed weight blobs (bf16 fragments) and the per-ray hit
masks of ray_aabb_stratified (0 / 1 flags): values, not indices.
"""
import contextlib
from typing import List, Set

import torch

PATTERNS = (0x00, 0x41, 0xFF)

_POISON_DTYPES = (torch.float32, torch.bfloat16, torch.float16, torch.uint8)

# blocks that hold indices: a stale word there could be an address
UNPOISONED_PURPOSES = {
    "hashgrid_bwd": "bucket tuples (table row indices) and bucket offsets of the bucketed scatter (hashgrid.hip)",
}

# blocks that hold values only; a stale word is a wrong number (or a hand-off count that is compared, never followed)
POISONED_PURPOSES = {
    "nerf_save": "forward activations (bf16 fragments), fp32 pre-activations and ReLU bit masks: operands and selects",
    "nerf_bwd": "two-launch backward: dy gradient dump (bf16 fragments) and fp32 partial-sum slabs",
    "nerf_bwd_ls": "layer-stationary backward: dy dump, fp32 slabs, hand-off counters and the status word; the counters "
                   "and the status are zeroed by the head launch or a memset before the pipeline reads them, and a "
                   "counter is only compared with a tile count: tile addresses come from the launch's own tile walk",
    "composite_bwd": "fp32 per-workgroup partial sums of the background gradient",
    "dense_wgrad": "fp32 split-K partial sums of the generic dense weight gradient",
    "gemm_det": "fp32 split-K partial sums of lnrf_gemm_f32_det",
    "ngp_scratch": "InstantNGP backward: fp32 partial dW rows and per-workgroup level maxima (floats; the scatter's "
                   "fixed-point scale comes from a torch.zeros vector, not from this block)",
    "ngp_g_enc": "fp32 gradient of the encoding (feature-major)",
    "ref_masks": "Ref-NeRF split-precision trunk: ReLU mask words (selects)",
    "ref_save": "Ref-NeRF trunk forward save (as nerf_save)",
    "ref_cdump": "Ref-NeRF chain-state dump (bf16 fragments) and fp32 slabs behind it",
    "ref_dsave": "Ref-NeRF directional block forward save (bf16 fragments)",
    "ref_dscratch": "Ref-NeRF directional block gradient dump and fp32 slabs",
    "ref_scratch": "Ref-NeRF layer-stationary trunk backward (as nerf_bwd_ls)",
    "ref_tscratch": "Ref-NeRF tangent (second-order) save (as nerf_save)",
}


class PoisonRecord:
    """What one poisoned() block saw: lease purposes (all, and the poisoned ones) and the count of poisoned empties."""

    def __init__(self, pattern: int):
        self.pattern = pattern
        self.purposes: Set[str] = set()
        self.poisoned_purposes: Set[str] = set()
        self.empties = 0
        self.unreviewed: List[str] = []


def _fill(t: torch.Tensor, pattern: int) -> None:
    if t.numel() == 0:
        return
    if t.dtype == torch.uint8:
        t.fill_(pattern)
    else:
        t.view(torch.uint8).fill_(pattern)  # the byte pattern, not the value: contiguous fresh tensors only


def _drop_pack_caches(models) -> None:
    for mdl in models:
        if hasattr(mdl, "_pack_cache"):
            mdl._pack_cache = None


@contextlib.contextmanager
def poisoned(pattern: int, models=()):
    """Poison every workspace lease and every CUDA float32 / bfloat16 / float16 / uint8 torch.empty(_like) inside the
    block with the byte `pattern`.  On entry the idle workspace blocks are dropped (_ws.clear()) and the given models'
    packed-weight caches are cleared, so the packed weights are repacked into poisoned memory; on exit the patches are
    undone, the idle blocks dropped and the caches cleared again (nothing poisoned outlives the block)."""
    from learn_nerf import _ws

    if not 0 <= pattern <= 0xFF:
        raise ValueError("pattern is one byte")
    rec = PoisonRecord(pattern)
    orig_lease, orig_empty, orig_empty_like = _ws.lease, torch.empty, torch.empty_like

    in_lease = [False]

    def lease(purpose, nbytes, device):
        in_lease[0] = True  # the block's own torch.empty is not poisoned: the purpose decides below
        try:
            blk = orig_lease(purpose, nbytes, device)
        finally:
            in_lease[0] = False
        rec.purposes.add(purpose)
        if purpose in POISONED_PURPOSES:
            _fill(blk.buf, pattern)
            rec.poisoned_purposes.add(purpose)
        elif purpose not in UNPOISONED_PURPOSES and purpose not in rec.unreviewed:
            rec.unreviewed.append(purpose)
        return blk

    def poison_result(t):
        if not in_lease[0] and isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in _POISON_DTYPES and t.is_contiguous():
            _fill(t, pattern)
            rec.empties += 1
        return t

    def empty(*args, **kwargs):
        return poison_result(orig_empty(*args, **kwargs))

    def empty_like(*args, **kwargs):
        return poison_result(orig_empty_like(*args, **kwargs))

    torch.cuda.synchronize()
    _ws.clear()
    _drop_pack_caches(models)
    _ws.lease, torch.empty, torch.empty_like = lease, empty, empty_like
    try:
        yield rec
    finally:
        _ws.lease, torch.empty, torch.empty_like = orig_lease, orig_empty, orig_empty_like
        torch.cuda.synchronize()
        _ws.clear()
        _drop_pack_caches(models)

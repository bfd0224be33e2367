"""
Connected components of a 3-D mask on the GPU (additive; lnrf_cc_*, csrc/components.hip, whose header comment fixes the
conventions): labels, component sizes and a keep filter.  learn_nerf/mesh.py and learn_nerf/occupancy.py use it to
remove floaters, the small blobs of density a trained model leaves in empty space.

The filter removes what is disconnected at the volume's resolution and threshold.  A floater that one cell joins to the
object is part of the object.
"""
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L
from . import ops


def _as_mask(mask: torch.Tensor) -> torch.Tensor:
    if mask.dim() != 3:
        raise ValueError(f"expected a 3-d mask, got shape {tuple(mask.shape)}")
    if min(mask.shape) < 1:
        raise ValueError(f"every dimension must be at least 1, got {tuple(mask.shape)}")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8:
        raise TypeError(f"expected a uint8 or bool mask, got {mask.dtype}")
    return mask.contiguous()


def _check_connectivity(connectivity: int) -> int:
    if connectivity not in (6, 26):
        raise ValueError(f"connectivity must be 6 or 26, got {connectivity!r}")
    return int(connectivity)


def label_components(mask: torch.Tensor, connectivity: int = 26) -> Tuple[torch.Tensor, int]:
    """
    mask: uint8 (non-zero = foreground) or bool [nx, ny, nz] on the GPU.
    -> (labels int32 [nx, ny, nz]: the smallest linear index (i*ny + j)*nz + k of the cell's component, -1 for
    background; the number of merge rounds run, the one that found nothing to change included).

    One read-back of a changed-word per round.  The loop is bounded by lnrf_cc_max_rounds(): the call for the round
    after the last allowed one fails in the library, so unconverged labels are never returned.
    """
    connectivity = _check_connectivity(connectivity)
    mask = _as_mask(mask)
    labels, scratch = ops.cc_local(mask, connectivity)
    changed = torch.empty(1, dtype=torch.int32, device=mask.device)
    cap = L.lib().lnrf_cc_max_rounds()
    for round_index in range(cap + 1):
        ops.cc_merge_round(labels, scratch, changed, connectivity, round_index)  # raises at round_index == cap
        if changed.item() == 0:
            return labels, round_index + 1
    raise RuntimeError(f"connected components: no fixed point after {cap} rounds")


def component_sizes(labels: torch.Tensor) -> torch.Tensor:
    """labels of label_components -> int32 sizes of the same shape: the number of cells of each component at its root
    (the cell whose label is its own index), 0 everywhere else."""
    if labels.dtype != torch.int32:
        raise TypeError(f"expected int32 labels, got {labels.dtype}")
    if labels.numel() < 1:
        raise ValueError("labels must not be empty")
    return ops.cc_sizes(labels.contiguous())


def keep_components(mask: torch.Tensor, min_cells: int = 1, keep_largest: Optional[int] = None,
                    connectivity: int = 26) -> Tuple[torch.Tensor, Dict[str, int]]:
    """
    -> (keep uint8 [nx, ny, nz], info).  A cell is kept iff it is foreground, its component has at least `min_cells`
    cells and, when `keep_largest` is given, its component is among the first `keep_largest` in the order (size
    descending, label ascending).  info: components, kept (components), removed (cells), rounds.
    """
    if min_cells < 1:
        raise ValueError("min_cells must be at least 1")
    if keep_largest is not None and keep_largest < 1:
        raise ValueError("keep_largest must be None or at least 1")
    labels, rounds = label_components(mask, connectivity)
    sizes = component_sizes(labels)
    flat = sizes.reshape(-1)
    roots = flat.nonzero().reshape(-1)  # ascending, so a stable sort by size breaks ties towards the lower label
    root_sizes = flat[roots]
    count = roots.numel()
    cut_size, cut_label = 0, -1
    if keep_largest is not None and keep_largest < count:
        order = torch.sort(root_sizes, descending=True, stable=True).indices
        last = order[keep_largest - 1]
        cut_size, cut_label = int(root_sizes[last]), int(roots[last])
    keep = ops.cc_keep(labels, sizes, min_cells, cut_size, cut_label)
    kept = (root_sizes >= min_cells) & ((root_sizes > cut_size) | ((root_sizes == cut_size) & (roots <= cut_label)))
    info = dict(components=count, kept=int(kept.sum()), removed=int(root_sizes[~kept].sum()), rounds=rounds)
    return keep, info

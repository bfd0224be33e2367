"""
Occupancy grid for the inference renderer (additive; the reference samples every ray over its whole range in the scene
box): a bitfield of the cells of an R^3 grid over the box in which a trained model's density is not negligible, and the
clipping of ray ranges to those cells (lnrf_occ_build / lnrf_occ_clip_rays, csrc/occupancy.hip and csrc/occ_geom.h,
whose header comments fix the conventions).

The density is sampled at the cell corners only.  That does not bound it inside a cell: a feature thinner than a cell
can sit between the corners.  The dilation and the low default threshold make a miss unlikely, not impossible; the grid
is an approximation the user opts into, and the renderer without a grid stays the yardstick.
"""
import math
from dataclasses import dataclass, replace
from typing import Any, Optional, Tuple

import torch

from . import ops
from .mesh import density_grid


def _vec3(v) -> Tuple[float, float, float]:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    return tuple(float(x) for x in v)


def sigma_threshold(threshold: float, bbox_min, bbox_max, resolution: int) -> float:
    """The density whose opacity over one cell diagonal is `threshold`: -log1p(-threshold) / |diagonal|, computed in
    float64; the kernel receives it rounded to float32.  threshold = 0 gives 0 (every cell occupied)."""
    if not 0.0 <= threshold < 1.0:
        raise ValueError("threshold is an opacity in [0, 1)")
    lo, hi = _vec3(bbox_min), _vec3(bbox_max)
    diagonal = math.sqrt(sum(((b - a) / resolution) ** 2 for a, b in zip(lo, hi)))
    return -math.log1p(-threshold) / diagonal


@dataclass
class OccupancyGrid:
    """
    :param bits: int32 [ceil(R^3 / 32)] on the GPU, the uint32 words of the bitfield (cell (i*R + j)*R + k is bit
                 idx & 31 of word idx >> 5).
    :param resolution: R, cells per axis.  :param bbox_min / bbox_max: the scene box the grid spans.
    :param sigma_thr: the density threshold the grid was built with.  :param occupied: number of occupied cells.
    """

    bits: torch.Tensor
    resolution: int
    bbox_min: Any
    bbox_max: Any
    sigma_thr: float
    occupied: int

    @classmethod
    def from_model(cls, model, params, bbox_min, bbox_max, resolution: int, threshold: float = 0.01,
                   dilate: int = 1, batch_size: int = 1 << 18, min_cells: int = 1, keep_largest: Optional[int] = None,
                   connectivity: int = 26) -> "OccupancyGrid":
        """Evaluate `model` at the (resolution + 1)^3 cell corners (direction d = 0) and build the grid: a cell is
        occupied when a corner of it, or of a cell within `dilate` cells (Chebyshev), reaches the density whose
        opacity over one cell diagonal is `threshold`.  With min_cells > 1 or keep_largest the grid is then
        `filtered`; with the defaults no component kernel runs."""
        resolution = int(resolution)
        lo, hi = _vec3(bbox_min), _vec3(bbox_max)
        sigma_thr = sigma_threshold(threshold, lo, hi, resolution)
        sigma = density_grid(model, params, lo, hi, resolution + 1, batch_size)
        bits, occupied = ops.occ_build(sigma.reshape(-1), resolution, sigma_thr, dilate)
        grid = cls(bits=bits, resolution=resolution, bbox_min=lo, bbox_max=hi, sigma_thr=sigma_thr,
                   occupied=occupied)
        if min_cells != 1 or keep_largest is not None:
            grid = grid.filtered(min_cells=min_cells, keep_largest=keep_largest, connectivity=connectivity)
        return grid

    @classmethod
    def from_renderer(cls, renderer, resolution: int, threshold: float = 0.01, dilate: int = 1,
                      batch_size: int = 1 << 18, min_cells: int = 1, keep_largest: Optional[int] = None,
                      connectivity: int = 26) -> "OccupancyGrid":
        """The grid of a NeRFRenderer's fine model over its scene box."""
        return cls.from_model(renderer.fine, renderer.fine_params, renderer.bbox_min, renderer.bbox_max, resolution,
                              threshold=threshold, dilate=dilate, batch_size=batch_size, min_cells=min_cells,
                              keep_largest=keep_largest, connectivity=connectivity)

    def cell_mask(self) -> torch.Tensor:
        """The bitfield as uint8 [R, R, R], 1 = occupied (torch integer operations on the GPU)."""
        shifts = torch.arange(32, dtype=torch.int32, device=self.bits.device)
        cells = ((self.bits[:, None] >> shifts[None, :]) & 1).to(torch.uint8).reshape(-1)
        r = self.resolution
        return cells[:r ** 3].reshape(r, r, r).contiguous()

    def filtered(self, min_cells: int = 1, keep_largest: Optional[int] = None,
                 connectivity: int = 26) -> "OccupancyGrid":
        """
        The grid without its floaters (additive; learn_nerf/components.py): the connected components of the occupied
        cells (the final, dilated bitfield the renderer walks) that have fewer than `min_cells` cells or, with
        `keep_largest`, are not among the largest become unoccupied.  -> a new grid over the same box and resolution
        with new bits and a new occupied count.  Run once per session: the bits are unpacked and repacked with torch.
        """
        from .components import keep_components

        keep, _ = keep_components(self.cell_mask(), min_cells=min_cells, keep_largest=keep_largest,
                                  connectivity=connectivity)
        flat = keep.reshape(-1)
        padded = torch.zeros(self.bits.numel() * 32, dtype=torch.int32, device=flat.device)
        padded[:flat.numel()] = flat
        shifts = torch.arange(32, dtype=torch.int32, device=flat.device)
        # 32 distinct bits: the int32 sum is their union and cannot overflow (bit 31 is the only negative term)
        bits = (padded.view(-1, 32) << shifts[None, :]).sum(dim=1, dtype=torch.int32)
        return replace(self, bits=bits, occupied=int(flat.sum()))

    @property
    def occupied_fraction(self) -> float:
        return self.occupied / float(self.resolution ** 3)

    def clip(self, rays: torch.Tensor, t_min: torch.Tensor, t_max: torch.Tensor, mask: torch.Tensor,
             min_t_range: float = 1e-3, epsilon: float = 1e-8):
        """(t_min, t_max, mask) of the box test -> the triple clipped to the occupied cells each ray crosses; a ray
        that crosses none gets mask 0 and the null range (0, min_t_range), like a ray that misses the box."""
        mask_u8 = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        return ops.occ_clip_rays(rays, self.bbox_min, self.bbox_max, self.bits, self.resolution, t_min.contiguous(),
                                 t_max.contiguous(), mask_u8.contiguous(), min_t_range=min_t_range, epsilon=epsilon)

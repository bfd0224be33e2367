"""
Mesh simplification (scripts/simplify_mesh.py, and --target_faces / --simplify_grid of the mesh producers): vertex
clustering with quadric error metrics (Lindstrom, "Out-of-core simplification of large polygonal models", 2000) on a
grid of cubic cells.  Every triangle corner falls into a cell; a triangle whose corners fall into three distinct cells
survives as the triple of those cells; each occupied cell becomes one vertex, placed where the area-weighted plane
quadrics of the cell's triangles are smallest, which keeps corners and creases where they are.  O(F), no priority queue,
and bit-reproducible: the cells are pinned fp32 arithmetic, the per-cell sums are fp64 in a fixed order
(csrc/simplify.hip), and an indexed mesh gives the bits of its triangle soup because everything is defined on corners.

  grid      origin lo = the fp32 minimum over all corners (or `origin`), cubic cells of edge h: cell_size, or the longest
            extent / grid; inv_h = float32(1 / h); n_a = floorf((hi_a - lo_a) * inv_h) + 1 in fp32 (the cell of the
            highest corner, plus one), capped at `grid` cells.  Fewer than 2^31 cells in all.
  target    target_faces = T: the grid with N cells along the longest axis, N found by bisection over [1, 1024] on the
            number of surviving triangles count(N) <= T.  Removing duplicates only lowers the count, so the result has at
            most T faces.
  faces     the survivors in input order, without the later copies of a face equal to an earlier one up to cyclic
            rotation (opposite winding is not a copy); vertices: the cells the faces name, in ascending key order.
  no        topology guarantees, manifold repair or attribute-aware quadrics: clustering can pinch a thin sheet into a
            non-manifold edge and can flip a face (info["flipped"] counts them).

The kernels run on the GPU; there is no CPU fallback.
"""
import math
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from learn_nerf import ops

INT32_MAX = 2**31 - 1
MAX_TARGET_CELLS = 1024  # upper end of the search for target_faces
PLACEMENTS = ("quadric", "mean")


@dataclass
class SimplifiedMesh:
    verts: torch.Tensor  # fp32 [V, 3]
    faces: torch.Tensor  # int32 [M, 3]
    colors: Optional[torch.Tensor]  # uint8 [V, 3] when colours were given
    info: dict


# ------------------------------------------------------------ host logic ----

def check_size_arguments(cell_size, grid, target_faces, placement="quadric") -> None:
    """Exactly one of the three, each positive; a known placement."""
    given = [name for name, v in (("cell_size", cell_size), ("grid", grid), ("target_faces", target_faces))
             if v is not None]
    if len(given) != 1:
        raise ValueError(f"give exactly one of cell_size, grid and target_faces, got {given or 'none'}")
    if cell_size is not None and not (float(cell_size) > 0 and math.isfinite(float(cell_size))):
        raise ValueError(f"cell_size must be positive and finite, got {cell_size}")
    for name, v in (("grid", grid), ("target_faces", target_faces)):
        if v is not None and (int(v) != v or int(v) < 1):
            raise ValueError(f"{name} must be a positive integer, got {v}")
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be one of {PLACEMENTS}, got {placement!r}")


def choose_grid(lo, hi, cell_size: Optional[float] = None, cells: Optional[int] = None):
    """(h float64, inv_h float32, dims) of the grid with origin lo (fp32 [3]) that holds hi: the rule of the module
    docstring.  ValueError for a cell edge without a finite positive float32 inverse (a mesh without extent under
    `cells`) and for 2^31 cells or more."""
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    if cells is not None:
        h = float(np.max(hi.astype(np.float64) - lo.astype(np.float64))) / int(cells)
    else:
        h = float(cell_size)
    if not (h > 0 and math.isfinite(h)):
        raise ValueError(f"the cell edge must be positive and finite, got {h} (a mesh without extent?)")
    with np.errstate(over="ignore"):
        inv_h = np.float32(1.0 / h)
    if not (inv_h > 0 and np.isfinite(inv_h)):
        raise ValueError(f"the cell edge {h} has no finite positive float32 inverse")
    with np.errstate(over="ignore"):
        t = np.floor((hi - lo) * inv_h)
    if not (t < 2.0**31).all():
        raise ValueError(f"a cell edge of {h} gives 2^31 cells or more along an axis")
    dims = [max(1, int(v) + 1) for v in t]
    if cells is not None:
        dims = [min(int(cells), n) for n in dims]
    if math.prod(dims) > INT32_MAX:
        raise ValueError(f"a cell edge of {h} gives a grid of {dims} cells: 2^31 or more, and the cell key is an int32")
    return h, inv_h, dims


def bisect_cells(count: Callable[[int], int], target: int, hi: int = MAX_TARGET_CELLS) -> int:
    """The N of target_faces: lo = 1; while lo < hi: mid = (lo + hi + 1) // 2; count(mid) <= target ? lo = mid :
    hi = mid - 1.  Every value lo takes was tested (or is 1, where nothing survives), so count(N) <= target also when
    count is not monotone."""
    lo = 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if count(mid) <= target:
            lo = mid
        else:
            hi = mid - 1
    return lo


# -------------------------------------------------------------- pipeline ----

def _as_soup(tris_or_verts, faces, colors, device) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(tris fp32 [F, 3, 3], corner colours uint8 [3F, 3] or None) on the GPU."""
    def tensor(x):
        return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))

    v = tensor(tris_or_verts)
    if faces is None:
        if v.dim() != 3 or tuple(v.shape[1:]) != (3, 3):
            raise ValueError(f"expected triangles [F, 3, 3] (or verts [V, 3] with faces), got {tuple(v.shape)}")
        n_verts = None
    else:
        f = tensor(faces)
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"expected verts [V, 3] and faces [F, 3], got {tuple(v.shape)} and {tuple(f.shape)}")
        n_verts = v.shape[0]
    if (v.shape[0] == 0) or (faces is not None and f.shape[0] == 0):
        raise ValueError("the mesh is empty")
    if device is None:
        device = v.device if v.is_cuda else torch.device("cuda")
    if torch.device(device).type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("mesh simplification needs a ROCm GPU device (no CPU fallback)")
    v = v.to(device=device, dtype=torch.float32)
    if not torch.isfinite(v).all():
        raise ValueError("the mesh holds non-finite vertices")
    if faces is not None:
        f = f.to(device=device, dtype=torch.int64)
        if int(f.min()) < 0 or int(f.max()) >= n_verts:
            raise ValueError(f"a face names a vertex outside [0, {n_verts})")
        tris = v[f]
    else:
        tris = v
    tris = tris.contiguous()
    n_tris = tris.shape[0]
    if n_tris > INT32_MAX // 3:
        raise ValueError(f"{n_tris} triangles: their corners do not fit in int32 indices")
    corner = None
    if colors is not None:
        c = tensor(colors)
        if c.dtype != torch.uint8:
            raise ValueError(f"colors must be uint8, got {c.dtype}")
        c = c.to(device)
        if faces is not None and tuple(c.shape) == (n_verts, 3):
            corner = c[f].reshape(-1, 3)
        elif tuple(c.shape) in ((n_tris, 3, 3), (3 * n_tris, 3)):
            corner = c.reshape(-1, 3)
        else:
            raise ValueError(f"colors must be one RGB per vertex or per corner, got {tuple(c.shape)}")
        corner = corner.contiguous()
    return tris, corner


def count_faces(tris: torch.Tensor, lo, hi, cells: int) -> int:
    """count(N): the triangles with three distinct cells on the grid with `cells` cells along the longest axis."""
    _, inv_h, dims = choose_grid(lo, hi, cells=cells)
    count = torch.zeros(1, dtype=torch.int64, device=tris.device)
    ops.simp_count_faces_(ops.simp_grid(lo, inv_h, dims), tris, count)
    return int(count.item())


def _first_occurrences(rows: torch.Tensor) -> torch.Tensor:
    """bool [M]: row i of rows int64 [M, 3] equals no earlier row.  Three stable sorts, last column first, leave equal
    rows adjacent and in their original order, so the first of a run is its earliest member."""
    m = rows.shape[0]
    perm = torch.arange(m, device=rows.device)
    for col in (2, 1, 0):
        perm = perm[torch.sort(rows[perm, col], stable=True).indices]
    ordered = rows[perm]
    head = torch.ones(m, dtype=torch.bool, device=rows.device)
    head[1:] = (ordered[1:] != ordered[:-1]).any(dim=1)
    keep = torch.empty(m, dtype=torch.bool, device=rows.device)
    keep[perm] = head
    return keep


def surviving_faces(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(source triangle int64 [M], cell keys int64 [M, 3], duplicates removed) of the output faces: the triangles of
    keys int32 [3F] with three distinct cells, in input order, without the later copies of an earlier face."""
    k3 = keys.view(-1, 3)
    alive = (k3[:, 0] != k3[:, 1]) & (k3[:, 1] != k3[:, 2]) & (k3[:, 0] != k3[:, 2])
    src = torch.nonzero(alive).squeeze(1)
    face_keys = k3[src].long()
    turn = (face_keys.argmin(dim=1, keepdim=True) + torch.arange(3, device=keys.device)) % 3
    keep = _first_occurrences(face_keys.gather(1, turn))  # smallest key first: equal up to cyclic rotation
    return src[keep], face_keys[keep], int(keep.numel() - keep.sum().item())


def simplify(tris_or_verts, faces=None, colors=None, *, cell_size: Optional[float] = None, grid: Optional[int] = None,
             target_faces: Optional[int] = None, placement: str = "quadric", origin: Optional[Sequence[float]] = None,
             device=None, fold_shape: str = "auto") -> SimplifiedMesh:
    """
    Simplify triangles [F, 3, 3], or verts [V, 3] with faces [F, 3] (arrays or tensors), onto a grid of cubic cells
    given by exactly one of cell_size (the cell edge), grid (cells along the longest axis of the bounding box) and
    target_faces (the finest such grid, up to 1024 cells, that leaves at most that many faces).  colors: uint8, one RGB
    per vertex (with faces) or per corner ([F, 3, 3] or [3F, 3]); each output vertex gets the rounded mean of its
    cell's corners.  placement: "quadric" (default) or "mean".  origin: the grid's origin instead of the corner minimum;
    it may not lie above it.  fold_shape: the launch shape of the per-cell fold ("auto", "groups", "waves"): same bits.

    Returns SimplifiedMesh(verts fp32 [V', 3], faces int32 [M, 3], colors uint8 [V', 3] or None, info) on the GPU;
    info: grid, h, occupied_cells, input_faces, output_faces, duplicates_removed, fallback_cells (output vertices whose
    quadric placement left the neighbourhood of its cell and fell back to the mean) and flipped.  ValueError for bad
    arguments, an empty mesh, non-finite vertices, a grid of 2^31 cells or more, and a result without faces.
    """
    check_size_arguments(cell_size, grid, target_faces, placement)
    if fold_shape not in ops.SIMP_SHAPES:
        raise ValueError(f"fold_shape must be one of {tuple(ops.SIMP_SHAPES)}, got {fold_shape!r}")
    tris, corner_colors = _as_soup(tris_or_verts, faces, colors, device)
    n_tris = tris.shape[0]
    pts = tris.view(-1, 3)
    lo = pts.amin(dim=0).cpu().numpy()
    hi = pts.amax(dim=0).cpu().numpy()
    if origin is not None:
        origin = np.asarray(origin, dtype=np.float32).reshape(3)
        if not (np.isfinite(origin).all() and (origin <= lo).all()):
            raise ValueError(f"origin {origin.tolist()} must be finite and at or below the corner minimum {lo.tolist()}")
        lo = origin
    if target_faces is not None:
        grid = bisect_cells(lambda n: count_faces(tris, lo, hi, n), int(target_faces))
    h, inv_h, dims = choose_grid(lo, hi, cell_size=cell_size, cells=None if grid is None else int(grid))
    g = ops.simp_grid(lo, inv_h, dims)

    keys = ops.simp_cell_keys(g, pts)
    sorted_keys, order = torch.sort(keys, stable=True)
    cells, lengths = torch.unique_consecutive(sorted_keys, return_counts=True)
    seg_start = torch.zeros(cells.numel() + 1, dtype=torch.int32, device=tris.device)
    seg_start[1:] = torch.cumsum(lengths, dim=0)
    counts, sums, col_sums = ops.simp_accumulate(tris, keys, order.to(torch.int32), seg_start, corner_colors,
                                                 fold_shape)
    cell_verts, cell_colors, fell_back = ops.simp_place(g, h, cells, counts, sums, col_sums, placement)

    src, face_keys, duplicates = surviving_faces(keys)
    if face_keys.shape[0] == 0:
        raise ValueError(f"no faces are left on the grid {dims} (h = {h:.6g})"
                         + (f": target_faces = {target_faces} is too small" if target_faces is not None else ""))
    used = torch.unique(face_keys)
    slot = torch.searchsorted(cells.long(), used)
    out_faces = torch.searchsorted(used, face_keys.reshape(-1)).reshape(-1, 3).to(torch.int32).contiguous()
    out_verts = cell_verts[slot].contiguous()
    flipped = ops.simp_flipped(tris, src.to(torch.int32), out_faces, out_verts)
    info = dict(grid=tuple(dims), h=h, occupied_cells=int(cells.numel()), input_faces=int(n_tris),
                output_faces=int(out_faces.shape[0]), duplicates_removed=duplicates,
                fallback_cells=int(fell_back[slot].sum().item()), flipped=int(flipped.item()))
    return SimplifiedMesh(out_verts, out_faces, None if cell_colors is None else cell_colors[slot].contiguous(), info)


def format_info(info: dict):
    """One 'key=value' line per item of info; the grid as AxBxC."""
    return [f"{k}=" + ("x".join(str(n) for n in v) if k == "grid" else (f"{v:.9g}" if isinstance(v, float) else str(v)))
            for k, v in info.items()]

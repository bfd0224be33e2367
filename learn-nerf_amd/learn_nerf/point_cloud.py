"""
Point-cloud export (the reference's Go command point_cloud/main.go): RGB-D views written by render_new_dataset.py are
back-projected into a coloured point cloud, thinned by local density or at random, turned into the distance field
thickness - dist(x, cloud) on a grid of spacing delta, meshed by marching cubes at level 0 (csrc/mesh.hip) and coloured
per vertex from the nearest point.  The three KD-tree queries of the Go program (k-th neighbour, distance, nearest
neighbour) are the exact grid search of csrc/pointcloud.hip, whose header fixes the conventions; PointGrid wraps it.
"""
import ctypes
import math
import os
from typing import Optional, Tuple

import numpy as np
import torch

from learn_nerf import _lib as L
from learn_nerf.dataset import CameraView

F32 = torch.float32
INT32_MAX = 2 ** 31 - 1
NO_DEPTH = 0xFFFF  # a pixel whose ray hit nothing (point_cloud/main.go:166)

# Cell-edge rule of PointGrid.  With d the number of axes of non-zero extent e_a, h = (2 * prod e_a / n)^(1/d): about two
# points per cell of a cloud that fills its box, more for a surface.  h is then raised until every dimension
# floor(e_a / h) + 1 is at most MAX_GRID_DIM and the cells number at most MAX_GRID_CELLS (a cell_start array of 64 MiB);
# a cloud of zero extent is one cell of edge 1.  Results do not depend on h, only the time does.
TARGET_POINTS_PER_CELL = 2.0
MAX_GRID_DIM = 4096
MAX_GRID_CELLS = 2 ** 24

# point_field refuses a volume of more points than this (4 bytes each, plus 2 for marching cubes)
MAX_FIELD_POINTS = 2 ** 29


def _depth_array(image) -> np.ndarray:
    """uint16 z-depth of a PIL image as render_new_dataset.py writes it: mode 'I' or 'I;16' depending on the PIL."""
    if image.mode not in ("I", "I;16", "I;16B", "I;16L"):
        raise ValueError(f"depth image has mode {image.mode!r}, expected a 16-bit greyscale PNG ('I' or 'I;16')")
    depth = np.asarray(image).astype(np.int64)
    if depth.ndim != 2 or depth.min() < 0 or depth.max() > NO_DEPTH:
        raise ValueError("depth image values do not fit 16 bits")
    return depth


def read_rgbd_view(json_path: str, depth_path: str, color_path: str, max_depth: float,
                   device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    One view back-projected (point_cloud/main.go:49-86, 134-175): points [n, 3] fp32 and colours [n, 3] fp32 in [0, 1]
    of the pixels whose depth is not 0xffff, in raster order.  z = depth / 65535 * max_depth is the distance along the
    camera direction, so point = origin + dir * z / (dir . camera_direction) with dir the pixel's unit direction of
    CameraView.bare_rays (lnrf_camera_rays on a GPU device).  Elementwise torch: works on CPU tensors too.
    """
    from PIL import Image

    view = CameraView.from_json(json_path)
    with Image.open(depth_path) as image:
        depth = _depth_array(image)
    with Image.open(color_path) as image:
        color = np.asarray(image.convert("RGB"))
    if depth.shape != color.shape[:2]:
        raise ValueError(f"mismatched size of RGB and depth images: colour {color.shape[:2]} in {color_path}, "
                         f"depth {depth.shape} in {depth_path}")
    device = torch.device("cpu" if device is None else device)
    height, width = depth.shape
    keep = torch.from_numpy(depth.reshape(-1) != NO_DEPTH).to(device)
    rays = view.bare_rays(width, height, device=device).to(device)
    origin, direction = rays[:, 0][keep], rays[:, 1][keep]
    z = torch.from_numpy(depth.reshape(-1).astype(np.float32)).to(device)[keep] / 65535 * max_depth
    axis = torch.tensor(view.camera_direction, dtype=F32, device=device)
    points = origin + direction * (z / (direction * axis).sum(-1))[:, None]
    colors = torch.from_numpy(color.reshape(-1, 3).copy()).to(device)[keep].to(F32) / 255
    return points.contiguous(), colors.contiguous()


def read_dataset(data_dir: str, max_depth: float, device=None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Views 00000, 00001, ... of `data_dir` until a NNNNN.json is missing -> (points, colours, number of views)."""
    points, colors = [], []
    while True:
        stem = os.path.join(data_dir, f"{len(points):05d}")
        if not os.path.exists(stem + ".json"):
            break
        p, c = read_rgbd_view(stem + ".json", stem + "_depth.png", stem + ".png", max_depth, device)
        points.append(p)
        colors.append(c)
    if not points:
        device = torch.device("cpu" if device is None else device)
        return torch.empty((0, 3), dtype=F32, device=device), torch.empty((0, 3), dtype=F32, device=device), 0
    return torch.cat(points), torch.cat(colors), len(points)


def choose_grid(lo, hi, n: int, cell_edge: Optional[float] = None):
    """(h as float32, dims) of the search grid over the box [lo, hi] of n points: the rule above, or a forced edge."""
    extent = [float(b) - float(a) for a, b in zip(lo, hi)]
    if cell_edge is not None:
        h = np.float32(cell_edge)
        if not (h > 0 and np.isfinite(h)):
            raise ValueError(f"cell_edge must be positive and finite, got {cell_edge}")
    else:
        live = [e for e in extent if e > 0]
        h = np.float32((TARGET_POINTS_PER_CELL * math.prod(live) / max(n, 1)) ** (1 / len(live)) if live else 1.0)
        if not (h > 0 and np.isfinite(h)):
            h = np.float32(max(live))

    def dims_of(edge):
        return [int(math.floor(e / float(edge))) + 1 for e in extent]

    dims = dims_of(h)
    while max(dims) > MAX_GRID_DIM or math.prod(dims) > MAX_GRID_CELLS:
        if cell_edge is not None:
            raise ValueError(f"cell_edge {cell_edge} gives a grid of {dims} cells: at most {MAX_GRID_DIM} per axis and "
                             f"{MAX_GRID_CELLS} in all")
        h = np.float32(float(h) * 1.1)
        dims = dims_of(h)
    return h, dims


class PointGrid:
    """
    The points [n, 3] (GPU, fp32, finite) sorted into a uniform grid of cubic cells, for exact k-th-neighbour and
    nearest-point queries (csrc/pointcloud.hip).  cell_edge forces the cell edge; by default the rule above chooses it.
    """

    def __init__(self, points: torch.Tensor, cell_edge: Optional[float] = None):
        points = _check_points(points, "points")
        n = points.shape[0]
        if n > INT32_MAX:
            raise ValueError(f"{n} points do not fit in int32 indices")
        self.n = n
        dev = points.device
        if n:
            lo, hi = points.min(dim=0).values.tolist(), points.max(dim=0).values.tolist()
        else:
            lo = hi = [0.0, 0.0, 0.0]
        self.h, self.dims = choose_grid(lo, hi, n, cell_edge)
        self.grid = L.PcGrid((ctypes.c_float * 3)(*lo), float(self.h), (ctypes.c_int32 * 3)(*self.dims), 0)
        ids = self.cell_ids(points)
        ids, order = torch.sort(ids, stable=True)
        self.order = order.to(torch.int32)
        self.sorted_points = points[order].contiguous()
        cells = torch.arange(math.prod(self.dims) + 1, dtype=torch.int32, device=dev)
        self.cell_start = torch.searchsorted(ids, cells, out_int32=True).contiguous()

    def cell_ids(self, points: torch.Tensor) -> torch.Tensor:
        """int32 [m]: the (clamped) cell of each point."""
        ids = torch.empty(points.shape[0], dtype=torch.int32, device=points.device)
        L.check(L.lib().lnrf_pc_cell_ids(ctypes.byref(self.grid), L.ptr(points), points.shape[0],
                                         L.ptr(ids, torch.int32), L.stream()), "pc_cell_ids")
        return ids

    def _in_cell_order(self, queries: torch.Tensor, sort: bool):
        queries = _check_points(queries, "queries")
        if queries.shape[0] > INT32_MAX:
            raise ValueError(f"{queries.shape[0]} queries do not fit in int32 indices")
        if not sort or queries.shape[0] == 0:
            return queries, None
        perm = torch.sort(self.cell_ids(queries), stable=True).indices
        return queries[perm].contiguous(), perm

    def knn_dist2(self, queries: torch.Tensor, k: int, sort: bool = True) -> torch.Tensor:
        """fp32 [m]: squared distance from each query to its k-th nearest point (1 <= k <= 32), a query that is one of
        the points counting itself; +inf with fewer than k points.  sort=False when the queries are spatially coherent
        already."""
        q, perm = self._in_cell_order(queries, sort)
        out = torch.empty(q.shape[0], dtype=F32, device=q.device)
        L.check(L.lib().lnrf_pc_knn_dist2(ctypes.byref(self.grid), L.ptr(self.sorted_points),
                                          L.ptr(self.cell_start, torch.int32), self.n, L.ptr(q), q.shape[0], int(k),
                                          L.ptr(out), L.stream()), "pc_knn_dist2")
        return out if perm is None else torch.empty_like(out).index_copy_(0, perm, out)

    def nearest(self, queries: torch.Tensor, max_radius: float = math.inf,
                sort: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """(d2 fp32 [m], index int32 [m]) of the nearest point within max_radius of each query, the lowest index among
        equal distances; (+inf, -1) without one.  Queries may lie anywhere."""
        q, perm = self._in_cell_order(queries, sort)
        d2 = torch.empty(q.shape[0], dtype=F32, device=q.device)
        idx = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
        L.check(L.lib().lnrf_pc_nearest(ctypes.byref(self.grid), L.ptr(self.sorted_points),
                                        L.ptr(self.order, torch.int32), L.ptr(self.cell_start, torch.int32), self.n,
                                        L.ptr(q), q.shape[0], float(max_radius), L.ptr(d2), L.ptr(idx, torch.int32),
                                        L.stream()), "pc_nearest")
        if perm is None:
            return d2, idx
        return torch.empty_like(d2).index_copy_(0, perm, d2), torch.empty_like(idx).index_copy_(0, perm, idx)


def _check_points(points: torch.Tensor, what: str) -> torch.Tensor:
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: expected shape [n, 3], got {tuple(points.shape)}")
    if not points.is_cuda:
        raise RuntimeError(f"{what}: the neighbour search needs tensors on a ROCm GPU device (no CPU fallback)")
    points = points.to(F32).contiguous()
    if not torch.isfinite(points).all():
        raise ValueError(f"{what}: non-finite coordinates")
    return points


def knn_dist2(points: torch.Tensor, k: int) -> torch.Tensor:
    """Squared distance from every point of the cloud to its k-th nearest point, itself included (the density measure
    of point_cloud/main.go:177-183)."""
    grid = PointGrid(points)
    # the points are the queries: reuse their cell order instead of sorting them again
    out = grid.knn_dist2(grid.sorted_points, k, sort=False)
    return torch.empty_like(out).index_copy_(0, grid.order.long(), out)


def subsample(points: torch.Tensor, colors: torch.Tensor, max_points: int, sort_density: bool = False, k: int = 5,
              seed: int = 0, knn=knn_dist2) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    point_cloud/main.go:88-102.  At or under max_points everything is returned unchanged.  With sort_density the points
    with the smallest k-th-neighbour distance, i.e. the densest, are kept: a stable ascending sort by knn(points, k), so
    ties keep their original order (the Go sort is not stable).  Otherwise the first max_points of
    np.random.RandomState(seed).permutation(n) (the Go program shuffles with its global generator).
    """
    n = points.shape[0]
    if n <= max_points:
        return points, colors
    if sort_density:
        keep = torch.sort(knn(points, k), stable=True).indices[:max_points]
    else:
        keep = torch.from_numpy(np.random.RandomState(seed).permutation(n)[:max_points]).to(points.device)
    return points[keep].contiguous(), colors[keep].contiguous()


def field_axes(lo, hi, thickness: float, delta: float):
    """Per axis the float64 grid lo_a - pad + i * delta, i < ceil((hi_a - lo_a + 2 pad) / delta) + 1, pad = thickness +
    delta, so the sphere of every point lies inside the grid with a layer of outside values around it."""
    pad = float(thickness) + float(delta)
    axes = []
    for a, b in zip(lo, hi):
        count = int(math.ceil((float(b) - float(a) + 2 * pad) / float(delta))) + 1
        axes.append(float(a) - pad + np.arange(count, dtype=np.float64) * float(delta))
    return axes


def point_field(points: torch.Tensor, thickness: float, delta: float, batch_size: int = 1 << 22,
                max_field_points: int = MAX_FIELD_POINTS, grid: Optional[PointGrid] = None):
    """
    -> (volume fp32 [nx, ny, nz], origin float64 [3], dims): thickness - sqrt(d2 to the nearest point) in fp32 at the
    grid points of field_axes (rounded to fp32), thickness - max_radius where no point lies within max_radius =
    thickness + delta.  Inside the solid of point_cloud/main.go:112-118 is volume > 0.  Built in chunks of batch_size grid
    points generated from the linear index; `grid` is a PointGrid of the same points, if the caller has one.
    """
    if not (thickness > 0 and delta > 0 and math.isfinite(thickness) and math.isfinite(delta)):
        raise ValueError("thickness and delta must be positive and finite")
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    if points.shape[0] == 0:
        raise ValueError("no points")
    lo, hi = points.min(dim=0).values.tolist(), points.max(dim=0).values.tolist()
    axes64 = field_axes(lo, hi, thickness, delta)
    dims = [len(a) for a in axes64]
    total = math.prod(dims)
    if total > max_field_points:
        raise ValueError(f"a field of {dims[0]} x {dims[1]} x {dims[2]} = {total} points exceeds the budget of "
                         f"{max_field_points}: use a larger --delta")
    grid = PointGrid(points) if grid is None else grid
    dev = points.device
    axes = [torch.from_numpy(a.astype(np.float32)).to(dev) for a in axes64]
    t32 = np.float32(thickness)
    max_radius = np.float32(float(thickness) + float(delta))
    outside = float(t32 - max_radius)
    out = torch.empty(total, dtype=F32, device=dev)
    ny, nz = dims[1], dims[2]
    for start in range(0, total, batch_size):
        idx = torch.arange(start, min(start + batch_size, total), dtype=torch.int64, device=dev)
        q = torch.stack([axes[0][idx // (ny * nz)], axes[1][(idx // nz) % ny], axes[2][idx % nz]], dim=1).contiguous()
        d2, nearest = grid.nearest(q, float(max_radius), sort=False)  # consecutive queries are neighbours along z
        # fp32 square root by way of float64: correctly rounded whatever the device's fp32 sqrt does
        value = float(t32) - d2.double().sqrt().to(F32)
        out[start:start + idx.numel()] = torch.where(nearest >= 0, value, torch.full_like(value, outside))
    origin = np.array([a[0] for a in axes64], dtype=np.float64)
    return out.view(*dims), origin, dims


def extract(points: torch.Tensor, colors: torch.Tensor, thickness: float, delta: float, batch_size: int = 1 << 22,
            max_field_points: int = MAX_FIELD_POINTS) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """
    The surface of the union of the balls of radius `thickness` about the points, with the colour of the nearest point
    at every vertex -> (verts [V, 3] fp32 in world coordinates, faces [F, 3] int32 outward, colours [V, 3] fp32).
    """
    from learn_nerf.mesh import marching_cubes

    grid = PointGrid(points)
    volume, origin, _ = point_field(points, thickness, delta, batch_size, max_field_points, grid)
    verts, faces = marching_cubes(volume, 0.0)
    world = (origin + verts.cpu().numpy().astype(np.float64) * float(delta)).astype(np.float32)
    if len(world) == 0:
        return world, faces.cpu().numpy(), np.zeros((0, 3), np.float32)
    _, nearest = grid.nearest(torch.from_numpy(world).to(points.device))
    return world, faces.cpu().numpy(), colors[nearest.long()].cpu().numpy()


def _rgb8(colors) -> np.ndarray:
    return np.clip(np.rint(np.asarray(colors, dtype=np.float64) * 255), 0, 255).astype(np.uint8)


def write_colored_obj(path: str, verts, faces, colors) -> None:
    """'v x y z r g b' (5 decimals each, colours in [0, 1]), then 1-based 'f a b c'."""
    rows = np.concatenate([np.asarray(verts, np.float32), np.asarray(colors, np.float32)], axis=1).tolist()
    with open(path, "w") as f:
        f.write("".join("v " + " ".join(f"{x:.5f}" for x in row) + "\n" for row in rows))
        f.write("".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in np.asarray(faces).reshape(-1, 3).tolist()))


def write_ply(path: str, verts, colors, faces=None) -> None:
    """Binary little-endian PLY: float32 x y z and uint8 red green blue per vertex, then (when there are any) faces as
    a uchar count of 3 and three int32 vertex indices.  For the mesh and for a bare cloud.  colors = None leaves the
    colour properties out."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.zeros((0, 3), np.int32) if faces is None else np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(verts)}", "property float x",
              "property float y", "property float z"]
    if colors is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    if len(faces):
        header += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
    header.append("end_header")
    vrec = np.zeros(len(verts), dtype=[("xyz", "<f4", (3,))] + ([("rgb", "u1", (3,))] if colors is not None else []))
    vrec["xyz"] = verts
    if colors is not None:
        vrec["rgb"] = _rgb8(colors).reshape(-1, 3)
    frec = np.zeros(len(faces), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    frec["n"] = 3
    frec["idx"] = faces
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())

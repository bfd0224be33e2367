"""
Mesh export (scripts/marching_cubes.py:20-117): the fine model's density on an R^3 grid inside the scene's bounding box,
occupancy 1 - exp(-sigma), one layer of zero padding, marching cubes at the threshold (lnrf_mc_count / lnrf_mc_emit,
csrc/mesh.hip, whose header fixes the vertex / face conventions), then the reference's frame and OBJ / STL writers.
"""
import struct
from typing import Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from learn_nerf import _lib as L

F32 = torch.float32
INT32_MAX = 2 ** 31 - 1


def grid_coordinates(bbox_min: Sequence[float], bbox_max: Sequence[float], resolution: int, start: int = 0,
                     count: int = None, device=None) -> torch.Tensor:
    """
    Rows [start, start + count) of the reference's grid_coordinates(...).reshape([-1, 3]) (scripts/marching_cubes.py:
    86-95) in float32: point (i, j, k), linear index (i*R + j)*R + k, is at (x_i, y_j, z_k) with x along axis 0.
    Generated from the linear index on `device`, so the full [R^3, 3] array is never built.
    """
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return _grid_rows(_axes(bbox_min, bbox_max, resolution, device), start, count)


def _axes(bbox_min, bbox_max, resolution: int, device):
    """Per axis the reference's np.linspace(min, max, R) (float64) as the float32 the model sees, on `device`."""
    return [torch.from_numpy(np.linspace(lo, hi, num=resolution, dtype=np.float64).astype(np.float32)).to(device)
            for lo, hi in zip(bbox_min, bbox_max)]


def _grid_rows(axes, start: int, count: int = None) -> torch.Tensor:
    r = axes[0].numel()
    total = r ** 3
    count = total - start if count is None else count
    if not (0 <= start and count >= 0 and start + count <= total):
        raise ValueError(f"rows [{start}, {start + count}) outside a grid of {total} points")
    idx = torch.arange(start, start + count, dtype=torch.int64, device=axes[0].device)
    return torch.stack([axes[0][idx // (r * r)], axes[1][(idx // r) % r], axes[2][idx % r]], dim=1).contiguous()


def density_grid(model, params, bbox_min, bbox_max, resolution: int, batch_size: int) -> torch.Tensor:
    """sigma [R, R, R] of `model` at the grid points, batch_size points per forward, direction d = 0
    (scripts/marching_cubes.py:41-47)."""
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    flat = model.flat(params)
    r = int(resolution)
    axes = _axes(bbox_min, bbox_max, r, flat.device)  # once: no host-to-device copy per chunk
    out = torch.empty(r ** 3, dtype=F32, device=flat.device)
    for start in range(0, r ** 3, batch_size):
        n = min(batch_size, r ** 3 - start)
        x = _grid_rows(axes, start, n)
        density, _, _, _ = model.forward_points(flat, x, torch.zeros_like(x), save=False)
        out[start:start + n] = density.reshape(-1)
    return out.view(r, r, r)


def marching_cubes(volume: torch.Tensor, level: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """
    Surface of {volume > level} of a GPU fp32 volume [nx, ny, nz] (each >= 2): verts [V, 3] fp32 in index space and
    faces [F, 3] int32, outward, in the deterministic order of csrc/mesh.hip.  An empty surface is not an error.
    """
    if volume.dim() != 3:
        raise ValueError(f"expected a 3-d volume, got shape {tuple(volume.shape)}")
    volume = volume.contiguous()
    nx, ny, nz = volume.shape
    lib = L.lib()
    nbytes = lib.lnrf_mc_scratch_bytes(nx, ny, nz)
    if nbytes < 0:
        raise ValueError(f"marching cubes needs every dimension >= 2, got {tuple(volume.shape)}")
    dev = volume.device
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    L.check(lib.lnrf_mc_count(L.ptr(volume), nx, ny, nz, float(level), L.ptr(scratch, torch.uint8),
                              L.ptr(counts, torch.int64), L.stream()), "mc_count")
    n_verts, n_faces = counts.tolist()  # the one read-back between the two passes
    if max(n_verts, n_faces) > INT32_MAX:
        raise ValueError(f"{n_verts} vertices / {n_faces} faces do not fit in int32 ids: use a coarser volume")
    verts = torch.empty((n_verts, 3), dtype=F32, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    if n_verts:
        L.check(lib.lnrf_mc_emit(L.ptr(volume), nx, ny, nz, float(level), L.ptr(scratch, torch.uint8), n_verts,
                                 n_faces, L.ptr(verts), L.ptr(faces, torch.int32), L.stream()), "mc_emit")
    return verts, faces


def filter_occupancy(occupancy: torch.Tensor, threshold: float, min_component: int = 1, keep_largest: int = None,
                     connectivity: int = 26) -> Tuple[torch.Tensor, dict]:
    """
    Floater removal on an occupancy volume [nx, ny, nz] (additive; learn_nerf/components.py): the foreground is
    occupancy > threshold, marching cubes' "inside" (so NaN is background); the points of every component smaller than
    `min_component` points or, with `keep_largest`, beyond the largest `keep_largest` components are set to 0, every
    other point keeps its value.  -> (filtered copy, info of keep_components).
    """
    from .components import keep_components

    inside = occupancy > threshold
    keep, info = keep_components(inside, min_cells=min_component, keep_largest=keep_largest, connectivity=connectivity)
    return occupancy.masked_fill(inside & (keep == 0), 0.0), info


def extract_mesh(model, params, bbox_min, bbox_max, resolution: int, batch_size: int, threshold: float,
                 min_component: int = 1, keep_largest: int = None, connectivity: int = 26,
                 info: dict = None) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """
    scripts/marching_cubes.py:38-66: occupancy 1 - exp(-sigma) (fp32) on the grid, one layer of zero padding, marching
    cubes at `threshold`.  -> (verts [V, 3] in padded index space, faces [F, 3], largest occupancy of the grid).
    Additive: with min_component > 1 or keep_largest the volume goes through filter_occupancy first, whose info is
    copied into `info` when one is given; with the defaults no component kernel runs.
    """
    sigma = density_grid(model, params, bbox_min, bbox_max, resolution, batch_size)
    occupancy = 1 - torch.exp(-sigma)
    largest = float(occupancy.max())
    if min_component != 1 or keep_largest is not None:
        occupancy, found = filter_occupancy(occupancy, threshold, min_component, keep_largest, connectivity)
        if info is not None:
            info.update(found)
    padded = F.pad(occupancy, (1, 1, 1, 1, 1, 1), mode="constant", value=0.0)
    verts, faces = marching_cubes(padded, threshold)
    return verts, faces, largest


def reference_frame(verts, faces, bbox_min, bbox_max, resolution: int) -> Tuple[np.ndarray, np.ndarray]:
    """
    The reference's output frame (scripts/marching_cubes.py:71-74): columns 0 and 2 swapped, scaled by
    (bbox_max - bbox_min) / R in float32 (column 0 by the x size, as there), centred on the vertex extent.
    """
    v = np.asarray(verts, dtype=np.float32)[:, ::-1].copy()
    scale = ((np.asarray(bbox_max, np.float64) - np.asarray(bbox_min, np.float64)) / resolution).astype(np.float32)
    v *= scale
    if len(v):
        v -= (v.max(axis=0) + v.min(axis=0)) / np.float32(2)
    # swapping two coordinates is a reflection: swap two indices of every face to keep it outward
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3)[:, [0, 2, 1]])
    return v, f


def world_frame(verts, bbox_min, bbox_max, resolution: int) -> np.ndarray:
    """Scene coordinates of padded index-space vertices: bbox_min + (a - 1) * (bbox_max - bbox_min) / (R - 1) per
    axis, no swap (unpadded grid point a - 1 lies at that linspace value)."""
    lo = np.asarray(bbox_min, np.float64)
    step = (np.asarray(bbox_max, np.float64) - lo) / (resolution - 1)
    return (lo + (np.asarray(verts, np.float64) - 1) * step).astype(np.float32)


def write_obj(path: str, verts, faces) -> None:
    """The reference's OBJ text (scripts/marching_cubes.py:98-104): 'v x y z' (5 decimals), then 1-based 'f a b c'."""
    vertex_strs = [f"v {x:.5f} {y:.5f} {z:.5f}" for x, y, z in np.asarray(verts).tolist()]
    face_strs = [f"f {a + 1} {b + 1} {c + 1}" for a, b, c in np.asarray(faces).tolist()]
    with open(path, "w") as f:
        f.write("\n".join(vertex_strs) + "\n")
        f.write("\n".join(face_strs) + "\n")


def write_stl(path: str, verts, faces) -> None:
    """
    Binary STL, the layout the reference's write_stl aims at (scripts/marching_cubes.py:106-117, which cannot run):
    80 zero bytes, uint32 triangle count, then per triangle the unit facet normal by the right-hand rule (zero for a
    degenerate triangle), the 3 vertices (12 float32 LE in all) and 2 zero bytes.
    """
    v = np.asarray(verts, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tri = v[f]
    n = np.cross((tri[:, 1] - tri[:, 0]).astype(np.float64), (tri[:, 2] - tri[:, 0]).astype(np.float64))
    norm = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.divide(n, norm, out=np.zeros_like(n), where=norm > 0)
    rec = np.zeros(len(f), dtype=[("normal", "<f4", (3,)), ("verts", "<f4", (3, 3)), ("attr", "<u2")])
    rec["normal"] = n
    rec["verts"] = tri
    with open(path, "wb") as fh:
        fh.write(b"\x00" * 80)
        fh.write(struct.pack("<I", len(f)))
        fh.write(rec.tobytes())

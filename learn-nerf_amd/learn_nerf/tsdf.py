"""
TSDF fusion (additive; Curless & Levoy 1996): the RGB-D views written by render_new_dataset.py are fused into a voxel
grid over the scene's bounding box, every voxel averaging the truncated signed distance to the depth each view saw
there, and marching cubes at level 0 (csrc/mesh.hip) turns the grid into one coloured surface.  Free space seen by any
view is carved, space that was only ever seen behind a surface is solid (which fills holes), and a depth pixel is used
at its nearest voxel projection only, so a silhouette pixel puts no point in mid-air.  The integration, the volume and
the vertex colours are lnrf_tsdf_* (csrc/tsdf.hip; csrc/tsdf_geom.h fixes the arithmetic); TsdfVolume drives them.
"""
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from learn_nerf import _lib as L
from learn_nerf.dataset import CameraView
from learn_nerf.point_cloud import _depth_array

F32 = torch.float32
INT32_MAX = 2 ** 31 - 1

# lnrf_tsdf_view (include/lnrf.h), 88 bytes
VIEW_DTYPE = np.dtype([("origin", "<f4", (3,)), ("inv", "<f4", (9,)), ("zaxis", "<f4", (3,)), ("width", "<i4"),
                       ("height", "<i4"), ("pad_", "<i4"), ("depth_offset", "<i8"), ("color_offset", "<i8")])
assert VIEW_DTYPE.itemsize == 88

# integrate() uploads views in chunks of at most this many image bytes (5 per pixel); any chunking gives the same bits
DEFAULT_CHUNK_BYTES = 256 << 20


def read_rgbd_views(data_dir: str) -> Tuple[List[CameraView], List[np.ndarray], List[np.ndarray]]:
    """Views 00000, 00001, ... of `data_dir` until a NNNNN.json is missing -> (cameras, depths uint16 [H, W], colours
    uint8 [H, W, 3]).  The errors of point_cloud.read_rgbd_view for a depth image of the wrong mode or another size
    than the colour image."""
    from PIL import Image

    cameras, depths, colors = [], [], []
    while True:
        stem = os.path.join(data_dir, f"{len(cameras):05d}")
        if not os.path.exists(stem + ".json"):
            break
        depth_path, color_path = stem + "_depth.png", stem + ".png"
        with Image.open(depth_path) as image:
            depth = _depth_array(image)
        with Image.open(color_path) as image:
            color = np.asarray(image.convert("RGB"))
        if depth.shape != color.shape[:2]:
            raise ValueError(f"mismatched size of RGB and depth images: colour {color.shape[:2]} in {color_path}, "
                             f"depth {depth.shape} in {depth_path}")
        cameras.append(CameraView.from_json(stem + ".json"))
        depths.append(depth.astype(np.uint16))
        colors.append(np.ascontiguousarray(color, dtype=np.uint8))
    return cameras, depths, colors


def pack_views(cameras: Sequence[CameraView], sizes: Sequence[Tuple[int, int]]) -> np.ndarray:
    """
    -> lnrf_tsdf_view descriptors (VIEW_DTYPE [n]) of `cameras` with images of `sizes` = (width, height) each, the
    images packed one after the other in view order.  inv holds the rows of M^-1 for M with columns tan(x_fov/2) x_axis,
    tan(y_fov/2) y_axis and camera_direction, inverted in float64 and rounded once, so a point p = origin + M (u, v, 1) s
    gives back (u s, v s, s): the pixel fractions of CameraView.bare_rays, also when the axes are not orthonormal.
    """
    if len(cameras) != len(sizes):
        raise ValueError(f"{len(cameras)} cameras but {len(sizes)} sizes")
    out = np.zeros(len(cameras), dtype=VIEW_DTYPE)
    pixels = 0
    for i, (cam, (width, height)) in enumerate(zip(cameras, sizes)):
        width, height = int(width), int(height)
        if width < 2 or height < 2 or width * height > INT32_MAX:
            raise ValueError(f"view {i}: an image of {width} x {height} pixels; each side must be at least 2")
        m = np.stack([np.asarray(cam.x_axis, np.float64) * math.tan(cam.x_fov / 2),
                      np.asarray(cam.y_axis, np.float64) * math.tan(cam.y_fov / 2),
                      np.asarray(cam.camera_direction, np.float64)], axis=1)
        if not np.isfinite(m).all() or np.linalg.matrix_rank(m) < 3:
            raise ValueError(f"view {i}: x_axis, y_axis and camera_direction are linearly dependent or not finite")
        inv = np.linalg.inv(m)
        out[i]["origin"] = np.asarray(cam.camera_origin, np.float64)
        out[i]["inv"] = inv.reshape(9)
        out[i]["zaxis"] = np.asarray(cam.camera_direction, np.float64)
        out[i]["width"], out[i]["height"] = width, height
        out[i]["depth_offset"], out[i]["color_offset"] = pixels, 3 * pixels
        pixels += width * height
    if not (np.isfinite(out["inv"]).all() and np.isfinite(out["origin"]).all()):
        raise ValueError("non-finite camera parameters")
    return out


class TsdfVolume:
    """
    The fusion state over the box [bbox_min, bbox_max]: resolution^3 grid points (or a (nx, ny, nz) triple) at the
    linspace coordinates of learn_nerf.mesh, on a ROCm GPU `device` (there is no CPU fallback).  trunc =
    truncation_voxels * the largest grid step, computed in float64 and rounded once to fp32; max_depth is the z-depth of
    a white depth pixel; with carve a 0xFFFF pixel (nothing hit) marks the voxels on its ray as free space.
    """

    def __init__(self, bbox_min, bbox_max, resolution, truncation_voxels: float = 3.0, max_depth: float = 10.0,
                 carve: bool = True, device=None):
        from learn_nerf.mesh import _axes

        dims = [int(resolution)] * 3 if np.ndim(resolution) == 0 else [int(r) for r in resolution]
        if len(dims) != 3 or min(dims) < 2:
            raise ValueError(f"resolution must be one number or three, each at least 2, got {resolution!r}")
        if math.prod(d + 2 for d in dims) > INT32_MAX:
            raise ValueError(f"a grid of {dims} points exceeds the int32 ids of marching cubes")
        lo, hi = [float(v) for v in bbox_min], [float(v) for v in bbox_max]
        if len(lo) != 3 or len(hi) != 3 or not all(b > a for a, b in zip(lo, hi)):
            raise ValueError("bbox_max must exceed bbox_min on every axis")
        if not (truncation_voxels > 0 and math.isfinite(truncation_voxels)):
            raise ValueError("truncation_voxels must be positive and finite")
        if not (max_depth > 0 and math.isfinite(max_depth)):
            raise ValueError("max_depth must be positive and finite")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("TSDF fusion needs a ROCm GPU device (no CPU fallback)")
        self.bbox_min, self.bbox_max, self.dims = lo, hi, dims
        self.trunc = float(np.float32(float(truncation_voxels) * max((b - a) / (d - 1) for a, b, d in zip(lo, hi, dims))))
        self.max_depth = float(np.float32(max_depth))
        self.carve = bool(carve)
        self.device = device
        self.axes = [_axes((a,), (b,), d, device)[0].contiguous() for a, b, d in zip(lo, hi, dims)]
        n = math.prod(dims)
        self.sum_t = torch.zeros(n, dtype=F32, device=device)
        self.n_obs = torch.zeros(n, dtype=torch.int32, device=device)
        self.behind = torch.zeros(n, dtype=torch.uint8, device=device)
        self.rgb_sum = torch.zeros((n, 3), dtype=torch.int32, device=device)
        self.n_col = torch.zeros(n, dtype=torch.int32, device=device)
        self.n_views = 0

    def integrate(self, cameras: Sequence[CameraView], depths: Sequence[np.ndarray], colors: Sequence[np.ndarray],
                  chunk_bytes: int = DEFAULT_CHUNK_BYTES) -> None:
        """Fuses the views, in order: depths uint16 [H, W] z-depth images (0xFFFF = nothing hit), colours uint8
        [H, W, 3].  The views are uploaded in chunks of at most chunk_bytes image bytes (one view at least), one launch
        per chunk; the result does not depend on the chunking."""
        if not len(cameras) == len(depths) == len(colors):
            raise ValueError(f"{len(cameras)} cameras, {len(depths)} depth images and {len(colors)} colour images")
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes must be positive")
        depths = [np.ascontiguousarray(d) for d in depths]
        colors = [np.ascontiguousarray(c) for c in colors]
        for i, (d, c) in enumerate(zip(depths, colors)):
            if d.dtype != np.uint16 or d.ndim != 2:
                raise TypeError(f"view {i}: the depth image must be uint16 [H, W], got {d.dtype} {d.shape}")
            if c.dtype != np.uint8 or c.shape != d.shape + (3,):
                raise ValueError(f"view {i}: the colour image must be uint8 {d.shape + (3,)}, got {c.dtype} {c.shape}")
        start = 0
        while start < len(cameras):
            stop, nbytes = start, 0
            while stop < len(cameras) and (stop == start or nbytes + 5 * depths[stop].size <= chunk_bytes):
                nbytes += 5 * depths[stop].size
                stop += 1
            self._integrate_chunk(cameras[start:stop], depths[start:stop], colors[start:stop])
            start = stop

    def upload(self, cameras, depths, colors) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One launch's inputs on the device: (descriptors as bytes, packed depth as int16 bits, packed colour)."""
        views = pack_views(cameras, [(d.shape[1], d.shape[0]) for d in depths])
        dev = self.device
        views_dev = torch.from_numpy(views.view(np.uint8).copy()).to(dev)
        # int16 carries the bits of uint16, which older torch builds cannot hold
        depth_dev = torch.from_numpy(np.concatenate([d.reshape(-1) for d in depths]).view(np.int16)).to(dev)
        color_dev = torch.from_numpy(np.concatenate([c.reshape(-1) for c in colors])).to(dev)
        return views_dev, depth_dev, color_dev

    def integrate_uploaded(self, views_dev: torch.Tensor, depth_dev: torch.Tensor, color_dev: torch.Tensor) -> None:
        """One lnrf_tsdf_integrate launch over the views of upload()."""
        nx, ny, nz = self.dims
        n_views = views_dev.numel() // VIEW_DTYPE.itemsize
        L.check(L.lib().lnrf_tsdf_integrate(
            L.ptr(self.axes[0]), L.ptr(self.axes[1]), L.ptr(self.axes[2]), nx, ny, nz, L.ptr(views_dev, torch.uint8),
            n_views, L.ptr(depth_dev, torch.int16), L.ptr(color_dev, torch.uint8), self.trunc, self.max_depth,
            int(self.carve), L.ptr(self.sum_t), L.ptr(self.n_obs, torch.int32), L.ptr(self.behind, torch.uint8),
            L.ptr(self.rgb_sum, torch.int32), L.ptr(self.n_col, torch.int32), L.stream()), "tsdf_integrate")
        self.n_views += n_views

    def _integrate_chunk(self, cameras, depths, colors) -> None:
        # the uploads are freed on return: the caching allocator reuses them in stream order, after the kernel
        self.integrate_uploaded(*self.upload(cameras, depths, colors))

    def volume(self, unseen: str = "inside") -> torch.Tensor:
        """fp32 [nx+2, ny+2, nz+2] for marching cubes at level 0: -F at the grid points, -1 on the padding layer.  A
        voxel that no view observed is solid with unseen="inside" when some view saw it behind a surface, else free."""
        if unseen not in ("inside", "outside"):
            raise ValueError(f"unseen must be 'inside' or 'outside', got {unseen!r}")
        nx, ny, nz = self.dims
        out = torch.empty((nx + 2, ny + 2, nz + 2), dtype=F32, device=self.device)
        L.check(L.lib().lnrf_tsdf_volume(L.ptr(self.sum_t), L.ptr(self.n_obs, torch.int32),
                                         L.ptr(self.behind, torch.uint8), nx, ny, nz, int(unseen == "inside"),
                                         L.ptr(out), L.stream()), "tsdf_volume")
        return out

    def vertex_colors(self, verts: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """(colours fp32 [V, 3] in [0, 1], number of vertices left grey) for padded index-space vertices [V, 3]."""
        if verts.dim() != 2 or verts.shape[1] != 3:
            raise ValueError(f"expected vertices [V, 3], got {tuple(verts.shape)}")
        verts = verts.contiguous()
        nx, ny, nz = self.dims
        out = torch.empty((verts.shape[0], 3), dtype=F32, device=self.device)
        missing = torch.empty(1, dtype=torch.int32, device=self.device)
        L.check(L.lib().lnrf_tsdf_vertex_colors(L.ptr(verts), verts.shape[0], nx, ny, nz,
                                                L.ptr(self.rgb_sum, torch.int32), L.ptr(self.n_col, torch.int32),
                                                L.ptr(out), L.ptr(missing, torch.int32), L.stream()),
                "tsdf_vertex_colors")
        return out, int(missing.item())

    def counts(self, unseen: str = "inside") -> dict:
        """observed: voxels with an observation; unseen_inside / unseen_outside: the others, by what volume() makes of
        them."""
        seen = self.n_obs > 0
        solid = ~seen & (self.behind != 0) if unseen == "inside" else torch.zeros_like(seen)
        observed, inside = int(seen.sum()), int(solid.sum())
        return dict(observed=observed, unseen_inside=inside, unseen_outside=self.n_obs.numel() - observed - inside)

    def extract(self, unseen: str = "inside", min_component: int = 1, keep_largest: Optional[int] = None,
                connectivity: int = 26) -> Tuple[np.ndarray, np.ndarray, np.ndarray, dict]:
        """
        -> (verts [V, 3] fp32 in scene coordinates, faces [F, 3] int32 outward, colours [V, 3] fp32, info).  With
        min_component > 1 or keep_largest the components of {volume > 0} that are too small or not among the largest
        (learn_nerf/components.py) are set to -1 first; with the defaults no component kernel runs.  info: the counts(),
        uncoloured (vertices left grey) and, when filtering, the info of keep_components.
        """
        from learn_nerf.mesh import marching_cubes, world_frame

        vol = self.volume(unseen)
        info = self.counts(unseen)
        if min_component != 1 or keep_largest is not None:
            from learn_nerf.components import keep_components

            inside = vol > 0
            keep, found = keep_components(inside, min_cells=min_component, keep_largest=keep_largest,
                                          connectivity=connectivity)
            vol = vol.masked_fill(inside & (keep == 0), -1.0)
            info.update(found)
        verts, faces = marching_cubes(vol, 0.0)
        colors, missing = self.vertex_colors(verts)
        info["uncoloured"] = missing
        world = world_frame(verts.cpu().numpy(), self.bbox_min, self.bbox_max, np.asarray(self.dims))
        return world, faces.cpu().numpy(), colors.cpu().numpy(), info

"""
Float64 NumPy versions of the two dataset-diagnostic statistics (learn_nerf/diagnostics.py, csrc/view_stats.hip), for
tests only: the rays of a view by the bare_rays formula (dataset.py:52-78), their hit mask by oracle.render.ray_t_range
(render.py:346-389), and the statistics of scripts/check_bbox.py over the pixels that miss.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from learn_nerf.dataset import CameraView, NeRFView
from oracle import render as OR

F64 = np.float64
STATS_INIT = np.array([0, 0, 0, 0, 255, 255, 255, 0, 0, 0], dtype=np.int64)  # count, sums, minima, maxima


def bare_rays_f64(view, width: int, height: int) -> np.ndarray:
    """[H*W, 2, 3] float64 (origin, unit direction) in raster order; linspace(-1, 1, 1) is [-1]."""
    xs = math.tan(view.x_fov / 2) * np.linspace(-1, 1, num=width, dtype=F64)[None, :, None] * np.asarray(view.x_axis, F64)
    ys = math.tan(view.y_fov / 2) * np.linspace(-1, 1, num=height, dtype=F64)[:, None, None] * np.asarray(view.y_axis, F64)
    directions = (xs + ys + np.asarray(view.camera_direction, F64)).reshape(-1, 3)
    directions = directions / np.linalg.norm(directions, axis=-1, keepdims=True)
    origins = np.broadcast_to(np.asarray(view.camera_origin, F64), directions.shape)
    return np.stack([origins, directions], axis=1)


def miss_reference(view, width: int, height: int, bbox_min, bbox_max, min_t_range: float = 1e-3,
                   epsilon: float = 1e-8):
    """(miss [H*W] bool, margin [H*W] float64): miss = not the mask of ray_t_range; margin = |max_t - min_t| of the
    slab test before the null range is substituted — a ray whose margin is far above fp32 rounding has the same mask
    in any precision."""
    rays = bare_rays_f64(view, width, height)
    bbox = np.array([bbox_min, bbox_max], dtype=F64)
    _, _, mask = OR.ray_t_range(torch.from_numpy(bbox), torch.from_numpy(rays), min_t_range, epsilon)
    ts = (bbox[None] - rays[:, :1]) / (rays[:, 1:2] + epsilon)  # [N, 2, 3] (render.py:370-371)
    min_t = np.maximum(ts.min(axis=1).max(axis=-1), 0.0)  # render.py:374-383
    max_t = ts.max(axis=1).min(axis=-1)  # render.py:384
    mask = mask.numpy()
    assert np.array_equal(mask, min_t < max_t)
    return ~mask, np.abs(max_t - min_t)


def reduce_miss(image_u8: np.ndarray, miss: np.ndarray, stats: np.ndarray = None) -> np.ndarray:
    """Combine the pixels of image_u8 [H, W, 3] selected by miss [H*W] into the int64 [10] statistics words."""
    out = STATS_INIT.copy() if stats is None else stats.copy()
    sel = image_u8.reshape(-1, 3)[np.asarray(miss, dtype=bool)].astype(np.int64)
    if sel.shape[0]:
        out[0] += sel.shape[0]
        out[1:4] += sel.sum(axis=0)
        out[4:7] = np.minimum(out[4:7], sel.min(axis=0))
        out[7:10] = np.maximum(out[7:10], sel.max(axis=0))
    return out


def colors_of_stats(stats: np.ndarray):
    """-> dict(count, min, max, mean) as scripts/check_bbox.py prints them: float32 colours px / 127.5 - 1; the mean is
    evaluated in float64 and rounded once.  None fields when no ray misses."""
    count = int(stats[0])
    if count == 0:
        return dict(count=0, min=None, max=None, mean=None)
    f32 = np.float32
    low = stats[4:7].astype(f32) / f32(127.5) - f32(1)
    high = stats[7:10].astype(f32) / f32(127.5) - f32(1)
    mean = ((stats[1:4].astype(F64) / count) / 127.5 - 1).astype(f32)
    return dict(count=count, min=low, max=high, mean=mean)


def bbox_stats_reference(dataset, bbox_min=None, bbox_max=None):
    """The statistics of a whole dataset (views with image() and camera fields) on the CPU."""
    lo = dataset.metadata.bbox_min if bbox_min is None else bbox_min
    hi = dataset.metadata.bbox_max if bbox_max is None else bbox_max
    stats = STATS_INIT.copy()
    for view in dataset.views:
        image = np.asarray(view.image())
        miss, _ = miss_reference(view, image.shape[1], image.shape[0], lo, hi)
        stats = reduce_miss(image, miss, stats)
    return colors_of_stats(stats)


def look_at(origin, target, x_fov: float, y_fov: float, cls=None, **kwargs):
    """A CameraView (or `cls`) at `origin` looking at `target`, y pointing down the image like the dataset tools."""
    origin, target = np.asarray(origin, F64), np.asarray(target, F64)
    z = (target - origin) / np.linalg.norm(target - origin)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.95 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return (cls or CameraView)(camera_direction=tuple(z.tolist()), camera_origin=tuple(origin.tolist()),
                               x_axis=tuple(x.tolist()), y_axis=tuple(y.tolist()), x_fov=float(x_fov),
                               y_fov=float(y_fov), **kwargs)


def camera_around(seed: int, radius: float = 2.5, fov: float = 0.9, jitter: float = 0.4, cls=None, **kwargs):
    """A seeded camera on the sphere of `radius` that looks near the origin: part of its rays hit a box there."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=3)
    return look_at(radius * v / np.linalg.norm(v), rng.uniform(-jitter, jitter, size=3), fov, fov * rng.uniform(0.7, 1.0),
                   cls=cls, **kwargs)


@dataclass
class ArrayView(NeRFView):
    """A view whose image is an array in memory (uint8 [H, W, 3])."""

    pixels: np.ndarray = None
    image_path: str = ""

    def image(self) -> np.ndarray:
        return self.pixels

"""
NumPy restatement of the point-cloud export (learn_nerf/point_cloud.py, csrc/pointcloud.hip): back-projection in
float64, brute-force k-th squared distance and nearest index in float32 with the pinned formula of the kernels' header
comment, the distance field and its grid geometry, tiny PLY / OBJ readers, and a generator of a synthetic RGB-D dataset
with a known surface (a sphere of radius 0.5 seen by 60-degree pinhole cameras on a sphere of radius 2).
"""
import json
import math
import os

import numpy as np

F32 = np.float32
NO_DEPTH = 0xFFFF
SPHERE_RADIUS = 0.5
CAMERA_RADIUS = 2.0
FOV = 60.0 * math.pi / 180
# dot(dir, z) at the corner pixel of a 60 x 60 degree view: 1 / sqrt(1 + 2 tan^2 30) = 0.7746
CORNER_COSINE = 1.0 / math.sqrt(1.0 + 2.0 * math.tan(FOV / 2) ** 2)


# ---- pinned float32 distances -----------------------------------------------------------------------------------
def dist2(queries, points) -> np.ndarray:
    """[m, n] float32: dx = q.x - p.x ..., d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded once."""
    q = np.asarray(queries, dtype=F32)[:, None, :]
    p = np.asarray(points, dtype=F32)[None, :, :]
    d = q - p
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def knn_dist2(points, queries, k: int, chunk: int = 512) -> np.ndarray:
    """float32 [m]: squared distance to the k-th nearest point (a query that is a point counts itself), +inf when
    there are fewer than k points."""
    points = np.asarray(points, dtype=F32)
    queries = np.asarray(queries, dtype=F32)
    out = np.full(len(queries), np.inf, dtype=F32)
    if len(points) < k:
        return out
    for s in range(0, len(queries), chunk):
        d = dist2(queries[s:s + chunk], points)
        out[s:s + chunk] = np.partition(d, k - 1, axis=1)[:, k - 1]
    return out


def nearest(points, queries, max_radius=np.inf, chunk: int = 512):
    """(d2 float32 [m], index int32 [m]): the nearest point with d2 <= max_radius^2 (one float32 multiply), the lowest
    index among equal d2; (+inf, -1) without one."""
    points = np.asarray(points, dtype=F32)
    queries = np.asarray(queries, dtype=F32)
    r2 = F32(max_radius) * F32(max_radius)
    d2 = np.full(len(queries), np.inf, dtype=F32)
    idx = np.full(len(queries), -1, dtype=np.int32)
    if len(points) == 0:
        return d2, idx
    for s in range(0, len(queries), chunk):
        d = dist2(queries[s:s + chunk], points)
        best = d.argmin(axis=1)  # the first, i.e. lowest, index of the minimum
        val = d[np.arange(len(best)), best]
        found = val <= r2
        d2[s:s + chunk] = np.where(found, val, F32(np.inf))
        idx[s:s + chunk] = np.where(found, best, -1)
    return d2, idx


# ---- the field ----------------------------------------------------------------------------------------------------
def field_axes(points, thickness: float, delta: float):
    """Per axis the float64 coordinates lo_a - pad + i * delta, i < ceil((hi_a - lo_a + 2 pad) / delta) + 1."""
    points = np.asarray(points, dtype=F32)
    pad = float(thickness) + float(delta)
    axes = []
    for a in range(3):
        lo, hi = float(points[:, a].min()), float(points[:, a].max())
        count = int(math.ceil((hi - lo + 2 * pad) / float(delta))) + 1
        axes.append(lo - pad + np.arange(count, dtype=np.float64) * float(delta))
    return axes


def point_field(points, thickness: float, delta: float) -> np.ndarray:
    """float32 [nx, ny, nz]: thickness - sqrt(d2 of the nearest point) in float32 at the float32-rounded grid points,
    thickness - max_radius where nothing lies within max_radius = float32(thickness + delta)."""
    axes = [a.astype(F32) for a in field_axes(points, thickness, delta)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    max_radius = F32(float(thickness) + float(delta))
    d2, idx = nearest(points, grid, max_radius)
    with np.errstate(invalid="ignore"):
        value = F32(thickness) - np.sqrt(d2, dtype=F32)
    value = np.where(idx >= 0, value, F32(thickness) - max_radius).astype(F32)
    return value.reshape([len(a) for a in axes])


# ---- back-projection ----------------------------------------------------------------------------------------------
def pixel_directions(view: dict, width: int, height: int) -> np.ndarray:
    """float64 [H*W, 3]: unit direction of every pixel in raster order (x fraction 2 col / (W - 1) - 1, likewise y)."""
    x = np.asarray(view["x"], np.float64) * math.tan(view["x_fov"] / 2)
    y = np.asarray(view["y"], np.float64) * math.tan(view["y_fov"] / 2)
    z = np.asarray(view["z"], np.float64)
    u = np.linspace(-1, 1, width)[None, :, None]
    v = np.linspace(-1, 1, height)[:, None, None]
    d = (z + u * x + v * y).reshape(-1, 3)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def back_project(view: dict, depth: np.ndarray, color: np.ndarray, max_depth: float):
    """point_cloud/main.go:76-84 in float64: (points [n, 3], colours [n, 3] in [0, 1]) of the pixels with depth !=
    0xffff, raster order."""
    height, width = depth.shape
    d = pixel_directions(view, width, height)
    keep = depth.reshape(-1) != NO_DEPTH
    z = depth.reshape(-1)[keep].astype(np.float64) / 65535 * max_depth
    d = d[keep]
    scale = z / (d @ np.asarray(view["z"], np.float64))
    points = np.asarray(view["origin"], np.float64) + d * scale[:, None]
    return points, color.reshape(-1, 3)[keep].astype(np.float64) / 255


# ---- the synthetic dataset ----------------------------------------------------------------------------------------
def sphere_view(direction) -> dict:
    """Camera on the sphere of radius 2 looking at the origin along `direction` (render_new_dataset.py's frame)."""
    z = np.asarray(direction, np.float64)
    z = z / np.linalg.norm(z)
    x = np.array([z[1], -z[0], 0.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = x - z * (x @ z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    return dict(origin=(-z * CAMERA_RADIUS).tolist(), x=x.tolist(), y=y.tolist(), z=z.tolist(), x_fov=FOV, y_fov=FOV)


def surface_color(points) -> np.ndarray:
    """uint8 colour as a function of position on the sphere."""
    return np.clip((np.asarray(points, np.float64) / SPHERE_RADIUS * 0.5 + 0.5) * 255, 0, 255).astype(np.uint8)


def render_sphere(view: dict, size: int, max_depth: float):
    """Analytic float64 z-depth of the sphere truncated to 16 bits as render_new_dataset.py does ((z / max_depth *
    0xffff).astype(uint32)); misses are 0xffff.  -> (depth uint32 [size, size], colour uint8 [size, size, 3])."""
    d = pixel_directions(view, size, size)
    o = np.asarray(view["origin"], np.float64)
    b = d @ o
    disc = b * b - (o @ o - SPHERE_RADIUS ** 2)
    hit = disc > 0
    t = -b - np.sqrt(np.where(hit, disc, 0.0))
    z = t * (d @ np.asarray(view["z"], np.float64))
    depth = np.where(hit, (np.clip(z / max_depth, 0, 1) * 0xFFFF).astype(np.uint32), NO_DEPTH).astype(np.uint32)
    color = np.where(hit[:, None], surface_color(o + d * t[:, None]), 0).astype(np.uint8)
    return depth.reshape(size, size), color.reshape(size, size, 3)


SPHERE_DIRECTIONS = ((0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 1, 1), (-1, -1, -1))


def write_sphere_dataset(path: str, size: int = 48, max_depth: float = 4.0, directions=SPHERE_DIRECTIONS,
                         all_missing: bool = False):
    """Writes NNNNN.json / NNNNN.png / NNNNN_depth.png with PIL; -> [(view, depth, colour)] as written."""
    from PIL import Image

    os.makedirs(path, exist_ok=True)
    views = []
    for i, direction in enumerate(directions):
        view = sphere_view(direction)
        depth, color = render_sphere(view, size, max_depth)
        if all_missing:
            depth[:] = NO_DEPTH
        stem = os.path.join(path, f"{i:05d}")
        with open(stem + ".json", "w") as fh:
            json.dump(view, fh)
        Image.fromarray(color).save(stem + ".png")
        Image.fromarray(depth.astype(np.uint16)).save(stem + "_depth.png")  # a 16-bit greyscale PNG
        views.append((view, depth, color))
    return views


# ---- tiny readers for the writers' round trips -------------------------------------------------------------------
def read_colored_obj(path: str):
    verts, faces = [], []
    for line in open(path).read().splitlines():
        parts = line.split()
        if parts[0] == "v":
            verts.append([float(x) for x in parts[1:]])
        elif parts[0] == "f":
            faces.append([int(x) - 1 for x in parts[1:]])
    verts = np.array(verts, np.float64).reshape(-1, 6)
    return verts[:, :3], verts[:, 3:], np.array(faces, np.int32).reshape(-1, 3)


def read_ply(path: str):
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    header = blob[:end].decode("ascii").splitlines()
    assert header[:2] == ["ply", "format binary_little_endian 1.0"]
    counts = {line.split()[1]: int(line.split()[2]) for line in header if line.startswith("element")}
    nv, nf = counts["vertex"], counts.get("face", 0)
    vrec = np.frombuffer(blob, dtype=[("xyz", "<f4", (3,)), ("rgb", "u1", (3,))], count=nv, offset=end)
    frec = np.frombuffer(blob, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nf, offset=end + nv * 15)
    assert end + nv * 15 + nf * 13 == len(blob) and (frec["n"] == 3).all()
    return vrec["xyz"].copy(), vrec["rgb"].copy(), frec["idx"].copy()

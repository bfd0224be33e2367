"""
STL dataset producer (the reference's Go command simple_dataset/): an .stl is read, normalised, and ray-cast from random
or rotating cameras under random point lights into the on-disk dataset format of learn_nerf.dataset.  The ray casting
(first hit and any hit against the triangles) is csrc/raycast.hip, whose header fixes the ray-triangle test, the tie
rule, the margin of the box test and the input domain; TriangleMesh wraps it.  model3d, which supplies the Go tool's
shading and camera fitting, is not vendored in the reference, so the conventions it would pin are fixed here:

  rays      CameraView.bare_rays(width, height, device): the loader's own pixel grid.
  shading   float64, one torch call per operation, for the pixels that hit (origin o, direction d, parameter t, hit
            triangle v0 v1 v2, all converted from fp32):
              P = o + t * d;  n = (v1 - v0) x (v2 - v0), components a.y*b.z - a.z*b.y and cyclic;
              len = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z);  N = n / len (0 where len is 0), negated where
              (N.x*d.x + N.y*d.y) + N.z*d.z > 0, so it faces the viewer;
              per light (position L, brightness b) in order: w = L - P, l = w / sqrt((w.x*w.x + w.y*w.y) + w.z*w.z),
              shadow ray from fp32(P + 1e-4 * N) along fp32(l) with t in (0, inf),
              total += (b * max(0, (N.x*l.x + N.y*l.y) + N.z*l.z)) * (1 - occluded);
              byte = rint(255 * min(max(color * total, 0), 1)), alpha 255; a miss is 0, 0, 0, 0.
  cameras   a unit direction v from the box centre c; origin c + dist * v, z = -v, up = +z unless |z.z| >= 0.95 (then
            +y), x = z x up normalised, y = z x x (down the image), as scripts/make_cube_dataset.random_camera.  dist is
            the smallest at which all eight corners of the box project into the central 90 % of the image.
"""
import ctypes
import math
import struct
from typing import Optional, Tuple

import numpy as np
import torch

from learn_nerf import _lib as L
from learn_nerf.dataset import CameraView

F32 = torch.float32
MAX_COORD = 2.0 ** 20  # the domain of the margin argument in csrc/raycast.hip
MIN_EXTENT = 2.0 ** -20
UNIT_TOL = 2.0 ** -9
MAX_TRIS = 2 ** 28
DEFAULT_LEAF = 4
SHADOW_OFFSET = 1e-4
LIGHT_DISTANCE = 1000.0  # simple_dataset/main.go:164
IMAGE_MARGIN = 0.05


# ------------------------------------------------------------------ STL ----

def read_stl(path: str) -> np.ndarray:
    """Triangles [n, 3, 3] float32 of a binary or ASCII STL; stored normals are ignored.  ValueError with a message for
    a truncated file, a triangle count that disagrees with the file size, zero triangles and non-finite vertices."""
    with open(path, "rb") as handle:
        data = handle.read()
    head = data[:512].lstrip()
    if head.startswith(b"solid") and (len(data) < 84 or b"facet" in data[:4096] or b"endsolid" in data[:4096]):
        tris = _parse_ascii_stl(path, data)
    else:
        if len(data) < 84:
            raise ValueError(f"{path}: truncated STL: {len(data)} bytes, a binary STL has a header of 84")
        (count,) = struct.unpack_from("<I", data, 80)
        if 84 + 50 * count != len(data):
            raise ValueError(f"{path}: the STL header counts {count} triangles ({84 + 50 * count} bytes), the file has "
                             f"{len(data)} bytes")
        rec = np.frombuffer(data, dtype=[("normal", "<f4", (3,)), ("verts", "<f4", (3, 3)), ("attr", "<u2")], offset=84)
        tris = rec["verts"].astype(np.float32)
    if len(tris) == 0:
        raise ValueError(f"{path}: the STL holds no triangles")
    if not np.isfinite(tris).all():
        raise ValueError(f"{path}: the STL holds non-finite vertices")
    return np.ascontiguousarray(tris)


def _parse_ascii_stl(path: str, data: bytes) -> np.ndarray:
    try:
        tokens = data.decode("ascii").split()
    except UnicodeDecodeError:
        raise ValueError(f"{path}: malformed ASCII STL: not ASCII text") from None
    if "endsolid" not in tokens:
        raise ValueError(f"{path}: truncated STL: the ASCII file has no 'endsolid'")
    coords = []
    try:
        for i, token in enumerate(tokens):
            if token == "vertex":
                coords.append([float(tokens[i + 1]), float(tokens[i + 2]), float(tokens[i + 3])])
    except (IndexError, ValueError):
        raise ValueError(f"{path}: malformed ASCII STL: a 'vertex' without three numbers") from None
    if len(coords) % 3 != 0 or tokens.count("facet") != len(coords) // 3:
        raise ValueError(f"{path}: malformed ASCII STL: {len(coords)} vertices in {tokens.count('facet')} facets")
    return np.asarray(coords, dtype=np.float64).reshape(-1, 3, 3).astype(np.float32)


def normalize(tris) -> np.ndarray:
    """normalizeMesh of simple_dataset/main.go:139-144: the box is centred on 0 and scaled by 1 / (its largest
    coordinate), in float64, rounded to float32 once."""
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    lo, hi = t.min(axis=(0, 1)), t.max(axis=(0, 1))
    t = t - (lo + hi) / 2
    size = t.max()
    if not size > 0:
        raise ValueError("the mesh has zero extent")
    return (t * (1 / size)).astype(np.float32)


# -------------------------------------------------------------- cameras ----

def camera_frame(direction) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(x, y, z) of a camera that sits in `direction` from what it looks at."""
    v = np.asarray(direction, dtype=np.float64)
    z = -v / np.linalg.norm(v)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.95 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return x, y, z


def fit_distance(lo, hi, direction, fov: float, margin: float = IMAGE_MARGIN) -> float:
    """The smallest distance from the box centre, along `direction`, at which every corner of [lo, hi] projects at
    least `margin` of the image inside each border: |r.x| <= (1 - 2 margin) tan(fov / 2) (dist + r.z) for the corner
    offsets r, and the same for y."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    x, y, z = camera_frame(direction)
    half = (hi - lo) / 2
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    r = signs * half
    scale = (1 - 2 * margin) * math.tan(fov / 2)
    return float(max((np.abs(r @ x) / scale - r @ z).max(), (np.abs(r @ y) / scale - r @ z).max()))


def camera_at(lo, hi, direction, dist: float, fov: float) -> CameraView:
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.asarray(direction, dtype=np.float64)
    v = v / np.linalg.norm(v)
    x, y, _ = camera_frame(v)
    z = np.cross(x, y)  # as camera_json writes it, so that the file reads back as this very view
    z /= np.linalg.norm(z)
    origin = (lo + hi) / 2 + dist * v
    return CameraView(camera_direction=tuple(z.tolist()), camera_origin=tuple(origin.tolist()), x_axis=tuple(x.tolist()),
                      y_axis=tuple(y.tolist()), x_fov=fov, y_fov=fov)


def random_unit(rs: np.random.RandomState) -> np.ndarray:
    v = rs.normal(size=3)
    return v / np.linalg.norm(v)


def random_lights(rs: np.random.RandomState, lo, hi, count: int, brightness: float) -> np.ndarray:
    """[count, 4] float64 (position, brightness): random directions at LIGHT_DISTANCE from the box centre
    (simple_dataset/main.go:158-169)."""
    center = (np.asarray(lo, dtype=np.float64) + np.asarray(hi, dtype=np.float64)) / 2
    lights = np.empty((count, 4), dtype=np.float64)
    for i in range(count):
        lights[i, :3] = center + random_unit(rs) * LIGHT_DISTANCE
        lights[i, 3] = brightness
    return lights


def random_camera(rs: np.random.RandomState, lo, hi, fov: float) -> CameraView:
    v = random_unit(rs)
    return camera_at(lo, hi, v, fit_distance(lo, hi, v, fov), fov)


def rotating_directions(axis, offset, total: int) -> np.ndarray:
    """[total, 3]: the unit offset rotated about the unit axis by 2 pi i / total (camera_gen.go:57-61), Rodrigues."""
    k = np.asarray(axis, dtype=np.float64)
    v = np.asarray(offset, dtype=np.float64)
    if not (np.linalg.norm(k) > 0 and np.linalg.norm(v) > 0):
        raise ValueError("the rotation axis and offset must be non-zero")
    k, v = k / np.linalg.norm(k), v / np.linalg.norm(v)
    out = np.empty((total, 3), dtype=np.float64)
    for i in range(total):
        theta = 2 * math.pi * i / total
        out[i] = v * math.cos(theta) + np.cross(k, v) * math.sin(theta) + k * (k @ v) * (1 - math.cos(theta))
    return out


def rotating_cameras(lo, hi, fov: float, axis, offset, total: int):
    """Every frame at the largest fitted distance of the whole path (camera_gen.go:44-55)."""
    directions = rotating_directions(axis, offset, total)
    dist = max(fit_distance(lo, hi, v, fov) for v in directions)
    return [camera_at(lo, hi, v, dist, fov) for v in directions]


def camera_json(view: CameraView) -> dict:
    """origin, x, y, z, x_fov, y_fov with z = x cross y normalised (simple_dataset/main.go:106-113)."""
    x, y = np.asarray(view.x_axis, dtype=np.float64), np.asarray(view.y_axis, dtype=np.float64)
    z = np.cross(x, y)
    z = z / np.linalg.norm(z)
    return dict(origin=list(view.camera_origin), x=x.tolist(), y=y.tolist(), z=z.tolist(), x_fov=view.x_fov,
                y_fov=view.y_fov)


# ------------------------------------------------------------ the tracer ----

class TriangleMesh:
    """
    The triangles [n, 3, 3] (GPU, fp32) in the tree of csrc/raycast.hip, for first-hit and any-hit ray queries, for the
    nearest-triangle query of a point and for area-weighted surface samples (learn_nerf/mesh_metrics.py).  leaf_size
    forces the triangles per leaf; results do not depend on it.  Input outside the domain stated in the kernel file's
    header (non-finite values, coordinates beyond 2^20, a mesh extent outside [2^-20, 2^20], directions that are not
    unit vectors, NaN windows) raises before any launch.
    """

    def __init__(self, tris: torch.Tensor, leaf_size: int = DEFAULT_LEAF):
        if not isinstance(tris, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(tris)}")
        if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
            raise ValueError(f"triangles: expected shape [n, 3, 3], got {tuple(tris.shape)}")
        if not tris.is_cuda:
            raise RuntimeError("triangles: the ray caster needs tensors on a ROCm GPU device (no CPU fallback)")
        n = tris.shape[0]
        if not 1 <= n <= MAX_TRIS:
            raise ValueError(f"{n} triangles: need between 1 and 2^28")
        if not 1 <= int(leaf_size) <= 64:
            raise ValueError(f"leaf_size must lie in [1, 64], got {leaf_size}")
        tris = tris.to(F32).contiguous()
        if not torch.isfinite(tris).all():
            raise ValueError("triangles: non-finite coordinates")
        flat = tris.view(-1, 3)
        lo = np.asarray(flat.min(dim=0).values.tolist(), dtype=np.float64)
        hi = np.asarray(flat.max(dim=0).values.tolist(), dtype=np.float64)
        if max(np.abs(lo).max(), np.abs(hi).max()) > MAX_COORD:
            raise ValueError("triangles: coordinates beyond 2^20 are outside the ray caster's domain")
        extent = float((hi - lo).max())
        if not MIN_EXTENT <= extent <= MAX_COORD:
            raise ValueError(f"triangles: a mesh extent of {extent} is outside the ray caster's domain [2^-20, 2^20]")
        self.n, self.leaf_size, self.lo, self.hi = n, int(leaf_size), lo, hi
        self.tris = tris
        half = (hi - lo) / 2
        radius = np.nextafter(np.float32(half.sum()), np.float32(np.inf))
        self.bvh = L.RtBvh((ctypes.c_float * 3)(*((lo + hi) / 2)), float(radius), (ctypes.c_float * 3)(*half), n,
                           self.leaf_size, 0)
        lib, dev = L.lib(), tris.device
        codes = torch.empty(n, dtype=torch.int32, device=dev)
        L.check(lib.lnrf_rt_morton(ctypes.byref(self.bvh), L.ptr(tris), L.ptr(codes, torch.int32), L.stream()),
                "rt_morton")
        order = torch.sort(codes, stable=True).indices
        self.order = order.to(torch.int32)
        self.sorted_tris = tris[order].contiguous()
        rows = lib.lnrf_rt_node_count(n, self.leaf_size)
        self.nodes = torch.empty((rows, 8), dtype=F32, device=dev)
        L.check(lib.lnrf_rt_fit(ctypes.byref(self.bvh), L.ptr(self.sorted_tris), L.ptr(self.nodes), L.stream()),
                "rt_fit")

    def _check_rays(self, rays: torch.Tensor, t_min, t_max):
        if rays.dim() != 3 or tuple(rays.shape[1:]) != (2, 3):
            raise ValueError(f"rays: expected shape [m, 2, 3] (origin, direction), got {tuple(rays.shape)}")
        if not rays.is_cuda:
            raise RuntimeError("rays: the ray caster needs tensors on a ROCm GPU device (no CPU fallback)")
        rays = rays.to(F32).contiguous()
        m = rays.shape[0]
        window = None
        if m:
            if not torch.isfinite(rays).all():
                raise ValueError("rays: non-finite origins or directions")
            if rays[:, 0].abs().max().item() > MAX_COORD:
                raise ValueError("rays: origins beyond 2^20 are outside the ray caster's domain")
            d = rays[:, 1].double()
            if ((d * d).sum(-1) - 1).abs().max().item() > UNIT_TOL:
                raise ValueError("rays: directions must be unit vectors")
        if not (isinstance(t_min, (int, float)) and t_min == 0 and isinstance(t_max, float) and t_max == math.inf):
            window = torch.empty((m, 2), dtype=F32, device=rays.device)
            window[:, 0] = torch.as_tensor(t_min, dtype=F32, device=rays.device)
            window[:, 1] = torch.as_tensor(t_max, dtype=F32, device=rays.device)
            if torch.isnan(window).any():
                raise ValueError("rays: NaN in t_min or t_max")
        return rays, window

    def closest(self, rays: torch.Tensor, t_min=0.0, t_max=math.inf,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(t fp32 [m], id int32 [m]) of the nearest accepted triangle of each ray of rays [m, 2, 3], the lowest index
        among equal t; (+inf, -1) for a miss.  t_min / t_max: scalars or [m] tensors."""
        rays, window = self._check_rays(rays, t_min, t_max)
        m = rays.shape[0]
        t, idx = out if out is not None else (torch.empty(m, dtype=F32, device=rays.device),
                                              torch.empty(m, dtype=torch.int32, device=rays.device))
        if t.shape != (m,) or idx.shape != (m,):
            raise ValueError("out: expected two tensors of shape [m]")
        L.check(L.lib().lnrf_rt_closest(ctypes.byref(self.bvh), L.ptr(self.sorted_tris), L.ptr(self.order, torch.int32),
                                        L.ptr(self.nodes), L.ptr(rays), L.ptr(window), m, L.ptr(t),
                                        L.ptr(idx, torch.int32), L.stream()), "rt_closest")
        return t, idx

    def occluded(self, rays: torch.Tensor, t_min=0.0, t_max=math.inf,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [m]: 1 iff any triangle is accepted in (t_min, t_max)."""
        rays, window = self._check_rays(rays, t_min, t_max)
        m = rays.shape[0]
        occ = out if out is not None else torch.empty(m, dtype=torch.uint8, device=rays.device)
        if occ.shape != (m,):
            raise ValueError("out: expected a tensor of shape [m]")
        L.check(L.lib().lnrf_rt_occluded(ctypes.byref(self.bvh), L.ptr(self.sorted_tris), L.ptr(self.nodes),
                                         L.ptr(rays), L.ptr(window), m, L.ptr(occ, torch.uint8), L.stream()),
                "rt_occluded")
        return occ

    def _check_points(self, points: torch.Tensor) -> torch.Tensor:
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(points)}")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: expected shape [m, 3], got {tuple(points.shape)}")
        if not points.is_cuda:
            raise RuntimeError("points: the ray caster needs tensors on a ROCm GPU device (no CPU fallback)")
        points = points.to(F32).contiguous()
        if points.shape[0]:
            if not torch.isfinite(points).all():
                raise ValueError("points: non-finite coordinates")
            if points.abs().max().item() > MAX_COORD:
                raise ValueError("points: coordinates beyond 2^20 are outside the ray caster's domain")
        return points

    def nearest(self, points: torch.Tensor,
                out: Optional[Tuple[torch.Tensor, ...]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(d2 fp32 [m], id int32 [m]) of the triangle nearest to each point of points [m, 3]: the pinned fp32
        point-triangle distance of csrc/raycast.hip ("Nearest triangle"), squared, the lowest index among equal d2.
        out: (d2, id) or (d2, id, closest fp32 [m, 3]); with the third tensor the closest point of that triangle is
        written too, and the three are returned."""
        points = self._check_points(points)
        m = points.shape[0]
        if out is None:
            out = (torch.empty(m, dtype=F32, device=points.device),
                   torch.empty(m, dtype=torch.int32, device=points.device))
        if len(out) not in (2, 3) or out[0].shape != (m,) or out[1].shape != (m,):
            raise ValueError("out: expected two tensors of shape [m], and optionally one of shape [m, 3]")
        closest = out[2] if len(out) == 3 else None
        if closest is not None and tuple(closest.shape) != (m, 3):
            raise ValueError("out: expected two tensors of shape [m], and optionally one of shape [m, 3]")
        L.check(L.lib().lnrf_mesh_nearest(ctypes.byref(self.bvh), L.ptr(self.sorted_tris),
                                          L.ptr(self.order, torch.int32), L.ptr(self.nodes), L.ptr(points), m,
                                          L.ptr(out[0]), L.ptr(out[1], torch.int32), L.ptr(closest), L.stream()),
                "mesh_nearest")
        return tuple(out)

    def tri_areas(self) -> torch.Tensor:
        """fp32 [n]: the pinned area of every triangle, in the original order."""
        areas = torch.empty(self.n, dtype=F32, device=self.tris.device)
        L.check(L.lib().lnrf_mesh_tri_areas(L.ptr(self.tris), self.n, L.ptr(areas), L.stream()), "mesh_tri_areas")
        return areas

    def surface_cdf(self) -> np.ndarray:
        """float64 [n] (host): the running sum of the pinned areas over the SORTED triangles, added one by one in
        float64, so that it is the same array on every device."""
        areas = torch.empty(self.n, dtype=F32, device=self.tris.device)
        L.check(L.lib().lnrf_mesh_tri_areas(L.ptr(self.sorted_tris), self.n, L.ptr(areas), L.stream()),
                "mesh_tri_areas")
        return np.cumsum(areas.cpu().numpy().astype(np.float64))

    def sample_surface(self, count: int, seed: int, stream_id: int = 0,
                       cdf: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(points fp32 [count, 3], id int32 [count]): stratified samples of the surface in proportion to area, and the
        original index of each sample's triangle (csrc/mesh_metrics.hip fixes every bit given the cdf).  Sample i draws
        elements 3i, 3i + 1, 3i + 2 of Philox stream `stream_id` under `seed`.  Samples follow the tree's sorted order
        of the triangles, so neighbours in the array are neighbours in space.  cdf: a device float64 [n] running sum
        of areas over self.sorted_tris to use in place of surface_cdf()."""
        count = int(count)
        if count < 0:
            raise ValueError(f"count must not be negative, got {count}")
        dev = self.tris.device
        if cdf is None:
            cdf = torch.from_numpy(self.surface_cdf()).to(dev)
        if not cdf.is_cuda:
            raise RuntimeError("cdf: the ray caster needs tensors on a ROCm GPU device (no CPU fallback)")
        if cdf.dtype != torch.float64 or tuple(cdf.shape) != (self.n,):
            raise ValueError(f"cdf: expected float64 of shape [{self.n}]")
        cdf = cdf.contiguous()
        total = float(cdf[-1].item())
        if not (total > 0 and math.isfinite(total)):
            raise ValueError("the mesh has zero total area: nothing to sample")
        if self.n > 1 and bool((cdf[1:] < cdf[:-1]).any().item()):
            raise ValueError("cdf: must be non-decreasing")
        pts = torch.empty((count, 3), dtype=F32, device=dev)
        ids = torch.empty(count, dtype=torch.int32, device=dev)
        L.check(L.lib().lnrf_mesh_sample_surface(L.ptr(self.sorted_tris), L.ptr(self.order, torch.int32),
                                                 L.ptr(cdf, torch.float64), self.n, count,
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF,
                                                 L.ptr(pts), L.ptr(ids, torch.int32), L.stream()),
                "mesh_sample_surface")
        return pts, ids

    def shade(self, rays: torch.Tensor, t: torch.Tensor, idx: torch.Tensor, lights, color) -> torch.Tensor:
        """uint8 [m, 4]: the RGBA of the module docstring for the rays and their closest() result."""
        dev = rays.device
        rgba = torch.zeros((rays.shape[0], 4), dtype=torch.uint8, device=dev)
        hit = torch.nonzero(idx >= 0).view(-1)
        if hit.numel() == 0:
            return rgba
        lights = np.asarray(lights, dtype=np.float64).reshape(-1, 4)
        o, d = rays[hit, 0].double(), rays[hit, 1].double()
        tt = t[hit].double()
        v = self.tris[idx[hit].long()].double()
        P = [o[:, a] + tt * d[:, a] for a in range(3)]
        e1 = [v[:, 1, a] - v[:, 0, a] for a in range(3)]
        e2 = [v[:, 2, a] - v[:, 0, a] for a in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        length = torch.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        zero = torch.zeros_like(length)
        N = [torch.where(length > 0, c / length, zero) for c in n]
        away = ((N[0] * d[:, 0] + N[1] * d[:, 1]) + N[2] * d[:, 2]) > 0
        N = [torch.where(away, -c, c) for c in N]
        start = torch.stack([P[a] + SHADOW_OFFSET * N[a] for a in range(3)], dim=1).to(F32)
        total = torch.zeros_like(length)
        for lx, ly, lz, brightness in lights.tolist():
            w = [lx - P[0], ly - P[1], lz - P[2]]
            dist = torch.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
            l = [c / dist for c in w]
            shadow = torch.stack([start, torch.stack(l, dim=1).to(F32)], dim=1).contiguous()
            lit = 1 - self.occluded(shadow).double()
            diffuse = torch.clamp((N[0] * l[0] + N[1] * l[1]) + N[2] * l[2], min=0)
            total = total + (brightness * diffuse) * lit
        for a, base in enumerate(float(c) for c in color):
            rgba[hit, a] = torch.round(255 * torch.clamp(base * total, min=0, max=1)).to(torch.uint8)
        rgba[hit, 3] = 255
        return rgba

    def render(self, view: CameraView, width: int, height: int, lights, color) -> torch.Tensor:
        """uint8 [height, width, 4] (GPU): the view ray-cast under `lights` [k, 4] (position, brightness) with the base
        `color` (r, g, b in [0, 1])."""
        rays = view.bare_rays(width, height, device=self.tris.device)
        t, idx = self.closest(rays)
        return self.shade(rays, t, idx, lights, color).view(height, width, 4)

"""
NumPy restatement of the STL dataset producer's conventions (csrc/raycast.hip, learn_nerf/raycast.py), for the tests:
the pinned fp32 ray-triangle test as a brute force over every (ray, triangle) pair with the tie rule, the float64
shading, the camera fit by bisection, and mesh builders.  Nothing here imports the package.
"""
import math

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------- meshes ----

def cube(half=0.5, center=(0.0, 0.0, 0.0)):
    """12 triangles [12, 3, 3] float32 of the axis-aligned cube, outward."""
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * half + center
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [f for a, b, cc, d in quads for f in ((a, b, cc), (a, cc, d))]
    return c[np.array(faces)].astype(F32)


def icosphere(subdivisions, radius=1.0):
    """20 * 4^subdivisions triangles of the subdivided icosahedron, vertices on the sphere (float32)."""
    p = (1 + math.sqrt(5)) / 2
    verts = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
             (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
             (8, 6, 7), (9, 8, 1)]
    tris = np.array(verts, dtype=np.float64)[np.array(faces)]
    for _ in range(subdivisions):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        tris = np.concatenate([np.stack(t, axis=1) for t in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    tris = tris / np.linalg.norm(tris, axis=-1, keepdims=True) * radius
    return tris.astype(F32)


def soup(n, seed=0, size=0.05):
    """n random triangles of edge about `size` with their first vertex in [-1, 1]^3."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, size=(n, 1, 3))
    return (base + rng.uniform(-size, size, size=(n, 3, 3))).astype(F32)


# ----------------------------------------------------------- brute force ----

def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def pair_test(tris, rays, t_min, t_max):
    """(accepted bool [m, n], t float32 [m, n]) of the pinned test, every operation one float32 rounding."""
    tris = np.asarray(tris, dtype=F32)
    rays = np.asarray(rays, dtype=F32)
    m = rays.shape[0]
    t_min = np.broadcast_to(np.asarray(t_min, dtype=F32), (m,))[:, None]
    t_max = np.broadcast_to(np.asarray(t_max, dtype=F32), (m,))[:, None]
    o = [rays[:, 0, a][:, None] for a in range(3)]
    d = [rays[:, 1, a][:, None] for a in range(3)]
    v0 = [tris[:, 0, a][None, :] for a in range(3)]
    e1 = [tris[:, 1, a][None, :] - v0[a] for a in range(3)]
    e2 = [tris[:, 2, a][None, :] - v0[a] for a in range(3)]
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        det = _dot(e1, p)
        inv = F32(1) / det
        s = [o[a] - v0[a] for a in range(3)]
        u = _dot(s, p) * inv
        q = _cross(s, e1)
        v = _dot(d, q) * inv
        t = _dot(e2, q) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_min) & (t < t_max)
    assert t.dtype == F32
    return ok, t


def brute_force(tris, rays, t_min=0.0, t_max=np.inf, chunk=256):
    """-> (t float32 [m], id int32 [m], occluded uint8 [m]): the smallest accepted t and the lowest triangle index
    among equal t (+inf, -1 for a miss), and whether anything is accepted."""
    rays = np.asarray(rays, dtype=F32)
    m = rays.shape[0]
    t_min = np.broadcast_to(np.asarray(t_min, dtype=F32), (m,))
    t_max = np.broadcast_to(np.asarray(t_max, dtype=F32), (m,))
    out_t = np.full(m, np.inf, dtype=F32)
    out_id = np.full(m, -1, dtype=np.int32)
    occ = np.zeros(m, dtype=np.uint8)
    for start in range(0, m, chunk):
        sl = slice(start, start + chunk)
        ok, t = pair_test(tris, rays[sl], t_min[sl], t_max[sl])
        t = np.where(ok, t, F32(np.inf))
        best = t.argmin(axis=1)  # the first of equal minima: the lowest index
        any_hit = ok.any(axis=1)
        out_t[sl] = np.where(any_hit, t[np.arange(len(best)), best], F32(np.inf))
        out_id[sl] = np.where(any_hit, best, -1)
        occ[sl] = any_hit
    return out_t, out_id, occ


# --------------------------------------------------------------- shading ----

def shade(tris, rays, t, idx, lights, color, occluded=None):
    """uint8 [m, 4] of the shading pinned in learn_nerf/raycast.py, float64.  occluded(shadow_rays) -> uint8 [k]
    defaults to the brute force."""
    tris = np.asarray(tris, dtype=F32)
    rays = np.asarray(rays, dtype=F32)
    if occluded is None:
        occluded = lambda shadow: brute_force(tris, shadow)[2]  # noqa: E731
    rgba = np.zeros((rays.shape[0], 4), dtype=np.uint8)
    hit = np.nonzero(np.asarray(idx) >= 0)[0]
    if len(hit) == 0:
        return rgba
    o, d = rays[hit, 0].astype(np.float64), rays[hit, 1].astype(np.float64)
    tt = np.asarray(t)[hit].astype(np.float64)
    v = tris[np.asarray(idx)[hit]].astype(np.float64)
    P = [o[:, a] + tt * d[:, a] for a in range(3)]
    n = _cross([v[:, 1, a] - v[:, 0, a] for a in range(3)], [v[:, 2, a] - v[:, 0, a] for a in range(3)])
    length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    with np.errstate(all="ignore"):
        N = [np.where(length > 0, c / length, 0.0) for c in n]
    away = ((N[0] * d[:, 0] + N[1] * d[:, 1]) + N[2] * d[:, 2]) > 0
    N = [np.where(away, -c, c) for c in N]
    start = np.stack([P[a] + 1e-4 * N[a] for a in range(3)], axis=1).astype(F32)
    total = np.zeros_like(length)
    for lx, ly, lz, brightness in np.asarray(lights, dtype=np.float64).reshape(-1, 4).tolist():
        w = [lx - P[0], ly - P[1], lz - P[2]]
        dist = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        l = [c / dist for c in w]
        shadow = np.stack([start, np.stack(l, axis=1).astype(F32)], axis=1)
        lit = 1 - occluded(shadow).astype(np.float64)
        diffuse = np.maximum((N[0] * l[0] + N[1] * l[1]) + N[2] * l[2], 0)
        total = total + (brightness * diffuse) * lit
    for a in range(3):
        rgba[hit, a] = np.rint(255 * np.clip(float(color[a]) * total, 0, 1)).astype(np.uint8)
    rgba[hit, 3] = 255
    return rgba


def shadowed(tris, rays, t, idx, lights):
    """bool [m]: pixels that hit and whose shadow ray toward at least one light is occluded (for test coverage)."""
    calls = []
    shade(tris, rays, t, idx, lights, (1, 1, 1), lambda s: calls.append(brute_force(tris, s)[2]) or calls[-1])
    out = np.zeros(len(rays), dtype=bool)
    out[np.nonzero(np.asarray(idx) >= 0)[0]] = np.any(calls, axis=0)
    return out


# --------------------------------------------------------------- cameras ----

def project(view, points):
    """Image coordinates in [0, 1]^2 (column, row) of world points under a CameraView-like object: the inverse of the
    pixel grid of CameraView.bare_rays."""
    origin = np.asarray(view.camera_origin, dtype=np.float64)
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (view.x_axis, view.y_axis, view.camera_direction))
    rel = np.asarray(points, dtype=np.float64) - origin
    depth = rel @ z
    assert (depth > 0).all()
    u = (rel @ x) / (depth * math.tan(view.x_fov / 2))
    v = (rel @ y) / (depth * math.tan(view.y_fov / 2))
    return np.stack([(u + 1) / 2, (v + 1) / 2], axis=1)


def box_corners(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])


def fit_distance_bisect(lo, hi, make_view, margin=0.05):
    """The smallest distance at which every box corner projects inside [margin, 1 - margin]^2, by bisection over
    make_view(dist) -> view (inside is monotone in the distance)."""
    corners = box_corners(lo, hi)

    def inside(dist):
        view = make_view(dist)
        rel = corners - np.asarray(view.camera_origin)
        if ((rel @ np.asarray(view.camera_direction)) <= 0).any():
            return False
        uv = project(view, corners)
        return bool((uv >= margin).all() and (uv <= 1 - margin).all())

    far = 1.0
    while not inside(far):
        far *= 2
    near = 0.0
    for _ in range(100):
        mid = (near + far) / 2
        near, far = (near, mid) if inside(mid) else (mid, far)
    return far

"""
NumPy restatement of the TSDF fusion (csrc/tsdf_geom.h, csrc/tsdf.hip, learn_nerf/tsdf.py): the per-voxel, per-view update
with the operation order of the header's convention block, in float32 (bit for bit what the kernels compute) and in
float64 (with a per-voxel margin to every decision the arithmetic takes), the volume and vertex-colour rules, and an
analytic RGB-D scene: a sphere of radius 0.6 in the box [-1, 1]^3 seen by pinhole cameras on a sphere of radius 4.
"""
import json
import math
import os

import numpy as np

NO_DEPTH = 0xFFFF
SPHERE_RADIUS = 0.6
CAMERA_RADIUS = 4.0
FOV = 0.6
BBOX_MIN, BBOX_MAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)

_PHI = (1 + math.sqrt(5)) / 2
# the 12 vertices of an icosahedron: an even cover of the sphere
ICOSAHEDRON = tuple((0.0, s1 * 1.0, s2 * _PHI)[r:] + (0.0, s1 * 1.0, s2 * _PHI)[:r]
                    for r in range(3) for s1 in (1, -1) for s2 in (1, -1))
AXES6 = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


# ---- cameras and the analytic scene -------------------------------------------------------------------------------
def look_at_camera(direction, radius=CAMERA_RADIUS, x_fov=FOV, y_fov=FOV, skew=0.0, origin=None):
    """A learn_nerf.dataset.CameraView at -direction * radius looking at the centre (or at `origin`, looking along
    direction).  skew != 0 adds skew * y_axis to x_axis and stretches y_axis: deliberately non-orthonormal axes."""
    from learn_nerf.dataset import CameraView

    z = np.asarray(direction, np.float64)
    z = z / np.linalg.norm(z)
    x = np.array([z[1], -z[0], 0.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = x - z * (x @ z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    if skew:
        x, y = x + skew * y, y * (1 + skew)
    o = -z * radius if origin is None else np.asarray(origin, np.float64)
    return CameraView(camera_direction=tuple(z.tolist()), camera_origin=tuple(o.tolist()), x_axis=tuple(x.tolist()),
                      y_axis=tuple(y.tolist()), x_fov=float(x_fov), y_fov=float(y_fov))


def pixel_rays(cam, width, height):
    """float64 [H*W, 3]: the (unnormalised) ray z + tan(x_fov/2) u x + tan(y_fov/2) v y of every pixel, raster order,
    u and v = linspace(-1, 1, .): its component along camera_direction is what z-depth measures."""
    x = np.asarray(cam.x_axis, np.float64) * math.tan(cam.x_fov / 2)
    y = np.asarray(cam.y_axis, np.float64) * math.tan(cam.y_fov / 2)
    z = np.asarray(cam.camera_direction, np.float64)
    u = np.linspace(-1, 1, width)[None, :, None]
    v = np.linspace(-1, 1, height)[:, None, None]
    return (z + u * x + v * y).reshape(-1, 3)


def analytic_color(points):
    """float64 [n, 3] in [0, 1]: normal * 0.5 + 0.5 of the sphere at (the direction of) `points`."""
    p = np.asarray(points, np.float64)
    return p / np.linalg.norm(p, axis=1, keepdims=True) * 0.5 + 0.5


FLOATER = ((0.7, 0.7, 0.7), 0.12)  # a small second sphere (centre, radius) in a corner of the box


def render_sphere(cam, width, height, max_depth, floater=None):
    """-> (depth uint16 [H, W]: floor(z / max_depth * 65535) with z the hit's distance along camera_direction, 0xFFFF
    for a miss; colour uint8 [H, W, 3]: rint(255 * analytic colour), 0 for a miss).  floater: a second sphere (centre,
    radius), coloured by its own normal; the nearer hit wins."""
    d = pixel_rays(cam, width, height)
    origin = np.asarray(cam.camera_origin, np.float64)
    a = (d * d).sum(1)
    best = np.full(len(d), np.inf)
    normal = np.zeros_like(d)
    for centre, radius in [((0.0, 0.0, 0.0), SPHERE_RADIUS)] + ([floater] if floater else []):
        o = origin - np.asarray(centre, np.float64)
        b = d @ o
        disc = b * b - a * (o @ o - radius ** 2)
        t = (-b - np.sqrt(np.where(disc > 0, disc, 0.0))) / a
        nearer = (disc > 0) & (t > 0) & (t < best)
        best = np.where(nearer, t, best)
        normal = np.where(nearer[:, None], o + d * t[:, None], normal)
    hit = np.isfinite(best)
    t = np.where(hit, best, 0.0)
    zaxis = np.asarray(cam.camera_direction, np.float64)
    z = t * (d @ zaxis) / (zaxis @ zaxis)
    depth = np.where(hit, np.floor(np.clip(z / max_depth, 0, 1) * 65535), NO_DEPTH)
    depth = np.minimum(depth, NO_DEPTH).astype(np.uint16)
    color = np.where(hit[:, None], np.rint(analytic_color(np.where(hit[:, None], normal, 1.0)) * 255), 0).astype(np.uint8)
    return depth.reshape(height, width), color.reshape(height, width, 3)


def sphere_scene(directions=ICOSAHEDRON, width=64, height=64, max_depth=10.0, floater=None):
    """-> (cameras, depths, colours) of the analytic sphere (and the floater, if any) seen along `directions`."""
    cameras = [look_at_camera(d) for d in directions]
    images = [render_sphere(c, width, height, max_depth, floater) for c in cameras]
    return cameras, [i[0] for i in images], [i[1] for i in images]


def write_dataset(path, cameras, depths, colors, bbox_min=BBOX_MIN, bbox_max=BBOX_MAX):
    """The directory render_new_dataset.py writes: NNNNN.json / NNNNN.png / NNNNN_depth.png and metadata.json."""
    from PIL import Image

    os.makedirs(path, exist_ok=True)
    for i, (cam, depth, color) in enumerate(zip(cameras, depths, colors)):
        stem = os.path.join(path, f"{i:05d}")
        with open(stem + ".json", "w") as fh:
            fh.write(cam.to_json())
        Image.fromarray(color).save(stem + ".png")
        Image.fromarray(depth.astype(np.uint16)).save(stem + "_depth.png")
    with open(os.path.join(path, "metadata.json"), "w") as fh:
        json.dump({"min": list(bbox_min), "max": list(bbox_max)}, fh)


# ---- the grid ------------------------------------------------------------------------------------------------------
def grid_axes(bbox_min, bbox_max, dims):
    """float32 linspace per axis, as learn_nerf.mesh._axes."""
    return [np.linspace(lo, hi, num=n, dtype=np.float64).astype(np.float32) for lo, hi, n in zip(bbox_min, bbox_max, dims)]


def truncation(bbox_min, bbox_max, dims, truncation_voxels=3.0):
    """float32(truncation_voxels * the largest grid step), computed in float64."""
    return np.float32(float(truncation_voxels) * max((float(b) - float(a)) / (n - 1)
                                                     for a, b, n in zip(bbox_min, bbox_max, dims)))


# ---- integration ---------------------------------------------------------------------------------------------------
def new_state(n):
    return dict(sum_t=np.zeros(n, np.float32), n_obs=np.zeros(n, np.int32), behind=np.zeros(n, np.uint8),
                rgb_sum=np.zeros((n, 3), np.int32), n_col=np.zeros(n, np.int32))


def _dot(r, d, T):
    return (d[0] * T(r[0]) + d[1] * T(r[1])) + d[2] * T(r[2])


def integrate(axes, views, depths, colors, trunc, max_depth, carve=True, state=None, dtype=np.float32):
    """
    The update of csrc/tsdf_geom.h for every voxel of the grid `axes` (float32 [nx], [ny], [nz]) and every view, in view
    order; views: the descriptors of learn_nerf.tsdf.pack_views (only origin, inv, zaxis, width, height are read),
    depths / colours: the images.  `dtype` float32 rounds every operation once, as the kernel does; float64 evaluates
    the same expressions on the same (float32) inputs.  -> (state, margin): margin float64 [N] is, per voxel, the
    smallest distance of any view's cf or rf to an integer and of |q| to 1: below it a rounding error can change a
    decision.
    """
    T = dtype
    p = [np.asarray(g, np.float32).astype(T).reshape(-1) for g in np.meshgrid(*axes, indexing="ij")]
    n = p[0].size
    st = new_state(n) if state is None else state
    sum_t = st["sum_t"].astype(T)
    margin = np.full(n, np.inf)
    trunc, max_depth = T(np.float32(trunc)), T(np.float32(max_depth))
    one, half = T(1), T(0.5)
    for view, depth, color in zip(views, depths, colors):
        W, H = int(view["width"]), int(view["height"])
        d = [p[a] - T(view["origin"][a]) for a in range(3)]
        inv = view["inv"]
        a_, b_, s = _dot(inv[0:3], d, T), _dot(inv[3:6], d, T), _dot(inv[6:9], d, T)
        zc = _dot(view["zaxis"], d, T)
        front = s > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u, v = a_ / s, b_ / s
            cf = ((u + one) * half) * T(W - 1) + half
            rf = ((v + one) * half) * T(H - 1) + half
        ok = front & (cf >= 0) & (cf < T(W)) & (rf >= 0) & (rf < T(H))
        with np.errstate(invalid="ignore"):
            near = np.minimum(np.abs(cf - np.rint(cf)), np.abs(rf - np.rint(rf))).astype(np.float64)
        margin = np.where(front & np.isfinite(near), np.minimum(margin, near), margin)
        idx = np.nonzero(ok)[0]
        row, col = np.floor(rf[idx]).astype(np.int64), np.floor(cf[idx]).astype(np.int64)
        d16 = depth[row, col]
        miss = d16 == NO_DEPTH
        if carve:
            hit_free = idx[miss]
            sum_t[hit_free] = sum_t[hit_free] + one
            st["n_obs"][hit_free] += 1
        idx, row, col, d16 = idx[~miss], row[~miss], col[~miss], d16[~miss]
        zd = d16.astype(T) / T(65535) * max_depth
        q = (zd - zc[idx]) / trunc
        margin[idx] = np.minimum(margin[idx], np.abs(np.abs(q) - one).astype(np.float64))
        is_behind = q < -one
        st["behind"][idx[is_behind]] = 1
        upd = idx[~is_behind]
        qq = q[~is_behind]
        sum_t[upd] = sum_t[upd] + np.where(qq > one, one, qq)
        st["n_obs"][upd] += 1
        col_ok = qq <= one
        st["rgb_sum"][upd[col_ok]] += color[row[~is_behind][col_ok], col[~is_behind][col_ok]].astype(np.int32)
        st["n_col"][upd[col_ok]] += 1
    st["sum_t"] = sum_t  # float32, or float64 for the float64 evaluation
    return st, margin


def distance(state, dtype=np.float32):
    """F = sum_t / n_obs where observed (NaN elsewhere), one rounded division."""
    with np.errstate(divide="ignore", invalid="ignore"):
        f = state["sum_t"].astype(dtype) / state["n_obs"].astype(dtype)
    return np.where(state["n_obs"] > 0, f, dtype(np.nan))


def volume(state, dims, unseen="inside"):
    """float32 [nx+2, ny+2, nz+2]: -F at the grid points, -1 on the padding layer (lnrf_tsdf_volume)."""
    assert unseen in ("inside", "outside")
    f = distance(state)
    fill = np.where((state["behind"] != 0) & (unseen == "inside"), np.float32(-1), np.float32(1))
    inner = -np.where(state["n_obs"] > 0, f, fill).astype(np.float32)
    out = np.full([n + 2 for n in dims], -1, np.float32)
    out[1:-1, 1:-1, 1:-1] = inner.reshape(dims)
    return out


def vertex_colors(verts, dims, state):
    """(float32 [V, 3], number of grey vertices): lnrf_tsdf_vertex_colors for padded index-space vertices."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    lo, hi = np.floor(v), np.ceil(v)
    frac = v - lo
    f = np.where(frac[:, 0] > 0, frac[:, 0], np.where(frac[:, 1] > 0, frac[:, 1], np.where(frac[:, 2] > 0, frac[:, 2],
                                                                                           np.float32(0))))
    top = np.asarray(dims, np.float32) - 1
    mean, has = [], []
    for end in (lo - 1, hi - 1):
        with np.errstate(invalid="ignore"):
            ok = ((end >= 0) & (end <= top)).all(axis=1)
        e = np.where(ok[:, None], end, 0).astype(np.int64)
        idx = (e[:, 0] * dims[1] + e[:, 1]) * dims[2] + e[:, 2]
        n = np.where(ok, state["n_col"][idx], 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = state["rgb_sum"][idx].astype(np.float32) / n.astype(np.float32)[:, None] / np.float32(255)
        has.append(n > 0)
        mean.append(np.where(has[-1][:, None], m, np.float32(0.5)).astype(np.float32))
    both = mean[0] + f[:, None] * (mean[1] - mean[0])
    out = np.where((has[0] & has[1])[:, None], both, np.where(has[0][:, None], mean[0], mean[1])).astype(np.float32)
    return out, int((~(has[0] | has[1])).sum())


def world_vertices(verts, bbox_min, bbox_max, dims):
    """learn_nerf.mesh.world_frame per axis."""
    lo = np.asarray(bbox_min, np.float64)
    step = (np.asarray(bbox_max, np.float64) - lo) / (np.asarray(dims, np.float64) - 1)
    return (lo + (np.asarray(verts, np.float64) - 1) * step).astype(np.float32)

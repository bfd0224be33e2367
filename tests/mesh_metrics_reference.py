"""
NumPy restatement of the mesh comparison (csrc/raycast.hip "Nearest triangle", csrc/mesh_metrics.hip,
learn_nerf/mesh_metrics.py), for the tests.  Nothing here imports the package.

  * the pinned fp32 point-triangle distance as a brute force over every (point, triangle) pair with the tie rule, and
    the same query through a restated tree (so that the pruning rule and the margin can be mutated);
  * the area and the stratified sampler, with oracle/philox.py;
  * the fixed-order fp64 fold of csrc/stat_reduce.h and the statistics and metrics built on it;
  * an exact (float64) point-triangle distance and the DERIVED BOUNDS that tie the pinned one to it.

DERIVED BOUNDS (EPS = 2^-24, the unit roundoff of fp32; rho = |p - c|_1 + 3 radius as in the kernel, so rho >= S + E
with S the distance from p to any vertex and E any edge length).  Every vector the formula forms is RELATIVE (p - a,
b - a, w - t d, ...), never an absolute position, so each rounding is a fraction EPS of a length <= S + E <= rho:
 * every candidate point q (a + t d with 0 <= t <= 1; a + u e1 + v e2 with u, v >= 0, fl(u + v) <= 1) lies in the
   triangle up to EPS E, and the residual r = w - t d (or (w - u e1) - v e2) is off by at most EPS (|w| + 2 |d| + |r|)
   (+ the same again for the second edge) <= 8 EPS (S + E); its squared norm adds 3.01 EPS relative, 1.51 EPS on the
   distance.  So the pinned distance is never more than LOWER_C EPS rho BELOW the exact one, LOWER_C = 16, for EVERY
   finite triangle, degenerate or not.  This is all the tree's margin needs (the kernel header has that argument).
 * a segment: dd and wd carry 5.01 EPS (two rounded factors, three roundings of the dot product), t = wd / dd is off by
   at most 11.2 EPS |w| / |d| before the clamp (which is 1-Lipschitz), so the point moves by 11.2 EPS S along the
   segment: with the residual's 5.6 EPS rho the segment distance is within 17 EPS rho of the exact one.
 * the face, for a triangle with s = |e1 x e2| / (|e1| |e2|) > 0: the computed normal N is off by at most
   4.5 EPS |e1| |e2| = eta |n|, eta = 4.5 EPS / s.  With N held fixed, u = ((w x e2) . N) / (N . N) and v are the
   coordinates of kappa q', q' the projection of w onto the plane ALONG N and |kappa - 1| <= 1.01 eta: q' is within
   1.01 eta S of the true foot, kappa moves it by 1.01 eta S more (9.2 EPS S / s together).  The roundings of w x e2,
   the dot product, N . N and the division move u by 11.8 EPS |w| / (|e1| s), i.e. the point by 11.8 EPS S / s, and
   the same for v.  So the foot is off by at most 33 EPS S / s, and a wrong inside / outside decision that close to
   the border costs no more than that either, because the segments cover the border.
   Together: the pinned distance is at most UPPER_C(s) EPS rho ABOVE the exact one, UPPER_C(s) = 32 + 40 / s (both
   terms rounded up), for a triangle the tree does not class as a sliver (s >= 2^-6) — and UPPER_C(1) for a triangle
   of exactly zero area, where every candidate lies on the segment the triangle has collapsed to.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import philox  # noqa: E402

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
LOWER_C = 16.0
MARGIN = 2.0 ** -11  # kMargin of csrc/raycast.hip: mu = MARGIN * rho
SLIVER_SIN = 2.0 ** -6
MAX_COORD, MIN_EXTENT = 2.0 ** 20, 2.0 ** -20


def upper_c(s=1.0):
    return 32.0 + 40.0 / s


# ------------------------------------------------------------------ the box of a mesh, as TriangleMesh states it ----

def mesh_box(tris):
    """(center float32 [3], radius float32) exactly as learn_nerf.raycast.TriangleMesh passes them to the kernels."""
    flat = np.asarray(tris, dtype=F32).reshape(-1, 3)
    lo, hi = flat.min(axis=0).astype(F64), flat.max(axis=0).astype(F64)
    half = (hi - lo) / 2
    return ((lo + hi) / 2).astype(F32), np.nextafter(F32(half.sum()), F32(np.inf))


def rho_of(tris, pts):
    """float64 [m]: rho = |p - c|_1 + 3 radius, exact to float64."""
    center, radius = mesh_box(tris)
    return np.abs(np.asarray(pts, F64) - center.astype(F64)).sum(axis=1) + 3.0 * float(radius)


def lower_bound(rho):
    return LOWER_C * EPS * rho


def upper_bound(rho, s=1.0):
    return upper_c(s) * EPS * rho


def shape_sine(tris):
    """float64 [n]: |e1 x e2| / (|e1| |e2|), 0 where an edge is 0."""
    t = np.asarray(tris, dtype=F64)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    den = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    with np.errstate(all="ignore"):
        return np.where(den > 0, np.linalg.norm(np.cross(e1, e2), axis=1) / den, 0.0)


# ------------------------------------------------------------------------------------ the pinned distance (fp32) ----

def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _segment(w, d):
    """(d2, t) of the clamped segment t d, t in [0, 1], against the offset w; a zero-length segment takes t = 0."""
    dd, wd = _dot(d, d), _dot(w, d)
    t = np.where(dd > 0, wd / dd, F32(0))
    t = np.where(t > 0, t, F32(0))
    t = np.where(t < 1, t, F32(1)).astype(F32)
    r = [w[a] - t * d[a] for a in range(3)]
    return _dot(r, r), t


def pair_distance(tris, pts, drop=None, want_point=False):
    """d2 float32 [m, n] of the pinned distance (and the closest points float32 [m, n, 3]), every operation one float32
    rounding.  drop in (0, 1, 2, 3) leaves out the candidate a-b, b-c, a-c or the face: a mutation for the tests."""
    tris = np.asarray(tris, dtype=F32)
    pts = np.asarray(pts, dtype=F32)
    p = [pts[:, a][:, None] for a in range(3)]
    va, vb, vc = ([tris[:, k, a][None, :] for a in range(3)] for k in range(3))
    with np.errstate(all="ignore"):
        e1 = [vb[a] - va[a] for a in range(3)]
        e2 = [vc[a] - va[a] for a in range(3)]
        e3 = [vc[a] - vb[a] for a in range(3)]
        w = [p[a] - va[a] for a in range(3)]
        z = [p[a] - vb[a] for a in range(3)]
        shape = np.broadcast(w[0], e1[0]).shape
        d2 = np.full(shape, np.inf, dtype=F32)
        which = np.zeros(shape, dtype=np.int8)
        params = []
        for k, (off, edge) in enumerate(((w, e1), (z, e3), (w, e2))):
            s2, t = _segment(off, edge)
            params.append(np.broadcast_to(t, shape))
            if drop == k:
                continue
            take = s2 < d2
            d2, which = np.where(take, s2, d2), np.where(take, np.int8(k), which)
        n = _cross(e1, e2)
        nn = _dot(n, n)
        u = _dot(_cross(w, e2), n) / nn
        v = _dot(_cross(e1, w), n) / nn
        inside = (nn > 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
        r = [(w[a] - u * e1[a]) - v * e2[a] for a in range(3)]
        f2 = _dot(r, r)
        take = inside & (f2 < d2)
        if drop != 3:
            d2, which = np.where(take, f2, d2), np.where(take, np.int8(3), which)
        assert d2.dtype == F32
        if not want_point:
            return d2
        cp = np.empty(shape + (3,), dtype=F32)
        for a in range(3):
            c0 = va[a] + params[0] * e1[a]
            c1 = vb[a] + params[1] * e3[a]
            c2 = va[a] + params[2] * e2[a]
            c3 = (va[a] + u * e1[a]) + v * e2[a]
            cp[..., a] = np.where(which == 0, c0, np.where(which == 1, c1, np.where(which == 2, c2, c3)))
    return d2, cp


def brute_force_nearest(tris, pts, chunk=512, drop=None, want_point=False):
    """-> (d2 float32 [m], id int32 [m][, closest float32 [m, 3]]): the smallest pinned d2 over all triangles and the
    lowest triangle index among equal d2."""
    pts = np.asarray(pts, dtype=F32)
    m = len(pts)
    out_d2, out_id = np.empty(m, dtype=F32), np.empty(m, dtype=np.int32)
    out_cp = np.empty((m, 3), dtype=F32)
    for start in range(0, m, chunk):
        sl = slice(start, start + chunk)
        res = pair_distance(tris, pts[sl], drop=drop, want_point=want_point)
        d2 = res[0] if want_point else res
        best = d2.argmin(axis=1)  # the first of equal minima: the lowest index
        rows = np.arange(len(best))
        out_d2[sl], out_id[sl] = d2[rows, best], best
        if want_point:
            out_cp[sl] = res[1][rows, best]
    return (out_d2, out_id, out_cp) if want_point else (out_d2, out_id)


def count_ties(tris, pts, chunk=512):
    """How many queries have their minimum d2 attained by more than one triangle."""
    pts = np.asarray(pts, dtype=F32)
    total = 0
    for start in range(0, len(pts), chunk):
        d2 = pair_distance(tris, pts[start:start + chunk])
        total += int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return total


# ----------------------------------------------------------------------------------------- the exact distance ----

def exact_distance(tris, pts):
    """float64 [m, n]: the point-triangle distance in float64 by another route (Gram-matrix barycentric coordinates of
    the plane projection, else the nearest of the three segments), valid for zero-area triangles too."""
    t = np.asarray(tris, dtype=F64)
    p = np.asarray(pts, dtype=F64)[:, None, :]
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]

    def seg(p0, p1):
        d = p1 - p0
        dd = (d * d).sum(-1)
        with np.errstate(all="ignore"):
            tt = np.where(dd > 0, ((p - p0) * d).sum(-1) / dd, 0.0)
        tt = np.clip(tt, 0.0, 1.0)
        return np.linalg.norm(p - (p0 + tt[..., None] * d), axis=-1)

    best = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    e1, e2, w = b - a, c - a, p - a
    g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    w1, w2 = (w * e1).sum(-1), (w * e2).sum(-1)
    det = g11 * g22 - g12 * g12
    with np.errstate(all="ignore"):
        u = (g22 * w1 - g12 * w2) / det
        v = (g11 * w2 - g12 * w1) / det
        inside = (det > 1e-24 * g11 * g22) & (u >= 0) & (v >= 0) & (u + v <= 1)
        foot = np.linalg.norm(w - u[..., None] * e1 - v[..., None] * e2, axis=-1)
    return np.where(inside, np.minimum(foot, best), best)


# ------------------------------------------------------------------------------------------ the tree, restated ----

def _is_sliver(v):
    v = v.astype(F32)
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n = np.stack(_cross(a.T, b.T), axis=1)
    n2, a2, b2 = (n * n).sum(1, dtype=F32), (a * a).sum(1, dtype=F32), (b * b).sum(1, dtype=F32)
    return ~(n2 > 0) | ~(n2 >= F32(2.0 ** -12) * (a2 * b2))


def build_tree(tris, leaf=4):
    """The structure of csrc/raycast.hip: Morton order of the centroids (slivers last, stable), leaves of `leaf`
    triangles, the implicit heap of boxes (slivers: (-inf, +inf); empty: lo > hi).  Results never depend on it."""
    tris = np.asarray(tris, dtype=F32)
    n = len(tris)
    flat = tris.reshape(-1, 3)
    lo, hi = flat.min(axis=0).astype(F64), flat.max(axis=0).astype(F64)
    sliver = _is_sliver(tris)
    cen = tris.astype(F64).mean(axis=1)
    ext = np.where(hi > lo, hi - lo, 1.0)
    q = np.clip(((cen - lo) / ext * 1024).astype(np.int64), 0, 1023)
    codes = np.zeros(n, dtype=np.int64)
    for bit in range(10):
        for a in range(3):
            codes |= ((q[:, a] >> bit) & 1) << (3 * bit + (2 - a))
    codes[sliver] = 1 << 30
    order = np.argsort(codes, kind="stable").astype(np.int32)
    sorted_tris = tris[order]
    leaves = 1
    while leaves * leaf < n:
        leaves *= 2
    nlo = np.full((2 * leaves, 3), np.inf, dtype=F32)
    nhi = np.full((2 * leaves, 3), -np.inf, dtype=F32)
    for j in range(leaves):
        part = sorted_tris[j * leaf:(j + 1) * leaf]
        if len(part) == 0:
            continue
        if sliver[order[j * leaf:(j + 1) * leaf]].any():
            nlo[leaves + j], nhi[leaves + j] = -np.inf, np.inf
        else:
            nlo[leaves + j], nhi[leaves + j] = part.reshape(-1, 3).min(axis=0), part.reshape(-1, 3).max(axis=0)
    for k in range(leaves - 1, 0, -1):
        nlo[k], nhi[k] = np.minimum(nlo[2 * k], nlo[2 * k + 1]), np.maximum(nhi[2 * k], nhi[2 * k + 1])
    center, radius = mesh_box(tris)
    return dict(n=n, leaf=leaf, leaves=leaves, order=order, sorted_tris=sorted_tris, lo=nlo, hi=nhi, center=center,
                radius=radius)


def tree_nearest(tree, pts, margin=MARGIN, strict=True, drop=None):
    """(d2 float32 [m], id int32 [m]) by the kernel's walk: a node is skipped when the squared distance from the point
    to its box, each face moved out by mu = margin * rho, exceeds the best d2 so far.  strict=False prunes with >=
    and margin=0 drops the widening: the two mutations the tests must reject."""
    pts = np.asarray(pts, dtype=F32)
    pair = pair_distance(tree["sorted_tris"], pts, drop=drop)
    lo, hi, order = tree["lo"], tree["hi"], tree["order"]
    leaves, leaf, n = tree["leaves"], tree["leaf"], tree["n"]
    c, radius, zero = tree["center"], tree["radius"], F32(0)
    out_d2, out_id = np.empty(len(pts), dtype=F32), np.empty(len(pts), dtype=np.int32)
    with np.errstate(all="ignore"):
        for i, p in enumerate(pts):
            mu = F32(margin) * (((abs(p[0] - c[0]) + abs(p[1] - c[1])) + abs(p[2] - c[2])) + F32(3) * radius)
            best, best_id, k = F32(np.inf), -1, 1
            while True:
                hit = False
                if lo[k][0] <= hi[k][0]:
                    g = np.maximum(np.maximum((lo[k] - p) - mu, (p - hi[k]) - mu), zero)
                    box = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
                    hit = not (box > best) if strict else not (box >= best)
                if hit and k < leaves:
                    k = 2 * k
                    continue
                if hit:
                    begin = (k - leaves) * leaf
                    for j in range(begin, min(begin + leaf, n)):
                        d2 = pair[i, j]
                        if d2 <= best and (d2 < best or best_id < 0 or order[j] < best_id):
                            best, best_id = d2, int(order[j])
                k += 1
                while k % 2 == 0:
                    k //= 2
                if k == 1:
                    break
            out_d2[i], out_id[i] = best, best_id
    return out_d2, out_id


# ------------------------------------------------------------------------------------------- areas and sampling ----

def tri_areas(tris):
    """float32 [n]: 0.5 * sqrt(|e1 x e2|^2), one float32 rounding per operation."""
    t = np.asarray(tris, dtype=F32)
    with np.errstate(all="ignore"):
        e1 = [t[:, 1, a] - t[:, 0, a] for a in range(3)]
        e2 = [t[:, 2, a] - t[:, 0, a] for a in range(3)]
        n = _cross(e1, e2)
        area = F32(0.5) * np.sqrt(_dot(n, n))
    assert area.dtype == F32
    return area


def area_cdf(tris):
    """float64 [n]: the running sum of the float32 areas, added one by one in float64."""
    return np.cumsum(tri_areas(tris).astype(F64))


def sample_surface(tris, order, cdf, m, seed, stream):
    """(points float32 [m, 3], ids int32 [m], j int64 [m]): the sampler of csrc/mesh_metrics.hip over `tris` in their
    given (sorted) order with the running sum `cdf`; ids = order[j], or j without an order."""
    t = np.asarray(tris, dtype=F32)
    cdf = np.asarray(cdf, dtype=F64)
    n, total = len(t), cdf[-1]
    u = philox.uniform(seed, stream, 0, 3 * m).reshape(m, 3)
    x = ((np.arange(m, dtype=F64) + u[:, 0].astype(F64)) / F64(m)) * total
    j = np.searchsorted(cdf, x, side="right")  # the first index with cdf[j] > x
    j = np.where(j == n, np.searchsorted(cdf, total, side="left"), j)
    u1, u2 = u[:, 1], u[:, 2]
    fold = (u1 + u2) > F32(1)
    u1, u2 = np.where(fold, F32(1) - u1, u1), np.where(fold, F32(1) - u2, u2)
    v = t[j]
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    pts = (v[:, 0] + u1[:, None] * e1) + u2[:, None] * e2
    assert pts.dtype == F32
    ids = (np.asarray(order)[j] if order is not None else j).astype(np.int32)
    return pts, ids, j


# ------------------------------------------------------------------------------------- the fixed-order fp64 fold ----

BLOCK, MAX_GRID = 256, 1024


def _block_sum(v):
    """[..., 256] -> [...]: xor butterfly (32, 16, ..., 1) within each wave of 64, then the four waves in order."""
    w = np.asarray(v, dtype=F64).reshape(v.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ off]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def fold_sum(terms, acc=0.0):
    """acc + the sum of the float64 terms in the order of csrc/stat_reduce.h (terms >= 0, so padding with +0 changes
    no bit)."""
    terms = np.asarray(terms, dtype=F64).reshape(-1)
    m = len(terms)
    if m == 0:
        return acc
    grid = min((m + BLOCK - 1) // BLOCK, MAX_GRID)
    rounds = (m + grid * BLOCK - 1) // (grid * BLOCK)
    padded = np.zeros(rounds * grid * BLOCK, dtype=F64)
    padded[:m] = terms
    padded = padded.reshape(rounds, grid, BLOCK)
    s = np.zeros((grid, BLOCK), dtype=F64)
    for r in range(rounds):
        s = s + padded[r]
    parts = np.zeros(MAX_GRID, dtype=F64)
    parts[:grid] = _block_sum(s)
    per_thread = parts.reshape(BLOCK, MAX_GRID // BLOCK)
    t = np.zeros(BLOCK, dtype=F64)
    for k in range(MAX_GRID // BLOCK):
        t = t + per_thread[:, k]
    return F64(acc) + _block_sum(t)


def dist_stats(d2, cosine, thresholds, acc=None):
    """float64 [4 + K]: lnrf_dist_stats_f64 added into acc (zeros by default)."""
    d2 = np.asarray(d2, dtype=F32)
    acc = np.zeros(4 + len(thresholds), dtype=F64) if acc is None else np.array(acc, dtype=F64)
    if len(d2) == 0:
        return acc
    dist = np.sqrt(d2.astype(F64))
    acc[0] = fold_sum(dist, acc[0])
    acc[1] = fold_sum(d2.astype(F64), acc[1])
    if cosine is not None:
        acc[2] = fold_sum(np.abs(np.asarray(cosine, dtype=F32).astype(F64)), acc[2])
    acc[3] = max(acc[3], float(d2.max()))
    for k, tau in enumerate(thresholds):
        acc[4 + k] += float((dist <= F64(tau)).sum())
    return acc


# --------------------------------------------------------------------------------------------------- the metrics ----

def unit_normals(tris, ids):
    """(n float64 [m, 3], length float64 [m]): e1 x e2 / length, 0 where length is 0."""
    v = np.asarray(tris, dtype=F32)[np.asarray(ids)].astype(F64)
    n = _cross([v[:, 1, a] - v[:, 0, a] for a in range(3)], [v[:, 2, a] - v[:, 0, a] for a in range(3)])
    length = np.sqrt(_dot(n, n))
    with np.errstate(all="ignore"):
        return np.stack([np.where(length > 0, c / length, 0.0) for c in n], axis=1), length


def normal_cosines(own_tris, own_ids, other_tris, near_ids):
    a, _ = unit_normals(own_tris, own_ids)
    b, length = unit_normals(other_tris, near_ids)
    return _dot(a.T, b.T).astype(F32), int((length == 0).sum())


def metrics_from_stats(pred_acc, ref_acc, samples, pred_valid, ref_valid, thresholds):
    m = float(samples)
    accuracy, completeness = float(pred_acc[0]) / m, float(ref_acc[0]) / m
    precision = tuple(float(pred_acc[4 + k]) / m for k in range(len(thresholds)))
    recall = tuple(float(ref_acc[4 + k]) / m for k in range(len(thresholds)))
    f_score = tuple(2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall))
    means = [float(a[2]) / v for a, v in ((pred_acc, pred_valid), (ref_acc, ref_valid)) if v > 0]
    return dict(accuracy=accuracy, completeness=completeness, chamfer=accuracy + completeness,
                chamfer_l2=float(pred_acc[1]) / m + float(ref_acc[1]) / m, precision=precision, recall=recall,
                f_score=f_score, hausdorff=math.sqrt(max(float(pred_acc[3]), float(ref_acc[3]))),
                normal_consistency=sum(means) / len(means) if means else math.nan)


def compare_from_samples(pred_tris, ref_tris, pred_pts, pred_ids, ref_pts, ref_ids, thresholds, chunk=256):
    """The metrics from given sample sets, by the brute force and the fold above."""
    accs, valid = [], []
    for own, other, pts, ids in ((pred_tris, ref_tris, pred_pts, pred_ids), (ref_tris, pred_tris, ref_pts, ref_ids)):
        d2, near = brute_force_nearest(other, pts, chunk=chunk)
        cosine, bad = normal_cosines(own, ids, other, near)
        accs.append(dist_stats(d2, cosine, thresholds))
        valid.append(len(pts) - bad)
    return metrics_from_stats(accs[0], accs[1], len(pred_pts), valid[0], valid[1], thresholds), accs


def compare_reference(pred_tris, ref_tris, samples, thresholds, seed=0):
    """compare_meshes from the restatement alone: the samples come from sample_surface over the restated tree order."""
    sets = []
    for tris, stream in ((pred_tris, 0), (ref_tris, 1)):
        tree = build_tree(tris)
        pts, ids, _ = sample_surface(tree["sorted_tris"], tree["order"], area_cdf(tree["sorted_tris"]), samples, seed,
                                     stream)
        sets += [pts, ids]
    return compare_from_samples(pred_tris, ref_tris, sets[0], sets[1], sets[2], sets[3], thresholds)[0]


# ---------------------------------------------------------------------------------------------------- test inputs ----

def degenerate_triangles():
    """Zero-area triangles and slivers, as marching cubes and TSDF fusion emit them: a point, segments with a repeated
    vertex, three distinct collinear vertices, and two needles of tiny but non-zero area."""
    p, q, r = np.array([0.1, 0.2, 0.9]), np.array([0.7, -0.3, 0.8]), np.array([-0.4, 0.6, -0.7])
    return np.array([[p, p, p], [p, p, q], [p, q, p], [q, p, p], [p, q, q], [p, (p + q) / 2, q], [r, r, r],
                     [r, q, (r + q) / 2 + [0.0, 1e-6, 0.0]], [p, r, r + [1e-7, 0.0, 0.0]]], dtype=F32)


def feature_points(tris, rng, count):
    """Points exactly on vertices, on edge midpoints and inside faces (as exactly as float32 allows) of random triangles
    of the mesh: d2 is 0 or a few ulps there, and triangles that share the feature tie."""
    tris = np.asarray(tris, dtype=F32)
    some = tris[rng.integers(0, len(tris), size=count)].astype(F64)
    w = rng.dirichlet(np.ones(3), size=count)
    return np.concatenate([some.reshape(-1, 3), ((some + np.roll(some, 1, axis=1)) / 2).reshape(-1, 3),
                           (some * w[:, :, None]).sum(axis=1)]).astype(F32)


def query_set(tris, seed=0, count=48, extra=None):
    """A few hundred queries of every kind the kernel treats differently: random in and around the box; on vertices,
    edge midpoints and faces; just off the vertices and faces (where a wrong margin shows); the box centre and points on
    its symmetry planes (ties on a symmetric mesh); far away (1000 extents, and near 2^20)."""
    rng = np.random.default_rng(seed)
    tris = np.asarray(tris, dtype=F32)
    flat = tris.reshape(-1, 3).astype(F64)
    lo, hi = flat.min(axis=0), flat.max(axis=0)
    mid, ext = (lo + hi) / 2, max(float((hi - lo).max()), 2.0 ** -20)
    sets = [mid + rng.uniform(-0.75, 0.75, size=(2 * count, 3)) * ext]
    on = feature_points(tris, rng, count // 3).astype(F64)
    sets.append(on)
    for scale in (1e-7, 1e-5, 1e-3):  # just off the features, outward and in random directions
        sets.append(on + (on - mid) * scale)
        sets.append(on + rng.normal(size=on.shape) * ext * scale)
    plane = mid + rng.uniform(-0.6, 0.6, size=(count // 2, 3)) * ext
    plane[:, 0] = mid[0]
    diag = mid + np.repeat(rng.uniform(-0.6, 0.6, size=(count // 2, 1)), 3, axis=1) * ext
    sets += [mid[None, :], plane, diag]
    unit = rng.normal(size=(count // 2, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    sets.append(mid + unit * ext * 1000.0)
    sets.append(np.clip(unit * 2.0 ** 20, -(2.0 ** 20), 2.0 ** 20))
    if extra is not None:
        sets.append(np.asarray(extra, dtype=F64).reshape(-1, 3))
    return np.clip(np.concatenate(sets), -MAX_COORD, MAX_COORD).astype(F32)


def nearest_cases():
    """name -> triangles of the meshes the nearest query is tested on (tests/raycast_reference.py builds them)."""
    import raycast_reference as R

    soup = R.soup(1000, seed=1)
    mixed = np.concatenate([degenerate_triangles()[:3], soup[:500], degenerate_triangles()[3:], soup[500:],
                            soup[10:14]])  # four duplicates at the end: ties that the lowest index wins
    return {"one": np.array([[[-1, -1, 0.2], [1, -1, 0.1], [0, 1, -0.3]]], dtype=F32), "cube": R.cube(0.5),
            "icosphere2": R.icosphere(2), "soup_mixed": mixed.astype(F32), "soup_13": R.soup(13, seed=2, size=0.3)}

"""
NumPy restatement of the mesh simplifier's conventions (csrc/simplify.hip, csrc/simplify_geom.h,
learn_nerf/simplify.py), for the tests: the cell of a corner in pinned float32, the surviving faces and their
duplicates, the per-cell fold in float64 in its fixed order, the placement by a cyclic Jacobi eigen-decomposition, the
grid rule and the search for target_faces.  Every float operation is one NumPy elementwise call, so it is rounded once
and never reassociated.  Nothing here imports the package.
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
INT32_MAX = 2**31 - 1
CHUNK = 16
JACOBI_SWEEPS = 6
RANK_THRESHOLD = 1e-3
MAX_TARGET_CELLS = 1024


# ------------------------------------------------------------------ grid ----

def make_grid(lo, hi, cell_size=None, cells=None):
    """(h float64, inv_h float32, dims [3] int) of the grid with origin lo (float32 [3]) that holds hi (float32 [3]):
    h = cell_size, or the longest extent / cells (float64); inv_h = float32(1 / h); n_a = floorf(fl(fl(hi_a - lo_a) *
    inv_h)) + 1 — the index of the highest corner plus one, in the arithmetic of the cell rule — capped at `cells`
    when that is given, so that the grid has `cells` cells along the longest axis."""
    lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    if cells is not None:
        h = float(np.max(hi.astype(F64) - lo.astype(F64))) / int(cells)
    else:
        h = float(cell_size)
    if not (h > 0 and math.isfinite(h)):
        raise ValueError(f"the cell edge must be positive and finite, got {h}")
    with np.errstate(over="ignore"):
        inv_h = F32(1.0 / h)
    if not (inv_h > 0 and np.isfinite(inv_h)):
        raise ValueError(f"the cell edge {h} has no finite positive float32 inverse")
    t = np.floor((hi - lo) * inv_h)
    if not (t < 2.0**31).all():
        raise ValueError("the grid has 2^31 cells or more along an axis")
    dims = [max(1, int(v) + 1) for v in t]
    if cells is not None:
        dims = [min(int(cells), n) for n in dims]
    if math.prod(dims) > INT32_MAX:
        raise ValueError(f"the grid {dims} has 2^31 cells or more: the cell key is an int32")
    return h, inv_h, dims


def cell_coords(pts, lo, inv_h, dims):
    """int64 [n, 3]: min(n_a - 1, (int)floorf((p_a - lo_a) * inv_h)) per axis, float32, one rounding per operation."""
    pts = np.asarray(pts, dtype=F32).reshape(-1, 3)
    t = np.floor((pts - np.asarray(lo, dtype=F32)) * F32(inv_h))
    top = np.asarray(dims, dtype=np.int64) - 1
    return np.where(t >= top.astype(F32), top, np.where(t > 0, t, 0).astype(np.int64))


def cell_keys(pts, lo, inv_h, dims):
    c = cell_coords(pts, lo, inv_h, dims)
    return ((c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]).astype(np.int32)


def wall_distance(pts, lo, h):
    """Distance of every coordinate to the nearest cell wall, in cells (float64)."""
    t = (np.asarray(pts, dtype=F64).reshape(-1, 3) - np.asarray(lo, dtype=F64)) / h
    return np.abs(t - np.rint(t))


# ----------------------------------------------------------------- faces ----

def survivors(keys):
    """bool [F]: the triangles whose three corners lie in three distinct cells; keys int32 [3F]."""
    k = np.asarray(keys).reshape(-1, 3)
    return (k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])


def output_faces(keys):
    """(face keys int64 [M, 3], source triangle int64 [M], duplicates removed): the survivors in input order without
    the later copies of a face that equals an earlier one up to cyclic rotation."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    seen, rows, src, dups = set(), [], [], 0
    for t in np.nonzero(survivors(keys))[0]:
        a, b, c = (int(v) for v in k[t])
        canon = min((a, b, c), (b, c, a), (c, a, b))
        if canon in seen:
            dups += 1
            continue
        seen.add(canon)
        rows.append((a, b, c))
        src.append(t)
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3), np.asarray(src, dtype=np.int64), dups


# ------------------------------------------------------------------ fold ----

def tri_normals(a, b, c):
    """(b - a) x (c - a) in float64, columns as separate arrays."""
    e1 = [b[:, i] - a[:, i] for i in range(3)]
    e2 = [c[:, i] - a[:, i] for i in range(3)]
    return [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]


def tri_quadrics(tris):
    """float64 [F, 10]: (A upper triangle, b, c) of the area-weighted plane quadric, 0 for a triangle without area."""
    v = np.asarray(tris, dtype=F32).reshape(-1, 3, 3).astype(F64)
    a = v[:, 0]
    n = tri_normals(a, v[:, 1], v[:, 2])
    w = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    d = (n[0] * a[:, 0] + n[1] * a[:, 1]) + n[2] * a[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        cols = [(n[0] * n[0]) / w, (n[0] * n[1]) / w, (n[0] * n[2]) / w, (n[1] * n[1]) / w, (n[1] * n[2]) / w,
                (n[2] * n[2]) / w, (n[0] * d) / w, (n[1] * d) / w, (n[2] * d) / w, (d * d) / w]
    q = np.stack(cols, axis=1)
    q[~(w > 0)] = 0.0
    return q


def entry_terms(tris, keys):
    """float64 [3F, 13]: the contribution of every entry e = 3t + k: the corner position and, when no earlier corner
    of t has the same key, the quadric of t."""
    v = np.asarray(tris, dtype=F32).reshape(-1, 3, 3)
    k = np.asarray(keys).reshape(-1, 3)
    first = np.stack([np.ones(len(k), bool), k[:, 1] != k[:, 0], (k[:, 2] != k[:, 0]) & (k[:, 2] != k[:, 1])], axis=1)
    q = tri_quadrics(v)
    u = np.zeros((len(k), 3, 13), F64)
    u[:, :, :3] = v.astype(F64)
    u[:, :, 3:] = np.where(first[:, :, None], q[:, None, :], 0.0)
    return u.reshape(-1, 13)


def fold_segment(u):
    """The fixed-order sum of the rows of u [L, w] float64: chunks of 16 rows (padded with +0) are summed by the
    balanced tree x_j + x_{j+8}, then + 4, + 2, + 1, and the chunk sums are added to +0 in chunk order."""
    u = np.asarray(u, dtype=F64)
    chunks = -(-len(u) // CHUNK)
    padded = np.zeros((chunks * CHUNK, u.shape[1]), F64)
    padded[:len(u)] = u
    x = padded.reshape(chunks, CHUNK, -1)
    for half in (8, 4, 2, 1):
        x = x[:, :half] + x[:, half:2 * half]
    acc = np.zeros(u.shape[1], F64)
    for m in range(chunks):
        acc = acc + x[m, 0]
    return acc


def segments(keys):
    """(cell keys int32 [C] ascending, order int64 [3F], seg_start int64 [C + 1]) of the stable sort by key."""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind="stable")
    cells, start = np.unique(keys[order], return_index=True)
    return cells.astype(np.int32), order, np.append(start, len(keys)).astype(np.int64)


def accumulate(tris, keys, colors=None):
    """Per occupied cell, ascending: (cell keys, counts int32 [C], sums float64 [C, 13], colour sums int64 [C, 3] or
    None).  colors: uint8 [3F, 3], one per corner."""
    cells, order, start = segments(keys)
    u = entry_terms(tris, keys)[order]
    sums = np.stack([fold_segment(u[start[i]:start[i + 1]]) for i in range(len(cells))]) if len(cells) else \
        np.zeros((0, 13), F64)
    counts = np.diff(start).astype(np.int32)
    col = None
    if colors is not None:
        c = np.asarray(colors, dtype=np.int64).reshape(-1, 3)[order]
        col = np.stack([c[start[i]:start[i + 1]].sum(axis=0) for i in range(len(cells))]).reshape(-1, 3)
    return cells, counts, sums, col


# ------------------------------------------------------------- placement ----

def jacobi(a, sweeps=JACOBI_SWEEPS):
    """(eigenvalues [C, 3], eigenvectors [C, 3, 3] as columns, off-diagonal mass / Frobenius norm [C]) of the symmetric
    matrices a [C, 3, 3] after `sweeps` cyclic sweeps over (0,1), (0,2), (1,2), the rotation of simplify_geom.h."""
    a = np.array(a, dtype=F64)
    v = np.broadcast_to(np.eye(3), a.shape).copy()
    norm = np.sqrt((a * a).sum(axis=(1, 2)))
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = a[:, p, q].copy()
                live = apq != 0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                t, c, s = np.where(live, t, 0.0), np.where(live, c, 1.0), np.where(live, s, 0.0)
                a[:, p, p] = np.where(live, a[:, p, p] - t * apq, a[:, p, p])
                a[:, q, q] = np.where(live, a[:, q, q] + t * apq, a[:, q, q])
                a[:, p, q] = a[:, q, p] = np.where(live, 0.0, apq)
                arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                a[:, r, p] = a[:, p, r] = np.where(live, c * arp - s * arq, arp)
                a[:, r, q] = a[:, q, r] = np.where(live, s * arp + c * arq, arq)
                for k in range(3):
                    vkp, vkq = v[:, k, p].copy(), v[:, k, q].copy()
                    v[:, k, p] = np.where(live, c * vkp - s * vkq, vkp)
                    v[:, k, q] = np.where(live, s * vkp + c * vkq, vkq)
        off = np.sqrt(2.0 * (a[:, 0, 1] ** 2 + a[:, 0, 2] ** 2 + a[:, 1, 2] ** 2))
        ratio = np.where(norm > 0, off / norm, 0.0)
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), v, ratio


def quadric_matrix(sums):
    q = np.asarray(sums, dtype=F64)[:, 3:]
    return np.stack([np.stack([q[:, 0], q[:, 1], q[:, 2]], 1), np.stack([q[:, 1], q[:, 3], q[:, 4]], 1),
                     np.stack([q[:, 2], q[:, 4], q[:, 5]], 1)], axis=1)


def place(cells, counts, sums, lo, h, dims, placement="quadric", sweeps=JACOBI_SWEEPS):
    """(vertices float32 [C, 3], fell back bool [C], diagnostics) of the occupied cells.  diagnostics: eigenvalue
    ratios lambda_i / lambda_max [C, 3] (NaN where A = 0), kept eigenvalues per cell and the Jacobi residue."""
    cells = np.asarray(cells, dtype=np.int64)
    n = np.asarray(counts, dtype=F64)
    sums = np.asarray(sums, dtype=F64)
    x0 = np.stack([sums[:, 0] / n, sums[:, 1] / n, sums[:, 2] / n], axis=1)
    fell = np.zeros(len(cells), bool)
    if placement == "mean":
        return x0.astype(F32), fell, {}
    if placement != "quadric":
        raise ValueError(f"unknown placement {placement!r}")
    a = quadric_matrix(sums)
    r = np.stack([sums[:, 9 + i] - ((a[:, i, 0] * x0[:, 0] + a[:, i, 1] * x0[:, 1]) + a[:, i, 2] * x0[:, 2])
                  for i in range(3)], axis=1)
    lam, v, residue = jacobi(a, sweeps)
    lmax = np.maximum(np.maximum(lam[:, 0], lam[:, 1]), lam[:, 2])
    solve = lmax > 0
    cut = RANK_THRESHOLD * lmax
    x = x0.copy()
    rank = np.zeros(len(cells), np.int64)
    with np.errstate(all="ignore"):
        for i in range(3):
            keep = solve & (lam[:, i] > cut)
            g = ((v[:, 0, i] * r[:, 0] + v[:, 1, i] * r[:, 1]) + v[:, 2, i] * r[:, 2]) / lam[:, i]
            for k in range(3):
                x[:, k] = np.where(keep, x[:, k] + v[:, k, i] * g, x[:, k])
            rank += keep
        ratios = np.where(solve[:, None], lam / lmax[:, None], np.nan)
    cz, cy, cx = cells % dims[2], (cells // dims[2]) % dims[1], cells // (dims[2] * dims[1])
    lo64 = np.asarray(lo, dtype=F32).astype(F64)
    centre = np.stack([lo64[k] + (c.astype(F64) + 0.5) * h for k, c in enumerate((cx, cy, cz))], axis=1)
    with np.errstate(invalid="ignore"):
        ok = (np.isfinite(x) & (np.abs(x - centre) <= h)).all(axis=1)
    fell = solve & ~ok
    x[fell] = x0[fell]
    return x.astype(F32), fell, dict(ratios=ratios, rank=rank, residue=residue, solved=solve)


def cell_colors(col_sums, counts):
    """uint8 [C, 3]: floor(sum / count + 0.5) = (2 sum + count) // (2 count)."""
    n = np.asarray(counts, dtype=np.int64)[:, None]
    return np.clip((2 * np.asarray(col_sums, dtype=np.int64) + n) // (2 * n), 0, 255).astype(np.uint8)


def count_flipped(tris, src, verts, faces):
    """Output faces whose float64 normal has a negative dot product with their input triangle's."""
    if len(faces) == 0:
        return 0
    v = np.asarray(tris, dtype=F32).reshape(-1, 3, 3)[src].astype(F64)
    n_in = tri_normals(v[:, 0], v[:, 1], v[:, 2])
    o = np.asarray(verts, dtype=F32)[np.asarray(faces)].astype(F64)
    n_out = tri_normals(o[:, 0], o[:, 1], o[:, 2])
    dot = (n_in[0] * n_out[0] + n_in[1] * n_out[1]) + n_in[2] * n_out[2]
    return int((dot < 0).sum())


# ------------------------------------------------------------- the whole ----

def bisect_cells(count, target, hi=MAX_TARGET_CELLS):
    """The search of learn_nerf.simplify for target_faces: the last N the bisection reaches with count(N) <= target."""
    lo = 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if count(mid) <= target:
            lo = mid
        else:
            hi = mid - 1
    return lo


def simplify(tris, colors=None, cell_size=None, grid=None, target_faces=None, placement="quadric", origin=None,
             sweeps=JACOBI_SWEEPS):
    """The restated pipeline on a triangle soup [F, 3, 3] (colours uint8 [3F, 3] per corner): a dict of verts float32
    [V, 3], faces int64 [V, 3], colors uint8 [V, 3] or None, info, and the intermediate arrays the tests compare."""
    tris = np.ascontiguousarray(np.asarray(tris, dtype=F32).reshape(-1, 3, 3))
    pts = tris.reshape(-1, 3)
    lo = pts.min(axis=0) if origin is None else np.asarray(origin, dtype=F32)
    hi = pts.max(axis=0)
    if target_faces is not None:
        def count(n):
            _, inv, d = make_grid(lo, hi, cells=n)
            return int(survivors(cell_keys(pts, lo, inv, d)).sum())

        grid = bisect_cells(count, int(target_faces))
    h, inv_h, dims = make_grid(lo, hi, cell_size=cell_size, cells=grid)
    keys = cell_keys(pts, lo, inv_h, dims)
    face_keys, src, dups = output_faces(keys)
    cells, counts, sums, col = accumulate(tris, keys, colors)
    verts, fell, diag = place(cells, counts, sums, lo, h, dims, placement, sweeps)
    used = np.unique(face_keys)
    slot = np.searchsorted(cells, used)
    out_verts = verts[slot]
    faces = np.searchsorted(used, face_keys).reshape(-1, 3)
    info = dict(grid=tuple(dims), h=h, occupied_cells=len(cells), input_faces=len(tris), output_faces=len(faces),
                duplicates_removed=dups, fallback_cells=int(fell[slot].sum()),
                flipped=count_flipped(tris, src, out_verts, faces))
    return dict(verts=out_verts, faces=faces, colors=None if col is None else cell_colors(col, counts)[slot],
                info=info, keys=keys, cells=cells, counts=counts, sums=sums, col_sums=col, cell_verts=verts,
                fell_back=fell, diag=diag, slot=slot, src=src, lo=lo, inv_h=inv_h, dims=dims, n_cells=grid)


# ---------------------------------------------------------------- meshes ----

def cube_mesh(n=24, half=0.5):
    """(verts float32 [V, 3], faces int64 [12 n^2, 3]) of the cube [-half, half]^3, each face cut into n x n quads of
    two triangles, outward, the vertices shared (indexed)."""
    line = -half + (2 * half) * np.arange(n + 1, dtype=F64) / n
    index, verts, faces = {}, [], []

    def vid(p):
        key = tuple(np.round(np.asarray(p) * 4 * n).astype(np.int64))
        if key not in index:
            index[key] = len(verts)
            verts.append(p)
        return index[key]

    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (-1, 1):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[u], p[v] = side * half, line[i + di], line[j + dj]
                        quad.append(vid(p))
                    if side < 0:
                        quad = quad[::-1]
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return np.asarray(verts, dtype=F32), np.asarray(faces, dtype=np.int64)


def fan(length, seed=0):
    """A soup for the grid with origin 0, h = 1 and 2 x 2 x 2 cells whose cell 0 holds exactly `length` corners:
    `length` // 3 triangles inside it, the remaining corners on one more triangle whose other corners lie in cell 7, and
    two triangles that span several cells."""
    rng = np.random.default_rng(seed)
    full, rest = divmod(length, 3)
    tris = [rng.uniform(0.05, 0.95, size=(full, 3, 3))]
    if rest:
        extra = rng.uniform(1.05, 1.95, size=(1, 3, 3))
        extra[0, :rest] = rng.uniform(0.05, 0.95, size=(rest, 3))
        tris.append(extra)
    tris.append(np.array([[[1.5, 0.25, 0.5], [0.25, 1.5, 1.75], [1.25, 1.5, 0.5]],
                          [[1.9, 1.9, 1.9], [1.2, 0.7, 1.3], [0.5, 1.25, 0.75]]]))
    return np.concatenate(tris).astype(F32)

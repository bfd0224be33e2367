"""
NumPy restatement of the marching cubes of csrc/mesh.hip (the conventions are in that file's header comment), with a
case-table generator of its own: the face walks come from the cube's geometry here, not from a list.  Plus the mesh
measures the tests use (closure, Euler characteristic, components, signed volume) and the reference's grid.
"""
from collections import Counter

import numpy as np

CORNER_XYZ = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], dtype=np.int64)


def edge_number(c0: int, c1: int) -> int:
    """Axis-major numbering: axis a, then the rank of the lower corner among the corners with bit a clear."""
    a = (c0 ^ c1).bit_length() - 1
    lower = [c for c in range(8) if not (c >> a) & 1]
    return 4 * a + lower.index(min(c0, c1))


# per edge: its lower corner and its axis
EDGE_LO = np.zeros(12, dtype=np.int64)
EDGE_AXIS = np.zeros(12, dtype=np.int64)
for _a in range(3):
    for _c in range(8):
        if not (_c >> _a) & 1:
            _e = edge_number(_c, _c | 1 << _a)
            EDGE_LO[_e], EDGE_AXIS[_e] = _c, _a


def face_walks():
    """The 6 cube faces as corner cycles, counter-clockwise seen from outside (checked with the outward normal)."""
    walks = []
    for a in range(3):
        u, v = [b for b in range(3) if b != a]
        for side in (0, 1):
            cyc = [side << a | x << u | y << v for x, y in ((0, 0), (1, 0), (1, 1), (0, 1))]
            p = CORNER_XYZ[cyc]
            normal = np.zeros(3, dtype=np.int64)
            normal[a] = 1 if side else -1
            if np.dot(np.cross(p[1] - p[0], p[2] - p[1]), normal) < 0:
                cyc = cyc[::-1]
            walks.append(cyc)
    return walks


def case_table() -> np.ndarray:
    """[256, 16] int8: triangles as edge triples, -1 terminated."""
    walks = face_walks()
    table = np.full((256, 16), -1, dtype=np.int8)
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        succ = {}
        for w in walks:
            steps = [(w[s], w[(s + 1) % 4]) for s in range(4)]
            crossing = [inside[x] != inside[y] for x, y in steps]
            for s, (x, y) in enumerate(steps):
                if inside[x] or not inside[y]:
                    continue  # not where the walk enters a run of inside corners
                t = next((s + d) % 4 for d in range(1, 4) if crossing[(s + d) % 4])
                assert edge_number(x, y) not in succ
                succ[edge_number(x, y)] = edge_number(*steps[t])
        tris, done = [], set()
        for start in sorted(succ):
            if start in done:
                continue
            loop = [start]
            while succ[loop[-1]] != start:
                loop.append(succ[loop[-1]])
            done.update(loop)
            tris += [(loop[0], loop[k], loop[k + 1]) for k in range(1, len(loop) - 1)]
        flat = [e for tri in tris for e in tri]
        assert len(flat) <= 15
        table[case, :len(flat)] = flat
    return table


TABLE = case_table()
NTRI = (TABLE >= 0).sum(axis=1) // 3


def marching_cubes(vol, level):
    """-> verts [V, 3] float32 (index space), faces [F, 3] int32, in the order of csrc/mesh.hip."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    level = np.float32(level)
    nx, ny, nz = vol.shape
    inside = vol > level
    cross = np.zeros(vol.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    owned = cross.reshape(-1)  # (p, axis) order
    ids = np.full(owned.shape, -1, dtype=np.int32)
    ids[owned] = np.arange(int(owned.sum()), dtype=np.int32)
    ids = ids.reshape(cross.shape)

    which = np.nonzero(owned)[0]
    p, axis = which // 3, which % 3
    verts = np.stack(np.unravel_index(p, vol.shape), axis=1).astype(np.float32)
    flat = vol.reshape(-1)
    v0 = flat[p]
    v1 = flat[p + np.array([ny * nz, nz, 1])[axis]]
    rows = np.arange(len(p))
    with np.errstate(divide="ignore", invalid="ignore"):
        verts[rows, axis] = verts[rows, axis] + (level - v0) / (v1 - v0)

    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int32)
    for c in range(8):
        dx, dy, dz = CORNER_XYZ[c]
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int32) << c
    case = case.reshape(-1)
    cells = np.nonzero(NTRI[case] > 0)[0]
    tris = TABLE[case[cells], :15].reshape(-1, 5, 3).astype(np.int64)
    row, slot = np.nonzero(tris[:, :, 0] >= 0)  # cell order, then table order
    edges = tris[row, slot]
    ci, cj, ck = np.unravel_index(cells[row], (nx - 1, ny - 1, nz - 1))
    lo = EDGE_LO[edges]
    faces = ids[ci[:, None] + CORNER_XYZ[lo, 0], cj[:, None] + CORNER_XYZ[lo, 1], ck[:, None] + CORNER_XYZ[lo, 2],
                EDGE_AXIS[edges]]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32).reshape(-1, 3)


def grid_coordinates(bbox_min, bbox_max, resolution) -> np.ndarray:
    """The reference's grid (scripts/marching_cubes.py:86-95) as the float32 its model sees, [R^3, 3]."""
    axes = [np.linspace(lo, hi, num=resolution, dtype=np.float64).astype(np.float32)
            for lo, hi in zip(bbox_min, bbox_max)]
    g = np.meshgrid(*axes, indexing="ij")
    return np.stack(g, axis=-1).reshape(-1, 3)


# ---- a default-shape NeRFModel with a known surface -----------------------------------------------------------
# sigma = softplus(C * (cos x + cos y + cos z) - B): unit 0 of every hidden layer carries C * sum cos + B0 (B0 keeps it
# positive through the ReLUs), fed by the cos(2^0 x_c) slots (columns 20c + 10) of the 10-frequency embedding.
ANALYTIC_C, ANALYTIC_K, ANALYTIC_B0 = 4.0, 2.7, 12.0


def analytic_level_offset(threshold: float = 0.9) -> float:
    """B such that occupancy 1 - exp(-sigma) = threshold exactly where sum cos = ANALYTIC_K."""
    sigma = -np.log1p(-threshold)
    return ANALYTIC_C * ANALYTIC_K - np.log(np.expm1(sigma))


def set_analytic_nerf(tree, threshold: float = 0.9) -> None:
    """Overwrite a default NeRFModel parameter tree (Dense_0..11) in place."""
    for layer in tree.values():
        for leaf in layer.values():
            leaf.zero_()
    for c in range(3):
        tree["Dense_0"]["kernel"][20 * c + 10, 0] = ANALYTIC_C
    tree["Dense_0"]["bias"][0] = ANALYTIC_B0
    for i in range(1, 10):
        tree[f"Dense_{i}"]["kernel"][0, 0] = 1.0
    tree["Dense_9"]["bias"][0] = -(ANALYTIC_B0 + analytic_level_offset(threshold))


def analytic_volume(k: float = ANALYTIC_K, n: int = 4000) -> float:
    """Volume of {cos x + cos y + cos z > k} in [-1, 1]^3 (k > 1 + 2 cos 1: the set lies inside the box), midpoint
    rule over (x, y) of the exact z extent."""
    x = (np.arange(n) + 0.5) / n * 2 - 1
    a = k - np.cos(x)[:, None] - np.cos(x)[None, :]
    extent = np.where(a < 1, 2 * np.arccos(np.clip(a, -1, 1)), 0.0)
    return float(np.minimum(extent, 2.0).sum() * (2 / n) ** 2)


# ---- mesh measures ----------------------------------------------------------------------------------------------
def directed_edges(faces) -> np.ndarray:
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces) -> bool:
    """Every directed edge occurs exactly once and its reverse exactly once (a closed, oriented 2-manifold)."""
    e = directed_edges(faces)
    if len(e) == 0:
        return True
    base = int(e.max()) + 1
    keys = e[:, 0] * base + e[:, 1]
    if len(np.unique(keys)) != len(keys):
        return False
    return bool(np.isin(e[:, 1] * base + e[:, 0], keys).all())


def is_balanced(faces) -> bool:
    """Every directed edge occurs as often as its reverse: closed and consistently oriented, also where an edge is
    shared by four triangles (the fan diagonals of two neighbouring cells can meet on their common face)."""
    count = Counter(map(tuple, directed_edges(faces).tolist()))
    return all(count[(b, a)] == n for (a, b), n in count.items())


def euler_characteristic(verts, faces) -> int:
    e = directed_edges(faces)
    undirected = np.unique(np.sort(e, axis=1), axis=0)
    used = np.unique(np.asarray(faces).reshape(-1))
    return len(used) - len(undirected) + len(faces)


def components(faces) -> int:
    f = np.asarray(faces, dtype=np.int64)
    if len(f) == 0:
        return 0
    parent = np.arange(int(f.max()) + 1)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in directed_edges(f):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    return len({find(v) for v in np.unique(f)})


def signed_volume(verts, faces) -> float:
    t = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)

"""
NumPy restatement of the connected-component kernels (csrc/components.hip): labels in the convention of that file's
header comment (the smallest linear index of the component, -1 for background), sizes at the root indices and the keep
mask with the order (size descending, label ascending); the checker the GPU tests use, with seeded mutations it must
reject (tests/test_components_cpu.py); and the generators of the test volumes.
"""
import numpy as np

TILE = 8  # csrc/components.hip kTile
MUTATIONS = ("not_minimum", "faces_only", "size_off_by_one", "tie_to_higher_label", "unflattened")


def offsets(connectivity: int):
    assert connectivity in (6, 26), connectivity
    out = []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for dk in (-1, 0, 1):
                if (di, dj, dk) != (0, 0, 0) and (connectivity == 26 or abs(di) + abs(dj) + abs(dk) == 1):
                    out.append((di, dj, dk))
    return out


def label(mask, connectivity: int = 26) -> np.ndarray:
    """int32 labels, the shape of mask: breadth-first search from every unlabelled foreground cell in raster order, so
    the seed of a component is its smallest linear index."""
    fg = np.asarray(mask) != 0
    nx, ny, nz = fg.shape
    out = np.full(fg.shape, -1, dtype=np.int32)
    steps = offsets(connectivity)
    for seed in np.flatnonzero(fg):
        i, j, k = np.unravel_index(seed, fg.shape)
        if out[i, j, k] >= 0:
            continue
        out[i, j, k] = seed
        queue = [(int(i), int(j), int(k))]
        while queue:
            a, b, c = queue.pop()
            for da, db, dc in steps:
                x, y, z = a + da, b + db, c + dc
                if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and fg[x, y, z] and out[x, y, z] < 0:
                    out[x, y, z] = seed
                    queue.append((x, y, z))
    return out


def sizes(labels) -> np.ndarray:
    """int32, the shape of labels: the cell count of each component at its root index, 0 elsewhere."""
    flat = np.asarray(labels).reshape(-1)
    count = np.bincount(flat[flat >= 0], minlength=flat.size).astype(np.int32)
    return count.reshape(np.asarray(labels).shape)


def ranked(size_array, mutate=None):
    """[(label, size)] of the components in the order (size descending, label ascending)."""
    flat = np.asarray(size_array).reshape(-1)
    roots = np.flatnonzero(flat)
    sign = -1 if mutate == "tie_to_higher_label" else 1
    return sorted(((int(r), int(flat[r])) for r in roots), key=lambda c: (-c[1], sign * c[0]))


def keep(labels, size_array, min_cells: int = 1, keep_largest=None, mutate=None) -> np.ndarray:
    """uint8 keep mask, the shape of labels."""
    order = ranked(size_array, mutate)
    if keep_largest is not None:
        order = order[:keep_largest]
    chosen = np.array([r for r, s in order if s >= min_cells], dtype=np.int64)
    return (np.isin(labels, chosen) & (np.asarray(labels) >= 0)).astype(np.uint8)


def reference(mask, connectivity: int = 26, mutate=None):
    """(labels, sizes) of the restatement, with one seeded defect when `mutate` names it."""
    lab = label(mask, 6 if mutate == "faces_only" else connectivity)
    size = sizes(lab)
    if mutate == "not_minimum":  # the largest member of the first component with two cells or more, not the smallest
        root = next(r for r, s in ranked(size) if s > 1)
        members = np.flatnonzero(lab.reshape(-1) == root)
        lab = np.where(lab == root, np.int32(members[-1]), lab)
        size = sizes(lab)
    if mutate == "unflattened":  # the last member of such a component points at another member, not at the root
        root = next(r for r, s in ranked(size) if s > 2)
        members = np.flatnonzero(lab.reshape(-1) == root)
        lab = lab.copy()
        lab.reshape(-1)[members[-1]] = members[1]
    if mutate == "size_off_by_one":
        size = size.copy()
        size.reshape(-1)[np.flatnonzero(size)[0]] += 1
    return lab, size


def check(mask, connectivity: int, labels, size_array) -> None:
    """Raises AssertionError unless (labels, size_array) is THE labelling of mask in the convention.  Independent of
    label(): it checks the defining properties."""
    fg = np.asarray(mask) != 0
    lab = np.asarray(labels)
    flat = lab.reshape(-1)
    assert lab.shape == fg.shape and lab.dtype == np.int32
    assert ((lab >= 0) == fg).all(), "background must be -1 and foreground >= 0"
    cells = np.flatnonzero(fg)
    assert (flat[cells] <= cells).all(), "a label above its own cell"
    assert (flat[flat[cells]] == flat[cells]).all(), "unflattened label"
    # neighbours agree (no component is split) ...
    nx, ny, nz = fg.shape
    for di, dj, dk in offsets(connectivity):
        src, dst = _shifted(fg.shape, di, dj, dk)
        both = fg[src] & fg[dst]
        assert (lab[src][both] == lab[dst][both]).all(), "two neighbours with different labels"
    # ... and every label class is connected to the cell it names, which is a member labelled with itself (no two
    # components are joined); with label <= cell for every member, that cell is the class's minimum
    assert _reaches_root(fg, lab, connectivity), "a label class that is not connected to its root"
    assert np.array_equal(np.asarray(size_array), sizes(lab)), "sizes"
    assert np.asarray(size_array).dtype == np.int32


def _shifted(shape, *step):
    """(src, dst) slices of the cell pairs (c, c + step) that lie inside a volume of `shape`."""
    src = tuple(slice(max(0, -d), n - max(0, d)) for n, d in zip(shape, step))
    dst = tuple(slice(max(0, d), n - max(0, -d)) for n, d in zip(shape, step))
    return src, dst


def _reaches_root(fg, lab, connectivity) -> bool:
    """Every foreground cell is joined to the cell its label names by a path inside its label class."""
    seen = np.zeros(fg.shape, bool)
    flat_seen = seen.reshape(-1)
    roots = np.unique(lab[fg])
    if roots.size == 0:
        return True
    if not fg.reshape(-1)[roots].all() or not (lab.reshape(-1)[roots] == roots).all():
        return False
    flat_seen[roots] = True
    nx, ny, nz = fg.shape
    steps = offsets(connectivity)
    while True:  # grow every class from its root, one ring per sweep
        grown = seen.copy()
        for di, dj, dk in steps:
            src, dst = _shifted(fg.shape, di, dj, dk)
            grown[dst] |= seen[src] & fg[dst] & (lab[src] == lab[dst])
        if (grown == seen).all():
            return bool((seen == fg).all())
        seen = grown


# ------------------------------------------------------------------------------------------------- generators
def random_mask(shape, p: float, seed: int) -> np.ndarray:
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def runs(n: int = 70) -> np.ndarray:
    """(1, 1, n): runs of 1, 2, 3, ... foreground cells separated by single background cells."""
    line = np.zeros(n, np.uint8)
    at, length = 0, 1
    while at < n:
        line[at:at + length] = 1
        at += length + 1
        length += 1
    return line.reshape(1, 1, n)


def checkerboard(shape=(9, 10, 11)) -> np.ndarray:
    i, j, k = np.indices(shape)
    return ((i + j + k) % 2 == 0).astype(np.uint8)


def two_blocks(touch: str) -> np.ndarray:
    """Two 3^3 blocks that touch only at a corner, or only along an edge."""
    m = np.zeros((7, 7, 7), np.uint8)
    m[0:3, 0:3, 0:3] = 1
    if touch == "corner":
        m[3:6, 3:6, 3:6] = 1
    else:
        m[3:6, 3:6, 0:3] = 1
    return m


def serpentine(n: int = 33) -> np.ndarray:
    """One 6-connected path of width 1 through every second layer and every second row of (n, n, n), boustrophedon:
    row j of layer i runs along k, a single cell in the row between joins two rows at alternating ends, and a single
    cell in the layer between joins two layers.  Its smallest index, cell (0, 0, 0), is one end of the path."""
    assert n % 2 == 1
    m = np.zeros((n, n, n), np.uint8)
    end = 0  # the k at which the path leaves the current row
    rows = list(range(0, n, 2))
    for li, i in enumerate(range(0, n, 2)):
        order = rows if li % 2 == 0 else rows[::-1]
        for pos, j in enumerate(order):
            m[i, j, :] = 1
            end = n - 1 - end  # the row is walked from `end` to the other side
            if pos + 1 < len(order):
                m[i, (j + order[pos + 1]) // 2, end] = 1
        if i + 2 < n:
            m[i + 1, order[-1], end] = 1
    return m


def tie_mask() -> np.ndarray:
    """Two components of 4 cells (labels 0 and 110: the order puts 0 first), one of 2 cells and one of 1."""
    m = np.zeros((9, 5, 5), np.uint8)
    m[0, 0, 0:4] = 1
    m[4, 2, 0:4] = 1
    m[8, 4, 0:2] = 1
    m[8, 0, 4] = 1
    return m


def blobs_volume(n: int = 20) -> np.ndarray:
    """float32 occupancy [n, n, n] in [0, 1): one large smooth blob, two small ones apart from it and one small blob
    whose only contact with the large one is diagonal (a corner) at the level 0.5."""
    vol = np.zeros((n, n, n), np.float32)
    i, j, k = np.indices(vol.shape).astype(np.float32)
    ball = 1.0 - ((i - 7) ** 2 + (j - 7) ** 2 + (k - 7) ** 2) / 30.0
    vol = np.maximum(vol, np.clip(ball, 0, 0.95)).astype(np.float32)
    inside = vol > 0.5
    vol[15:17, 15:17, 3:5] = 0.9
    vol[3, 16, 16] = 0.8
    # the corner blob: find a foreground cell whose (+1, +1, +1) neighbour and the three face neighbours on the way
    # are background, and start a 2^3 block there
    for a, b, c in np.argwhere(inside)[::-1]:
        block = (slice(a + 1, a + 3), slice(b + 1, b + 3), slice(c + 1, c + 3))
        shell = inside[a:a + 4, b:b + 4, c:c + 4].sum()
        if shell == 1 and max(a, b, c) + 3 < n:
            vol[block] = 0.7
            break
    else:
        raise AssertionError("no free corner on the large blob")
    return vol

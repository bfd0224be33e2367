"""
Mesh simplification without a GPU: properties of the NumPy restatement (tests/simplify_reference.py) that the GPU
tests then hold the kernels to, and the host logic of learn_nerf.simplify (grid rule, bisection, validation).

The cube: [-0.5, 0.5]^3, each face cut into 24 x 24 quads (6912 triangles), on the grid with h = 0.25 and origin
-0.625, so that the cube's faces, edges and corners sit in the middle of their cells.  Vertex clustering with quadric
placement must then return the cube exactly: a cell that meets one face holds rank-1 quadrics and its vertex stays in
the plane, a cell on an edge has rank 2 and lands on the edge, and the eight corner cells have rank 3 and return the
corners.  The mean placement cannot: it pulls the vertices of edge and corner cells inwards by O(h).

Cell walls.  The mesh vertices are -0.5 + i / 24, i.e. (i / 6 + 0.5) cells from the origin: for i = 3, 9, 15, 21 that is
a whole number and the vertex lies ON a wall.  Those coordinates (-0.375, -0.125, 0.125, 0.375), the origin and 1 / h = 4
are dyadic, so the float32 cell rule is exact there and the vertex belongs to the upper cell without any rounding being
involved; every other vertex is at least 1/6 of a cell from a wall.  The condition asserted below is therefore: a corner
is either exactly on a wall in exact arithmetic or at least 0.1 h away from one, and the cube's own faces and corners
are half a cell away.
"""
import math

import numpy as np
import pytest

import simplify_reference as S
from raycast_reference import icosphere

H, ORIGIN = 0.25, (-0.625, -0.625, -0.625)


@pytest.fixture(scope="module")
def cube():
    verts, faces = S.cube_mesh(24)
    assert len(faces) == 6912
    tris = verts[faces]
    return verts, faces, tris, S.simplify(tris, cell_size=H, origin=ORIGIN), \
        S.simplify(tris, cell_size=H, origin=ORIGIN, placement="mean")


def on_cube_error(points):
    """Distance in the max norm of each point to the surface of the cube [-0.5, 0.5]^3 (points inside or on it)."""
    p = np.abs(np.asarray(points, dtype=np.float64))
    outside = np.maximum(p - 0.5, 0).max(axis=1)
    return np.maximum(outside, np.abs(p.max(axis=1) - 0.5))


def face_plane_error(tris, result):
    """Largest distance of an output triangle's vertices from the face plane of its input triangle."""
    src = tris[result["src"]].astype(np.float64)
    axis = np.argmax(np.abs(np.cross(src[:, 1] - src[:, 0], src[:, 2] - src[:, 0])), axis=1)
    level = src[np.arange(len(src)), 0, axis]
    out = result["verts"][result["faces"]].astype(np.float64)
    return np.abs(out[np.arange(len(src)), :, axis] - level[:, None]).max()


def test_cube_conditions(cube):
    verts, _, tris, quad, _ = cube
    assert quad["dims"] == [5, 5, 5] and quad["info"]["h"] == H
    wall = S.wall_distance(verts, ORIGIN, H)
    assert ((wall == 0) | (wall >= 0.1)).all() and (wall == 0).any()  # docstring: exact hits or a wide margin
    assert np.allclose(S.wall_distance([[0.5, -0.5, 0.5]], ORIGIN, H), 0.5)
    ratios = quad["diag"]["ratios"]
    assert np.isfinite(ratios).all()
    assert not ((ratios > 0.5e-3) & (ratios < 2e-3)).any()  # no rank decision within a factor 2 of the threshold
    assert not quad["fell_back"].any() and quad["info"]["fallback_cells"] == 0
    assert quad["diag"]["residue"].max() <= 1e-15


def test_cube_quadric_placement_returns_the_cube(cube):
    _, _, tris, quad, _ = cube
    info = quad["info"]
    assert info["occupied_cells"] == 98 and len(quad["verts"]) == 98  # the surface cells of 5^3
    assert info["input_faces"] == 6912 and 0 < info["output_faces"] < 6912
    assert info["flipped"] == 0
    # fp64 placement rounded to fp32: half an ulp of coordinates up to 0.5 is 2^-25
    assert on_cube_error(quad["verts"]).max() <= 2.0**-24
    corners = quad["cell_verts"][np.isin(quad["cells"], [(x * 5 + y) * 5 + z for x in (0, 4) for y in (0, 4)
                                                          for z in (0, 4)])]
    assert len(corners) == 8 and np.array_equal(np.abs(corners), np.full((8, 3), 0.5, np.float32))
    assert face_plane_error(tris, quad) <= 2.0**-24
    rank = quad["diag"]["rank"]
    assert sorted(np.unique(rank)) == [1, 2, 3] and (rank == 3).sum() == 8 and (rank == 2).sum() == 36


def test_cube_mean_placement_misses_by_a_fraction_of_h(cube):
    _, _, tris, _, mean = cube
    assert on_cube_error(mean["verts"]).max() > 0.1 * H
    assert face_plane_error(tris, mean) > 0.1 * H
    corner = mean["cell_verts"][mean["cells"] == 0][0]
    assert np.abs(np.abs(corner) - 0.5).max() > 0.1 * H


def test_indexed_mesh_and_soup_agree_and_faces_are_consistent(cube):
    verts, faces, tris, quad, _ = cube
    # the restatement is defined on corners: an indexed mesh is its soup, and a soup whose copies of a vertex are
    # separate arrays gives the same bits (the GPU test feeds learn_nerf.simplify both forms)
    soup = np.stack([verts[faces[:, k]].copy() for k in range(3)], axis=1)
    again = S.simplify(soup, cell_size=H, origin=ORIGIN)
    for name in ("verts", "faces", "sums", "keys"):
        assert np.array_equal(quad[name], again[name]), name
    f = quad["faces"]
    assert f.min() == 0 and f.max() == len(quad["verts"]) - 1
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    canon = {min((a, b, c), (b, c, a), (c, a, b)) for a, b, c in f.tolist()}
    assert len(canon) == len(f)
    # duplicates: two triangles over the same three cells, one of them rotated; opposite winding is kept
    t = np.array([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1]], np.float32)
    soup = np.stack([t, t[[1, 2, 0]] + np.float32(0.05), t[[0, 2, 1]], t + np.float32(0.1)])
    out = S.simplify(soup, cell_size=1.0, origin=(0, 0, 0))
    assert out["info"]["duplicates_removed"] == 2 and out["src"].tolist() == [0, 2]
    assert out["faces"].tolist() == [[0, 2, 1], [0, 1, 2]]


def test_planar_patch_stays_in_its_plane_with_rank_one():
    n = 12
    u, v = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n, indexing="ij")
    normal = np.array([1.0, 2.0, 2.0]) / 3.0
    e1, e2 = np.array([2.0, -1.0, 0.0]) / math.sqrt(5), np.cross(normal, np.array([2.0, -1.0, 0.0]) / math.sqrt(5))
    grid = (0.3 * normal + u[..., None] * e1 + v[..., None] * e2).astype(np.float32)
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    faces = np.concatenate([np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:]], -1).reshape(-1, 3),
                            np.stack([idx[:-1, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 3)])
    out = S.simplify(grid.reshape(-1, 3)[faces], cell_size=0.21)
    assert out["info"]["output_faces"] > 4 and (out["diag"]["rank"] == 1).all()
    # the fp32 vertices are off the plane by their own rounding (2^-24 relative to coordinates below 2), and so is
    # the plane the quadrics see; the placement adds the fp32 rounding of its result
    dist = np.abs(out["verts"].astype(np.float64) @ normal - 0.3)
    assert dist.max() <= 4 * 2.0**-24 * 2
    assert out["info"]["flipped"] == 0 and not out["fell_back"].any()


def test_fold_order_is_fixed_and_not_a_plain_sum():
    rng = np.random.default_rng(3)
    u = rng.standard_normal((100, 2)) * 10.0 ** rng.integers(-8, 8, size=(100, 2))
    got = S.fold_segment(u)
    # by hand: chunk trees, then chunks in order
    padded = np.zeros((112, 2))
    padded[:100] = u
    acc = np.zeros(2)
    for m in range(7):
        c = padded[16 * m:16 * m + 16]
        tree = (((c[0] + c[8]) + (c[4] + c[12])) + ((c[2] + c[10]) + (c[6] + c[14]))) + \
               (((c[1] + c[9]) + (c[5] + c[13])) + ((c[3] + c[11]) + (c[7] + c[15])))
        acc = acc + tree
    assert np.array_equal(got, acc)
    assert not np.array_equal(got, np.cumsum(u, axis=0)[-1])  # the order matters on this input
    assert np.array_equal(S.fold_segment(u[:1]), u[0])


def test_quadric_counts_a_triangle_once_per_distinct_cell():
    tris = S.fan(7)
    lo, inv_h, dims = (0.0, 0.0, 0.0), np.float32(1.0), [2, 2, 2]
    keys = S.cell_keys(tris.reshape(-1, 3), lo, inv_h, dims)
    cells, counts, sums, _ = S.accumulate(tris, keys)
    assert counts[cells == 0][0] == 7
    q = S.tri_quadrics(tris)
    inside = S.fold_segment(np.concatenate([np.repeat(q[:2], 3, axis=0) * np.array([1, 0, 0] * 2)[:, None], q[2:3]]))
    assert np.array_equal(sums[cells == 0][0, 3:], inside)
    zero_area = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2]]], np.float32)
    assert not S.tri_quadrics(zero_area).any()


def test_jacobi_sweep_count_on_the_test_population():
    """DESIGN.md records 6 sweeps: on every cell of the cube, the icosphere, a random soup and on random symmetric
    matrices the off-diagonal mass is below 1e-15 of the norm from 4 sweeps on (3 do not reach it), so 6 keeps two in
    hand, and the eigen-pairs reproduce the matrix."""
    rng = np.random.default_rng(0)
    mats = [S.quadric_matrix(S.simplify(icosphere(3), grid=6)["sums"]),
            S.quadric_matrix(S.simplify(S.cube_mesh(24)[0][S.cube_mesh(24)[1]], cell_size=H, origin=ORIGIN)["sums"]),
            S.quadric_matrix(S.simplify(rng.uniform(-1, 1, (400, 3, 3)).astype(np.float32), grid=5)["sums"])]
    r = rng.standard_normal((2000, 3, 3))
    mats.append(r @ r.transpose(0, 2, 1) * 10.0 ** rng.integers(-6, 6, size=(2000, 1, 1)))
    a = np.concatenate(mats)
    lam, v, residue = S.jacobi(a, S.JACOBI_SWEEPS)
    assert residue.max() <= 1e-15
    rebuilt = np.einsum("cik,ck,cjk->cij", v, lam, v)
    scale = np.abs(a).max(axis=(1, 2))
    assert (np.abs(rebuilt - a).max(axis=(1, 2)) <= 1e-13 * scale).all()
    assert S.jacobi(a, 4)[2].max() <= 1e-15 < S.jacobi(a, 3)[2].max() and S.JACOBI_SWEEPS == 6


# ---------------------------------------------------------------- host ----

def test_host_grid_rule_matches_the_restatement_and_refuses_large_grids():
    from learn_nerf import simplify as M

    rng = np.random.default_rng(1)
    for _ in range(50):
        lo = rng.uniform(-3, 3, 3).astype(np.float32)
        hi = (lo + rng.uniform(0, 4, 3)).astype(np.float32)
        for kwargs in (dict(cell_size=float(rng.uniform(0.01, 1))), dict(cells=int(rng.integers(1, 300)))):
            got, want = M.choose_grid(lo, hi, **kwargs), S.make_grid(lo, hi, **kwargs)
            assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
            # large enough to hold the extent: the highest corner's cell exists
            assert (S.cell_coords([hi], lo, got[1], got[2]) < np.array(got[2])).all()
    h, inv_h, dims = M.choose_grid((0, 0, 0), (1, 1, 0.5), cells=7)
    assert dims[0] == 7 and dims[1] == 7 and 3 <= dims[2] <= 4 and h == 1 / 7
    assert M.choose_grid((0, 0, 0), (0, 0, 0), cell_size=1.0)[2] == [1, 1, 1]
    with pytest.raises(ValueError, match="2\\^31"):
        M.choose_grid((0, 0, 0), (1, 1, 1), cell_size=1e-4)  # 10^12 cells
    with pytest.raises(ValueError, match="2\\^31"):
        M.choose_grid((0, 0, 0), (1, 1, 1), cell_size=1e-12)
    assert math.prod(M.choose_grid((0, 0, 0), (1, 1, 1), cell_size=1 / 1200)[2]) < 2**31
    with pytest.raises(ValueError, match="extent"):
        M.choose_grid((1, 1, 1), (1, 1, 1), cells=4)
    with pytest.raises(ValueError):
        M.choose_grid((0, 0, 0), (1, 1, 1), cell_size=1e-60)


def test_bisection_with_a_stub_counter():
    from learn_nerf import simplify as M

    calls = []

    def monotone(n):
        calls.append(n)
        return 0 if n == 1 else 3 * n * n

    for target in (0, 11, 12, 500, 3 * 1024 * 1024, 10**9):
        calls.clear()
        n = M.bisect_cells(monotone, target)
        assert len(calls) == 10 and all(1 < c <= 1024 for c in calls)  # [1, 1024] halves ten times
        assert n == S.bisect_cells(monotone, target)
        assert monotone(n) <= target and (n == 1024 or monotone(n + 1) > target)

    # not monotone (a grid that lines up with the mesh can leave fewer survivors than a coarser one): the answer was
    # still tested, so it still holds
    rng = np.random.default_rng(5)
    noise = rng.integers(-400, 400, size=1025)

    def bumpy(n):
        return 0 if n == 1 else max(0, 3 * n * n + int(noise[n]))

    for target in (0, 50, 700, 5000, 123456):
        n = M.bisect_cells(bumpy, target)
        assert bumpy(n) <= target and n == S.bisect_cells(bumpy, target)
    assert M.bisect_cells(lambda n: 10, 5) == 1  # nothing fits: the caller then finds no faces


def test_argument_validation_needs_no_gpu():
    from learn_nerf import simplify as M

    tris = np.zeros((2, 3, 3), np.float32)
    for kwargs in (dict(), dict(cell_size=0.1, grid=4), dict(grid=4, target_faces=10),
                   dict(cell_size=0.1, grid=4, target_faces=10)):
        with pytest.raises(ValueError, match="exactly one"):
            M.simplify(tris, **kwargs)
    for kwargs in (dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=math.inf), dict(cell_size=math.nan),
                   dict(grid=0), dict(grid=2.5), dict(target_faces=0), dict(grid=4, placement="median"),
                   dict(grid=4, fold_shape="blocks")):
        with pytest.raises(ValueError):
            M.simplify(tris, **kwargs)
    with pytest.raises(ValueError, match="empty"):
        M.simplify(np.zeros((0, 3, 3), np.float32), grid=4)
    with pytest.raises(ValueError, match="empty"):
        M.simplify(np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int64), grid=4)
    with pytest.raises(ValueError, match="expected"):
        M.simplify(np.zeros((5, 3), np.float32), grid=4)
    lines = M.format_info(dict(grid=(5, 4, 3), h=0.25, flipped=0))
    assert lines == ["grid=5x4x3", "h=0.25", "flipped=0"]

"""
The neighbour search of csrc/pointcloud.hip (lnrf_pc_cell_ids / lnrf_pc_knn_dist2 / lnrf_pc_nearest) against the float32
brute force of tests/point_cloud_reference.py: every distance bit-identical and every index identical, whatever the cell
edge; then subsampling, the distance field and the properties of the meshes made from it.
"""
import numpy as np
import pytest
import torch

import mesh_reference as M
import point_cloud_reference as R

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_search(points, queries=None, ks=(1,), radii=(np.inf,), cell_edge=None):
    """knn_dist2 (queries default to the points) and nearest of a PointGrid equal the brute force bit for bit."""
    from learn_nerf.point_cloud import PointGrid

    points = np.ascontiguousarray(points, np.float32)
    queries = points if queries is None else np.ascontiguousarray(queries, np.float32)
    grid = PointGrid(cuda(points), cell_edge=cell_edge)
    assert all(1 <= g <= 4096 for g in grid.dims)
    for k in ks:
        got = grid.knn_dist2(cuda(queries), k).cpu().numpy()
        want = R.knn_dist2(points, queries, k)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (k, np.abs(got - want).max())
    for radius in radii:
        d2, idx = grid.nearest(cuda(queries), radius)
        want_d2, want_idx = R.nearest(points, queries, radius)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want_idx), radius
        assert np.array_equal(bits(d2.cpu().numpy()), bits(want_d2)), radius
    return grid


@pytest.fixture(scope="module")
def cloud5000():
    return np.random.default_rng(5).random((5000, 3), dtype=np.float32)


def test_tiny_clouds_and_copies():
    one = np.array([[0.25, -1.5, 3.0]], np.float32)
    grid = assert_search(one, ks=(1, 2))
    assert grid.dims == [1, 1, 1]
    assert grid.knn_dist2(cuda(one), 1).item() == 0.0 and grid.knn_dist2(cuda(one), 2).item() == np.inf
    three = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0.5]], np.float32)
    grid = assert_search(three, ks=(1, 3, 5))
    assert torch.isinf(grid.knn_dist2(cuda(three), 5)).all()
    copies = np.tile(np.array([[0.3, 0.7, -0.2]], np.float32), (100, 1))
    grid = assert_search(copies, queries=np.vstack([copies[:3], [[0.0, 0.0, 0.0]]]), ks=(1, 32))
    assert grid.dims == [1, 1, 1]
    _, idx = grid.nearest(cuda(copies[:1]))
    assert idx.item() == 0  # 100 equal distances: the lowest index


def test_lattice_on_cell_boundaries_and_upper_faces():
    g = np.arange(9, dtype=np.float32) * np.float32(0.25)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(0)
    lattice = lattice[rng.permutation(len(lattice))]
    queries = np.vstack([lattice, rng.random((200, 3), dtype=np.float32) * 2])
    for edge, dims in ((0.25, 9), (0.5, 5), (None, None)):
        grid = assert_search(lattice, queries, ks=(1, 5, 8), cell_edge=edge)
        if dims:  # the points with coordinate 2.0 lie on the grid's upper faces, in the last cell
            assert grid.dims == [dims] * 3
            ids = grid.cell_ids(cuda(lattice)).cpu().numpy()
            top = lattice[:, 2] == 2.0
            assert (ids[top] % dims == dims - 1).all() and ids.max() == dims ** 3 - 1 and ids.min() == 0
            assert grid.cell_start[-1].item() == len(lattice) and grid.cell_start[0].item() == 0


def test_search_crosses_an_empty_grid():
    a = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], np.float32)
    two = np.vstack([a, a + np.float32([1000, 0, 0])])
    grid = assert_search(two, ks=(1, 3, 5, 6), cell_edge=1.0)
    assert grid.dims == [1001, 1, 1]
    d = grid.knn_dist2(cuda(two), 5).cpu().numpy()
    assert (d > 999.0 ** 2).all() and np.isfinite(d).all()
    assert_search(two, queries=np.float32([[500, 0, 0], [499, 3, -2], [-50, 0, 0], [2000, 1, 1]]), ks=(1, 4, 6))
    spread = two * np.float32([1, 1, 0]) + np.float32([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 40, 30], [0, 40, 30],
                                                       [0, 40, 30]])
    grid = assert_search(spread, ks=(5,), cell_edge=1.0)  # the rings are clipped on three axes
    assert grid.dims == [1001, 41, 31]


def test_flat_cloud():
    flat = np.random.default_rng(1).random((2000, 3), dtype=np.float32)
    flat[:, 2] = 0
    grid = assert_search(flat, ks=(1, 5))
    assert grid.dims[2] == 1 and grid.dims[0] > 1
    line = flat * np.float32([1, 0, 0]) + np.float32([0, 2, -1])
    assert assert_search(line, ks=(5,)).dims[1:] == [1, 1]


def test_uniform_cloud_every_k_kernel(cloud5000):
    grid = assert_search(cloud5000, ks=(1, 2, 4, 5, 8, 9, 16, 17, 32))
    assert min(grid.dims) > 4  # several rings of cells


def test_results_do_not_depend_on_the_cell_edge(cloud5000):
    from learn_nerf.point_cloud import PointGrid

    queries = cuda(np.random.default_rng(6).random((3000, 3), dtype=np.float32) * 1.5 - 0.25)
    results = []
    for edge in (0.013, 0.21, None):
        grid = PointGrid(cuda(cloud5000), cell_edge=edge)
        results.append((grid.knn_dist2(queries, 5), *grid.nearest(queries), *grid.nearest(queries, 0.05)))
    assert PointGrid(cuda(cloud5000), cell_edge=0.013).dims != PointGrid(cuda(cloud5000), cell_edge=0.21).dims
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want = R.knn_dist2(cloud5000, queries.cpu().numpy(), 5)
    assert np.array_equal(bits(results[0][0].cpu().numpy()), bits(want))


def torch_knn_dist2(points, k, chunk=1024):
    """Brute force on the GPU from elementwise ops, so that every operation rounds once (no cdist, no matmul)."""
    px, py, pz = (points[:, a].contiguous()[None, :] for a in range(3))
    out = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
    for s in range(0, points.shape[0], chunk):
        q = points[s:s + chunk]
        dx, dy, dz = q[:, 0:1] - px, q[:, 1:2] - py, q[:, 2:3] - pz
        d2 = (dx * dx + dy * dy) + dz * dz
        out[s:s + chunk] = torch.topk(d2, k, dim=1, largest=False).values[:, k - 1]
    return out


def test_large_cloud_spans_many_workgroups(cloud5000):
    from learn_nerf.point_cloud import knn_dist2

    small = cuda(cloud5000)
    assert np.array_equal(bits(torch_knn_dist2(small, 5).cpu().numpy()), bits(R.knn_dist2(cloud5000, cloud5000, 5)))
    points = cuda(np.random.default_rng(7).random((70001, 3), dtype=np.float32))
    got = knn_dist2(points, 5)
    assert torch.equal(got.view(torch.int32), torch_knn_dist2(points, 5).view(torch.int32))


def test_nearest_outside_the_box_beyond_the_radius_and_ties(cloud5000):
    rng = np.random.default_rng(8)
    outside = np.vstack([rng.random((500, 3), dtype=np.float32) * 6 - 2.5,  # mostly outside [0, 1]^3
                         np.float32([[-100, 0.5, 0.5], [0.5, 1e6, 0.5], [7, 7, 7], [1, 1, 1], [0, 0, 0]])])
    grid = assert_search(cloud5000, outside, radii=(np.inf, 0.5, 0.05, 0.0))
    d2, idx = grid.nearest(cuda(outside), 0.05)
    far = np.linalg.norm(np.maximum(np.maximum(-outside, outside - 1), 0), axis=1) > 0.06
    assert far.sum() > 300 and (idx.cpu().numpy()[far] == -1).all() and torch.isinf(d2[torch.from_numpy(far)]).all()
    assert (idx.cpu().numpy() >= 0).any()

    ties = np.float32([[0.25, 0, 0], [-0.25, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.25], [0, 0, -0.25]])
    extra = rng.random((50, 3), dtype=np.float32) * 4 - 2
    extra = extra[np.linalg.norm(extra, axis=1) > 0.5]
    for seed in range(4):
        pts = np.vstack([ties, extra])[np.random.default_rng(seed).permutation(6 + len(extra))]
        lowest = min(i for i, p in enumerate(pts) if np.abs(p).sum() == 0.25 and np.abs(p).max() == 0.25)
        for edge in (0.2, 0.3, None):
            grid = assert_search(pts, np.zeros((1, 3), np.float32), cell_edge=edge)
            d2, idx = grid.nearest(cuda(np.zeros((1, 3))))
            assert idx.item() == lowest and d2.item() == 0.0625


def test_unsupported_k_and_bad_arguments(cloud5000):
    import ctypes

    from learn_nerf import _lib as L
    from learn_nerf.point_cloud import PointGrid

    grid = PointGrid(cuda(cloud5000))
    with pytest.raises(RuntimeError, match="-3"):
        grid.knn_dist2(cuda(cloud5000[:4]), 33)
    q, out = cuda(cloud5000[:4]), torch.empty(4, device="cuda")
    args = (L.ptr(grid.sorted_points), L.ptr(grid.cell_start, torch.int32), grid.n, L.ptr(q), 4)
    lib = L.lib()
    assert lib.lnrf_pc_knn_dist2(ctypes.byref(grid.grid), *args, 33, L.ptr(out), L.stream()) == L.ERR_UNSUPPORTED
    assert b"32" in lib.lnrf_last_error()
    assert lib.lnrf_pc_knn_dist2(ctypes.byref(grid.grid), *args, 0, L.ptr(out), L.stream()) == -1
    too_many = (L.ptr(grid.sorted_points), L.ptr(grid.cell_start, torch.int32), 2 ** 31, L.ptr(q), 4)
    assert lib.lnrf_pc_knn_dist2(ctypes.byref(grid.grid), *too_many, 5, L.ptr(out), L.stream()) == -2
    bad = L.PcGrid((ctypes.c_float * 3)(0, 0, 0), 1.0, (ctypes.c_int32 * 3)(4097, 1, 1), 0)
    assert lib.lnrf_pc_knn_dist2(ctypes.byref(bad), *args, 5, L.ptr(out), L.stream()) == -2
    with pytest.raises(ValueError, match="non-finite"):
        PointGrid(cuda(np.float32([[0, 0, np.nan]])))
    with pytest.raises(ValueError, match="non-finite"):
        grid.nearest(cuda(np.float32([[0, np.inf, 0]])))
    with pytest.raises(ValueError, match="4096"):
        PointGrid(cuda(cloud5000), cell_edge=1e-5)


def test_subsample_keeps_the_densest_in_stable_order(cloud5000):
    from learn_nerf.point_cloud import subsample

    points = cloud5000.copy()
    points[1000:1200] = points[:200]  # exact duplicates: ties at distance 0 for k = 2
    colors = np.random.default_rng(9).random((5000, 3), dtype=np.float32)
    for k in (2, 5):
        keep = np.argsort(R.knn_dist2(points, points, k), kind="stable")[:1000]
        p, c = subsample(cuda(points), cuda(colors), 1000, sort_density=True, k=k)
        assert np.array_equal(p.cpu().numpy(), points[keep]) and np.array_equal(c.cpu().numpy(), colors[keep])


def test_field_equals_the_restatement_bit_for_bit():
    from learn_nerf.point_cloud import point_field

    points = np.random.default_rng(10).random((500, 3), dtype=np.float32) * np.float32(0.5)
    want = R.point_field(points, 0.05, 0.025)
    for batch in (5000, 1 << 22):
        volume, origin, dims = point_field(cuda(points), 0.05, 0.025, batch_size=batch)
        assert list(volume.shape) == dims == list(want.shape)
        assert np.array_equal(bits(volume.cpu().numpy()), bits(want))
    assert np.array_equal(origin, [a[0] for a in R.field_axes(points, 0.05, 0.025)])
    assert (want > 0).any() and (want == np.float32(0.05) - np.float32(0.05 + 0.025)).any()


def test_mesh_of_one_isolated_point():
    from learn_nerf.point_cloud import extract

    delta, point = 0.05, np.float32([[0.3, -0.2, 1.1]])
    thickness = 4 * delta
    verts, faces, colors = extract(cuda(point), cuda([[0.2, 0.4, 0.6]]), thickness, delta)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and len(faces) > 100
    assert M.is_closed_oriented(faces) and M.components(faces) == 1 and M.euler_characteristic(verts, faces) == 2
    assert M.signed_volume(verts, faces) > 0
    # the field is 1-Lipschitz, so the linear crossing on an edge of length delta is off by at most delta; fp32 slack
    dist = np.linalg.norm(verts.astype(np.float64) - point.astype(np.float64), axis=1)
    assert np.abs(dist - thickness).max() <= delta + 1e-5, np.abs(dist - thickness).max()
    assert np.array_equal(colors, np.tile(np.float32([[0.2, 0.4, 0.6]]), (len(verts), 1)))


def test_mesh_of_the_sphere_dataset(tmp_path):
    from learn_nerf.point_cloud import extract, read_dataset, subsample

    R.write_sphere_dataset(str(tmp_path), size=64, max_depth=4.0)
    points, colors, views = read_dataset(str(tmp_path), 4.0, "cuda")
    assert views == len(R.SPHERE_DIRECTIONS) and points.shape[0] > 4000 and points.is_cuda
    norm = points.double().norm(dim=1)
    assert (norm - R.SPHERE_RADIUS).abs().max().item() <= (4.0 / 65535) / 0.7746 + 1e-5  # the CPU test's bound
    points, colors = subsample(points, colors, 2000, sort_density=True, k=5)
    assert points.shape == (2000, 3)
    thickness, delta = 0.05, 0.025
    verts, faces, vertex_colors = extract(points, colors, thickness, delta)
    assert len(faces) > 1000 and M.is_balanced(faces) and M.signed_volume(verts, faces) > 0
    # distance of every vertex to its nearest kept point, float64 brute force
    v64, p64 = torch.from_numpy(verts).cuda().double(), points.double()
    nearest = torch.cat([(v64[s:s + 4096, None, :] - p64[None]).square().sum(-1).min(dim=1).values.sqrt()
                         for s in range(0, len(v64), 4096)]).cpu().numpy()
    assert np.abs(nearest - thickness).max() <= delta + 1e-5, np.abs(nearest - thickness).max()
    # colour of the nearest kept point by the pinned float32 brute force, the lowest index on ties
    _, idx = R.nearest(points.cpu().numpy(), verts)
    assert (idx >= 0).all() and np.array_equal(vertex_colors, colors.cpu().numpy()[idx])

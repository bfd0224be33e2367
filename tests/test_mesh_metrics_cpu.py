"""
CPU-side checks of the mesh comparison (no GPU).  They tie the NumPy restatement tests/mesh_metrics_reference.py — which
the GPU tests hold the kernels to bit for bit — to the truth: the pinned fp32 point-triangle distance lies within the
derived bounds of an exact float64 distance over the whole domain, degenerate triangles included, and is never NaN;
seeded mutations of the restatement (one candidate dropped, pruning with >=, a zero margin) are rejected by the very
comparison the GPU test applies; the sampler is stratified; read_mesh round-trips every writer of the project and
names the file in every error; and the metric definitions give the known answers on concentric cubes.
"""
import os
import struct

import numpy as np
import pytest

import mesh_metrics_reference as M
import raycast_reference as R

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the pinned distance ----

def check_bounds(tris, pts):
    """-LOWER <= pinned - exact for every pair; pinned - exact <= UPPER(s) for the triangles the tree does not class as
    slivers (s >= 2^-6) and, with s = 1, for those of exactly zero area.  No NaN anywhere."""
    tris, pts = np.asarray(tris, dtype=F32), np.asarray(pts, dtype=F32)
    d2 = M.pair_distance(tris, pts)
    assert np.isfinite(d2).all() and (d2 >= 0).all()
    diff = np.sqrt(d2.astype(F64)) - M.exact_distance(tris, pts)
    rho = M.rho_of(tris, pts)[:, None]
    worst_low = (diff + M.lower_bound(rho)).min()
    assert worst_low >= 0, ("below the exact distance by more than the bound", worst_low)
    s = M.shape_sine(tris)
    exact_zero = (M.tri_areas(tris).astype(F64) == 0) & (np.linalg.norm(np.cross(
        tris[:, 1].astype(F64) - tris[:, 0], tris[:, 2].astype(F64) - tris[:, 0]), axis=1) == 0)
    bounded = (s >= M.SLIVER_SIN) | exact_zero
    assert bounded.any()
    upper = M.upper_bound(rho, np.where(exact_zero, 1.0, np.maximum(s, M.SLIVER_SIN))[None, :])
    worst_high = (upper - diff)[:, bounded].min()
    assert worst_high >= 0, ("above the exact distance by more than the bound", worst_high)
    return diff / (M.EPS * rho)


def test_pinned_distance_is_within_the_derived_bounds_of_float64():
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1.5, 1.5, size=(300, 3)).astype(F32)
    soup, cube = R.soup(1000), R.cube(0.5)
    check_bounds(soup, pts)
    check_bounds(soup, M.query_set(soup, seed=1))
    check_bounds(cube, pts)
    check_bounds(cube, M.query_set(cube, seed=2))
    check_bounds(cube, M.feature_points(cube, rng, 64))  # exactly on vertices, edges and faces
    check_bounds(R.icosphere(2), M.query_set(R.icosphere(2), seed=3))


def test_zero_area_triangles_give_the_distance_to_their_segment_or_point():
    rng = np.random.default_rng(1)
    dead = M.degenerate_triangles()
    pts = np.concatenate([rng.uniform(-1.5, 1.5, size=(300, 3)), dead.reshape(-1, 3),
                          dead.reshape(-1, 3) + rng.normal(size=(27, 3)) * 1e-6]).astype(F32)
    check_bounds(dead, pts)
    p, q = dead[1, 0].astype(F64), dead[1, 2].astype(F64)
    got = np.sqrt(M.pair_distance(dead[:2], pts).astype(F64))
    bound = M.upper_bound(M.rho_of(dead, pts))
    assert (np.abs(got[:, 0] - np.linalg.norm(pts.astype(F64) - p, axis=1)) <= bound).all()  # [p p p]: a point
    t = np.clip(((pts.astype(F64) - p) @ (q - p)) / ((q - p) @ (q - p)), 0, 1)
    seg = np.linalg.norm(pts.astype(F64) - (p + t[:, None] * (q - p)), axis=1)
    assert (np.abs(got[:, 1] - seg) <= bound).all()  # [p p q]: a segment


def test_bounds_hold_at_the_edges_of_the_domain():
    rng = np.random.default_rng(2)
    soup = R.soup(200, seed=3)
    pts = rng.uniform(-1.5, 1.5, size=(200, 3)).astype(F32)
    # coordinates at 2^20: the mesh fills the domain; and a unit mesh pushed to the corner of the domain
    big = (soup * F32(2.0 ** 19)).astype(F32)
    assert np.abs(big).max() > 2.0 ** 19
    check_bounds(big, np.clip(pts * F32(2.0 ** 19), -2.0 ** 20, 2.0 ** 20))
    corner = (R.cube(0.5) + F32(2.0 ** 20 - 0.5)).astype(F32)
    assert corner.max() == 2.0 ** 20
    check_bounds(corner, np.clip(pts + F32(2.0 ** 20 - 1), -2.0 ** 20, 2.0 ** 20).astype(F32))
    # an extent of 2^-20, at the origin and away from it
    tiny = (R.cube(0.5) * F32(2.0 ** -20)).astype(F32)
    assert float(np.ptp(tiny.reshape(-1, 3), axis=0).max()) == 2.0 ** -20
    check_bounds(tiny, pts * F32(2.0 ** -20))
    check_bounds(tiny, M.query_set(tiny, seed=4))
    check_bounds((tiny + F32(0.25)).astype(F32), pts * F32(2.0 ** -20) + F32(0.25))


def test_tree_walk_equals_the_brute_force_and_every_mutation_is_rejected():
    """The comparison of tests/test_gpu_mesh_metrics.py — (d2, id) bit for bit against the brute force — applied to the
    restated tree walk: it passes as stated, and fails for each seeded mutation, so the GPU test can fail."""
    def mismatches(tree, pts, want, **mutation):
        d2, idx = M.tree_nearest(tree, pts, **mutation)
        return int(((d2.view(np.uint32) != want[0].view(np.uint32)) | (idx != want[1])).sum())

    for name in ("cube", "icosphere2"):
        tris = M.nearest_cases()[name]
        pts = M.query_set(tris, seed=3)
        want = M.brute_force_nearest(tris, pts)
        assert len(np.unique(want[1])) > 1 and M.count_ties(tris, pts) > 0
        for drop in range(4):  # one candidate of the formula left out: no tree is needed to see it
            d2, idx = M.brute_force_nearest(tris, pts, drop=drop)
            assert ((d2.view(np.uint32) != want[0].view(np.uint32)) | (idx != want[1])).any(), (name, drop)
        for leaf in (4, 3):
            tree = M.build_tree(tris, leaf)
            assert mismatches(tree, pts, want) == 0
            assert mismatches(tree, pts, want, strict=False) > 0, (name, leaf, "pruning with >=")
            assert mismatches(tree, pts, want, margin=0.0) > 0, (name, leaf, "zero margin")
    for name in ("one", "soup_13"):
        tris = M.nearest_cases()[name]
        pts = M.query_set(tris, seed=3)
        want = M.brute_force_nearest(tris, pts)
        assert mismatches(M.build_tree(tris, 4), pts, want) == 0
        assert all(mismatches(M.build_tree(tris, 3), pts, want, drop=drop) > 0 for drop in range(4))


def test_closest_point_lies_on_the_triangle_at_the_pinned_distance():
    tris = R.icosphere(1)
    pts = M.query_set(tris, seed=5)
    d2, idx, cp = M.brute_force_nearest(tris, pts, want_point=True)
    again = np.linalg.norm(pts.astype(F64) - cp.astype(F64), axis=1)
    # the closest point is rounded as an absolute position: half an ulp of the coordinates per axis on top
    slack = M.upper_bound(M.rho_of(tris, pts)) + 2 * M.EPS * np.abs(tris).max() * np.sqrt(3)
    assert (np.abs(again - np.sqrt(d2.astype(F64))) <= slack).all()
    on_tri = M.exact_distance(tris, cp)[np.arange(len(cp)), idx]
    assert (on_tri <= slack).all()


# --------------------------------------------------------------------------------------------------- the sampler ----

def test_sampler_is_stratified_and_never_picks_a_zero_area_triangle():
    dead = M.degenerate_triangles()[[0, 1, 2, 3, 4, 6]]  # exactly zero area in fp32
    base = R.soup(40, seed=5, size=0.3)
    tris = np.concatenate([dead[:2], base[:20], dead[2:4], base[20:], dead[4:]]).astype(F32)
    areas = M.tri_areas(tris)
    assert (areas[:2] == 0).all() and (areas[-2:] == 0).all() and (areas == 0).sum() == 6
    cdf = M.area_cdf(tris)
    for m in (1, 63, 64, 65, 4097):
        pts, ids, j = M.sample_surface(tris, None, cdf, m, seed=7, stream=3)
        assert pts.shape == (m, 3) and pts.dtype == F32 and np.array_equal(ids, j)
        assert (np.diff(j) >= 0).all()  # stratified: in the order of the triangles
        counts = np.bincount(j, minlength=len(tris))
        assert (counts[areas == 0] == 0).all()
        expect = m * areas.astype(F64) / cdf[-1]
        assert (np.abs(counts - expect) < 2).all(), np.abs(counts - expect).max()
        d2 = M.pair_distance(tris, pts)[np.arange(m), j]
        # every point lies on its triangle: its own rounding as an absolute position on top of the distance bound
        slack = M.upper_bound(M.rho_of(tris, pts), np.maximum(M.shape_sine(tris)[j], M.SLIVER_SIN)) + \
            4 * M.EPS * np.abs(tris).max()
        assert (np.sqrt(d2.astype(F64)) <= slack).all()
    order = np.arange(len(tris))[::-1].copy()
    assert np.array_equal(M.sample_surface(tris, order, cdf, 65, 7, 3)[1], order[M.sample_surface(tris, None, cdf, 65, 7, 3)[2]])
    a = M.sample_surface(tris, None, cdf, 65, 7, 3)[0]
    assert not np.array_equal(a, M.sample_surface(tris, None, cdf, 65, 8, 3)[0])
    assert not np.array_equal(a, M.sample_surface(tris, None, cdf, 65, 7, 4)[0])


def test_fixed_order_fold_is_a_sum():
    rng = np.random.default_rng(6)
    for m in (1, 255, 256, 257, 1024 * 256 + 300):
        terms = rng.random(m)
        got = M.fold_sum(terms, 1.5)
        assert abs(got - (1.5 + np.sum(terms, dtype=np.longdouble))) <= (m + 1032) * 2.0 ** -53 * (terms.sum() + 1.5)
    acc = M.dist_stats(np.array([4.0, 0.25, 1.0], F32), np.array([-1.0, 0.5, 0.0], F32), (1.0, 0.4))
    assert acc.tolist() == [3.5, 5.25, 1.5, 4.0, 2.0, 0.0]
    assert M.dist_stats(np.array([9.0], F32), None, (1.0, 3.0), acc).tolist() == [6.5, 14.25, 1.5, 9.0, 2.0, 1.0]


# -------------------------------------------------------------------------------------------------------- readers ----

def _indexed(tris):
    verts, inverse = np.unique(tris.reshape(-1, 3), axis=0, return_inverse=True)
    return verts.astype(F32), inverse.reshape(-1, 3).astype(np.int32)


def test_read_mesh_round_trips_every_writer_bit_for_bit(tmp_path):
    from learn_nerf.mesh import write_obj, write_stl
    from learn_nerf.mesh_metrics import read_mesh, read_ply
    from learn_nerf.point_cloud import write_colored_obj, write_ply

    # multiples of 1 / 32 survive the OBJ writers' five decimals exactly
    exact = (R.cube(0.5) * F32([1.0, 1.5, 0.25]) + F32([3.0, -2.03125, 0.0])).astype(F32)
    verts, faces = _indexed(exact)
    colors = np.linspace(0, 1, verts.size).reshape(-1, 3).astype(F32)
    write_obj(str(tmp_path / "a.obj"), verts, faces)
    write_colored_obj(str(tmp_path / "b.obj"), verts, faces, colors)
    for name in ("a.obj", "b.obj"):
        got = read_mesh(str(tmp_path / name))
        assert got.dtype == F32 and got.tobytes() == exact.tobytes(), name
    rough = R.icosphere(1)  # arbitrary float32 values: the binary formats keep every bit
    verts, faces = _indexed(rough)
    write_stl(str(tmp_path / "c.stl"), verts, faces)
    write_ply(str(tmp_path / "d.ply"), verts, np.zeros_like(verts), faces)
    for name in ("c.stl", "d.ply", ):
        assert read_mesh(str(tmp_path / name)).tobytes() == rough.tobytes(), name
    cloud_verts, cloud_colors, cloud_faces = read_ply(str(tmp_path / "d.ply"))
    assert cloud_verts.tobytes() == verts.tobytes() and cloud_colors.shape == verts.shape and len(cloud_faces) == 80
    write_ply(str(tmp_path / "cloud.ply"), verts, np.ones_like(verts))  # a bare cloud parses, but is no mesh
    assert read_ply(str(tmp_path / "cloud.ply"))[1].max() == 255
    with pytest.raises(ValueError, match="cloud.ply.*no triangles"):
        read_mesh(str(tmp_path / "cloud.ply"))


def test_read_mesh_obj_forms_and_ply_variants(tmp_path):
    from learn_nerf.mesh_metrics import read_mesh

    quad = "# a quad and a triangle\nv 0 0 0\nv 1 0 0 0.5 0.5 0.5\nv 1 1 0\nvt 0 0\nvn 0 0 1\nv 0 1 0\n" \
           "f 1/1/1 2//1 3/1 4\nv 0 0 1\nf -1 -5 -4\n"
    (tmp_path / "q.obj").write_text(quad)
    got = read_mesh(str(tmp_path / "q.obj"))
    want = np.array([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]],
                     [[0, 0, 1], [0, 0, 0], [1, 0, 0]]], dtype=F32)
    assert np.array_equal(got, want)
    ascii_ply = "ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty uchar red\nproperty float z\n" \
                "property double x\nproperty float y\nelement face 1\nproperty list uchar uint vertex_index\n" \
                "end_header\n7 0 0 0\n7 0 1 0\n7 0 1 1\n7 0 0 1\n4 0 1 2 3\n"
    (tmp_path / "a.ply").write_text(ascii_ply)
    assert np.array_equal(read_mesh(str(tmp_path / "a.ply")), want[:2])
    header = b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float y\nproperty float x\n" \
             b"property short extra\nproperty float z\nelement face 2\nproperty uchar flag\n" \
             b"property list uchar int vertex_indices\nend_header\n"
    body = b"".join(struct.pack("<ffhf", y, x, 9, 0.0) for x, y in ((0, 0), (1, 0), (1, 1), (0, 1)))
    body += struct.pack("<BBiiii", 1, 4, 0, 1, 2, 3)[:18] + struct.pack("<BBiii", 0, 3, 0, 1, 2)
    (tmp_path / "b.ply").write_bytes(header + body)
    assert np.array_equal(read_mesh(str(tmp_path / "b.ply")), np.concatenate([want[:2], want[:1]]))


def test_read_mesh_names_the_file_in_every_error(tmp_path):
    from learn_nerf.mesh_metrics import read_mesh

    good_ply = b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\n" \
               b"property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n" + \
               struct.pack("<9f", 0, 0, 0, 1, 0, 0, 0, 1, 0) + struct.pack("<Biii", 3, 0, 1, 2)
    (tmp_path / "good.ply").write_bytes(good_ply)
    assert read_mesh(str(tmp_path / "good.ply")).shape == (1, 3, 3)
    cases = {
        "two.obj": b"v 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
        "word.obj": b"v 0 0 zero\nf 1 1 1\n",
        "range.obj": b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n",
        "zero.obj": b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n",
        "back.obj": b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n",
        "short.obj": b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n",
        "entry.obj": b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x/1\n",
        "none.obj": b"v 0 0 0\nv 1 0 0\nv 0 1 0\n",
        "nan.obj": b"v 0 0 nan\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
        "binary.obj": b"\xff\xfe\x00v",
        "magic.ply": b"plx\n" + good_ply[4:],
        "header.ply": good_ply[:good_ply.index(b"end_header")],
        "cut.ply": good_ply[:-5],
        "cutverts.ply": good_ply[:good_ply.index(b"end_header\n") + 11 + 20],
        "endian.ply": good_ply.replace(b"binary_little_endian", b"binary_big_endian"),
        "type.ply": good_ply.replace(b"property float y", b"property real y"),
        "noy.ply": good_ply.replace(b"property float y", b"property float w"),
        "index.ply": good_ply[:-4] + struct.pack("<i", 3),
        "count.ply": good_ply.replace(b"element vertex 3", b"element vertex three"),
        "asciicut.ply": b"ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
                        b"property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                        b"0 0 0\n1 0 0\n0 1 0\n3 0 1\n",
        "asciiword.ply": b"ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
                         b"property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                         b"0 0 0\n1 0 zero\n0 1 0\n3 0 1 2\n",
        "mesh.off": b"OFF\n",
        "short.stl": b"\x00" * 40,
    }
    for name, blob in cases.items():
        (tmp_path / name).write_bytes(blob)
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            read_mesh(str(tmp_path / name))


# -------------------------------------------------------------------------------------------------- known answers ----

H, DELTA, SAMPLES = 0.5, 0.0625, 1500


@pytest.fixture(scope="module")
def cube_pair():
    """pred = the outer cube, ref = the inner one, sampled by the restatement alone."""
    pred, ref = R.cube(H + DELTA), R.cube(H)
    sets = []
    for tris, stream in ((pred, 0), (ref, 1)):
        tree = M.build_tree(tris)
        pts, ids, _ = M.sample_surface(tree["sorted_tris"], tree["order"], M.area_cdf(tree["sorted_tris"]), SAMPLES, 0,
                                       stream)
        sets.append((pts, ids))
    bound = float(M.upper_bound(M.rho_of(pred, sets[0][0]).max()))  # covers both directions: the outer box is larger
    return pred, ref, sets, bound


def test_concentric_cubes_give_the_known_answers(cube_pair):
    pred, ref, ((ppts, pids), (rpts, rids)), bound = cube_pair
    inner_to_outer = np.sqrt(M.brute_force_nearest(pred, rpts)[0].astype(F64))
    assert (np.abs(inner_to_outer - DELTA) <= bound).all()
    outer_to_inner = np.sqrt(M.brute_force_nearest(ref, ppts)[0].astype(F64))
    assert (outer_to_inner >= DELTA - bound).all() and (outer_to_inner <= np.sqrt(3) * DELTA + bound).all()
    taus = (DELTA + bound, DELTA - bound, np.sqrt(3) * DELTA + bound)
    got, accs = M.compare_from_samples(pred, ref, ppts, pids, rpts, rids, taus)
    assert got["recall"] == (1.0, 0.0, 1.0)
    assert 0.0 < got["precision"][0] < 1.0 and got["precision"][1] == 0.0 and got["precision"][2] == 1.0
    assert got["f_score"][1] == 0.0 and got["f_score"][2] == 1.0
    assert got["f_score"][0] == 2 * got["precision"][0] / (got["precision"][0] + 1.0)
    assert abs(got["completeness"] - DELTA) <= bound
    assert DELTA - bound <= got["accuracy"] <= np.sqrt(3) * DELTA + bound
    assert got["chamfer"] == got["accuracy"] + got["completeness"]
    assert 2 * (DELTA - bound) ** 2 <= got["chamfer_l2"] <= 4 * (DELTA + bound) ** 2
    assert DELTA < got["hausdorff"] <= np.sqrt(3) * DELTA + bound
    assert got["hausdorff"] == np.sqrt(max(accs[0][3], accs[1][3]))
    # inner -> outer always lands on the parallel face; outer -> inner lands on an inner EDGE for the samples near the
    # outer cube's edges, where the two faces tie and the lower index may be the perpendicular one
    assert accs[1][2] == SAMPLES and 0.5 < got["normal_consistency"] <= 1.0
    assert M.compare_reference(pred, ref, SAMPLES, taus) == got  # the same digits from a second run


def test_a_mesh_against_itself():
    tris = R.icosphere(1)
    got = M.compare_reference(tris, tris, 700, (0.0, 1e-6))
    bound = float(M.upper_bound(M.rho_of(tris, tris.reshape(-1, 3)).max(),
                                np.maximum(M.shape_sine(tris).min(), M.SLIVER_SIN))) + 4 * M.EPS
    # 1, but for a sample that rounds across an edge onto the neighbouring face (about 20 degrees away on this mesh)
    assert got["normal_consistency"] > 0.9
    assert got["hausdorff"] <= bound and got["chamfer"] <= 2 * bound
    assert got["recall"][1] == 1.0 and got["precision"][1] == 1.0 and got["f_score"][1] == 1.0
    flat = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0], [0, 1, 0]]], dtype=F32)
    assert M.compare_reference(flat, flat, 300, (0.0,))["normal_consistency"] == 1.0


def test_new_entry_points_have_prototypes_and_host_size_queries():
    import re

    from learn_nerf import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lnrf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lnrf_(?:mesh|dist)_[a-z0-9_]+)\s*\(", text))
    assert declared == {"lnrf_mesh_nearest", "lnrf_mesh_tri_areas", "lnrf_mesh_sample_surface",
                        "lnrf_dist_stats_scratch_bytes", "lnrf_dist_stats_f64"}
    assert declared <= set(_lib.PROTOTYPES)
    lib = _lib.lib()
    assert lib.lnrf_version() == 200
    assert lib.lnrf_dist_stats_scratch_bytes(-1) == -1 and lib.lnrf_dist_stats_scratch_bytes(0) == 0
    assert lib.lnrf_dist_stats_scratch_bytes(1) == 12 * 8 and lib.lnrf_dist_stats_scratch_bytes(257) == 2 * 12 * 8
    assert lib.lnrf_dist_stats_scratch_bytes(10 ** 9) == 1024 * 12 * 8


def test_product_path_has_no_cpu_fallback():
    import torch

    from learn_nerf.mesh_metrics import compare_meshes, dist_stats_

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compare_meshes(R.cube(0.5), R.cube(0.6), samples=10, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dist_stats_(torch.ones(4), None, (1.0,), torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="thresholds"):
        compare_meshes(R.cube(0.5), R.cube(0.6), thresholds=())
    with pytest.raises(ValueError, match="thresholds"):
        compare_meshes(R.cube(0.5), R.cube(0.6), thresholds=tuple(range(9)))

"""
The mesh-comparison kernels on the GPU against the NumPy restatement tests/mesh_metrics_reference.py, bit for bit:
lnrf_mesh_nearest (d2, id and the optional closest point) against the brute force over every pair, under two leaf
sizes and over outputs pre-filled with 0x00, 0x41 and 0xFF bytes; lnrf_mesh_tri_areas and lnrf_mesh_sample_surface
given the same cdf; lnrf_dist_stats_f64 against the restated fold.  compare_meshes gives the known answers on concentric
cubes and spheres within the derived bound, equals the restatement run on the GPU's own samples, and prints the same
digits twice; scripts/eval_mesh.py runs end to end.  tests/test_mesh_metrics_cpu.py shows that these comparisons can fail.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import mesh_metrics_reference as M
import raycast_reference as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
LEAVES = (4, 3)
FILLS = (0x00, 0x41, 0xFF)
GRID_CAP = 2048 * 256  # kMaxGrid * kBlock of csrc/raycast.hip: beyond it a lane takes a second query


def _filled(shape, fill, dtype, dev):
    count = int(np.prod(shape)) * 4
    return torch.full((count,), fill, dtype=torch.uint8, device=dev).view(dtype).view(*shape)


def _nearest(tris, pts, leaf, fill, want_point):
    from learn_nerf.raycast import TriangleMesh

    dev = torch.device("cuda")
    mesh = TriangleMesh(torch.from_numpy(np.ascontiguousarray(tris)).to(dev), leaf_size=leaf)
    m = len(pts)
    out = [_filled((m,), fill, torch.float32, dev), _filled((m,), fill, torch.int32, dev)]
    if want_point:
        out.append(_filled((m, 3), fill, torch.float32, dev))
    got = mesh.nearest(torch.from_numpy(np.ascontiguousarray(pts)).to(dev), out=tuple(out))
    return [t.cpu().numpy() for t in got]


def check_nearest(tris, pts, leaves=LEAVES, chunk=512):
    tris, pts = np.asarray(tris, dtype=F32), np.asarray(pts, dtype=F32)
    want_d2, want_id, want_cp = M.brute_force_nearest(tris, pts, chunk=chunk, want_point=True)
    for leaf in leaves:
        for fill in FILLS if leaf == leaves[0] else FILLS[:1]:
            for want_point in (True, False):
                got = _nearest(tris, pts, leaf, fill, want_point)
                bad = np.nonzero(got[1] != want_id)[0]
                assert len(bad) == 0, (leaf, fill, bad[:8], got[1][bad[:8]], want_id[bad[:8]])
                assert np.array_equal(got[0].view(np.uint32), want_d2.view(np.uint32)), (leaf, fill)
                if want_point:
                    assert np.array_equal(got[2].view(np.uint32), want_cp.view(np.uint32)), (leaf, fill)
    return want_d2, want_id


@pytest.mark.parametrize("name", ["one", "cube", "icosphere2", "soup_mixed", "soup_13"])
def test_nearest_equals_the_brute_force_bit_for_bit(name):
    tris = M.nearest_cases()[name]
    assert len(tris) == {"one": 1, "cube": 12, "icosphere2": 320, "soup_mixed": 1013, "soup_13": 13}[name]
    pts = M.query_set(tris, seed=3)
    assert 300 < len(pts) < 1200
    d2, idx = check_nearest(tris, pts)
    assert (d2 == 0).any() and (d2 > 1e6).any()  # on the surface, and far away
    if len(tris) > 1:  # otherwise the case exercises nothing
        assert len(np.unique(idx)) > min(len(tris), 100) // 2
        assert M.count_ties(tris, pts) > 0


def test_nearest_beyond_the_grid_cap():
    tris = M.nearest_cases()["one"]  # the smallest mesh keeps the NumPy side short
    rng = np.random.default_rng(11)
    pts = rng.uniform(-2, 2, size=(GRID_CAP + 77, 3)).astype(F32)
    check_nearest(tris, pts, leaves=(4,), chunk=1 << 16)


def test_nearest_input_outside_the_domain_raises():
    from learn_nerf.raycast import TriangleMesh

    dev = torch.device("cuda")
    mesh = TriangleMesh(torch.from_numpy(R.cube(0.5)).to(dev))
    pts = torch.from_numpy(M.query_set(R.cube(0.5))[:16]).to(dev)
    for bad in (math.nan, math.inf, -math.inf, 2.0 ** 21):
        broken = pts.clone()
        broken[5, 1] = bad
        with pytest.raises(ValueError):
            mesh.nearest(broken)
    with pytest.raises(ValueError, match=r"\[m, 3\]"):
        mesh.nearest(pts[:, :2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.nearest(pts.cpu())
    with pytest.raises(ValueError, match="out"):
        mesh.nearest(pts, out=(torch.empty(3, device=dev), torch.empty(3, dtype=torch.int32, device=dev)))
    d2, idx = mesh.nearest(pts[:0])
    assert d2.shape == (0,) and idx.shape == (0,)
    with pytest.raises(ValueError, match="zero total area"):
        TriangleMesh(torch.from_numpy(M.degenerate_triangles()[[0, 1, 2, 3, 4, 6]]).to(dev)).sample_surface(4, 0)
    with pytest.raises(ValueError, match="cdf"):
        mesh.sample_surface(4, 0, cdf=torch.ones(3, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.sample_surface(4, 0, cdf=torch.ones(12, dtype=torch.float64))


# ------------------------------------------------------------------------------------------- areas and sampling ----

def _raw_sample(tris, order, cdf, m, seed, stream, fill=0x41):
    from learn_nerf import _lib as L

    dev = torch.device("cuda")
    t = torch.from_numpy(np.ascontiguousarray(tris)).to(dev)
    o = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(cdf)).to(dev)
    pts, ids = _filled((m, 3), fill, torch.float32, dev), _filled((m,), fill, torch.int32, dev)
    L.check(L.lib().lnrf_mesh_sample_surface(L.ptr(t), L.ptr(o, torch.int32), L.ptr(c, torch.float64), len(tris), m,
                                             seed, stream, L.ptr(pts), L.ptr(ids, torch.int32), L.stream()))
    return pts.cpu().numpy(), ids.cpu().numpy()


def _mesh_with_dead_triangles():
    dead = M.degenerate_triangles()[[0, 1, 2, 3, 4, 6]]
    base = R.soup(40, seed=5, size=0.3)
    return np.concatenate([dead[:2], base[:20], dead[2:4], base[20:], dead[4:]]).astype(F32)


def test_tri_areas_equal_the_restatement():
    from learn_nerf.raycast import TriangleMesh

    for tris in (_mesh_with_dead_triangles(), M.nearest_cases()["soup_mixed"], R.cube(0.5) * F32(2.0 ** 19)):
        mesh = TriangleMesh(torch.from_numpy(np.ascontiguousarray(tris)).cuda())
        got = mesh.tri_areas().cpu().numpy()
        assert np.array_equal(got.view(np.uint32), M.tri_areas(tris).view(np.uint32))
        assert np.array_equal(mesh.surface_cdf(), M.area_cdf(mesh.sorted_tris.cpu().numpy()))


@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097])
def test_sample_surface_equals_the_restatement(m):
    from learn_nerf.raycast import TriangleMesh

    # the raw entry point over triangles in the given order: zero area at the start, in the middle and at the end
    tris = _mesh_with_dead_triangles()
    cdf = M.area_cdf(tris)
    order = np.arange(len(tris), dtype=np.int32)[::-1].copy()
    for use_order in (None, order):
        want_pts, want_ids, j = M.sample_surface(tris, use_order, cdf, m, seed=2 ** 40 + 7, stream=3)
        got_pts, got_ids = _raw_sample(tris, use_order, cdf, m, 2 ** 40 + 7, 3)
        assert np.array_equal(got_ids, want_ids)
        assert np.array_equal(got_pts.view(np.uint32), want_pts.view(np.uint32))
        assert (M.tri_areas(tris)[j] > 0).all()
    # the same areas on another scale: only the ratios matter, and the total is read from the cdf
    flat_tail = cdf.copy()
    want_pts, want_ids, j = M.sample_surface(tris, None, flat_tail * 1e-300, m, 5, 0)
    got_pts, got_ids = _raw_sample(tris, None, flat_tail * 1e-300, m, 5, 0)
    assert np.array_equal(got_ids, want_ids) and np.array_equal(got_pts.view(np.uint32), want_pts.view(np.uint32))
    # and through TriangleMesh, whose sorted order puts the zero-area triangles last
    mesh = TriangleMesh(torch.from_numpy(tris).cuda())
    pts, ids = mesh.sample_surface(m, seed=9, stream_id=1)
    sorted_tris, sorted_order = mesh.sorted_tris.cpu().numpy(), mesh.order.cpu().numpy()
    want_pts, want_ids, _ = M.sample_surface(sorted_tris, sorted_order, M.area_cdf(sorted_tris), m, 9, 1)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), want_pts.view(np.uint32))
    assert (M.tri_areas(tris)[want_ids] > 0).all()


# ---------------------------------------------------------------------------------------------------- statistics ----

def _raw_stats(d2, cosine, thresholds, acc):
    """lnrf_dist_stats_f64 through the C ABI over a scratch block the test owns, pre-filled with NaN."""
    from learn_nerf import _lib as L

    dev = torch.device("cuda")
    m = len(d2)
    nbytes = L.lib().lnrf_dist_stats_scratch_bytes(m)
    scratch = torch.full((nbytes // 8 + 4,), math.nan, dtype=torch.float64, device=dev)
    taus = (ctypes.c_double * max(len(thresholds), 1))(*thresholds)
    d = torch.from_numpy(d2).to(dev)
    c = None if cosine is None else torch.from_numpy(cosine).to(dev)
    L.check(L.lib().lnrf_dist_stats_f64(L.ptr(d), L.ptr(c), m, taus, len(thresholds), L.ptr(acc, torch.float64),
                                        L.ptr(scratch, torch.float64), nbytes, L.stream()))
    assert torch.isnan(scratch[nbytes // 8:]).all()  # nothing written past the size asked for
    return acc


@pytest.mark.parametrize("m", [1, 255, 256, 257, 1024 * 256 + 300])
def test_dist_stats_equal_the_restated_fold(m):
    rng = np.random.default_rng(m)
    d2 = (rng.random(m) ** 2 * 3.0).astype(F32)
    cosine = rng.uniform(-1, 1, size=m).astype(F32)
    dist = np.sqrt(d2.astype(F64))
    eight = tuple(float(x) for x in np.quantile(dist, np.linspace(0.05, 0.95, 7))) + (float(dist[m // 2]),)
    for thresholds in ((float(dist[0]),), eight):  # each holds a threshold EQUAL to one of the distances
        for with_cosine in (True, False):
            acc = torch.zeros(4 + len(thresholds), dtype=torch.float64, device="cuda")
            _raw_stats(d2, cosine if with_cosine else None, thresholds, acc)
            want = M.dist_stats(d2, cosine if with_cosine else None, thresholds)
            assert acc.cpu().numpy().tobytes() == want.tobytes(), (thresholds, with_cosine, acc.tolist(), want.tolist())
            assert want[4] >= 1 and (with_cosine or want[2] == 0)
            # a second call into the non-zero accumulator adds
            other = (rng.random(300) * 5.0).astype(F32)
            _raw_stats(other, None, thresholds, acc)
            want = M.dist_stats(other, None, thresholds, want)
            assert acc.cpu().numpy().tobytes() == want.tobytes()
    assert abs(want[0] - (math.fsum(dist.tolist()) + math.fsum(np.sqrt(other.astype(F64)).tolist()))) <= \
        (m + 300 + 2 * 1032) * 2.0 ** -53 * want[0]


def test_dist_stats_through_the_python_layer_and_an_empty_call():
    from learn_nerf.mesh_metrics import dist_stats_

    d2 = np.array([4.0, 0.25, 1.0], dtype=F32)
    acc = torch.zeros(6, dtype=torch.float64, device="cuda")
    dist_stats_(torch.from_numpy(d2).cuda(), torch.tensor([-1.0, 0.5, 0.0], device="cuda"), (1.0, 0.4), acc)
    assert acc.tolist() == [3.5, 5.25, 1.5, 4.0, 2.0, 0.0]
    dist_stats_(torch.empty(0, device="cuda"), None, (1.0, 0.4), acc)
    assert acc.tolist() == [3.5, 5.25, 1.5, 4.0, 2.0, 0.0]
    with pytest.raises(ValueError, match="acc"):
        dist_stats_(torch.from_numpy(d2).cuda(), None, (1.0,), acc)


# ------------------------------------------------------------------------------------------------ compare_meshes ----

def _compare_twice(pred, ref, samples, thresholds):
    from learn_nerf.mesh_metrics import compare_meshes

    first = compare_meshes(pred, ref, samples=samples, thresholds=thresholds, seed=4)
    second = compare_meshes(pred, ref, samples=samples, thresholds=thresholds, seed=4)
    fields = ("accuracy", "completeness", "chamfer", "chamfer_l2", "precision", "recall", "f_score", "hausdorff",
              "normal_consistency", "normals_skipped", "degenerate_triangles")
    got = {f: getattr(first, f) for f in fields}
    assert got == {f: getattr(second, f) for f in fields}  # identical floats
    # the restatement, from the GPU's own samples: every metric to the last digit
    s = {k: v.cpu().numpy() for k, v in first.per_sample.items()}
    want, _ = M.compare_from_samples(pred, ref, s["pred_points"], s["pred_ids"], s["ref_points"], s["ref_ids"],
                                     thresholds)
    assert {f: got[f] for f in want} == want
    # and the samples are the restatement's, given the GPU's sorted order
    return first, s


def test_compare_meshes_on_concentric_cubes():
    h, delta, samples = 0.5, 0.0625, 3000
    pred, ref = R.cube(h + delta), R.cube(h)
    bound = float(M.upper_bound(M.rho_of(pred, pred.reshape(-1, 3)).max()))
    taus = (delta + bound, delta - bound, math.sqrt(3) * delta + bound)
    got, s = _compare_twice(pred, ref, samples, taus)
    tol = bound + math.sqrt(3) * delta * M.EPS  # per_sample distances are rounded to fp32
    assert (np.abs(s["ref_distance"].astype(F64) - delta) <= tol).all()  # inner -> outer
    assert got.recall == (1.0, 0.0, 1.0) and got.precision[1] == 0.0 and got.precision[2] == 1.0
    assert 0.0 < got.precision[0] < 1.0 and got.f_score[1] == 0.0 and got.f_score[2] == 1.0
    assert abs(got.completeness - delta) <= bound
    assert delta - bound <= got.accuracy <= math.sqrt(3) * delta + bound
    assert (s["pred_distance"] >= delta - tol).all() and (s["pred_distance"] <= math.sqrt(3) * delta + tol).all()
    assert delta < got.hausdorff <= math.sqrt(3) * delta + bound
    assert got.chamfer == got.accuracy + got.completeness
    assert got.normals_skipped == 0 and got.degenerate_triangles == (0, 0) and got.samples == samples
    same, _ = _compare_twice(ref, ref, 1000, (0.0, 1e-6))
    assert same.normal_consistency == 1.0 and same.hausdorff <= bound and same.f_score[1] == 1.0


def test_compare_meshes_on_concentric_icospheres():
    pred, ref = R.icosphere(3, radius=1.1), R.icosphere(3, radius=1.0)
    # the faces of the unit mesh lie between the radii c and 1, so both directed distances lie in [1.1 c - 1, 0.1]:
    # the radial image of a sample lies on the other mesh, 0.1 |x| away (0.1 |x| / 1.1 outward in)
    t = ref.astype(F64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    c = float((np.abs((n * t[:, 0]).sum(1)) / np.linalg.norm(n, axis=1)).min())
    low, high = 1.1 * c - 1.0, 0.1
    assert 0.09 < low < high
    s_min = float(M.shape_sine(ref).min())
    bound = float(M.upper_bound(M.rho_of(pred, pred.reshape(-1, 3)).max(), s_min)) + 4 * M.EPS  # + the samples' rounding
    got, s = _compare_twice(pred, ref, 3000, (high + bound, (low - bound) * 0.999))
    for side in ("pred", "ref"):
        d = s[side + "_distance"].astype(F64)
        assert (d >= low - bound - high * M.EPS).all() and (d <= high + bound + high * M.EPS).all()
        assert len(np.unique(s[side + "_ids"])) > 640 and len(np.unique(s[side + "_nearest"])) > 640  # of 1280
    assert got.precision == (1.0, 0.0) and got.recall == (1.0, 0.0) and got.f_score == (1.0, 0.0)
    assert low - bound <= got.accuracy <= high + bound and low - bound <= got.completeness <= high + bound
    assert 2 * (low - bound) ** 2 <= got.chamfer_l2 <= 2 * (high + bound) ** 2
    assert low - bound <= got.hausdorff <= high + bound
    assert got.normal_consistency > math.cos(math.radians(10))  # faces of this mesh subtend less than 10 degrees


# ---------------------------------------------------------------------------------------------------- the script ----

def _run(capsys, argv):
    from learn_nerf.scripts import eval_mesh

    eval_mesh.main(argv)
    return capsys.readouterr().out


def test_eval_mesh_end_to_end(tmp_path, capsys):
    from learn_nerf.mesh import write_obj, write_stl
    from learn_nerf.mesh_metrics import read_ply
    from learn_nerf.point_cloud import write_ply
    from learn_nerf.raycast import normalize

    def indexed(tris):
        verts, inverse = np.unique(tris.reshape(-1, 3), axis=0, return_inverse=True)
        return verts.astype(F32), inverse.reshape(-1, 3).astype(np.int32)

    pred = R.cube(1.0 + 1 / 32)  # multiples of 1 / 32 survive the OBJ writer exactly
    raw = (R.cube(0.5) * F32(3.0) + F32([5.0, 0.0, -1.0])).astype(F32)  # off-centre, and three times the size
    pre = normalize(raw)
    assert np.array_equal(pre, R.cube(1.0))
    write_obj(str(tmp_path / "pred.obj"), *indexed(pred))
    write_stl(str(tmp_path / "raw.stl"), *indexed(raw))
    verts, faces = indexed(pre)
    write_ply(str(tmp_path / "pre.ply"), verts, np.zeros_like(verts), faces)
    common = ["--samples", "20000", "--seed", "3"]
    first = _run(capsys, common + ["--normalize_reference", str(tmp_path / "pred.obj"), str(tmp_path / "raw.stl")])
    again = _run(capsys, common + ["--normalize_reference", str(tmp_path / "pred.obj"), str(tmp_path / "raw.stl")])
    assert first == again  # identical text
    values = dict(line.split("=", 1) for line in first.splitlines())
    assert len(values) == len(first.splitlines())  # every line parses, no key twice
    assert values["samples"] == "20000" and values["pred_triangles"] == "12" and values["ref_triangles"] == "12"
    assert values["pred_degenerate_triangles_skipped"] == "0" and values["normal_samples_skipped"] == "0"
    tau = float(values["threshold"])
    assert tau == 0.01 * float(np.linalg.norm([2.0, 2.0, 2.0]))  # 1 % of the reference box's diagonal
    numbers = {k: float(v) for k, v in values.items()}
    bound = float(M.upper_bound(M.rho_of(pred, pred.reshape(-1, 3)).max()))
    assert abs(numbers["completeness"] - 1 / 32) <= bound
    assert 1 / 32 < numbers["hausdorff"] <= math.sqrt(3) / 32 + bound
    assert numbers[f"recall[{tau!r}]"] == 1.0 and 0.0 < numbers[f"precision[{tau!r}]"] < 1.0
    # the pre-normalised reference without the flag: the same result; the raw one without it: another
    assert _run(capsys, common + [str(tmp_path / "pred.obj"), str(tmp_path / "pre.ply")]) == first
    other = _run(capsys, common + [str(tmp_path / "pred.obj"), str(tmp_path / "raw.stl")])
    assert other != first and float(dict(l.split("=", 1) for l in other.splitlines())["completeness"]) > 1.0
    out = _run(capsys, common + ["--threshold", "0.04", "--threshold", "0.02", "--per_sample_dir",
                                 str(tmp_path / "samples"), str(tmp_path / "pred.obj"), str(tmp_path / "pre.ply")])
    assert "recall[0.04]=1.0" in out.splitlines() and "recall[0.02]=0.0" in out.splitlines()
    for name in ("pred_samples.ply", "ref_samples.ply"):
        points, colors, faces = read_ply(str(tmp_path / "samples" / name))
        assert points.shape == (20000, 3) and colors.shape == (20000, 3) and len(faces) == 0
        assert colors[:, 1].max() == 0 and colors[:, 0].min() > 0  # every sample is at least 1 / 32 away
    with pytest.raises(SystemExit, match="nothing.stl"):
        _run(capsys, [str(tmp_path / "pred.obj"), str(tmp_path / "nothing.stl")])

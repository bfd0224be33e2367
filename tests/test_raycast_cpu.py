"""
STL dataset producer without a GPU: the NumPy brute force of the pinned ray-triangle test against the analytic cube of
scripts/make_cube_dataset.py, the STL reader and its errors, normalize, the camera fit and the camera files, and the
ABI table of the lnrf_rt_* entry points.
"""
import json
import math
import os
import re
import struct

import numpy as np
import pytest

import raycast_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_brute_force_hit_mask_equals_the_analytic_cube():
    """8 random 64^2 views (default_rng(0), radius 2.5, fov 40 degrees): the pinned test over the 12 triangles hits
    exactly where render_cube's alpha is 255; at most 4 pixels per view may differ (the restatement gives 0)."""
    from learn_nerf.dataset import CameraView
    from learn_nerf.scripts.make_cube_dataset import random_camera, render_cube

    rng = np.random.default_rng(0)
    fov = math.radians(40.0)
    tris = R.cube(0.5)
    for _ in range(8):
        origin, x, y, z = random_camera(rng, 2.5)
        alpha = render_cube(origin, x, y, z, fov, 64)[..., 3].reshape(-1)
        view = CameraView(tuple(z), tuple(origin), tuple(x), tuple(y), fov, fov)
        t, idx, occ = R.brute_force(tris, view.bare_rays(64, 64).numpy())
        differ = int(((idx >= 0) != (alpha == 255)).sum())
        print("pixels that differ:", differ)
        assert differ <= 4
        assert np.array_equal(occ == 1, idx >= 0) and np.array_equal(np.isfinite(t), idx >= 0)
        assert 500 < (idx >= 0).sum() < 4096


def test_brute_force_tie_goes_to_the_lowest_index():
    tris = np.concatenate([R.cube(0.5)] * 2)
    rays = np.array([[[0.1, 0.2, 3.0], [0.0, 0.0, -1.0]]], dtype=np.float32)
    t, idx, _ = R.brute_force(tris, rays)
    assert idx[0] < 12 and abs(float(t[0]) - 2.5) < 1e-6
    t2, idx2, _ = R.brute_force(tris[::-1].copy(), rays)
    assert t2[0] == t[0] and idx2[0] < 12


def _write_binary(path, tris, count=None, cut=None):
    tris = np.asarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    rec = np.zeros(len(tris), dtype=[("normal", "<f4", (3,)), ("verts", "<f4", (3, 3)), ("attr", "<u2")])
    rec["verts"] = tris
    data = b"\x00" * 80 + struct.pack("<I", len(tris) if count is None else count) + rec.tobytes()
    with open(path, "wb") as f:
        f.write(data if cut is None else data[:cut])


def _write_ascii(path, tris, end=True):
    lines = ["solid test"]
    for tri in np.asarray(tris, dtype=np.float32):
        lines += ["facet normal 0 0 0", " outer loop"]
        lines += [f"  vertex {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}" for v in tri]
        lines += [" endloop", "endfacet"]
    if end:
        lines.append("endsolid test")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_stl_reader_round_trips_binary_and_ascii(tmp_path):
    from learn_nerf.mesh import write_stl
    from learn_nerf.raycast import read_stl

    tris = R.icosphere(1) * np.float32(0.37) + np.float32(0.123)
    verts = tris.reshape(-1, 3)
    faces = np.arange(len(verts)).reshape(-1, 3)
    write_stl(str(tmp_path / "a.stl"), verts, faces)
    got = read_stl(str(tmp_path / "a.stl"))
    assert got.dtype == np.float32 and got.shape == tris.shape and got.tobytes() == tris.tobytes()
    _write_ascii(tmp_path / "b.stl", tris)
    assert read_stl(str(tmp_path / "b.stl")).tobytes() == tris.tobytes()


def test_stl_reader_errors(tmp_path):
    from learn_nerf.raycast import read_stl

    tris = R.cube()
    _write_binary(tmp_path / "short.stl", tris, cut=60)
    with pytest.raises(ValueError, match="truncated STL"):
        read_stl(str(tmp_path / "short.stl"))
    _write_binary(tmp_path / "cut.stl", tris, cut=84 + 50 * 7 + 11)
    with pytest.raises(ValueError, match="counts 12 triangles"):
        read_stl(str(tmp_path / "cut.stl"))
    _write_binary(tmp_path / "count.stl", tris, count=13)
    with pytest.raises(ValueError, match="counts 13 triangles"):
        read_stl(str(tmp_path / "count.stl"))
    _write_binary(tmp_path / "empty.stl", tris[:0])
    with pytest.raises(ValueError, match="no triangles"):
        read_stl(str(tmp_path / "empty.stl"))
    bad = tris.copy()
    bad[3, 1, 2] = np.inf
    _write_binary(tmp_path / "inf.stl", bad)
    with pytest.raises(ValueError, match="non-finite"):
        read_stl(str(tmp_path / "inf.stl"))
    _write_ascii(tmp_path / "open.stl", tris, end=False)
    with pytest.raises(ValueError, match="truncated STL"):
        read_stl(str(tmp_path / "open.stl"))
    with open(tmp_path / "vertex.stl", "w") as f:
        f.write("solid x\nfacet normal 0 0 0\nouter loop\nvertex 0 0 0\nvertex 1 0\nendloop\nendfacet\nendsolid x\n")
    with pytest.raises(ValueError, match="malformed ASCII STL"):
        read_stl(str(tmp_path / "vertex.stl"))
    with pytest.raises(OSError):
        read_stl(str(tmp_path / "missing.stl"))


def test_normalize_centres_the_box_and_scales_the_largest_coordinate_to_one():
    from learn_nerf.raycast import normalize

    tris = R.icosphere(1) * np.float32([3.0, 0.5, 1.25]) + np.float32([10.0, -4.0, 0.25])
    out = normalize(tris)
    assert out.dtype == np.float32 and out.shape == tris.shape
    lo, hi = out.min(axis=(0, 1)), out.max(axis=(0, 1))
    assert np.abs(lo + hi).max() <= 2e-7
    assert hi.max() == np.float32(1.0)
    t64 = tris.astype(np.float64)
    mid = (t64.min(axis=(0, 1)) + t64.max(axis=(0, 1))) / 2
    expect = ((t64 - mid) * (1 / (t64 - mid).max())).astype(np.float32)
    assert out.tobytes() == expect.tobytes()
    with pytest.raises(ValueError, match="zero extent"):
        normalize(np.ones((2, 3, 3), np.float32))


@pytest.mark.parametrize("fov_degrees", [60.0, 25.0])
def test_fitted_camera_puts_every_corner_inside_the_central_90_percent(fov_degrees):
    from learn_nerf.raycast import camera_at, fit_distance, random_unit

    lo, hi = np.array([-1.0, -0.4, -0.7]), np.array([1.0, 0.4, 0.7])
    fov = math.radians(fov_degrees)
    rs = np.random.RandomState(3)
    directions = [random_unit(rs) for _ in range(6)] + [np.array([0.0, 0.0, 1.0]), np.array([0.1, 0.0, -1.0])]
    for v in directions:
        dist = fit_distance(lo, hi, v, fov)
        view = camera_at(lo, hi, v, dist, fov)
        uv = R.project(view, R.box_corners(lo, hi))
        assert uv.min() >= 0.05 - 1e-9 and uv.max() <= 0.95 + 1e-9
        assert min(abs(uv - 0.05).min(), abs(uv - 0.95).min()) < 1e-3
        bisect = R.fit_distance_bisect(lo, hi, lambda d: camera_at(lo, hi, v, d, fov))
        assert abs(bisect - dist) <= 1e-9 * dist
        x, y, z = (np.asarray(a) for a in (view.x_axis, view.y_axis, view.camera_direction))
        assert np.allclose(np.cross(x, y), z, atol=1e-12) and abs(x @ z) < 1e-12  # y = z cross x, down the image
        assert np.allclose(np.asarray(view.camera_origin), (lo + hi) / 2 + dist * v / np.linalg.norm(v))


def test_rotating_cameras_share_one_distance_and_circle_the_axis():
    from learn_nerf.raycast import fit_distance, rotating_cameras, rotating_directions

    lo, hi = np.array([-1.0, -0.4, -0.7]), np.array([1.0, 0.4, 0.7])
    fov = math.radians(60.0)
    views = rotating_cameras(lo, hi, fov, (0, 0, 1), (0, -1, 0), 8)
    dists = [np.linalg.norm(np.asarray(v.camera_origin) - (lo + hi) / 2) for v in views]
    assert np.allclose(dists, dists[0], rtol=1e-12)
    directions = rotating_directions((0, 0, 1), (0, -1, 0), 8)
    assert np.isclose(dists[0], max(fit_distance(lo, hi, v, fov) for v in directions), rtol=1e-12)
    assert np.allclose(directions[0], [0, -1, 0]) and np.allclose(directions[2], [1, 0, 0], atol=1e-12)
    assert np.allclose(directions[:, 2], 0, atol=1e-12)


def test_cli_no_images_writes_camera_files_that_the_loader_parses(tmp_path):
    """--no_images needs no GPU: NNNN.json and metadata.json only; the JSON parses with CameraView.from_json and
    --rotate gives origins on a circle about the axis."""
    from learn_nerf.dataset import CameraView, ModelMetadata
    from learn_nerf.raycast import normalize
    from learn_nerf.scripts import stl_dataset

    tris = R.cube(0.5) * np.float32([2.0, 1.0, 0.5])
    _write_binary(tmp_path / "box.stl", tris)
    out = tmp_path / "data"
    stl_dataset.main(["--no_images", "--rotate", "--images", "4", str(tmp_path / "box.stl"), str(out)])
    assert sorted(os.listdir(out)) == ["0000.json", "0001.json", "0002.json", "0003.json", "metadata.json"]
    meta = ModelMetadata.from_json(str(out / "metadata.json"))
    norm = normalize(tris)
    assert list(meta.bbox_min) == norm.min(axis=(0, 1)).tolist() and list(meta.bbox_max) == norm.max(axis=(0, 1)).tolist()
    assert max(meta.bbox_max) == 1.0
    origins = []
    for i in range(4):
        view = CameraView.from_json(str(out / f"{i:04d}.json"))
        assert view.x_fov == view.y_fov == math.radians(60.0)
        x, y, z = (np.asarray(a) for a in (view.x_axis, view.y_axis, view.camera_direction))
        assert np.allclose(np.cross(x, y), z, atol=1e-12)
        assert set(json.load(open(out / f"{i:04d}.json"))) == {"origin", "x", "y", "z", "x_fov", "y_fov"}
        origins.append(np.asarray(view.camera_origin))
    origins = np.array(origins)
    assert np.allclose(origins[:, 2], 0, atol=1e-12)
    radii = np.linalg.norm(origins[:, :2], axis=1)
    assert np.allclose(radii, radii[0], rtol=1e-12)
    assert np.allclose(origins[0] / radii[0], [0, -1, 0], atol=1e-12)
    assert np.allclose(origins[1] / radii[0], [1, 0, 0], atol=1e-12)


def test_cli_refuses_bad_input_before_writing(tmp_path, capsys):
    from learn_nerf.scripts import stl_dataset

    _write_binary(tmp_path / "bad.stl", R.cube(), count=99)
    with pytest.raises(SystemExit) as err:
        stl_dataset.main(["--no_images", str(tmp_path / "bad.stl"), str(tmp_path / "out")])
    assert "counts 99 triangles" in str(err.value.code) and not os.path.exists(tmp_path / "out")
    _write_binary(tmp_path / "point.stl", np.ones((1, 3, 3), np.float32))
    with pytest.raises(SystemExit) as err:
        stl_dataset.main(["--no_images", str(tmp_path / "point.stl"), str(tmp_path / "out")])
    assert "zero extent" in str(err.value.code) and not os.path.exists(tmp_path / "out")
    _write_binary(tmp_path / "good.stl", R.cube())
    (tmp_path / "file").write_text("x")
    with pytest.raises(SystemExit) as err:
        stl_dataset.main(["--no_images", str(tmp_path / "good.stl"), str(tmp_path / "file")])
    assert "output directory already exists" in str(err.value.code)


def test_ray_casting_entry_points_have_prototypes():
    from learn_nerf import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lnrf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lnrf_rt_[a-z0-9_]+)\s*\(", text))
    assert declared == {"lnrf_rt_node_count", "lnrf_rt_morton", "lnrf_rt_fit", "lnrf_rt_closest", "lnrf_rt_occluded"}
    assert declared <= set(_lib.PROTOTYPES)
    lib = _lib.lib()
    assert lib.lnrf_rt_node_count(1, 4) == 2 and lib.lnrf_rt_node_count(5, 4) == 4
    assert lib.lnrf_rt_node_count(1025, 4) == 1024 and lib.lnrf_rt_node_count(0, 4) == -1
    assert lib.lnrf_rt_node_count(8, 65) == -1
    assert ctypes_sizeof_bvh() == 40


def ctypes_sizeof_bvh():
    import ctypes

    from learn_nerf import _lib

    return ctypes.sizeof(_lib.RtBvh)

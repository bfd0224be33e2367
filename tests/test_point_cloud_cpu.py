"""
CPU checks of the point-cloud export (learn_nerf/point_cloud.py, scripts/point_cloud.py): the command line, the
back-projection of a synthetic RGB-D dataset with a known surface, subsampling, the writers and the field's grid
geometry.  The neighbour search itself needs the GPU (tests/test_gpu_point_cloud.py).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import point_cloud_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "learn-nerf_amd")
SCRIPT = os.path.join(PKG, "learn_nerf", "scripts", "point_cloud.py")
MAX_DEPTH = 4.0


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, SCRIPT, *args], env=env, capture_output=True, text=True, timeout=300)


def test_parser_flags_and_defaults_are_the_go_programs():
    from learn_nerf.scripts.point_cloud import build_parser

    args = build_parser().parse_args(["data", "out.obj"])
    assert (args.max_depth, args.thickness, args.delta, args.max_points) == (10.0, 0.02, 0.02, 50000)
    assert args.sort_density is False and args.sort_density_k == 5 and args.seed == 0
    assert args.batch_size >= 1 and args.cloud_path is None
    assert (args.data_dir, args.output_path) == ("data", "out.obj")
    args = build_parser().parse_args(["--max_depth", "3", "--thickness", "0.1", "--delta", "0.05", "--max_points", "7",
                                      "--sort_density", "--sort_density_k", "3", "--seed", "9", "--batch_size", "64",
                                      "--cloud_path", "c.ply", "d", "o.ply"])
    assert (args.max_depth, args.thickness, args.delta, args.max_points) == (3.0, 0.1, 0.05, 7)
    assert args.sort_density is True and (args.sort_density_k, args.seed, args.batch_size) == (3, 9, 64)
    assert args.cloud_path == "c.ply"


def test_cli_bad_extension_and_empty_directory_fail_with_a_message(tmp_path):
    res = run_cli(str(tmp_path / "missing"), str(tmp_path / "mesh.stl"))
    assert res.returncode == 2
    assert ".obj or .ply" in res.stderr and "Computing" not in res.stdout
    res = run_cli(str(tmp_path), str(tmp_path / "mesh.obj"))
    assert res.returncode not in (0, 2)
    assert "00000.json" in res.stderr and not os.path.exists(tmp_path / "mesh.obj")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sphere_views"))
    return d, R.write_sphere_dataset(d, size=33, max_depth=MAX_DEPTH)


def test_back_projection_of_the_sphere_dataset(dataset):
    from learn_nerf.point_cloud import read_dataset, read_rgbd_view

    d, views = dataset
    bound = (MAX_DEPTH / 65535) / 0.7746 + 1e-5  # truncation step over the corner pixel's cosine, plus fp32 slack
    assert abs(R.CORNER_COSINE - 0.7746) < 1e-4
    total = 0
    for i, (view, depth, color) in enumerate(views):
        stem = os.path.join(d, f"{i:05d}")
        points, colors = read_rgbd_view(stem + ".json", stem + "_depth.png", stem + ".png", MAX_DEPTH)
        assert points.dtype == torch.float32 and colors.dtype == torch.float32 and points.device.type == "cpu"
        hit = depth.reshape(-1) != R.NO_DEPTH
        assert 100 < hit.sum() < hit.size and points.shape == (hit.sum(), 3) and colors.shape == points.shape
        norm = np.linalg.norm(points.numpy().astype(np.float64), axis=1)
        assert np.abs(norm - R.SPHERE_RADIUS).max() <= bound, np.abs(norm - R.SPHERE_RADIUS).max()
        want_p, want_c = R.back_project(view, depth, color, MAX_DEPTH)  # raster order
        assert np.abs(points.numpy() - want_p).max() < 1e-5
        assert np.array_equal(colors.numpy(), want_c.astype(np.float32))
        total += int(hit.sum())
    points, colors, count = read_dataset(d, MAX_DEPTH)
    assert count == len(views) and points.shape == (total, 3) and colors.shape == (total, 3)
    first, _ = read_rgbd_view(os.path.join(d, "00000.json"), os.path.join(d, "00000_depth.png"),
                              os.path.join(d, "00000.png"), MAX_DEPTH)
    assert torch.equal(points[:len(first)], first)  # views in file-number order


def write_view(tmp_path, depth, color, mode=None):
    from PIL import Image

    view = dict(origin=[0.0, 0.0, -2.0], x=[1.0, 0.0, 0.0], y=[0.0, 1.0, 0.0], z=[0.0, 0.0, 1.0], x_fov=R.FOV,
                y_fov=R.FOV)
    paths = [str(tmp_path / n) for n in ("00000.json", "00000_depth.png", "00000.png")]
    with open(paths[0], "w") as fh:
        json.dump(view, fh)
    image = Image.fromarray(depth)
    assert mode is None or image.mode == mode
    image.save(paths[1])
    Image.fromarray(color).save(paths[2])
    return paths


def test_centre_pixel_is_exactly_origin_plus_z_times_depth(tmp_path):
    from PIL import Image

    from learn_nerf.point_cloud import _depth_array, read_rgbd_view

    depth = np.full((5, 7), R.NO_DEPTH, dtype=np.uint16)
    depth[2, 3] = 40000
    depth[0, 0] = 12345
    color = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    # a 16-bit PNG opens as mode 'I;16' or as 'I' (32-bit) depending on the PIL: both read alike
    wide = Image.fromarray(depth.astype(np.int32))
    assert wide.mode == "I" and np.array_equal(_depth_array(wide), depth)
    assert np.array_equal(_depth_array(Image.fromarray(depth)), depth)
    with pytest.raises(ValueError, match="mode"):
        _depth_array(Image.fromarray(depth.astype(np.uint8)))
    points, colors = read_rgbd_view(*write_view(tmp_path, depth, color, "I;16"), 10.0)
    assert points.shape == (2, 3)  # raster order: the corner first, then the centre
    z = np.float32(40000) / np.float32(65535) * np.float32(10.0)
    assert np.array_equal(points[1].numpy(), np.array([0, 0, np.float32(-2) + z], np.float32))
    assert np.array_equal(colors.numpy(), color[[0, 2], [0, 3]].astype(np.float32) / np.float32(255))
    assert points[0, 0] < 0 and points[0, 1] < 0


def test_mismatched_image_sizes_raise_with_both_shapes(tmp_path):
    from learn_nerf.point_cloud import read_rgbd_view

    paths = write_view(tmp_path, np.zeros((5, 7), np.uint16), np.zeros((5, 6, 3), np.uint8))
    with pytest.raises(ValueError, match=r"\(5, 6\).*\(5, 7\)"):
        read_rgbd_view(*paths, 10.0)


def test_subsample_identity_seeded_shuffle_and_stable_density_prefix():
    from learn_nerf.point_cloud import subsample

    rng = np.random.default_rng(0)
    points = torch.from_numpy(rng.random((50, 3), dtype=np.float32))
    colors = torch.from_numpy(rng.random((50, 3), dtype=np.float32))
    for limit in (50, 51):
        p, c = subsample(points, colors, limit, sort_density=True, k=5, knn=None)  # the search is not even called
        assert p is points and c is colors
    a = subsample(points, colors, 20, seed=3)
    b = subsample(points, colors, 20, seed=3)
    other = subsample(points, colors, 20, seed=4)
    keep = np.random.RandomState(3).permutation(50)[:20]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], other[0])
    assert torch.equal(a[0], points[keep]) and torch.equal(a[1], colors[keep])

    dist = torch.from_numpy(rng.integers(0, 4, size=50).astype(np.float32))  # many ties
    calls = []

    def fake_knn(pts, k):
        calls.append((pts, k))
        return dist

    p, c = subsample(points, colors, 20, sort_density=True, k=7, knn=fake_knn)
    keep = np.argsort(dist.numpy(), kind="stable")[:20]
    assert calls[0][0] is points and calls[0][1] == 7 and len(calls) == 1
    assert torch.equal(p, points[keep]) and torch.equal(c, colors[keep])


def test_writers_round_trip(tmp_path):
    from learn_nerf.point_cloud import write_colored_obj, write_ply

    verts = np.array([[0, 0.5, 1.25], [-2, 3.5, 1e-7], [1, 1, 1]], np.float32)
    colors = np.array([[0, 0.5, 1], [0.25, 0.2, 1.0 / 255], [1, 1, 1]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    obj = str(tmp_path / "m.obj")
    write_colored_obj(obj, verts, faces, colors)
    assert open(obj).read().splitlines()[:2] == ["v 0.00000 0.50000 1.25000 0.00000 0.50000 1.00000",
                                                 "v -2.00000 3.50000 0.00000 0.25000 0.20000 0.00392"]
    assert open(obj).read().endswith("f 1 2 3\nf 3 2 1\n")
    v, c, f = R.read_colored_obj(obj)
    assert np.abs(v - verts).max() <= 5e-6 and np.abs(c - colors).max() <= 5e-6 and np.array_equal(f, faces)

    ply = str(tmp_path / "m.ply")
    write_ply(ply, verts, colors, faces)
    v, c, f = R.read_ply(ply)
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    assert np.array_equal(c, np.array([[0, 128, 255], [64, 51, 1], [255, 255, 255]], np.uint8))
    cloud = str(tmp_path / "c.ply")
    write_ply(cloud, verts, colors)
    v, c, f = R.read_ply(cloud)
    assert np.array_equal(v, verts) and len(f) == 0 and b"element face" not in open(cloud, "rb").read()


def test_field_geometry_and_point_budget():
    from learn_nerf.point_cloud import field_axes, point_field

    lo, hi = (-0.5, 0.0, 1.0), (0.5, 0.0, 1.33)
    axes = field_axes(lo, hi, 0.1, 0.05)
    pad = 0.1 + 0.05
    # extents 1.3, 0.3, 0.63 over 0.05 -> 26, 6 (7 where the float64 quotient lands just above 6) and 13 steps
    assert [len(a) for a in axes] == [int(np.ceil((h - l + 2 * pad) / 0.05)) + 1 for l, h in zip(lo, hi)]
    assert len(axes[0]) == 27 and len(axes[1]) in (7, 8) and len(axes[2]) == 14
    for a, l, h in zip(axes, lo, hi):
        assert a.dtype == np.float64 and a[0] == l - pad and np.allclose(np.diff(a), 0.05, atol=1e-12)
        assert a[-1] >= h + pad - 1e-12  # the whole padded box is covered
    pts = np.array([lo, hi], np.float32)
    mine = R.field_axes(pts, 0.1, 0.05)
    assert all(np.array_equal(a, b) for a, b in zip(axes, mine))

    # the budget is checked before anything is allocated or launched: a CPU tensor gets as far as the message
    points = torch.tensor([lo, hi], dtype=torch.float32)
    with pytest.raises(ValueError, match="--delta"):
        point_field(points, 0.1, 0.05, max_field_points=1000)
    with pytest.raises(ValueError, match="--delta"):
        point_field(points, 0.02, 1e-4)  # the default budget
    with pytest.raises(RuntimeError, match="GPU"):
        point_field(points, 0.1, 0.05)  # within the budget: the search needs a GPU

"""
scripts/tsdf_mesh.py on the GPU, in a child process, on the analytic sphere dataset of tests/tsdf_reference.py (with a
small second sphere as a floater): the .obj and .ply it writes hold the vertices, faces and colours of
TsdfVolume.extract for the same arguments, with and without --keep_largest 1, and the counts it prints are the
library's.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import point_cloud_reference as P
import tsdf_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "learn-nerf_amd")
SCRIPT = os.path.join(PKG, "learn_nerf", "scripts", "tsdf_mesh.py")
RESOLUTION, MAX_DEPTH = 32, 8.0


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, SCRIPT, *args], env=env, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def fused(tmp_path_factory):
    """The dataset on disk and the library's volume of it, shared by the cases."""
    from learn_nerf.tsdf import TsdfVolume, read_rgbd_views

    data = str(tmp_path_factory.mktemp("tsdf") / "views")
    R.write_dataset(data, *R.sphere_scene(R.ICOSAHEDRON, 64, 64, MAX_DEPTH, floater=R.FLOATER))
    cameras, depths, colors = read_rgbd_views(data)
    assert len(cameras) == 12
    vol = TsdfVolume(R.BBOX_MIN, R.BBOX_MAX, RESOLUTION, truncation_voxels=2.5, max_depth=MAX_DEPTH, device="cuda")
    vol.integrate(cameras, depths, colors)
    return data, vol


@pytest.mark.parametrize("ext", [".obj", ".ply"])
@pytest.mark.parametrize("keep_largest", [None, 1], ids=["all", "keep_largest"])
def test_cli_outputs_equal_the_library(fused, tmp_path, keep_largest, ext):
    from learn_nerf.point_cloud import write_colored_obj

    data, vol = fused
    flags = ["--resolution", str(RESOLUTION), "--truncation", "2.5", "--max_depth", str(MAX_DEPTH)]
    kwargs = {}
    if keep_largest:  # removes the floater
        flags += ["--keep_largest", str(keep_largest), "--connectivity", "6"]
        kwargs = dict(keep_largest=keep_largest, connectivity=6)
    verts, faces, vertex_colors, info = vol.extract(**kwargs)
    assert len(faces) > 1000
    out = str(tmp_path / ("mesh" + ext))
    res = run_cli(*flags, data, out)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    want = ["Fusing 12 views...",
            f"voxels: observed={info['observed']} unseen_inside={info['unseen_inside']} "
            f"unseen_outside={info['unseen_outside']}"]
    if keep_largest:
        assert info["components"] == 2 and info["kept"] == 1 and info["removed"] > 0
        assert len(faces) < len(vol.extract()[1])
        want.append(f"components: kept 1 of 2, removed {info['removed']} points")
    want += [f"vertices={len(verts)} faces={len(faces)} uncoloured={info['uncoloured']}", "Saving mesh..."]
    assert res.stdout.splitlines() == want
    if ext == ".obj":
        xyz, rgb, idx = P.read_colored_obj(out)
        assert np.array_equal(idx, faces)
        # the file holds 5 decimals: the library's writer gives the same text
        assert np.abs(xyz - verts).max() <= 0.51e-5 and np.abs(rgb - vertex_colors).max() <= 0.51e-5
        write_colored_obj(str(tmp_path / "lib.obj"), verts, faces, vertex_colors)
        assert open(out, "rb").read() == open(tmp_path / "lib.obj", "rb").read()
    else:
        xyz, rgb, idx = P.read_ply(out)
        assert np.array_equal(xyz, verts) and np.array_equal(idx, faces)
        want_rgb = np.clip(np.rint(vertex_colors.astype(np.float64) * 255), 0, 255).astype(np.uint8)
        assert np.array_equal(rgb, want_rgb)


def test_cli_without_a_surface_fails_with_a_message(tmp_path):
    cameras, depths, colors = R.sphere_scene(R.AXES6[:2], 16, 16, MAX_DEPTH)
    data = str(tmp_path / "empty_views")
    R.write_dataset(data, cameras, [np.full_like(d, R.NO_DEPTH) for d in depths], colors)
    res = run_cli("--resolution", "16", "--max_depth", str(MAX_DEPTH), data, str(tmp_path / "none.ply"))
    assert res.returncode != 0
    assert "no surface" in res.stderr and re.search(r"voxels: observed=\d+ unseen_inside=0", res.stdout)
    assert not os.path.exists(tmp_path / "none.ply")

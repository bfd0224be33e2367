"""
scripts/texture_mesh.py on the GPU, in a child process, on the cube scene of tests/texture_cases.py written as a dataset:
the files it writes hold the library's texture and the input's triangles, its key=value lines come in the documented
order, --target_faces simplifies first, and a texture that is too small ends with the message that says what to do.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import texture_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "learn-nerf_amd")
SCRIPT = os.path.join(PKG, "learn_nerf", "scripts", "texture_mesh.py")
KEYS = ["faces", "texture_size", "cell", "views", "offset", "texels_used", "seen", "filled", "unseen",
        "degenerate_faces"]


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, SCRIPT, *args], env=env, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from learn_nerf.mesh import write_stl

    case = C.cube_case()
    root = tmp_path_factory.mktemp("texture")
    data, mesh = str(root / "data"), str(root / "cube.stl")
    C.write_dataset(data, case.cameras, case.images)
    verts = case.tris.reshape(-1, 3)
    write_stl(mesh, verts, np.arange(len(verts)).reshape(-1, 3))
    return case, data, mesh


def parse(stdout):
    pairs = [line.split("=", 1) for line in stdout.splitlines() if "=" in line]
    return [k for k, _ in pairs], {k: v for k, v in pairs if not k.startswith("reprojection_psnr")}


def test_cli_writes_the_librarys_texture(scene, tmp_path):
    from PIL import Image

    from learn_nerf.mesh_metrics import read_mesh
    from learn_nerf.raycast import TriangleMesh
    from learn_nerf.texture import TextureAtlas, bake_views, read_views

    case, data, mesh_path = scene
    out = str(tmp_path / "cube.obj")
    res = run_cli("--texture_size", "64", "--check", mesh_path, data, out)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    keys, values = parse(res.stdout)
    assert keys == KEYS + ["reprojection_psnr"] * 6 + ["reprojection_psnr_mean"]
    tris = torch.from_numpy(read_mesh(mesh_path)).cuda()
    assert np.array_equal(tris.cpu().numpy(), case.tris)
    cameras, images, _ = read_views(data)
    atlas = TextureAtlas(tris, 64)
    texture, info = bake_views(atlas, TriangleMesh(tris), cameras, images, verbose=False)
    want = dict(faces=12, texture_size=63, cell=21, views=6, offset=f"{info['offset']:.9g}",
                **{k: info[k] for k in KEYS[5:]})
    assert values == {k: str(v) for k, v in want.items()}
    assert info["seen"] == 2646 and np.array_equal(texture.cpu().numpy(), case.baked()[0])
    for ext in (".obj", ".mtl", ".png"):
        assert os.path.exists(out[:-4] + ext)
    with Image.open(out[:-4] + ".png") as image:
        assert np.array_equal(np.asarray(image), texture.cpu().numpy())
    assert np.array_equal(read_mesh(out), case.tris)
    text = open(out).read()
    assert text.count("\nvt ") == 36 and text.count("\nv ") == 8  # welded back to the cube's corners
    assert "map_Kd cube.png" in open(out[:-4] + ".mtl").read()
    psnr = [float(m) for m in re.findall(r"^reprojection_psnr=(\S+) \S+\.png$", res.stdout, flags=re.M)]
    assert len(psnr) == 6 and all(np.isfinite(psnr))
    mean = float(re.search(r"^reprojection_psnr_mean=(\S+)$", res.stdout, flags=re.M).group(1))
    assert abs(mean - sum(psnr) / 6) < 1e-9


def test_cli_simplifies_first_and_limits_the_views(scene, tmp_path):
    from learn_nerf.mesh_metrics import read_mesh
    from learn_nerf.raycast import TriangleMesh
    from learn_nerf.simplify import simplify

    case, data, _ = scene
    # the sphere of 1,280 faces, so that there is something to simplify
    import raycast_reference as RC
    from learn_nerf.mesh import write_stl

    sphere = RC.icosphere(3, radius=0.7)
    mesh_path = str(tmp_path / "sphere.stl")
    write_stl(mesh_path, sphere.reshape(-1, 3), np.arange(3 * len(sphere)).reshape(-1, 3))
    out = str(tmp_path / "small.obj")
    res = run_cli("--texture_size", "128", "--target_faces", "200", "--max_views", "4", mesh_path, data, out)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    keys, values = parse(res.stdout)
    assert keys == KEYS and values["views"] == "4"
    small = simplify(read_mesh(mesh_path), target_faces=200, device="cuda")
    want = small.verts[small.faces.long()].cpu().numpy()
    assert 0 < len(want) <= 200 and int(values["faces"]) == len(want)
    assert np.array_equal(read_mesh(out), want)
    assert TriangleMesh(torch.from_numpy(want).cuda()).n == len(want)


def test_cli_refuses_a_texture_that_is_too_small(scene, tmp_path):
    case, data, mesh_path = scene
    out = str(tmp_path / "none.obj")
    res = run_cli("--texture_size", "17", mesh_path, data, out)
    assert res.returncode != 0
    assert "too small for 12 faces" in res.stderr and "18 x 18" in res.stderr and "--target_faces" in res.stderr
    assert not os.path.exists(out) and not os.path.exists(out[:-4] + ".png")

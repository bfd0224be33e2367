"""
CPU checks of the mesh export (csrc/mesh.hip, learn_nerf/mesh.py, scripts/marching_cubes.py): the compile-time case
table against its rules and against the independent generator of tests/mesh_reference.py, known answers of the
restatement the GPU tests compare against, the reference's grid and output frames, the OBJ / STL writers and the
command line.
"""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import mesh_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "learn-nerf_amd")
SCRIPT = os.path.join(PKG, "learn_nerf", "scripts", "marching_cubes.py")


def sphere(n, r, centre=None):
    c = np.full(3, (n - 1) / 2) if centre is None else np.asarray(centre, np.float64)
    g = np.indices((n, n, n)).astype(np.float64)
    return (r - np.sqrt(((g - c[:, None, None, None]) ** 2).sum(0))).astype(np.float32)


def test_case_table_follows_its_rules_and_matches_the_library():
    from learn_nerf import _lib

    lib_table = np.zeros((256, 16), dtype=np.int8)
    assert _lib.lib().lnrf_mc_case_table(lib_table.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(lib_table, M.TABLE)
    assert M.NTRI[0] == 0 and M.NTRI[255] == 0 and M.NTRI.max() <= 5
    for case in range(256):
        row = lib_table[case].tolist()
        n = row.index(-1)
        assert n % 3 == 0 and all(e == -1 for e in row[n:])
        crossing = {e for e in range(12)
                    if (case >> int(M.EDGE_LO[e])) & 1 != (case >> int(M.EDGE_LO[e] | 1 << M.EDGE_AXIS[e])) & 1}
        assert set(row[:n]) == crossing, case  # only crossing edges, and every one of them


@pytest.mark.parametrize("shape", [(7, 9, 5), (11, 11, 11), (3, 4, 2)])
@pytest.mark.parametrize("seed", range(4))
def test_random_padded_fields_give_closed_oriented_meshes(shape, seed):
    vol = np.pad(np.random.default_rng(seed).random(shape, dtype=np.float32), 1)
    verts, faces = M.marching_cubes(vol, 0.5)
    assert len(faces) > 0 and faces.max() < len(verts)
    assert M.is_balanced(faces)


def test_sphere_known_answers():
    r = 6.0
    verts, faces = M.marching_cubes(np.pad(sphere(20, r), 1, constant_values=-1), 0.0)
    assert M.is_closed_oriented(faces)
    assert M.euler_characteristic(verts, faces) == 2 and M.components(faces) == 1
    vol = M.signed_volume(verts, faces)
    assert abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.03, vol
    radii = np.sqrt(((verts - 1 - 9.5) ** 2).sum(1))
    assert np.abs(radii - r).max() < 0.05


def test_torus_two_spheres_empty_and_full():
    g = np.indices((40, 40, 40)).astype(np.float64) - 19.5
    ring = np.sqrt(g[0] ** 2 + g[1] ** 2) - 10.0
    torus = (4.0 - np.sqrt(ring ** 2 + g[2] ** 2)).astype(np.float32)
    verts, faces = M.marching_cubes(np.pad(torus, 1, constant_values=-1), 0.0)
    assert M.is_closed_oriented(faces) and M.euler_characteristic(verts, faces) == 0
    assert abs(M.signed_volume(verts, faces) / (2 * np.pi ** 2 * 10.0 * 4.0 ** 2) - 1) < 0.03

    two = np.maximum(sphere(30, 5.0, (8, 8, 8)), sphere(30, 6.0, (20, 19, 21)))
    verts, faces = M.marching_cubes(two, 0.0)
    assert M.is_closed_oriented(faces) and M.components(faces) == 2

    for vol in (np.zeros((5, 6, 7), np.float32), np.ones((5, 6, 7), np.float32)):
        verts, faces = M.marching_cubes(vol, 0.5)
        assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_every_single_cell_case_has_the_tables_triangles():
    for case in range(256):
        cell = np.array([(case >> c) & 1 for c in range(8)], np.float32).reshape(2, 2, 2).transpose(2, 1, 0)
        verts, faces = M.marching_cubes(cell, 0.5)
        assert len(faces) == M.NTRI[case], case
        assert ((verts == 0) | (verts == 0.5) | (verts == 1)).all()


def test_grid_coordinates_are_the_references_bit_for_bit():
    import torch

    from learn_nerf.mesh import grid_coordinates

    lo, hi, r = (-1.3, 0.1, -2.0), (0.7, 2.9, 1.5), 7
    want = M.grid_coordinates(lo, hi, r)
    full = grid_coordinates(lo, hi, r, device="cpu").numpy()
    assert full.dtype == np.float32 and np.array_equal(full.view(np.uint32), want.view(np.uint32))
    part = grid_coordinates(lo, hi, r, start=50, count=123, device="cpu").numpy()
    assert np.array_equal(part.view(np.uint32), want[50:173].view(np.uint32))
    assert np.array_equal(full[-1], np.float32(hi)) and np.array_equal(full[0], np.float32(lo))
    assert np.array_equal(full[1], np.float32([lo[0], lo[1], np.linspace(lo[2], hi[2], r)[1]]))
    assert isinstance(grid_coordinates(lo, hi, r, 0, 0, device="cpu"), torch.Tensor)


def test_reference_frame_world_frame_and_face_flip():
    from learn_nerf.mesh import reference_frame, world_frame

    verts = np.array([[1, 2, 3], [4, 5, 6], [2, 2, 5]], np.float32)
    v, f = reference_frame(verts, np.array([[0, 1, 2]], np.int32), (0, 0, 0), (2, 4, 8), 4)
    # swapped: (3,2,1) (6,5,4) (5,2,2); scaled by (0.5, 1, 2): (1.5,2,2) (3,5,8) (2.5,2,4); centre (2.25, 3.5, 5)
    assert np.array_equal(v, np.array([[-0.75, -1.5, -3], [0.75, 1.5, 3], [0.25, -1.5, -1]], np.float32))
    assert v.dtype == np.float32 and f.dtype == np.int32 and f.tolist() == [[0, 2, 1]]

    sv, sf = M.marching_cubes(np.pad(sphere(12, 4.0), 1, constant_values=-1), 0.0)
    rv, rf = reference_frame(sv, sf, (-1, -2, -3), (1, 2, 3), 12)
    assert M.signed_volume(rv, rf) > 0 and M.signed_volume(rv, sf) < 0

    w = world_frame(np.array([[1, 1, 1], [8, 8, 8], [4.5, 1, 8]], np.float32), (-1, 0, 2), (1, 3, 9), 8)
    assert np.allclose(w, [[-1, 0, 2], [1, 3, 9], [0, 0, 9]], atol=1e-6) and w.dtype == np.float32
    assert M.signed_volume(world_frame(sv, (-1, -1, -1), (1, 1, 1), 12), sf) > 0


def test_obj_text_is_the_references(tmp_path):
    from learn_nerf.mesh import write_obj

    path = str(tmp_path / "m.obj")
    write_obj(path, np.array([[0, 0.5, 1.25], [-2, 3.5, 1e-7]], np.float32), np.array([[0, 1, 0]], np.int32))
    assert open(path).read() == "v 0.00000 0.50000 1.25000\nv -2.00000 3.50000 0.00000\nf 1 2 1\n"


def test_stl_layout_and_outward_unit_normals(tmp_path):
    from learn_nerf.mesh import write_stl

    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [0, 1, 1]], np.int32)  # last one degenerate
    assert M.signed_volume(verts, faces) > 0
    path = str(tmp_path / "m.stl")
    write_stl(path, verts, faces)
    blob = open(path, "rb").read()
    assert len(blob) == 84 + 50 * len(faces)
    assert blob[:80] == b"\x00" * 80 and struct.unpack_from("<I", blob, 80)[0] == len(faces)
    rec = np.frombuffer(blob, dtype=[("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("a", "<u2")], offset=84)
    assert np.array_equal(rec["v"], verts[faces]) and (rec["a"] == 0).all()
    n = rec["n"].astype(np.float64)
    assert np.allclose(np.linalg.norm(n[:4], axis=1), 1, atol=1e-6)
    centroid = verts.mean(0)
    assert (np.einsum("ij,ij->i", n[:4], verts[faces[:4]].mean(1) - centroid) > 0).all()
    assert np.array_equal(n[4], np.zeros(3))


def run_cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, SCRIPT, *args], env=env, capture_output=True, text=True, timeout=300)


def test_cli_help_shows_the_references_defaults():
    res = run_cli("--help")
    assert res.returncode == 0, res.stderr
    text = " ".join(res.stdout.split())
    for flag, default in (("--batch_size", "1024"), ("--resolution", "32"), ("--threshold", "0.9"),
                          ("--model_path", "nerf.pkl")):
        assert f"{flag} " in text and f"(default: {default})" in text, flag
    assert "rays per batch" in text and "--world_coords" in text and "--precision" in text
    assert "metadata_json" in text and "output_obj" in text


def test_cli_bad_extension_fails_before_loading_anything(tmp_path):
    res = run_cli("--model_path", str(tmp_path / "missing.pkl"), str(tmp_path / "missing.json"),
                  str(tmp_path / "mesh.ply"))
    assert res.returncode == 2
    assert ".obj or .stl" in res.stderr and "loading" not in res.stdout

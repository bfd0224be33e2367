"""
GPU marching cubes (lnrf_mc_count / lnrf_mc_emit) against the NumPy restatement of tests/mesh_reference.py: identical
faces and bit-identical vertices, deterministic, no unwritten memory read; density_grid of every model family against
model.apply; and a model whose density has a known surface through the whole model-to-mesh path.
"""
import numpy as np
import pytest
import torch

import mesh_reference as M

pytestmark = pytest.mark.gpu


def gpu_mc(vol, level):
    from learn_nerf.mesh import marching_cubes

    verts, faces = marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, np.float32)).cuda(), level)
    return verts.cpu().numpy(), faces.cpu().numpy()


def assert_same(vol, level):
    rv, rf = M.marching_cubes(vol, level)
    gv, gf = gpu_mc(vol, level)
    assert gf.dtype == np.int32 and gf.shape == rf.shape and np.array_equal(gf, rf)
    assert gv.dtype == np.float32 and gv.shape == rv.shape
    nan = np.isnan(rv)
    assert np.array_equal(nan, np.isnan(gv))
    assert np.array_equal(gv[~nan].view(np.uint32), rv[~nan].view(np.uint32))
    return gv, gf


def test_sphere_and_odd_shaped_noise():
    g = np.indices((20, 20, 20)).astype(np.float64) - 9.5
    sphere = (6.0 - np.sqrt((g ** 2).sum(0))).astype(np.float32)
    _, faces = assert_same(np.pad(sphere, 1, constant_values=-1), 0.0)
    assert M.is_closed_oriented(faces)
    noise = np.random.default_rng(1).random((40, 17, 23), dtype=np.float32)
    _, faces = assert_same(noise, 0.5)
    assert len(faces) > 1000


def test_all_256_cases_and_levels_nan_empty_full():
    for case in range(256):
        cell = np.array([(case >> c) & 1 for c in range(8)], np.float32).reshape(2, 2, 2).transpose(2, 1, 0)
        cell = cell * np.float32(0.75) + np.float32(0.125)
        _, faces = assert_same(cell, 0.5)
        assert len(faces) == M.NTRI[case]
    rng = np.random.default_rng(2)
    at_level = rng.choice(np.float32([0.25, 0.5, 0.75]), size=(9, 10, 11))
    _, faces = assert_same(at_level, 0.5)
    assert len(faces) > 0
    with_nan = rng.random((12, 13, 14), dtype=np.float32)
    with_nan[rng.random(with_nan.shape) < 0.1] = np.nan
    gv, _ = assert_same(with_nan, 0.5)
    assert np.isnan(gv).any()
    for vol in (np.zeros((5, 6, 7), np.float32), np.ones((5, 6, 7), np.float32)):
        gv, gf = assert_same(vol, 0.5)
        assert gv.shape == (0, 3) and gf.shape == (0, 3)


def test_large_volume_spans_many_workgroups():
    n = 300  # 27M points = 26,368 tiles: four rounds of the tile scan (the last partial), grid-stride workgroups
    ax = np.arange(n, dtype=np.float32)
    vol = (np.sin(ax / 7)[:, None, None] + np.sin(ax / 9)[None, :, None] + np.sin(ax / 11)[None, None, :])
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    _, faces = assert_same(vol, 0.3)
    assert len(faces) > 1_000_000


def test_deterministic_and_reads_only_what_it_wrote():
    from learn_nerf import _lib as L
    from learn_nerf.mesh import marching_cubes

    vol = torch.from_numpy(np.random.default_rng(3).random((40, 17, 23), dtype=np.float32)).cuda()
    v1, f1 = marching_cubes(vol, 0.5)
    v2, f2 = marching_cubes(vol, 0.5)
    assert torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(f1, f2)

    lib = L.lib()
    nx, ny, nz = vol.shape
    scratch = torch.full((lib.lnrf_mc_scratch_bytes(nx, ny, nz),), 0xFF, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    L.check(lib.lnrf_mc_count(L.ptr(vol), nx, ny, nz, 0.5, L.ptr(scratch, torch.uint8), L.ptr(counts, torch.int64),
                              L.stream()))
    assert counts.tolist() == [v1.shape[0], f1.shape[0]]
    nv, nf = v1.shape[0], f1.shape[0]
    verts = torch.full((nv + 5, 3), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    faces = torch.full((nf + 5, 3), -1, dtype=torch.int32, device="cuda")
    L.check(lib.lnrf_mc_emit(L.ptr(vol), nx, ny, nz, 0.5, L.ptr(scratch, torch.uint8), nv, nf, L.ptr(verts),
                             L.ptr(faces, torch.int32), L.stream()))
    assert torch.equal(verts[:nv].view(torch.int32), v1.view(torch.int32)) and torch.equal(faces[:nf], f1)
    assert (verts[nv:].view(torch.int32) == -1).all() and (faces[nf:] == -1).all()  # nothing beyond the counts
    # counts smaller than the scratch's: the emit stays inside them
    L.check(lib.lnrf_mc_emit(L.ptr(vol), nx, ny, nz, 0.5, L.ptr(scratch, torch.uint8), nv // 2, nf // 2,
                             L.ptr(verts), L.ptr(faces, torch.int32), L.stream()))
    torch.cuda.synchronize()
    assert (verts[nv:].view(torch.int32) == -1).all() and (faces[nf:] == -1).all()
    assert lib.lnrf_mc_count(L.ptr(vol), 1, ny, nz, 0.5, L.ptr(scratch, torch.uint8), L.ptr(counts, torch.int64),
                             L.stream()) == -1
    assert lib.lnrf_mc_emit(L.ptr(vol), nx, ny, nz, 0.5, L.ptr(scratch, torch.uint8), 2 ** 31, nf, L.ptr(verts),
                            L.ptr(faces, torch.int32), L.stream()) == -2  # V does not fit in int32 ids


BOX = ((-1.5, -1.2, -1.0), (1.0, 1.3, 1.1))


def make_family(name):
    from learn_nerf.instant_ngp import InstantNGPModel, InstantNGPRefNERFModel
    from learn_nerf.model import NeRFModel
    from learn_nerf.ref_nerf import RefNERFModel

    grid = dict(table_sizes=[2 ** 12] * 4, grid_sizes=[4, 8, 16, 32], bbox_min=BOX[0], bbox_max=BOX[1])
    model = {"nerf": lambda: NeRFModel(), "nerf_fp32": lambda: NeRFModel(precision="fp32"),
             "ngp": lambda: InstantNGPModel(**grid), "refnerf": lambda: RefNERFModel(sh_degree=4),
             "ngp_refnerf": lambda: InstantNGPRefNERFModel(sh_degree=4, **grid)}[name]()
    params = model.init(dict(params=7))["params"]
    if name.startswith("ngp"):  # the U(-1e-4, 1e-4) table init would make the density nearly constant
        flat = model.flat(params)
        nt = model.encoding().num_table_floats()
        gen = torch.Generator().manual_seed(7)
        flat[:nt] = ((torch.rand(nt, generator=gen) * 2 - 1) * 0.5).to(flat.device)
    return model, params


@pytest.mark.parametrize("name", ["nerf", "nerf_fp32", "ngp", "refnerf", "ngp_refnerf"])
def test_density_grid_is_model_apply_on_the_references_grid(name):
    from learn_nerf.mesh import density_grid

    model, params = make_family(name)
    r = 17
    small = density_grid(model, params, *BOX, r, 1000)
    large = density_grid(model, params, *BOX, r, 4096)
    assert small.shape == (r, r, r) and torch.isfinite(small).all()
    x = torch.from_numpy(M.grid_coordinates(*BOX, r)).cuda()
    density, _, _ = model.apply(dict(params=params), x, torch.zeros_like(x))
    want = density.reshape(r, r, r)
    assert torch.equal(small, large), (small - large).abs().max().item()
    assert torch.equal(small, want), (small - want).abs().max().item()
    assert small.std().item() > 0


def analytic_model():
    from learn_nerf.model import NeRFModel

    model = NeRFModel()
    params = model.init(dict(params=0))["params"]
    with torch.no_grad():
        M.set_analytic_nerf(params)
    return model, params


def test_known_surface_through_the_whole_path():
    from learn_nerf.mesh import extract_mesh, world_frame

    model, params = analytic_model()
    r, box = 64, ((-1, -1, -1), (1, 1, 1))
    verts, faces, largest = extract_mesh(model, params, *box, r, 4096, 0.9)
    assert 0.9 < largest < 1
    v = world_frame(verts.cpu().numpy(), *box, r)
    f = faces.cpu().numpy()
    assert M.is_closed_oriented(f) and M.components(f) == 1 and M.euler_characteristic(v, f) == 2
    # exact arithmetic gives 3e-4 at spacing 2/63 (linear interpolation of the occupancy along grid edges)
    level = np.cos(v.astype(np.float64)).sum(1)
    assert np.abs(level - M.ANALYTIC_K).max() < 2e-3
    assert abs(M.signed_volume(v, f) / M.analytic_volume() - 1) < 0.03

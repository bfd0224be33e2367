"""
lnrf_tsdf_* and learn_nerf.tsdf.TsdfVolume on the GPU against the NumPy float32 restatement (tests/tsdf_reference.py):
every state array, the volume, the mesh and its colours are equal bit for bit, for the analytic sphere, for a grid with
tail lanes and unequal axes under awkward views, for every split of the views over launches, and on poisoned or
guarded outputs.
"""
import functools

import numpy as np
import pytest
import torch

import mesh_reference as M
import tsdf_reference as R
from gpu_poison import PATTERNS, poisoned

pytestmark = pytest.mark.gpu
MAX_DEPTH = 10.0
STATE = ("sum_t", "n_obs", "behind", "rgb_sum", "n_col")
ODD_DIMS = (33, 20, 17)  # 9 x 5 x 5 tiles of 4^3 voxels, the last ones along i and k one voxel thick; 57 workgroups
BIG_DIMS = (130, 128, 133)  # 35904 tiles for the 32768 waves of the largest launch; 2.3 M padded points for 2 M lanes


def reference(dims, cameras, depths, colors, carve=True):
    from learn_nerf.tsdf import pack_views

    views = pack_views(cameras, [(d.shape[1], d.shape[0]) for d in depths])
    axes = R.grid_axes(R.BBOX_MIN, R.BBOX_MAX, dims)
    trunc = R.truncation(R.BBOX_MIN, R.BBOX_MAX, dims, 3.0)
    state, _ = R.integrate(axes, views, depths, colors, trunc, MAX_DEPTH, carve=carve)
    return state


def fuse(dims, cameras, depths, colors, carve=True, chunks=None):
    from learn_nerf.tsdf import TsdfVolume

    vol = TsdfVolume(R.BBOX_MIN, R.BBOX_MAX, dims, truncation_voxels=3.0, max_depth=MAX_DEPTH, carve=carve,
                     device="cuda")
    assert vol.trunc == float(R.truncation(R.BBOX_MIN, R.BBOX_MAX, dims, 3.0))
    start = 0
    for count in chunks or [len(cameras)]:
        vol.integrate(cameras[start:start + count], depths[start:start + count], colors[start:start + count])
        start += count
    assert start == len(cameras) == vol.n_views
    return vol


def assert_state_equal(vol, state):
    for name in STATE:
        got = getattr(vol, name).cpu()
        want = torch.from_numpy(state[name])
        assert got.dtype == want.dtype and torch.equal(got.reshape(want.shape), want), name


def assert_mesh_equal(vol, state, dims, unseen="inside"):
    """Volume, marching cubes and vertex colours of `vol` against the restatement -> the reference's faces."""
    want_vol = R.volume(state, dims, unseen)
    got_vol = vol.volume(unseen)
    assert torch.equal(got_vol.cpu(), torch.from_numpy(want_vol))
    verts, faces = M.marching_cubes(want_vol, 0.0)
    colors, missing = R.vertex_colors(verts, dims, state)
    got_verts, got_faces, got_colors, info = vol.extract(unseen=unseen)
    assert torch.equal(torch.from_numpy(got_verts), torch.from_numpy(R.world_vertices(verts, R.BBOX_MIN, R.BBOX_MAX, dims)))
    assert torch.equal(torch.from_numpy(got_faces), torch.from_numpy(faces))
    assert torch.equal(torch.from_numpy(got_colors), torch.from_numpy(colors))
    assert info["uncoloured"] == missing
    seen = state["n_obs"] > 0
    solid = ~seen & (state["behind"] != 0) & (unseen == "inside")
    assert (info["observed"], info["unseen_inside"]) == (int(seen.sum()), int(solid.sum()))
    assert info["observed"] + info["unseen_inside"] + info["unseen_outside"] == seen.size
    return faces


@functools.lru_cache(maxsize=None)
def sphere():
    dims = (32, 32, 32)
    scene = R.sphere_scene(R.ICOSAHEDRON, 64, 64, MAX_DEPTH)
    return dims, scene, reference(dims, *scene)


@functools.lru_cache(maxsize=None)
def odd_scene():
    """Views of 40 x 25 with x_fov != y_fov around the sphere, one of them with non-orthonormal axes."""
    cameras = [R.look_at_camera(d, x_fov=0.7, y_fov=0.45) for d in R.AXES6[:5]]
    cameras.append(R.look_at_camera((1, 1, 1), x_fov=0.7, y_fov=0.5, skew=0.15))
    images = [R.render_sphere(c, 40, 25, MAX_DEPTH) for c in cameras]
    return cameras, [i[0] for i in images], [i[1] for i in images]


def test_sphere_scene_equals_the_restatement():
    dims, scene, state = sphere()
    vol = fuse(dims, *scene)
    assert_state_equal(vol, state)
    faces = assert_mesh_equal(vol, state, dims, "inside")
    assert M.is_closed_oriented(faces) and M.components(faces) == 1
    faces_outside = assert_mesh_equal(vol, state, dims, "outside")
    assert len(faces_outside) > len(faces)


def test_tail_lanes_unequal_axes_and_skewed_camera():
    scene = odd_scene()
    state = reference(ODD_DIMS, *scene)
    assert (state["n_obs"] > 0).sum() > 1000 and state["behind"].sum() > 100 and state["n_col"].sum() > 100
    vol = fuse(ODD_DIMS, *scene)
    assert_state_equal(vol, state)
    assert_mesh_equal(vol, state, ODD_DIMS)


def test_grid_larger_than_the_launch():
    """More tiles than the largest launch has waves, and more padded points than lanes: the strided loops run twice
    for some waves and lanes."""
    cameras, depths, colors = [x[4:6] for x in odd_scene()]
    state = reference(BIG_DIMS, cameras, depths, colors)
    vol = fuse(BIG_DIMS, cameras, depths, colors)
    assert_state_equal(vol, state)
    assert torch.equal(vol.volume().cpu(), torch.from_numpy(R.volume(state, BIG_DIMS)))


@pytest.mark.parametrize("chunks", [(5, 5, 2), (1,) * 12], ids=["5+5+2", "one-per-launch"])
def test_any_split_of_the_views_gives_the_same_bits(chunks):
    dims, scene, state = sphere()
    assert_state_equal(fuse(dims, *scene, chunks=list(chunks)), state)


def test_chunk_byte_budget_splits_without_changing_bits():
    dims, scene, state = sphere()
    from learn_nerf.tsdf import TsdfVolume

    vol = TsdfVolume(R.BBOX_MIN, R.BBOX_MAX, dims, max_depth=MAX_DEPTH, device="cuda")
    vol.integrate(*scene, chunk_bytes=5 * 64 * 64 * 5)  # 5 views per launch
    assert_state_equal(vol, state)


def test_camera_inside_the_box():
    """Voxels behind the camera have s <= 0 and are skipped; the ones in front are carved or hit."""
    cameras, depths, colors = [list(x) for x in odd_scene()]
    inside = R.look_at_camera((0, 0, 1), x_fov=0.7, y_fov=0.45, origin=(0.1, 0.2, -0.9))
    depth, color = R.render_sphere(inside, 40, 25, MAX_DEPTH)
    alone = reference(ODD_DIMS, [inside], [depth], [color])
    assert 0 < (alone["n_obs"] > 0).sum() < alone["n_obs"].size // 2  # most of the grid is behind it or off-frustum
    cameras.append(inside), depths.append(depth), colors.append(color)
    state = reference(ODD_DIMS, cameras, depths, colors)
    vol = fuse(ODD_DIMS, cameras, depths, colors)
    assert_state_equal(vol, state)
    assert_state_equal(fuse(ODD_DIMS, [inside], [depth], [color]), alone)


def test_view_whose_frustum_misses_the_box():
    away = R.look_at_camera((0, 0, 1), origin=(0.0, 0.0, 3.0))  # beyond the box, looking further away
    sideways = R.look_at_camera((0, 1, 0), x_fov=0.2, y_fov=0.2, origin=(5.0, 0.0, 0.0))  # in front, but off to the side
    cameras = [away, sideways]
    depths = [np.full((25, 40), 1000, np.uint16)] * 2
    colors = [np.full((25, 40, 3), 200, np.uint8)] * 2
    state = reference(ODD_DIMS, cameras, depths, colors)
    assert not any(state[name].any() for name in STATE)
    vol = fuse(ODD_DIMS, cameras, depths, colors)
    assert_state_equal(vol, state)
    assert not bool((vol.volume() > 0).any())
    verts, faces, vertex_colors, info = vol.extract()
    assert len(verts) == 0 and len(faces) == 0 and info["observed"] == 0 and info["uncoloured"] == 0


@pytest.mark.parametrize("carve", [True, False])
def test_view_without_a_hit(carve):
    cam = R.look_at_camera((1, 0, 0), x_fov=0.7, y_fov=0.45)
    depths = [np.full((25, 40), R.NO_DEPTH, np.uint16)]
    colors = [np.zeros((25, 40, 3), np.uint8)]
    state = reference(ODD_DIMS, [cam], depths, colors, carve=carve)
    if carve:
        seen = state["n_obs"] == 1
        assert seen.sum() > 1000 and np.array_equal(state["sum_t"], seen.astype(np.float32))
    else:
        assert not state["n_obs"].any() and not state["sum_t"].any()
    assert not state["behind"].any() and not state["n_col"].any()
    assert_state_equal(fuse(ODD_DIMS, [cam], depths, colors, carve=carve), state)


def test_depth_zero_view_puts_its_frustum_behind():
    cam = R.look_at_camera((1, 0, 0), x_fov=0.7, y_fov=0.45)
    depths = [np.zeros((25, 40), np.uint16)]
    colors = [np.full((25, 40, 3), 9, np.uint8)]
    state = reference(ODD_DIMS, [cam], depths, colors)
    assert state["behind"].sum() > 1000 and not state["n_obs"].any() and not state["n_col"].any()
    vol = fuse(ODD_DIMS, [cam], depths, colors)
    assert_state_equal(vol, state)
    assert torch.equal(vol.volume("inside").cpu(), torch.from_numpy(R.volume(state, ODD_DIMS, "inside")))
    assert torch.equal(vol.volume("outside").cpu(), torch.from_numpy(R.volume(state, ODD_DIMS, "outside")))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_outputs_are_fully_written_under_poison(pattern):
    """The volume, the colours and everything marching cubes allocates start as the byte pattern: a point or a vertex
    that the kernels left unwritten would keep it."""
    scene = odd_scene()
    state = reference(ODD_DIMS, *scene)
    vol = fuse(ODD_DIMS, *scene)
    with poisoned(pattern) as rec:
        assert_mesh_equal(vol, state, ODD_DIMS)
    assert rec.empties >= 2


def test_nothing_is_written_beyond_the_outputs():
    """Raw entry points on buffers with a guard behind every output: the guard keeps its sentinel."""
    from learn_nerf import _lib as L
    from learn_nerf.tsdf import pack_views

    cameras, depths, colors = odd_scene()
    state = reference(ODD_DIMS, cameras, depths, colors)
    nx, ny, nz = ODD_DIMS
    n, guard = nx * ny * nz, 1024
    dev = torch.device("cuda")
    views = torch.from_numpy(pack_views(cameras, [(40, 25)] * len(cameras)).view(np.uint8).copy()).to(dev)
    depth = torch.from_numpy(np.concatenate([d.reshape(-1) for d in depths]).view(np.int16)).to(dev)
    color = torch.from_numpy(np.concatenate([c.reshape(-1) for c in colors])).to(dev)
    axes = [torch.from_numpy(a).to(dev) for a in R.grid_axes(R.BBOX_MIN, R.BBOX_MAX, ODD_DIMS)]

    def guarded(count, dtype, sentinel, zero=True):
        t = torch.full((count + guard,), sentinel, dtype=dtype, device=dev)
        if zero:
            t[:count] = 0
        return t

    sum_t, n_obs = guarded(n, torch.float32, -7.5), guarded(n, torch.int32, -77)
    behind, rgb_sum, n_col = guarded(n, torch.uint8, 0xAB), guarded(3 * n, torch.int32, -77), guarded(n, torch.int32, -77)
    lib = L.lib()
    trunc = float(R.truncation(R.BBOX_MIN, R.BBOX_MAX, ODD_DIMS, 3.0))
    L.check(lib.lnrf_tsdf_integrate(L.ptr(axes[0]), L.ptr(axes[1]), L.ptr(axes[2]), nx, ny, nz,
                                    L.ptr(views, torch.uint8), len(cameras), L.ptr(depth, torch.int16),
                                    L.ptr(color, torch.uint8), trunc, MAX_DEPTH, 1, L.ptr(sum_t),
                                    L.ptr(n_obs, torch.int32), L.ptr(behind, torch.uint8), L.ptr(rgb_sum, torch.int32),
                                    L.ptr(n_col, torch.int32), L.stream()), "integrate")
    for name, t, count, sentinel in (("sum_t", sum_t, n, -7.5), ("n_obs", n_obs, n, -77), ("behind", behind, n, 0xAB),
                                     ("rgb_sum", rgb_sum, 3 * n, -77), ("n_col", n_col, n, -77)):
        assert torch.equal(t[:count].cpu(), torch.from_numpy(state[name].reshape(-1))), name
        assert bool((t[count:] == sentinel).all()), name
    total = (nx + 2) * (ny + 2) * (nz + 2)
    out = guarded(total, torch.float32, -7.5, zero=False)
    L.check(lib.lnrf_tsdf_volume(L.ptr(sum_t), L.ptr(n_obs, torch.int32), L.ptr(behind, torch.uint8), nx, ny, nz, 1,
                                 L.ptr(out), L.stream()), "volume")
    want_vol = R.volume(state, ODD_DIMS, "inside")
    assert torch.equal(out[:total].cpu(), torch.from_numpy(want_vol.reshape(-1)))
    assert bool((out[total:] == -7.5).all())
    verts, _ = M.marching_cubes(want_vol, 0.0)
    want_colors, want_missing = R.vertex_colors(verts, ODD_DIMS, state)
    v = len(verts)
    rgb_out = guarded(3 * v, torch.float32, -7.5, zero=False)
    missing = torch.full((1 + guard,), -77, dtype=torch.int32, device=dev)
    L.check(lib.lnrf_tsdf_vertex_colors(L.ptr(torch.from_numpy(verts).to(dev)), v, nx, ny, nz,
                                        L.ptr(rgb_sum, torch.int32), L.ptr(n_col, torch.int32), L.ptr(rgb_out),
                                        L.ptr(missing, torch.int32), L.stream()), "vertex_colors")
    assert torch.equal(rgb_out[:3 * v].cpu(), torch.from_numpy(want_colors.reshape(-1)))
    assert bool((rgb_out[3 * v:] == -7.5).all())
    assert int(missing[0]) == want_missing and bool((missing[1:] == -77).all())
    # no vertices: only the counter is cleared
    L.check(lib.lnrf_tsdf_vertex_colors(None, 0, nx, ny, nz, L.ptr(rgb_sum, torch.int32), L.ptr(n_col, torch.int32),
                                        None, L.ptr(missing, torch.int32), L.stream()), "vertex_colors")
    assert int(missing[0]) == 0 and bool((missing[1:] == -77).all())


def test_dimension_errors_return_err_shape():
    from learn_nerf import _lib as L

    dev = torch.device("cuda")
    f = torch.zeros(64, device=dev)
    i = torch.zeros(64, dtype=torch.int32, device=dev)
    b = torch.zeros(64, dtype=torch.uint8, device=dev)
    h = torch.zeros(64, dtype=torch.int16, device=dev)
    lib = L.lib()
    P, I = L.ptr, lambda t: L.ptr(t, torch.int32)
    for dims in ((0, 2, 2), (2, 2, -3), (2 ** 31, 1, 1), (1300, 1300, 1300)):
        assert lib.lnrf_tsdf_integrate(P(f), P(f), P(f), *dims, P(b, torch.uint8), 1, P(h, torch.int16),
                                       P(b, torch.uint8), 0.1, MAX_DEPTH, 1, P(f), I(i), P(b, torch.uint8), I(i), I(i),
                                       L.stream()) == -2, dims
        assert lib.lnrf_tsdf_volume(P(f), I(i), P(b, torch.uint8), *dims, 1, P(f), L.stream()) == -2, dims
        assert lib.lnrf_tsdf_vertex_colors(P(f), 1, *dims, I(i), I(i), P(f), I(i), L.stream()) == -2, dims
    assert lib.lnrf_tsdf_integrate(P(f), P(f), P(f), 2, 2, 2, P(b, torch.uint8), -1, P(h, torch.int16),
                                   P(b, torch.uint8), 0.1, MAX_DEPTH, 1, P(f), I(i), P(b, torch.uint8), I(i), I(i),
                                   L.stream()) == -2
    assert lib.lnrf_tsdf_vertex_colors(P(f), 2 ** 31, 2, 2, 2, I(i), I(i), P(f), I(i), L.stream()) == -2
    torch.cuda.synchronize()
    assert not f.any() and not i.any() and not b.any()  # nothing ran
    with pytest.raises(ValueError, match="int32"):
        from learn_nerf.tsdf import TsdfVolume

        TsdfVolume(R.BBOX_MIN, R.BBOX_MAX, 1300, device="cuda")

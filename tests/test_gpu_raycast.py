"""
csrc/raycast.hip on the GPU against the NumPy brute force of tests/raycast_reference.py: closest (t, id) and occluded
are bit-identical on every mesh and ray set below, under two leaf sizes and over outputs pre-filled with 0x00, 0x41 and
0xFF bytes; input outside the stated domain raises in Python; TriangleMesh.render equals the NumPy shading byte for
byte, with pixels in shadow on a two-object scene.
"""
import math

import numpy as np
import pytest
import torch

import raycast_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
LEAVES = (4, 3)  # the default and a forced one
FILLS = (0x00, 0x41, 0xFF)


def _trace(tris, rays, t_min, t_max, leaf, fill):
    """closest and occluded of a fresh TriangleMesh with this leaf size, over outputs pre-filled with `fill` bytes."""
    from learn_nerf.raycast import TriangleMesh

    dev = torch.device("cuda")
    mesh = TriangleMesh(torch.from_numpy(np.ascontiguousarray(tris)).to(dev), leaf_size=leaf)
    r = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
    m = len(rays)
    lo = t_min if np.isscalar(t_min) else torch.from_numpy(np.asarray(t_min, dtype=F32)).to(dev)
    hi = t_max if np.isscalar(t_max) else torch.from_numpy(np.asarray(t_max, dtype=F32)).to(dev)
    t = torch.full((m,), fill, dtype=torch.uint8, device=dev).repeat_interleave(4).view(torch.float32)
    idx = torch.full((m,), fill, dtype=torch.uint8, device=dev).repeat_interleave(4).view(torch.int32)
    occ = torch.full((m,), fill, dtype=torch.uint8, device=dev)
    mesh.closest(r, lo, hi, out=(t, idx))
    mesh.occluded(r, lo, hi, out=occ)
    return t.cpu().numpy(), idx.cpu().numpy(), occ.cpu().numpy()


def check(tris, rays, t_min=0.0, t_max=math.inf, expect_hits=True):
    """The GPU equals the brute force bit for bit; returns the brute force's (t, id, occluded)."""
    tris, rays = np.asarray(tris, dtype=F32), np.asarray(rays, dtype=F32)
    ref_t, ref_id, ref_occ = R.brute_force(tris, rays, t_min, t_max)
    if expect_hits:
        assert (ref_id >= 0).any(), "the case exercises nothing: no ray hits"
    for leaf in LEAVES:
        for fill in FILLS if leaf == LEAVES[0] else FILLS[:1]:
            t, idx, occ = _trace(tris, rays, t_min, t_max, leaf, fill)
            assert np.array_equal(idx, ref_id), (leaf, fill, np.nonzero(idx != ref_id)[0][:8])
            assert np.array_equal(t.view(np.uint32), ref_t.view(np.uint32)), (leaf, fill)
            assert np.array_equal(occ, ref_occ), (leaf, fill, np.nonzero(occ != ref_occ)[0][:8])
    return ref_t, ref_id, ref_occ


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def _rays(origins, directions):
    origins = np.asarray(origins, dtype=F32).reshape(-1, 3)
    directions = np.broadcast_to(np.asarray(directions, dtype=F32).reshape(-1, 3), origins.shape)
    return np.stack([origins, directions], axis=1)


def _aimed(origins, targets):
    origins = np.broadcast_to(np.asarray(origins, dtype=F32).reshape(-1, 3), np.asarray(targets).reshape(-1, 3).shape)
    return _rays(origins, _unit(np.asarray(targets, dtype=np.float64).reshape(-1, 3) - origins.astype(np.float64)))


def ray_set(tris, seed=0, count=160):
    """Rays of every kind the kernel treats differently, around a mesh in about [-1, 1]^3."""
    rng = np.random.default_rng(seed)
    tris = np.asarray(tris, dtype=F32)
    lo, hi = tris.min(axis=(0, 1)).astype(np.float64), tris.max(axis=(0, 1)).astype(np.float64)
    mid, ext = (lo + hi) / 2, np.maximum(hi - lo, 0.5)
    sets = []
    # from outside toward random points of the box, and toward the triangles themselves
    outside = mid + _unit(rng.normal(size=(count, 3))) * 3.0
    sets.append(_aimed(outside, mid + rng.uniform(-0.5, 0.5, size=(count, 3)) * ext))
    pick = rng.integers(0, len(tris), size=count)
    w = rng.dirichlet(np.ones(3), size=count)
    sets.append(_aimed(outside, (tris[pick].astype(np.float64) * w[:, :, None]).sum(axis=1)))
    # exactly at vertices and at edge midpoints
    some = tris[rng.integers(0, len(tris), size=24)].astype(np.float64)
    sets.append(_aimed(mid + [2.5, 1.5, 2.0], some.reshape(-1, 3)))
    sets.append(_aimed(mid + [-2.0, 2.5, -1.5], ((some + np.roll(some, 1, axis=1)) / 2).reshape(-1, 3)))
    # axis-parallel (two zero components), both ways along each axis, through a lattice and through vertices
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = np.zeros(3)
            d[axis] = sign
            start = mid + rng.uniform(-0.55, 0.55, size=(16, 3)) * ext
            start = np.concatenate([start, some[:4, 0]])
            start[:, axis] = mid[axis] - sign * 3.0
            sets.append(_rays(start, d))
    # one zero component
    for axis in range(3):
        target = mid + rng.uniform(-0.5, 0.5, size=(16, 3)) * ext
        start = mid + _unit(rng.normal(size=(16, 3))) * 3.0
        start[:, axis] = target[:, axis]
        r = _aimed(start, target)
        r[:, 1, axis] = 0.0
        r[:, 1] = _unit(r[:, 1])
        sets.append(r)
    # origins inside the mesh's box
    inside = mid + rng.uniform(-0.3, 0.3, size=(48, 3)) * ext
    sets.append(_rays(inside, _unit(rng.normal(size=(48, 3)))))
    # rays that miss everything
    sets.append(_rays(outside[:16], _unit(outside[:16] - mid)))
    return np.concatenate(sets).astype(F32)


@pytest.fixture(scope="module")
def soup():
    return R.soup(5000, seed=1)


def test_one_triangle_and_two_that_share_an_edge():
    one = np.array([[[-1, -1, 0.2], [1, -1, 0.1], [0, 1, -0.3]]], dtype=F32)
    check(one, ray_set(one))
    two = np.array([[[-1, -1, 0], [1, -1, 0.5], [1, 1, 0]], [[-1, -1, 0], [1, 1, 0], [-1, 1, 0.5]]], dtype=F32)
    rays = ray_set(two)
    edge = _aimed([0.3, -0.2, 3.0], np.linspace([-1, -1, 0], [1, 1, 0], 33))  # along the shared edge
    check(two, np.concatenate([rays, edge]))


def test_cube_and_its_64x64_camera_view():
    from learn_nerf.raycast import camera_at, fit_distance

    tris = R.cube(0.5)
    check(tris, ray_set(tris))
    v = np.array([0.3, -0.8, 0.52])
    view = camera_at([-0.5] * 3, [0.5] * 3, v, fit_distance([-0.5] * 3, [0.5] * 3, v, 0.7), 0.7)
    rays = view.bare_rays(64, 64, device="cuda").cpu().numpy()
    _, idx, _ = check(tris, rays)
    assert 500 < (idx >= 0).sum() < 4096


def test_icosphere_1280():
    tris = R.icosphere(3)
    assert len(tris) == 1280
    _, idx, _ = check(tris, ray_set(tris, seed=2))
    assert len(np.unique(idx)) > 100


def test_soup_5000(soup):
    _, idx, _ = check(soup, ray_set(soup, seed=3))
    assert len(np.unique(idx)) > 50


def test_duplicated_triangles_tie_goes_to_the_lowest_index():
    base = R.icosphere(1)
    tris = np.concatenate([base, base[::-1], base])
    _, idx, _ = check(tris, ray_set(tris, seed=4))
    hit = idx[idx >= 0]
    assert len(hit) > 100 and (hit < 80).all()
    # every hit names the first of the three copies of its triangle
    first = {tri.tobytes(): i for i, tri in reversed(list(enumerate(tris)))}
    assert all(first[tris[i].tobytes()] == i for i in hit)


def test_zero_area_triangles_are_never_hit():
    """Degenerate triangles among the cube's.  Where an edge vector is 0 (a repeated first vertex, a point) the pinned
    det is exactly 0 and the triangle is never hit.  For e1 == e2 or three distinct collinear vertices det is rounding
    noise, so the pinned test itself accepts some rays aimed at the segment: whatever it does, the GPU does the same."""
    good = R.cube(0.5)
    p, q, r = np.array([0.1, 0.2, 0.9]), np.array([0.7, -0.3, 0.8]), np.array([-0.4, 0.6, 1.0])
    dead = np.array([[p, p, p], [p, p, q], [p, q, p], [q, p, p], [p, q, q], [p, (p + q) / 2, q], [r, r, r]], dtype=F32)
    tris = np.concatenate([dead[:3], good[:6], dead[3:], good[6:]])
    exact = [0, 1, 2, 12]  # [p p p], [p p q], [p q p], [r r r] within tris
    rays = np.concatenate([ray_set(tris, seed=5), _aimed([0.2, 0.1, 3.0], dead.reshape(-1, 3).astype(np.float64))])
    _, idx, _ = check(tris, rays)
    assert (idx >= 0).sum() > 100 and not np.isin(idx, exact).any()
    _, idx, _ = check(dead, rays, expect_hits=False)  # nothing but degenerate triangles
    assert not np.isin(idx, [0, 1, 2, 6]).any()


def test_coplanar_triangles_in_z0_have_flat_boxes():
    rng = np.random.default_rng(6)
    xy = rng.uniform(-1, 1, size=(40, 1, 2)) + rng.uniform(-0.2, 0.2, size=(40, 3, 2))
    tris = np.concatenate([xy, np.zeros((40, 3, 1))], axis=2).astype(F32)
    rays = ray_set(tris, seed=7)
    # rays lying in the plane z = 0: along x, along a diagonal, and from inside the set
    in_plane = np.concatenate([
        _rays(np.stack([np.full(9, -3.0), np.linspace(-1, 1, 9), np.zeros(9)], axis=1), [1.0, 0.0, 0.0]),
        _rays(np.stack([np.linspace(-3, -1, 9), np.full(9, -3.0), np.zeros(9)], axis=1), _unit([1.0, 1.0, 0.0])),
        _rays(tris[:8, 0], _unit([0.6, -0.8, 0.0]))])
    # and straight down through the plane, t exactly representable
    down = _rays(np.concatenate([tris[:8].mean(axis=1)[:, :2], np.full((8, 1), 2.0)], axis=1), [0.0, 0.0, -1.0])
    check(tris, np.concatenate([rays, in_plane, down]))
    _, in_plane_id, _ = R.brute_force(tris, in_plane)
    assert (in_plane_id < 0).all()  # det is exactly 0 for a ray in the plane


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 15, 17, 31, 33, 255, 257])
def test_triangle_counts_around_the_leaf_sizes_and_powers_of_two(soup, n):
    tris = soup[:n] * F32(4.0) - soup[:n, :1] * F32(3.0)  # the same soup with triangles four times the size
    check(tris, ray_set(tris, seed=n, count=48))


@pytest.mark.parametrize("m", [1, 63, 65, 257])
def test_ray_counts(m):
    tris = R.icosphere(1)
    check(tris, ray_set(tris, seed=8)[160:160 + m])  # from the rays aimed at the triangles


def test_windows_that_exclude_the_nearest_hit():
    tris = R.icosphere(2)
    rays = ray_set(tris, seed=9)
    t, idx, _ = R.brute_force(tris, rays)
    hit = idx >= 0
    assert hit.sum() > 100
    # t > t_min is strict: the nearest hit itself is excluded and the next one (the far side) is found
    t2, idx2, _ = check(tris, rays, np.where(hit, t, F32(0)).astype(F32), np.full(len(rays), np.inf, F32))
    assert (idx2[hit] != idx[hit]).all() and (t2[hit] > t[hit]).all() and (idx2 >= 0).sum() > 50
    # t < t_max is strict too: nothing is left in front of the nearest hit
    _, idx3, occ3 = check(tris, rays, np.zeros(len(rays), F32), np.where(hit, t, F32(np.inf)).astype(F32),
                          expect_hits=False)
    assert (idx3 < 0).all() and not occ3.any()
    check(tris, rays, 2.2, 3.5)  # a scalar window that cuts the sphere
    check(tris, rays, -5.0, 2.5)


def test_input_outside_the_domain_raises():
    from learn_nerf.raycast import TriangleMesh

    dev = torch.device("cuda")
    tris = torch.from_numpy(R.cube(0.5)).to(dev)
    rays = torch.from_numpy(ray_set(R.cube(0.5))[:8]).to(dev)
    mesh = TriangleMesh(tris)
    for bad, where in ((math.nan, (0, 0, 1)), (math.inf, (3, 1, 0)), (2.0 ** 21, (2, 0, 2))):
        broken = rays.clone()
        broken[where] = bad
        with pytest.raises(ValueError):
            mesh.closest(broken)
        with pytest.raises(ValueError):
            mesh.occluded(broken)
    scaled = rays.clone()
    scaled[:, 1] *= 1.01
    with pytest.raises(ValueError, match="unit"):
        mesh.closest(scaled)
    with pytest.raises(ValueError, match="NaN"):
        mesh.closest(rays, 0.0, math.nan)
    with pytest.raises(ValueError):
        mesh.closest(rays[:, 0])
    with pytest.raises(RuntimeError, match="GPU"):
        mesh.closest(rays.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        TriangleMesh(tris.cpu())
    for bad in (math.nan, math.inf, 2.0 ** 21):
        broken = tris.clone()
        broken[5, 1, 2] = bad
        with pytest.raises(ValueError):
            TriangleMesh(broken)
    with pytest.raises(ValueError, match="extent"):
        TriangleMesh(torch.ones((4, 3, 3), device=dev))
    with pytest.raises(ValueError, match="extent"):
        TriangleMesh(tris * 2.0 ** -24)
    with pytest.raises(ValueError):
        TriangleMesh(tris[:0])
    with pytest.raises(ValueError, match="leaf_size"):
        TriangleMesh(tris, leaf_size=65)
    t, idx = mesh.closest(rays[:0])
    assert t.shape == (0,) and idx.shape == (0,)


LIGHTS = np.array([[0.0, 0.0, 1000.0, 0.5], [600.0, 0.0, 800.0, 0.5], [-700.0, 600.0, 400.0, 0.4]])
COLOR = (0.8, 0.8, 0.0)


def _render_both(tris, direction, fov=math.radians(60.0), size=48):
    from learn_nerf.raycast import TriangleMesh, camera_at, fit_distance

    lo, hi = tris.min(axis=(0, 1)), tris.max(axis=(0, 1))
    view = camera_at(lo, hi, direction, fit_distance(lo, hi, direction, fov), fov)
    mesh = TriangleMesh(torch.from_numpy(tris).cuda())
    got = mesh.render(view, size, size, LIGHTS, COLOR).cpu().numpy()
    rays = view.bare_rays(size, size, device="cuda").cpu().numpy()
    t, idx, _ = R.brute_force(tris, rays)
    want = R.shade(tris, rays, t, idx, LIGHTS, COLOR).reshape(size, size, 4)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8]
    return got, (tris, rays, t, idx)


def test_render_of_cube_and_icosphere_equals_the_numpy_shading():
    from learn_nerf.raycast import normalize

    for tris in (normalize(R.cube(0.5)), R.icosphere(3)):
        got, _ = _render_both(tris, np.array([0.5, -0.7, 0.6]))
        hit = got[..., 3] == 255
        assert 400 < hit.sum() < 2304 and (got[~hit] == 0).all()
        assert len(np.unique(got[hit][:, 0])) >= 2 and (got[hit][:, 2] == 0).all()  # shaded, and blue stays 0


def test_render_casts_shadows_on_a_two_object_scene():
    plate = R.cube(0.5) * F32([2.0, 2.0, 0.1]) - F32([0.0, 0.0, 0.6])
    block = R.cube(0.2) + F32([0.1, -0.1, 0.1])
    tris = np.concatenate([plate, block]).astype(F32)
    got, (tris, rays, t, idx) = _render_both(tris, np.array([0.3, -0.6, 0.75]))
    shadow = R.shadowed(tris, rays, t, idx, LIGHTS[:1])  # the light straight above
    on_plate_top = (idx >= 0) & (idx < 12) & shadow
    assert on_plate_top.sum() >= 10, "no pixel of the plate lies in the block's shadow"

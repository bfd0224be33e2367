"""
The texture kernels on the GPU against the NumPy restatement (tests/texture_reference.py), bit for bit: lnrf_tex_texels,
lnrf_tex_uv, lnrf_tex_sample, lnrf_tex_resolve, lnrf_tex_fill on small atlases, and lnrf_tex_bake_views on the scenes of
tests/texture_cases.py (occlusion, culling, image borders, alpha, no views, split launches, the accuracy fixture).
"""
import math

import numpy as np
import pytest
import torch

import texture_cases as C
import texture_reference as T

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def some_tris(faces, seed):
    """Random triangles, one of them (when there are several) collapsed to a segment: zero area."""
    rng = np.random.RandomState(seed)
    tris = rng.uniform(-2, 2, size=(faces, 3, 3)).astype(F32)
    if faces > 1:
        tris[faces // 2, 2] = tris[faces // 2, 1]
    return tris


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# (faces, texture_size) -> cells of 6, 7 and 13 texels; 169 = 13^2 and 196 = 14^2 texels are no multiples of 64
SHAPES = [(1, 6), (1, 7), (2, 6), (2, 7), (3, 12), (3, 14), (7, 12), (7, 14), (7, 26), (2, 13)]


@pytest.mark.parametrize("faces, size", SHAPES)
def test_texels_and_uv_equal_the_reference(faces, size):
    from learn_nerf.texture import TextureAtlas

    tris = some_tris(faces, faces + size)
    atlas = TextureAtlas(dev(tris), size)
    k, c, s = T.layout(faces, size)
    assert (atlas.K, atlas.c, atlas.S) == (k, c, s)
    face, position, normal, bary = (t.cpu().numpy() for t in atlas.texels())
    want = T.texel_geometry(tris, k, c)
    assert np.array_equal(face, want[0])
    for name, got, ref in zip(("position", "normal", "bary"), (position, normal, bary), want[1:]):
        assert np.array_equal(bits(got), bits(ref)), name
    if faces > 1:
        assert (normal[face == faces // 2] == 0).all()  # the zero-area face is flagged
    points, ids = C.surface_samples(tris, 333, seed=faces)
    rng = np.random.RandomState(size)
    points = (points + rng.normal(scale=0.05, size=points.shape)).astype(F32)  # off the faces: projection and clamp
    ids[:faces] = np.arange(faces)
    uv = atlas.uv(dev(points), dev(ids.astype(np.int32))).cpu().numpy()
    assert np.array_equal(bits(uv), bits(T.point_uv(tris, k, c, points, ids)))
    assert atlas.uv(dev(points[:0]), dev(ids[:0].astype(np.int32))).shape == (0, 2)
    with pytest.raises(ValueError, match="face indices"):
        atlas.uv(dev(points[:2]), dev(np.asarray([0, faces], np.int32)))


@pytest.mark.parametrize("height, width", [(6, 6), (13, 13), (7, 12)])
@pytest.mark.parametrize("dtype", [np.uint8, F32])
def test_sample_equals_the_reference(height, width, dtype):
    from learn_nerf.texture import sample

    rng = np.random.RandomState(height * width)
    texture = rng.randint(0, 256, size=(height, width, 3)).astype(dtype)
    if dtype is F32:
        texture = (texture * F32(0.37) - F32(11)).astype(F32)
    uv = rng.uniform(-1.5, max(height, width) + 1.5, size=(1000, 2)).astype(F32)
    centres = np.stack(np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5), axis=-1).reshape(-1, 2)
    corners = np.stack(np.meshgrid(np.arange(width + 1), np.arange(height + 1)), axis=-1).reshape(-1, 2)
    uv = np.concatenate([uv, centres, corners]).astype(F32)  # 1000 + ... samples: no multiple of the block either
    got = sample(dev(texture), dev(uv)).cpu().numpy()
    assert np.array_equal(bits(got), bits(T.sample(texture, uv)))
    at_centres = got[1000:1000 + len(centres)].reshape(height, width, 3)
    assert np.array_equal(at_centres, texture.astype(F32))  # a texel centre returns the texel exactly
    flat = np.full((height, width, 3), 77, dtype=dtype)
    assert (sample(dev(flat), dev(uv)).cpu().numpy() == 77).all()  # equal texels return that value exactly


@pytest.mark.parametrize("faces, size", [(1, 6), (3, 14), (7, 12), (7, 26)])
def test_resolve_and_fill_equal_the_reference(faces, size):
    import ctypes

    from learn_nerf import _lib as L
    from learn_nerf.texture import TextureAtlas, fill

    atlas = TextureAtlas(dev(some_tris(faces, 1)), size)
    s = atlas.S
    rng = np.random.RandomState(faces * size)
    state = np.zeros((s, s, 4), dtype=F32)
    weight = rng.uniform(0.01, 3.0, size=(s, s)).astype(F32)
    weight[rng.uniform(size=(s, s)) < 0.6] = 0  # most texels unseen
    state[:, :, 3] = weight
    state[:, :, :3] = rng.uniform(-20, 300, size=(s, s, 3)).astype(F32) * weight[:, :, None]
    state[0, 0] = (F32(2 * 10.5), F32(2 * 254.5), F32(2 * 255.5), F32(2))  # halves: round up, clamp
    rgb = torch.empty((s, s, 3), dtype=torch.uint8, device=DEV)
    seen = torch.empty((s, s), dtype=torch.uint8, device=DEV)
    L.check(L.lib().lnrf_tex_resolve(ctypes.byref(atlas.desc), L.ptr(dev(state)), 9, 8, 7, L.ptr(rgb, torch.uint8),
                                     L.ptr(seen, torch.uint8), L.stream()))
    want_rgb, want_seen = T.resolve(state, (9, 8, 7))
    assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(seen.cpu().numpy(), want_seen)
    face = T.texel_faces(faces, atlas.K, atlas.c)[0]
    for passes in (0, 1, 2, 5):
        got_rgb, got_seen, filled = fill(atlas, rgb, seen, passes)
        ref_rgb, ref_seen, ref_filled = T.fill(face, want_rgb, want_seen, passes)
        assert np.array_equal(got_rgb.cpu().numpy(), ref_rgb) and np.array_equal(got_seen.cpu().numpy(), ref_seen)
        assert filled == ref_filled == int((ref_seen == 2).sum())
        assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(seen.cpu().numpy(), want_seen)  # inputs kept
    assert ref_filled > 0 and (ref_seen[face < 0] != 2).all()  # texels without a face are never filled
    # a patch whose texels are all unseen takes nothing from its neighbours
    lonely = want_seen.copy()
    lonely[face == 0] = 0
    out_rgb, out_seen, _ = fill(atlas, dev(want_rgb), dev(lonely), 6)
    assert (out_seen.cpu().numpy()[face == 0] == 0).all()
    assert np.array_equal(out_rgb.cpu().numpy()[face == 0], want_rgb[face == 0])


def gpu_bake(case, splits=None, fill_passes=8, tris=None, views=slice(None)):
    """(texture, seen, state, info) of learn_nerf.texture on the case; splits: view counts per launch."""
    from learn_nerf.raycast import TriangleMesh
    from learn_nerf.texture import TextureAtlas, TextureBake

    tris_dev = dev(case.tris if tris is None else tris)
    atlas, mesh = TextureAtlas(tris_dev, case.texture_size), TriangleMesh(tris_dev)
    bake = TextureBake(atlas, mesh, max_angle=math.radians(C.MAX_ANGLE), power=C.POWER)
    assert bake.offset == float(case.offset) and bake.cos_max == float(T.cos_of(C.MAX_ANGLE))
    cameras, images = case.cameras[views], case.images[views]
    start = 0
    for count in (splits or [len(cameras)]):
        bake.add(cameras[start:start + count], images[start:start + count])
        start += count
    assert start == len(cameras)
    state = bake.state.cpu().numpy().reshape(atlas.S, atlas.S, 4)
    texture, seen, info = bake.finish(fill_passes)
    return texture.cpu().numpy(), seen.cpu().numpy(), state, info


def assert_bake_equals_reference(case, got):
    texture, seen, state, info = got
    ref_texture, ref_seen, ref_state, ref_info = case.baked()
    assert np.array_equal(bits(state), bits(ref_state))
    assert np.array_equal(texture, ref_texture) and np.array_equal(seen, ref_seen)
    for key in ("texels_used", "seen", "filled", "unseen"):
        assert info[key] == ref_info[key], key


def test_bake_cube_sees_every_texel():
    """Every face of the cube fronts one axis camera and lies inside its frustum: with opaque images every used texel
    is seen by exactly that camera, so nothing occludes itself at the default offset."""
    case = C.cube_case()
    got = gpu_bake(case)
    assert_bake_equals_reference(case, got)
    info = got[3]
    assert info["seen"] == info["texels_used"] == 2646 and info["filled"] == info["unseen"] == 0
    assert info["degenerate_faces"] == 0 and info["views"] == 6
    assert case.baked()[3]["traversals"] == 2646  # one shadow ray per texel: the other five views are culled before


def test_bake_occlusion_between_parallel_squares():
    case = C.quads_case()
    face = T.texel_faces(4, case.k, case.c)[0]
    rear = (face == 2) | (face == 3)
    first = gpu_bake(case, views=slice(0, 1))[2]
    assert (first[rear, 3] == 0).all() and (first[~rear & (face >= 0), 3] > 0).sum() > 300
    # it is the front square that hides it: without it the same camera sees the rear one
    alone = T.bake(case.tris[2:], 1, case.c, case.views[:1], case.images[:1], T.cos_of(C.MAX_ANGLE), C.POWER, case.offset)
    assert (alone[:, :, 3] > 0).sum() > 300
    assert np.array_equal(bits(first), bits(T.bake(case.tris, case.k, case.c, case.views[:1], case.images[:1],
                                                   T.cos_of(C.MAX_ANGLE), C.POWER, case.offset)))
    got = gpu_bake(case)
    assert_bake_equals_reference(case, got)
    assert (got[2][rear, 3] > 0).sum() > 200  # the second camera colours the rear square


def test_bake_culls_by_side_angle_and_image_border():
    case = C.culling_case()
    face, position, _, _ = T.texel_geometry(case.tris, case.k, case.c)
    used = face >= 0
    for v, expect_any in enumerate([False, False, True, True]):  # behind, grazing, border, ordinary
        state = gpu_bake(case, views=slice(v, v + 1))[2]
        ref = T.bake(case.tris, case.k, case.c, case.views[v:v + 1], case.images[v:v + 1], T.cos_of(C.MAX_ANGLE),
                     C.POWER, case.offset)
        assert np.array_equal(bits(state), bits(ref))
        assert (state[:, :, 3] > 0).any() == expect_any
    # the border view: texels clamped onto the vertex (1, 0, 0) project exactly onto the last column and count;
    # the part of the big triangle beyond it is outside the image
    view = case.views[2]
    xf, yf, front = T.project(view, position.reshape(-1, 3))
    xf, weight = xf.reshape(face.shape), ref_weight(case, 2)
    last = F32(view["width"] - 1)
    assert ((xf == last) & used).sum() >= 2 and (weight[(xf == last) & used] > 0).all()
    assert ((xf > last) & used).sum() > 50 and (weight[(xf > last) & used] == 0).all()
    assert_bake_equals_reference(case, gpu_bake(case))


def ref_weight(case, v):
    return T.bake(case.tris, case.k, case.c, case.views[v:v + 1], case.images[v:v + 1], T.cos_of(C.MAX_ANGLE), C.POWER,
                  case.offset)[:, :, 3]


def test_bake_respects_the_alpha_of_the_footprint():
    case = C.silhouette_case()
    got = gpu_bake(case)
    assert_bake_equals_reference(case, got)
    face, position, _, _ = T.texel_geometry(case.tris, case.k, case.c)
    xf = T.project(case.views[0], position.reshape(-1, 3))[0].reshape(face.shape)
    weight = got[2][:, :, 3]
    assert (weight[xf < 11] == 0).all()  # a footprint that touches column 10 (alpha 127) or less is left out
    assert (weight[(xf >= 11) & (xf <= 22)] > 0).all()  # alpha 128 counts
    for f in (0, 1):  # the silhouette crosses both patches
        assert (weight[face == f] > 0).any() and (weight[face == f] == 0).any()
    info = got[3]
    assert info["filled"] > 0 and info["unseen"] > 0  # eight passes do not reach across the transparent half


def test_bake_without_views():
    from learn_nerf.raycast import TriangleMesh
    from learn_nerf.texture import TextureAtlas, bake_views

    case = C.cube_case()
    tris = dev(case.tris)
    atlas = TextureAtlas(tris, 64)
    texture, info = bake_views(atlas, TriangleMesh(tris), [], [], unseen_color=(1, 2, 3), verbose=False)
    assert texture.shape == (63, 63, 3) and (texture.cpu().numpy() == np.array([1, 2, 3], np.uint8)).all()
    assert info["seen"] == info["filled"] == info["views"] == 0 and info["unseen"] == info["texels_used"] == 2646
    assert not info["seen_mask"].any()


def test_bake_does_not_depend_on_how_views_are_split():
    case = C.sphere_case()
    sub = C.Case(case.tris, case.cameras[:3], case.images[:3], 96)
    whole = gpu_bake(sub, [3])
    assert (whole[2][:, :, 3] > 0).sum() > 1000
    for splits in ([1, 2], [1, 1, 1]):
        other = gpu_bake(sub, splits)
        assert np.array_equal(bits(whole[2]), bits(other[2])) and np.array_equal(whole[0], other[0])
    # and a chunk size of one byte uploads view by view
    from learn_nerf.raycast import TriangleMesh
    from learn_nerf.texture import TextureAtlas, bake_views

    tris = dev(sub.tris)
    texture, info = bake_views(TextureAtlas(tris, 96), TriangleMesh(tris), sub.cameras, sub.images, chunk_bytes=1,
                               verbose=False)
    assert np.array_equal(texture.cpu().numpy(), whole[0]) and info["views"] == 3


def test_bake_of_the_accuracy_fixture_equals_the_reference():
    """The texture equals the reference's, so its accuracy is the one tests/test_texture_cpu.py measures."""
    case = C.sphere_case()
    assert_bake_equals_reference(case, gpu_bake(case))


def test_no_bleed_on_the_device():
    """uv() then sample() of 4,096 surface samples on a texture coloured by face id return each sample's own face."""
    from learn_nerf.raycast import TriangleMesh
    from learn_nerf.texture import TextureAtlas

    rng = np.random.RandomState(11)
    tris = dev(rng.uniform(-1, 1, size=(7, 3, 3)).astype(F32))
    atlas = TextureAtlas(tris, 12)
    assert atlas.c == 6
    face = atlas.texels()[0]
    texture = (face + 1).to(torch.float32)[:, :, None].repeat(1, 1, 3).contiguous()
    points, ids = TriangleMesh(tris).sample_surface(4096, seed=3)
    assert len(torch.unique(ids)) == 7
    got = atlas.sample(texture, atlas.uv(points, ids))
    assert torch.equal(got, (ids + 1).to(torch.float32)[:, None].repeat(1, 3))
    as_bytes = (face + 1).to(torch.uint8)[:, :, None].repeat(1, 1, 3).contiguous()
    assert torch.equal(atlas.sample(as_bytes, atlas.uv(points, ids)), got)


def test_reprojection_psnr_prefers_the_baked_texture():
    from learn_nerf.raycast import TriangleMesh
    from learn_nerf.texture import TextureAtlas, bake_views, reprojection_psnr

    case = C.cube_case()
    tris = dev(case.tris)
    atlas, mesh = TextureAtlas(tris, 64), TriangleMesh(tris)
    texture, info = bake_views(atlas, mesh, case.cameras, case.images, verbose=False)
    per_view, mean = reprojection_psnr(atlas, mesh, texture, case.cameras, case.images)
    assert len(per_view) == 6 and all(math.isfinite(p) for p in per_view) and math.isfinite(mean)
    used = atlas.texels()[0] >= 0
    flat = torch.empty_like(texture)
    flat[:] = texture[used].float().mean(dim=0).round().to(torch.uint8)
    _, flat_mean = reprojection_psnr(atlas, mesh, flat, case.cameras, case.images)
    print(f"reprojection PSNR: baked {mean:.2f} dB, mean colour {flat_mean:.2f} dB")
    assert math.isfinite(flat_mean) and mean > flat_mean


def test_domain_checks_raise_before_any_launch():
    from learn_nerf.raycast import TriangleMesh
    from learn_nerf.texture import TextureAtlas, TextureBake, bake_views

    case = C.cube_case()
    tris = dev(case.tris)
    atlas, mesh = TextureAtlas(tris, 64), TriangleMesh(tris)
    with pytest.raises(ValueError, match="same triangles"):
        TextureBake(atlas, TriangleMesh(tris[:6].contiguous()))
    with pytest.raises(ValueError, match="power"):
        TextureBake(atlas, mesh, power=1.5)
    with pytest.raises(ValueError, match="max_angle"):
        TextureBake(atlas, mesh, max_angle=2.0)
    with pytest.raises(ValueError, match="offset"):
        TextureBake(atlas, mesh, offset=-1.0)
    with pytest.raises(ValueError, match="cameras and"):
        bake_views(atlas, mesh, case.cameras, case.images[:2], verbose=False)
    with pytest.raises(ValueError, match="uint8"):
        bake_views(atlas, mesh, case.cameras[:1], [case.images[0].astype(np.float32)], verbose=False)
    with pytest.raises(ValueError, match="unseen_color"):
        bake_views(atlas, mesh, [], [], unseen_color=(0, 0, 300), verbose=False)
    with pytest.raises(ValueError, match="non-finite"):
        atlas.uv(torch.full((1, 3), float("nan"), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))

"""
Texture baking without a GPU: the atlas layout and its no-bleed property on the NumPy restatement
(tests/texture_reference.py), the host side of learn_nerf/texture.py against it, csrc/tex_geom.h compiled for the host
against it bit for bit, the projection against CameraView.bare_rays, the written files, and the accuracy of the
reference bake on an analytic colour field.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raycast_reference as RC
import texture_cases as C
import texture_reference as T
import tsdf_reference as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "learn-nerf_amd", "csrc")
F32 = np.float32


def lattice_uvs(c, half, shift=0, steps=64):
    """Every point A + (a/steps)(B - A) + (b/steps)(C - A), a + b <= steps, of a patch: vertices, edges and interior.
    The legs are integers and steps a power of two, so every coordinate is exact in float32."""
    (ax, ay), (bx, by), (cx, cy) = T.patch_corners(c, half, shift)
    a, b = np.meshgrid(np.arange(steps + 1), np.arange(steps + 1), indexing="ij")
    keep = a + b <= steps
    a, b = a[keep].astype(np.float64) / steps, b[keep].astype(np.float64) / steps
    uv = np.stack([ax + a * (bx - ax) + b * (cx - ax), ay + a * (by - ay) + b * (cy - ay)], axis=1)
    assert np.array_equal(uv.astype(F32).astype(np.float64), uv)
    return uv.astype(F32)


def bleeding_samples(c, shift=0):
    """The number of lattice samples, over all 8 faces of a 2 x 2 atlas of cell c, that do not return their own face's
    colour exactly from a texture coloured by face id."""
    faces, k = 8, 2
    face = T.texel_faces(faces, k, c)[0]
    texture = np.repeat((face + 1).astype(F32)[:, :, None], 3, axis=2)
    bad = 0
    for f in range(faces):
        ox, oy = T.cell_origin(f, k, c)
        uv = lattice_uvs(c, f % 2, shift) + np.array([ox, oy], dtype=F32)
        got = T.sample(texture, uv)
        bad += int((got != F32(f + 1)).any(axis=1).sum())
    return bad


@pytest.mark.parametrize("c", range(T.MIN_CELL, 21))
def test_bilinear_samples_of_a_patch_read_only_its_own_texels(c):
    assert bleeding_samples(c) == 0
    # the constants are tight: a patch moved one texel towards the diagonal bleeds
    assert bleeding_samples(c, shift=1) > 0


@pytest.mark.parametrize("faces", [1, 2, 3, 7, 8, 9])
def test_every_half_cell_maps_to_its_own_face(faces):
    k, c, s = T.layout(faces, 64)
    assert s == k * c and k * k >= (faces + 1) // 2 > (k - 1) * (k - 1)
    face, i, j = T.texel_faces(faces, k, c)
    assert face.shape == (s, s)
    lower, upper = c * (c + 1) // 2, c * (c - 1) // 2
    ids, counts = np.unique(face[face >= 0], return_counts=True)
    assert ids.tolist() == list(range(faces))
    assert counts.tolist() == [lower if f % 2 == 0 else upper for f in range(faces)]
    for f in range(faces):  # one half of one cell each
        ys, xs = np.nonzero(face == f)
        pair = f // 2
        assert (xs // c == pair % k).all() and (ys // c == pair // k).all()
        assert ((i[ys, xs] + j[ys, xs] + 1 <= c) == (f % 2 == 0)).all()
    empty = (face < 0).sum()
    whole_cells = k * k - (faces + 1) // 2
    assert empty == whole_cells * c * c + (upper if faces % 2 else 0)  # an odd F leaves exactly one half-cell empty


def test_layout_of_the_package_and_its_errors():
    from learn_nerf.texture import MAX_CELL, MIN_CELL, TextureAtlas, atlas_layout

    assert (MIN_CELL, MAX_CELL) == (T.MIN_CELL, T.MAX_CELL)
    for faces in (1, 2, 3, 7, 8, 9, 80, 50_000, 1_000_001):
        for size in (64, 100, 2048, 4096):
            try:
                want = T.layout(faces, size)
            except ValueError:
                with pytest.raises(ValueError, match="too small"):
                    atlas_layout(faces, size)
                continue
            k, c, s = atlas_layout(faces, size)
            assert (k, c, s) == want and s == k * c and s <= size and T.MIN_CELL <= c <= T.MAX_CELL
    assert atlas_layout(2, 2048) == (1, 256, 256)  # the cell is capped
    # 50,000 faces are 25,000 pairs: 159 x 159 cells of at least 6 texels, 954
    with pytest.raises(ValueError) as err:
        atlas_layout(50_000, 512)
    assert "954 x 954" in str(err.value) and "--target_faces" in str(err.value) and "simplify_mesh.py" in str(err.value)
    assert atlas_layout(50_000, 954) == (159, 6, 954)
    tris = RC.cube(0.5)
    atlas = TextureAtlas(tris, 64)
    assert (atlas.F, atlas.K, atlas.c, atlas.S) == (12, 3, 21, 63)
    assert atlas.texels_used == int((T.texel_faces(12, 3, 21)[0] >= 0).sum())
    odd = TextureAtlas(tris[:7], 64)
    assert odd.texels_used == int((T.texel_faces(7, odd.K, odd.c)[0] >= 0).sum())
    with pytest.raises(ValueError, match=r"\[F, 3, 3\]"):
        TextureAtlas(np.zeros((4, 3)), 64)
    with pytest.raises(ValueError, match="non-finite"):
        TextureAtlas(np.full((1, 3, 3), np.nan), 64)


def test_gpu_methods_refuse_the_cpu():
    from learn_nerf.texture import TextureAtlas, fill, sample

    atlas = TextureAtlas(RC.cube(0.5), 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        atlas.texels()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        atlas.uv(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sample(torch.zeros(4, 4, 3), torch.zeros(2, 2))
    with pytest.raises(ValueError, match="uint8 or float32"):
        sample(torch.zeros(4, 4, 3, dtype=torch.float64), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fill(atlas, torch.zeros(63, 63, 3, dtype=torch.uint8), torch.zeros(63, 63, dtype=torch.uint8), 1)


def test_atlas_errors_are_err_shape_without_a_gpu():
    """The atlas is checked before any pointer is looked at, so the entry points can be asked on the host."""
    import ctypes

    from learn_nerf import _lib as L

    lib = L.lib()
    bvh = L.RtBvh((ctypes.c_float * 3)(0, 0, 0), 3.0, (ctypes.c_float * 3)(1, 1, 1), 12, 4, 0)
    for desc in ((0, 1, 6, 6), (2, 1, 5, 5), (2, 1, 257, 257), (2, 2, 6, 12), (9, 2, 6, 12), (2, 1, 6, 7)):
        atlas = ctypes.byref(L.TexAtlas(*desc))
        assert lib.lnrf_tex_texels(atlas, None, None, None, None, None, None) == -2, desc
        assert lib.lnrf_tex_uv(atlas, None, None, None, 1, None, None) == -2, desc
        assert lib.lnrf_tex_resolve(atlas, None, 0, 0, 0, None, None, None) == -2, desc
        assert lib.lnrf_tex_fill(atlas, None, None, None, None, None, None) == -2, desc
        assert lib.lnrf_tex_bake_views(ctypes.byref(bvh), None, None, atlas, None, None, 1, None, 0.1, 2, 0.0, None,
                                       None) == -2, desc
    good = ctypes.byref(L.TexAtlas(7, 2, 6, 12))
    assert lib.lnrf_tex_texels(good, None, None, None, None, None, None) == -1  # LNRF_ERR_ARG: null pointers
    assert lib.lnrf_tex_bake_views(ctypes.byref(bvh), None, None, good, None, None, 1, None, 0.1, 65, 0.0, None,
                                   None) == -1
    assert lib.lnrf_tex_sample(None, 0, 0, 4, None, 1, None, None) == -2
    assert lib.lnrf_tex_sample(None, 0, 4, 4, None, 0, None, None) == 0  # nothing to do


TIES = [  # (triangle, corner that goes to the right angle)
    ([(0, 0, 0), (1, 0, 0), (0, 1, 0)], 0),      # l = (2, 1, 1)
    ([(1, 0, 0), (0, 1, 0), (0, 0, 0)], 2),      # the same triangle, rotated
    ([(-1, 0, 0), (1, 0, 0), (0, 5, 0)], 0),     # l = (26, 26, 4): the first of the two longest
    ([(0, 5, 0), (-1, 0, 0), (1, 0, 0)], 1),     # l = (4, 26, 26)
    ([(-1, 0, 0), (0, 5, 0), (1, 0, 0)], 0),     # l = (26, 4, 26)
    ([(1, 0, 0), (0, 1, 0), (0, 0, 1)], 0),      # equilateral: all 2
    ([(0, 0, 0), (0, 0, 0), (0, 0, 0)], 0),      # a point
]


def test_the_longest_edge_lands_on_the_hypotenuse():
    from learn_nerf.texture import TextureAtlas, degenerate_faces, right_angles

    tris = np.asarray([t for t, _ in TIES], dtype=F32)
    want = [r for _, r in TIES]
    assert T.right_angles(tris).tolist() == want and right_angles(tris).tolist() == want
    assert degenerate_faces(tris).tolist() == [False] * 6 + [True]
    rng = np.random.RandomState(0)
    soup = rng.uniform(-1, 1, size=(500, 3, 3)).astype(F32)
    r = T.right_angles(soup)
    assert np.array_equal(r, right_angles(soup))
    d = soup.astype(np.float64)
    lengths = np.stack([np.linalg.norm(d[:, (k + 1) % 3] - d[:, (k + 2) % 3], axis=1) for k in range(3)], axis=1)
    assert np.array_equal(r, lengths.argmax(axis=1))  # no near-ties in this soup
    # in the atlas: the vertex at the right angle has the patch's corner A, the other two the hypotenuse
    both = np.concatenate([tris, soup])
    atlas = TextureAtlas(both, 2048)
    uvs = atlas.vertex_uvs().reshape(-1, 3, 2)
    assert np.array_equal(uvs, T.vertex_uvs(both, atlas.K, atlas.c).reshape(-1, 3, 2))
    rr = T.right_angles(both)
    for f in range(len(both)):
        ox, oy = T.cell_origin(f, atlas.K, atlas.c)
        corners = [(ox + x, oy + y) for x, y in T.patch_corners(atlas.c, f % 2)]
        assert [tuple(uvs[f, (rr[f] + slot) % 3]) for slot in range(3)] == corners


def test_texels_of_the_reference_lie_on_their_faces():
    """The texel geometry in float64 terms: barycentrics sum to 1 and are inside, the position is their combination, a
    patch's interior texels reproduce the affine map of the UV triangle, and the gutter is clamped onto the edges."""
    rng = np.random.RandomState(1)
    tris = rng.uniform(-1, 1, size=(7, 3, 3)).astype(F32)
    tris[4] = tris[4, 0]  # a point: degenerate
    k, c, s = T.layout(7, 22)
    assert c == 11
    face, position, normal, bary = T.texel_geometry(tris, k, c)
    used = face >= 0
    assert (bary[used] >= -1e-6).all() and np.abs(bary[used].sum(axis=1) - 1).max() < 1e-6
    want = np.einsum("nk,nkd->nd", bary[used].astype(np.float64), tris[face[used]].astype(np.float64))
    assert np.abs(position[used] - want).max() < 1e-6
    assert (normal[face == 4] == 0).all() and (position[face == 4] == tris[4, 0]).all()
    lengths = np.linalg.norm(normal[used & (face != 4)], axis=1)
    assert np.abs(lengths - 1).max() < 1e-6
    assert (position[~used] == 0).all() and (normal[~used] == 0).all() and (bary[~used] == 0).all()
    # the uv of a texel's own point is its centre, for the texels whose centre lies inside the UV triangle
    inside = used & (bary.min(axis=2) > 1e-3) & (face != 4)
    assert inside.sum() > 100
    ys, xs = np.nonzero(inside)
    uv = T.point_uv(tris, k, c, position[ys, xs], face[ys, xs])
    assert np.abs(uv - np.stack([xs + 0.5, ys + 0.5], axis=1)).max() < 1e-3
    # a degenerate face's points all go to corner A
    uv = T.point_uv(tris, k, c, tris[4, :1], [4])
    assert uv.tolist() == [[c * 0 + 1.0, c * 1 + 1.0]]


def host_program(tmp_path):
    exe = str(tmp_path / "tex_geom_host")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
           os.path.join(ROOT, "tests", "tex_geom_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("faces, size", [(7, 14), (2, 6), (9, 63)])
def test_tex_geom_h_on_the_host_agrees_bit_for_bit(tmp_path, faces, size):
    """csrc/tex_geom.h, compiled for the host without contraction, gives the bits of the NumPy restatement."""
    rng = np.random.RandomState(faces)
    tris = rng.uniform(-2, 2, size=(faces, 3, 3)).astype(F32)
    tris[faces // 2, 2] = tris[faces // 2, 1]  # zero area
    k, c, s = T.layout(faces, size)
    points, ids = C.surface_samples(tris, 300, seed=3)
    points = (points + rng.normal(scale=0.05, size=points.shape)).astype(F32)  # off the faces: projection and clamp
    ids[:faces] = np.arange(faces)  # the degenerate face too
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as handle:
        handle.write(np.asarray([faces, k, c, len(ids)], np.int32).tobytes() + tris.tobytes() + points.tobytes() +
                     ids.astype(np.int32).tobytes())
    subprocess.run([host_program(tmp_path), src, dst], check=True)
    raw = np.fromfile(dst, dtype=np.uint8)
    n = s * s
    assert len(raw) == 4 * (n + 9 * n + 2 * len(ids))
    face = raw[:4 * n].view(np.int32).reshape(s, s)
    position, normal, bary = (raw[4 * n * (1 + 3 * a):4 * n * (4 + 3 * a)].view(F32).reshape(s, s, 3) for a in range(3))
    uv = raw[40 * n:].view(F32).reshape(-1, 2)
    want = T.texel_geometry(tris, k, c)
    assert np.array_equal(face, want[0])
    for name, got, ref in zip(("position", "normal", "bary"), (position, normal, bary), want[1:]):
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name
    assert np.array_equal(uv.view(np.uint32), T.point_uv(tris, k, c, points, ids).view(np.uint32))


def _projection_cases():
    yield TS.look_at_camera((0.3, -0.5, 0.8)), 64, 64
    yield TS.look_at_camera((1.0, 0.2, -0.1), x_fov=0.7, y_fov=0.45), 40, 25
    yield TS.look_at_camera((-0.4, 0.9, 0.3), x_fov=0.5, y_fov=0.8, skew=0.15), 31, 47  # not orthonormal


@pytest.mark.parametrize("case", range(3))
def test_a_pixel_centres_ray_projects_back_onto_that_centre(case):
    from learn_nerf.texture import VIEW_DTYPE, pack_views

    cam, width, height = list(_projection_cases())[case]
    views = pack_views([cam, cam], [(width, height), (width, height)])
    assert views.dtype == VIEW_DTYPE and views["pixel_offset"].tolist() == [0, width * height]
    rays = cam.bare_rays(width, height).numpy()
    rng = np.random.RandomState(case)
    depth = rng.uniform(2.0, 6.0, size=len(rays)).astype(F32)
    points = (rays[:, 0] + rays[:, 1] * depth[:, None]).astype(F32)
    xf, yf, front = T.project(views[0], points)
    assert front.all()
    col, row = np.meshgrid(np.arange(width), np.arange(height))
    worst = max(np.abs(xf - col.reshape(-1)).max(), np.abs(yf - row.reshape(-1)).max())
    print(f"largest distance from the pixel centre: {worst:.2e} pixels")
    assert worst < 1e-3
    behind = (rays[:, 0] - rays[:, 1] * depth[:, None]).astype(F32)
    assert not T.project(views[0], behind)[2].any()


def test_resolve_and_fill_of_the_reference():
    state = np.zeros((2, 3, 4), dtype=F32)
    state[0, 0] = (2 * 10.5, 2 * 254.6, 2 * 300.0, 2.0)  # rounds half up, clamps above 255
    state[0, 1] = (-3.0, 0.0, 0.4999, 1.0)  # clamps below 0
    state[1, 2] = (5.0, 5.0, 5.0, 0.0)  # no weight: unseen
    rgb, seen = T.resolve(state, (1, 2, 3))
    assert rgb[0, 0].tolist() == [11, 255, 255] and rgb[0, 1].tolist() == [0, 0, 0]
    assert seen.tolist() == [[1, 1, 0], [0, 0, 0]] and rgb[1, 2].tolist() == [1, 2, 3]
    # filling never crosses a patch, takes the mean of the seen neighbours and grows by one texel per pass
    face = T.texel_faces(2, 1, 6)[0]
    rgb = np.zeros((6, 6, 3), np.uint8)
    seen = np.zeros((6, 6), np.uint8)
    rgb[0, 0], seen[0, 0] = (10, 20, 30), 1
    rgb[0, 2], seen[0, 2] = (13, 20, 31), 1
    rgb[5, 5], seen[5, 5] = (200, 200, 200), 1
    out, mark, n = T.fill_pass(face, rgb, seen)
    assert out[0, 1].tolist() == [12, 20, 31] and mark[0, 1] == 2  # (10 + 13) / 2 = 11.5 -> 12, 30.5 -> 31
    assert n == int((mark == 2).sum()) == 6  # (1,0), (0,1), (1,2), (0,3) in the lower half, (4,5), (5,4) in the upper
    out8, mark8, n8 = T.fill(face, rgb, seen, 12)
    assert (mark8 != 0).all() and n8 == 33
    assert (out8[face == 1] == 200).all() and (out8[face == 0] < 200).all()


def test_written_files(tmp_path):
    from PIL import Image

    from learn_nerf.mesh_metrics import read_mesh
    from learn_nerf.texture import TextureAtlas, weld, write_textured_obj

    tris = RC.cube(0.5)
    tris[0, 0, 0] = F32(-0.1234567)  # a coordinate that needs all its digits
    atlas = TextureAtlas(tris, 64)
    rng = np.random.RandomState(2)
    texture = rng.randint(0, 256, size=(atlas.S, atlas.S, 3), dtype=np.uint8)
    path = str(tmp_path / "baked.obj")
    mtl, png = write_textured_obj(path, tris, atlas, texture)
    assert (mtl, png) == (str(tmp_path / "baked.mtl"), str(tmp_path / "baked.png"))
    lines = open(path).read().splitlines()
    assert lines[0] == "mtllib baked.mtl"
    verts, faces = weld(tris)
    assert len(verts) == 9 and np.array_equal(verts[faces], tris)  # 8 corners and the moved one
    assert sum(line.startswith("v ") for line in lines) == 9
    vts = np.asarray([[float(x) for x in line.split()[1:]] for line in lines if line.startswith("vt ")])
    assert vts.shape == (3 * len(tris), 2) and (vts >= 0).all() and (vts <= 1).all()
    back = np.stack([vts[:, 0] * atlas.S, (1 - vts[:, 1]) * atlas.S], axis=1)
    assert np.abs(back - atlas.vertex_uvs()).max() < 1e-9
    face_lines = [line for line in lines if line.startswith("f ")]
    assert len(face_lines) == len(tris) and face_lines[0].count("/") == 3 and "//" not in face_lines[0]
    assert [int(e.split("/")[1]) for line in face_lines for e in line.split()[1:]] == list(range(1, 3 * len(tris) + 1))
    assert "map_Kd baked.png" in open(mtl).read().splitlines()
    with Image.open(png) as image:
        assert image.size == (atlas.S, atlas.S) and image.mode == "RGB"
        assert np.array_equal(np.asarray(image), texture)
    assert np.array_equal(read_mesh(path), tris)
    with pytest.raises(ValueError, match=".obj"):
        write_textured_obj(str(tmp_path / "baked.ply"), tris, atlas, texture)
    with pytest.raises(ValueError, match="texture"):
        write_textured_obj(path, tris, atlas, texture[:-1])


def test_read_views_keeps_the_alpha(tmp_path):
    from learn_nerf.texture import read_views

    case = C.quads_case()
    data = str(tmp_path / "data")
    C.write_dataset(data, case.cameras, case.images)
    cameras, images, paths = read_views(data)
    assert [os.path.basename(p) for p in paths] == ["00000.png", "00001.png"]
    for got, want, cam, ref in zip(images, case.images, cameras, case.cameras):
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert cam.camera_origin == ref.camera_origin and cam.x_axis == ref.x_axis
    assert len(read_views(data, max_views=1)[0]) == 1


def _cli(argv):
    scripts = os.path.join(ROOT, "learn-nerf_amd", "learn_nerf", "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import texture_mesh

    return texture_mesh.main(argv)


def test_cli_argument_errors_exit_with_their_messages(tmp_path):
    from learn_nerf.mesh import write_stl

    case = C.quads_case()
    data = str(tmp_path / "data")
    C.write_dataset(data, case.cameras, case.images)
    mesh = str(tmp_path / "mesh.stl")
    verts = case.tris.reshape(-1, 3)
    write_stl(mesh, verts, np.arange(len(verts)).reshape(-1, 3))
    out = str(tmp_path / "out.obj")
    cases = [
        ([mesh, data, str(tmp_path / "out.ply")], ".obj"),
        (["--texture_size", "0", mesh, data, out], "--texture_size must be positive"),
        (["--max_angle", "95", mesh, data, out], "--max_angle"),
        (["--angle_power", "-1", mesh, data, out], "--angle_power"),
        (["--offset", "-1", mesh, data, out], "--offset"),
        (["--fill_passes", "-1", mesh, data, out], "--fill_passes"),
        (["--unseen_color", "0", "0", "256", mesh, data, out], "--unseen_color"),
        (["--target_faces", "0", mesh, data, out], "--target_faces"),
        (["--max_views", "0", mesh, data, out], "--max_views"),
        ([str(tmp_path / "missing.stl"), data, out], "missing.stl"),
        ([str(tmp_path / "mesh.xyz"), data, out], "unknown mesh format"),
    ]
    for argv, message in cases:
        with pytest.raises(SystemExit) as err:
            _cli(argv)
        assert message in str(err.value.code), (argv, err.value.code)
    assert not os.path.exists(out)


def test_the_reference_bake_reproduces_an_analytic_colour_field():
    """
    The accuracy gate.  The icosphere of 80 faces carries the colour field of tests/texture_cases.py (Lipschitz constant
    0.8 per channel), twelve 64 x 64 views see it on a transparent background, and the reference bakes them at
    texture_size 256.  At 2,000 area-weighted surface points the mean absolute error of the sampled texture against the
    field must be at most a quarter of the error of the best constant colour (the per-channel median), and every texel
    that a sample reads must be seen or filled.  Measured: mean absolute error 0.0009 against 0.2084 for the best
    constant (a ratio of 0.0041), largest error 0.0067; all 51,840 used texels are seen, none needs filling.
    """
    case = C.sphere_case()
    assert (case.k, case.c, case.s) == (7, 36, 252)
    texture, seen, state, info = case.baked()
    points, ids = C.surface_samples(case.tris, 2000, seed=7)
    uv = T.point_uv(case.tris, case.k, case.c, points, ids)
    got = T.sample(texture, uv).astype(np.float64) / 255
    want = C.field(points)
    error = np.abs(got - want)
    constant = np.abs(want - np.median(want, axis=0)).mean()
    print(f"mean |error| {error.mean():.4f}, max {error.max():.4f}; best constant {constant:.4f}; "
          f"ratio {error.mean() / constant:.4f}; texels {info}")
    i0, i1, _ = T.tap_at(uv[:, 0] - F32(0.5), case.s)
    j0, j1, _ = T.tap_at(uv[:, 1] - F32(0.5), case.s)
    for j in (j0, j1):
        for i in (i0, i1):
            assert (seen[j, i] != 0).all()
    assert error.mean() <= constant / 4
    assert info["unseen"] == 0

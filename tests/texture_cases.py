"""
Scenes shared by tests/test_texture_cpu.py and the GPU texture tests: meshes, cameras and images made by first-hit brute
force in NumPy (tests/raycast_reference.py), and the reference bake of each (tests/texture_reference.py), computed once
per process and left unchanged.
"""
import functools
import math

import numpy as np

import raycast_reference as RC
import texture_reference as T
import tsdf_reference as TS

F32 = np.float32
MAX_ANGLE = 80.0
POWER = 2

# the smooth colour field of the fixtures: channel k is 0.5 + 0.4 sin(2 a_k . p + k) with unit a_k, so its gradient is at
# most 0.8 everywhere: Lipschitz constant 0.8 per channel in the Euclidean distance
FIELD_AXES = np.array([[1.0, 0.0, 0.0], [0.0, 0.6, 0.8], [0.6, -0.8, 0.0]])
FIELD_LIPSCHITZ = 0.8


def field(points):
    """float64 [n, 3] in [0.1, 0.9]."""
    p = np.asarray(points, np.float64)
    return 0.5 + 0.4 * np.sin(2.0 * (p @ FIELD_AXES.T) + np.arange(3))


def render(tris, cam, width, height, alpha_background=True, color=field):
    """uint8 [H, W, 4] (or [H, W, 3] on black without alpha_background): the first hit of every pixel's ray of
    CameraView.bare_rays, coloured rint(255 color(hit)); a miss is 0, 0, 0 with alpha 0."""
    rays = cam.bare_rays(width, height).numpy()
    t, idx, _ = RC.brute_force(tris, rays)
    hit = idx >= 0
    out = np.zeros((width * height, 4), dtype=np.uint8)
    points = rays[hit, 0].astype(np.float64) + t[hit, None].astype(np.float64) * rays[hit, 1].astype(np.float64)
    out[hit, :3] = np.rint(255 * color(points)).astype(np.uint8)
    out[hit, 3] = 255
    out = out.reshape(height, width, 4)
    return out if alpha_background else np.ascontiguousarray(out[:, :, :3])


def pack(cameras, images):
    from learn_nerf.texture import pack_views

    return pack_views(cameras, [(im.shape[1], im.shape[0]) for im in images])


def quad(z, half=0.5, flip=False):
    """Two triangles of the square [-half, half]^2 at height z, normal +z (or -z with flip)."""
    a, b, c, d = (-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)
    tris = [(a, b, c), (a, c, d)]
    if flip:
        tris = [(p, r, q) for p, q, r in tris]
    return np.asarray(tris, dtype=F32)


class Case:
    """A mesh, its views and the atlas (K, c, S) that `texture_size` gives."""

    def __init__(self, tris, cameras, images, texture_size, offset=None):
        self.tris = np.ascontiguousarray(tris, dtype=F32)
        self.cameras, self.images = list(cameras), list(images)
        self.texture_size = texture_size
        self.k, self.c, self.s = T.layout(len(self.tris), texture_size)
        self.offset = T.default_offset(self.tris) if offset is None else F32(offset)
        self.views = pack(self.cameras, self.images) if self.cameras else []

    @functools.lru_cache(maxsize=None)
    def baked(self, fill_passes=8):
        """(texture, seen, state, info) of the reference, with the traversal count in info."""
        stats = {}
        state = T.bake(self.tris, self.k, self.c, self.views, self.images, T.cos_of(MAX_ANGLE), POWER, self.offset,
                       stats=stats)
        rgb, seen = T.resolve(state)
        n_seen = int((seen == 1).sum())
        face = T.texel_faces(len(self.tris), self.k, self.c)[0]
        rgb, seen, filled = T.fill(face, rgb, seen, fill_passes)
        used = int((face >= 0).sum())
        info = dict(texels_used=used, seen=n_seen, filled=filled, unseen=used - n_seen - filled,
                    traversals=stats.get("traversals", 0))
        for a in (rgb, seen, state):
            a.setflags(write=False)
        return rgb, seen, state, info


@functools.lru_cache(maxsize=None)
def cube_case():
    """The unit cube under six axis cameras at 32 x 32, opaque images (black background): every face fronts a camera."""
    tris = RC.cube(0.5)
    cameras = [TS.look_at_camera(d) for d in TS.AXES6]
    images = [render(tris, cam, 32, 32, alpha_background=False) for cam in cameras]
    return Case(tris, cameras, images, 64)


@functools.lru_cache(maxsize=None)
def quads_case():
    """Two parallel squares, both facing +z, at z = 1 and z = -1.  Camera 0 looks down on them from +z: the front one
    hides the rear one.  Camera 1 stands beside and above the pair and sees the rear square past the front one."""
    tris = np.concatenate([quad(1.0), quad(-1.0)])
    cameras = [TS.look_at_camera((0, 0, -1), x_fov=0.8, y_fov=0.8),  # at (0, 0, 4)
               TS.look_at_camera((-1, 0, -1), x_fov=0.9, y_fov=0.9, origin=(3.0, 0.0, 2.0))]
    images = [render(tris, cam, 24, 24) for cam in cameras]
    return Case(tris, cameras, images, 40)


@functools.lru_cache(maxsize=None)
def culling_case():
    """One square facing +z and a larger triangle beside it, under: a camera behind the surface; a camera 85 degrees
    off the normal (beyond max_angle); a camera whose image border passes through the vertex (1, 0, 0), so that the
    gutter texels clamped onto that vertex project exactly onto the last pixel column, and beyond which the big triangle
    leaves the image; and an ordinary camera."""
    from learn_nerf.dataset import CameraView

    tris = np.concatenate([quad(0.0), np.asarray([[(0.5, -0.5, 0.0), (1.0, 0.0, 0.0), (0.5, 0.5, 0.0)],
                                                  [(1.0, 0.0, 0.0), (2.0, -1.0, 0.0), (2.0, 1.0, 0.0)]], dtype=F32)])
    grazing = math.radians(85.0)
    border = CameraView(camera_direction=(0.0, 0.0, -1.0), camera_origin=(0.0, 0.0, 4.0), x_axis=(1.0, 0.0, 0.0),
                        y_axis=(0.0, -1.0, 0.0), x_fov=2 * math.atan(0.25), y_fov=2 * math.atan(0.25))
    cameras = [TS.look_at_camera((0, 0, 1)),  # at (0, 0, -4): behind
               TS.look_at_camera((-math.sin(grazing), 0, -math.cos(grazing))),
               border,
               TS.look_at_camera((0.3, -0.2, -1), x_fov=0.9, y_fov=0.9)]
    images = [render(tris, cam, w, h, alpha_background=False) for cam, (w, h) in zip(cameras, [(16, 16), (16, 16),
                                                                                             (17, 13), (20, 16)])]
    return Case(tris, cameras, images, 36)


@functools.lru_cache(maxsize=None)
def silhouette_case():
    """One square whose view is transparent (alpha 0) left of column 10 of 24: the silhouette crosses both patches."""
    tris = quad(0.0)
    cam = TS.look_at_camera((0.1, 0.2, -1), x_fov=0.5, y_fov=0.5)
    image = render(tris, cam, 24, 20, alpha_background=False)
    rng = np.random.RandomState(5)
    rgba = np.concatenate([rng.randint(0, 256, size=image.shape, dtype=np.uint8),
                           np.full(image.shape[:2] + (1,), 255, np.uint8)], axis=2)
    rgba[:, :10, 3] = 0
    rgba[:, 10, 3] = 127  # just below the threshold
    rgba[:, 11, 3] = 128  # just at it
    return Case(tris, [cam], [rgba], 24)


@functools.lru_cache(maxsize=None)
def sphere_case():
    """The accuracy fixture: the icosphere of 80 faces coloured by field(), twelve 64 x 64 views on alpha 0, S <= 256."""
    tris = RC.icosphere(1)
    assert len(tris) == 80
    cameras = [TS.look_at_camera(d) for d in TS.ICOSAHEDRON]
    images = [render(tris, cam, 64, 64) for cam in cameras]
    return Case(tris, cameras, images, 256)


def surface_samples(tris, count, seed):
    """(points float32 [count, 3], face ids int64 [count]): area-weighted uniform samples."""
    t = np.asarray(tris, np.float64)
    areas = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    rng = np.random.RandomState(seed)
    ids = rng.choice(len(t), size=count, p=areas / areas.sum())
    u, v = rng.uniform(size=count), rng.uniform(size=count)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    points = t[ids, 0] + u[:, None] * (t[ids, 1] - t[ids, 0]) + v[:, None] * (t[ids, 2] - t[ids, 0])
    return points.astype(F32), ids.astype(np.int64)


def write_dataset(path, cameras, images, bbox=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))):
    """NNNNN.json / NNNNN.png and metadata.json, as learn_nerf.dataset.load_dataset reads them."""
    import json
    import os

    from PIL import Image

    os.makedirs(path, exist_ok=True)
    for i, (cam, image) in enumerate(zip(cameras, images)):
        with open(os.path.join(path, f"{i:05d}.json"), "w") as handle:
            handle.write(cam.to_json())
        Image.fromarray(image).save(os.path.join(path, f"{i:05d}.png"))
    with open(os.path.join(path, "metadata.json"), "w") as handle:
        json.dump(dict(min=list(bbox[0]), max=list(bbox[1])), handle)

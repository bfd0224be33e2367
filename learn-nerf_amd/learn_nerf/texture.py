"""
Texture baking (scripts/texture_mesh.py; additive, no counterpart in the reference): a triangle mesh gets a texture
atlas with one right-angled patch per triangle, and the photographs of a dataset are projected into it.  Every texel
knows its surface point and normal (csrc/tex_geom.h fixes the layout, the argument that bilinear sampling never reads
another face's texels, and every fp32 operation); for every view that faces the point, sees it inside its image, is
opaque there and is not occluded (an any-hit ray against the mesh itself, csrc/raycast.hip), the bilinear colour of the
projection is added with weight cos^power.  The state is resolved to bytes, and texels no view saw take the colour of
seen neighbours of their own patch for a few passes.  lnrf_tex_* (csrc/texture.hip, csrc/raycast.hip); TextureAtlas
and bake_views drive them, tests/texture_reference.py restates them in NumPy.

Out of scope: chart-based unwrapping (every face gets the same patch whatever its area, so a mesh with very uneven
triangles wastes texels), seam levelling or exposure compensation between views (view-dependent colour is averaged),
and baking from a model instead of photographs (TextureAtlas.texels() is the hook for that).
"""
import ctypes
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from learn_nerf import _lib as L
from learn_nerf.dataset import CameraView
from learn_nerf.raycast import TriangleMesh

F32 = torch.float32
MIN_CELL = 6  # csrc/tex_geom.h: kMinCell, kMaxCell, kMaxSize
MAX_CELL = 256
MAX_SIZE = 1 << 15
INT32_MAX = 2 ** 31 - 1

# lnrf_tex_view (include/lnrf.h), 64 bytes
VIEW_DTYPE = np.dtype([("origin", "<f4", (3,)), ("inv", "<f4", (9,)), ("width", "<i4"), ("height", "<i4"),
                       ("pixel_offset", "<i8")])
assert VIEW_DTYPE.itemsize == 64

# bake_views() uploads views in chunks of at most this many image bytes (4 per pixel); any chunking gives the same bits
DEFAULT_CHUNK_BYTES = 256 << 20


def atlas_layout(faces: int, texture_size: int) -> Tuple[int, int, int]:
    """(K cells per row, c texels per cell edge, S = K c) for `faces` faces in a texture of at most texture_size.
    ValueError, naming the size that would be needed, when the cells would be smaller than MIN_CELL."""
    faces, texture_size = int(faces), int(texture_size)
    if faces < 1:
        raise ValueError(f"{faces} faces: an atlas needs at least one")
    if texture_size < 1:
        raise ValueError(f"texture_size must be positive, got {texture_size}")
    k = math.isqrt((faces + 1) // 2 - 1) + 1  # ceil(sqrt(ceil(F / 2)))
    cell = min(texture_size // k, MAX_CELL)
    if cell < MIN_CELL or k * MIN_CELL > MAX_SIZE:
        need = k * MIN_CELL
        hint = (f"a texture of at least {need} x {need} is needed" if need <= MAX_SIZE else
                f"it would need {need} x {need}, beyond the largest texture of {MAX_SIZE}")
        raise ValueError(f"texture_size {texture_size} is too small for {faces} faces ({k} x {k} cells of at least "
                         f"{MIN_CELL} texels): {hint}; reduce the mesh first (--target_faces, or simplify_mesh.py)")
    cell = min(cell, MAX_SIZE // k)
    return k, cell, k * cell


def right_angles(tris: np.ndarray) -> np.ndarray:
    """int64 [F]: the corner of each triangle that goes to its patch's right angle (csrc/tex_geom.h "Corners"): the one
    opposite the longest edge, squared lengths in float32 in the header's order, the lowest index among equals."""
    v = np.asarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    lengths = []
    for k in range(3):
        d = v[:, (k + 1) % 3] - v[:, (k + 2) % 3]
        lengths.append((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    r = np.zeros(len(v), dtype=np.int64)
    best = lengths[0].copy()
    for k in (1, 2):
        better = lengths[k] > best
        r[better] = k
        best[better] = lengths[k][better]
    return r


def degenerate_faces(tris: np.ndarray) -> np.ndarray:
    """bool [F]: the faces without a normal, by the header's float32 rule (nn > 0 fails)."""
    v = np.asarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    r = right_angles(v)
    rows = np.arange(len(v))
    a, b, c = v[rows, r], v[rows, (r + 1) % 3], v[rows, (r + 2) % 3]
    e1, e2 = b - a, c - a
    n = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
         e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
    with np.errstate(over="ignore"):
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    return ~(nn > 0)


class TextureAtlas:
    """
    The atlas of `tris` [F, 3, 3] (a torch tensor or an array) in a texture of at most texture_size: F faces, K cells
    per row of c texels, size S = K c.  The layout and vertex_uvs() are host arithmetic; texels(), uv() and sample() are
    HIP kernels and need the triangles on a ROCm GPU (there is no CPU fallback).
    """

    def __init__(self, tris, texture_size: int = 2048):
        if not isinstance(tris, torch.Tensor):
            tris = torch.from_numpy(np.ascontiguousarray(np.asarray(tris, dtype=np.float32)))
        if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
            raise ValueError(f"triangles: expected shape [F, 3, 3], got {tuple(tris.shape)}")
        if tris.shape[0] > INT32_MAX // 2:
            raise ValueError(f"{tris.shape[0]} triangles: too many for an atlas")
        tris = tris.to(F32).contiguous()
        if not torch.isfinite(tris).all():
            raise ValueError("triangles: non-finite coordinates")
        self.F = int(tris.shape[0])
        self.K, self.c, self.S = atlas_layout(self.F, texture_size)
        self.tris = tris
        self.desc = L.TexAtlas(self.F, self.K, self.c, self.S)

    @property
    def texels_used(self) -> int:
        """The texels that belong to a face: c^2 per full cell, the lower half (c (c + 1) / 2) of the last cell when F
        is odd."""
        return (self.F // 2) * self.c * self.c + (self.F % 2) * (self.c * (self.c + 1) // 2)

    def _device_tris(self) -> torch.Tensor:
        if not self.tris.is_cuda:
            raise RuntimeError("the texture kernels need the triangles on a ROCm GPU device (no CPU fallback)")
        return self.tris

    def vertex_uvs(self) -> np.ndarray:
        """float32 [3F, 2]: the atlas coordinates, in texels, of corner k of face f in row 3f + k (OBJ coordinates are
        u = x / S, v = 1 - y / S).  Integers, so exact."""
        c, k = self.c, self.K
        r = right_angles(self.tris.cpu().numpy())
        f = np.arange(self.F)
        pair, upper = f // 2, (f % 2 == 1)
        ox, oy = (pair % k) * c, (pair // k) * c
        # corners A, B, C of the patch, cell-local
        local = np.where(upper[:, None, None], np.array([[c - 1, c - 1], [3, c - 1], [c - 1, 3]]),
                         np.array([[1, 1], [c - 2, 1], [1, c - 2]]))
        out = np.empty((self.F, 3, 2), dtype=np.float32)
        for slot in range(3):  # patch corner `slot` is vertex (r + slot) % 3
            out[f, (r + slot) % 3, 0] = ox + local[:, slot, 0]
            out[f, (r + slot) % 3, 1] = oy + local[:, slot, 1]
        return out.reshape(-1, 2)

    def texels(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(face int32 [S, S] with -1 for none, position fp32 [S, S, 3], unit normal fp32 [S, S, 3] with (0, 0, 0) on a
        zero-area face, barycentrics fp32 [S, S, 3] in the face's vertex order) of every texel [row y, column x]."""
        tris = self._device_tris()
        s, dev = self.S, tris.device
        face = torch.empty((s, s), dtype=torch.int32, device=dev)
        position, normal, bary = (torch.empty((s, s, 3), dtype=F32, device=dev) for _ in range(3))
        L.check(L.lib().lnrf_tex_texels(ctypes.byref(self.desc), L.ptr(tris), L.ptr(face, torch.int32), L.ptr(position),
                                        L.ptr(normal), L.ptr(bary), L.stream()), "tex_texels")
        return face, position, normal, bary

    def uv(self, points: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        """fp32 [m, 2]: atlas coordinates in texels of the surface points [m, 3] of the faces ids [m]."""
        tris = self._device_tris()
        if not isinstance(points, torch.Tensor) or not isinstance(ids, torch.Tensor):
            raise TypeError("points and ids must be torch tensors")
        if points.dim() != 2 or points.shape[1] != 3 or ids.shape != (points.shape[0],):
            raise ValueError(f"expected points [m, 3] and ids [m], got {tuple(points.shape)} and {tuple(ids.shape)}")
        if not (points.is_cuda and ids.is_cuda):
            raise RuntimeError("points and ids: the texture kernels need tensors on a ROCm GPU device (no CPU fallback)")
        points, ids = points.to(F32).contiguous(), ids.to(torch.int32).contiguous()
        m = points.shape[0]
        if m:
            if not torch.isfinite(points).all():
                raise ValueError("points: non-finite coordinates")
            if int(ids.min()) < 0 or int(ids.max()) >= self.F:
                raise ValueError(f"ids: face indices must lie in [0, {self.F})")
        out = torch.empty((m, 2), dtype=F32, device=points.device)
        L.check(L.lib().lnrf_tex_uv(ctypes.byref(self.desc), L.ptr(tris), L.ptr(points), L.ptr(ids, torch.int32), m,
                                    L.ptr(out), L.stream()), "tex_uv")
        return out

    def sample(self, texture: torch.Tensor, uv: torch.Tensor) -> torch.Tensor:
        """fp32 [m, 3]: bilinear samples of texture [H, W, 3] (uint8 or fp32, GPU) at uv [m, 2] in texels; indices are
        clamped at the border."""
        return sample(texture, uv)


def sample(texture: torch.Tensor, uv: torch.Tensor) -> torch.Tensor:
    if not isinstance(texture, torch.Tensor) or not isinstance(uv, torch.Tensor):
        raise TypeError("texture and uv must be torch tensors")
    if texture.dim() != 3 or texture.shape[2] != 3 or texture.dtype not in (torch.uint8, F32):
        raise ValueError(f"texture: expected uint8 or float32 [H, W, 3], got {texture.dtype} {tuple(texture.shape)}")
    if uv.dim() != 2 or uv.shape[1] != 2:
        raise ValueError(f"uv: expected shape [m, 2], got {tuple(uv.shape)}")
    if not (texture.is_cuda and uv.is_cuda):
        raise RuntimeError("texture and uv: the texture kernels need tensors on a ROCm GPU device (no CPU fallback)")
    height, width = int(texture.shape[0]), int(texture.shape[1])
    if not (1 <= height <= MAX_SIZE and 1 <= width <= MAX_SIZE):
        raise ValueError(f"texture: sides must lie in [1, {MAX_SIZE}], got {height} x {width}")
    texture, uv = texture.contiguous(), uv.to(F32).contiguous()
    out = torch.empty((uv.shape[0], 3), dtype=F32, device=uv.device)
    L.check(L.lib().lnrf_tex_sample(L.ptr(texture, texture.dtype), int(texture.dtype == F32), height, width, L.ptr(uv),
                                    uv.shape[0], L.ptr(out), L.stream()), "tex_sample")
    return out


def pack_views(cameras: Sequence[CameraView], sizes: Sequence[Tuple[int, int]]) -> np.ndarray:
    """-> lnrf_tex_view descriptors (VIEW_DTYPE [n]) of `cameras` with images of `sizes` = (width, height), packed one
    after the other in view order: origin and inv of learn_nerf.tsdf.pack_views, which inverts CameraView.bare_rays
    also for axes that are not orthonormal, without what only depth needs."""
    from learn_nerf.tsdf import pack_views as pack_tsdf_views

    full = pack_tsdf_views(cameras, sizes)
    out = np.zeros(len(full), dtype=VIEW_DTYPE)
    for name in ("origin", "inv", "width", "height"):
        out[name] = full[name]
    out["pixel_offset"] = full["depth_offset"]
    return out


def as_rgba(image: np.ndarray, index: int = 0) -> np.ndarray:
    """uint8 [H, W, 4] of a uint8 [H, W, 3] (alpha 255) or [H, W, 4] image."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] not in (3, 4):
        raise ValueError(f"view {index}: the image must be uint8 [H, W, 3] or [H, W, 4], got {image.dtype} "
                         f"{image.shape}")
    if image.shape[2] == 4:
        return np.ascontiguousarray(image)
    out = np.full(image.shape[:2] + (4,), 255, dtype=np.uint8)
    out[:, :, :3] = image
    return out


def default_offset(mesh: TriangleMesh) -> float:
    """1e-3 of the diagonal of the mesh's bounding box, rounded to float32."""
    return float(np.float32(1e-3 * float(np.linalg.norm(mesh.hi - mesh.lo))))


class TextureBake:
    """The accumulation state of one bake: add() any number of times, in view order, then finish()."""

    def __init__(self, atlas: TextureAtlas, mesh: TriangleMesh, max_angle: float = math.radians(80.0), power: int = 2,
                 offset: Optional[float] = None):
        tris = atlas._device_tris()
        if not isinstance(mesh, TriangleMesh):
            raise TypeError(f"mesh: expected a TriangleMesh, got {type(mesh)}")
        if mesh.tris.device != tris.device or mesh.tris.shape != tris.shape or not torch.equal(mesh.tris, tris):
            raise ValueError("the atlas and the mesh must hold the same triangles on the same device")
        if not (isinstance(power, int) and 0 <= power <= 64):
            raise ValueError(f"power must be an integer in [0, 64], got {power!r}")
        if not (0 < max_angle <= math.pi / 2):
            raise ValueError(f"max_angle must lie in (0, pi / 2], got {max_angle}")
        offset = default_offset(mesh) if offset is None else float(np.float32(offset))
        if not (offset >= 0 and math.isfinite(offset)):
            raise ValueError(f"offset must be finite and not negative, got {offset}")
        self.atlas, self.mesh, self.power, self.offset = atlas, mesh, power, offset
        self.cos_max = float(np.float32(math.cos(max_angle)))
        self.state = torch.zeros((atlas.S * atlas.S, 4), dtype=F32, device=tris.device)
        self.views = 0

    def upload(self, cameras, images) -> Tuple[torch.Tensor, torch.Tensor]:
        """One launch's inputs on the device: (descriptors as bytes, packed RGBA)."""
        images = [as_rgba(im, i) for i, im in enumerate(images)]
        views = pack_views(cameras, [(im.shape[1], im.shape[0]) for im in images])
        dev = self.state.device
        views_dev = torch.from_numpy(views.view(np.uint8).copy()).to(dev)
        rgba_dev = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(dev)
        return views_dev, rgba_dev

    def add_uploaded(self, views_dev: torch.Tensor, rgba_dev: torch.Tensor) -> None:
        """One lnrf_tex_bake_views launch over the views of upload()."""
        mesh, atlas = self.mesh, self.atlas
        n_views = views_dev.numel() // VIEW_DTYPE.itemsize
        L.check(L.lib().lnrf_tex_bake_views(
            ctypes.byref(mesh.bvh), L.ptr(mesh.sorted_tris), L.ptr(mesh.nodes), ctypes.byref(atlas.desc),
            L.ptr(atlas.tris), L.ptr(views_dev, torch.uint8), n_views, L.ptr(rgba_dev, torch.uint8), self.cos_max,
            self.power, self.offset, L.ptr(self.state), L.stream()), "tex_bake_views")
        self.views += n_views

    def add(self, cameras: Sequence[CameraView], images: Sequence[np.ndarray],
            chunk_bytes: int = DEFAULT_CHUNK_BYTES) -> None:
        """Adds the views, in order: images uint8 [H, W, 3] or [H, W, 4] (a pixel with alpha < 128 is background).  The
        views are uploaded in chunks of at most chunk_bytes image bytes (one view at least), one launch per chunk; the
        result does not depend on the chunking."""
        if len(cameras) != len(images):
            raise ValueError(f"{len(cameras)} cameras and {len(images)} images")
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes must be positive")
        images = [as_rgba(im, i) for i, im in enumerate(images)]
        start = 0
        while start < len(cameras):
            stop, nbytes = start, 0
            while stop < len(cameras) and (stop == start or nbytes + images[stop].size <= chunk_bytes):
                nbytes += images[stop].size
                stop += 1
            # the uploads are freed on return: the caching allocator reuses them in stream order, after the kernel
            self.add_uploaded(*self.upload(cameras[start:stop], images[start:stop]))
            start = stop

    def resolve(self, unseen_color=(128, 128, 128)) -> Tuple[torch.Tensor, torch.Tensor]:
        """(texture uint8 [S, S, 3], seen uint8 [S, S]) of the state as it stands."""
        color = [int(c) for c in unseen_color]
        if len(color) != 3 or not all(0 <= c <= 255 for c in color):
            raise ValueError(f"unseen_color must be three integers in [0, 255], got {unseen_color!r}")
        s, dev = self.atlas.S, self.state.device
        rgb = torch.empty((s, s, 3), dtype=torch.uint8, device=dev)
        seen = torch.empty((s, s), dtype=torch.uint8, device=dev)
        L.check(L.lib().lnrf_tex_resolve(ctypes.byref(self.atlas.desc), L.ptr(self.state), *color,
                                         L.ptr(rgb, torch.uint8), L.ptr(seen, torch.uint8), L.stream()), "tex_resolve")
        return rgb, seen

    def finish(self, fill_passes: int = 8, unseen_color=(128, 128, 128)) -> Tuple[torch.Tensor, torch.Tensor, dict]:
        """(texture uint8 [S, S, 3], seen uint8 [S, S]: 1 seen by a view, 2 filled from neighbours, 0 neither; info)."""
        if not (isinstance(fill_passes, int) and fill_passes >= 0):
            raise ValueError(f"fill_passes must be a non-negative integer, got {fill_passes!r}")
        rgb, seen = self.resolve(unseen_color)
        n_seen = int((seen == 1).sum())
        rgb, seen, filled = fill(self.atlas, rgb, seen, fill_passes)
        used = self.atlas.texels_used
        info = dict(texels_used=used, seen=n_seen, filled=filled, unseen=used - n_seen - filled,
                    degenerate_faces=int(degenerate_faces(self.atlas.tris.cpu().numpy()).sum()), views=self.views)
        return rgb, seen, info


def fill(atlas: TextureAtlas, rgb: torch.Tensor, seen: torch.Tensor, passes: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """`passes` Jacobi passes of lnrf_tex_fill over (rgb uint8 [S, S, 3], seen uint8 [S, S]) -> (rgb, seen, texels
    filled); the counter is read once, after the last pass."""
    s = atlas.S
    if tuple(rgb.shape) != (s, s, 3) or tuple(seen.shape) != (s, s) or rgb.dtype != torch.uint8 or \
            seen.dtype != torch.uint8:
        raise ValueError(f"expected rgb uint8 [{s}, {s}, 3] and seen uint8 [{s}, {s}]")
    if not (rgb.is_cuda and seen.is_cuda):
        raise RuntimeError("rgb and seen: the texture kernels need tensors on a ROCm GPU device (no CPU fallback)")
    if passes == 0:
        return rgb, seen, 0
    rgb, seen = rgb.contiguous(), seen.contiguous()
    counter = torch.zeros(1, dtype=torch.int32, device=rgb.device)
    # ping-pong between two images of its own: the caller's are read by the first pass and never written
    source, spare = (rgb, seen), None
    for _ in range(passes):
        target = spare if spare is not None else (torch.empty_like(rgb), torch.empty_like(seen))
        L.check(L.lib().lnrf_tex_fill(ctypes.byref(atlas.desc), L.ptr(source[0], torch.uint8),
                                      L.ptr(source[1], torch.uint8), L.ptr(target[0], torch.uint8),
                                      L.ptr(target[1], torch.uint8), L.ptr(counter, torch.int32), L.stream()),
                "tex_fill")
        spare = source if source[0] is not rgb else None
        source = target
    return source[0], source[1], int(counter.item())


def bake_views(atlas: TextureAtlas, mesh: TriangleMesh, cameras: Sequence[CameraView], images: Sequence[np.ndarray], *,
               max_angle: float = math.radians(80.0), power: int = 2, offset: Optional[float] = None,
               fill_passes: int = 8, unseen_color=(128, 128, 128), chunk_bytes: int = DEFAULT_CHUNK_BYTES,
               verbose: bool = True) -> Tuple[torch.Tensor, dict]:
    """
    -> (texture uint8 [S, S, 3] on the GPU, info) of `mesh` (a TriangleMesh of atlas.tris) under the views: cameras and
    their images uint8 [H, W, 3] or [H, W, 4].  max_angle (radians): the largest angle between the normal and the
    direction to a camera that still counts; weight cos^power; offset: how far the shadow ray starts off the surface,
    None = 1e-3 of the bounding-box diagonal (the value used is printed); fill_passes: passes that give unseen texels
    the colour of seen neighbours of their patch; what is left gets unseen_color.  info: texels_used, seen, filled,
    unseen, degenerate_faces, views, offset, and seen_mask (uint8 [S, S]: 1 seen, 2 filled).
    """
    bake = TextureBake(atlas, mesh, max_angle=max_angle, power=power, offset=offset)
    if verbose:
        print(f"offset={bake.offset:.9g}")
    bake.add(cameras, images, chunk_bytes=chunk_bytes)
    texture, seen, info = bake.finish(fill_passes, unseen_color)
    info.update(offset=bake.offset, seen_mask=seen)
    return texture, info


# -------------------------------------------------------------- files ----

def weld(tris: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(verts float32 [V, 3], faces int64 [F, 3]): corners with exactly equal coordinates become one vertex, numbered in
    order of first appearance, so an indexed mesh read into triangles gets its indexing back."""
    corners = np.ascontiguousarray(np.asarray(tris, dtype=np.float32).reshape(-1, 3))
    keys = (corners + np.float32(0.0)).view(np.uint32)  # -0.0 + 0.0 = +0.0: equal coordinates, equal bits
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return corners[first[order]], rank[np.asarray(inverse).reshape(-1)].reshape(-1, 3)


def write_textured_obj(path: str, tris, atlas: TextureAtlas, texture) -> Tuple[str, str]:
    """Writes `path` (v, vt and `f v/vt` records), then <stem>.mtl (one material with a map_Kd line) and <stem>.png (the
    texture) beside it -> (mtl path, png path)."""
    from PIL import Image

    if not path.lower().endswith(".obj"):
        raise ValueError(f"{path!r}: expected a .obj file")
    tris = np.asarray(tris.cpu().numpy() if isinstance(tris, torch.Tensor) else tris, dtype=np.float32)
    if tris.shape != (atlas.F, 3, 3):
        raise ValueError(f"triangles: expected shape {(atlas.F, 3, 3)}, got {tris.shape}")
    texture = np.asarray(texture.cpu().numpy() if isinstance(texture, torch.Tensor) else texture)
    if texture.dtype != np.uint8 or texture.shape != (atlas.S, atlas.S, 3):
        raise ValueError(f"texture: expected uint8 {(atlas.S, atlas.S, 3)}, got {texture.dtype} {texture.shape}")
    stem = path[:-4]
    name = os.path.basename(stem)
    verts, faces = weld(tris)
    uvs = atlas.vertex_uvs().astype(np.float64)
    size = float(atlas.S)
    lines = [f"mtllib {name}.mtl", "usemtl baked"]
    lines += [f"v {x!r} {y!r} {z!r}" for x, y, z in verts.astype(np.float64).tolist()]
    lines += [f"vt {x / size!r} {1.0 - y / size!r}" for x, y in uvs.tolist()]
    lines += [f"f {a + 1}/{3 * i + 1} {b + 1}/{3 * i + 2} {c + 1}/{3 * i + 3}" for i, (a, b, c) in
              enumerate(faces.tolist())]
    with open(path, "w") as handle:
        handle.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w") as handle:
        handle.write(f"newmtl baked\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    Image.fromarray(texture, "RGB").save(stem + ".png")
    return stem + ".mtl", stem + ".png"


def read_views(data_dir: str, max_views: Optional[int] = None) -> Tuple[List[CameraView], List[np.ndarray], List[str]]:
    """(cameras, images uint8 [H, W, 4], image paths) of the dataset `data_dir` in the order of load_dataset, the first
    max_views of them; the images keep their alpha (255 where the file has none) and are not pre-multiplied."""
    from PIL import Image

    from learn_nerf.dataset import load_dataset

    views = load_dataset(data_dir).views
    if max_views is not None:
        views = views[:max_views]
    images = []
    for view in views:
        with Image.open(view.image_path) as image:
            images.append(np.ascontiguousarray(np.asarray(image.convert("RGBA"), dtype=np.uint8)))
    return list(views), images, [v.image_path for v in views]


# ---------------------------------------------------------------- check ----

def reprojection_psnr(atlas: TextureAtlas, mesh: TriangleMesh, texture: torch.Tensor, cameras: Sequence[CameraView],
                      images: Sequence[np.ndarray]) -> Tuple[List[float], float]:
    """
    (PSNR per view, their mean) of the textured mesh seen from the views: every pixel's ray (CameraView.bare_rays) is
    cast, the first hit goes through uv() and sample(), and the colour is compared with the image as [0, 1] values over
    the pixels that hit and have alpha >= 128; PSNR = -10 log10(mse), the squared errors summed in float64 (torch).  A
    view without such a pixel gives nan and is left out of the mean.
    """
    if len(cameras) != len(images):
        raise ValueError(f"{len(cameras)} cameras and {len(images)} images")
    dev = atlas._device_tris().device
    texture = texture.to(dev)
    out = []
    for i, (cam, image) in enumerate(zip(cameras, images)):
        image = as_rgba(image, i)
        height, width = image.shape[:2]
        rays = cam.bare_rays(width, height, device=dev)
        t, idx = mesh.closest(rays)
        pixels = torch.from_numpy(image.reshape(-1, 4)).to(dev)
        keep = torch.nonzero((idx >= 0) & (pixels[:, 3] >= 128)).view(-1)
        if keep.numel() == 0:
            out.append(math.nan)
            continue
        points = rays[keep, 0] + t[keep, None] * rays[keep, 1]
        colors = atlas.sample(texture, atlas.uv(points, idx[keep]))
        diff = colors.double() / 255 - pixels[keep, :3].double() / 255
        mse = float((diff * diff).sum() / diff.numel())
        out.append(math.inf if mse == 0 else -10 * math.log10(mse))
    finite = [p for p in out if not math.isnan(p)]
    return out, (math.fsum(finite) / len(finite) if finite else math.nan)

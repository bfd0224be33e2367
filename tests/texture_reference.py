"""
NumPy restatement of csrc/tex_geom.h and of the passes built on it (csrc/texture.hip, lnrf_tex_bake_views in
csrc/raycast.hip): float32 arrays throughout, one NumPy call per rounded operation, in the header's order.  Occlusion is
the brute force of tests/raycast_reference.py.  The patch corners take a `shift` so that a test can move a patch towards
the diagonal and watch the no-bleed property fail.
"""
import math

import numpy as np

import raycast_reference as RC

F32 = np.float32
MIN_CELL, MAX_CELL, MAX_SIZE = 6, 256, 1 << 15


def f32(x):
    return np.asarray(x, dtype=F32)


# ---- layout ---------------------------------------------------------------------------------------------------------
def layout(faces, texture_size):
    """(K, c, S): K = ceil(sqrt(ceil(F / 2))), c = min(texture_size // K, MAX_CELL), S = K c."""
    pairs = (faces + 1) // 2
    k = 1
    while k * k < pairs:
        k += 1
    c = min(texture_size // k, MAX_CELL)
    if c < MIN_CELL:
        raise ValueError(f"needs {k * MIN_CELL}")
    return k, c, k * c


def texel_faces(faces, k, c):
    """(face int32 [S, S] indexed [y, x], -1 for none; cell-local i, j int [S, S])."""
    s = k * c
    y, x = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    i, j = x % c, y % c
    f = 2 * ((y // c) * k + x // c) + np.where(i + j + 1 <= c, 0, 1)
    return np.where(f < faces, f, -1).astype(np.int32), i, j


def patch_corners(c, half, shift=0):
    """Cell-local UV corners (A, B, C) of a patch; shift moves the patch that many texels towards the diagonal."""
    if half == 0:
        base = [(1, 1), (c - 2, 1), (1, c - 2)]
        return [(x + shift, y + shift) for x, y in base]
    base = [(c - 1, c - 1), (3, c - 1), (c - 1, 3)]
    return [(x - shift, y - shift) for x, y in base]


def cell_origin(f, k, c):
    pair = np.asarray(f) // 2
    return (pair % k) * c, (pair // k) * c


# ---- faces ----------------------------------------------------------------------------------------------------------
def right_angles(tris):
    v = f32(tris).reshape(-1, 3, 3)
    lengths = []
    for a in range(3):
        d = v[:, (a + 1) % 3] - v[:, (a + 2) % 3]
        lengths.append((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    r = np.zeros(len(v), dtype=np.int64)
    best = lengths[0].copy()
    for a in (1, 2):
        better = lengths[a] > best
        r[better] = a
        best = np.where(better, lengths[a], best)
    return r


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def frames(tris):
    """dict of per-face arrays: r, a [F, 3], e1, e2, n (lists of 3 arrays [F]), nn, degenerate, normal [F, 3]."""
    v = f32(tris).reshape(-1, 3, 3)
    r = right_angles(v)
    rows = np.arange(len(v))
    a, b, c = v[rows, r], v[rows, (r + 1) % 3], v[rows, (r + 2) % 3]
    e1 = [b[:, k] - a[:, k] for k in range(3)]
    e2 = [c[:, k] - a[:, k] for k in range(3)]
    n = _cross(e1, e2)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        nn = _dot(n, n)
        degenerate = ~(nn > 0)
        length = np.sqrt(nn)
        normal = np.stack([np.where(degenerate, F32(0), n[k] / length) for k in range(3)], axis=1).astype(F32)
    return dict(r=r, a=a, e1=e1, e2=e2, n=n, nn=nn, degenerate=degenerate, normal=normal)


def clamp_bary(bb, bc):
    bb = np.where(bb > 0, bb, F32(0)).astype(F32)
    bc = np.where(bc > 0, bc, F32(0)).astype(F32)
    s = bb + bc
    over = s > 1
    safe = np.where(over, s, F32(1))
    return np.where(over, bb / safe, bb).astype(F32), np.where(over, bc / safe, bc).astype(F32)


def texel_bary(c, half, i, j):
    """Clamped (bB, bC) of the centres of the cell-local texels (i, j) of halves `half` (arrays)."""
    px, py = f32(i) + F32(0.5), f32(j) + F32(0.5)
    lower_b, lower_c = (px - F32(1)) / F32(c - 3), (py - F32(1)) / F32(c - 3)
    upper_b, upper_c = (F32(c - 1) - px) / F32(c - 4), (F32(c - 1) - py) / F32(c - 4)
    half = np.asarray(half)
    return clamp_bary(np.where(half == 0, lower_b, upper_b), np.where(half == 0, lower_c, upper_c))


def texel_geometry(tris, k, c):
    """lnrf_tex_texels: (face int32 [S, S], position, normal, bary float32 [S, S, 3])."""
    tris = f32(tris).reshape(-1, 3, 3)
    face, i, j = texel_faces(len(tris), k, c)
    fr = frames(tris)
    s = k * c
    position, normal, bary = (np.zeros((s, s, 3), dtype=F32) for _ in range(3))
    used = face >= 0
    f = face[used].astype(np.int64)
    bb, bc = texel_bary(c, f % 2, i[used], j[used])
    for a in range(3):
        position[used, a] = (fr["a"][f, a] + bb * fr["e1"][a][f]) + bc * fr["e2"][a][f]
    normal[used] = fr["normal"][f]
    w = np.zeros((len(f), 3), dtype=F32)
    rows = np.arange(len(f))
    r = fr["r"][f]
    w[rows, r] = (F32(1) - bb) - bc
    w[rows, (r + 1) % 3] = bb
    w[rows, (r + 2) % 3] = bc
    bary[used] = w
    return face, position, normal, bary


def vertex_uvs(tris, k, c):
    """float32 [3F, 2], texels: the patch corner of every face corner."""
    tris = f32(tris).reshape(-1, 3, 3)
    r = right_angles(tris)
    out = np.zeros((len(tris), 3, 2), dtype=F32)
    for f in range(len(tris)):
        ox, oy = cell_origin(f, k, c)
        for slot, (x, y) in enumerate(patch_corners(c, f % 2)):
            out[f, (r[f] + slot) % 3] = (ox + x, oy + y)
    return out.reshape(-1, 2)


def point_uv(tris, k, c, points, ids):
    """lnrf_tex_uv: float32 [m, 2]."""
    tris = f32(tris).reshape(-1, 3, 3)
    fr = frames(tris)
    q = f32(points).reshape(-1, 3)
    f = np.asarray(ids, dtype=np.int64)
    w = [q[:, a] - fr["a"][f, a] for a in range(3)]
    e1 = [fr["e1"][a][f] for a in range(3)]
    e2 = [fr["e2"][a][f] for a in range(3)]
    n = [fr["n"][a][f] for a in range(3)]
    nn, deg = fr["nn"][f], fr["degenerate"][f]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        bb = np.where(deg, F32(0), _dot(_cross(w, e2), n) / nn).astype(F32)
        bc = np.where(deg, F32(0), _dot(_cross(e1, w), n) / nn).astype(F32)
    bb, bc = clamp_bary(bb, bc)
    lower_x, lower_y = F32(1) + bb * F32(c - 3), F32(1) + bc * F32(c - 3)
    upper_x, upper_y = F32(c - 1) - bb * F32(c - 4), F32(c - 1) - bc * F32(c - 4)
    half = f % 2
    ox, oy = cell_origin(f, k, c)
    x = f32(ox) + np.where(half == 0, lower_x, upper_x).astype(F32)
    y = f32(oy) + np.where(half == 0, lower_y, upper_y).astype(F32)
    return np.stack([x, y], axis=1).astype(F32)


# ---- sampling -------------------------------------------------------------------------------------------------------
def tap_at(x, n):
    """(i0, i1 int64, t float32) of the header's tap_at for an array x."""
    x = f32(x)
    with np.errstate(invalid="ignore"):
        fl = np.floor(x)
        t = (x - fl).astype(F32)
        nx = np.where(t > 0, fl + F32(1), fl).astype(F32)
        last = F32(n - 1)

        def index(v):
            return np.where(v > 0, np.where(v < last, v, last), F32(0)).astype(np.int64)

        return index(fl), index(nx), t


def bilerp(c00, c10, c01, c11, tx, ty):
    top = c00 + tx * (c10 - c00)
    bottom = c01 + tx * (c11 - c01)
    return (top + ty * (bottom - top)).astype(F32)


def sample(texture, uv):
    """lnrf_tex_sample: float32 [m, 3] of texture [H, W, 3] (uint8 or float32) at uv [m, 2] in texels."""
    texture = np.asarray(texture)
    uv = f32(uv).reshape(-1, 2)
    i0, i1, tx = tap_at(uv[:, 0] - F32(0.5), texture.shape[1])
    j0, j1, ty = tap_at(uv[:, 1] - F32(0.5), texture.shape[0])
    tex = texture.astype(F32)
    with np.errstate(invalid="ignore"):
        return np.stack([bilerp(tex[j0, i0, k], tex[j0, i1, k], tex[j1, i0, k], tex[j1, i1, k], tx, ty)
                         for k in range(3)], axis=1)


# ---- views ----------------------------------------------------------------------------------------------------------
def project(view, p):
    """(xf, yf float32 [m], in front bool [m]) of points p [m, 3] under one descriptor (origin, inv, width, height)."""
    origin, inv = f32(view["origin"]), f32(view["inv"]).reshape(9)
    d = [p[:, a] - origin[a] for a in range(3)]
    a = (d[0] * inv[0] + d[1] * inv[1]) + d[2] * inv[2]
    b = (d[0] * inv[3] + d[1] * inv[4]) + d[2] * inv[5]
    s = (d[0] * inv[6] + d[1] * inv[7]) + d[2] * inv[8]
    with np.errstate(invalid="ignore", divide="ignore"):
        front = s > 0
        xf = ((a / s + F32(1)) * F32(0.5)) * F32(int(view["width"]) - 1)
        yf = ((b / s + F32(1)) * F32(0.5)) * F32(int(view["height"]) - 1)
    return xf.astype(F32), yf.astype(F32), front


def as_rgba(image):
    image = np.asarray(image, dtype=np.uint8)
    if image.shape[2] == 4:
        return image
    return np.concatenate([image, np.full(image.shape[:2] + (1,), 255, np.uint8)], axis=2)


def new_state(size):
    return np.zeros((size, size, 4), dtype=F32)


def bake(tris, k, c, views, images, cos_max, power, offset, state=None, stats=None):
    """
    lnrf_tex_bake_views over the descriptors `views` (learn_nerf.texture.pack_views; origin, inv, width, height are read)
    and their images, in order -> state float32 [S, S, 4], updated in place when given.  stats (a dict) receives
    `traversals`: the (texel, view) pairs that reached the occlusion test.
    """
    tris = f32(tris).reshape(-1, 3, 3)
    face, position, normal, _ = texel_geometry(tris, k, c)
    fr = frames(tris)
    state = new_state(k * c) if state is None else state
    live = face >= 0
    live[live] = ~fr["degenerate"][face[live]]
    ys, xs = np.nonzero(live)
    p, n = position[ys, xs], normal[ys, xs]
    cos_max, offset = F32(cos_max), F32(offset)
    start = np.stack([p[:, a] + offset * n[:, a] for a in range(3)], axis=1).astype(F32)
    traversals = 0
    for view, image in zip(views, images):
        image = as_rgba(image)
        width, height = int(view["width"]), int(view["height"])
        assert image.shape[:2] == (height, width)
        origin = f32(view["origin"])
        v = [origin[a] - p[:, a] for a in range(3)]
        with np.errstate(invalid="ignore", divide="ignore"):
            dist = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            ok = dist > 0
            l = [v[a] / dist for a in range(3)]
            cosv = (n[:, 0] * l[0] + n[:, 1] * l[1]) + n[:, 2] * l[2]
            ok &= cosv > cos_max
            xf, yf, front = project(view, p)
            ok &= front & (xf >= 0) & (xf <= F32(width - 1)) & (yf >= 0) & (yf <= F32(height - 1))
        i0, i1, tx = tap_at(xf, width)
        j0, j1, ty = tap_at(yf, height)
        pix = [image[j0, i0], image[j0, i1], image[j1, i0], image[j1, i1]]  # c00, c10, c01, c11
        for q in pix:
            ok &= q[:, 3] >= 128
        idx = np.nonzero(ok)[0]
        traversals += len(idx)
        if len(idx) == 0:
            continue
        rays = np.stack([start[idx], np.stack([l[a][idx] for a in range(3)], axis=1)], axis=1).astype(F32)
        occluded = RC.brute_force(tris, rays, 0.0, dist[idx])[2]
        idx = idx[occluded == 0]
        w = np.ones(len(idx), dtype=F32)
        for _ in range(power):
            w = w * cosv[idx]
        sy, sx = ys[idx], xs[idx]
        for ch in range(3):
            value = bilerp(*(q[idx, ch].astype(F32) for q in pix), tx[idx], ty[idx])
            state[sy, sx, ch] = state[sy, sx, ch] + w * value
        state[sy, sx, 3] = state[sy, sx, 3] + w
    if stats is not None:
        stats["traversals"] = stats.get("traversals", 0) + traversals
    return state


def resolve(state, unseen_color=(128, 128, 128)):
    """lnrf_tex_resolve: (rgb uint8 [S, S, 3], seen uint8 [S, S])."""
    state = f32(state)
    weight = state[:, :, 3]
    seen = weight > 0
    rgb = np.empty(state.shape[:2] + (3,), dtype=np.uint8)
    safe = np.where(seen, weight, F32(1))
    for ch in range(3):
        x = (state[:, :, ch] / safe) / F32(255)
        x = np.where(x > 0, x, F32(0)).astype(F32)
        x = np.where(x < 1, x, F32(1)).astype(F32)
        byte = np.floor(F32(255) * x + F32(0.5)).astype(np.uint8)
        rgb[:, :, ch] = np.where(seen, byte, np.uint8(unseen_color[ch]))
    return rgb, seen.astype(np.uint8)


def fill_pass(face, rgb, seen):
    """lnrf_tex_fill: one pass -> (rgb, seen, texels filled)."""
    s = face.shape[0]
    want = (seen == 0) & (face >= 0)
    total = np.zeros((s, s, 3), dtype=np.int64)
    count = np.zeros((s, s), dtype=np.int64)
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        ys, xs = np.nonzero(want)
        ny, nx = ys + dy, xs + dx
        inside = (nx >= 0) & (nx < s) & (ny >= 0) & (ny < s)
        ys, xs, ny, nx = ys[inside], xs[inside], ny[inside], nx[inside]
        good = (seen[ny, nx] != 0) & (face[ny, nx] == face[ys, xs])
        ys, xs, ny, nx = ys[good], xs[good], ny[good], nx[good]
        total[ys, xs] += rgb[ny, nx].astype(np.int64)
        count[ys, xs] += 1
    got = want & (count > 0)
    out_rgb, out_seen = rgb.copy(), seen.copy()
    n = count[got][:, None]
    out_rgb[got] = ((2 * total[got] + n) // (2 * n)).astype(np.uint8)
    out_seen[got] = 2
    return out_rgb, out_seen, int(got.sum())


def fill(face, rgb, seen, passes):
    filled = 0
    for _ in range(passes):
        rgb, seen, n = fill_pass(face, rgb, seen)
        filled += n
    return rgb, seen, filled


def bake_texture(tris, k, c, views, images, cos_max, power, offset, fill_passes=8, unseen_color=(128, 128, 128)):
    """The whole of learn_nerf.texture.bake_views -> (texture, seen after filling, state, info)."""
    tris = f32(tris).reshape(-1, 3, 3)
    state = bake(tris, k, c, views, images, cos_max, power, offset)
    rgb, seen = resolve(state, unseen_color)
    n_seen = int((seen == 1).sum())
    face = texel_faces(len(tris), k, c)[0]
    rgb, seen, filled = fill(face, rgb, seen, fill_passes)
    used = int((face >= 0).sum())
    info = dict(texels_used=used, seen=n_seen, filled=filled, unseen=used - n_seen - filled,
                degenerate_faces=int(frames(tris)["degenerate"].sum()), views=len(views))
    return rgb, seen, state, info


def cos_of(max_angle_degrees):
    return F32(math.cos(math.radians(max_angle_degrees)))


def default_offset(tris):
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    return F32(1e-3 * float(np.linalg.norm(t.max(axis=0) - t.min(axis=0))))

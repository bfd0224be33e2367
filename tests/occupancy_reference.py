"""
NumPy float32 restatement of the occupancy-grid kernels (csrc/occupancy.hip, csrc/occ_geom.h): build, clip and
compaction, operation by operation, so that the GPU results can be compared bit for bit; and float64 brute-force
definitions that the restatement itself is checked against (tests/test_occupancy_cpu.py).

`mutate` switches on one seeded defect of the restatement; the brute-force checkers must reject each of them.
"""
import numpy as np

F = np.float32
PAD_ABS = F(2.0 ** -21)  # 8 * 2^-24
PAD_REL = F(2.0 ** -22)  # 4 * 2^-24
MUTATIONS = ("pad0_shrunk_last", "no_tie_break", "plane_off_by_one", "no_dilate")


# ---------------------------------------------------------------------------------------------- bit layout
def pack_bits(occ: np.ndarray) -> np.ndarray:
    """bool [R, R, R] -> uint32 [ceil(R^3 / 32)]: cell (i*R + j)*R + k is bit idx & 31 of word idx >> 5."""
    flat = np.asarray(occ, bool).reshape(-1)
    padded = np.zeros((flat.size + 31) // 32 * 32, dtype=np.uint64)
    padded[:flat.size] = flat
    words = (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    return words.astype(np.uint32)


def unpack_bits(bits: np.ndarray, res: int) -> np.ndarray:
    idx = np.arange(res ** 3)
    flat = (np.asarray(bits, np.uint32)[idx >> 5] >> (idx & 31).astype(np.uint32)) & np.uint32(1)
    return flat.astype(bool).reshape(res, res, res)


def popcount(bits: np.ndarray) -> int:
    return int(np.unpackbits(np.asarray(bits, np.uint32).view(np.uint8)).sum())


# ---------------------------------------------------------------------------------------------- build
def build(sigma, res: int, sigma_thr, dilate: int, mutate=None):
    """lnrf_occ_build: (bits uint32, count).  sigma: (res + 1)^3 corner densities."""
    s = np.asarray(sigma, F).reshape(res + 1, res + 1, res + 1)
    thr = F(sigma_thr)
    raw = np.zeros((res, res, res), bool)
    for c in range(8):
        di, dj, dk = c >> 2, (c >> 1) & 1, c & 1
        with np.errstate(invalid="ignore"):
            raw |= ~(s[di:di + res, dj:dj + res, dk:dk + res] < thr)
    occ = raw.copy()
    if mutate != "no_dilate":
        reach = min(dilate, res - 1)
        for axis in range(3):  # a Chebyshev ball is a product of intervals: one 1-d dilation per axis
            grown = occ.copy()
            for shift in range(1, reach + 1):
                lo = [slice(None)] * 3
                hi = [slice(None)] * 3
                lo[axis], hi[axis] = slice(0, res - shift), slice(shift, res)
                grown[tuple(lo)] |= occ[tuple(hi)]
                grown[tuple(hi)] |= occ[tuple(lo)]
            occ = grown
    return pack_bits(occ), int(occ.sum())


def build_f64(sigma, res: int, sigma_thr, dilate: int) -> np.ndarray:
    """The definition, cell by cell in float64: occupied [R, R, R] bool."""
    s = np.asarray(sigma, np.float64).reshape(res + 1, res + 1, res + 1)
    thr = float(F(sigma_thr))
    raw = np.zeros((res, res, res), bool)
    for i in range(res):
        for j in range(res):
            for k in range(res):
                corners = s[i:i + 2, j:j + 2, k:k + 2]
                top = np.nan if np.isnan(corners).any() else corners.max()  # a max that NaN wins
                raw[i, j, k] = not (top < thr)
    occ = np.zeros_like(raw)
    for i in range(res):
        for j in range(res):
            for k in range(res):
                occ[i, j, k] = raw[max(i - dilate, 0):i + dilate + 1, max(j - dilate, 0):j + dilate + 1,
                                   max(k - dilate, 0):k + dilate + 1].any()
    return occ


# ---------------------------------------------------------------------------------------------- clip
def _pad(amp, den, eps, t):
    at = np.abs(t)
    return (PAD_ABS * amp + eps * at) / np.abs(den) + PAD_REL * at


def clip(rays, bbox_min, bbox_max, res: int, bits, t_min, t_max, mask, min_t_range=1e-3, eps=1e-8, mutate=None):
    """lnrf_occ_clip_rays (occ_clip_ray of occ_geom.h) for rays [N, >=2, 3] -> (t_min', t_max', mask' uint8)."""
    rays = np.asarray(rays, F)
    n = rays.shape[0]
    o, d = rays[:, 0, :], rays[:, 1, :]
    bmin, bmax = np.asarray(bbox_min, F), np.asarray(bbox_max, F)
    eps, mtr = F(eps), F(min_t_range)
    t_min, t_max = np.asarray(t_min, F), np.asarray(t_max, F)
    bits = np.asarray(bits, np.uint32)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        den = d + eps
        h = (bmax - bmin) / F(res)
        amp = (np.abs(bmin) + np.abs(bmax)) + np.abs(o)
        step = np.where(den > 0, 1, np.where(den < 0, -1, 0)).astype(np.int64)
        x = o + d * t_min[:, None]
        cf = np.floor((x - bmin) / h)
        c = np.where(cf >= F(res - 1), F(res - 1), np.where(cf > 0, cf, F(0))).astype(np.int64)

        active = np.asarray(mask).astype(bool).copy()
        found = np.zeros(n, bool)
        t_first, pad_first = np.zeros(n, F), np.zeros(n, F)
        t_last, pad_last = np.zeros(n, F), np.zeros(n, F)
        t_enter, enter_axis = t_min.copy(), np.full(n, -1, np.int64)
        for _ in range(3 * res + 3):
            if not active.any():
                break
            idx = (c[:, 0] * res + c[:, 1]) * res + c[:, 2]
            occupied = ((bits[idx >> 5] >> (idx & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
            plane = c + (step > 0) if mutate != "plane_off_by_one" else c
            tn = ((bmin + plane.astype(F) * h) - o) / den
            tn = np.where(step == 0, F(np.inf), tn).astype(F)
            if mutate == "no_tie_break":  # strict comparisons both ways: a tie falls through to z
                first = (tn[:, 0] < tn[:, 1]) & (tn[:, 0] < tn[:, 2])
                second = (tn[:, 1] < tn[:, 0]) & (tn[:, 1] < tn[:, 2])
                axis = np.where(first, 0, np.where(second, 1, 2))
                t_exit = tn[rows, axis]
            else:
                axis = np.zeros(n, np.int64)
                t_exit = tn[:, 0].copy()
                for a in (1, 2):
                    lower = tn[:, a] < t_exit
                    axis = np.where(lower, a, axis)
                    t_exit = np.where(lower, tn[:, a], t_exit)
            nxt = c[rows, axis] + step[rows, axis]
            leaves = ~(t_exit < t_max) | (nxt < 0) | (nxt >= res)
            hit = active & occupied
            newly = hit & ~found
            ea = np.maximum(enter_axis, 0)
            pf = np.where(enter_axis < 0, F(0), _pad(amp[rows, ea], den[rows, ea], eps, t_enter)).astype(F)
            t_first = np.where(newly, t_enter, t_first)
            pad_first = np.where(newly, pf, pad_first)
            found |= newly
            pl = _pad(amp[rows, axis], den[rows, axis], eps, t_exit).astype(F)
            t_last = np.where(hit, np.where(leaves, F(np.inf), t_exit), t_last).astype(F)
            pad_last = np.where(hit, np.where(leaves, F(0), pl), pad_last).astype(F)
            advance = active & ~leaves
            c[rows[advance], axis[advance]] = nxt[advance]
            t_enter = np.where(advance, t_exit, t_enter)
            enter_axis = np.where(advance, axis, enter_axis)
            active = advance
        capped = active  # still walking after 3R + 3 steps: returned unclipped

        if mutate == "pad0_shrunk_last":
            pad_first, pad_last = np.zeros(n, F), np.zeros(n, F)
            t_last = (t_last * F(1.0 - 2.0 ** -6)).astype(F)
        lo = np.fmax(t_min, t_first - pad_first)
        hi = np.fmin(t_max, np.fmax(t_last + pad_last, lo + mtr))
    alive = np.asarray(mask).astype(bool) & (found | capped)
    lo = np.where(capped, t_min, lo)
    hi = np.where(capped, t_max, hi)
    out_lo = np.where(alive, lo, F(0)).astype(F)
    out_hi = np.where(alive, hi, mtr).astype(F)
    return out_lo, out_hi, alive.astype(np.uint8)


def box_range(rays, bbox_min, bbox_max, min_t_range=1e-3, eps=1e-8):
    """ray_t_range of csrc/ray_geom.h in float32 -> (t_min, t_max, mask uint8), the inputs of clip."""
    rays = np.asarray(rays, F)
    o, d = rays[:, 0, :], rays[:, 1, :]
    bmin, bmax = np.asarray(bbox_min, F), np.asarray(bbox_max, F)
    with np.errstate(all="ignore"):
        den = d + F(eps)
        t0, t1 = (bmin - o) / den, (bmax - o) / den
        lo = np.full(len(rays), -np.inf, F)
        hi = np.full(len(rays), np.inf, F)
        for a in range(3):
            lo = np.fmax(lo, np.fmin(t0[:, a], t1[:, a]))
            hi = np.fmin(hi, np.fmax(t0[:, a], t1[:, a]))
        min_t = np.fmax(F(0), lo)
        max_c = np.fmax(hi, min_t + F(min_t_range))
        mask = min_t < hi
    return (np.where(mask, min_t, F(0)).astype(F), np.where(mask, max_c, F(min_t_range)).astype(F),
            mask.astype(np.uint8))


def compact(mask):
    """lnrf_compact_mask: (ascending int32 indices of the non-zero entries, their count)."""
    idx = np.nonzero(np.asarray(mask) != 0)[0].astype(np.int32)
    return idx, int(idx.size)


# ---------------------------------------------------------------------------------------------- test inputs
BOX_MIN, BOX_MAX = (-1.0, -0.5, -2.0), (1.0, 0.7, 0.3)  # anisotropic on purpose
GRID_KINDS = ("empty", "full", "single", "random5", "shell")


def make_grid(kind: str, res: int, seed: int = 0) -> np.ndarray:
    """occupied [R, R, R] bool of one of GRID_KINDS."""
    rng = np.random.default_rng(seed)
    occ = np.zeros((res, res, res), bool)
    if kind == "full":
        occ[:] = True
    elif kind == "single":
        occ[tuple(rng.integers(0, res, 3))] = True
    elif kind == "random5":
        occ = rng.random((res, res, res)) < 0.05
    elif kind == "shell":  # a hollow box two cells inside the grid (the whole grid where that does not fit)
        m = 1 if res >= 4 else 0
        occ[m:res - m, m:res - m, m:res - m] = True
        if res - 2 * m > 2:
            occ[m + 1:res - m - 1, m + 1:res - m - 1, m + 1:res - m - 1] = False
    elif kind != "empty":
        raise ValueError(kind)
    return occ


def make_rays(n: int, res: int, seed: int = 0, bbox_min=BOX_MIN, bbox_max=BOX_MAX) -> np.ndarray:
    """[n, 2, 3] float32: hand-made rays first (as many as fit), random rays after them."""
    rng = np.random.default_rng(seed)
    bmin, bmax = np.asarray(bbox_min, F), np.asarray(bbox_max, F)
    h = (bmax - bmin) / F(res)
    centre, size = (bmin + bmax) / F(2), bmax - bmin
    plane = lambda a, p: F(bmin[a] + F(p) * h[a])  # noqa: E731  (the fp32 plane the walk uses)
    mid = res // 2
    hand = []
    # origin inside the box, general and axis-aligned directions
    hand.append((centre + F(0.013) * size, (0.3, -0.5, 0.8)))
    hand.append((centre, (1.0, 0.0, 0.0)))
    hand.append((centre, (0.0, -0.0, -1.0)))
    # components exactly 0.0 and -0.0, from outside
    hand.append(((-3.0, 0.05, -0.9), (1.0, 0.0, -0.0)))
    hand.append(((0.1, 3.0, -0.9), (-0.0, -1.0, 0.0)))
    hand.append(((0.1, 0.05, 4.0), (0.0, 0.0, -1.0)))
    # rays lying in a cell plane (a coordinate exactly on a plane, no motion along that axis)
    hand.append(((plane(0, mid), -3.0, -0.9), (0.0, 1.0, 0.1)))
    hand.append(((-3.0, plane(1, mid), plane(2, mid)), (1.0, 0.0, 0.0)))
    hand.append(((plane(0, 0), plane(1, res), -5.0), (0.0, -0.0, 1.0)))  # along a box edge
    # rays through cell corners: along the cell diagonal through lattice points, both ways, and in a face diagonal
    corner = np.array([plane(0, mid), plane(1, mid), plane(2, mid)], F)
    for sign in (1.0, -1.0):
        hand.append((corner - F(sign * 4.0) * h, tuple(F(sign) * h)))
    hand.append((corner - F(4.0) * np.array([h[0], h[1], 0], F), (h[0], h[1], 0.0)))
    hand.append((corner - F(4.0) * np.array([h[0], -h[1], h[2]], F), (h[0], -h[1], h[2])))
    # rays missing the box
    hand.append(((0.0, 5.0, 0.0), (1.0, 0.0, 0.0)))
    hand.append(((4.0, 4.0, 4.0), (1.0, 1.0, 1.0)))
    rays = np.zeros((n, 2, 3), F)
    k = min(n, len(hand))
    for i in range(k):
        o, d = np.asarray(hand[i][0], F), np.asarray(hand[i][1], np.float64)
        rays[i, 0] = o
        rays[i, 1] = (d / np.linalg.norm(d)).astype(F)  # keeps the sign of -0.0
    m = n - k
    if m:
        o = rng.normal(size=(m, 3))
        o = 3.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
        o[: m // 4] = centre + (rng.random((m // 4, 3)) - 0.5) * size * 0.98  # a quarter starts inside
        target = centre + (rng.random((m, 3)) - 0.5) * size * 1.6  # some miss
        d = target - o
        rays[k:, 0] = o.astype(F)
        rays[k:, 1] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return rays


# ---------------------------------------------------------------------------------------------- brute force
def conservativeness_violations(rays, bbox_min, bbox_max, res: int, occ, t_min, t_max, mask, lo, hi, mask_out,
                                samples: int = 4096, standoff: float = 1e-4) -> int:
    """
    Float64 brute force: `samples` points per ray over [t_min, t_max]; a point whose cell (found in float64) is
    occupied and which stays `standoff` of a cell away from every cell face must lie inside the clipped range of a ray
    that is still live.  Returns the number of points for which that fails (the allowance is zero).
    """
    rays = np.asarray(rays, np.float64)
    o, d = rays[:, 0, :], rays[:, 1, :]
    bmin, bmax = np.asarray(bbox_min, F).astype(np.float64), np.asarray(bbox_max, F).astype(np.float64)
    t_min, t_max = np.asarray(t_min, np.float64), np.asarray(t_max, np.float64)
    t = t_min[:, None] + (t_max - t_min)[:, None] * np.linspace(0.0, 1.0, samples)[None, :]
    g = (o[:, None, :] + d[:, None, :] * t[..., None] - bmin) / (bmax - bmin) * res
    cell = np.floor(g)
    frac = g - cell
    inside = ((cell >= 0) & (cell < res)).all(-1)
    clear = ((frac >= standoff) & (frac <= 1.0 - standoff)).all(-1)
    ci = np.clip(cell, 0, res - 1).astype(np.int64)
    occupied = np.asarray(occ, bool)[ci[..., 0], ci[..., 1], ci[..., 2]]
    must = (np.asarray(mask) != 0)[:, None] & inside & clear & occupied
    kept = ((np.asarray(mask_out) != 0)[:, None] & (t >= np.asarray(lo, np.float64)[:, None])
            & (t <= np.asarray(hi, np.float64)[:, None]))
    return int((must & ~kept).sum())

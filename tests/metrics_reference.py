"""
Float64 NumPy restatement of the image metrics (learn_nerf/metrics.py, csrc/image_metrics.hip), for tests only: the
separable 11-tap Gaussian filter over the valid region, the SSIM map of Wang et al. 2004, its mean, PSNR, and the two
unit conversions in fp32 — with the error bounds that the GPU tests hold the kernel to.  ssim_map takes switches that turn
the definition into the wrong variants a port is likely to produce; the CPU tests check that the bounds reject each.

DERIVED BOUNDS (u = 2^-53; everything below is computed from u, TAPS, C1 and C2, nothing is a literal).

An entry.  Let E bound the distance of ANY fp64 evaluation of an entry, in any order of its sums, from the exact real
value; two such evaluations (the kernel and this file) are then within PER_ENTRY = 2 E.
 * Taps.  exp() within one ulp (2u relative), the sum of TAPS positive terms ((TAPS - 1) u), one division (u):
   TAP_REL = (TAPS + 2) u relative per tap.
 * Moments.  Each of mu_x, mu_y, E[xx], E[yy], E[xy] is sum_j sum_k w_j w_k v_jk with v in [0, 1] (x x, x y of fp32
   values are exact in fp64) and weights of sum 1, so it lies in [0, 1].  Each 11-term pass adds at most TAPS u times
   the sum of |terms| <= TAPS u, and every term carries two taps: E_MOMENT = (2 TAPS + 2 (TAPS + 2)) u = (4 TAPS + 4) u.
 * The four factors.  A central moment s = E[..] - mu mu has error <= 3 E_MOMENT + 2u (one product of two moments, one
   subtraction, all values <= 1).  2 mu_x mu_y + C1 and mu_x^2 + mu_y^2 + C1: <= 4 E_MOMENT + 6u.  2 s_xy + C2 and
   s_xx + s_yy + C2: <= 6 E_MOMENT + 7u.  All four: E_FACTOR = 6 E_MOMENT + 8u.
 * The two ratios.  Exactly, 0 < 2 mu_x mu_y + C1 <= mu_x^2 + mu_y^2 + C1 and |2 s_xy| <= s_xx + s_yy (Cauchy-Schwarz;
   exact variances are >= 0), so both ratios are at most 1 in magnitude, and their exact denominators are >= C1 and
   >= C2.  |A'/B' - A/B| <= (|dA| + |A/B| |dB|) / (B - |dB|) <= 2 E_FACTOR / (C - E_FACTOR) =: R(C).
 * The product of the ratios: R(C1) + R(C2) + R(C1) R(C2), and three more roundings (two products and the division, in
   whichever association) of a value <= 1 + that: 4u.
   E = R(C1) + R(C2) + R(C1) R(C2) + 4u  (about 7.3e-10, dominated by 2 E_FACTOR / C1),   PER_ENTRY = 2 E.

The sum.  Against math.fsum of this file's entries: entries * PER_ENTRY for the differences of the terms, plus
(entries + 1024 + 8) u sum|ssim| for the order of summation — `entries` additions inside the threads, at most 1024
partials and 8 levels of butterfly and fold, each a rounding of a partial sum whose magnitude is at most sum|ssim|
(the argument of tests/test_gpu_diagnostics.py, with |.| because SSIM entries may be negative).
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U53 = 2.0 ** -53
TAPS, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2

TAP_REL = (TAPS + 2) * U53
E_MOMENT = (2 * TAPS) * U53 + 2 * TAP_REL
E_FACTOR = 6 * E_MOMENT + 8 * U53


def _ratio_error(c):
    return 2 * E_FACTOR / (c - E_FACTOR)


E_ENTRY = _ratio_error(C1) + _ratio_error(C2) + _ratio_error(C1) * _ratio_error(C2) + 4 * U53
PER_ENTRY = 2 * E_ENTRY


def sum_bound(entries: int, sum_abs: float) -> float:
    return entries * PER_ENTRY + (entries + 1024 + 8) * U53 * sum_abs


def sq_err_bound(n_terms: int, s: float) -> float:
    """lnrf_sq_err_f64 against math.fsum of the same non-negative float64 terms (tests/test_gpu_diagnostics.py)."""
    return (n_terms + 1024 + 8) * U53 * s


# ------------------------------------------------------------------------------------------------- unit images (fp32)

def unit_image(image_u8: np.ndarray) -> np.ndarray:
    """byte / 255 as an IEEE fp32 division."""
    return np.asarray(image_u8).astype(F32) / F32(255)


def unit_prediction(colors: np.ndarray) -> np.ndarray:
    """clamp((c + 1) * 0.5, 0, 1) in fp32."""
    return np.clip((np.asarray(colors, dtype=F32) + F32(1)) * F32(0.5), F32(0), F32(1))


# -------------------------------------------------------------------------------------------------------------- PSNR

def sq_err_terms(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return (np.asarray(a).astype(F64) - np.asarray(b).astype(F64)) ** 2


def mse(a: np.ndarray, b: np.ndarray) -> float:
    terms = sq_err_terms(a, b)
    return math.fsum(terms.reshape(-1).tolist()) / terms.size


def psnr_of_mse(value: float) -> float:
    return math.inf if value == 0 else -10.0 * math.log10(value)


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    return psnr_of_mse(mse(a, b))


# -------------------------------------------------------------------------------------------------------------- SSIM

def window(sigma: float = SIGMA, normalise: bool = True) -> np.ndarray:
    g = np.exp(-((np.arange(TAPS, dtype=F64) - TAPS // 2) ** 2) / (2.0 * sigma * sigma))
    return g / g.sum() if normalise else g


def filter_valid(image: np.ndarray, taps: np.ndarray, vertical_first: bool = False) -> np.ndarray:
    """[H, W, C] -> [H - 10, W - 10, C]: the separable window over the valid region, in the dtype of `image`."""
    n = len(taps)
    taps = taps.astype(image.dtype)

    def rows(x):
        return sum(taps[k] * x[:, k:k + x.shape[1] - n + 1] for k in range(n))

    def cols(x):
        return sum(taps[k] * x[k:k + x.shape[0] - n + 1] for k in range(n))

    return rows(cols(image)) if vertical_first else cols(rows(image))


def ssim_map(a: np.ndarray, b: np.ndarray, *, sigma: float = SIGMA, normalise: bool = True, c1: float = C1,
             c2: float = C2, pad_same: bool = False, sample_covariance: bool = False, clamp_moments: bool = False,
             moment_dtype=F64, vertical_first: bool = False) -> np.ndarray:
    """The SSIM map of two fp32 [H, W, 3] unit images, float64 [H - 10, W - 10, 3].  With the defaults this is the
    definition; every keyword switches to a wrong variant (pad_same: zero-padded 'same' region; sample_covariance: the
    n / (n - 1) factor of 121 samples; clamp_moments: central moments clamped at 0; moment_dtype: precision of the
    filter and the moments)."""
    x, y = np.asarray(a).astype(moment_dtype), np.asarray(b).astype(moment_dtype)
    if pad_same:
        half = TAPS // 2
        x, y = (np.pad(v, ((half, half), (half, half), (0, 0))) for v in (x, y))
    taps = window(sigma, normalise)

    def filt(v):
        return filter_valid(v, taps, vertical_first)

    mu_x, mu_y = filt(x), filt(y)
    s_xx, s_yy, s_xy = filt(x * x) - mu_x * mu_x, filt(y * y) - mu_y * mu_y, filt(x * y) - mu_x * mu_y
    if sample_covariance:
        factor = (TAPS * TAPS) / (TAPS * TAPS - 1.0)
        s_xx, s_yy, s_xy = s_xx * factor, s_yy * factor, s_xy * factor
    if clamp_moments:
        s_xx, s_yy, s_xy = (np.maximum(s, 0) for s in (s_xx, s_yy, s_xy))
    mu_x, mu_y, s_xx, s_yy, s_xy = (v.astype(F64) for v in (mu_x, mu_y, s_xx, s_yy, s_xy))
    return ((2 * mu_x * mu_y + c1) * (2 * s_xy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_xx + s_yy + c2))


def ssim_sum(values: np.ndarray) -> float:
    return math.fsum(np.asarray(values).reshape(-1).tolist())


def ssim(a: np.ndarray, b: np.ndarray) -> float:
    values = ssim_map(a, b)
    return ssim_sum(values) / values.size


def ssim_map_brute_force(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The same map with the 121-tap 2-D window applied directly, entry by entry."""
    x, y = np.asarray(a).astype(F64), np.asarray(b).astype(F64)
    g = window()
    w2 = np.outer(g, g)[:, :, None]
    height, width = x.shape[0] - TAPS + 1, x.shape[1] - TAPS + 1
    out = np.empty((height, width, 3), dtype=F64)
    for i in range(height):
        for j in range(width):
            px, py = x[i:i + TAPS, j:j + TAPS], y[i:i + TAPS, j:j + TAPS]
            mu_x, mu_y = (w2 * px).sum(axis=(0, 1)), (w2 * py).sum(axis=(0, 1))
            s_xx = (w2 * px * px).sum(axis=(0, 1)) - mu_x ** 2
            s_yy = (w2 * py * py).sum(axis=(0, 1)) - mu_y ** 2
            s_xy = (w2 * px * py).sum(axis=(0, 1)) - mu_x * mu_y
            out[i, j] = ((2 * mu_x * mu_y + C1) * (2 * s_xy + C2)) / ((mu_x ** 2 + mu_y ** 2 + C1) * (s_xx + s_yy + C2))
    return out


# ------------------------------------------------------------------------------------------------------------ inputs

def image_pair(kind: str, height: int, width: int, seed: int = 0):
    """Two fp32 [H, W, 3] unit images: 'noise' (uniform noise against noise), 'near' (an image against itself plus small
    noise), 'dark' (values <= 0.02, where the C1 denominator is smallest), 'checker' (a checkerboard against its
    negative: negative SSIM), 'same' (an image against itself)."""
    rng = np.random.default_rng(1000 * height + width + seed)
    shape = (height, width, 3)
    if kind == "noise":
        a, b = rng.random(shape), rng.random(shape)
    elif kind == "near":
        a = rng.random(shape)
        b = np.clip(a + rng.normal(scale=0.01, size=shape), 0, 1)
    elif kind == "dark":
        a, b = rng.random(shape) * 0.02, rng.random(shape) * 0.02
    elif kind == "checker":
        yy, xx = np.mgrid[0:height, 0:width]
        a = np.repeat((((yy // 3) + (xx // 3)) % 2).astype(F64)[:, :, None], 3, axis=2) * 0.8 + 0.1
        b = 1.0 - a
    elif kind == "same":
        a = rng.random(shape)
        b = a
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)

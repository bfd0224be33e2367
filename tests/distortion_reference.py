"""
The distortion loss (csrc/rays.hip distortion_kernel; mip-NeRF 360, Barron et al. 2022, eq. 15): cases, two float64
references, a float32 emulation of the kernel's order of operations and a derived error bound.  No GPU.

A plain module that tests import (not a conftest).  tests/test_distortion_cpu.py checks it on the CPU,
tests/test_gpu_distortion.py runs the kernel on the same cases.  Cases carry float32 inputs (rays_edge_cases.QuadCase) and
hand exactly those values to both sides, so any difference is arithmetic and not input.

Definition, for ray n with mask[n] != 0 and T >= 1 ascending samples (restated here in float64):
  start_0 = t_min, end_{T-1} = t_max, midpoints of neighbouring samples otherwise;
  delta_i = end_i - start_i,  a_i = sigma_i delta_i,  A_i = sum_{j<=i} a_j;
  w_i = exp(-A_{i-1}) (1 - exp(-a_i))      (the background's share exp(-A_{T-1}) takes no part);
  r = t_max - t_min,  m_i = ((start_i + end_i) / 2 - t_min) / r,  d_i = delta_i / r;
  L_n = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i.
A ray with mask == 0, r <= 0 or a non-finite r has L_n = 0 and no gradient.  With the exclusive prefixes W_<i, M_<i of w
and w m (and the suffixes W_>i, M_>i):
  L_n = 2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 d_i
  G_i = dL_n/dw_i = 2 (m_i W_<i - M_<i + M_>i - m_i W_>i) + (2/3) w_i d_i
  dL_n/dsigma_k = delta_k (G_k exp(-A_k) - sum_{i>k} G_i w_i).

The bound (error_bound) — worst-case, first order in u = 2^-24, every figure per ray from the float64 reference:
  tau = max |t|;  C = ceil(T / 64) chunks;  e_x = 2^-22 relative error of expf ("a couple of ulp", as
  tests/test_gpu_per_sample_kernels.py takes it).
  edges      an inner edge fl((t_i + t_j) / 2) is off by <= u tau (the sum is <= 2 tau, halving is exact); t_min and t_max
             are exact.  delta_i = fl(end - start): eps_d(i) = 2 u tau + u delta_i.
  a, A       a_i = fl(sigma_i delta_i): da_i = sigma_i eps_d(i) + u a_i.  A wave scan adds along a path of 6 levels and
             one carry per chunk, all terms >= 0: dA_i = sum_{j<=i} da_j + 7 C u A_i.
  exp        S_i = exp(-A_i): dS_i = [exp(-max(A_i - dA_i, 0)) - exp(-A_i)] + e_x S_i, evaluated as it stands (a density of
             1e30 makes dA_i huge and the bracket exactly 0, which is what happens).  x_i = 1 - exp(-a_i):
             dx_i = [exp(-max(a_i - da_i, 0)) - exp(-a_i)] + e_x exp(-a_i) + u x_i.
  w          w_i = S_{i-1} x_i: dw_i = dS_{i-1} x_i + S_{i-1} dx_i + u w_i  (S_{-1} = 1 exactly).
  m, d       r = fl(t_max - t_min) is off by u r; the bin centre by 2 u tau (two edge errors halved, one rounding of a
             sum <= 2 tau halved); minus t_min: + u r; divided by r: 2 more roundings of a value <= 1:
             eps_m = 2 u tau / r + 3 u.   eps_dn(i) = eps_d(i) / r + 2 u d_i.
  scans      with sum w <= 1 and m <= 1, every prefix and the total of w is off by <= DW = sum_j dw_j + 7 C u, of w m by
             <= DM = sum_j dw_j + eps_m + u + 7 C u.
  p, q       p_i = m_i W_<i - M_<i and q_i = (M_T - M_<=i) - m_i (W_T - W_<=i) lie in [0, 1] (p_i + q_i = sum_j w_j
             |m_i - m_j|): dp = eps_m + DW + DM + 3 u,  dq = eps_m + 2 DW + 2 DM + 4 u.  These are where `total - prefix`
             cancels; the bound counts them as absolute errors of quantities <= 1.
  loss       term_i = 2 w_i p_i + (1/3) w_i^2 d_i (6 roundings):
             dL = sum_i [2 dw_i + (2/3) w_i dw_i + (1/3) w_i^2 eps_dn(i)] + 2 dp + (6 + C + 6) u L
             (sum_i 2 w_i dp <= 2 dp; the per-lane accumulation adds C times and the wave sum 6).
  G          |G_i| <= 2 + 2/3 < 3: dG_i = 2 (dp + dq) + (2/3) (dw_i + w_i eps_dn(i)) + 24 u.
  Gamma, P   products G_i w_i: w_i dG_i + 3 dw_i + 3 u w_i; sum |G w| <= 3:
             DP = sum_i (w_i dG_i + 3 dw_i) + 3 u + 21 C u for every prefix and for Gamma.
  gradient   h_k = G_k S_k - (Gamma - P_k), |h_k| <= 6: dh_k = dG_k S_k + 3 dS_k + 2 DP + 12 u;
             g_k = delta_k h_k: dg_k = eps_d(k) |h_k| + delta_k dh_k + 2 u |g_k|  (the 2nd u: times grad_scale).
This is a worst-case bound: it assumes that every edge error of a ray pushes the optical depth the same way
(sum_j sigma_j 2 u tau), where rounding errors in fact scatter.  On the cases below the emulation uses at most 0.5 %
of it (loss) and 10 % (gradient, clustered case); tests/test_distortion_cpu.py prints the figures per case, and its
mutation test shows that the bound still separates a wrong kernel from a right one.
"""
import math
from typing import Callable, List, Optional, Tuple

import numpy as np
import torch

import rays_edge_cases as RC

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
EXPF_REL = 2.0 ** -22

N_RAYS = 37                       # 10 workgroups of 4 rays, the last one with a single ray
MISS_ROWS = (0, 17, 36)           # the first ray, an inner one and the only ray of the last workgroup
SEAM_TS = (1, 2, 63, 64, 65, 128, 129, 192)
CLUSTER_T, CLUSTER_LO, CLUSTER_HI = 192, 32, 160   # samples [32, 160) sit inside 1 % of the range
ZERO_RANGE_ROWS = (2, 9)


# ---------------------------------------------------------------------------------------------------------------------
# cases

def seam_case(t: int) -> RC.QuadCase:
    return RC.quad_case(N_RAYS, t, 0, seed=100 + t, miss=MISS_ROWS)


def clustered_case() -> RC.QuadCase:
    """128 of 192 samples inside 1 % of the range (at 45 % of it), with ten times the density there so that the cluster
    holds a visible share of the weight; 32 samples in front and 32 behind."""
    case = RC.quad_case(N_RAYS, CLUSTER_T, 0, seed=301, miss=MISS_ROWS)
    gen = torch.Generator().manual_seed(302)
    r = (case.t_max - case.t_min)[:, None]
    lo = case.t_min[:, None]
    n_in = CLUSTER_HI - CLUSTER_LO
    front = torch.sort(torch.rand(N_RAYS, CLUSTER_LO, generator=gen), 1).values * 0.44
    inside = 0.45 + torch.sort(torch.rand(N_RAYS, n_in, generator=gen), 1).values * 0.01
    back = 0.47 + torch.sort(torch.rand(N_RAYS, CLUSTER_T - CLUSTER_HI, generator=gen), 1).values * 0.52
    case.ts = (lo + r * torch.cat([front, inside, back], 1)).to(F32).contiguous()
    case.ts = torch.sort(case.ts, 1).values.contiguous()  # float32 rounding keeps the order; make that certain
    case.dens[:, CLUSTER_LO:CLUSTER_HI] *= 10.0
    return case


def repeated_case() -> RC.QuadCase:
    """T = 65 with runs of equal samples (delta = 0 for the inner ones), one run across the 64-lane seam."""
    case = RC.quad_case(N_RAYS, 65, 0, seed=303, miss=MISS_ROWS)
    case.ts[:, 10:13] = case.ts[:, 10:11]
    case.ts[:, 62:65] = case.ts[:, 62:63]
    case.ts[:, 0:2] = case.ts[:, 0:1]
    return case


def zero_range_case() -> RC.QuadCase:
    """T = 5; the rays of ZERO_RANGE_ROWS hit (mask 1) with t_max == t_min, every sample at that point."""
    case = RC.quad_case(N_RAYS, 5, 0, seed=304, miss=MISS_ROWS)
    for row in ZERO_RANGE_ROWS:
        case.t_max[row] = case.t_min[row]
        case.ts[row] = case.t_min[row]
    return case


def all_cases() -> List[Tuple[str, Callable[[], RC.QuadCase]]]:
    out = [(f"T{t}", lambda t=t: seam_case(t)) for t in SEAM_TS]
    out += [(name, fn) for name, fn in sorted(RC.FAMILIES.items())]
    out += [("clustered", clustered_case), ("repeated", repeated_case), ("zero_range", zero_range_case)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64 references

class Stages:
    """Every stage of the definition in float64 for a case (rows of rays without a loss hold harmless values)."""

    def __init__(self, case: RC.QuadCase, dens: Optional[torch.Tensor] = None):
        ts, lo, hi = case.ts.double(), case.t_min.double()[:, None], case.t_max.double()[:, None]
        n, t = ts.shape
        self.r = (hi - lo)[:, 0]
        self.valid = case.mask.bool() & torch.isfinite(self.r) & (self.r > 0)
        mid = (ts[:, 1:] + ts[:, :-1]) / 2
        self.starts = torch.cat([lo, mid], 1)
        self.ends = torch.cat([mid, hi], 1)
        self.delta = self.ends - self.starts
        self.sigma = case.dens.double() if dens is None else dens
        self.a = self.sigma * self.delta
        self.A = torch.cumsum(self.a, 1)
        self.A_prev = torch.cat([torch.zeros(n, 1, dtype=F64), self.A[:, :-1]], 1)
        self.x = -torch.expm1(-self.a)
        self.w = torch.exp(-self.A_prev) * self.x
        rr = torch.where(self.valid, self.r, torch.ones_like(self.r))[:, None]
        self.m = ((self.starts + self.ends) / 2 - lo) / rr
        self.d = self.delta / rr


def per_ray_loss(samples, sigma: torch.Tensor) -> torch.Tensor:
    """The O(T^2) definition in float64, differentiable in `sigma` [N,T]; `samples` has ts, t_min, t_max and mask (a
    QuadCase or an oracle.render.RaySamples)."""
    s = Stages(samples, sigma.double())
    pair = (s.w[:, :, None] * s.w[:, None, :] * (s.m[:, :, None] - s.m[:, None, :]).abs()).sum((1, 2))
    loss = pair + (s.w ** 2 * s.d).sum(1) / 3
    return torch.where(s.valid, loss, torch.zeros_like(loss))


def brute_force(case: RC.QuadCase):
    """The O(T^2) definition under autograd -> (loss[N], dloss/dsigma[N,T]), float64."""
    sigma = case.dens.double().clone().requires_grad_(True)
    loss = per_ray_loss(case, sigma)
    (grad,) = torch.autograd.grad(loss.sum(), sigma)
    return loss.detach(), grad


def _excl(x):
    return torch.cumsum(x, 1) - x


def stage_formulas(case: RC.QuadCase):
    """The O(T) prefix-sum form and its hand-derived gradient -> (loss[N], dloss/dsigma[N,T]), float64."""
    s = Stages(case)
    wm = s.w * s.m
    w_lt, m_lt = _excl(s.w), _excl(wm)
    w_gt = torch.flip(_excl(torch.flip(s.w, [1])), [1])
    m_gt = torch.flip(_excl(torch.flip(wm, [1])), [1])
    loss = (2 * s.w * (s.m * w_lt - m_lt) + s.w ** 2 * s.d / 3).sum(1)
    g = 2 * (s.m * w_lt - m_lt + m_gt - s.m * w_gt) + (2.0 / 3.0) * s.w * s.d
    gw = g * s.w
    gw_gt = torch.flip(_excl(torch.flip(gw, [1])), [1])
    grad = s.delta * (g * torch.exp(-s.A) - gw_gt)
    keep = s.valid[:, None]
    return torch.where(s.valid, loss, torch.zeros_like(loss)), torch.where(keep, grad, torch.zeros_like(grad))


# ---------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernel

MUTATIONS = ("no_third", "no_factor_2", "ts_for_midpoints", "no_range_division", "with_background",
             "exp_prev_in_gradient", "suffix_sign", "lost_carry")

_LANES = np.arange(64)


def _scan(v):
    """wave_incl_scan: Hillis-Steele over 64 lanes, float32."""
    v = v.copy()
    for off in (1, 2, 4, 8, 16, 32):
        v[:, off:] = v[:, off:] + v[:, :-off]
    return v


def _wave_sum(v):
    """wave_sum: xor butterfly 32, 16, ..., 1; every lane ends with the same float32 value."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, _LANES ^ off]
    return v[:, 0]


def emulate(case: RC.QuadCase, mutate: Optional[str] = None):
    """distortion_kernel's order of operations in NumPy float32 (separate products and sums: the compiler may fuse some
    into fmas, which the bound covers) -> (loss[N] float32, gradient[N,T] float32 for grad_scale 1 into zeros)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    f = np.float32
    ts, dens = case.ts.numpy().astype(f), case.dens.numpy().astype(f)
    tmin, tmax = case.t_min.numpy().astype(f)[:, None], case.t_max.numpy().astype(f)[:, None]
    n, t = ts.shape
    two, half, third, two_thirds = f(2), f(0.5), f(1) / f(3), f(2) / f(3)
    with np.errstate(all="ignore"):
        r = tmax - tmin
        valid_ray = (case.mask.numpy() != 0) & (r[:, 0] > 0) & (r[:, 0] <= np.finfo(f).max)
        rdiv = np.ones_like(r) if mutate == "no_range_division" else r

        def sweep(fn):
            carry = dict(a=np.zeros(n, f), w=np.zeros(n, f), m=np.zeros(n, f))
            for base in range(0, t, 64):
                i = base + _LANES
                ok = (i < t)[None, :]
                ic = np.minimum(i, t - 1)
                t_i = ts[:, ic]
                t_p = np.where(ic > 0, ts[:, np.maximum(ic - 1, 0)], f(0))
                t_n = np.where(ic < t - 1, ts[:, np.minimum(ic + 1, t - 1)], f(0))
                start = np.where(ic == 0, tmin, (t_i + t_p) / two)
                end = np.where(ic == t - 1, tmax, (t_n + t_i) / two)
                delta = end - start
                a = np.where(ok, dens[:, ic] * delta, f(0))
                incl = _scan(a) + carry["a"][:, None]
                prev = np.concatenate([carry["a"][:, None], incl[:, :-1]], 1)
                w = np.where(ok, np.exp(-prev) * (f(1) - np.exp(-a)), f(0))
                centre = t_i if mutate == "ts_for_midpoints" else (start + end) / two
                m = (centre - tmin) / rdiv
                d = delta / rdiv
                w_in = _scan(w) + carry["w"][:, None]
                m_in = _scan(w * m) + carry["m"][:, None]
                w_ex = np.concatenate([carry["w"][:, None], w_in[:, :-1]], 1)
                m_ex = np.concatenate([carry["m"][:, None], m_in[:, :-1]], 1)
                carry = dict(a=incl[:, 63], w=w_in[:, 63], m=m_in[:, 63])
                if mutate == "lost_carry" and base + 64 < t:  # the next chunk's scan of w starts from 0 again
                    carry["w"] = np.zeros(n, f)
                fn(base, ok, dict(w=w, m=m, d=d, delta=delta, incl=incl, prev=prev, w_ex=w_ex, m_ex=m_ex, w_in=w_in,
                                  m_in=m_in))
            return carry

        k2 = f(1) if mutate == "no_factor_2" else two
        k3 = f(0) if mutate == "no_third" else third
        k23 = f(0) if mutate == "no_third" else two_thirds

        l_part = np.zeros((n, 64), f)

        def first(base, ok, s):
            nonlocal l_part
            l_part = l_part + (k2 * s["w"] * (s["m"] * s["w_ex"] - s["m_ex"]) + k3 * s["w"] * s["w"] * s["d"])

        tot = sweep(first)
        w_tot, m_tot = tot["w"][:, None], tot["m"][:, None]
        loss = _wave_sum(l_part)
        if mutate == "with_background":  # the share exp(-A_{T-1}) as one more weight at m = 1 of width 0
            loss = loss + two * np.exp(-tot["a"]) * (tot["w"] - tot["m"])

        def big_g(s):
            return (k2 * (s["m"] * s["w_ex"] - s["m_ex"] + (m_tot - s["m_in"]) - s["m"] * (w_tot - s["w_in"]))
                    + k23 * s["w"] * s["d"])

        gw_part = np.zeros((n, 64), f)

        def second(base, ok, s):
            nonlocal gw_part
            gw_part = gw_part + big_g(s) * s["w"]

        sweep(second)
        gamma = _wave_sum(gw_part)[:, None]

        grad = np.zeros((n, t), f)
        gw_carry = np.zeros(n, f)

        def third_sweep(base, ok, s):
            nonlocal gw_carry
            gk = big_g(s)
            gw_incl = _scan(gk * s["w"]) + gw_carry[:, None]
            s_next = np.exp(-(s["prev"] if mutate == "exp_prev_in_gradient" else s["incl"]))
            rest = gamma - gw_incl
            v = s["delta"] * (gk * s_next + rest if mutate == "suffix_sign" else gk * s_next - rest)
            cols = min(64, t - base)
            grad[:, base:base + cols] = v[:, :cols]
            gw_carry = gw_incl[:, 63]

        sweep(third_sweep)
    loss = np.where(valid_ray, loss, f(0)).astype(f)
    grad = np.where(valid_ray[:, None], grad, f(0)).astype(f)
    return loss, grad


# ---------------------------------------------------------------------------------------------------------------------
# the bound (derivation: module docstring)

def error_bound(case: RC.QuadCase, grad_scale: float = 1.0):
    """(loss bound[N], gradient bound[N,T]) float64: absolute, 0 for rays without a loss (those are exact)."""
    s = Stages(case)
    loss_ref, grad_ref = stage_formulas(case)
    n, t = case.ts.shape
    chunks = math.ceil(t / 64)
    u, ex = U, EXPF_REL
    tau = torch.maximum(case.ts.double().abs().max(1).values,
                        torch.maximum(case.t_min.double().abs(), case.t_max.double().abs()))[:, None]
    r = torch.where(s.valid, s.r, torch.ones_like(s.r))[:, None]
    eps_d = 2 * u * tau + u * s.delta
    da = s.sigma * eps_d + u * s.a
    d_big_a = torch.cumsum(da, 1) + 7 * chunks * u * s.A
    surv = torch.exp(-s.A)
    d_surv = (torch.exp(-torch.clamp(s.A - d_big_a, min=0)) - surv) + ex * surv
    ea = torch.exp(-s.a)
    dx = (torch.exp(-torch.clamp(s.a - da, min=0)) - ea) + ex * ea + u * s.x
    surv_prev = torch.exp(-s.A_prev)
    d_surv_prev = torch.cat([torch.zeros(n, 1, dtype=F64), d_surv[:, :-1]], 1)
    dw = d_surv_prev * s.x + surv_prev * dx + u * s.w
    eps_m = 2 * u * tau / r + 3 * u
    eps_dn = eps_d / r + 2 * u * s.d
    sum_dw = dw.sum(1, keepdim=True)
    big_dw = sum_dw + 7 * chunks * u
    big_dm = sum_dw + eps_m + u + 7 * chunks * u
    dp = eps_m + big_dw + big_dm + 3 * u
    dq = eps_m + 2 * big_dw + 2 * big_dm + 4 * u
    d_loss = ((2 * dw + (2.0 / 3.0) * s.w * dw + s.w ** 2 * eps_dn / 3).sum(1) + 2 * dp[:, 0]
              + (12 + chunks) * u * loss_ref.abs())
    dg = 2 * (dp + dq) + (2.0 / 3.0) * (dw + s.w * eps_dn) + 24 * u
    big_dp = (s.w * dg + 3 * dw).sum(1, keepdim=True) + 3 * u + 21 * chunks * u
    dh = dg * surv + 3 * d_surv + 2 * big_dp + 12 * u
    h_abs = torch.where(s.delta > 0, grad_ref.abs() / torch.where(s.delta > 0, s.delta, torch.ones_like(s.delta)),
                        torch.full_like(s.delta, 6.0))
    d_grad = eps_d * torch.clamp(h_abs, max=6.0) + s.delta * dh + 2 * u * grad_ref.abs()
    zero = torch.zeros((), dtype=F64)
    return (torch.where(s.valid, d_loss, zero), torch.where(s.valid[:, None], d_grad, zero) * abs(grad_scale))

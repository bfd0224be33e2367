"""
Edge cases of the per-ray kernels (csrc/rays.hip, csrc/ray_geom.h): case tables and float64 references, no GPU.

A plain module that tests import (not a conftest).  tests/test_rays_edge_cases_cpu.py checks on the CPU that every case
is well posed (the float32 and float64 oracles agree on it, the references are finite, the sizes are the ones the
comments claim); tests/test_gpu_rays_edges.py runs the kernels on them.  Everything is built from oracle.render
(ray_t_range, stratified_ts, RaySamples, interp_rows) and oracle.philox.

The quadrature cases carry float32 inputs and hand exactly those values to both sides: the kernel reads them as they
are, the reference reads them widened to float64, so any difference is the kernel's arithmetic and not its inputs.
"""
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from oracle import render as OR

F32 = torch.float32
F64 = torch.float64
BBOX_MIN = (-1.0, -1.0, -1.0)
BBOX_MAX = (1.0, 1.0, 1.0)
MIN_T_RANGE = 1e-3
EPSILON = 1e-8

_S2 = 1.0 / math.sqrt(2.0)
_S3 = 1.0 / math.sqrt(3.0)

# (origin, direction, note) against the box [-1,1]^3.  den = d + epsilon (render.py:371); in float32 a zero component
# gives den = 1e-8 and d = -1e-8 gives den = 0 exactly.
DEGENERATE_RAYS = [
    ((-3.0, 0.2, 0.1), (1.0, 0.0, 0.0), "axis-parallel hit, t = [2, 4]"),
    ((-3.0, 1.5, 0.1), (1.0, 0.0, 0.0), "axis-parallel, outside the y slab: miss"),
    ((-3.0, 1.0, 0.0), (1.0, 0.0, 0.0), "along the face plane y = 1: miss"),
    ((0.1, 0.2, -0.3), (0.6, 0.0, 0.8), "origin inside, one zero component: t_min = 0"),
    ((0.0, 0.0, 3.0), (0.0, 0.0, 1.0), "pointing away: miss"),
    ((-3.0, 0.2, 0.1), (1.0, -1e-8, 0.0), "den == 0, origin strictly inside that slab: -inf / +inf, hit"),
    ((-3.0, 1.0, 0.1), (1.0, -1e-8, 0.0), "den == 0 and origin on the plane: 0/0, miss"),
    ((-2.0, 0.0, 0.0), (_S2, _S2, 0.0), "touches the edge at (-1, 1): miss"),
    ((-1.9995, 0.0, 0.0), (_S2, _S2, 0.0), "chord shorter than min_t_range: t_max = t_min + min_t_range"),
    ((1.0, 1.0, 1.0), (-_S3, -_S3, -_S3), "origin on a corner, entering: hit from t = 0 (the oracle's t_min is -0.0)"),
    ((1.0, 1.0, 1.0), (_S3, _S3, _S3), "origin on a corner, leaving: miss"),
    ((0.1, 0.2, -0.3), (0.0, 0.0, 1.0), "origin inside, two zero components: t_min = 0"),
    ((0.1, 0.2, -0.3), (0.0, -1.0, 0.0), "origin inside, along -y: t_min = 0"),
    ((3.0, -0.2, 0.4), (-1.0, 0.0, 0.0), "axis-parallel hit along -x, t = [2, 4]"),
    ((1.0, 0.3, 0.2), (-1.0, 0.0, 0.0), "origin on a face, entering: hit from t = 0"),
    ((1.0, 0.3, 0.2), (1.0, 0.0, 0.0), "origin on a face, leaving: miss"),
    ((0.0, 0.0, -5.0), (0.0, 0.0, 1.0), "two zero components from outside: hit, t = [4, 6]"),
]


def degenerate_rays(rows: Optional[int] = None) -> torch.Tensor:
    """The table as float32 rays [N,2,3]; `rows` tiles it (cyclically) to that many rays."""
    rays = torch.tensor([[o, d] for o, d, _ in DEGENERATE_RAYS], dtype=F64).to(F32)
    if rows is not None:
        idx = torch.arange(rows) % rays.shape[0]
        rays = rays[idx]
    return rays.contiguous()


def bbox(dtype) -> torch.Tensor:
    return torch.tensor([BBOX_MIN, BBOX_MAX], dtype=dtype)


def oracle_t_range(rays: torch.Tensor, dtype):
    """(t_min, t_max, mask) of the oracle evaluated in `dtype` on the float32 rays."""
    return OR.ray_t_range(bbox(dtype), rays.to(dtype), min_t_range=MIN_T_RANGE, epsilon=EPSILON)


def oracle_samples(rays: torch.Tensor, count: int, u: torch.Tensor) -> OR.RaySamples:
    """float64 slab test + stratified samples of float32 rays and uniforms."""
    t_min, t_max, mask = oracle_t_range(rays, F64)
    return OR.RaySamples(t_min, t_max, mask, OR.stratified_ts(t_min, t_max, count, u.double()))


def nan_intermediate_rows(rays: torch.Tensor) -> torch.Tensor:
    """Rows whose float32 slab quotients offsets / (d + eps) contain a NaN (0/0)."""
    r = rays.to(F32)
    q = (bbox(F32)[None] - r[:, 0][:, None]) / (r[:, 1][:, None] + torch.tensor(EPSILON, dtype=F32))
    return torch.isnan(q).flatten(1).any(1)


# ---------------------------------------------------------------------------------------------------------------------
# fine sampling

def fine_sample_lds_bytes(tc: int, tf: int) -> int:
    """Dynamic LDS of one lnrf_fine_sample workgroup: 4 waves, each xs[tc+1], ys[tc+1], comb[tc+tf] floats."""
    return 16 * (3 * tc + tf + 2)


FINE_LDS_TC = 64
FINE_LDS_TFS = (3902, 3903, 10046)   # 65 536 B, 65 552 B, 163 840 B (the largest the host accepts)
FINE_LDS_TF_TOO_LARGE = 10047        # 163 856 B


def fine_cdf_check(new_only: torch.Tensor, s: OR.RaySamples, dens: torch.Tensor, uf: torch.Tensor,
                   eps: float = 1e-8) -> None:
    """Acceptance of the new fine samples `new_only` [N,tf] (combine=False) drawn from the float64 coarse samples `s`
    with coarse densities `dens` and uniforms `uf`.

    Inverse-CDF sampling is ill-conditioned in t wherever the coarse CDF is flat (the float32 and float64 oracles
    themselves differ by >1e-3 of the span there), so parity is checked in CDF space: F(t_new) must reproduce the
    stratified u' to 2e-6, F = float64 oracle CDF.  fp32 rounding of t (~1e-6) is amplified in CDF space where the CDF
    is steep, and fp32 rounding of the CDF (~1e-7) is amplified in t where it is flat: every sample must be accurate in
    at least one of the two spaces, and in both to a looser bound."""
    n, tf = new_only.shape
    new_only = new_only.cpu().double()
    w = s.termination_probs(dens.cpu().double())[:, :-1] + eps
    xs = torch.cat([torch.zeros(n, 1, dtype=F64), torch.cumsum(w, 1)], 1)
    xs = xs / xs[:, -1:]
    ys = torch.cat([s.t_min[:, None], s.ends()], 1)
    up = (torch.arange(tf, dtype=F64)[None] + uf.cpu().double()) / tf
    f_at = OR.interp_rows(new_only, ys, xs)
    ref_new = s.fine_sampling(tf, uf.cpu().double(), dens.cpu().double(), combine=False, eps=eps).ts
    err_f = (f_at - up).abs()
    err_t = (new_only - ref_new).abs()
    ok = (err_f <= 1e-5) | (err_t <= 2e-5)
    assert ok.all(), (err_f[~ok].max().item(), err_t[~ok].max().item())
    assert err_f.max().item() <= 1e-3
    assert (new_only >= s.t_min[:, None] - 1e-6).all() and (new_only <= s.t_max[:, None] + 1e-6).all()
    span = (s.t_max - s.t_min)[:, None]
    frac_close = (err_t <= 1e-4 * span + 1e-6).double().mean().item()
    assert frac_close > 0.99


@dataclass
class FineCase:
    """Coarse samples (float32, on the CPU) for lnrf_fine_sample and the uniforms of the fine draw."""
    ts: torch.Tensor      # [N,tc]
    t_min: torch.Tensor   # [N]
    t_max: torch.Tensor   # [N]
    dens: torch.Tensor    # [N,tc]
    uf: torch.Tensor      # [N,tf]

    def samples64(self) -> OR.RaySamples:
        n = self.ts.shape[0]
        return OR.RaySamples(self.t_min.double(), self.t_max.double(), torch.ones(n, dtype=torch.bool),
                             self.ts.double())


def _ranges(n: int, gen) -> tuple:
    t_min = (2.0 + torch.rand(n, generator=gen)).to(F32)
    t_max = (t_min + 1.0 + torch.rand(n, generator=gen)).to(F32)
    return t_min, t_max


def _stratified32(t_min, t_max, count: int, gen) -> torch.Tensor:
    u = torch.rand(t_min.shape[0], count, generator=gen).to(F32)
    return OR.stratified_ts(t_min, t_max, count, u).contiguous()


def fine_case(n: int, tc: int, tf: int, seed: int = 0, uf: Optional[float] = None, shuffle: bool = False) -> FineCase:
    """Sorted (or, with `shuffle`, permuted) coarse samples with empty space in front (flat CDF segments) and a peaked
    density behind it, as test_fine_sample uses; `uf` fixes every fine uniform to one value."""
    gen = torch.Generator().manual_seed(1000 + seed)
    t_min, t_max = _ranges(n, gen)
    ts = _stratified32(t_min, t_max, tc, gen)
    dens = (torch.rand(n, tc, generator=gen) ** 4 * 30).to(F32)
    dens[:, : tc // 3] = 0.0
    if shuffle:
        perm = torch.stack([torch.randperm(tc, generator=gen) for _ in range(n)])
        ts = torch.gather(ts, 1, perm).contiguous()
    u = torch.rand(n, tf, generator=gen).to(F32) if uf is None else torch.full((n, tf), uf, dtype=F32)
    return FineCase(ts, t_min, t_max, dens, u)


U_MAX = 1.0 - 2.0 ** -24  # the largest uniform Philox returns: (2^24 - 1) * 2^-24


# ---------------------------------------------------------------------------------------------------------------------
# quadrature (termination_probs, composite forward and backward)

AUX_WEIGHTS = (0.3, 0.05, -0.2, 0.11)   # four distinct weights: a swapped index shows
BACKGROUND = (-0.5, 0.1, 0.7)


@dataclass
class QuadCase:
    """Inputs of the compositing kernels, float32 on the CPU.  The upstream gradient of `outputs` is either explicit
    (`g_out`) or that of mean((outputs - tgt)^2) as in test_composite_bwd_matches_autograd."""
    ts: torch.Tensor        # [N,T]
    t_min: torch.Tensor     # [N]
    t_max: torch.Tensor     # [N]
    mask: torch.Tensor      # [N] bool
    dens: torch.Tensor      # [N,T]
    rgb: torch.Tensor       # [N,T,3]
    aux: torch.Tensor       # [N,T,n_aux]
    bg: torch.Tensor        # [3]
    tgt: torch.Tensor       # [N,3]
    gw: Sequence[float]     # n_aux weights of the aux sums in the loss
    g_out: Optional[torch.Tensor] = None   # [N,3]

    @property
    def n(self) -> int:
        return self.ts.shape[0]

    @property
    def t(self) -> int:
        return self.ts.shape[1]

    @property
    def n_aux(self) -> int:
        return self.aux.shape[-1]

    @property
    def out_scale(self) -> float:
        return 2.0 / (3 * self.n)

    def samples(self, dtype=F64) -> OR.RaySamples:
        return OR.RaySamples(self.t_min.to(dtype), self.t_max.to(dtype), self.mask, self.ts.to(dtype))


@dataclass
class QuadRef:
    probs: torch.Tensor
    outputs: torch.Tensor
    alphas: torch.Tensor
    aux_sum: torch.Tensor
    g_density: torch.Tensor
    g_rgb: torch.Tensor
    g_background: torch.Tensor
    g_aux: torch.Tensor

    def tensors(self):
        return (self.probs, self.outputs, self.alphas, self.aux_sum, self.g_density, self.g_rgb, self.g_background,
                self.g_aux)


def quad_reference(case: QuadCase, dtype=F64) -> QuadRef:
    """Oracle forward and autograd gradients of the case, evaluated in `dtype` (float64: the reference; float32: the
    measure of what float32 arithmetic of the same formulas loses)."""
    s = case.samples(dtype)
    d = case.dens.to(dtype).requires_grad_(True)
    c = case.rgb.to(dtype).requires_grad_(True)
    a = case.aux.to(dtype).requires_grad_(True)
    b = case.bg.to(dtype).requires_grad_(True)
    probs = s.termination_probs(d)
    out = s.render_rays(d, c, b)
    alphas = s.render_alpha(d)[:, 0]
    aux_sum = torch.where(s.mask[:, None], (a * probs[:, :-1, None]).sum(1), torch.zeros(case.n, case.n_aux, dtype=dtype))
    if case.g_out is not None:
        loss = (out * case.g_out.to(dtype)).sum()
    else:
        loss = ((out - case.tgt.to(dtype)) ** 2).mean()
    if case.n_aux:
        loss = loss + (aux_sum * torch.tensor(list(case.gw), dtype=dtype)).sum()
    grads = torch.autograd.grad(loss, [d, c, b] + ([a] if case.n_aux else []))
    g_aux = grads[3] if case.n_aux else torch.zeros_like(a)
    return QuadRef(probs.detach(), out.detach(), alphas.detach(), aux_sum.detach(), grads[0], grads[1], grads[2], g_aux)


def quad_case(n: int, t: int, n_aux: int, seed: int = 0, miss: Sequence[int] = (), g_out: bool = False,
              dens_scale: float = 4.0) -> QuadCase:
    """Random sorted samples, densities in [0, dens_scale), colours in [-1, 1); rays listed in `miss` are masked out.
    With `g_out` the upstream gradient is explicit: mixed signs, magnitudes spread over about 1e-3 .. 1."""
    gen = torch.Generator().manual_seed(2000 + seed)
    t_min, t_max = _ranges(n, gen)
    ts = _stratified32(t_min, t_max, t, gen)
    mask = torch.ones(n, dtype=torch.bool)
    if len(miss):
        mask[torch.as_tensor(list(miss))] = False
    dens = (torch.rand(n, t, generator=gen) * dens_scale).to(F32)
    rgb = (torch.rand(n, t, 3, generator=gen) * 2 - 1).to(F32)
    aux = torch.rand(n, t, max(n_aux, 1), generator=gen).to(F32)[..., :n_aux].contiguous()
    tgt = (torch.rand(n, 3, generator=gen) * 2 - 1).to(F32)
    go = None
    if g_out:
        mag = 10.0 ** (-3.0 * torch.rand(n, 3, generator=gen))
        sign = torch.where(torch.rand(n, 3, generator=gen) < 0.5, -1.0, 1.0)
        go = (mag * sign).to(F32).contiguous()
    return QuadCase(ts, t_min, t_max, mask, dens, rgb, aux, torch.tensor(BACKGROUND, dtype=F32), tgt,
                    AUX_WEIGHTS[:n_aux], go)


OPAQUE_DENSITY = 1e30
FAMILY_N, FAMILY_T, FAMILY_AUX = 8, 70, 2
# the opaque sample of each ray of the opaque family: first, last, both sides of the 64-lane seam, mid-ray
OPAQUE_AT = (0, FAMILY_T - 1, 63, 64, 30, 35, 17, 66)


def opaque_case() -> QuadCase:
    """Moderate densities with one sample of density 1e30 per ray (exp(-density * delta) == 0 in float32)."""
    case = quad_case(FAMILY_N, FAMILY_T, FAMILY_AUX, seed=11, dens_scale=2.0)
    for r, k in enumerate(OPAQUE_AT):
        case.dens[r, k] = OPAQUE_DENSITY
    return case


def empty_case() -> QuadCase:
    """All densities 0: outputs are the background, alpha 0."""
    case = quad_case(FAMILY_N, FAMILY_T, FAMILY_AUX, seed=12)
    case.dens.zero_()
    return case


def late_case() -> QuadCase:
    """Zeros up to lane 63, density from sample 64 on: the second chunk's carry starts from exactly 0."""
    case = quad_case(FAMILY_N, FAMILY_T, FAMILY_AUX, seed=13)
    case.dens[:, :64] = 0.0
    case.dens[:, 64:] += 0.5
    return case


FAMILIES = {"opaque": opaque_case, "empty": empty_case, "late": late_case}

SEAM_FWD_TS = (2, 63, 65, 128, 129)
SEAM_BWD = ((3, 1, 0), (5, 65, 3), (6, 129, 4), (17, 2, 4))

MISS_N, MISS_T, MISS_AUX, MISS_ROWS = 9, 65, 2, (0, 4, 8)


def missed_case() -> QuadCase:
    return quad_case(MISS_N, MISS_T, MISS_AUX, seed=21, miss=MISS_ROWS, g_out=True)


def all_missed_case() -> QuadCase:
    return quad_case(5, MISS_T, MISS_AUX, seed=22, miss=range(5), g_out=True)


FOLD_T = 3
FOLD_NS = (1029, 4 * 256 * 2 + 1)   # 258 and 513 workgroups of 4 rays: fold threads take a second / a third trip


FOLD_TRIP_RAYS = 4 * 256                 # rays whose partial rows one trip of the 256 fold threads covers
FOLD_MARK = (0.9, -0.8, 0.7)             # upstream gradient of the marked rays


def fold_case(n: int) -> QuadCase:
    """Many short rays, every seventh one missed, explicit per-ray gradients of mixed sign and magnitude.  The first
    rays of every later trip of the fold loop (up to five) are missed rays with the gradient FOLD_MARK, so each trip's
    rows carry a share of g_background far above the tolerance."""
    case = quad_case(n, FOLD_T, 0, seed=31, miss=range(3, n, 7), g_out=True)
    for start in range(FOLD_TRIP_RAYS, n, FOLD_TRIP_RAYS):
        case.mask[start:start + 5] = False
        case.g_out[start:start + 5] = torch.tensor(FOLD_MARK, dtype=F32)
    return case


def fold_trip_shares(case: QuadCase, ref: "QuadRef") -> torch.Tensor:
    """[trips, 3]: what the partial rows of each trip of the fold loop add to g_background (float64)."""
    go = case.g_out.double()
    per_ray = torch.where(case.mask[:, None], ref.probs[:, -1:] * go, go)
    return torch.stack([per_ray[s:s + FOLD_TRIP_RAYS].sum(0) for s in range(0, case.n, FOLD_TRIP_RAYS)])


def all_quad_cases():
    """(name, builder) of every quadrature case the GPU tests run."""
    out = [(name, fn) for name, fn in FAMILIES.items()]
    out += [(f"fwd_T{t}", lambda t=t: quad_case(5, t, 2, seed=t)) for t in SEAM_FWD_TS]
    out += [(f"bwd_{n}_{t}_{a}", lambda n=n, t=t, a=a: quad_case(n, t, a, seed=n + t)) for n, t, a in SEAM_BWD]
    out += [("missed", missed_case), ("all_missed", all_missed_case)]
    out += [(f"fold_{n}", lambda n=n: fold_case(n)) for n in FOLD_NS]
    return out

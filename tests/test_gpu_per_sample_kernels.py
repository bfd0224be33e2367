"""
Per-sample kernels against float64 autograd of the oracle, held to fp32 rounding: the Ref-NeRF head and colour map
(lnrf_refnerf_head_fwd/_bwd, lnrf_refnerf_color_fwd/_bwd), the derivative maps of the sinusoidal embedding
(lnrf_sinusoidal_emb_bwd/_jvp) and of the hash grid (lnrf_hashgrid_jvp / _input_grad / _bwd_dir) and the hash-grid
gather / scatters on table shapes the model tests never use (non-power-of-two and prime table sizes, ragged last
slices, the LDS-staged gather with a direction, points outside the box, smooth = False derivatives).

The inputs take every branch on purpose: clipped and linear-segment colours, saturated sigmoid / softplus, zero and
tiny normals, both signs of d.n, points on and outside the faces of the bounding box.

TOLERANCE.  Calibrated against the oracle, not the kernel: for every compared tensor the same oracle function is also
evaluated in float32 on the CPU on the same inputs (torch.autograd where a derivative is compared), and with

    err(a) = max_ij |a_ij - o64_ij| / (floor + |o64_ij|)

the kernel passes if err(kernel) <= 4 * err(o32) + 1e-6.  The kernels use equivalent but different formulas (FMA
contraction, forward-mode duals instead of reverse mode, expf / powf within a couple of ulp), each adding roundings
of the order the float32 oracle already has; a wrong coefficient or branch gives 1e-3 and above.  `floor` comes from
the float64 reference alone: 1e-2 of the typical row maximum of the tensor (median over its non-zero rows) for the
head, the colour map and the embedding, i.e. elements within two decades of the typical magnitude and all larger
ones are compared relatively, smaller ones absolutely; ~0 for the density (compared relatively over e^-20 .. e^20);
the tensor maximum for the hash-grid tensors (sums over 8 corners x 6 levels of entries of one scale).
The embedding maps have a derived bound instead (2^f x is exact in fp32; see the tests).

MEASURED on an MI355X (e32 = err(o32), kernel = err(kernel); the largest over the parametrised cases of a row;
"one upstream" is the largest over the six runs with a single non-zero upstream gradient):

    tensor                                                           e32    kernel
    color rgb                                                    3.7e-06   2.3e-06
    color g_dir_out                                              4.8e-06   8.9e-06
    color g_spectral                                             6.9e-06   7.8e-06
    color g_diffuse                                              4.4e-06   8.4e-06
    head_fwd density                                             5.9e-08   7.4e-08
    head_fwd diffuse                                             2.3e-07   2.3e-07
    head_fwd spectral                                            9.8e-08   1.1e-07
    head_fwd tail                                                5.4e-05   6.7e-05
    head_fwd aux                                                 4.2e-07   5.7e-07
    head_bwd all upstream: g_spatial[:, :9]                      4.0e-05   2.4e-05
    head_bwd all upstream: g_nraw                                1.1e-04   1.3e-04
    head_bwd one upstream: g_spatial[:, :9]                      4.7e-05   4.5e-05
    head_bwd one upstream: g_nraw                                1.1e-04   1.3e-04
    emb bwd freqs=1 (absolute; derived bound 1.53e-06)           2.1e-07   2.1e-07
    emb jvp (error / derived bound)                              1.8e-01   1.9e-01
    emb bwd freqs=4 (absolute; derived bound 2.68e-05)           2.0e-06   2.3e-06
    emb bwd freqs=10 (absolute; derived bound 2.12e-03)          3.2e-04   2.0e-04
    grid m=321 fwd                                               5.0e-06   5.0e-06
    grid m=321 jvp                                               5.2e-06   5.2e-06
    grid m=321 input_grad                                        4.0e-06   4.0e-06
    grid m=321 bwd bucketed                                      1.9e-06   1.9e-06
    grid m=321 bwd direct                                        1.9e-06   1.9e-06
    grid m=321 bwd_dir bucketed                                  3.5e-06   3.5e-06
    grid m=321 bwd_dir direct                                    3.5e-06   3.5e-06
    grid m=20000 fwd                                             6.5e-06   6.5e-06
    grid m=20000 jvp                                             4.7e-06   4.7e-06
    grid m=20000 input_grad                                      5.0e-06   4.9e-06
    grid m=20000 bwd bucketed                                    4.0e-07   3.3e-07
    grid m=20000 bwd direct                                      4.0e-07   3.2e-07
    grid m=20000 bwd_dir bucketed                                6.1e-06   6.1e-06
    grid m=20000 bwd_dir direct                                  6.1e-06   6.2e-06
The adjoint identities: embedding |<jvp(u), g> - <u, bwd(g)>| = 1.1e-6 / 2.3e-6 / 6.2e-4 for freqs 1 / 4 / 10 (of
|<jvp(u), g>| = 48 / 174 / 3.8e4); hash grid at most 6.2e-8 of the scale of the summed terms (bound 7.6e-6).
Bucketed against direct scatter: at most 2.5e-7 of the maximum (bound 1e-5).  smooth = False leaves out 0.9 % (m = 321)
and 3.2 % (m = 20000) of the rows.
"""
import pytest
import torch

from oracle import instant_ngp as ON
from oracle import model as OM
from oracle import ref_nerf as ORF

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
EPS = 2.0 ** -23


# ---------------------------------------------------------------- comparison helpers

def typical_floor(ref: torch.Tensor) -> float:
    """1e-2 of the median row maximum of |ref| over its non-zero rows (from the float64 reference alone)."""
    r = ref.detach().abs().reshape(ref.shape[0], -1).max(dim=1).values
    r = r[r > 0]
    return 1e-2 * r.median().item() + 1e-30 if r.numel() else 1e-30


def max_floor(ref: torch.Tensor) -> float:
    return ref.detach().abs().max().item() + 1e-30


def nerr(a: torch.Tensor, ref: torch.Tensor, floor: float) -> float:
    ref = ref.detach().double()
    return ((a.detach().cpu().double() - ref).abs() / (floor + ref.abs())).max().item()


class Checks:
    """Collects every comparison of a test, prints e32 and the kernel's error, asserts them together at the end."""

    def __init__(self, case: str):
        self.case, self.failed = case, []

    def close(self, name, got, o64, o32, floor=None, rows=None):
        if rows is not None:
            got, o64, o32 = got.cpu()[rows], o64[rows], o32[rows]
        floor = typical_floor(o64) if floor is None else floor
        e32, ek = nerr(o32, o64, floor), nerr(got, o64, floor)
        bound = 4.0 * e32 + 1e-6
        print(f"{self.case} {name}: e32 {e32:.2e} kernel {ek:.2e} bound {bound:.2e}")
        if not ek <= bound:
            self.failed.append(f"{name}: kernel {ek:.3e} > 4 * e32 ({e32:.3e}) + 1e-6")
        return e32, ek

    def true(self, name, cond, detail=""):
        if not cond:
            self.failed.append(f"{name} {detail}")

    def finish(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# ---------------------------------------------------------------- (a) colour map

C_VALUES = [-0.5, -1e-3, 0.0, 3e-6, 5e-4, 0.003, 0.00314, 0.2, 0.999, 1.0, 1.001, 2.0]
O_VALUES = [-30.0, -2.0, 0.0, 2.0, 30.0]
S_VALUES = [0.07, 0.5, 0.93]


def color_inputs():
    """Every (c, o) combination in every channel, three different ones mixed within a sample, for three spectral
    weights: the pre-clip value c = sigmoid(o) s + diffuse is chosen directly through diffuse."""
    combos = [(c, o) for c in C_VALUES for o in O_VALUES]
    n = len(combos)
    c = torch.empty(n * len(S_VALUES), 3, dtype=F64)
    o = torch.empty_like(c)
    s = torch.empty(n * len(S_VALUES), 1, dtype=F64)
    for si, sv in enumerate(S_VALUES):
        for j in range(n):
            for k in range(3):
                c[si * n + j, k], o[si * n + j, k] = combos[(j + 17 * k) % n]  # 17 is coprime to 60
            s[si * n + j, 0] = sv
    diffuse = c - torch.sigmoid(o) * s
    g = torch.randn(c.shape, generator=torch.Generator().manual_seed(5), dtype=F64)
    return o.float(), s.float(), diffuse.float(), g.float(), c


def color_oracle(dt, o, s, diffuse, g):
    o, s, diffuse = (t.to(dt).requires_grad_(True) for t in (o, s, diffuse))
    rgb = ORF.ref_nerf_color(o, s, diffuse)
    g_o, g_s, g_d = torch.autograd.grad((rgb * g.to(dt)).sum(), (o, s, diffuse))
    return rgb.detach(), g_o, g_s, g_d


def test_color_map_all_branches():
    """rgb and the three input gradients over clipped (< 0, > 1), linear-segment (<= 0.0031308, below and above the
    max(c, 1e-5) guard) and power-segment colours, for saturated and unsaturated sigmoids.  The derivative of
    srgb(leaky_clip(c)) is continuous at c = 0 and c = 1 (identity slope of the clip, srgb' taken at the clipped
    value), so those samples stay in the gradient comparison as well: no sample is left out."""
    from learn_nerf import ops

    o, s, diffuse, g, c = color_inputs()
    c32 = torch.sigmoid(o.double()) * s.double() + diffuse.double()  # the value the float64 oracle sees
    # rounding the inputs to fp32 moves c by less than 2e-7, and no c is closer than 2e-6 to a branch point (3e-6 to
    # 0, 0.00314 is 9.2e-6 above 0.0031308), except the exact 0 and 1: every sample is on a known side
    assert (c32 - c).abs().max().item() < 2e-7
    for thr in (0.0031308, 0.0, 1.0):
        assert not (((c - thr).abs() < 2e-6) & (c != thr)).any()
    assert (c < 0).any() and (c > 1).any() and ((c > 0) & (c < 1e-5)).any() and ((c > 1e-5) & (c <= 0.0031308)).any()
    r64, r32 = color_oracle(F64, o, s, diffuse, g), color_oracle(F32, o, s, diffuse, g)
    sd = s.reshape(-1).contiguous().cuda()
    rgb = ops.refnerf_color_fwd(o.cuda(), sd, diffuse.cuda())
    g_o, g_s, g_d = ops.refnerf_color_bwd(o.cuda(), sd, diffuse.cuda(), g.cuda())
    ck = Checks("color")
    ck.close("rgb", rgb, r64[0], r32[0])
    ck.close("g_dir_out", g_o, r64[1], r32[1])
    ck.close("g_spectral", g_s.reshape(-1, 1), r64[2], r32[2])
    ck.close("g_diffuse", g_d, r64[3], r32[3])
    ck.finish()


# ---------------------------------------------------------------- (b) head

HD = 256  # width of spatial_out in the models: the tail columns start here


def head_inputs(m=600, seed=21):
    """spatial[:, :9] (scale 2), n_raw, unit d; rows 400.. are edge rows.  |d.n| >= 1e-3 by rejection, so relu(d.n)
    is taken on a known side (rows with an exactly zero normal have d.n = 0 in every precision)."""
    gen = torch.Generator().manual_seed(seed)
    sp = (2.0 * torch.randn(m, 9, generator=gen)).float()
    nr = torch.randn(m, 3, generator=gen).float()
    sp[400:420, 0] = torch.tensor([-20.0, 20.0]).repeat(10)  # density e^-20 .. e^20
    for i in range(32):  # saturated diffuse / spectral sigmoids, every sign pattern twice
        sp[420 + i, 1:5] = torch.tensor([30.0 if (i >> b) & 1 else -30.0 for b in range(4)])
    sp[452:482, 5] = torch.tensor([-30.0, 0.0, 30.0]).repeat(10)  # softplus: ~0, ln 2, linear
    sp[482:512, 6:9] = 0.0  # _safe_normalize at a zero vector
    sp[512:542, 6:9] = (1e-6 * torch.randn(30, 3, generator=gen)).float()  # |v|^2 far below the 1e-10 guard
    nr[542:557] = 0.0
    nr[557:572] = (1e-7 * torch.randn(15, 3, generator=gen)).float()
    nr[572:587] = (1e-5 * torch.randn(15, 3, generator=gen)).float()
    nr[587:600] = (1e3 * torch.randn(13, 3, generator=gen)).float()
    n = ORF._safe_normalize(sp[:, 6:9].double())
    d = torch.empty(m, 3)
    todo = torch.ones(m, dtype=torch.bool)
    while todo.any():
        v = torch.randn(int(todo.sum()), 3, generator=gen, dtype=F64)
        d[todo] = (v / v.norm(dim=-1, keepdim=True)).float()
        dn = (d.double() * n).sum(-1)
        todo = (dn.abs() < 1e-3) & (n.abs().sum(-1) > 0)
    dn = (d.double() * n).sum(-1)
    assert (dn >= 1e-3).sum() >= 100 and (dn <= -1e-3).sum() >= 100
    return sp, nr.contiguous(), d.contiguous()


def head_ld(sh):
    return (HD + sh * sh + 1 + 3) // 4 * 4  # 276 for degree 4


def head_forward_oracle(dt, sp, nr, d, sh):
    sp, nr = sp.to(dt).requires_grad_(True), nr.to(dt).requires_grad_(True)
    return sp, nr, ORF.ref_nerf_head(sp, nr, d.to(dt), sh)


@pytest.mark.parametrize("sh", range(1, 9))
def test_head_forward(sh):
    """All five outputs for every harmonic degree, called as the models call it: spatial is a wide buffer, the tail
    is written into columns 256.. of that same buffer and nothing else of the buffer changes."""
    from learn_nerf import ops

    sp, nr, d = head_inputs()
    m, ne, ld = sp.shape[0], sh * sh, head_ld(sh)
    buf = torch.randn(m, ld, generator=torch.Generator().manual_seed(sh))
    buf[:, :9] = sp
    dbuf = buf.cuda()
    view = dbuf[:, :HD + ne + 1]
    density, diffuse, spectral, aux = ops.refnerf_head_fwd(view, nr.cuda(), d.cuda(), sh, view[:, HD:])
    after = dbuf.cpu()
    o64, o32 = head_forward_oracle(F64, sp, nr, d, sh)[2], head_forward_oracle(F32, sp, nr, d, sh)[2]
    ck = Checks(f"head_fwd[sh={sh}]")
    ck.true("spatial columns unchanged", bits_equal(after[:, :HD], buf[:, :HD]))
    ck.true("padding columns unchanged", bits_equal(after[:, HD + ne + 1:], buf[:, HD + ne + 1:]))
    ck.close("density", density.reshape(-1, 1), o64[0], o32[0], floor=1e-30)
    ck.close("diffuse", diffuse, o64[1], o32[1])
    ck.close("spectral", spectral.reshape(-1, 1), o64[2], o32[2])
    ck.close("tail", after[:, HD:HD + ne + 1], o64[3], o32[3])
    ck.close("aux", aux, o64[4], o32[4])
    ck.finish()


HEAD_UPSTREAMS = ["all", "density", "diffuse", "spectral", "tail", "normal_mse", "neg_normal"]


@pytest.mark.parametrize("sh", [1, 4, 8])
def test_head_backward(sh):
    """The VJP with all upstream gradients at once and with each one alone (the others zero), so that no term hides
    behind another.  g_tail is a column view of the buffer that is also g_spatial, which is prefilled with random
    numbers: columns 0..8 must be prefill + VJP, every other column bit-identical to the prefill."""
    from learn_nerf import ops

    sp, nr, d = head_inputs()
    m, ne, ld = sp.shape[0], sh * sh, head_ld(sh)
    gen = torch.Generator().manual_seed(100 + sh)
    buf = torch.randn(m, ld, generator=gen)
    buf[:, :9] = sp
    dbuf, dnr, dd = buf.cuda(), nr.cuda(), d.cuda()
    full = dict(density=torch.randn(m, generator=gen), diffuse=torch.randn(m, 3, generator=gen),
                spectral=torch.randn(m, generator=gen), tail=torch.randn(m, ne + 1, generator=gen),
                aux=torch.randn(m, 2, generator=gen))
    prefill = torch.randn(m, ld, generator=gen)
    graphs = {dt: head_forward_oracle(dt, sp, nr, d, sh) for dt in (F64, F32)}
    ck = Checks(f"head_bwd[sh={sh}]")
    for which in HEAD_UPSTREAMS:
        g = {k: (v.clone() if which in ("all", k) else torch.zeros_like(v)) for k, v in full.items()}
        if which == "normal_mse":
            g["aux"][:, 0] = full["aux"][:, 0]
        if which == "neg_normal":
            g["aux"][:, 1] = full["aux"][:, 1]
        gbuf = prefill.clone()
        gbuf[:, HD:HD + ne + 1] = g["tail"]
        dg = gbuf.cuda()
        gview = dg[:, :HD + ne + 1]
        g_nraw = ops.refnerf_head_bwd(dbuf[:, :HD + ne + 1], dnr, dd, sh, g["density"].cuda(), g["diffuse"].cuda(),
                                      g["spectral"].cuda(), gview[:, HD:], g["aux"].cuda(), gview)
        after = dg.cpu()
        ref = {}
        for dt, (spv, nrv, (den, dif, spc, tail, aux)) in graphs.items():
            s = ((den[:, 0] * g["density"].to(dt)).sum() + (dif * g["diffuse"].to(dt)).sum() +
                 (spc[:, 0] * g["spectral"].to(dt)).sum() + (tail * g["tail"].to(dt)).sum() +
                 (aux * g["aux"].to(dt)).sum())
            g_sp, g_nr = torch.autograd.grad(s, (spv, nrv), retain_graph=True)
            ref[dt] = (gbuf[:, :9].to(dt) + g_sp, g_nr)
        ck.true(f"{which}: columns >= 9 unchanged", bits_equal(after[:, 9:], gbuf[:, 9:]))
        # the floor of columns 0..8 is that of the VJP itself: the prefill is only carried along
        ck.close(f"{which}: g_spatial[:, :9]", after[:, :9], ref[F64][0], ref[F32][0],
                 floor=max(typical_floor(ref[F64][0] - gbuf[:, :9].double()), 1e-2))
        ck.close(f"{which}: g_nraw", g_nraw, ref[F64][1], ref[F32][1])
    ck.true("forward inputs unchanged", bits_equal(dbuf, buf))
    ck.finish()


# ---------------------------------------------------------------- (c) sinusoidal embedding derivative maps

def emb_inputs(freqs, m=300):
    gen = torch.Generator().manual_seed(40 + freqs)
    batch = (torch.rand(m, 9, generator=gen) * 8 - 4).float()  # x in [-4, 4], read with the batch's row stride
    batch[0, 3:6], batch[1, 3:6], batch[2, 3:6] = 0.0, 1.0, -1.0
    batch[3, 3:6] = torch.tensor([4.0, -4.0, 0.0])
    col_off, ld = 256, 256 + 6 * freqs + 4
    g_emb = torch.randn(m, ld, generator=gen).float()
    u = torch.randn(m, 3, generator=gen).float()
    u[5] = 0.0
    return batch, g_emb, u, col_off, ld


@pytest.mark.parametrize("freqs", [1, 4, 10])
def test_sinusoidal_emb_bwd_jvp(freqs):
    """2^f x is exact in fp32, so the only errors are those of sincosf (a couple of ulp of 1), two products and the
    sum:  |err bwd| <= 4 * 2^-23 * sum_f 2^f * max|g|,  |err jvp| <= 4 * 2^-23 * 2^f * |u| per element; the adjoint
    identity <jvp(u), g> = <u, bwd(g)> then holds to the sum of the two bounds."""
    from learn_nerf import ops

    batch, g_emb, u, col_off, ld = emb_inputs(freqs)
    m, w = batch.shape[0], 6 * freqs
    dbatch = batch.cuda()
    x = dbatch[:, 3:6]
    assert x.stride(0) == 9
    g_x = ops.sinusoidal_emb_bwd(x, freqs, g_emb.cuda(), col_off=col_off).cpu().double()
    prefill = torch.randn(m, ld, generator=torch.Generator().manual_seed(9)).float()
    out = prefill.cuda()
    ops.sinusoidal_emb_jvp_into(x, freqs, u.cuda(), out, col_off=col_off)
    out = out.cpu()
    v = out[:, col_off:col_off + w].double()
    g = g_emb[:, col_off:col_off + w]

    ref = {}
    for dt in (F64, F32):
        xx = batch[:, 3:6].to(dt).requires_grad_(True)
        emb = OM.sinusoidal_emb(xx, freqs)
        (gx,) = torch.autograd.grad((emb * g.to(dt)).sum(), xx)
        _, jv = torch.autograd.functional.jvp(lambda t: OM.sinusoidal_emb(t, freqs), batch[:, 3:6].to(dt), u.to(dt))
        ref[dt] = (gx.double(), jv.double())
    ck = Checks(f"emb[freqs={freqs}]")
    ck.true("columns outside the embedding unchanged",
            bits_equal(out[:, :col_off], prefill[:, :col_off]) and bits_equal(out[:, col_off + w:], prefill[:, col_off + w:]))
    sum2f = float(2 ** freqs - 1)
    bound_bwd = 4 * EPS * sum2f * g.abs().max().item()
    err_bwd = (g_x - ref[F64][0]).abs().max().item()
    e32_bwd = (ref[F32][0] - ref[F64][0]).abs().max().item()
    print(f"emb[freqs={freqs}] bwd: e32 {e32_bwd:.2e} kernel {err_bwd:.2e} bound {bound_bwd:.2e}")
    ck.true("bwd", err_bwd <= bound_bwd, f"{err_bwd:.3e} > {bound_bwd:.3e}")
    scale = (2.0 ** torch.arange(freqs, dtype=F64)).repeat(2)[None, None, :] * u.double().abs()[:, :, None]
    bound_jvp = 4 * EPS * scale.reshape(m, w)
    err_jvp = (v - ref[F64][1]).abs()
    ratio = (err_jvp / bound_jvp.clamp_min(1e-300)).max().item()
    e32_jvp = ((ref[F32][1] - ref[F64][1]).abs() / bound_jvp.clamp_min(1e-300)).max().item()
    print(f"emb[freqs={freqs}] jvp: e32 / bound {e32_jvp:.2e} kernel / bound {ratio:.2e}")
    ck.true("jvp", bool((err_jvp <= bound_jvp).all()), f"worst err / bound {ratio:.3e}")
    lhs, rhs = (v * g.double()).sum().item(), (u.double() * g_x).sum().item()
    bound_adj = 2 * 4 * EPS * sum2f * g.abs().max().item() * u.abs().sum().item()
    print(f"emb[freqs={freqs}] adjoint: |lhs - rhs| {abs(lhs - rhs):.2e} bound {bound_adj:.2e} (|lhs| {abs(lhs):.2e})")
    ck.true("adjoint identity", abs(lhs - rhs) <= bound_adj, f"{abs(lhs - rhs):.3e} > {bound_adj:.3e}")
    ck.finish()


# ---------------------------------------------------------------- (d) hash grid

BMIN, BMAX = (-1.0, -0.5, -2.0), (1.0, 1.5, 0.5)
GRIDS = [4, 16, 20, 24, 48, 64]
TABLES = [4096, 4096, 8000, 5000, 12289, 16384]
# dense 64 rows | dense 4096 rows (LDS-staged) | dense 8000 rows (20^3 is not > 8000; staged, ragged second 4096-slice)
# | hashed, not a power of two, ragged | hashed, prime, last 4096-slice holds one row | hashed, power of two
ROWS = [64, 4096, 8000, 5000, 12289, 16384]
HASHED = [False, False, False, True, True, True]


def grid_points_small(m=300, seed=31):
    """Uniform in the box widened by 5 % per side, plus rows far outside on one, two and three axes, rows exactly on
    faces, and the centre."""
    gen = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(BMIN), torch.tensor(BMAX)
    x = torch.rand(m, 3, generator=gen) * (hi - lo) * 1.1 + lo - 0.05 * (hi - lo)
    c = (lo + hi) / 2
    extra = [c.clone() for _ in range(12)]
    extra[0][0] = 50.0                      # far outside on one axis
    extra[1][1] = -40.0
    extra[2][2] = 1e4
    extra[3][0], extra[3][2] = -30.0, 7.0   # two axes
    extra[4][1], extra[4][2] = 1e3, -1e3
    extra[5][:] = torch.tensor([9.0, -9.0, 9.0])  # three axes
    extra[6][:] = torch.tensor([-1e6, 1e6, -1e6])
    extra[7][0] = lo[0]                     # exactly on faces
    extra[8][1] = hi[1]
    extra[9][:] = lo
    extra[10][:] = hi
    # extra[11]: the centre
    mix = x[:12].clone()                    # random in the other axes, not the centre
    for i in range(7):
        far = (extra[i] != c)
        extra.append(torch.where(far, extra[i], mix[i]))
    for i in (7, 8):
        onf = (extra[i] != c)
        extra.append(torch.where(onf, extra[i], mix[i]))
    return torch.cat([x, torch.stack(extra)]).float().contiguous()


def grid_points_big(m=20000, seed=32):
    gen = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(BMIN), torch.tensor(BMAX)
    return (lo + (hi - lo) * (0.01 + 0.98 * torch.rand(m, 3, generator=gen))).float().contiguous()


def grid_masks(x, smooth):
    """outside[m,3] (strictly), face rows, and the rows kept for derivative comparisons: not on a face, and for
    smooth = False more than 1e-3 (in float64 cell coordinates) from a cell face on every level and every axis on
    which the point is inside the box (outside, the coordinate is clamped: constant, nothing jumps)."""
    lo, hi = torch.tensor(BMIN, dtype=F64), torch.tensor(BMAX, dtype=F64)
    xd = x.double()
    outside = (xd < lo) | (xd > hi)
    face = ((xd == lo) | (xd == hi)).any(dim=1)
    keep = ~face
    if not smooth:
        frac = torch.clamp((xd - lo) / (hi - lo), 0, 1)
        for g in GRIDS:
            fi = (g - 1) * frac
            near = ((fi - torch.round(fi)).abs() <= 1e-3) & ~outside
            keep &= ~near.any(dim=1)
    return outside, face, keep


def grid_oracle(dt, tables, x, u, g, smooth):
    """enc [m, 2L], (d enc / d x) u, (d enc / d x)^T g, d <enc, g> / d tables, d <J u, g> / d tables by autograd
    through the oracle's encoding.  g, and the first two results, are feature-major [2L, m] like the kernels'."""
    t = tables.to(dt).requires_grad_(True)
    xx = x.to(dt).requires_grad_(True)
    bmin, bmax = torch.tensor(BMIN, dtype=dt), torch.tensor(BMAX, dtype=dt)
    off, feats = 0, []
    for r, ts, gs in zip(ROWS, TABLES, GRIDS):
        feats.append(ON.hash_table_encoding(xx, t[off:off + 2 * r].reshape(r, 2), gs, ts, bmin, bmax, smooth))
        off += 2 * r
    enc = torch.cat(feats, dim=1)
    s = (enc * g.to(dt).t()).sum()
    (g_x,) = torch.autograd.grad(s, xx, create_graph=True)
    (g_t,) = torch.autograd.grad(s, t, retain_graph=True)
    (g_t_dir,) = torch.autograd.grad((g_x * u.to(dt)).sum(), t, retain_graph=True)
    v = torch.zeros_like(enc).requires_grad_(True)
    (jt,) = torch.autograd.grad(enc, xx, grad_outputs=v, create_graph=True)
    (jvp,) = torch.autograd.grad((jt * u.to(dt)).sum(), v)
    return dict(enc=enc.detach().t(), jvp=jvp.t(), g_x=g_x.detach(), g_t=g_t, g_t_dir=g_t_dir)


def grid_setup(x, smooth, seed):
    from learn_nerf.instant_ngp import MultiresHashTableEncoding

    enc = MultiresHashTableEncoding(TABLES, GRIDS, BMIN, BMAX, 2, smooth)
    assert enc.rows() == ROWS and [bool(enc.desc().hashed[i]) for i in range(len(GRIDS))] == HASHED
    gen = torch.Generator().manual_seed(seed)
    m = x.shape[0]
    tables = (torch.rand(enc.num_table_floats(), generator=gen) * 2 - 1).float()
    u = torch.randn(m, 3, generator=gen).float()
    g = torch.randn(2 * len(GRIDS), m, generator=gen).float()
    return enc, tables, u, g


def scatter_both_ways(ck, name, desc, x, u, g, o64, o32):
    """The scatter through the bucketed path (ops, with scratch) and through the direct / LDS / sliced kernels
    (scratch = NULL), against each other at 1e-5 of the maximum and both against float64."""
    import ctypes

    from learn_nerf import _lib as L
    from learn_nerf import ops

    a = torch.zeros(o64.numel(), device="cuda")
    b = torch.zeros_like(a)
    ops.hashgrid_bwd(desc, x, g, a, u=u)
    L.check(L.lib().lnrf_hashgrid_bwd_bucketed(ctypes.byref(desc), L.ptr(x), L.ptr(u), x.shape[0], L.ptr(g), None,
                                               L.ptr(b), None, 0, L.stream()), "hashgrid_bwd_bucketed(no scratch)")
    floor = max_floor(o64)
    ck.close(f"{name} bucketed", a, o64, o32, floor=floor)
    ck.close(f"{name} direct", b, o64, o32, floor=floor)
    diff = (a - b).abs().max().item()
    print(f"{ck.case} {name}: bucketed vs direct {diff / floor:.2e} of the maximum")
    ck.true(f"{name}: bucketed vs direct", diff <= 1e-5 * floor, f"{diff / floor:.3e} of the maximum")
    off = 0
    for r in ROWS:  # every level contributes, in both
        ck.true(f"{name}: level with {r} rows", a[off:off + 2 * r].abs().sum().item() > 0 and
                b[off:off + 2 * r].abs().sum().item() > 0)
        off += 2 * r


def run_grid_case(case, x, smooth, seed, refs=None, max_dropped=0.10):
    from learn_nerf import ops

    enc, tables, u, g = grid_setup(x, smooth, seed)
    desc = enc.desc()
    outside, face, keep = grid_masks(x, smooth)
    ck = Checks(case)
    dropped = 1.0 - keep.float().mean().item() - face.float().mean().item()
    print(f"{case}: {face.sum().item()} face rows, {dropped * 100:.1f} % of the rows near a cell face left out")
    ck.true("share of rows left out", dropped <= max_dropped, f"{dropped:.3f}")
    if smooth:
        ck.true("smooth: every row off the faces compared", bool((keep == ~face).all()))
    if refs is None:
        refs = grid_references(x, smooth, tables, u, g, keep)
    full, kept = refs
    dx, dt_, du, dg = x.cuda(), tables.cuda(), u.cuda(), g.cuda()
    fl = max_floor(full[F64]["enc"])
    ck.close("fwd", ops.hashgrid_fwd(desc, dt_, dx), full[F64]["enc"], full[F32]["enc"], floor=fl)
    jvp = ops.hashgrid_jvp(desc, dt_, dx, du)
    ck.close("jvp", jvp.t(), full[F64]["jvp"].t(), full[F32]["jvp"].t(), floor=max_floor(full[F64]["jvp"][:, keep]),
             rows=keep)
    g_x = ops.hashgrid_input_grad(desc, dt_, dx, dg)
    ck.close("input_grad", g_x, full[F64]["g_x"], full[F32]["g_x"], floor=max_floor(full[F64]["g_x"][keep]), rows=keep)
    # conventions: exactly zero derivative along an axis on which the point is strictly outside the box
    if outside.any():
        ck.true("input_grad outside: +0.0 bit for bit", bool((g_x.cpu().view(torch.int32)[outside] == 0).all()))
        ck.true("input_grad inside is not zero", bool((g_x.cpu()[~outside & ~face[:, None]] != 0).all()))
        for a in range(3):
            ua = torch.zeros_like(u)
            ua[:, a] = u[:, a]
            ja = ops.hashgrid_jvp(desc, dt_, dx, ua.cuda()).cpu()
            ck.true(f"jvp of a u along axis {a}, outside on it: exactly 0", bool((ja[:, outside[:, a]] == 0).all()))
            ck.true(f"jvp of a u along axis {a}, inside: not 0",
                    bool((ja[:, ~outside[:, a] & ~face].abs().sum(dim=0) > 0).all()))
    # adjoint identity on ALL rows (outside and face rows included): the two kernels must share one convention
    lhs = (jvp.cpu().double() * g.double()).sum(dim=0)
    rhs = (u.double() * g_x.cpu().double()).sum(dim=1)
    # Scale of the terms either side sums, per row: the 8 corner weights' derivatives along an axis sum to 2 slope in
    # absolute value and |table| <= 1, so sum_terms <= sum_l (|g_l0| + |g_l1|) * 2 sum_a |u_a| slope_la, with the
    # largest slope of a level: (G - 1) / extent, or 1.5 (G - 2) / extent under the smoothstep.  Each side sums
    # 8 x 3 x 12 such terms in fp32, each formed with a handful of roundings: 32 eps of that scale per side.
    ext = torch.tensor(BMAX, dtype=F64) - torch.tensor(BMIN, dtype=F64)
    scale = torch.zeros(x.shape[0], dtype=F64)
    for l, gs in enumerate(GRIDS):
        slope = (1.5 * (gs - 2) if smooth else float(gs - 1)) / ext
        scale += (g[2 * l].double().abs() + g[2 * l + 1].double().abs()) * 2 * (u.double().abs() * slope).sum(dim=1)
    adj = ((lhs - rhs).abs() / (scale + 1e-30)).max().item()
    print(f"{case} adjoint: max |lhs - rhs| / scale {adj:.2e} (bound {64 * EPS:.2e})")
    ck.true("adjoint identity", adj <= 64 * EPS, f"{adj:.3e}")
    # scatters: on the kept rows only (the kernel gets the filtered point set)
    xk, uk, gk = x[keep].contiguous().cuda(), u[keep].contiguous().cuda(), g[:, keep].contiguous().cuda()
    scatter_both_ways(ck, "bwd", desc, xk, None, gk, kept[F64]["g_t"], kept[F32]["g_t"])
    scatter_both_ways(ck, "bwd_dir", desc, xk, uk, gk, kept[F64]["g_t_dir"], kept[F32]["g_t_dir"])
    ck.finish()
    return kept[F64]


def grid_references(x, smooth, tables, u, g, keep):
    full = {dt: grid_oracle(dt, tables, x, u, g, smooth) for dt in (F64, F32)}
    kept = {dt: grid_oracle(dt, tables, x[keep], u[keep], g[:, keep], smooth) for dt in (F64, F32)}
    return full, kept


@pytest.mark.parametrize("smooth", [False, True])
def test_hashgrid_maps_small(smooth):
    """m = 321: points inside, outside (near and far, on one to three axes), on faces and at the centre."""
    x = grid_points_small()
    outside, face, _ = grid_masks(x, smooth)
    assert face.sum() >= 6 and (outside.sum(dim=1) == 3).sum() >= 2 and (outside.sum(dim=1) == 2).sum() >= 2
    run_grid_case(f"grid[m={x.shape[0]},smooth={int(smooth)}]", x, smooth, seed=33)


@pytest.fixture(scope="module")
def big_grid_reference():
    """float64 (and float32) oracle results of the m = 20000 case, computed once per module and per `smooth`."""
    cache = {}

    def get(smooth):
        if smooth not in cache:
            x = grid_points_big()
            _, tables, u, g = grid_setup(x, smooth, seed=34)
            cache[smooth] = (x, grid_references(x, smooth, tables, u, g, grid_masks(x, smooth)[2]))
        return cache[smooth]

    return get


@pytest.mark.parametrize("smooth", [False, True])
def test_hashgrid_maps_staged(smooth, big_grid_reference):
    """m = 20000 inside the box: the three dense levels are gathered from LDS (m >= 16384, <= 8192 rows), without
    and with a direction u; the scatters meet the ragged slices with thousands of tuples per bucket."""
    x, refs = big_grid_reference(smooth)
    g_t = run_grid_case(f"grid[m={x.shape[0]},smooth={int(smooth)}]", x, smooth, seed=34, refs=refs)["g_t"]
    off = 2 * sum(ROWS[:4])
    assert g_t[off + 2 * 12288:off + 2 * 12289].abs().sum().item() > 0  # the one-row last slice of the prime table is hit

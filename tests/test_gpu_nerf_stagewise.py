"""
The fused bf16 NeRFModel kernels, stage by stage, against their own saved dumps.

lnrf_nerf_mlp_fwd / _fwd_ls leave every activation in the forward save, lnrf_nerf_mlp_bwd_chain / _bwd_ls every
pre-activation gradient in the gradient dump (csrc/nerf_layout.h kSave*, kGrad*; decoded by nerf_dump_decode.py).  Each
stage is recomputed in float64 from the KERNEL'S OWN decoded inputs, so no bf16 rounding that flips in one layer moves
anything downstream, and a stage is "exact products of bf16 values, accumulated in fp32, rounded once":

  tensors rounded to bf16 (h_l, z, h10, every dy)   check_rounded: got == bf16_rne(ref) bit for bit unless ref lies within
                                                    delta = (K + 2) 2^-23 (sum |a||b| + |bias|) of a rounding boundary
  fp32 sums (dW_l, db_l)                            check_accumulated: |got - ref| <= (n_add + 2) 2^-23 sum |x||dy|
  cap                                               the share of elements that differ from bf16_rne(ref) is at most 10 x
                                                    that of the torch.float32 CPU result of the same operands, + 8 elements

Both bounds are worst cases of fp32 accumulation (they cannot fail a correct kernel); the cap keeps the allowance region
(2 % ... 35 % of the elements) from hiding a kernel that picks the wrong neighbour.  A failure names the stage, the entry
point, the worst elements and the device.  The end-to-end oracle gates (test_gpu_nerf_mlp.py, 3e-2 per layer) remain as the
check that the stages compose.

Sizes: one partial tile, a tile boundary, several workgroups and a ragged last tile; m <= 4000 in every accumulated check
(above that the bound m 2^-23 S grows past the S / m one dropped evaluation contributes).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nerf_dump_decode as D
from nerf_grad_helpers import make_model, make_points
from test_gpu_nerf_backward_edges import SIZES, device_tag, pipelines

pytestmark = pytest.mark.gpu

MS = [1, 31, 33, 1000, 2053]
LS_SIZES = ["33", "32P-5", "32(P+8)-31", "96P+1"]
K_FWD = {0: 64, 5: 320, 10: 288, 9: 288, 11: 128}  # contraction lengths with their pad k-steps; every other layer 256
STATS = {}  # (run, stage) -> the printed figures, for the table in DESIGN.md


def _f64(t):
    return t.detach().cpu().double()


def weights_of(flat):
    """per Dense layer: bf16(kernel) as float64 [in, out] (the operand the packed streams carry), kernel in fp32 rounded
    the same way for the CPU fp32 product, and the fp32 bias"""
    f = flat.detach().cpu()
    out = []
    for w, b, fi, fo in D.dense_offsets():
        wb = f[w:b].view(fi, fo).bfloat16()
        out.append((wb.double(), wb.float(), f[b:b + fo].clone()))
    return out


def report(run, stage, m, n, n_allow, n_diff, cpu_share, need):
    STATS[(run, stage, m)] = (n_allow / n, n_diff / n, cpu_share, need)
    print(f"[stage] {run:5s} m={m:5d} {stage:8s} allowance share {n_allow / n:.3e}  mismatch share {n_diff / n:.3e}  "
          f"CPU fp32 flip share {cpu_share:.3e}  largest needed part of delta {need:.3f}")


def rounded_stage(run, entry, stage, m, got, ref, delta, cpu_f32, relu=False):
    """check_rounded + the cap for one tensor; `cpu_f32`: the torch.float32 result of the same operands (before the ReLU)"""
    what = f"{stage} ({entry}, m={m}, {device_tag()})"
    got, ref, delta, cpu = (np.asarray(_f64(a) if isinstance(a, torch.Tensor) else a, dtype=np.float64)
                            for a in (got, ref, delta, cpu_f32))
    f = (lambda v: np.maximum(v, 0.0)) if relu else (lambda v: v)
    cpu_share = float((D.bf16_rne(f(cpu)) != D.bf16_rne(f(ref))).mean())
    n_allow, n_diff = D.check_rounded(got, ref, delta, relu=relu, what=what)
    report(run, stage, m, got.size, n_allow, n_diff, cpu_share, D.needed_share_of_delta(got, ref, delta, relu=relu))
    D.check_cap(n_diff, got.size, cpu_share, what=what)


def dense_stage(run, entry, stage, m, got, inp, w, k, relu=False, mask=None):
    """one Dense stage from decoded operands: ref = inp bf16(W) (+ b), masked by `mask` where given"""
    w64, w32, b = w
    ref, s = inp @ w64, inp.abs() @ w64.abs()
    cpu = inp.float() @ w32
    if b is not None:
        ref, s, cpu = ref + b.double(), s + b.double().abs(), cpu + b
    delta = torch.from_numpy(D.dot_delta(k, s.numpy()))
    if mask is not None:
        ref, delta, cpu = ref * mask, delta * mask, cpu * mask.float()
    rounded_stage(run, entry, stage, m, got, ref, delta, cpu.double(), relu=relu)


def embedding(v32, freqs):
    """model.py:72-77 on the fp32 argument v 2^f (exact in fp32): float64 sin / cos, the torch.float32 ones, feature order
    [coordinate][sin f0.. | cos f0..]"""
    arg = (v32[:, :, None] * (2.0 ** torch.arange(freqs, dtype=torch.float32))[None, None, :])  # [m, 3, F] fp32, exact
    a64 = arg.double()
    ref = torch.cat([torch.sin(a64), torch.cos(a64)], -1).reshape(v32.shape[0], -1)
    cpu = torch.cat([torch.sin(arg), torch.cos(arg)], -1).reshape(v32.shape[0], -1)
    return ref, cpu.double()


class Run:
    pass


def lib_and_shape():
    from learn_nerf import _lib as L
    return L, L.lib(), L.NerfShape(5, 4, 256, 128, 10, 4)


def forward(model, flat, x, d, m, ls):
    """lnrf_nerf_mlp_fwd (or _fwd_ls) into a zeroed save buffer -> density, rgb, save (GPU tensors)"""
    L, lib, shape = lib_and_shape()
    packed = model.packed_weights(flat)
    save = torch.zeros(lib.lnrf_nerf_save_bytes(ctypes.byref(shape), m), dtype=torch.uint8, device="cuda")
    dens = torch.empty(m, dtype=torch.float32, device="cuda")
    rgb = torch.empty((m, 3), dtype=torch.float32, device="cuda")
    fn = lib.lnrf_nerf_mlp_fwd_ls if ls else lib.lnrf_nerf_mlp_fwd
    L.check(fn(ctypes.byref(shape), L.ptr(packed, torch.uint8), L.ptr(x), L.ptr(d), None, 6, None, 0, m, L.ptr(dens),
               L.ptr(rgb), L.ptr(save, torch.uint8), L.stream()), "nerf_mlp_fwd")
    torch.cuda.synchronize()
    return dens, rgb, save, packed


@functools.lru_cache(maxsize=None)
def split_run(m):
    """forward with save, input-gradient chain, weight gradients (twice) through the C ABI, everything decoded on the CPU;
    computed once per m and shared, unchanged, by the tests below"""
    L, lib, shape = lib_and_shape()
    model, _, flat = make_model("bf16")
    x, d, gen = make_points(m, seed=100 + m)
    g_dens = torch.randn(m, generator=gen).float()
    g_rgb = torch.randn(m, 3, generator=gen).float()
    xg, dg = x.cuda(), d.cuda()
    r = Run()
    dens, rgb, save, packed = forward(model, flat, xg, dg, m, ls=False)
    dens_ls, rgb_ls, save_ls, _ = forward(model, flat, xg, dg, m, ls=True)
    scratch = torch.zeros(lib.lnrf_nerf_bwd_scratch_bytes(ctypes.byref(shape), m), dtype=torch.uint8, device="cuda")
    gdg, grg = g_dens.cuda(), g_rgb.cuda()
    L.check(lib.lnrf_nerf_mlp_bwd_chain(ctypes.byref(shape), L.ptr(packed, torch.uint8), L.ptr(save, torch.uint8),
                                        L.ptr(dens), L.ptr(rgb), L.ptr(gdg), L.ptr(grg), m, L.ptr(scratch, torch.uint8),
                                        L.stream()), "nerf_mlp_bwd_chain")
    torch.cuda.synchronize()
    dump = scratch[:D.grad_dump_bytes(m)].cpu()
    grads = torch.zeros(D.N_PARAMS, dtype=torch.float32, device="cuda")
    out = []
    for _ in range(2):
        L.check(lib.lnrf_nerf_mlp_bwd_weights(ctypes.byref(shape), L.ptr(save, torch.uint8), L.ptr(scratch, torch.uint8), m,
                                              L.ptr(grads), L.stream()), "nerf_mlp_bwd_weights")
        torch.cuda.synchronize()
        out.append(grads.cpu().clone())
    r.m, r.x, r.d, r.g_dens, r.g_rgb = m, x, d, g_dens, g_rgb
    r.dens, r.rgb, r.dens_ls, r.rgb_ls = dens.cpu(), rgb.cpu(), dens_ls.cpu(), rgb_ls.cpu()
    r.save_raw, r.save_ls_raw, r.dump_raw = save.cpu(), save_ls.cpu(), dump
    r.save, r.grad = D.decode_save(r.save_raw, m), D.decode_grad(dump, m)
    r.grads, r.grads2 = out
    r.w = weights_of(flat)
    return r


# ---- forward ------------------------------------------------------------------------------------------------------------
def forward_stages(run, entry, r_save, x, d, w, m):
    """x_emb, d_emb, Dense_0..8, Dense_10 and the masks of one decoded save"""
    s = r_save
    for name, v, freqs in (("x_emb", x, 10), ("d_emb", d, 4)):
        ref, cpu = embedding(v, freqs)
        rounded_stage(run, entry, name, m, s[name], ref, torch.full_like(ref, 2e-7), cpu)
    ins = [s["x_emb"]] + [s["h"][l] for l in range(4)] + [torch.cat([s["h"][4], s["x_emb"]], 1)] + [s["h"][5], s["h"][6]]
    for l in range(8):
        dense_stage(run, entry, f"h{l}", m, s["h"][l], ins[l], w[l], K_FWD.get(l, 256), relu=True)
    dense_stage(run, entry, "z", m, s["z"], s["h"][7], w[8], 256)
    dense_stage(run, entry, "h10", m, s["h10"], torch.cat([s["z"], s["d_emb"]], 1), w[10], K_FWD[10], relu=True)
    what = f"({entry}, m={m}, {device_tag()})"
    for l in range(8):
        if s["mask"][l] is not None:
            bad = s["mask"][l] != (s["h"][l] > 0)
            assert not bad.any(), f"ReLU mask of h{l} {what}: {int(bad.sum())} bits differ from h{l} > 0, first at " \
                                  f"(evaluation, feature) {tuple(bad.nonzero()[0].tolist())}"
    bad = s["mask10"] != (s["h10"] > 0)
    assert not bad.any(), f"ReLU mask of h10 {what}: {int(bad.sum())} bits differ, first {tuple(bad.nonzero()[0].tolist())}"
    assert not s["mask10_high"].any(), f"h10 mask slot {what}: the 64 unused bits per lane are not zero"
    assert all(not v.any() for v in s["pad_slots"].values()), f"unused k-slots of x_emb / d_emb {what} are not zero"
    assert all(torch.isfinite(v).all() for k, v in s["pad"].items() if v.dtype == torch.float64), \
        f"pad evaluations {what} hold non-finite activations"


def ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float64))
    return np.ldexp(1.0, np.maximum(np.frexp(v)[1] - 1, -126) - 23)


def head_stage(run, entry, name, m, got32, pre, delta, fn64, fn32):
    """fp32 outputs behind softplus / tanh: |got - fn(pre)| <= delta (the accumulation bound of `pre`, both derivatives
    are <= 1) + the libm margin: 4 x the excess torch.float32 shows on the CPU for the same pre-activations, at least 4 fp32
    ulp of the result.  -> (largest excess of the kernel, of the CPU) in ulp of the result."""
    ref = fn64(pre)
    got, cpu = _f64(got32).reshape(ref.shape), fn32(pre.float()).double()
    u = torch.from_numpy(ulp32(ref.numpy()))
    ex_k = ((got - ref).abs() - delta).clamp_min(0.0)
    ex_c = ((cpu - ref).abs() - delta).clamp_min(0.0)
    gate = torch.maximum(torch.full_like(u, 4 * ex_c.max().item()), 4 * u)
    print(f"[stage] {run:5s} m={m:5d} {name:8s} libm excess over the accumulation bound: kernel {(ex_k / u).max():.2f} ulp, "
          f"CPU fp32 {(ex_c / u).max():.2f} ulp; largest |got - ref| / delta {((got - ref).abs() / delta).max():.3f}")
    STATS[(run, name, m)] = ((ex_k / u).max().item(), (ex_c / u).max().item(), ((got - ref).abs() / delta).max().item())
    bad = ex_k > gate
    assert not bad.any(), (f"{name} ({entry}, m={m}, {device_tag()}): {int(bad.sum())} values exceed the accumulation bound "
                           f"by more than the libm margin; worst excess {(ex_k / u).max():.1f} ulp at "
                           f"{tuple(((ex_k / u) == (ex_k / u).max()).nonzero()[0].tolist())}")


def head_stages(run, entry, s, dens, rgb, w, m):
    w9, w11 = w[9], w[11]
    logit = s["z"] @ w9[0] + w9[2].double()
    dl = torch.from_numpy(D.dot_delta(K_FWD[9], (s["z"].abs() @ w9[0].abs() + w9[2].double().abs()).numpy()))
    head_stage(run, entry, "density", m, dens, logit[:, 0], dl[:, 0], lambda v: torch.from_numpy(np.logaddexp(v.numpy(), 0.0)),
               torch.nn.functional.softplus)
    pre = s["h10"] @ w11[0] + w11[2].double()
    dp = torch.from_numpy(D.dot_delta(K_FWD[11], (s["h10"].abs() @ w11[0].abs() + w11[2].double().abs()).numpy()))
    head_stage(run, entry, "rgb", m, rgb, pre, dp, torch.tanh, torch.tanh)


@pytest.mark.parametrize("m", MS)
def test_forward_stage_by_stage(m):
    """lnrf_nerf_mlp_fwd: embeddings at 2e-7, every Dense output by check_rounded from its decoded input, masks == h > 0,
    density / rgb against softplus / tanh of the float64 head pre-activations.
    libm excess over the accumulation bound, measured on an MI355X over these sizes: kernel 0.00 fp32 ulp, torch.float32
    on the CPU 0.00 ulp — the whole error stays at 0.001 (density) and 0.003 (rgb) of the accumulation bound."""
    r = split_run(m)
    forward_stages("fwd", "lnrf_nerf_mlp_fwd", r.save, r.x, r.d, r.w, m)
    head_stages("fwd", "lnrf_nerf_mlp_fwd", r.save, r.dens, r.rgb, r.w, m)


@pytest.mark.parametrize("m", MS)
def test_forward_ls_writes_the_same_save(m):
    """lnrf_nerf_mlp_fwd_ls: density / rgb bit-identical, the save byte-identical outside the eight hidden-mask slots
    (which it leaves untouched: still the zeros the buffer was allocated with), the h10 mask slot identical; its stages
    are checked on its own decoded save too."""
    r = split_run(m)
    what = f"(lnrf_nerf_mlp_fwd_ls vs lnrf_nerf_mlp_fwd, m={m}, {device_tag()})"
    assert torch.equal(r.dens, r.dens_ls) and torch.equal(r.rgb, r.rgb_ls), f"density / rgb differ {what}"
    lay, _ = D.layouts()
    a, b = (t.numpy().reshape(-1, lay.n_slots, lay.frag_bytes) for t in (r.save_raw, r.save_ls_raw))
    hidden = [lay.masks[f"mask{l}"].slot for l in range(8)]
    for slot in range(lay.n_slots):
        if slot in hidden:
            assert not b[:, slot].any(), f"hidden-mask slot {slot} was written {what}"
            assert a[:, slot].any(), f"hidden-mask slot {slot} of the full save is empty {what}"
        else:
            diff = a[:, slot] != b[:, slot]
            assert not diff.any(), f"slot {slot}: {int(diff.sum())} bytes differ, first in tile {int(diff.any(1).argmax())} {what}"
    s = D.decode_save(r.save_ls_raw, m, hidden_masks=False)
    forward_stages("fwdls", "lnrf_nerf_mlp_fwd_ls", s, r.x, r.d, r.w, m)
    head_stages("fwdls", "lnrf_nerf_mlp_fwd_ls", s, r.dens_ls, r.rgb_ls, r.w, m)


# ---- input-gradient chain -----------------------------------------------------------------------------------------------
def chain_stages(run, entry, g, s, dens, rgb, g_dens, g_rgb, w, m, masks):
    """every dy of one decoded dump from the dy that feeds it (the kernel's own), the decoded masks and the kernel's own
    fp32 density / rgb"""
    what = f"({entry}, m={m}, {device_tag()})"
    y, gr = rgb.double(), g_rgb.double()
    rounded_stage(run, entry, "dy11", m, g["dy11"], gr * (1 - y * y), 4 * 2.0 ** -24 * gr.abs(), (g_rgb * (1 - rgb * rgb)).double())
    gd = g_dens.double()
    rounded_stage(run, entry, "dlogit", m, g["dlogit"], gd * -torch.expm1(-dens.double()), 8 * 2.0 ** -24 * gd.abs(),
                  (g_dens * -torch.expm1(-dens)).double())
    w64, w32, _ = w[11]
    dense_stage(run, entry, "dy10", m, g["dy10"], g["dy11"], (w64.T.contiguous(), w32.T.contiguous(), None), 3,
                mask=s["mask10"].double())
    w64 = torch.cat([w[10][0][:256], w[9][0]], 1)  # [256, 129]: the z rows of Dense_10, Dense_9
    w32 = torch.cat([w[10][1][:256], w[9][1]], 1)
    dense_stage(run, entry, "dy8", m, g["dy"][8], torch.cat([g["dy10"], g["dlogit"][:, None]], 1),
                (w64.T.contiguous(), w32.T.contiguous(), None), 129)
    for l in range(8, 0, -1):  # Dense_l^T, the h rows only of Dense_5
        w64, w32 = w[l][0][:256].T.contiguous(), w[l][1][:256].T.contiguous()
        dense_stage(run, entry, f"dy{l - 1}", m, g["dy"][l - 1], g["dy"][l], (w64, w32, None), 256, mask=masks[l - 1].double())
    for name, v in g["pad"].items():
        assert not v.any(), f"{name} {what}: the pad evaluations {m}.. hold {int((v != 0).sum())} non-zero gradients"
    for slot, v in g["zero_slots"].items():
        assert not v.any(), f"gradient-dump slot {slot} {what} is documented zero and is not"
    for name, v in g["pad_slots"].items():
        assert not v.any(), f"unused k-slots of {name} {what} are not zero"
    assert any(t.abs().max() > 0 for t in g["dy"]), what


@pytest.mark.parametrize("m", MS)
def test_chain_stage_by_stage(m):
    """lnrf_nerf_mlp_bwd_chain: dy11, dlogit, dy10, dy8, dy7..dy0 by check_rounded, zero pads and zero slots"""
    r = split_run(m)
    chain_stages("chain", "lnrf_nerf_mlp_bwd_chain", r.grad, r.save, r.dens, r.rgb, r.g_dens, r.g_rgb, r.w, m, r.save["mask"])


# ---- weight and bias gradients --------------------------------------------------------------------------------------------
def wgrad_reference(s, g):
    """float64 dW_l = in_l^T dy_l, db_l = sum dy_l from decoded operands -> reference vector, the same contractions with
    absolute values, and how often each entry of the parameter vector was written"""
    ins = [s["x_emb"]] + [s["h"][l] for l in range(4)] + [torch.cat([s["h"][4], s["x_emb"]], 1)] + \
          [s["h"][5], s["h"][6], s["h"][7], s["z"], torch.cat([s["z"], s["d_emb"]], 1), s["h10"]]
    dys = [g["dy"][l] for l in range(9)] + [g["dlogit"][:, None], g["dy10"], g["dy11"]]
    ref, ab, cover = (torch.zeros(D.N_PARAMS, dtype=torch.float64) for _ in range(3))
    for (wo, bo, fi, fo), x, dy in zip(D.dense_offsets(), ins, dys):
        assert x.shape[1] == fi and dy.shape[1] == fo
        ref[wo:bo], ab[wo:bo] = (x.T @ dy).reshape(-1), (x.abs().T @ dy.abs()).reshape(-1)
        ref[bo:bo + fo], ab[bo:bo + fo] = dy.sum(0), dy.abs().sum(0)
        cover[wo:bo + fo] += 1
    return ref, ab, cover


def wgrad_stages(run, entry, m, got, ref, ab, n_add, scale=1.0):
    worst = {}
    for l, (wo, bo, fi, fo) in enumerate(D.dense_offsets()):
        for name, a, b in ((f"dW{l}", wo, bo), (f"db{l}", bo, bo + fo)):
            worst[name] = D.check_accumulated(got[a:b].reshape(-1, fo), scale * ref[a:b].reshape(-1, fo), n_add,
                                              scale * ab[a:b].reshape(-1, fo),
                                              what=f"{name} ({entry}, m={m}, x{scale:g}, {device_tag()})")
    top = max(worst, key=worst.get)
    STATS[(run, "wgrad", m, scale)] = worst
    print(f"[stage] {run:5s} m={m:5d} dW / db x{scale:g}: largest error-to-bound ratio {worst[top]:.3f} ({top}); " +
          " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("m", MS)
def test_weight_gradients_stage_by_stage(m):
    """lnrf_nerf_mlp_bwd_weights into a zeroed vector: every dW_l and db_l (Dense_9 = z x dlogit, Dense_10 = [z | d_emb] x
    dy10 and the merged problem x_emb x [dy0 | dy5] included) by check_accumulated with n_add = m + 64 from the decoded save
    and dump; all 593,924 entries covered exactly once; a second call doubles the result within the same bound."""
    r = split_run(m)
    ref, ab, cover = wgrad_reference(r.save, r.grad)
    assert D.N_PARAMS == 593_924 and (cover == 1).all()
    assert r.grads.abs().max() > 0
    wgrad_stages("split", "lnrf_nerf_mlp_bwd_weights", m, r.grads, ref, ab, m + 64)
    wgrad_stages("split", "lnrf_nerf_mlp_bwd_weights, second call", m, r.grads2, ref, ab, m + 64, scale=2.0)


# ---- layer-stationary backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", LS_SIZES)
def test_layer_stationary_backward_stage_by_stage(size):
    """model.backward_kernel = "ls": the dump at the front of ctx["ls_scratch"] passes the chain checks (masks of the hidden
    layers = saved activation > 0, which is what the pipeline gates with), its gradient vector passes check_accumulated
    (n_add = m + 128) against the reference built from ITS OWN dump and save, the status word is 0, and its dump is
    byte-identical to the one lnrf_nerf_mlp_bwd_chain writes for the same inputs."""
    from learn_nerf.model import ls_status

    L, lib, shape = lib_and_shape()
    m = SIZES[size](pipelines())
    assert m <= 4000
    model, _, flat = make_model("bf16")
    x, d, gen = make_points(m, seed=300 + m)
    g_dens = torch.randn(m, generator=gen).float()
    g_rgb = torch.randn(m, 3, generator=gen).float()
    xg, dg, gdg, grg = x.cuda(), d.cuda(), g_dens.cuda(), g_rgb.cuda()
    model.backward_kernel = "ls"
    dens, rgb, _, ctx = model.forward_points(flat, xg, dg, save=True)
    grads = torch.zeros_like(flat)
    model.backward(ctx, gdg, grg, None, grads)
    status = ls_status(ctx)  # synchronises
    dump_ls = ctx["ls_scratch"][:D.grad_dump_bytes(m)].cpu()
    save_ls = ctx["save"][:lib.lnrf_nerf_save_bytes(ctypes.byref(shape), m)].cpu()
    dens, rgb, grads = dens.cpu(), rgb.cpu(), grads.cpu()
    what = f"(m={m}, {device_tag()})"
    assert status == 0, f"ls_status {status} {what}"
    w = weights_of(flat)
    s, g = D.decode_save(save_ls, m, hidden_masks=False), D.decode_grad(dump_ls, m)
    chain_stages("ls", "lnrf_nerf_mlp_bwd_ls", g, s, dens, rgb, g_dens, g_rgb, w, m, [h > 0 for h in s["h"]])
    ref, ab, cover = wgrad_reference(s, g)
    assert (cover == 1).all() and grads.abs().max() > 0
    wgrad_stages("ls", "lnrf_nerf_mlp_bwd_ls", m, grads, ref, ab, m + 128)

    # the two-launch path on the same inputs: the pre-activation gradients are identical, byte for byte
    dens2, rgb2, save2, packed = forward(model, flat, xg, dg, m, ls=False)
    scratch = torch.zeros(lib.lnrf_nerf_bwd_scratch_bytes(ctypes.byref(shape), m), dtype=torch.uint8, device="cuda")
    L.check(lib.lnrf_nerf_mlp_bwd_chain(ctypes.byref(shape), L.ptr(packed, torch.uint8), L.ptr(save2, torch.uint8),
                                        L.ptr(dens2), L.ptr(rgb2), L.ptr(gdg), L.ptr(grg), m, L.ptr(scratch, torch.uint8),
                                        L.stream()), "nerf_mlp_bwd_chain")
    torch.cuda.synchronize()
    dump2 = scratch[:D.grad_dump_bytes(m)].cpu()
    g2 = D.decode_grad(dump2, m)
    for name, a, b in [(f"dy{l}", g["dy"][l], g2["dy"][l]) for l in range(8, -1, -1)] + \
                      [(k, g[k], g2[k]) for k in ("dy11", "dy10", "dlogit")]:
        diff = a != b
        assert not diff.any(), (f"{name}: {int(diff.sum())} elements differ between lnrf_nerf_mlp_bwd_ls and "
                                f"lnrf_nerf_mlp_bwd_chain, first at {tuple(diff.nonzero()[0].tolist())} {what}")
    assert torch.equal(dump_ls, dump2), f"the two gradient dumps decode alike but differ in their bytes {what}"

"""
lnrf_distortion (csrc/rays.hip distortion_kernel) against the float64 reference on the kernel's own float32 inputs, within
the derived bound of tests/distortion_reference.py (whose CPU half is tests/test_distortion_cpu.py).

Cases: 37 rays (ten workgroups, the last with one ray) with three missed ones at T = 1, 2, 63, 64, 65, 128, 129, 192; the
opaque / empty / late families of rays_edge_cases; 128 of 192 samples clustered into 1 % of the range; repeated samples
(delta = 0); rays with t_max == t_min.  Beyond the values: accumulation into a filled gradient, untouched rows and exact
zeros for rays without a loss (on poisoned loss buffers), loss-only and gradient-only calls, bit reproducibility, guard
words behind both outputs and the argument errors.
"""
import functools

import pytest
import torch

import distortion_reference as DR
from gpu_poison import poisoned

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ERR_ARG = -1
CASES = dict(DR.all_cases())
GUARD_WORDS, GUARD_VALUE = 64, 12345.0


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, loss[N], gradient[N,T], loss bound, gradient bound, rays with a loss) — float64, computed once per case."""
    case = CASES[name]()
    loss, grad = DR.stage_formulas(case)
    l_b, g_b = DR.error_bound(case)
    return case, loss, grad, l_b, g_b, DR.Stages(case).valid


class Dev:
    def __init__(self, case):
        self.n, self.t = case.ts.shape
        self.ts, self.t_min, self.t_max = case.ts.cuda(), case.t_min.cuda(), case.t_max.cuda()
        self.mask, self.dens = case.mask.to(torch.uint8).cuda(), case.dens.cuda()

    def run(self, g_density=None, grad_scale=0.0, want_loss=True):
        from learn_nerf import ops

        return ops.distortion(self.ts, self.t_min, self.t_max, self.mask, self.dens, g_density=g_density,
                              grad_scale=grad_scale, want_loss=want_loss)

    def abi(self, n, t, loss_ptr, g_ptr, grad_scale=1.0):
        from learn_nerf import _lib as L

        return L.lib().lnrf_distortion(L.ptr(self.ts), L.ptr(self.t_min), L.ptr(self.t_max), L.ptr(self.mask, torch.uint8),
                                       L.ptr(self.dens), n, t, grad_scale, loss_ptr, g_ptr, L.stream())


def last_error() -> str:
    from learn_nerf import _lib as L

    return (L.lib().lnrf_last_error() or b"").decode()


@pytest.mark.parametrize("name", list(CASES))
def test_matches_float64_within_the_bound(name):
    case, l_ref, g_ref, l_b, g_b, valid = reference(name)
    d = Dev(case)
    gd = torch.zeros(d.n, d.t, device="cuda")
    with poisoned(0xFF):  # the loss buffer starts as NaN words: a ray the kernel skipped would show
        loss = d.run(gd, grad_scale=1.0)
    assert torch.isfinite(loss).all() and torch.isfinite(gd).all()
    l_err = (loss.cpu().double() - l_ref).abs()
    g_err = (gd.cpu().double() - g_ref).abs()
    l_ratio = torch.where(l_err == 0, torch.zeros_like(l_err), l_err / l_b).max().item()
    g_ratio = torch.where(g_err == 0, torch.zeros_like(g_err), g_err / g_b).max().item()
    print(f"{name}: loss |d| {l_err.max().item():.2e} (bound up to {l_b.max().item():.2e}, worst ratio {l_ratio:.3f}); "
          f"gradient |d| {g_err.max().item():.2e} (bound up to {g_b.max().item():.2e}, worst ratio {g_ratio:.3f})")
    assert l_ratio <= 1.0 and g_ratio <= 1.0
    assert (loss.cpu()[~valid] == 0).all() and (gd.cpu()[~valid] == 0).all()
    if name == "empty":
        assert (loss == 0).all() and (gd == 0).all()
    if name == "zero_range":
        assert (~valid)[list(DR.ZERO_RANGE_ROWS)].all() and case.mask[list(DR.ZERO_RANGE_ROWS)].all()


@pytest.mark.parametrize("name", ["T1", "T65", "T192", "opaque", "zero_range"])
def test_accumulates_and_leaves_rays_without_a_loss_alone(name):
    """g_density += grad_scale * dL/dsigma: into a random prefill the result is prefill + x bit for bit, x the fp32 values
    a call into zeros stores; rows of rays without a loss keep the prefill's bits, their loss is exactly 0 on a poisoned
    buffer; loss-only and gradient-only calls and a second run give the same bits."""
    case, _, _, _, _, valid = reference(name)
    d = Dev(case)
    scale = 0.375
    zero = torch.zeros(d.n, d.t, device="cuda")
    loss = d.run(zero, grad_scale=scale)
    assert zero.abs().max().item() > 0
    gen = torch.Generator().manual_seed(7)
    prefill = torch.randn(d.n, d.t, generator=gen).cuda()
    for pattern in (0x41, 0xFF):
        acc = prefill.clone()
        with poisoned(pattern):
            loss2 = d.run(acc, grad_scale=scale)
        assert torch.equal(acc, prefill + zero)
        assert torch.equal(loss2, loss)
        assert (loss2.cpu()[~valid] == 0).all()
        assert torch.equal(acc.cpu()[~valid].view(torch.int32), prefill.cpu()[~valid].view(torch.int32))
    assert torch.equal(d.run(), loss)                       # loss only
    only_g = torch.zeros(d.n, d.t, device="cuda")
    assert d.run(only_g, grad_scale=scale, want_loss=False) is None
    assert torch.equal(only_g.view(torch.int32), zero.view(torch.int32))
    # grad_scale 0 adds zeros: monitor mode may as well pass no gradient
    same = prefill.clone()
    d.run(same, grad_scale=0.0)
    assert torch.equal(same, prefill)


@pytest.mark.parametrize("name", ["T1", "T129"])
def test_guard_words_and_argument_errors(name):
    from learn_nerf import _lib as L

    case, l_ref, g_ref, l_b, g_b, _ = reference(name)
    d = Dev(case)
    n, t = d.n, d.t
    loss = torch.full((n + GUARD_WORDS,), GUARD_VALUE, device="cuda")
    gd = torch.full((n * t + GUARD_WORDS,), GUARD_VALUE, device="cuda")
    gd[:n * t] = 0
    assert d.abi(n, t, L.ptr(loss), L.ptr(gd)) == 0, last_error()
    torch.cuda.synchronize()
    assert (loss[n:] == GUARD_VALUE).all() and (gd[n * t:] == GUARD_VALUE).all()
    assert ((loss[:n].cpu().double() - l_ref).abs() <= l_b).all()
    assert ((gd[:n * t].cpu().double().reshape(n, t) - g_ref).abs() <= g_b).all()

    before_l, before_g = loss.clone(), gd.clone()
    assert d.abi(n, 0, L.ptr(loss), L.ptr(gd)) == ERR_ARG and "bad sizes" in last_error()
    assert d.abi(-1, t, L.ptr(loss), L.ptr(gd)) == ERR_ARG and "bad sizes" in last_error()
    assert d.abi(n, t, None, None) == ERR_ARG and "NULL" in last_error()
    assert d.abi(0, t, L.ptr(loss), L.ptr(gd)) == 0  # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert torch.equal(loss, before_l) and torch.equal(gd, before_g)

"""
GPU parity of the per-ray kernels (HIP, through the C ABI) against the oracle on identical
rays / uniforms.  Tolerances: fp32 kernels vs the float64 oracle, stated per assert.
"""
import numpy as np
import pytest
import torch

from oracle import philox
from oracle import render as OR
from rays_edge_cases import fine_cdf_check

pytestmark = pytest.mark.gpu

F64 = torch.float64
BBOX_MIN = (-1.0, -1.0, -1.0)
BBOX_MAX = (1.0, 1.0, 1.0)


def make_rays(n, seed=0, miss_frac=0.1):
    gen = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=gen)
    o = 4 * o / o.norm(dim=-1, keepdim=True)
    d = -o + (torch.rand(n, 3, generator=gen) - 0.5) * 0.6
    n_miss = int(n * miss_frac)
    if n_miss:
        d[:n_miss] = torch.randn(n_miss, 3, generator=gen)  # mostly misses
    d = d / d.norm(dim=-1, keepdim=True)
    return torch.stack([o, d], dim=1).float().contiguous(), gen


def oracle_samples(rays, count, u):
    bbox = torch.tensor([BBOX_MIN, BBOX_MAX], dtype=F64)
    r = rays.double()
    t_min, t_max, mask = OR.ray_t_range(bbox, r)
    ts = OR.stratified_ts(t_min, t_max, count, u.double())
    return OR.RaySamples(t_min, t_max, mask, ts)


@pytest.mark.parametrize("n,count", [(1, 1), (257, 64), (1000, 7)])
def test_ray_aabb_stratified_explicit_u(n, count):
    from learn_nerf import ops

    rays, gen = make_rays(n)
    u = torch.rand(n, count, generator=gen)
    s = oracle_samples(rays, count, u)
    t_min, t_max, mask, ts = ops.ray_aabb_stratified(rays.cuda(), BBOX_MIN, BBOX_MAX, count, u=u.cuda())
    assert torch.equal(mask.cpu().bool(), s.mask)
    assert torch.allclose(t_min.cpu().double(), s.t_min, rtol=1e-5, atol=1e-6)
    assert torch.allclose(t_max.cpu().double(), s.t_max, rtol=1e-5, atol=1e-6)
    assert torch.allclose(ts.cpu().double(), s.ts, rtol=1e-5, atol=1e-5)


def test_ray_aabb_training_batch_stride_and_count0():
    from learn_nerf import ops

    rays, gen = make_rays(100)
    batch = torch.cat([rays, torch.rand(100, 1, 3, generator=gen)], dim=1).contiguous()  # [N,3,3]
    a = ops.ray_aabb_stratified(batch.cuda(), BBOX_MIN, BBOX_MAX, 0)
    b = ops.ray_aabb_stratified(rays.cuda(), BBOX_MIN, BBOX_MAX, 0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[3].shape == (100, 0)


def test_philox_uniforms_bit_exact_and_offset():
    from learn_nerf import ops

    n, count = 300, 64
    rays, _ = make_rays(n, miss_frac=0.0)
    # recover u from ts: ts = t_min + (i + u) * bin  -> use explicit path for comparison instead
    u_ref = torch.from_numpy(philox.ray_uniforms(0xDEADBEEFCAFE, 3, 17, n, count))
    a = ops.ray_aabb_stratified(rays.cuda(), BBOX_MIN, BBOX_MAX, count, u=u_ref.cuda())
    b = ops.ray_aabb_stratified(rays.cuda(), BBOX_MIN, BBOX_MAX, count, seed=0xDEADBEEFCAFE, stream_id=3,
                                ray_offset=17)
    assert torch.equal(a[3], b[3])  # bit-exact: kernel Philox == oracle Philox
    ts2 = ops.stratified(a[0], a[1], count, seed=0xDEADBEEFCAFE, stream_id=3, ray_offset=17)
    assert torch.equal(ts2, a[3])


@pytest.mark.parametrize("n,t", [(5, 1), (130, 64), (64, 192), (33, 200)])
def test_termination_probs_and_composite_fwd(n, t):
    from learn_nerf import ops

    rays, gen = make_rays(n)
    u = torch.rand(n, t, generator=gen)
    s = oracle_samples(rays, t, u)
    dens = (torch.rand(n, t, generator=gen) * 6).float()
    dens[:, ::5] = 0.0
    rgb = (torch.rand(n, t, 3, generator=gen) * 2 - 1).float()
    aux = torch.rand(n, t, 2, generator=gen).float()
    bg = torch.tensor([-1.0, 0.25, 0.5])
    tgt = (torch.rand(n, 3, generator=gen) * 2 - 1).float()

    p_ref = s.termination_probs(dens.double())
    out_ref = s.render_rays(dens.double(), rgb.double(), bg.double())
    alpha_ref = s.render_alpha(dens.double())[:, 0]
    coords_ref = s.render_rays(dens.double(), s.points(rays.double()), torch.zeros(3, dtype=F64))
    aux_ref = torch.where(s.mask[:, None], (aux.double() * p_ref[:, :-1, None]).sum(1), torch.zeros(n, 2, dtype=F64))

    g = lambda x: x.cuda()
    t_min, t_max, mask, ts = ops.ray_aabb_stratified(g(rays), BBOX_MIN, BBOX_MAX, t, u=g(u))
    probs = ops.termination_probs(ts, t_min, t_max, g(dens))
    assert torch.allclose(probs.cpu().double(), p_ref, atol=2e-6)
    sq = torch.zeros(1, device="cuda")
    outputs, alphas, coords, aux_sum = ops.composite_fwd(g(rays), ts, t_min, t_max, mask, g(dens), g(rgb),
                                                        g(bg), aux=g(aux), targets=g(tgt), sq_err=sq)
    assert torch.allclose(outputs.cpu().double(), out_ref, atol=5e-6)
    assert torch.allclose(alphas.cpu().double(), alpha_ref, atol=5e-6)
    assert torch.allclose(coords.cpu().double(), coords_ref, atol=2e-5)
    assert torch.allclose(aux_sum.cpu().double(), aux_ref, atol=5e-6)
    sq_ref = ((out_ref - tgt.double()) ** 2).sum()
    assert abs(sq.item() - sq_ref.item()) <= 1e-5 * max(1.0, sq_ref.item())
    # masked rays: exactly the background, alpha 0
    miss = ~s.mask
    if miss.any():
        assert torch.equal(outputs.cpu()[miss], bg.expand(int(miss.sum()), 3))
        assert (alphas.cpu()[miss] == 0).all()


@pytest.mark.parametrize("n,tc,tf", [(64, 64, 128), (37, 16, 0), (50, 64, 5), (20, 100, 150)])
def test_fine_sample(n, tc, tf):
    from learn_nerf import ops

    rays, gen = make_rays(n)
    u = torch.rand(n, tc, generator=gen)
    uf = torch.rand(n, tf, generator=gen)
    s = oracle_samples(rays, tc, u)
    dens = (torch.rand(n, tc, generator=gen) ** 4 * 30).float()
    dens[:, : tc // 3] = 0.0  # empty space in front: flat CDF segments
    g = lambda x: x.cuda()
    t_min, t_max, mask, ts = ops.ray_aabb_stratified(g(rays), BBOX_MIN, BBOX_MAX, tc, u=g(u))
    out = ops.fine_sample(ts, t_min, t_max, g(dens), tf, u=g(uf))
    assert out.shape == (n, tc + tf)
    o = out.cpu()
    assert (o[:, 1:] >= o[:, :-1]).all(), "fine samples must be sorted (render.py:255)"
    new_only = ops.fine_sample(ts, t_min, t_max, g(dens), tf, u=g(uf), combine=False).cpu()
    # combine == exact sort of [coarse ts, new ts] (render.py:253-255): bit-exact check
    assert torch.equal(o, torch.sort(torch.cat([ts.cpu(), new_only], 1), 1).values)
    if tf == 0:
        return
    # parity in CDF space, see fine_cdf_check (the same bounds the edge-case tests use)
    fine_cdf_check(new_only, s, dens, uf)


def test_fine_sample_sorts_unsorted_and_tied_input():
    """lnrf_fine_sample's final sort (render.py:253-255) must not depend on the coarse ts being in order: shuffled
    coarse ts take the rank-count path, ties between the two lists (density 0 everywhere -> flat CDF -> new ts pile up
    on bin edges) take the merge path; both must equal torch.sort bit for bit."""
    from learn_nerf import ops

    n, tc, tf = 33, 64, 128
    rays, gen = make_rays(n)
    g = lambda x: x.cuda()
    t_min, t_max, mask, ts = ops.ray_aabb_stratified(g(rays), BBOX_MIN, BBOX_MAX, tc, u=g(torch.rand(n, tc, generator=gen)))
    uf = g(torch.rand(n, tf, generator=gen))
    perm = torch.stack([torch.randperm(tc, generator=gen) for _ in range(n)]).cuda()
    cases = {"shuffled": (torch.gather(ts, 1, perm), g((torch.rand(n, tc, generator=gen) * 5).float())),
             "ties": (ts, torch.zeros(n, tc, device="cuda"))}
    for name, (ts_in, dens) in cases.items():
        out = ops.fine_sample(ts_in, t_min, t_max, dens, tf, u=uf)
        new_only = ops.fine_sample(ts_in, t_min, t_max, dens, tf, u=uf, combine=False)
        want = torch.sort(torch.cat([ts_in, new_only], 1), 1).values
        assert torch.equal(out, want), name


@pytest.mark.parametrize("n,t,n_aux", [(40, 64, 0), (33, 192, 2), (7, 70, 1)])
def test_composite_bwd_matches_autograd(n, t, n_aux):
    from learn_nerf import ops

    rays, gen = make_rays(n)
    u = torch.rand(n, t, generator=gen)
    s = oracle_samples(rays, t, u)
    dens = (torch.rand(n, t, generator=gen) * 4).float()
    rgb = (torch.rand(n, t, 3, generator=gen) * 2 - 1).float()
    aux = torch.rand(n, t, max(n_aux, 1), generator=gen).float()[..., :n_aux]
    bg = torch.tensor([-0.5, 0.1, 0.7])
    tgt = (torch.rand(n, 3, generator=gen) * 2 - 1).float()
    gw = [0.3, 0.05][:n_aux]
    scale = 2.0 / (3 * n)

    d64 = dens.double().requires_grad_(True)
    c64 = rgb.double().requires_grad_(True)
    a64 = aux.double().requires_grad_(True)
    b64 = bg.double().requires_grad_(True)
    out = s.render_rays(d64, c64, b64)
    loss = ((out - tgt.double()) ** 2).mean()
    if n_aux:
        p = s.termination_probs(d64)[:, :-1]
        aux_sum = torch.where(s.mask[:, None], (a64 * p[..., None]).sum(1), torch.zeros(n, n_aux, dtype=F64))
        loss = loss + (aux_sum * torch.tensor(gw, dtype=F64)).sum()
    grads = torch.autograd.grad(loss, [d64, c64, b64] + ([a64] if n_aux else []))

    g = lambda x: x.cuda()
    t_min, t_max, mask, ts = ops.ray_aabb_stratified(g(rays), BBOX_MIN, BBOX_MAX, t, u=g(u))
    outputs, _, _, _ = ops.composite_fwd(None, ts, t_min, t_max, mask, g(dens), g(rgb), g(bg),
                                         aux=g(aux) if n_aux else None, want_coords=False)
    g_bg = torch.zeros(3, device="cuda")
    gd, gc, ga = ops.composite_bwd(ts, t_min, t_max, mask, g(dens), g(rgb), g(bg), g_bg, outputs=outputs,
                                   targets=g(tgt), out_scale=scale, aux=g(aux) if n_aux else None, g_aux_w=gw)
    assert torch.allclose(gd.cpu().double(), grads[0], atol=2e-6, rtol=1e-4)
    assert torch.allclose(gc.cpu().double(), grads[1], atol=2e-7, rtol=1e-4)
    assert torch.allclose(g_bg.cpu().double(), grads[2], atol=2e-6, rtol=1e-4)
    if n_aux:
        assert torch.allclose(ga.cpu().double(), grads[3], atol=2e-7, rtol=1e-4)
    # explicit upstream gradient path gives the same answer
    g_out = (scale * (outputs - g(tgt))).contiguous()
    g_bg2 = torch.zeros(3, device="cuda")
    gd2, gc2, _ = ops.composite_bwd(ts, t_min, t_max, mask, g(dens), g(rgb), g(bg), g_bg2, g_out=g_out,
                                    aux=g(aux) if n_aux else None, g_aux_w=gw)
    assert torch.equal(gd, gd2) and torch.equal(gc, gc2)


def test_ray_points():
    from learn_nerf import ops

    rays, gen = make_rays(50)
    ts = torch.rand(50, 9, generator=gen) * 5
    pts, dirs = ops.ray_points(rays.cuda(), ts.cuda())
    ref = rays[:, :1] + rays[:, 1:2] * ts[:, :, None]
    assert torch.allclose(pts.cpu(), ref, atol=1e-6)
    assert torch.equal(dirs.cpu(), rays[:, 1:2].expand(50, 9, 3))

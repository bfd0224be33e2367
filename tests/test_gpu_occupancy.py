"""
The occupancy-grid kernels (lnrf_occ_build, lnrf_occ_clip_rays, lnrf_compact_mask, lnrf_scatter_rows) against the NumPy
float32 restatement of tests/occupancy_reference.py, bit for bit, and NeRFRenderer.occupancy against the pipeline
without compaction.
"""
import numpy as np
import pytest
import torch

import occupancy_reference as R

pytestmark = pytest.mark.gpu
F = np.float32
NS = (1, 63, 64, 65, 4113)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits_tensor(bits_u32: np.ndarray) -> torch.Tensor:
    return cuda(bits_u32.view(np.int32))


def same_bits(t: torch.Tensor, a: np.ndarray) -> bool:
    """bit-for-bit equality of a GPU tensor and a NumPy array (float32 compared as words, so -0.0 != 0.0, NaN == NaN)"""
    want = torch.from_numpy(np.ascontiguousarray(a))
    if want.dtype == torch.float32:
        return t.dtype == torch.float32 and torch.equal(t.cpu().view(torch.int32), want.view(torch.int32))
    return torch.equal(t.cpu(), want)


# ------------------------------------------------------------------------------------------------ build
@pytest.mark.parametrize("res", [1, 2, 5, 33])
def test_build_equals_the_restatement(res):
    from learn_nerf import ops

    rng = np.random.default_rng(res)
    sigma = (rng.random((res + 1) ** 3) * 1.1).astype(F)  # about 10 % above the threshold 1.0
    sigma[sigma > 1.0] += F(1.0)
    sigma[rng.integers(0, sigma.size)] = np.nan
    sigma[rng.integers(0, sigma.size)] = np.inf
    dev = cuda(sigma)
    for thr, dilate in ((1.0, 0), (1.0, 1), (1.0, 2), (0.0, 0), (0.0, 1)):
        bits, count = ops.occ_build(dev, res, thr, dilate)
        want_bits, want_count = R.build(sigma, res, thr, dilate)
        assert bits.dtype == torch.int32 and bits.shape == ((res ** 3 + 31) // 32,)
        assert torch.equal(bits.cpu(), torch.from_numpy(want_bits.view(np.int32))), (thr, dilate)
        assert count == want_count == R.popcount(bits.cpu().numpy().view(np.uint32))
        if thr == 0.0:
            assert count == res ** 3


def test_build_rejects_bad_arguments():
    from learn_nerf import ops

    with pytest.raises(ValueError):
        ops.occ_build(torch.zeros(27, device="cuda"), 3, 1.0, 0)  # 3^3 corners are a resolution of 2
    with pytest.raises(ValueError):
        ops.occ_build(torch.zeros(1, device="cuda"), 0, 1.0, 0)
    with pytest.raises(RuntimeError, match="dilate"):
        ops.occ_build(torch.zeros(27, device="cuda"), 2, 1.0, -1)


# ------------------------------------------------------------------------------------------------ clip
@pytest.mark.parametrize("res", [1, 4, 33])
@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_clip_equals_the_restatement(res, kind):
    from learn_nerf import ops

    rays = R.make_rays(max(NS), res, seed=res)
    occ = R.make_grid(kind, res, seed=1)
    bits = R.pack_bits(occ)
    t_min, t_max, mask = R.box_range(rays, R.BOX_MIN, R.BOX_MAX)
    want = R.clip(rays, R.BOX_MIN, R.BOX_MAX, res, bits, t_min, t_max, mask)  # per ray: one restatement serves every n
    dev_bits = bits_tensor(bits)
    for n in NS:
        r = cuda(rays[:n])
        b_min, b_max, b_mask, _ = ops.ray_aabb_stratified(r, R.BOX_MIN, R.BOX_MAX, 0)
        # the inputs are the existing box test's, and the restatement of that test agrees with it
        assert same_bits(b_min, t_min[:n]) and same_bits(b_max, t_max[:n]) and same_bits(b_mask, mask[:n])
        lo, hi, out = ops.occ_clip_rays(r, R.BOX_MIN, R.BOX_MAX, dev_bits, res, b_min, b_max, b_mask)
        assert same_bits(lo, want[0][:n]), (n, "t_min")
        assert same_bits(hi, want[1][:n]), (n, "t_max")
        assert same_bits(out, want[2][:n]), (n, "mask")
        if kind == "full":
            assert torch.equal(lo, b_min) and torch.equal(hi, b_max) and torch.equal(out, b_mask)
        if kind == "empty":
            assert not out.any()
    if kind in ("single", "random5", "shell") and res > 1:
        assert 0 < int(want[2].sum()) < int(mask.sum())  # the case does clip


def test_clip_accepts_training_batches_and_the_grid_object():
    """[N, 3, 3] rays (stride 9) and OccupancyGrid.clip with a bool mask give what the plain call gives."""
    from learn_nerf import ops
    from learn_nerf.occupancy import OccupancyGrid

    res = 4
    rays = R.make_rays(65, res, seed=2)
    occ = R.make_grid("shell", res)
    bits = bits_tensor(R.pack_bits(occ))
    r2 = cuda(rays)
    r3 = torch.cat([r2, torch.rand(65, 1, 3, device="cuda")], dim=1).contiguous()
    t_min, t_max, mask, _ = ops.ray_aabb_stratified(r2, R.BOX_MIN, R.BOX_MAX, 0)
    plain = ops.occ_clip_rays(r2, R.BOX_MIN, R.BOX_MAX, bits, res, t_min, t_max, mask)
    grid = OccupancyGrid(bits=bits, resolution=res, bbox_min=R.BOX_MIN, bbox_max=R.BOX_MAX, sigma_thr=0.0,
                         occupied=int(occ.sum()))
    for got in (ops.occ_clip_rays(r3, R.BOX_MIN, R.BOX_MAX, bits, res, t_min, t_max, mask),
                grid.clip(r2, t_min, t_max, mask.bool())):
        assert all(torch.equal(a, b) for a, b in zip(got, plain))
    assert grid.occupied_fraction == occ.mean()


# ------------------------------------------------------------------------------------------------ compact, scatter
@pytest.mark.parametrize("n", NS)
def test_compact_and_scatter(n):
    from learn_nerf import ops

    rng = np.random.default_rng(n)
    src = torch.from_numpy(rng.normal(size=(n, 7)).astype(F)).cuda()
    for mask in (np.zeros(n, np.uint8), np.ones(n, np.uint8), (rng.random(n) < 0.4).astype(np.uint8) * 3):
        idx = ops.compact_mask(cuda(mask))
        want, count = R.compact(mask)
        assert idx.dtype == torch.int32 and idx.shape == (count,)
        assert torch.equal(idx.cpu(), torch.from_numpy(want))
        gathered = ops.gather_rows_into(src, idx, torch.empty((count, 7), device="cuda"))
        out = torch.full((n, 7), -7.0, device="cuda")
        ops.scatter_rows_into(gathered, idx, out)
        live = torch.from_numpy(mask != 0).cuda()
        assert torch.equal(out[live], src[live])  # scatter after gather: the identity on the named rows
        assert (out[~live] == -7.0).all()  # and the others are left alone


def test_scatter_skips_indices_outside_the_output():
    from learn_nerf import ops

    src = torch.ones((3, 2), device="cuda")
    out = torch.zeros((4, 2), device="cuda")
    ops.scatter_rows_into(src, torch.tensor([-1, 2, 4], dtype=torch.int32, device="cuda"), out)
    assert torch.equal(out.cpu(), torch.tensor([[0.0, 0], [0, 0], [1, 1], [0, 0]]))


# ------------------------------------------------------------------------------------------------ renderer
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
TC = TF = 8
N_RAYS = 300
GRID_RES = 8


def model_pair(kind):
    from learn_nerf.instant_ngp import InstantNGPModel
    from learn_nerf.model import NeRFModel

    if kind == "nerf":  # the default shape: the fused split-precision kernels
        return NeRFModel(), NeRFModel()
    if kind == "refnerf":  # a model with aux losses, whose means over rays count a culled ray as zero
        from learn_nerf.ref_nerf import RefNERFModel

        return RefNERFModel(), RefNERFModel()
    small = dict(table_sizes=[256, 256], grid_sizes=[4, 8], bbox_min=BMIN, bbox_max=BMAX, hidden_dim=64)
    return InstantNGPModel(**small), InstantNGPModel(**small)


@pytest.fixture(scope="module", params=["nerf", "ngp", "refnerf"])
def renderer(request):
    from learn_nerf.render import NeRFRenderer

    coarse, fine = model_pair(request.param)
    cp = coarse.init(dict(params=1))["params"]
    fp = fine.init(dict(params=2))["params"]
    background = torch.tensor([0.25, -0.5, 0.75], device="cuda")
    return NeRFRenderer(coarse=coarse, fine=fine, coarse_params=cp, fine_params=fp, background=background,
                        bbox_min=BMIN, bbox_max=BMAX, coarse_ts=TC, fine_ts=TF)


def render_batch(hit_only: bool):
    rays = R.make_rays(4 * N_RAYS, GRID_RES, seed=5, bbox_min=BMIN, bbox_max=BMAX)
    rays = rays[R.box_range(rays, BMIN, BMAX)[2] != 0][:N_RAYS].copy()
    assert len(rays) == N_RAYS
    if not hit_only:
        rays[5::10, 0, 1] += F(50.0)  # every tenth ray is moved far off and misses the box
    return cuda(rays)


def same_aux(got, want) -> bool:
    return list(got) == list(want) and all(torch.equal(got[name], want[name]) for name in want)


def with_grid(renderer, occ: np.ndarray):
    import dataclasses

    from learn_nerf.occupancy import OccupancyGrid

    grid = OccupancyGrid(bits=bits_tensor(R.pack_bits(occ)), resolution=GRID_RES, bbox_min=BMIN, bbox_max=BMAX,
                         sigma_thr=0.0, occupied=int(occ.sum()))
    return dataclasses.replace(renderer, occupancy=grid)


def uncompacted(renderer, grid, key, batch):
    """The pipeline of NeRFRenderer.render_rays from public pieces, every model on every ray, with the clipped ranges."""
    from learn_nerf import ops
    from learn_nerf.render import RaySamples, render_rays
    from learn_nerf.rng import split

    coarse_key, fine_key = split(key, 2)
    t_min, t_max, mask, _ = ops.ray_aabb_stratified(batch, BMIN, BMAX, 0, min_t_range=renderer.min_t_range)
    t_min, t_max, mask = grid.clip(batch, t_min, t_max, mask, min_t_range=renderer.min_t_range)
    coarse_ts = RaySamples.stratified_sampling(t_min, t_max, mask, renderer.coarse_ts, coarse_key)
    coarse_out, coarse_aux = render_rays(renderer.coarse, renderer.coarse_params, renderer.background, batch, coarse_ts)
    fine_ts = coarse_ts.fine_sampling(count=renderer.fine_ts, key=fine_key, densities=coarse_out["densities"])
    fine_out, fine_aux = render_rays(renderer.fine, renderer.fine_params, renderer.background, batch, fine_ts)
    return dict(coarse=coarse_out, fine=fine_out, coarse_aux=coarse_aux, fine_aux=fine_aux), mask


def test_renderer_full_grid_equals_no_grid(renderer):
    """Every entry of the returned dict, for rays that hit the box (a ray that misses it is not evaluated with a grid,
    so its unused per-sample entries are zero instead of model values: the next test covers such rays)."""
    from learn_nerf.rng import Key

    batch = render_batch(hit_only=True)
    plain = renderer.render_rays(Key(11), batch)
    full = with_grid(renderer, np.ones((GRID_RES,) * 3, bool)).render_rays(Key(11), batch)
    assert set(full) == set(plain) == {"coarse", "fine", "coarse_aux", "fine_aux"}
    for level in ("coarse", "fine"):
        assert set(full[level]) == set(plain[level])
        for name in plain[level]:
            assert full[level][name].shape == plain[level][name].shape
            assert torch.equal(full[level][name], plain[level][name]), (level, name)
        assert same_aux(full[level + "_aux"], plain[level + "_aux"])
    assert (plain["fine"]["alphas"] > 0).any()


def test_renderer_random_grid_equals_the_uncompacted_pipeline(renderer):
    from learn_nerf.rng import Key

    batch = render_batch(hit_only=False)
    occ = np.random.default_rng(3).random((GRID_RES,) * 3) < 0.08
    clipped = with_grid(renderer, occ)
    got = clipped.render_rays(Key(12), batch)
    want, mask = uncompacted(renderer, clipped.occupancy, Key(12), batch)
    live = mask != 0
    plain = renderer.render_rays(Key(12), batch)
    box_mask = renderer.t_range(batch)[2]
    culled = box_mask & ~live
    assert 20 < int(live.sum()) < N_RAYS - 20 and int(culled.sum()) > 20 and int((~box_mask).sum()) > 5
    for level in ("coarse", "fine"):
        for name in ("outputs", "alphas", "coords"):  # what compositing returns: every ray
            assert torch.equal(got[level][name], want[level][name]), (level, name)
        for name in ("densities", "rgbs"):  # per sample: the evaluated rays, and zeros where nothing was evaluated
            assert got[level][name].shape == want[level][name].shape
            assert torch.equal(got[level][name][live], want[level][name][live]), (level, name)
            assert (got[level][name][~live] == 0).all()
        assert same_aux(got[level + "_aux"], want[level + "_aux"])
        assert list(got[level + "_aux"]) == list(renderer.coarse.AUX_NAMES)
        # a culled ray yields exactly what a ray that misses the box yields today
        assert (got[level]["outputs"][culled] == renderer.background).all()
        assert (got[level]["alphas"][culled] == 0).all() and (got[level]["coords"][culled] == 0).all()
        assert torch.equal(got[level]["outputs"][~box_mask], plain[level]["outputs"][~box_mask])


def test_renderer_empty_grid_is_all_background(renderer, monkeypatch):
    from learn_nerf.rng import Key

    batch = render_batch(hit_only=False)
    empty = with_grid(renderer, np.zeros((GRID_RES,) * 3, bool))

    def no_model(*args, **kwargs):
        raise AssertionError("a model ran although no ray is live")

    for model in {id(empty.coarse): empty.coarse, id(empty.fine): empty.fine}.values():
        monkeypatch.setattr(type(model), "forward_rays", no_model)
    out = empty.render_rays(Key(13), batch)
    for level in ("coarse", "fine"):
        t = TC if level == "coarse" else TC + TF
        assert (out[level]["outputs"] == renderer.background).all() and out[level]["outputs"].shape == (N_RAYS, 3)
        assert (out[level]["alphas"] == 0).all() and out[level]["alphas"].shape == (N_RAYS, 1)
        assert (out[level]["coords"] == 0).all()
        assert out[level]["densities"].shape == (N_RAYS, t) and not out[level]["densities"].any()
        assert out[level]["rgbs"].shape == (N_RAYS, t, 3) and not out[level]["rgbs"].any()
        assert list(out[level + "_aux"]) == list(renderer.coarse.AUX_NAMES)  # the keys of a run with live rays
        assert all(float(v) == 0.0 for v in out[level + "_aux"].values())


def test_grid_from_model_thresholds(renderer):
    """OccupancyGrid.from_renderer: threshold 0 is the full grid; the corner densities are mesh.density_grid's."""
    from learn_nerf import ops
    from learn_nerf.mesh import density_grid
    from learn_nerf.occupancy import OccupancyGrid, sigma_threshold

    full = OccupancyGrid.from_renderer(renderer, GRID_RES, threshold=0.0)
    assert full.occupied == GRID_RES ** 3 and full.sigma_thr == 0.0 and full.occupied_fraction == 1.0
    grid = OccupancyGrid.from_renderer(renderer, GRID_RES, threshold=0.3, dilate=0)
    sigma = density_grid(renderer.fine, renderer.fine_params, BMIN, BMAX, GRID_RES + 1, 1 << 18)
    thr = sigma_threshold(0.3, BMIN, BMAX, GRID_RES)
    assert abs(thr - (-np.log1p(-0.3) / (0.25 * np.sqrt(3)))) < 1e-12 and grid.sigma_thr == thr
    want_bits, want_count = R.build(sigma.cpu().numpy(), GRID_RES, thr, 0)
    assert torch.equal(grid.bits.cpu(), torch.from_numpy(want_bits.view(np.int32))) and grid.occupied == want_count
    assert ops.occ_build(sigma.reshape(-1), GRID_RES, thr, 0)[1] == want_count

"""
The dataset-diagnostic kernels (csrc/view_stats.hip) and their library layer (learn_nerf/diagnostics.py) on the GPU.

lnrf_sq_err_f64: S against math.fsum of the float64 terms under (3n + 1024 + 8) 2^-53 S — 3n terms per call, at most
1024 partials and 8 levels of the fold, every one a rounding of a partial sum of NON-NEGATIVE terms, hence <= 2^-53 S each;
any order of summation meets it.  ray_err: one rounding of a float64 value to fp32, 2^-24 relative.
lnrf_view_miss_stats: integers, so equality — with the kernel's own mask; the mask itself against the float64 reference
wherever the reference's |max_t - min_t| exceeds 1e-4 (two orders above the fp32 error of the three divisions).
"""
import ctypes
import math
import sys

import numpy as np
import pytest
import torch

import diagnostics_reference as DR

pytestmark = pytest.mark.gpu

U53, U24 = 2.0 ** -53, 2.0 ** -24
BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
LNRF_ERR_SHAPE = -2


def dev():
    return torch.device("cuda", 0)


def sum_bound(n, s):
    return (3 * n + 1024 + 8) * U53 * s


# ------------------------------------------------------------------------------------------------ lnrf_sq_err_f64

def sq_err_inputs(n, stride, seed=0):
    gen = torch.Generator().manual_seed(1000 * stride + n + seed)
    outputs = torch.rand(n, 3, generator=gen) * 2 - 1
    batch = torch.rand(n, stride // 3, 3, generator=gen) * 2 - 1
    targets = batch[:, -1]  # stride 9: the colour column of an [n, 3, 3] batch
    terms = ((outputs.double() - targets.double()) ** 2)
    return outputs.to(dev()), batch.to(dev())[:, -1], terms


def raw_sq_err(outputs, targets, acc, ray_err, fill=float("nan"), guard=16):
    """lnrf_sq_err_f64 through the C ABI with a scratch block the test owns: pre-filled, and followed by guard words
    that must come back untouched."""
    from learn_nerf import _lib as L

    n = outputs.shape[0]
    nbytes = L.lib().lnrf_sq_err_scratch_bytes(n)
    assert nbytes == min((n + 255) // 256, 1024) * 8
    scratch = torch.full((nbytes // 8 + guard,), fill, dtype=torch.float64, device=dev())
    rc = L.lib().lnrf_sq_err_f64(L.ptr(outputs), ctypes.c_void_p(targets.data_ptr()), targets.stride(0), n,
                                 L.ptr(ray_err), L.ptr(acc, torch.float64), ctypes.c_void_p(scratch.data_ptr()), nbytes,
                                 L.stream())
    assert rc == 0
    assert torch.isnan(scratch[nbytes // 8:]).all(), "wrote beyond its scratch"
    return acc


# 262,221 rays: more than 1024 workgroups' worth, so the grid-stride loop runs more than once
@pytest.mark.parametrize("stride", [3, 9])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000, 4097, 256 * 1024 + 77])
def test_sq_err_f64_against_fsum(n, stride):
    from learn_nerf import ops

    outputs, targets, terms = sq_err_inputs(n, stride)
    s_ref = math.fsum(terms.reshape(-1).tolist())
    acc = torch.tensor([-1.5, 0.0, 2.5], dtype=torch.float64, device=dev())
    ray_err = torch.full((n + 2,), -7.0, dtype=torch.float32, device=dev())
    raw_sq_err(outputs, targets, acc[1:2], ray_err[1:n + 1])
    got = acc.cpu()
    print(f"n={n} stride={stride}: S={got[1].item()!r} fsum={s_ref!r} |d|={abs(got[1].item() - s_ref):.3e} "
          f"bound={sum_bound(n, s_ref):.3e}")
    assert abs(got[1].item() - s_ref) <= sum_bound(n, s_ref)
    assert got[0].item() == -1.5 and got[2].item() == 2.5  # the neighbouring slots, bit for bit
    per_ray = terms.sum(dim=1)  # float64
    err = ray_err.cpu()
    assert err[0].item() == -7.0 and err[-1].item() == -7.0
    assert ((err[1:-1].double() - per_ray).abs() <= U24 * per_ray).all()
    # a second run, through the binding (its own uninitialised scratch): the same bits
    acc2 = torch.zeros(1, dtype=torch.float64, device=dev())
    ray_err2 = torch.empty(n, dtype=torch.float32, device=dev())
    ops.sq_err_f64_(outputs, targets, acc2, ray_err2)
    assert acc2.cpu()[0].item() == got[1].item() and torch.equal(ray_err2.cpu(), err[1:-1])
    # without ray_err: the same sum
    acc3 = torch.zeros(1, dtype=torch.float64, device=dev())
    ops.sq_err_f64_(outputs, targets, acc3)
    assert acc3.cpu()[0].item() == got[1].item()


def test_sq_err_f64_accumulates_and_leaves_an_empty_call_alone():
    from learn_nerf import _lib as L
    from learn_nerf import ops

    a_out, a_tgt, _ = sq_err_inputs(1000, 9, seed=1)
    b_out, b_tgt, _ = sq_err_inputs(257, 3, seed=2)
    single = torch.zeros(2, dtype=torch.float64, device=dev())
    raw_sq_err(a_out, a_tgt, single[0:1], None)
    raw_sq_err(b_out, b_tgt, single[1:2], None)
    both = torch.zeros(1, dtype=torch.float64, device=dev())
    raw_sq_err(a_out, a_tgt, both, None)
    raw_sq_err(b_out, b_tgt, both, None)
    sa, sb = single.cpu().tolist()
    assert sa > 0 and sb > 0 and both.cpu()[0].item() == sa + sb  # one fp64 addition per call
    # n == 0: through the binding and through the C ABI with null data pointers
    ops.sq_err_f64_(a_out[:0], a_tgt[:0], both)
    assert L.lib().lnrf_sq_err_f64(None, None, 3, 0, None, L.ptr(both, torch.float64), None, 0, L.stream()) == 0
    assert L.lib().lnrf_sq_err_scratch_bytes(0) == 0 and L.lib().lnrf_sq_err_scratch_bytes(-1) == -1
    assert both.cpu()[0].item() == sa + sb


def test_sq_err_f64_propagates_nan_and_inf():
    from learn_nerf import ops

    outputs, targets, _ = sq_err_inputs(300, 3)
    acc = torch.zeros(2, dtype=torch.float64, device=dev())
    with_inf = outputs.clone()
    with_inf[299, 1] = float("inf")
    ops.sq_err_f64_(with_inf, targets, acc[0:1])
    with_nan = outputs.clone()
    with_nan[0, 0] = float("nan")
    ops.sq_err_f64_(with_nan, targets, acc[1:2])
    got = acc.cpu()
    assert got[0].item() == float("inf") and math.isnan(got[1].item())


# ------------------------------------------------------------------------------------------- lnrf_view_miss_stats

# (width, height, camera seed): seeds picked on the CPU so that the float64 reference excludes at most 2 % of the rays
# and both hits and misses occur; 600 x 450 pixels need more than 1024 workgroups' worth (grid-stride loop)
VIEWS = [(37, 29, 1), (64, 64, 2), (1, 17, 103), (23, 1, 8), (600, 450, 5)]


def random_image(width, height, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(height, width, 3), dtype=np.uint8)


def raw_view_miss(view, image, box, stats, miss, guard=16):
    """lnrf_view_miss_stats through the C ABI with a scratch block of the test's, filled with 0xFF bytes."""
    from learn_nerf import _lib as L

    height, width = image.shape[:2]
    nbytes = L.lib().lnrf_view_miss_scratch_bytes(width, height)
    assert nbytes == min((width * height + 255) // 256, 1024) * 80
    scratch = torch.full((nbytes + 8 * guard,), 0xFF, dtype=torch.uint8, device=dev())
    rc = L.lib().lnrf_view_miss_stats(L.f3(view.camera_origin), L.f3(view.x_axis), L.f3(view.y_axis),
                                      L.f3(view.camera_direction), view.x_fov, view.y_fov, width, height,
                                      L.ptr(image, torch.uint8), L.f3(box[0]), L.f3(box[1]), 1e-3, 1e-8,
                                      L.ptr(miss, torch.uint8), L.ptr(stats, torch.int64),
                                      ctypes.c_void_p(scratch.data_ptr()), nbytes, L.stream())
    assert rc == 0
    assert (scratch[nbytes:] == 0xFF).all(), "wrote beyond its scratch"


def fresh_stats():
    return torch.from_numpy(DR.STATS_INIT.copy()).to(dev())


@pytest.mark.parametrize("width,height,seed", VIEWS)
def test_view_miss_stats_mask_and_reduction(width, height, seed):
    from learn_nerf import ops

    view = DR.camera_around(seed)
    image = random_image(width, height, seed)
    ref_miss, margin = DR.miss_reference(view, width, height, *BOX)
    decided = margin > 1e-4
    excluded = 1.0 - decided.mean()
    print(f"{width}x{height}: {int(ref_miss.sum())} of {ref_miss.size} rays miss, {excluded:.4%} within the margin")
    assert excluded <= 0.02 and 0 < ref_miss.sum() < ref_miss.size  # a property of the case, not of the kernel

    stats, miss = fresh_stats(), torch.full((width * height + 2,), 9, dtype=torch.uint8, device=dev())
    raw_view_miss(view, torch.from_numpy(image).to(dev()), BOX, stats, miss[1:-1])
    got_miss = miss.cpu().numpy()
    assert got_miss[0] == 9 and got_miss[-1] == 9 and set(np.unique(got_miss[1:-1])) <= {0, 1}
    got_miss = got_miss[1:-1].astype(bool)
    assert np.array_equal(got_miss[decided], ref_miss[decided])
    assert np.array_equal(stats.cpu().numpy(), DR.reduce_miss(image, got_miss))
    # through the binding, without the mask: the same words
    stats2 = fresh_stats()
    ops.view_miss_stats_(view, torch.from_numpy(image).to(dev()), *BOX, stats2)
    assert torch.equal(stats2, stats)
    # the same rays as the renderer's kernels see them (shared header): lnrf_camera_rays + lnrf_ray_aabb_stratified
    rays = view.bare_rays(width, height, device=dev())
    _, _, mask, _ = ops.ray_aabb_stratified(rays, *BOX, 0)
    assert np.array_equal(~mask.cpu().numpy().astype(bool), got_miss)


def test_view_miss_stats_all_hit_all_miss_and_three_views():
    from learn_nerf import ops

    width, height = 37, 29
    image = random_image(width, height, 11)
    image_dev = torch.from_numpy(image).to(dev())
    inside = DR.look_at((0.0, 0.3, 2.0), (0.0, 0.0, 0.0), 0.2, 0.2)  # sees only the box
    away = DR.look_at((0.0, 0.3, 2.0), (0.0, 0.6, 4.0), 0.9, 0.7)  # looks away from it
    for view in (inside, away):
        assert DR.miss_reference(view, width, height, *BOX)[1].min() > 1e-4
    assert not DR.miss_reference(inside, width, height, *BOX)[0].any()
    assert DR.miss_reference(away, width, height, *BOX)[0].all()

    stats, miss = fresh_stats(), torch.full((width * height,), 9, dtype=torch.uint8, device=dev())
    raw_view_miss(inside, image_dev, BOX, stats, miss)
    assert np.array_equal(stats.cpu().numpy(), DR.STATS_INIT) and not miss.any()  # count 0: the initial values stay
    raw_view_miss(away, image_dev, BOX, stats, miss)
    assert miss.all() and np.array_equal(stats.cpu().numpy(), DR.reduce_miss(image, np.ones(width * height, bool)))

    # three views of different sizes into one statistics tensor = the combined reduction
    stats, want = fresh_stats(), DR.STATS_INIT.copy()
    for w, h, seed in VIEWS[:3]:
        view, img = DR.camera_around(seed), random_image(w, h, seed + 20)
        miss = torch.empty(w * h, dtype=torch.uint8, device=dev())
        ops.view_miss_stats_(view, torch.from_numpy(img).to(dev()), *BOX, stats, miss=miss)
        want = DR.reduce_miss(img, miss.cpu().numpy().astype(bool), want)
    assert want[0] > 0 and np.array_equal(stats.cpu().numpy(), want)


def test_view_miss_stats_rejects_bad_shapes():
    from learn_nerf import _lib as L
    from learn_nerf import ops

    lib, view, stats = L.lib(), DR.camera_around(1), fresh_stats()
    word = torch.zeros(16, dtype=torch.uint8, device=dev())
    for width, height in ((0, 5), (5, 0), (-1, 3), (3, -2), (65536, 32768), (2 ** 31 - 1, 2)):
        assert lib.lnrf_view_miss_scratch_bytes(width, height) == -1
        rc = lib.lnrf_view_miss_stats(L.f3(view.camera_origin), L.f3(view.x_axis), L.f3(view.y_axis),
                                      L.f3(view.camera_direction), view.x_fov, view.y_fov, width, height,
                                      L.ptr(word, torch.uint8), L.f3(BOX[0]), L.f3(BOX[1]), 1e-3, 1e-8, None,
                                      L.ptr(stats, torch.int64), L.ptr(word, torch.uint8), 16, L.stream())
        assert rc == LNRF_ERR_SHAPE, (width, height, rc)
    assert lib.lnrf_view_miss_scratch_bytes(2 ** 31 - 1, 1) == 1024 * 80  # the largest view accepted
    with pytest.raises(RuntimeError, match="lnrf error -2"):
        ops.view_miss_stats_(view, torch.empty((0, 4, 3), dtype=torch.uint8, device=dev()), *BOX, stats)
    assert np.array_equal(stats.cpu().numpy(), DR.STATS_INIT)


# ---------------------------------------------------------------------------------------------- library layer

def test_device_colours_equal_the_host_division_for_every_byte():
    """px / 127.5 - 1 on the device is the IEEE fp32 division of the host path (NeRFView.rays), for all 256 values."""
    from learn_nerf.diagnostics import colored_rays

    pixels = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) % 256
    pixels = pixels.astype(np.uint8)
    view = DR.camera_around(7, cls=DR.ArrayView, pixels=pixels)
    got = colored_rays(view, torch.from_numpy(pixels).to(dev()))
    want = view.rays()
    assert torch.equal(got[:, 2].cpu(), want[:, 2])
    assert torch.equal(got[:, :2], view.bare_rays(16, 16, device=dev()))


@pytest.fixture(scope="module")
def validation_setup():
    from learn_nerf.dataset import ModelMetadata, NeRFDataset
    from learn_nerf.model import NeRFModel
    from learn_nerf.train import TrainLoop

    width, height = 16, 12
    views = [DR.camera_around(30 + i, radius=3.0, cls=DR.ArrayView, pixels=random_image(width, height, 40 + i),
                              image_path=f"view{i}") for i in range(2)]
    data = NeRFDataset(metadata=ModelMetadata((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), views=views)
    loop = TrainLoop(NeRFModel(), NeRFModel(), init_rng=0, lr=1e-3, coarse_ts=8, fine_ts=8)
    return data, loop, width, height


def test_validation_losses_against_float64_recomputation(validation_setup):
    from learn_nerf.diagnostics import validation_losses
    from learn_nerf.render import NeRFRenderer
    from learn_nerf.rng import Key, split

    data, loop, width, height = validation_setup
    batch_size, n = 100, width * height  # 192 rays: sub-batches of 100 and 92
    maps = []
    losses = list(validation_losses(Key(5), loop, data, batch_size, error_maps=maps))
    assert len(losses) == 2 and len(maps) == 2 and all(isinstance(x, float) for x in losses)

    params = loop.state.params
    renderer = NeRFRenderer(coarse=loop.coarse, fine=loop.fine, coarse_params=params["coarse"],
                            fine_params=params["fine"], background=params["background"], bbox_min=data.metadata.bbox_min,
                            bbox_max=data.metadata.bbox_max, coarse_ts=8, fine_ts=8)
    key = Key(5)
    for v, view in enumerate(data.views):
        geometry = view.bare_rays(width, height, device=dev())
        targets = view.rays()[:, 2]  # host colours: uint8 / 127.5 - 1 in NumPy
        terms = []
        for i in range(0, n, batch_size):
            test_key, key = split(key, 2)
            out = renderer.render_rays(split(test_key, 2)[0], geometry[i:i + batch_size].contiguous())
            terms.append((out["fine"]["outputs"].cpu().double() - targets[i:i + batch_size].double()) ** 2)
        terms = torch.cat(terms)
        s_ref = math.fsum(terms.reshape(-1).tolist())
        want = s_ref / (3 * n)
        bound = sum_bound(n, s_ref) / (3 * n)
        print(f"view {v}: loss={losses[v]!r} float64={want!r} |d|={abs(losses[v] - want):.3e} bound={bound:.3e}")
        assert want > 0 and abs(losses[v] - want) <= bound
        assert maps[v].shape == (height, width) and maps[v].dtype == torch.float32
        per_ray = terms.sum(dim=1)
        assert ((maps[v].cpu().reshape(-1).double() - per_ray).abs() <= U24 * per_ray).all()
        map_sum = math.fsum(maps[v].cpu().reshape(-1).tolist())
        assert abs(map_sum / (3 * n) - want) <= bound + U24 * want  # one fp32 rounding per ray on top
    # a second call: the same floats, bit for bit
    assert list(validation_losses(Key(5), loop, data, batch_size)) == losses
    assert list(validation_losses(Key(6), loop, data, batch_size)) != losses  # and they do depend on the key


def make_cube_dataset(directory, views, size, monkeypatch):
    from learn_nerf.scripts import make_cube_dataset as producer

    monkeypatch.setattr(sys, "argv", ["make_cube_dataset.py", "--views", str(views), "--size", str(size), str(directory)])
    producer.main()


def test_bbox_miss_stats_on_a_cube_dataset(tmp_path, monkeypatch):
    from learn_nerf.dataset import ModelMetadata, NeRFDataset, load_dataset
    from learn_nerf.diagnostics import bbox_miss_stats

    make_cube_dataset(tmp_path / "cube", 3, 16, monkeypatch)
    data = load_dataset(str(tmp_path / "cube"))
    assert len(data.views) == 3 and data.metadata.bbox_max == (1.0, 1.0, 1.0)

    def check(dataset):
        got, want = bbox_miss_stats(dataset, dev()), DR.bbox_stats_reference(dataset)
        assert got["count"] == want["count"] > 0
        assert np.array_equal(got["min"], want["min"]) and np.array_equal(got["max"], want["max"])
        assert got["mean"].dtype == np.float32
        assert (np.abs(got["mean"].astype(np.float64) - want["mean"]) <= np.spacing(np.abs(want["mean"]))).all()
        return got

    # every ray of these views meets the box of metadata.json, (-1 .. 1)^3: nothing to report
    assert DR.bbox_stats_reference(data)["count"] == 0
    assert bbox_miss_stats(data, dev()) == dict(count=0, min=None, max=None, mean=None)
    # shrunk to half its size, (-0.5 .. 0.5)^3, the box is the cube's own surface: rays miss it now, and all of them
    # see the black background
    half = check(NeRFDataset(metadata=ModelMetadata((-0.5,) * 3, (0.5,) * 3), views=data.views))
    assert half["max"].tolist() == [-1.0, -1.0, -1.0] and half["min"].tolist() == [-1.0, -1.0, -1.0]
    # halved once more it cuts the cube, and rays that pass the small box but hit the cube bring coloured pixels in:
    # the maximum moves, which is how the tool shows a box that cuts the object
    cut = check(NeRFDataset(metadata=ModelMetadata((-0.25,) * 3, (0.25,) * 3), views=data.views))
    assert cut["count"] > half["count"] and (cut["max"] > half["max"]).all()
    assert cut["min"].tolist() == [-1.0, -1.0, -1.0] and (cut["mean"] > -1.0).all()

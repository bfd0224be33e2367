"""
The SSIM kernel (csrc/image_metrics.hip, lnrf_ssim_f64) and the evaluation layer (learn_nerf/metrics.py) on the GPU,
against the float64 reference of tests/metrics_reference.py under ITS derived bounds (the docstring there): every map
entry within PER_ENTRY, no entry excluded, and the accumulated sum within sum_bound of math.fsum of the reference's
entries.  Reproducibility is equality of bits: across runs, across scratch contents, with and without a map.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import metrics_reference as MR

pytestmark = pytest.mark.gpu

TH, TW = 16, 32  # the kernel's tile of map entries (csrc/image_metrics.hip)
HALO = MR.TAPS - 1
LNRF_ERR_ARG, LNRF_ERR_SHAPE = -1, -2
GUARD = 16
SENTINEL = -7.0


def dev():
    return torch.device("cuda", 0)


def scratch_bytes_formula(width, height):
    tiles = 3 * -(-(height - HALO) // TH) * -(-(width - HALO) // TW)
    return min(tiles, 1024) * 8


def raw_ssim(a, b, acc, want_map=True):
    """lnrf_ssim_f64 through the C ABI with a scratch block the test owns — NaN-filled, followed by guard words that
    must come back untouched — and a map with sentinel entries on both sides.  -> the map on the host (or None)."""
    from learn_nerf import _lib as L

    height, width = a.shape[:2]
    nbytes = L.lib().lnrf_ssim_scratch_bytes(width, height)
    assert nbytes == scratch_bytes_formula(width, height)
    scratch = torch.full((nbytes // 8 + GUARD,), float("nan"), dtype=torch.float64, device=dev())
    entries = (height - HALO) * (width - HALO) * 3
    padded = torch.full((entries + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev()) if want_map else None
    map_ptr = ctypes.c_void_p(padded.data_ptr() + 8 * GUARD) if want_map else None
    rc = L.lib().lnrf_ssim_f64(L.ptr(a), L.ptr(b), width, height, map_ptr, L.ptr(acc, torch.float64),
                               ctypes.c_void_p(scratch.data_ptr()), nbytes, L.stream())
    assert rc == 0
    assert torch.isnan(scratch[nbytes // 8:]).all(), "wrote beyond its scratch"
    if not want_map:
        return None
    host = padded.cpu()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "wrote beyond its map"
    return host[GUARD:-GUARD].reshape(height - HALO, width - HALO, 3).numpy()


def on_device(*images):
    return [torch.from_numpy(x).to(dev()) for x in images]


def check_against_reference(a, b):
    """every check of one pair of host images; -> (sum, map) of the kernel"""
    from learn_nerf import ops

    height, width = a.shape[:2]
    ref = MR.ssim_map(a, b)
    entries = ref.size
    a_dev, b_dev = on_device(a, b)
    acc = torch.tensor([-1.5, 0.0, 2.5], dtype=torch.float64, device=dev())
    got_map = raw_ssim(a_dev, b_dev, acc[1:2])
    got = acc.cpu().tolist()
    assert got[0] == -1.5 and got[2] == 2.5  # the neighbouring slots, bit for bit
    err = np.abs(got_map - ref)
    s_ref, s_abs = MR.ssim_sum(ref), MR.ssim_sum(np.abs(ref))
    bound = MR.sum_bound(entries, s_abs)
    print(f"{width}x{height}: max entry |d|={err.max():.3e} bound={MR.PER_ENTRY:.3e}; sum={got[1]!r} fsum={s_ref!r} "
          f"|d|={abs(got[1] - s_ref):.3e} bound={bound:.3e}; min entry {ref.min():.4f}")
    assert got_map.shape == ref.shape and np.isfinite(got_map).all()
    assert (err <= MR.PER_ENTRY).all()  # every entry, none excluded
    assert abs(got[1] - s_ref) <= bound
    # a second run through the binding, with its own uninitialised scratch: the same bits
    acc2 = torch.zeros(1, dtype=torch.float64, device=dev())
    map2 = torch.empty((height - HALO, width - HALO, 3), dtype=torch.float64, device=dev())
    ops.ssim_f64_(a_dev, b_dev, acc2, map2)
    assert acc2.cpu()[0].item() == got[1] and np.array_equal(map2.cpu().numpy(), got_map)
    # without a map: the same sum
    acc3 = torch.zeros(1, dtype=torch.float64, device=dev())
    assert raw_ssim(a_dev, b_dev, acc3, want_map=False) is None
    acc4 = torch.zeros(1, dtype=torch.float64, device=dev())
    ops.ssim_f64_(a_dev, b_dev, acc4)
    assert acc3.cpu()[0].item() == got[1] and acc4.cpu()[0].item() == got[1]
    return got[1], got_map


# valid regions of 1, TH-1, TH, TH+1, 2TH+1 rows x 1, TW-1, TW, TW+1, 2TW+1 columns: every row count and every column
# count occurs, with every kind of input; not the full product
ROWS = (1, TH - 1, TH, TH + 1, 2 * TH + 1)
COLS = (1, TW - 1, TW, TW + 1, 2 * TW + 1)
CASES = [
    ("noise", ROWS[0], COLS[0]), ("near", ROWS[1], COLS[1]), ("dark", ROWS[2], COLS[2]), ("checker", ROWS[3], COLS[3]),
    ("noise", ROWS[4], COLS[4]), ("near", ROWS[0], COLS[4]), ("dark", ROWS[4], COLS[0]), ("checker", ROWS[2], COLS[3]),
    ("noise", ROWS[3], COLS[1]), ("near", ROWS[3], COLS[2]), ("dark", ROWS[1], COLS[3]), ("checker", ROWS[4], COLS[2]),
    ("checker", ROWS[0], COLS[1]), ("dark", ROWS[2], COLS[4]),
]


@pytest.mark.parametrize("kind,rows,cols", CASES)
def test_ssim_f64_against_the_float64_reference(kind, rows, cols):
    a, b = MR.image_pair(kind, rows + HALO, cols + HALO)
    if kind == "dark":
        assert max(a.max(), b.max()) <= 0.02
    _, got_map = check_against_reference(a, b)
    if kind == "checker" and rows > 3 and cols > 3:
        assert got_map.min() < 0  # negative SSIM occurs


def test_ssim_f64_on_800_x_800_runs_the_stride_loop():
    """3 * 50 * 25 = 3750 tiles on 1024 workgroups"""
    assert scratch_bytes_formula(800, 800) == 1024 * 8 and 3 * 50 * 25 > 1024
    a, b = MR.image_pair("near", 800, 800)
    total, _ = check_against_reference(a, b)
    assert 0.5 < total / (790 * 790 * 3) < 1.0


@pytest.mark.parametrize("rows,cols", [(1, 1), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1)])
def test_identical_images_give_one_everywhere(rows, cols):
    a, _ = MR.image_pair("same", rows + HALO, cols + HALO)
    (a_dev,) = on_device(a)
    acc = torch.zeros(1, dtype=torch.float64, device=dev())
    got_map = raw_ssim(a_dev, a_dev.clone(), acc)
    assert (np.abs(got_map - 1.0) <= MR.PER_ENTRY).all()
    entries = got_map.size
    assert abs(acc.cpu()[0].item() - entries) <= MR.sum_bound(entries, entries)


def test_two_calls_into_one_accumulator_add_in_fp64():
    a1, b1 = on_device(*MR.image_pair("noise", 30, 50))
    a2, b2 = on_device(*MR.image_pair("checker", 44, 21))
    single = torch.zeros(2, dtype=torch.float64, device=dev())
    raw_ssim(a1, b1, single[0:1], want_map=False)
    raw_ssim(a2, b2, single[1:2], want_map=False)
    both = torch.zeros(1, dtype=torch.float64, device=dev())
    raw_ssim(a1, b1, both, want_map=False)
    raw_ssim(a2, b2, both, want_map=False)
    s1, s2 = single.cpu().tolist()
    assert s1 > 0 > s2 and both.cpu()[0].item() == s1 + s2  # one fp64 addition per call


def test_ssim_f64_error_codes():
    from learn_nerf import _lib as L
    from learn_nerf import ops

    lib = L.lib()
    a, b = on_device(*MR.image_pair("noise", 12, 13))
    acc = torch.full((1,), 3.25, dtype=torch.float64, device=dev())
    nbytes = lib.lnrf_ssim_scratch_bytes(13, 12)
    scratch = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=dev())
    pa, pb, pacc, ps, stream = L.ptr(a), L.ptr(b), L.ptr(acc, torch.float64), scratch.data_ptr(), L.stream()
    for width, height in ((10, 11), (11, 10), (0, 12), (13, -1), (65536, 32768), (2 ** 31 - 1, 11)):
        assert lib.lnrf_ssim_scratch_bytes(width, height) == -1
        assert lib.lnrf_ssim_f64(pa, pb, width, height, None, pacc, ctypes.c_void_p(ps), nbytes, stream) == LNRF_ERR_SHAPE
    for args in ((None, pb, pacc, ps, nbytes), (pa, None, pacc, ps, nbytes), (pa, pb, None, ps, nbytes),
                 (pa, pb, pacc, None, nbytes), (pa, pb, pacc, ps, nbytes - 8), (pa, pb, pacc, ps + 4, nbytes)):
        x, y, z, s, n = args
        rc = lib.lnrf_ssim_f64(x, y, 13, 12, None, z, None if s is None else ctypes.c_void_p(s), n, stream)
        assert rc == LNRF_ERR_ARG, args
    assert b"lnrf_ssim_f64" in lib.lnrf_last_error()
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        ops.ssim_f64_(a[:10].contiguous(), b[:10].contiguous(), acc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ssim_f64_(a.cpu(), b.cpu(), acc)
    assert acc.cpu()[0].item() == 3.25  # no refused call touched it


def test_ssim_f64_propagates_nan():
    from learn_nerf import ops

    a, b = MR.image_pair("noise", 40, 60)
    a[20, 30, 1] = float("nan")
    a_dev, b_dev = on_device(a, b)
    acc = torch.zeros(1, dtype=torch.float64, device=dev())
    ssim_map = torch.empty((30, 50, 3), dtype=torch.float64, device=dev())
    ops.ssim_f64_(a_dev, b_dev, acc, ssim_map)
    assert math.isnan(acc.cpu()[0].item())
    nan = torch.isnan(ssim_map).cpu().numpy()
    want = np.zeros((30, 50, 3), dtype=bool)
    want[10:21, 20:31, 1] = True  # the entries whose window holds the pixel, in its channel only
    assert np.array_equal(nan, want)


# ---------------------------------------------------------------------------------------------- library layer

WIDTH, HEIGHT = 24, 20


@pytest.fixture(scope="module")
def cube_scene(tmp_path_factory):
    """three views of scripts/make_cube_dataset.py, their images cut to 24 x 20 (the producer writes squares; what a
    view shows is irrelevant here, its own size is not), and an untrained default model"""
    from PIL import Image

    from learn_nerf.dataset import load_dataset
    from learn_nerf.model import NeRFModel
    from learn_nerf.render import NeRFRenderer
    from learn_nerf.scripts import make_cube_dataset as producer
    from learn_nerf.train import TrainLoop

    directory = str(tmp_path_factory.mktemp("metrics") / "cube")
    argv, sys.argv = sys.argv, ["make_cube_dataset.py", "--views", "3", "--size", str(WIDTH), directory]
    try:
        producer.main()
    finally:
        sys.argv = argv
    for name in sorted(os.listdir(directory)):
        if name.endswith(".png"):
            path = os.path.join(directory, name)
            Image.fromarray(np.array(Image.open(path))[2:2 + HEIGHT]).save(path)
    data = load_dataset(directory)
    assert [np.asarray(v.image()).shape for v in data.views] == [(HEIGHT, WIDTH, 3)] * 3
    loop = TrainLoop(NeRFModel(), NeRFModel(), init_rng=0, lr=1e-3, coarse_ts=8, fine_ts=8)
    params = loop.state.params
    renderer = NeRFRenderer(coarse=loop.coarse, fine=loop.fine, coarse_params=params["coarse"],
                            fine_params=params["fine"], background=params["background"],
                            bbox_min=data.metadata.bbox_min, bbox_max=data.metadata.bbox_max, coarse_ts=8, fine_ts=8)
    return data, renderer


def test_evaluate_views_against_the_reference_on_its_own_renders(cube_scene):
    from learn_nerf.metrics import evaluate_views
    from learn_nerf.rng import Key

    data, renderer = cube_scene
    batch_size = 100  # 480 rays: four full slices and one of 80
    renders, maps = [], []
    results = list(evaluate_views(Key(5), renderer, data, batch_size, renders=renders, ssim_maps=maps))
    assert len(results) == len(renders) == len(maps) == 3
    assert [r["image_path"] for r in results] == [v.image_path for v in data.views]

    key = Key(5)
    for view, result, colors, ssim_map in zip(data.views, results, renders, maps):
        assert colors.shape == (HEIGHT, WIDTH, 3) and colors.dtype == torch.float32 and colors.is_cuda
        assert ssim_map.shape == (HEIGHT - HALO, WIDTH - HALO, 3) and ssim_map.dtype == torch.float64
        # the renders are those of RenderSession.render_view's key schedule, carried across the views
        rays = view.bare_rays(WIDTH, HEIGHT, device=dev())
        pieces = []
        for start in range(0, rays.shape[0], batch_size):
            key, slice_key = key.split(2)
            pieces.append(renderer.render_rays(slice_key, rays[start:start + batch_size].contiguous())["fine"]["outputs"])
        assert torch.equal(torch.cat(pieces).view(HEIGHT, WIDTH, 3), colors)

        prediction = MR.unit_prediction(colors.cpu().numpy())
        truth = MR.unit_image(np.asarray(view.image()))
        terms = MR.sq_err_terms(prediction, truth)
        s_ref = math.fsum(terms.reshape(-1).tolist())
        mse_ref = s_ref / terms.size
        mse_bound = MR.sq_err_bound(terms.size, s_ref) / terms.size + MR.U53 * mse_ref
        ref_map = MR.ssim_map(prediction, truth)
        ssim_ref = MR.ssim_sum(ref_map) / ref_map.size
        ssim_bound = MR.sum_bound(ref_map.size, MR.ssim_sum(np.abs(ref_map))) / ref_map.size + MR.U53 * abs(ssim_ref)
        print(f"{result['image_path']}: mse={result['mse']!r} ref={mse_ref!r} bound={mse_bound:.3e}; "
              f"ssim={result['ssim']!r} ref={ssim_ref!r} bound={ssim_bound:.3e}; psnr={result['psnr']!r}")
        assert mse_ref > 0 and abs(result["mse"] - mse_ref) <= mse_bound
        assert abs(result["ssim"] - ssim_ref) <= ssim_bound
        assert (np.abs(ssim_map.cpu().numpy() - ref_map) <= MR.PER_ENTRY).all()
        # psnr: the library's own mse through -10 log10 exactly; against the reference's, d(psnr) = 10 / ln 10 * d(mse) / mse
        assert result["psnr"] == MR.psnr_of_mse(result["mse"])
        psnr_bound = 10 / math.log(10) * (mse_bound / (mse_ref - mse_bound)) + 4 * MR.U53 * abs(MR.psnr_of_mse(mse_ref))
        assert abs(result["psnr"] - MR.psnr_of_mse(mse_ref)) <= psnr_bound

    # a second call with the same key: equal floats; another key: other renders
    assert list(evaluate_views(Key(5), renderer, data, batch_size)) == results
    assert list(evaluate_views(Key(6), renderer, data, batch_size)) != results

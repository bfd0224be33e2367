"""
CPU side of the image metrics (learn_nerf/metrics.py, scripts/eval_nerf.py, lnrf_ssim_f64): the float64 reference of
tests/metrics_reference.py against a direct 121-tap evaluation and closed forms; its derived bounds accept a correct
evaluation in another order and reject each wrong variant a port is likely to produce; the scratch query, the parser and
the size check of evaluate_views need no GPU.
"""
import math

import numpy as np
import pytest

import diagnostics_reference as DR
import metrics_reference as MR


def test_bounds_are_derived_and_of_the_expected_size():
    assert MR.E_MOMENT == (4 * MR.TAPS + 4) * MR.U53
    assert MR.E_FACTOR == 6 * MR.E_MOMENT + 8 * MR.U53
    assert 2 * MR.E_FACTOR / MR.C1 < MR.E_ENTRY < 1.2 * 2 * MR.E_FACTOR / MR.C1  # the C1 ratio dominates
    assert 1e-10 < MR.PER_ENTRY < 1e-8
    assert math.isclose(MR.window().sum(), 1.0, rel_tol=1e-15) and MR.window()[5] == MR.window().max()
    assert np.array_equal(MR.window(), MR.window()[::-1])


def test_separable_reference_equals_the_121_tap_brute_force():
    for kind in ("noise", "near", "checker"):
        a, b = MR.image_pair(kind, 13, 17)
        fast, slow = MR.ssim_map(a, b), MR.ssim_map_brute_force(a, b)
        assert fast.shape == slow.shape == (3, 7, 3) and fast.dtype == np.float64
        assert np.abs(fast - slow).max() <= 1e-14


def test_closed_forms():
    a, _ = MR.image_pair("noise", 19, 23)
    assert np.abs(MR.ssim_map(a, a) - 1.0).max() <= MR.PER_ENTRY and abs(MR.ssim(a, a) - 1.0) <= MR.PER_ENTRY
    for c1, c2 in ((0.25, 0.75), (0.0, 1.0), (0.5, 0.5), (0.0, 0.0), (0.015, 0.004)):
        x = np.full((12, 14, 3), c1, dtype=np.float32)
        y = np.full((12, 14, 3), c2, dtype=np.float32)
        f1, f2 = float(np.float32(c1)), float(np.float32(c2))
        want = (2 * f1 * f2 + MR.C1) / (f1 * f1 + f2 * f2 + MR.C1)
        assert np.abs(MR.ssim_map(x, y) - want).max() <= MR.PER_ENTRY
    # images that differ by a constant d: PSNR = -20 log10 d
    x = np.full((11, 12, 3), 0.25, dtype=np.float32)
    for d in (0.5, 0.125, 2.0 ** -10):
        assert math.isclose(MR.psnr(x, x + np.float32(d)), -20 * math.log10(d), rel_tol=1e-15)
    assert MR.psnr(x, x) == math.inf
    # the unit conversions, in fp32
    assert MR.unit_image(np.array([0, 51, 255], np.uint8)).tolist() == [0.0, float(np.float32(51) / np.float32(255)), 1.0]
    assert MR.unit_image(np.zeros(2, np.uint8)).dtype == np.float32
    assert MR.unit_prediction(np.array([-3.0, -1.0, 0.0, 0.5, 1.0, 7.0])).tolist() == [0.0, 0.0, 0.5, 0.75, 1.0, 1.0]


def accepts(got_map, got_sum, ref_map):
    """what tests/test_gpu_metrics.py asserts of the kernel"""
    if got_map.shape != ref_map.shape:
        return False
    entries = ref_map.size
    ok_map = bool((np.abs(got_map - ref_map) <= MR.PER_ENTRY).all())
    ok_sum = abs(got_sum - MR.ssim_sum(ref_map)) <= MR.sum_bound(entries, MR.ssim_sum(np.abs(ref_map)))
    return ok_map and ok_sum


def emulated_sum(values):
    """another fixed order: per-column running sums, highest row first, then the columns right to left"""
    total = 0.0
    for col in reversed(np.moveaxis(values, 1, 0).reshape(values.shape[1], -1).tolist()):
        part = 0.0
        for v in reversed(col):
            part += v
        total += part
    return total


PAIRS = [("noise", 40, 50), ("near", 40, 50), ("dark", 27, 43), ("checker", 33, 31)]


@pytest.mark.parametrize("kind,height,width", PAIRS)
def test_an_emulated_correct_kernel_passes_the_bounds(kind, height, width):
    a, b = MR.image_pair(kind, height, width)
    ref = MR.ssim_map(a, b)
    got = MR.ssim_map(a, b, vertical_first=True)  # taps applied columns first
    assert not np.array_equal(got, ref)  # a different evaluation, not a copy
    assert accepts(got, emulated_sum(got), ref)
    if kind == "checker":
        assert ref.max() < 0  # a pattern against its negative: every entry is negative


MUTATIONS = {
    "unnormalised window": dict(normalise=False),
    "sigma 1.0": dict(sigma=1.0),
    "C1 and C2 swapped": dict(c1=MR.C2, c2=MR.C1),
    "sample covariance": dict(sample_covariance=True),
    "fp32 moments": dict(moment_dtype=np.float32),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_each_seeded_mutation_is_rejected(name):
    for kind, height, width in PAIRS[:3]:
        a, b = MR.image_pair(kind, height, width)
        ref, got = MR.ssim_map(a, b), MR.ssim_map(a, b, **MUTATIONS[name])
        assert not accepts(got, MR.ssim_sum(got), ref), (name, kind)
        assert np.abs(got - ref).max() > MR.PER_ENTRY, (name, kind)


def test_zero_padded_same_region_is_rejected():
    a, b = MR.image_pair("noise", 40, 50)
    ref, got = MR.ssim_map(a, b), MR.ssim_map(a, b, pad_same=True)
    assert got.shape == (40, 50, 3) and not accepts(got, MR.ssim_sum(got), ref)
    # its interior is the valid map; what differs is the border, and with it the mean
    assert np.abs(got[5:-5, 5:-5] - ref).max() <= MR.PER_ENTRY
    assert abs(MR.ssim_sum(got) / got.size - MR.ssim_sum(ref) / ref.size) > MR.sum_bound(ref.size, ref.size) / ref.size


def test_clamped_central_moments_are_rejected_where_one_is_negative():
    # exact variances are never negative, so only the covariance can show a clamp: a checkerboard against its negative
    a, b = MR.image_pair("checker", 33, 31)
    x, y = a.astype(np.float64), b.astype(np.float64)
    taps = MR.window()
    s_xy = MR.filter_valid(x * y, taps) - MR.filter_valid(x, taps) * MR.filter_valid(y, taps)
    assert (s_xy < -1e-3).any()
    ref, got = MR.ssim_map(a, b), MR.ssim_map(a, b, clamp_moments=True)
    assert ref.min() < 0 <= got.min() and not accepts(got, MR.ssim_sum(got), ref)


def test_ssim_scratch_bytes_without_a_gpu():
    from learn_nerf import _lib

    lib = _lib.lib()
    th, tw = 16, 32  # the kernel's tile (csrc/image_metrics.hip)

    def want(width, height):
        tiles = 3 * -(-(height - 10) // th) * -(-(width - 10) // tw)
        return min(tiles, 1024) * 8

    for width, height in ((11, 11), (42, 26), (43, 26), (42, 27), (75, 43), (800, 800), (11, 4000), (4000, 11),
                          (46340, 46340)):
        assert lib.lnrf_ssim_scratch_bytes(width, height) == want(width, height), (width, height)
    assert lib.lnrf_ssim_scratch_bytes(11, 11) == 3 * 8 and lib.lnrf_ssim_scratch_bytes(800, 800) == 1024 * 8
    assert lib.lnrf_ssim_scratch_bytes(43, 27) == 3 * 2 * 2 * 8
    for width, height in ((10, 11), (11, 10), (0, 0), (-5, 20), (65536, 32768), (2 ** 31 - 1, 11)):
        assert lib.lnrf_ssim_scratch_bytes(width, height) == -1, (width, height)


def test_eval_nerf_parser_defaults():
    from learn_nerf.scripts import eval_nerf, render_nerf

    args = eval_nerf.build_parser().parse_args(["some/dir"])
    assert (args.seed, args.batch_size, args.coarse_samples, args.fine_samples) == (0, 1024, 64, 128)
    assert (args.model_path, args.output_dir, args.data_dir) == ("nerf.pkl", None, "some/dir")
    assert (args.occupancy_grid, args.occupancy_threshold, args.occupancy_dilate) == (0, 0.01, 1)
    assert args.instant_ngp is False and args.ref_nerf is False
    assert not hasattr(args, "width") and not hasattr(args, "height")  # a view is evaluated at its own size
    rendered = render_nerf.argparser().parse_args(["m.json"])
    for name in ("batch_size", "coarse_samples", "fine_samples", "model_path", "occupancy_grid",
                 "occupancy_threshold", "occupancy_dilate"):
        assert getattr(args, name) == getattr(rendered, name)
    args = eval_nerf.build_parser().parse_args(
        ["--seed", "3", "--batch_size", "64", "--coarse_samples", "8", "--fine_samples", "16", "--model_path", "m.pkl",
         "--occupancy_grid", "32", "--occupancy_threshold", "0.5", "--occupancy_dilate", "2", "--output_dir", "out",
         "--instant_ngp", "d"])
    assert (args.seed, args.batch_size, args.coarse_samples, args.fine_samples, args.model_path, args.occupancy_grid,
            args.occupancy_threshold, args.occupancy_dilate, args.output_dir, args.instant_ngp, args.data_dir) == (
        3, 64, 8, 16, "m.pkl", 32, 0.5, 2, "out", True, "d")
    with pytest.raises(SystemExit):
        eval_nerf.build_parser().parse_args([])


def test_eval_nerf_formats_lines_with_repr_and_means_with_fsum():
    from learn_nerf.scripts import eval_nerf

    results = [dict(image_path="a/0000.png", mse=0.01, psnr=20.0, ssim=0.1),
               dict(image_path="a/0001.png", mse=0.001, psnr=30.000000000000004, ssim=0.2),
               dict(image_path="a/0002.png", mse=0.1, psnr=10.0, ssim=0.3)]
    assert eval_nerf.format_view(results[1]) == "psnr=30.000000000000004 ssim=0.2 mse=0.001 a/0001.png"
    psnr = math.fsum([20.0, 30.000000000000004, 10.0]) / 3
    ssim = math.fsum([0.1, 0.2, 0.3]) / 3
    assert eval_nerf.format_mean(results) == f"mean: psnr={psnr!r} ssim={ssim!r} views=3"


def test_evaluate_views_refuses_a_ten_pixel_view_before_rendering():
    from learn_nerf.dataset import ModelMetadata, NeRFDataset
    from learn_nerf.metrics import evaluate_views

    class NoRenderer:
        def __getattr__(self, name):
            raise AssertionError(f"the renderer was touched ({name}) before the views were checked")

    def view(width, height, name):
        return DR.camera_around(3, cls=DR.ArrayView, pixels=np.zeros((height, width, 3), np.uint8), image_path=name)

    meta = ModelMetadata((-1.0,) * 3, (1.0,) * 3)
    for width, height in ((10, 24), (24, 10)):
        data = NeRFDataset(metadata=meta, views=[view(24, 20, "fine.png"), view(width, height, "small.png")])
        with pytest.raises(ValueError, match=r"small\.png.*" + f"{width} x {height}"):
            list(evaluate_views(0, NoRenderer(), data, 64))


def test_unit_conversions_of_the_library_equal_the_reference():
    import torch

    from learn_nerf.metrics import psnr_of_mse, unit_image, unit_prediction

    pixels = np.arange(256, dtype=np.uint8)
    assert np.array_equal(unit_image(torch.from_numpy(pixels)).numpy(), MR.unit_image(pixels))
    colors = np.random.default_rng(0).uniform(-1.5, 1.5, size=(500, 3)).astype(np.float32)
    got = unit_prediction(torch.from_numpy(colors))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), MR.unit_prediction(colors))
    assert psnr_of_mse(0.0) == math.inf and psnr_of_mse(0.01) == MR.psnr_of_mse(0.01) == 20.0


def test_ssim_binding_checks_shapes_before_it_needs_a_gpu():
    import torch

    from learn_nerf import ops

    acc = torch.zeros(1, dtype=torch.float64)
    image = torch.zeros(12, 12, 3)
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        ops.ssim_f64_(torch.zeros(10, 12, 3), torch.zeros(10, 12, 3), acc)
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        ops.ssim_f64_(torch.zeros(12, 10, 3), torch.zeros(12, 10, 3), acc)
    with pytest.raises(ValueError, match="one shape"):
        ops.ssim_f64_(image, torch.zeros(12, 13, 3), acc)
    with pytest.raises(ValueError, match="acc"):
        ops.ssim_f64_(image, image, torch.zeros(1))
    with pytest.raises(ValueError, match="ssim_map"):
        ops.ssim_f64_(image, image, acc, torch.zeros(2, 2, 4, dtype=torch.float64))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.ssim_f64_(image, image, acc)

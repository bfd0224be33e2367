"""
CPU side of the dataset diagnostics (learn_nerf/diagnostics.py, scripts/cv_nerf.py, scripts/check_bbox.py): the fold
dealer against hand-written cases, the float64 reference statistics of tests/diagnostics_reference.py on a 2 x 2 view
whose answer is written out, and the two command lines against the reference's flags and defaults.
"""
import math

import numpy as np
import pytest

import diagnostics_reference as DR


def test_chunk_indices_sizes_order_and_coverage():
    from learn_nerf.diagnostics import chunk_indices

    indices = [7, 3, 9, 0, 4, 8, 1, 6, 2, 5]
    chunks = list(chunk_indices(3, indices))
    assert [len(c) for c in chunks] == [4, 3, 3]
    assert chunks == [{7, 3, 9, 0}, {4, 8, 1}, {6, 2, 5}]  # dealt in the order given
    assert sorted(i for c in chunks for i in c) == sorted(indices) and sum(len(c) for c in chunks) == 10
    # more chunks than indices: the empty ones are not produced
    assert list(chunk_indices(5, [4, 2])) == [{4}, {2}]
    assert list(chunk_indices(1, [1, 2, 3])) == [{1, 2, 3}]
    assert list(chunk_indices(4, [0, 1, 2, 3])) == [{0}, {1}, {2}, {3}]
    assert list(chunk_indices(3, [])) == []
    for n, k in ((10, 10), (11, 4), (6, 2), (3, 7)):
        chunks = list(chunk_indices(k, list(range(n))))
        sizes = [len(c) for c in chunks]
        assert len(chunks) == min(n, k) and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
        assert [i for c in chunks for i in sorted(c)] == list(range(n))


def two_by_two():
    # at the origin of a box that only the right-hand image column can see: tan(fov / 2) = 1, so the four rays leave
    # (0, 0, 3) along (-1 | +1, -1 | +1, -1) / sqrt(3) and pass z = 1 .. -1 at x = -+2 .. -+4, |y| = 2 .. 4
    view = DR.ArrayView(camera_direction=(0.0, 0.0, -1.0), camera_origin=(0.0, 0.0, 3.0), x_axis=(1.0, 0.0, 0.0),
                        y_axis=(0.0, -1.0, 0.0), x_fov=math.pi / 2, y_fov=math.pi / 2,
                        pixels=np.array([[[10, 20, 30], [1, 2, 3]], [[50, 5, 250], [4, 5, 6]]], dtype=np.uint8))
    return view, (0.5, -3.0, -1.0), (3.0, 3.0, 1.0)


def test_reference_statistics_on_a_two_by_two_view():
    view, lo, hi = two_by_two()
    rays = DR.bare_rays_f64(view, 2, 2)
    s = 1 / math.sqrt(3)
    assert np.allclose(rays[:, 0], [0, 0, 3])
    assert np.allclose(rays[:, 1], [[-s, s, -s], [s, s, -s], [-s, -s, -s], [s, -s, -s]])
    miss, margin = DR.miss_reference(view, 2, 2, lo, hi)
    assert miss.tolist() == [True, False, True, False]  # raster order: the left column misses
    # the right column enters at z = 1 (t = 2 sqrt 3) and leaves through x = 3 (t = 3 sqrt 3)
    assert np.allclose(margin[[1, 3]], math.sqrt(3), rtol=1e-6)
    stats = DR.reduce_miss(view.pixels, miss)
    assert stats.tolist() == [2, 60, 25, 280, 10, 5, 30, 50, 20, 250]
    colors = DR.colors_of_stats(stats)
    assert colors["count"] == 2 and all(colors[k].dtype == np.float32 for k in ("min", "max", "mean"))
    assert np.allclose(colors["min"], [-0.92156863, -0.96078431, -0.76470588], atol=1e-7)
    assert np.allclose(colors["max"], [-0.60784314, -0.84313725, 0.96078431], atol=1e-7)
    assert np.allclose(colors["mean"], [-0.76470588, -0.90196078, 0.09803922], atol=1e-7)
    # a second view into the same words, and the whole-dataset form
    again = DR.reduce_miss(np.full((2, 2, 3), 7, dtype=np.uint8), [False, False, False, True], stats)
    assert again.tolist() == [3, 67, 32, 287, 7, 5, 7, 50, 20, 250]

    class Meta:
        bbox_min, bbox_max = lo, hi

    class Data:
        metadata, views = Meta, [view, view]

    both = DR.bbox_stats_reference(Data)
    assert both["count"] == 4
    assert np.array_equal(both["mean"], colors["mean"]) and np.array_equal(both["max"], colors["max"])
    # a box that every ray hits: nothing to report
    nothing = DR.bbox_stats_reference(Data, (-9.0, -9.0, -1.0), (9.0, 9.0, 1.0))
    assert nothing == dict(count=0, min=None, max=None, mean=None)


def test_width_or_height_of_one_sits_at_the_minus_one_end():
    view, _, _ = two_by_two()
    s = 1 / math.sqrt(3)
    assert np.allclose(DR.bare_rays_f64(view, 1, 2)[:, 1], [[-s, s, -s], [-s, -s, -s]])
    assert np.allclose(DR.bare_rays_f64(view, 2, 1)[:, 1], [[-s, s, -s], [s, s, -s]])


def test_cv_nerf_parser_has_the_reference_flags_and_defaults():
    from learn_nerf.scripts import cv_nerf

    args = cv_nerf.build_parser().parse_args(["some/dir"])
    assert (args.seed, args.lr, args.batch_size, args.folds) == (0, 1e-4, 4096, 10)
    assert (args.coarse_samples, args.fine_samples, args.train_iters) == (64, 128, 1500)
    assert args.instant_ngp is False and args.ref_nerf is False and args.data_dir == "some/dir"
    assert args.error_map_dir is None  # the additive flag is off by default
    args = cv_nerf.build_parser().parse_args(
        ["--seed", "5", "--lr", "3e-4", "--batch_size", "128", "--folds", "3", "--coarse_samples", "16",
         "--fine_samples", "32", "--train_iters", "7", "--instant_ngp", "--ref_nerf", "--error_map_dir", "maps", "d"])
    assert (args.seed, args.lr, args.batch_size, args.folds, args.coarse_samples, args.fine_samples, args.train_iters,
            args.instant_ngp, args.ref_nerf, args.error_map_dir) == (5, 3e-4, 128, 3, 16, 32, 7, True, True, "maps")
    with pytest.raises(SystemExit):
        cv_nerf.build_parser().parse_args([])  # data_dir is required


def test_check_bbox_parser_takes_the_data_dir_only():
    from learn_nerf.scripts import check_bbox

    assert check_bbox.build_parser().parse_args(["some/dir"]).data_dir == "some/dir"
    with pytest.raises(SystemExit):
        check_bbox.build_parser().parse_args([])
    with pytest.raises(SystemExit):
        check_bbox.build_parser().parse_args(["a", "b"])

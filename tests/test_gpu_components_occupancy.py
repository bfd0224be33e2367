"""
OccupancyGrid.filtered on the GPU: the bits of a grid built by lnrf_occ_build from synthetic corner densities, filtered
by component size, equal the pack of the restatement's keep mask (tests/components_reference.py on the unpacked bits of
tests/occupancy_reference.py); the filtered grid clips rays like the restatement's clip on those bits; and the flags of
the rendering commands leave the output alone at their defaults.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import components_reference as C
import mesh_reference as M
import occupancy_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "learn-nerf_amd")
RES, THR = 13, 1.0  # 2197 cells: 69 words, the last one partly used


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def corner_densities() -> np.ndarray:
    """(RES + 1)^3 corner densities: one object, three floaters of different sizes apart from it, and a floater whose
    dilated cells touch the object's only at a corner."""
    s = np.zeros((RES + 1,) * 3, np.float32)
    s[2:6, 2:6, 2:6] = 2.0      # the object
    s[10, 10, 2] = 3.0          # floaters
    s[10:12, 2, 10] = 3.0
    s[2, 11, 11] = np.inf
    s[9, 9, 9] = 5.0            # cells 7..10 after dilation: they meet the object's (0..6) at the corner of (6, 6, 6) only
    return s


@pytest.fixture(scope="module")
def grids():
    from learn_nerf import ops
    from learn_nerf.occupancy import OccupancyGrid

    sigma = corner_densities()
    bits, occupied = ops.occ_build(cuda(sigma).reshape(-1), RES, THR, 1)
    want_bits, want_count = R.build(sigma, RES, THR, 1)
    assert torch.equal(bits.cpu(), torch.from_numpy(want_bits.view(np.int32))) and occupied == want_count
    grid = OccupancyGrid(bits=bits, resolution=RES, bbox_min=R.BOX_MIN, bbox_max=R.BOX_MAX, sigma_thr=THR,
                         occupied=occupied)
    return grid, R.unpack_bits(want_bits, RES)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_filtered_equals_the_pack_of_the_reference_keep_mask(grids, connectivity):
    grid, occ = grids
    lab = C.label(occ, connectivity)
    size = C.sizes(lab)
    assert np.count_nonzero(size) >= 4
    assert torch.equal(grid.cell_mask().cpu(), torch.from_numpy(occ.astype(np.uint8)))
    second = C.ranked(size)[1][1]
    for min_cells, keep_largest in ((1, None), (second, None), (second + 1, None), (1, 1), (1, 2), (2, 3)):
        keep = C.keep(lab, size, min_cells, keep_largest)
        got = grid.filtered(min_cells=min_cells, keep_largest=keep_largest, connectivity=connectivity)
        assert got.bits.dtype == torch.int32 and got.bits.shape == grid.bits.shape
        assert torch.equal(got.bits.cpu(), torch.from_numpy(R.pack_bits(keep).view(np.int32))), (min_cells, keep_largest)
        assert got.occupied == int(keep.sum()) == R.popcount(got.bits.cpu().numpy().view(np.uint32))
        assert (got.resolution, got.bbox_min, got.bbox_max, got.sigma_thr) == (RES, R.BOX_MIN, R.BOX_MAX, THR)
    same = grid.filtered()
    assert torch.equal(same.bits, grid.bits) and same.occupied == grid.occupied and same.bits is not grid.bits


def test_clip_on_the_filtered_grid_equals_the_restatement(grids):
    grid, occ = grids
    lab = C.label(occ, 26)
    keep = C.keep(lab, C.sizes(lab), keep_largest=1)
    assert 0 < keep.sum() < occ.sum()
    rays = R.make_rays(600, RES, seed=4)
    t_min, t_max, mask = R.box_range(rays, R.BOX_MIN, R.BOX_MAX)
    want = R.clip(rays, R.BOX_MIN, R.BOX_MAX, RES, R.pack_bits(keep), t_min, t_max, mask)
    before = R.clip(rays, R.BOX_MIN, R.BOX_MAX, RES, R.pack_bits(occ), t_min, t_max, mask)
    assert want[2].sum() < before[2].sum(), "the floaters were keeping some rays alive"
    got = grid.filtered(keep_largest=1).clip(cuda(rays), cuda(t_min), cuda(t_max), cuda(mask))
    for g, w in zip(got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert torch.equal(g.cpu().view(torch.int32) if w.dtype == torch.float32 else g.cpu(),
                           w.view(torch.int32) if w.dtype == torch.float32 else w)


BOX = ((-1.5, -1.5, -1.5), (6.0, 1.5, 1.5))  # one whole blob of the analytic field and one cut by the face x = 6
GRID = 16


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from learn_nerf.dataset import CameraView
    from learn_nerf.model import NeRFModel
    from learn_nerf.train import TrainLoop

    d = tmp_path_factory.mktemp("components_occupancy_cli")
    loop = TrainLoop(NeRFModel(), NeRFModel(), init_rng=0, lr=1e-3, coarse_ts=8, fine_ts=8)
    with torch.no_grad():
        M.set_analytic_nerf(loop.state.params["fine"])
    ckpt, meta, view = str(d / "nerf.pkl"), str(d / "metadata.json"), str(d / "view.json")
    loop.save(ckpt)
    with open(meta, "w") as fh:
        json.dump({"min": list(BOX[0]), "max": list(BOX[1])}, fh)
    with open(view, "w") as fh:
        fh.write(CameraView(camera_direction=(0.0, 0.0, -1.0), camera_origin=(2.0, 0.0, 5.0), x_axis=(1.0, 0.0, 0.0),
                            y_axis=(0.0, -1.0, 0.0), x_fov=1.2, y_fov=0.6).to_json())
    return d, ckpt, meta, view


def render(scene, name, *flags):
    """-> (the PNG's bytes, the occupied count of the command's `occupancy grid` line); no dilation, so that the two
    empty cells between the blobs stay empty."""
    d, ckpt, meta, view = scene
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    png = str(d / f"{name}.png")
    res = subprocess.run([sys.executable, os.path.join(PKG, "learn_nerf", "scripts", "render_nerf.py"), "--width", "24",
                          "--height", "12", "--seed", "0", "--batch_size", "100", "--coarse_samples", "8",
                          "--fine_samples", "8", "--model_path", ckpt, "--occupancy_grid", str(GRID),
                          "--occupancy_dilate", "0", *flags, meta, view, png],
                         env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith(f"occupancy grid {GRID}^3: ")]
    assert len(line) == 1
    return open(png, "rb").read(), int(line[0].split()[3])


def test_render_command_with_the_default_filter_writes_the_same_png(scene):
    assert render(scene, "grid") == render(scene, "default", "--occupancy_min_component", "1")


def test_render_command_passes_the_filter_flags_on(scene):
    from learn_nerf.model import NeRFModel
    from learn_nerf.occupancy import OccupancyGrid
    from learn_nerf.train import load_params

    _, ckpt, _, _ = scene
    fine = NeRFModel()
    params = load_params(ckpt, NeRFModel(), fine, torch.device("cuda", 0))["fine"]
    whole = OccupancyGrid.from_model(fine, params, *BOX, GRID, dilate=0)
    largest = OccupancyGrid.from_model(fine, params, *BOX, GRID, dilate=0, keep_largest=1, connectivity=6)
    assert 0 < largest.occupied < whole.occupied
    assert torch.equal(largest.bits, whole.filtered(keep_largest=1, connectivity=6).bits)
    _, count = render(scene, "largest", "--occupancy_keep_largest", "1", "--occupancy_connectivity", "6")
    assert count == largest.occupied

"""
learn_nerf.metrics — image quality of a checkpoint on a dataset: PSNR and SSIM per view (scripts/eval_nerf.py).

Built like learn_nerf.diagnostics: a view's rays come from lnrf_camera_rays, its prediction and its ground truth stay on
the device as whole images, and both reductions run in fp64 in a fixed order — PSNR from lnrf_sq_err_f64, SSIM from
lnrf_ssim_f64 (csrc/image_metrics.hip) — into one float64 slot per view, read back ONCE for the whole dataset.  Two runs
with one key print the same digits.

Unit images.  Both metrics compare fp32 [H, W, 3] images with values in [0, 1]: the ground truth is byte / 255, the
prediction is clamp((c + 1) / 2, 0, 1) of the fine model's colours c in [-1, 1] — what an image file can hold.

  PSNR = -10 log10(mse), mse = sum((a - b)^2) / (3 H W); the logarithm is taken on the host in float64, inf for mse 0.
  SSIM = the mean over all entries of all three channels of the structural similarity map of Wang et al. 2004 with an
         11 x 11 Gaussian window of sigma 1.5, valid region only ([H - 10, W - 10, 3]), population moments, C1 = 0.01^2,
         C2 = 0.03^2 — what skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5,
         use_sample_covariance=False, data_range=1, channel_axis=-1) computes (skimage is not a dependency).
"""
import math
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from . import ops
from .dataset import NeRFDataset
from .diagnostics import _upload_image
from .render import NeRFRenderer
from .rng import KeyLike, as_key

F32 = torch.float32
WINDOW = ops.SSIM_WINDOW


def unit_prediction(colors: torch.Tensor) -> torch.Tensor:
    """The package's colours in [-1, 1] -> [0, 1]: clamp((c + 1) * 0.5, 0, 1), in the dtype of `colors`."""
    return ((colors + 1) * 0.5).clamp(0, 1)


def unit_image(image_u8: torch.Tensor) -> torch.Tensor:
    """uint8 pixels -> fp32 byte / 255 with a true fp32 division: the divisor is a device tensor, for the reason given
    in diagnostics.colored_rays (a division by a Python number becomes a multiplication by its reciprocal)."""
    scale = torch.full((), 255.0, dtype=F32, device=image_u8.device)
    return torch.div(image_u8.to(F32), scale)


def psnr_of_mse(mse: float) -> float:
    """-10 log10(mse) in float64; inf for mse == 0."""
    return math.inf if mse == 0 else -10.0 * math.log10(mse)


def ssim_map_image(ssim_map: torch.Tensor) -> np.ndarray:
    """[H - 10, W - 10, 3] SSIM map -> uint8 grey image of its channel mean: clamp to [0, 1], times 255, rounded."""
    return (ssim_map.mean(dim=2).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()


def evaluate_views(key: KeyLike, renderer: NeRFRenderer, data: NeRFDataset, batch_size: int,
                   renders: Optional[list] = None, ssim_maps: Optional[list] = None) -> Iterator[Dict[str, object]]:
    """
    PSNR and SSIM of the renderer's fine output on every view of `data`: yields dict(image_path, mse, psnr, ssim) per
    view, in dataset order.  Each view is rendered at its own image size from view.bare_rays(device=) in slices of
    batch_size rays, keys split per slice as RenderSession.render_view does (`key, slice_key = key.split(2)`) and
    carried across the views.  The squared error and the SSIM sum of view v go into slot v of two float64 device
    tensors; nothing of this function waits for the device inside a view, and the whole call reads back once, so every
    view is evaluated before the first dict is produced.  renders (a list) receives the [H, W, 3] fp32 device
    predictions in [-1, 1], ssim_maps (a list) the float64 [H - 10, W - 10, 3] device maps.
    A view under 11 pixels in either dimension has no SSIM: ValueError naming it, before anything is rendered.
    """
    shapes = []
    for view in data.views:
        height, width = np.asarray(view.image()).shape[:2]
        if height < WINDOW or width < WINDOW:
            raise ValueError(f"{getattr(view, 'image_path', view)}: a view of {width} x {height} pixels is smaller "
                             f"than the {WINDOW} x {WINDOW} SSIM window")
        shapes.append((height, width))
    key = as_key(key)
    device = renderer.background.device
    slots = max(len(data.views), 1)
    sq_acc = torch.zeros(slots, dtype=torch.float64, device=device)
    ssim_acc = torch.zeros(slots, dtype=torch.float64, device=device)
    for v, (view, (height, width)) in enumerate(zip(data.views, shapes)):
        truth = unit_image(_upload_image(view, device))
        rays = view.bare_rays(width, height, device=device)
        pieces = []
        for start in range(0, rays.shape[0], batch_size):
            key, slice_key = key.split(2)
            pieces.append(renderer.render_rays(slice_key, rays[start:start + batch_size].contiguous())["fine"]["outputs"])
        colors = torch.cat(pieces, dim=0).view(height, width, 3)
        prediction = unit_prediction(colors)
        ops.sq_err_f64_(prediction.view(-1, 3), truth.view(-1, 3), sq_acc[v:v + 1])
        ssim_map = None
        if ssim_maps is not None:
            ssim_map = torch.empty((height - WINDOW + 1, width - WINDOW + 1, 3), dtype=torch.float64, device=device)
            ssim_maps.append(ssim_map)
        ops.ssim_f64_(prediction, truth, ssim_acc[v:v + 1], ssim_map)
        if renders is not None:
            renders.append(colors)
    sums = torch.stack([sq_acc, ssim_acc]).cpu().tolist()  # the one read-back
    for view, (height, width), sq, ss in zip(data.views, shapes, *sums):
        mse = sq / (3 * height * width)
        yield dict(image_path=getattr(view, "image_path", None), mse=mse, psnr=psnr_of_mse(mse),
                   ssim=ss / (3 * (height - WINDOW + 1) * (width - WINDOW + 1)))

"""
learn_nerf.diagnostics — is a dataset fit to train on?  The library side of the reference's scripts/cv_nerf.py (K-fold
cross-validation: the held-out views with the highest loss probably have a wrong camera pose) and scripts/check_bbox.py
(the pixels whose rays miss the scene box should all be background; anything else means the box cuts the object).

Both do per-pixel work over whole views, and both keep it on the device: the uint8 image of a view is uploaded once, its
rays come from lnrf_camera_rays, and the two reductions are the fixed-order kernels of csrc/view_stats.hip
(lnrf_sq_err_f64, lnrf_view_miss_stats) — a tool whose output is a ranking of views prints the same digits on every run,
and a fold (or a dataset) costs ONE read-back.
"""
import random
import tempfile
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Set, Tuple

import numpy as np
import torch

from . import ops
from .dataset import NeRFDataset
from .render import NeRFRenderer
from .rng import Key, KeyLike, as_key, split

F32 = torch.float32


def chunk_indices(num_chunks: int, indices: List[int]) -> Iterator[Set[int]]:
    """Deal `indices`, in order, into num_chunks sets whose sizes differ by at most one, the larger ones first; with
    more chunks than indices the empty ones are not produced (scripts/cv_nerf.py:119-132)."""
    chunk_size, extra = divmod(len(indices), num_chunks)
    offset = 0
    for i in range(num_chunks):
        size = chunk_size + 1 if i < extra else chunk_size
        if not size:
            return
        yield set(indices[offset:offset + size])
        offset += size
    assert offset == len(indices)


def colored_rays(view, image_u8: torch.Tensor) -> torch.Tensor:
    """NeRFView.rays() (dataset.py:89-101) made on the device of image_u8 (uint8 [H, W, 3]): [H*W, 3, 3] rows of
    (origin, direction, colour).  The colour is px / 127.5 - 1 with a true fp32 division: the divisor is a device
    tensor, because torch turns a division by a Python number into a multiplication by its reciprocal, which differs
    from the reference's (and the host path's) colours in the last bit for some of the 256 values."""
    height, width = int(image_u8.shape[0]), int(image_u8.shape[1])
    device = image_u8.device
    out = torch.empty((height * width, 3, 3), dtype=F32, device=device)
    out[:, :2] = view.bare_rays(width, height, device=device)
    scale = torch.full((), 127.5, dtype=F32, device=device)
    out[:, 2] = torch.div(image_u8.reshape(-1, 3).to(F32), scale) - 1
    return out


def _upload_image(view, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(view.image(), dtype=np.uint8)).to(device)


def validation_losses(key: KeyLike, loop, data: NeRFDataset, batch_size: int,
                      error_maps: Optional[list] = None) -> Iterator[float]:
    """
    The fine model's mean squared error on every view of `data` under the loop's current parameters, one float per view
    (scripts/cv_nerf.py:96-116).  Keys as in the reference: `test_key, key = split(key)` per sub-batch, carried across
    the views.  Each sub-batch of batch_size rays is rendered by NeRFRenderer.render_rays (no backward: the
    split-precision kernels, this package's closest to the reference's fp32 evaluation) with the key that
    TrainLoop.losses would derive (split(test_key, 2)[0]), and its fine outputs go through lnrf_sq_err_f64 into slot v
    of one float64 device tensor: loss(v) = acc[v] / (3 H W), summed in fp64 and in a fixed order.  Nothing inside a view
    waits for the device and the whole call reads back once, so all views are evaluated before the first float is
    produced.  error_maps (a list) receives one [H, W] fp32 device tensor per view: the squared error of each ray, summed
    over the three channels.
    """
    device = loop.device
    params = loop.state.params
    renderer = NeRFRenderer(coarse=loop.coarse, fine=loop.fine, coarse_params=params["coarse"],
                            fine_params=params["fine"], background=params["background"],
                            bbox_min=data.metadata.bbox_min, bbox_max=data.metadata.bbox_max,
                            coarse_ts=loop.coarse_ts, fine_ts=loop.fine_ts)
    key = as_key(key)
    acc = torch.zeros(max(len(data.views), 1), dtype=torch.float64, device=device)
    pixels = []
    for v, view in enumerate(data.views):
        image = _upload_image(view, device)
        rays = colored_rays(view, image)
        total = rays.shape[0]
        ray_err = torch.empty(total, dtype=F32, device=device) if error_maps is not None else None
        for i in range(0, total, batch_size):
            test_key, key = split(key, 2)
            sub_batch = rays[i:i + batch_size]
            render_key = split(test_key, 2)[0]  # train.py:137
            outputs = renderer.render_rays(render_key, sub_batch)["fine"]["outputs"]
            ops.sq_err_f64_(outputs, sub_batch[:, 2], acc[v:v + 1],
                            None if ray_err is None else ray_err[i:i + sub_batch.shape[0]])
        if error_maps is not None:
            error_maps.append(ray_err.view(image.shape[0], image.shape[1]))
        pixels.append(total)
    sums = acc.cpu().tolist()  # the one read-back
    for total, s in zip(pixels, sums):
        yield s / (3 * total)


_STATS_INIT = (0, 0, 0, 0, 255, 255, 255, 0, 0, 0)  # count, sums, minima, maxima (lnrf_view_miss_stats)


def bbox_miss_stats(data: NeRFDataset, device, progress: Callable[[Iterable], Iterable] = iter) -> Dict[str, object]:
    """
    min / max / mean colour of the pixels whose rays miss the scene box, over every view of `data`
    (scripts/check_bbox.py:27-50), and their count.  lnrf_view_miss_stats combines the uint8 pixels of every view into
    one int64 statistics tensor, read back once.  min and max are the float32 colours k / 127.5 - 1 of the extreme bytes
    (the map is monotone, so it commutes with min / max); mean is (sum / count) / 127.5 - 1 evaluated in float64 and
    rounded to float32.  With no missing ray the three are None (the reference divides by zero there).
    """
    stats = torch.tensor(_STATS_INIT, dtype=torch.int64, device=device)
    for view in progress(data.views):
        ops.view_miss_stats_(view, _upload_image(view, device), data.metadata.bbox_min, data.metadata.bbox_max, stats)
    words = stats.cpu().numpy()
    count = int(words[0])
    if count == 0:
        return dict(count=0, min=None, max=None, mean=None)
    f32 = np.float32
    low, high = (words[a:a + 3].astype(f32) / f32(127.5) - f32(1) for a in (4, 7))
    mean = ((words[1:4].astype(np.float64) / count) / 127.5 - 1).astype(f32)
    return dict(count=count, min=low, max=high, mean=mean)


def error_map_image(ray_err: torch.Tensor) -> np.ndarray:
    """[H, W] per-ray squared errors -> uint8 grey image of sqrt(err / 3) / 2: the RMS channel error, whose range
    [0, 2] (colours live in [-1, 1]) maps to black .. white."""
    level = torch.sqrt(ray_err / 3) / 2
    return (level.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()


def cross_validate(args, data: NeRFDataset, say: Callable[[str], None] = lambda message: None,
                   progress: Callable[[Iterable], Iterable] = iter,
                   error_maps: Optional[Dict[str, torch.Tensor]] = None
                   ) -> Iterator[Tuple[int, List[Tuple[float, str]]]]:
    """
    K-fold cross-validation (the fold loop of scripts/cv_nerf.py:44-93): the views are permuted and dealt into
    args.folds chunks; for each chunk a fresh model is trained for args.train_iters steps on the other views and
    yields (fold, [(validation loss, image path) of each held-out view, in dataset order]).  `args` carries the
    command line of scripts/cv_nerf.py (seed, lr, batch_size, folds, coarse_samples, fine_samples, train_iters and the
    model switches of add_model_args).

    Keys: init, shuffle, global = Key(seed).split(3).  The permutation is np.random.default_rng(shuffle.seed)'s (JAX's
    is not reproducible here, and nothing depends on which one it is).  Every fold starts from the SAME initial
    parameters (init) and the same key stream (global), as in the reference, so folds differ by their data alone.
    Single process only: no data-parallel path, the train step runs on one device.

    say: receives the reference's two progress lines; progress: wraps the iteration over the training steps (tqdm);
    error_maps (a dict): image path -> [H, W] per-ray squared error of the held-out view.
    """
    from .scripts.train_nerf import create_model
    from .train import TrainLoop

    seed = args.seed if args.seed is not None else random.randint(0, 2 ** 32 - 1)
    init_key, shuffle_key, global_key = Key(seed).split(3)
    order = np.random.default_rng(shuffle_key.seed).permutation(len(data.views)).tolist()
    box = (data.metadata.bbox_min, data.metadata.bbox_max)

    for fold, held_out in enumerate(chunk_indices(args.folds, order)):
        say(f"performing cross validation for fold {fold}...")
        train_data = NeRFDataset(metadata=data.metadata, views=[x for j, x in enumerate(data.views) if j not in held_out])
        valid_data = NeRFDataset(metadata=data.metadata, views=[x for j, x in enumerate(data.views) if j in held_out])
        coarse, fine, train_kwargs = create_model(args, data.metadata)
        loop = TrainLoop(coarse, fine, init_rng=init_key.seed, lr=args.lr, coarse_ts=args.coarse_samples,
                         fine_ts=args.fine_samples, **train_kwargs)
        step_fn = loop.step_fn(*box)
        key = global_key
        with tempfile.TemporaryDirectory() as tmp_dir:
            data_key, key = key.split(2)
            batches = train_data.iterate_batches(tmp_dir, data_key.seed, args.batch_size, device=loop.device)
            batch = next(batches)
            say("dataset shuffling complete.")
            for _ in progress(range(args.train_iters)):
                step_key, key = key.split(2)
                step_fn(step_key, batch)
                batch = next(batches)
            batches.close()  # the shard files are open until the iterator ends
        maps = [] if error_maps is not None else None
        losses = list(validation_losses(key, loop, valid_data, args.batch_size, error_maps=maps))
        if error_maps is not None:
            error_maps.update((view.image_path, m) for view, m in zip(valid_data.views, maps))
        yield fold, [(loss, view.image_path) for view, loss in zip(valid_data.views, losses)]

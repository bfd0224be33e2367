"""
Edges of the fused training backwards: the layer-stationary (LS) NeRF backward (nerf_bwd_ls.hip) at the tile and
pipeline counts where its arithmetic can go wrong, in the launch form the training step uses (the coarse + fine pair of
lnrf_nerf_mlp_bwd_ls2), in the phased form of the kernel timers, and on poisoned workspaces (tests/gpu_poison.py), for
it and for the other fused training backwards (two-launch NeRF, Ref-NeRF, InstantNGP).

Edge sizes follow the device: P = min(64, CUs / 8) pipelines, and pipeline p takes ceil((T - p) / P) of the T tiles
(ceil(m / 32) rounded up to a multiple of 8).  With P = 32:
    m = 1, 33           pipelines p >= 8 get no tile (the zero-slab branch)
    32P - 5             one tile each              32(P + 8) - 31   two and one
    96P + 1             four and three             128P - 1         four each (the prefetch distance is 3)
    70000               69 and 68                  262161           large and ragged
Pairs share the P pipelines in proportion to their evaluations, clamped to [1, P - 1].

Every failure message carries the per-layer relative error tables (ls vs split, split vs split), the status words of
the LS launches, the poison pattern and the device (name, uuid), so that a failure seen once can be diagnosed.
"""
import contextlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from gpu_poison import PATTERNS, poisoned
from nerf_grad_helpers import make_model, make_points, oracle_grads, per_layer_rel_err
from oracle import model as OM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_MAX_M = 8192  # the float64 CPU oracle is too slow above this
LAYER_TOL = 1e-5     # ls vs two-launch, pair vs single: same bf16 operands, only the fp32 summation order differs
ORACLE_TOL = 3e-2    # vs the bf16-operand float64 oracle (as test_gpu_nerf_mlp.py)

SIZES = {
    "1": lambda p: 1,
    "33": lambda p: 33,
    "32P-5": lambda p: 32 * p - 5,
    "32(P+8)-31": lambda p: 32 * (p + 8) - 31,
    "96P+1": lambda p: 96 * p + 1,
    "128P-1": lambda p: 128 * p - 1,
    "70000": lambda p: 70000,
    "262161": lambda p: 262161,
}
PAIRS = [(1, 1), (1, 70000), (70000, 1), (8192, 24576), (70000, 140001), (262144, 786432)]
PHASED_PAIRS = [(8192, 24576), (70000, 140001)]


def pipelines() -> int:
    return min(64, torch.cuda.get_device_properties(0).multi_processor_count // 8)


def tiles_for(m: int) -> int:
    return ((m + 31) // 32 + 7) // 8 * 8


def tiles_per_pipeline(m: int, p: int) -> str:
    t = tiles_for(m)
    counts = sorted({(t - q + p - 1) // p if q < t else 0 for q in range(p)}, reverse=True)
    return f"{t} tiles, per pipeline {counts}"


def pair_split(ma: int, mb: int, p: int):
    """the pipeline split of ls_backward (nerf_bwd_ls.hip)"""
    a = int(p * (ma / (ma + mb)) + 0.5)
    a = min(max(a, 1), p - 1)
    return a, p - a


def device_tag() -> str:
    prop = torch.cuda.get_device_properties(0)
    return f"device {prop.name!r} uuid {getattr(prop, 'uuid', '?')} CUs {prop.multi_processor_count} P {pipelines()}"


def pattern_name(pattern) -> str:
    return "none" if pattern is None else f"0x{pattern:02X}"


def layer_table(model, got, ref, title) -> str:
    rows = per_layer_rel_err(model, got.detach().cpu().double(), ref.detach().cpu().double())
    return "\n".join([f"  {title}:"] + [f"    {n:16s} rel L2 {e:.3e}  (|ref| {r:.3e})" for n, e, r in rows])


def diagnosis(model, ls, split, split2, statuses, pattern, what="") -> str:
    lines = [f"{what}", f"  {device_tag()}", f"  poison pattern {pattern_name(pattern)}, ls_status words {statuses}"]
    if ls is not None and split is not None:
        lines.append(layer_table(model, ls, split, "ls vs split"))
    if split is not None and split2 is not None:
        lines.append(layer_table(model, split2, split, "split vs split"))
    return "\n".join(lines)


@contextlib.contextmanager
def timed(label):
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"[time] {label}: {time.perf_counter() - t0:.2f} s")


def nerf_inputs(m, seed):
    x, d, gen = make_points(m, seed=seed)
    g_dens = torch.randn(m, generator=gen).float()
    g_rgb = torch.randn(m, 3, generator=gen).float()
    return (x.cuda(), d.cuda(), g_dens.cuda(), g_rgb.cuda()), (x, d, g_dens, g_rgb)


def run_single(model, flat, inp, kind):
    """saving forward + backward of `kind` ("ls" | "split") -> density, rgb, gradient, LS status word (None: split)"""
    from learn_nerf.model import ls_status

    model.backward_kernel = kind
    x, d, gd, gr = inp
    dens, rgb, _, ctx = model.forward_points(flat, x, d, save=True)
    g = torch.zeros_like(flat)
    model.backward(ctx, gd, gr, None, g)
    status = ls_status(ctx) if kind == "ls" else None  # read straight after the call (synchronises)
    torch.cuda.synchronize()
    return dens.clone(), rgb.clone(), g, status


def run_pair(models, flats, inps):
    """both saving forwards, then ONE lnrf_nerf_mlp_bwd_ls2 launch -> [(density, rgb, gradient)] x 2, status words"""
    from learn_nerf.model import backward_ls_pair, ls_status

    outs, ctxs = [], []
    for model, flat, (x, d, _, _) in zip(models, flats, inps):
        model.backward_kernel = "ls"
        dens, rgb, _, ctx = model.forward_points(flat, x, d, save=True)
        outs.append([dens, rgb, torch.zeros_like(flat)])
        ctxs.append(ctx)
    backward_ls_pair(ctxs[0], inps[0][2], inps[0][3], outs[0][2], ctxs[1], inps[1][2], inps[1][3], outs[1][2])
    statuses = (ls_status(ctxs[0]), ls_status(ctxs[1]))
    torch.cuda.synchronize()
    return [tuple(t.clone() for t in o) for o in outs], statuses


def assert_layers_close(model, got, ref, tol, msg_fn, what):
    for name, err, nrm in per_layer_rel_err(model, got.detach().cpu().double(), ref.detach().cpu().double()):
        assert err < tol, f"{what}: {name} rel L2 {err:.3e} >= {tol:g} (|ref| {nrm:.3e})\n{msg_fn()}"


def assert_oracle(model, flat, host, got, msg_fn, what):
    ref = oracle_grads(flat.cpu().double(), *host, operand_round=OM.bf16_round)
    assert_layers_close(model, got, ref, ORACLE_TOL, msg_fn, f"{what} vs bf16-operand oracle")


def assert_bits(a, b, msg_fn, what):
    assert torch.equal(a, b), f"{what}: not bit-identical (max |d| {(a - b).abs().max().item():.3e})\n{msg_fn()}"


def assert_finite(t, msg_fn, what):
    assert torch.isfinite(t).all(), f"{what}: {int((~torch.isfinite(t)).sum())} non-finite values\n{msg_fn()}"


def poison_or_clean(pattern, models):
    return contextlib.nullcontext() if pattern is None else poisoned(pattern, models=models)


# ---------------------------------------------------------------------------------------------------------------------
def test_poison_helper_is_not_vacuous():
    """Inside poisoned(): a leased block and a torch.empty on the GPU read back as the pattern; integer tensors and the
    hash-grid bucket lease stay unpoisoned; an LS forward / backward registers nerf_save and nerf_bwd_ls, a two-launch one
    nerf_save and nerf_bwd (a renamed purpose fails here instead of leaving the poison tests poisoning nothing)."""
    from learn_nerf import _ws

    orig_empty, orig_lease = torch.empty, _ws.lease
    for pat in PATTERNS:
        with poisoned(pat) as rec:
            blk = _ws.lease("nerf_bwd", 4096 + 3, "cuda")
            assert (blk.buf == pat).all(), pattern_name(pat)
            blk.release()
            for dt in (torch.float32, torch.bfloat16, torch.float16, torch.uint8):
                t = torch.empty(1000, dtype=dt, device="cuda")
                assert (t.view(torch.uint8) == pat).all(), (pattern_name(pat), dt)
                assert (torch.empty_like(t).view(torch.uint8) == pat).all(), (pattern_name(pat), dt)
            n = rec.empties
            assert n == 8, n
            for dt in (torch.int16, torch.int32, torch.int64):
                torch.empty(1000, dtype=dt, device="cuda")
            assert rec.empties == n, "integer tensors of 16 bits and wider must not be poisoned"
            hb = _ws.lease("hashgrid_bwd", 1 << 16, "cuda")  # its fresh block is allocated with the empty patch suspended
            assert rec.empties == n and "hashgrid_bwd" in rec.purposes
            hb.buf.fill_(0x5A)
            hb.release()
            hb = _ws.lease("hashgrid_bwd", 1 << 16, "cuda")  # the re-used block keeps what its last user wrote
            assert (hb.buf == 0x5A).all(), "the hashgrid_bwd lease must never be poisoned"
            hb.release()
            assert "hashgrid_bwd" not in rec.poisoned_purposes
        assert torch.empty is orig_empty and _ws.lease is orig_lease  # restored on exit

    model, _, flat = make_model("bf16")
    inp, _ = nerf_inputs(777, seed=3)
    for kind, want in (("ls", {"nerf_save", "nerf_bwd_ls"}), ("split", {"nerf_save", "nerf_bwd"})):
        with poisoned(0x41, models=(model,)) as rec:
            run_single(model, flat, inp, kind)
        assert want <= rec.poisoned_purposes, (kind, sorted(rec.purposes))
        assert not rec.unreviewed, rec.unreviewed


@pytest.mark.parametrize("size", list(SIZES))
def test_ls_backward_equals_two_launch_per_layer(size):
    """Single-model LS backward vs the two-launch backward, per Dense layer (kernel and bias) at 1e-5; status word 0;
    and for m <= 8192 both against the bf16-operand float64 oracle at 3e-2."""
    p = pipelines()
    m = SIZES[size](p)
    model, _, flat = make_model("bf16")
    inp, host = nerf_inputs(m, seed=11)
    with timed(f"m={m} ls + 2x split"):
        _, _, g_ls, st = run_single(model, flat, inp, "ls")
        _, _, g_sp, _ = run_single(model, flat, inp, "split")
        _, _, g_sp2, _ = run_single(model, flat, inp, "split")
    msg = lambda: diagnosis(model, g_ls, g_sp, g_sp2, (st,), None, f"m={m} ({tiles_per_pipeline(m, p)})")  # noqa: E731
    assert st == 0, msg()
    assert g_ls.abs().max().item() > 0, msg()
    assert_finite(g_ls, msg, "ls gradient")
    assert_layers_close(model, g_ls, g_sp, LAYER_TOL, msg, "ls vs split")
    assert_bits(g_sp, g_sp2, msg, "split vs split")
    if m <= ORACLE_MAX_M:
        with timed(f"m={m} oracle"):
            assert_oracle(model, flat, host, g_ls, msg, "ls")


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}+{b}" for a, b in PAIRS])
def test_pair_backward_equals_single_model_and_two_launch(pair):
    """backward_ls_pair (lnrf_nerf_mlp_bwd_ls2, the step's launch form: the pipelines shared in proportion to the
    evaluations, clamped to [1, P - 1]) vs the single-model LS backward and vs the two-launch backward, per model and per
    Dense layer at 1e-5; both status words 0; for both m <= 8192 also the oracle gate."""
    p = pipelines()
    ms = pair
    models, flats, inps, hosts = [], [], [], []
    for k, m in enumerate(ms):
        model, _, flat = make_model("bf16", seed=1 + k)
        inp, host = nerf_inputs(m, seed=21 + k)
        models.append(model), flats.append(flat), inps.append(inp), hosts.append(host)
    with timed(f"pair {ms}: pair + single + 2x split"):
        outs, st = run_pair(models, flats, inps)
        singles = [run_single(models[k], flats[k], inps[k], "ls") for k in range(2)]
        splits = [run_single(models[k], flats[k], inps[k], "split") for k in range(2)]
        splits2 = [run_single(models[k], flats[k], inps[k], "split") for k in range(2)]
    split_at = pair_split(*ms, p)
    for k in range(2):
        g_pair = outs[k][2]
        what = (f"pair {ms} model {'ab'[k]} (m={ms[k]}, {split_at[k]} of {p} pipelines, "
                f"{tiles_per_pipeline(ms[k], split_at[k])})")
        msg = lambda: diagnosis(models[k], g_pair, splits[k][2], splits2[k][2],  # noqa: E731
                                (st, singles[k][3]), None, what) + "\n" + \
            layer_table(models[k], g_pair, singles[k][2], "pair vs single-model ls")
        assert st == (0, 0) and singles[k][3] == 0, msg()
        assert g_pair.abs().max().item() > 0, msg()
        assert_finite(g_pair, msg, "pair gradient")
        assert_layers_close(models[k], g_pair, singles[k][2], LAYER_TOL, msg, "pair vs single-model ls")
        assert_layers_close(models[k], g_pair, splits[k][2], LAYER_TOL, msg, "pair vs split")
        assert_bits(outs[k][0], singles[k][0], msg, "pair-forward density")
        if max(ms) <= ORACLE_MAX_M:
            assert_oracle(models[k], flats[k], hosts[k], g_pair, msg, "pair")


@pytest.mark.parametrize("pair", PHASED_PAIRS, ids=[f"{a}+{b}" for a, b in PHASED_PAIRS])
def test_phased_pair_launch_equals_single_launch(pair):
    """With the kernel timers on (bench.py --full) the pair backward runs as three calls (phases 1, 2, 4; the counters
    cleared by a memset): it must give the same bits as the one phases=7 call of the product."""
    from learn_nerf import _prof

    models, flats, inps = [], [], []
    for k, m in enumerate(pair):
        model, _, flat = make_model("bf16", seed=1 + k)
        models.append(model), flats.append(flat), inps.append(nerf_inputs(m, seed=21 + k)[0])
    one, st1 = run_pair(models, flats, inps)
    _prof.enable(True)
    try:
        phased, st3 = run_pair(models, flats, inps)
    finally:
        _prof.enable(False)
    for k in range(2):
        msg = lambda: diagnosis(models[k], phased[k][2], one[k][2], None, (st1, st3), None,  # noqa: E731
                                f"pair {pair} model {'ab'[k]}: phased (first) vs phases=7 (second)")
        assert st1 == (0, 0) and st3 == (0, 0), msg()
        assert_bits(phased[k][2], one[k][2], msg, "phased vs single-launch gradient")


# ---- poison invariance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_single_model_backwards_are_poison_invariant(size):
    """Saving forward + LS backward and saving forward + two-launch backward under the three poison patterns: density,
    rgb and gradients bit-identical to an unpoisoned run (so across the patterns) and finite."""
    p = pipelines()
    m = SIZES[size](p)
    model, _, flat = make_model("bf16")
    inp, _ = nerf_inputs(m, seed=11)
    clean = {k: run_single(model, flat, inp, k) for k in ("ls", "split")}
    for pat in PATTERNS:
        with timed(f"m={m} pattern {pattern_name(pat)}"), poisoned(pat, models=(model,)) as rec:
            got = {k: run_single(model, flat, inp, k) for k in ("ls", "split")}
        assert {"nerf_save", "nerf_bwd_ls", "nerf_bwd"} <= rec.poisoned_purposes, sorted(rec.purposes)
        msg = lambda: diagnosis(model, got["ls"][2], got["split"][2], clean["split"][2],  # noqa: E731
                                (got["ls"][3], clean["ls"][3]), pat, f"m={m} ({tiles_per_pipeline(m, p)})") + "\n" + \
            layer_table(model, got["ls"][2], clean["ls"][2], "ls poisoned vs ls clean")
        assert got["ls"][3] == 0 and clean["ls"][3] == 0, msg()
        for kind in ("ls", "split"):
            for i, name in enumerate(("density", "rgb", "gradient")):
                assert_finite(got[kind][i], msg, f"{kind} {name}")
                assert_bits(got[kind][i], clean[kind][i], msg, f"{kind} {name} poisoned vs clean")


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}+{b}" for a, b in PAIRS])
def test_pair_backward_is_poison_invariant(pair):
    """The pair backward (the step's launch) under the three poison patterns: bit-identical to an unpoisoned run, finite."""
    p = pipelines()
    models, flats, inps = [], [], []
    for k, m in enumerate(pair):
        model, _, flat = make_model("bf16", seed=1 + k)
        models.append(model), flats.append(flat), inps.append(nerf_inputs(m, seed=21 + k)[0])
    clean, st0 = run_pair(models, flats, inps)
    for pat in PATTERNS:
        with timed(f"pair {pair} pattern {pattern_name(pat)}"), poisoned(pat, models=models) as rec:
            got, st = run_pair(models, flats, inps)
        assert {"nerf_save", "nerf_bwd_ls"} <= rec.poisoned_purposes, sorted(rec.purposes)
        split_at = pair_split(*pair, p)
        for k in range(2):
            msg = lambda: diagnosis(models[k], got[k][2], None, None, (st, st0), pat,  # noqa: E731
                                    f"pair {pair} model {'ab'[k]} ({split_at[k]} of {p} pipelines, "
                                    f"{tiles_per_pipeline(pair[k], split_at[k])})") + "\n" + \
                layer_table(models[k], got[k][2], clean[k][2], "pair poisoned vs pair clean")
            assert st == (0, 0) and st0 == (0, 0), msg()
            for i, name in enumerate(("density", "rgb", "gradient")):
                assert_finite(got[k][i], msg, name)
                assert_bits(got[k][i], clean[k][i], msg, f"{name} poisoned vs clean")


def test_rays_mode_forward_backward_is_poison_invariant():
    """Rays-mode forwards (the step's form: points formed in the kernel) at a ragged (n, t) = (37, 19): the saving forward
    with the LS and the two-launch backward, and the render forward, bit-identical under the three patterns."""
    from learn_nerf.model import ls_status

    n, t = 37, 19
    model, _, flat = make_model("bf16")
    gen = torch.Generator().manual_seed(4)
    o = torch.rand(n, 3, generator=gen) * 0.4 - 0.2
    dv = torch.randn(n, 3, generator=gen)
    rays = torch.stack([o, dv / dv.norm(dim=-1, keepdim=True)], 1).float().contiguous().cuda()
    ts = torch.sort(torch.rand(n, t, generator=gen) * 1.5 + 0.1, dim=1).values.float().contiguous().cuda()
    gd = torch.randn(n, t, generator=gen).float().cuda()
    gr = torch.randn(n, t, 3, generator=gen).float().cuda()

    def run():
        out = []
        for kind in ("ls", "split"):
            model.backward_kernel = kind
            dens, rgb, _, ctx = model.forward_rays(flat, rays, ts, save=True)
            g = torch.zeros_like(flat)
            model.backward(ctx, gd, gr, None, g)
            out += [dens.clone(), rgb.clone(), g, torch.tensor(float(ls_status(ctx)))]
        dens, rgb, _, _ = model.forward_rays(flat, rays, ts, save=False)
        torch.cuda.synchronize()
        return out + [dens.clone(), rgb.clone()]

    names = ["ls density", "ls rgb", "ls gradient", "ls status", "split density", "split rgb", "split gradient",
             "split status", "render density", "render rgb"]
    clean = run()
    assert clean[3].item() == 0
    for pat in PATTERNS:
        with poisoned(pat, models=(model,)):
            got = run()
        msg = lambda: diagnosis(model, got[2], got[6], clean[6], (got[3].item(), clean[3].item()), pat,  # noqa: E731
                                f"rays mode (n, t) = ({n}, {t})")
        for name, a, b in zip(names, got, clean):
            assert_finite(a, msg, name)
            assert_bits(a, b, msg, f"{name} poisoned vs clean")


# ---- first call vs later calls --------------------------------------------------------------------------------------
FIRST_CALL_M = 70000


def first_call_case():
    """model, flat and inputs of the first-call cases (the worker builds the same ones)"""
    model, _, flat = make_model("bf16")
    inp, _ = nerf_inputs(FIRST_CALL_M, seed=11)
    return model, flat, inp


def test_first_calls_equal_later_calls_from_an_empty_pool():
    """After _ws.clear() and torch.cuda.empty_cache() the first LS and the first two-launch backward at m = 70000 (the
    case recorded in DESIGN.md) are bit-identical to a second and a third call."""
    from learn_nerf import _ws

    model, flat, inp = first_call_case()
    torch.cuda.synchronize()
    _ws.clear()
    model._pack_cache = None
    torch.cuda.empty_cache()
    runs = {k: [run_single(model, flat, inp, k) for _ in range(3)] for k in ("ls", "split")}
    for kind in ("ls", "split"):
        first = runs[kind][0]
        for j in (1, 2):
            later = runs[kind][j]
            msg = lambda: diagnosis(model, runs["ls"][0][2], runs["split"][0][2], runs["split"][j][2],  # noqa: E731
                                    [r[3] for r in runs["ls"]], None,
                                    f"m={FIRST_CALL_M}: first {kind} call vs call {j + 1}") + "\n" + \
                layer_table(model, runs["ls"][j][2], runs["ls"][0][2], f"ls call {j + 1} vs ls call 1")
            assert runs["ls"][j][3] == 0 and runs["ls"][0][3] == 0, msg()
            for i, name in enumerate(("density", "rgb", "gradient")):
                assert_bits(later[i], first[i], msg, f"{kind} {name}")


def test_first_call_of_a_fresh_process_equals_this_process(tmp_path):
    """The recorded symptom was "the first LS run of a process": a fresh child process (tests/ls_first_call_worker.py)
    runs its first LS and first two-launch backward at m = 70000 and writes them as .npy; they must be bit-equal to this
    process's (warm) results."""
    worker = os.path.join(HERE, "ls_first_call_worker.py")
    with timed("fresh child process"):
        r = subprocess.run([sys.executable, worker, str(tmp_path)], timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    model, flat, inp = first_call_case()
    mine = {k: run_single(model, flat, inp, k) for k in ("ls", "split")}
    child = {name: torch.from_numpy(np.load(os.path.join(str(tmp_path), f"{name}.npy")))
             for name in ("ls_density", "ls_rgb", "ls_gradient", "split_density", "split_rgb", "split_gradient")}
    child_status = int(np.load(os.path.join(str(tmp_path), "ls_status.npy")))
    msg = lambda: diagnosis(model, child["ls_gradient"], child["split_gradient"], mine["split"][2],  # noqa: E731
                            (child_status, mine["ls"][3]), None,
                            f"m={FIRST_CALL_M}: first calls of a fresh process (child) vs this process; split vs split "
                            f"is this process vs the child") + "\n" + \
        layer_table(model, child["ls_gradient"], mine["ls"][2], "ls child vs ls this process") + \
        f"\n  child stdout: {r.stdout[-1500:]}"
    assert child_status == 0 and mine["ls"][3] == 0, msg()
    for kind in ("ls", "split"):
        for i, name in enumerate(("density", "rgb", "gradient")):
            assert_bits(child[f"{kind}_{name}"], mine[kind][i].cpu(), msg, f"{kind} {name}")


# ---- the whole step -------------------------------------------------------------------------------------------------
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def make_batch(n, seed=0):
    gen = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=gen)
    o = 4 * o / o.norm(dim=-1, keepdim=True)
    d = -o + (torch.rand(n, 3, generator=gen) - 0.5) * 0.6
    d[: n // 10] = torch.randn(n // 10, 3, generator=gen)  # some rays miss the box
    d = d / d.norm(dim=-1, keepdim=True)
    c = torch.rand(n, 3, generator=gen) * 2 - 1
    return torch.stack([o, d, c], 1).float().contiguous()


@pytest.mark.parametrize("n,tc,tf", [(4096, 64, 128), (333, 16, 32)])
def test_train_step_is_poison_invariant(n, tc, tf):
    """TrainLoop(NeRFModel(), NeRFModel()) as the product runs it (sampling, compositing, the pair backward, Adam,
    step_log): two steps under each pattern leave flat, opt_m, opt_v and the last gradient bit-identical to two
    unpoisoned steps, and the logged losses and norms finite and equal to rounding."""
    from learn_nerf.model import NeRFModel
    from learn_nerf.train import TrainLoop

    batch = make_batch(n, seed=5).cuda()

    def run(pattern):
        loop = TrainLoop(NeRFModel(), NeRFModel(), init_rng=11, lr=1e-3, coarse_ts=tc, fine_ts=tf)
        for name in ("coarse", "fine"):  # make the medium partly opaque so that compositing matters
            loop.state.params[name]["Dense_9"]["kernel"].mul_(6.0)
            loop.state.params[name]["Dense_9"]["bias"].add_(1.5)
        step = loop.step_fn(BMIN, BMAX)
        logs = []
        with poison_or_clean(pattern, (loop.coarse, loop.fine)) as rec:
            for it in range(2):
                logs.append(torch.stack([v.reshape(()) for v in step(100 + it, batch).values()]).clone())
            torch.cuda.synchronize()
        if rec is not None:
            assert {"nerf_save", "nerf_bwd_ls", "composite_bwd"} <= rec.poisoned_purposes, sorted(rec.purposes)
        return dict(flat=loop.flat.clone(), opt_m=loop.state.opt_m.clone(), opt_v=loop.state.opt_v.clone(),
                    grad=loop.grad.clone(), log0=logs[0], log1=logs[1]), loop

    clean, loop = run(None)
    for k, v in clean.items():
        assert torch.isfinite(v).all(), k
    for pat in PATTERNS:
        with timed(f"step {n}x({tc}+{tf}) pattern {pattern_name(pat)}"):
            got, _ = run(pat)
        c0, c1, _ = loop._slices(got["grad"])
        r0, r1, _ = loop._slices(clean["grad"])
        msg = lambda: (f"step {n} rays x ({tc} + {tf}), pattern {pattern_name(pat)}, {device_tag()}\n"  # noqa: E731
                       + layer_table(loop.coarse, c0, r0, "coarse gradient of step 2, poisoned vs clean") + "\n"
                       + layer_table(loop.fine, c1, r1, "fine gradient of step 2, poisoned vs clean")
                       + f"\n  logs poisoned {got['log1'].tolist()} clean {clean['log1'].tolist()}")
        for k in ("flat", "opt_m", "opt_v", "grad"):
            assert_finite(got[k], msg, k)
            assert_bits(got[k], clean[k], msg, k)
        # the logged sums (squared errors, norms) end in one fp32 atomic per workgroup (rays.hip, optim.hip): their
        # arrival order varies from run to run, so the log agrees to rounding, not bit for bit
        for k in ("log0", "log1"):
            assert_finite(got[k], msg, k)
            rel = ((got[k] - clean[k]).abs() / clean[k].abs().clamp_min(1e-30)).max().item()
            assert rel < 1e-5, f"{k}: rel {rel:.3e}\n{msg()}"


# ---- the other fused training backwards -----------------------------------------------------------------------------
REF_SIZES = {"1": lambda p: 1, "33": lambda p: 33, "32P+1": lambda p: 32 * p + 1, "70000": lambda p: 70000}


def make_ref_nerf(seed=3):
    from learn_nerf.ref_nerf import RefNERFModel

    model = RefNERFModel(precision="bf16")
    params = model.init(dict(params=seed))["params"]
    flat = model.flat(params)
    gen = torch.Generator().manual_seed(seed + 1)
    off = 0
    for fi, fo in model.layer_dims():  # non-zero biases
        off += fi * fo
        flat[off:off + fo] += (torch.randn(fo, generator=gen) * 0.1).cuda()
        off += fo
    return model, flat


@pytest.mark.parametrize("size", list(REF_SIZES))
def test_ref_nerf_fused_backward_is_poison_invariant(size):
    """RefNERFModel at default widths (fused trunk, normal pass, LS first-order trunk backward, directional block):
    outputs, aux and gradients bit-identical under the three patterns and finite; at m in {33, 32P+1} also the 3e-2
    bf16-operand oracle gate of test_ref_nerf_bf16_paths."""
    from oracle import ref_nerf as ORF
    from oracle.model import bf16_round

    p = pipelines()
    m = REF_SIZES[size](p)
    model, flat = make_ref_nerf()
    assert model._use_fused_trunk()
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(m, 3, generator=gen) * 2 - 1).float()
    dv = torch.randn(m, 3, generator=torch.Generator().manual_seed(9))
    d = (dv / dv.norm(dim=-1, keepdim=True)).float().contiguous()
    g_d = torch.randn(m, generator=gen).float()
    g_c = torch.randn(m, 3, generator=gen).float()
    g_a = {"normal_mse": torch.rand(m, generator=gen).float(), "neg_normal": torch.rand(m, generator=gen).float()}
    xc, dc, gdc, gcc = x.cuda(), d.cuda(), g_d.cuda(), g_c.cuda()
    gac = {k: v.cuda() for k, v in g_a.items()}

    def run():
        dens, rgb, aux, ctx = model.forward_points(flat, xc, dc, save=True)
        grad = torch.zeros_like(flat)
        model.backward(ctx, gdc, gcc, gac, grad)
        torch.cuda.synchronize()
        return [dens.clone(), rgb.clone()] + [aux[k].clone() for k in sorted(aux)] + [grad]

    clean = run()
    for pat in PATTERNS:
        with timed(f"ref-nerf m={m} pattern {pattern_name(pat)}"), poisoned(pat, models=(model,)) as rec:
            got = run()
        msg = lambda: (f"ref-nerf m={m}, pattern {pattern_name(pat)}, {device_tag()}, purposes "  # noqa: E731
                       f"{sorted(rec.poisoned_purposes)}; gradient rel L2 poisoned vs clean "
                       f"{((got[-1] - clean[-1]).norm() / clean[-1].norm()).item():.3e}")
        assert not rec.unreviewed, rec.unreviewed
        for i, (a, b) in enumerate(zip(got, clean)):
            assert_finite(a, msg, f"output {i}")
            assert_bits(a, b, msg, f"output {i} (density, rgb, aux..., gradient) poisoned vs clean")
    if size in ("33", "32P+1"):
        okw = dict(sh_degree=model.sh_degree, hidden_dim=model.hidden_dim, color_layer_dim=model.color_layer_dim)
        f32 = flat.cpu().float().requires_grad_(True)
        rd, rr, raux = ORF.ref_nerf_model(f32, x, d, operand_round=bf16_round, **okw)
        e_rgb = (clean[1].cpu() - rr).abs().max().item()
        e_den = ((clean[0].reshape(-1).cpu() - rd[:, 0]).abs() / (1 + rd[:, 0].abs())).max().item()
        assert e_rgb < 4e-3 and e_den < 4e-3, (e_rgb, e_den)
        loss = (rd[:, 0] * g_d).sum() + (rr * g_c).sum() + sum((raux[k] * g_a[k]).sum() for k in g_a)
        (g_ref,) = torch.autograd.grad(loss, f32)
        rel = ((clean[-1].cpu() - g_ref).norm() / g_ref.norm()).item()
        print(f"ref-nerf m={m}: rgb {e_rgb:.2e} density {e_den:.2e} gradient rel L2 {rel:.2e} vs bf16-operand oracle")
        assert rel < 3e-2, rel


NGP_BMIN, NGP_BMAX = (-1.0, -0.5, -2.0), (1.0, 1.5, 0.5)


@pytest.mark.parametrize("m", [1, 31, 70000])
def test_instant_ngp_fused_backward_is_poison_invariant(m):
    """Fused InstantNGP (16 levels, T = 2^14) under the three patterns: the Dense part of the gradient bit-identical to an
    unpoisoned run; the table part finite and within 1e-5 relative L2 (its split buckets meet in fp32 atomics, see
    test_ngp_fused_backward_dense_gradients_are_bit_reproducible); density and rgb bit-identical."""
    from learn_nerf.instant_ngp import InstantNGPModel

    levels = 16
    model = InstantNGPModel(table_sizes=[2 ** 14] * levels, grid_sizes=[2 ** (4 + i // 2) for i in range(levels)],
                            bbox_min=NGP_BMIN, bbox_max=NGP_BMAX, hidden_dim=64, precision="bf16")
    flat = model.flat(model.init(dict(params=2))["params"])
    nt = model.encoding().num_table_floats()
    gen = torch.Generator().manual_seed(2)
    flat[:nt] = ((torch.rand(nt, generator=gen) * 2 - 1) * 0.5).cuda()
    lo, hi = torch.tensor(NGP_BMIN), torch.tensor(NGP_BMAX)
    x = (torch.rand(m, 3, generator=gen) * (hi - lo) * 1.1 + lo - 0.05 * (hi - lo)).float().contiguous().cuda()
    dv = torch.randn(m, 3, generator=gen)
    d = (dv / dv.norm(dim=-1, keepdim=True)).float().contiguous().cuda()
    g_d = torch.randn(m, generator=gen).float().cuda()
    g_c = torch.randn(m, 3, generator=gen).float().cuda()

    def run():
        dens, rgb, _, ctx = model.forward_points(flat, x, d, save=True)
        g = torch.zeros_like(flat)
        model.backward(ctx, g_d, g_c, None, g)
        torch.cuda.synchronize()
        return dens.clone(), rgb.clone(), g

    clean = run()
    assert clean[2][nt:].abs().max().item() > 0
    for pat in PATTERNS:
        with timed(f"ngp m={m} pattern {pattern_name(pat)}"), poisoned(pat, models=(model,)) as rec:
            got = run()
        rel = ((got[2][:nt] - clean[2][:nt]).norm() / clean[2][:nt].norm().clamp_min(1e-30)).item()
        msg = lambda: (f"instant-ngp m={m}, pattern {pattern_name(pat)}, {device_tag()}, poisoned purposes "  # noqa: E731
                       f"{sorted(rec.poisoned_purposes)}; table gradient rel L2 {rel:.3e}, dense max |d| "
                       f"{(got[2][nt:] - clean[2][nt:]).abs().max().item():.3e}")
        assert "ngp_scratch" in rec.poisoned_purposes and "hashgrid_bwd" not in rec.poisoned_purposes, msg()
        for i, name in enumerate(("density", "rgb")):
            assert_finite(got[i], msg, name)
            assert_bits(got[i], clean[i], msg, name)
        assert_finite(got[2], msg, "gradient")
        assert_bits(got[2][nt:], clean[2][nt:], msg, "dense gradient")
        assert rel < 1e-5, msg()

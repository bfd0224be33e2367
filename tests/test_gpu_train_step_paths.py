"""
Whole training steps on the branches of TrainLoop._forward_backward that the per-kernel tests do not reach:

  A  the DEFAULT Ref-NeRF step (fused trunk, normal pass, fused directional block, first- and second-order fused backward,
     coarse backward on a second stream, Adam) against the oracle with the same operand rounding;
  B  density_penalty (train.py:153-184) for every model family: the only place of a step where a model's backward runs a
     second time into a gradient slice that already holds a gradient (ModelBase.backward: "grad_flat += ..."), plus that
     accumulate contract on its own at points level;
  C  the two-stream backward: bit equality with and without it for Ref-NeRF, the oracle comparison once more with it for
     NeRFModel (single layer-stationary launches instead of the paired one) and InstantNGPModel.

Shapes: 50 rays (5 of them point away from the box), 9 coarse + 14 fine samples, i.e. 450 and 1150 evaluations, neither a
multiple of the kernels' 32-row tile; 100 penalty points.  The gradient is compared per model slice and the three
background entries on their own (train_step_reference.compare_gradient).  Bounds: exact-fp32 paths 1e-5 (losses) / 5e-3
(gradient, relative L2), bf16-operand paths 2e-3 / 3e-2 against the oracle that rounds the same operands — the bounds of
test_train_step_matches_oracle, test_ref_nerf_bf16_paths and test_ngp_train_step_matches_oracle.
"""
import functools
from dataclasses import dataclass
from typing import Callable, Optional

import pytest
import torch

import train_step_reference as R
from oracle.model import bf16_round

pytestmark = pytest.mark.gpu
F64 = torch.float64
N, TC, TF, PENALTY_POINTS = 50, 9, 14, 100
BMIN, BMAX = R.BMIN, R.BMAX


@functools.lru_cache(maxsize=None)
def batch():
    return R.make_batch(N, seed=5, away=True)


# ---------------------------------------------------------------- model families
def _nerf(**kw):
    from learn_nerf.model import NeRFModel

    return lambda which: NeRFModel(**kw)


def _ref_nerf(**kw):
    from learn_nerf.ref_nerf import RefNERFModel

    return lambda which: RefNERFModel(**kw)


def _ngp(precision):
    from learn_nerf.instant_ngp import InstantNGPModel

    def make(which):  # as test_ngp_train_step_matches_oracle: 3 levels coarse, 5 levels fine
        levels = 3 if which == "coarse" else 5
        return InstantNGPModel(table_sizes=[2 ** 12] * levels, grid_sizes=[2 ** (4 + i // 2) for i in range(levels)],
                               bbox_min=BMIN, bbox_max=BMAX, precision=precision)

    return make


def _fill_tables(flat, model, gen):
    """U(-1e-4, 1e-4) tables (instant_ngp.py:181-185) would hide gather / scatter errors."""
    nt = model.encoding().num_table_floats()
    flat[:nt] = ((torch.rand(nt, generator=gen) * 2 - 1) * 0.5).to(flat.device)


@dataclass
class Family:
    make: Callable  # "coarse" | "fine" -> model
    precision: str  # arithmetic of the TRAINING path: "fp32" exact | "bf16" operands rounded, fp32 accumulate
    lam: float  # density_penalty of case B; the oracle share it gives is asserted there
    oracle_dtype: torch.dtype = F64  # Ref-NeRF bf16: float32 parameters, as test_ref_nerf_bf16_paths
    loop_kw: Optional[dict] = None
    boost: bool = False  # NeRFModel: scale the density head (random init is almost transparent)
    tables: bool = False

    @property
    def rnd(self):
        return bf16_round if self.precision == "bf16" else None

    @property
    def ltol(self):
        return 1e-5 if self.precision == "fp32" else 2e-3

    @property
    def gtol(self):
        return 5e-3 if self.precision == "fp32" else 3e-2

    def density_tol(self, ref):
        """the density bounds of the point-level tests (test_ref_nerf_forward_backward / test_ref_nerf_bf16_paths)"""
        return 1e-4 * max(1.0, abs(ref)) if self.precision == "fp32" else 4e-3 * (1.0 + abs(ref))


NGP_ADAM = dict(lr=1e-2, adam_eps=1e-15, adam_b1=0.9, adam_b2=0.99)  # scripts/train_nerf.py:161
# lam: chosen on the CPU oracle so that the penalty carries >= 0.3 of each slice's gradient norm (asserted in case B);
# |grad mean density| / |render gradient| per slice there: NeRF (boosted head) 11.3 / 0.38 and 10.4 / 0.43,
# Ref-NeRF 3.5 / 1.05 and 2.6 / 0.80, Ref-NeRF 64-wide 2.1 / 0.51 and 2.3 / 0.77, hash grid 1.19 / 0.58 and 1.08 / 0.44
FAMILIES = {
    "nerf-fp32": lambda: Family(_nerf(precision="fp32"), "fp32", 0.03, boost=True),
    "nerf-fused-ls": lambda: Family(_nerf(), "bf16", 0.03, boost=True),
    "nerf-fused-split": lambda: Family(_nerf(backward_kernel="split"), "bf16", 0.03, boost=True),
    "refnerf-fused": lambda: Family(_ref_nerf(), "bf16", 0.3, oracle_dtype=torch.float32),
    "refnerf-fp32-small": lambda: Family(_ref_nerf(precision="fp32", hidden_dim=64, color_layer_dim=32), "fp32", 0.3),
    "ngp-fp32": lambda: Family(_ngp("fp32"), "fp32", 0.3, loop_kw=NGP_ADAM, tables=True),
    "ngp-bf16": lambda: Family(_ngp("bf16"), "bf16", 0.3, loop_kw=NGP_ADAM, tables=True),
}


def build_loop(fam, init_rng=11, **kw):
    from learn_nerf.train import TrainLoop

    loop_kw = dict(lr=1e-3)
    loop_kw.update(fam.loop_kw or {})
    loop_kw.update(kw)
    loop = TrainLoop(fam.make("coarse"), fam.make("fine"), init_rng=init_rng, coarse_ts=TC, fine_ts=TF, **loop_kw)
    if fam.boost:
        R.boost_density(loop)
    if fam.tables:
        gen = torch.Generator().manual_seed(0)
        for mdl, sl in zip((loop.coarse, loop.fine), loop._slices(loop.flat)[:2]):
            _fill_tables(sl, mdl, gen)
    R.add_bias_noise_(loop)
    return loop


def capture_backward_contexts(loop):
    """Record the context of every model.backward call of the loop's two models: {"coarse": [ctx, ...], "fine": [...]}."""
    seen = {"coarse": [], "fine": []}
    for name, mdl in (("coarse", loop.coarse), ("fine", loop.fine)):
        def wrapped(ctx, *args, _orig=mdl.backward, _name=name):
            seen[_name].append(ctx)
            return _orig(ctx, *args)

        mdl.backward = wrapped
    return seen


def capture_penalty_points(loop):
    """Record the (x, d) of every forward_points call at the penalty batch size, per model."""
    seen = {"coarse": [], "fine": []}
    for name, mdl in (("coarse", loop.coarse), ("fine", loop.fine)):
        def wrapped(flat, x, d, save, _orig=mdl.forward_points, _name=name):
            if x.shape[0] == PENALTY_POINTS:
                seen[_name].append((x.clone(), d.clone()))
            return _orig(flat, x, d, save)

        mdl.forward_points = wrapped
    return seen


AUX_KEYS = ("coarse_normal_mse", "coarse_neg_normal", "fine_normal_mse", "fine_neg_normal")


def aux_bound(fam, key, ref, exact):
    """Bound on |device - oracle| of an aux loss in a training step.  Exact-fp32 path: the bounds of
    test_ref_nerf_train_step_matches_oracle (normal_mse compares unit normals built from fp32 input gradients: 2e-3;
    neg_normal 1e-4).  bf16 operands: the project has no bound for these, so the larger of the fp32 step test's
    normal_mse bound and the distance between the bf16-operand oracle and the exact float64 oracle for this key — what
    the operand rounding itself moves the quantity by on these inputs."""
    if fam.precision == "fp32":
        return (2e-3 if key.endswith("normal_mse") else 1e-4) * max(1.0, abs(ref))
    return max(2e-3 * max(1.0, abs(ref)), abs(ref - exact))


def run_steps(loop, fam, steps, key0, lam=None, ltol=None, check_adam=True, label=""):
    """`steps` training steps of `loop` on the shared batch, each compared with the oracle step from the same parameters,
    uniforms and (with lam) penalty points; after a step the oracle continues from the device's parameters and moments
    so that the next one compares like with like.  Returns the oracle results."""
    ltol = fam.ltol if ltol is None else ltol
    step = loop.step_fn(BMIN, BMAX)
    make_c, make_f = R.model_fn_factory(loop.coarse, fam.rnd), R.model_fn_factory(loop.fine, fam.rnd)
    exact_c, exact_f = R.model_fn_factory(loop.coarse), R.model_fn_factory(loop.fine)
    has_aux = bool(loop.coarse.AUX_NAMES)
    lr, adam = loop.lr, (loop.adam_b1, loop.adam_b2, loop.adam_eps)
    refs = []
    for it in range(steps):
        key = key0 + it
        tag = f"{label} step {it}:"
        p = R.split_flat(loop)
        opt = None if it == 0 else dict(m=list(R.split_flat(loop, loop.state.opt_m)),
                                        v=list(R.split_flat(loop, loop.state.opt_v)))
        uc, uf = R.uniforms_for(key, N, TC, TF)
        penalty = None
        if lam is not None:
            coords, dirs = loop.density_points(R.step_keys(key)[2], BMIN, BMAX)
            penalty = (lam, coords.cpu(), dirs.cpu())
        ref = R.oracle_step(make_c, make_f, p, batch(), TC, TF, uc, uf, dtype=fam.oracle_dtype,
                            loss_weights=loop.loss_weights, penalty=penalty)
        refs.append(ref)
        rl = {k: float(v) for k, v in ref["log"].items()}
        assert ref["hit"] == N - N // 10
        if it == 0:  # (one Adam step of lr per entry moves the boosted NeRF density head a long way: first step only)
            assert 0.3 < ref["mean_density"] < 3.0, "the scene must not be degenerate at the start"
        log = {k: float(v) for k, v in step(key, batch().cuda()).items()}
        assert set(log) == set(rl), (sorted(log), sorted(rl))
        for k in ("coarse", "fine"):
            print(f"{tag} {k} loss {log[k]:.6f} / oracle {rl[k]:.6f} |d| {abs(log[k] - rl[k]):.2e}")
            assert abs(log[k] - rl[k]) < ltol * max(1.0, abs(rl[k])), (k, log[k], rl[k])
        if has_aux:
            exact = rl
            if fam.precision == "bf16":
                ex = R.oracle_step(exact_c, exact_f, p, batch(), TC, TF, uc, uf, dtype=F64,
                                   loss_weights=loop.loss_weights, penalty=penalty, want_grad=False)
                exact = {k: float(v) for k, v in ex["log"].items()}
            for k in AUX_KEYS:
                bound = aux_bound(fam, k, rl[k], exact[k])
                print(f"{tag} {k} {log[k]:.6f} / oracle {rl[k]:.6f} |d| {abs(log[k] - rl[k]):.2e}; oracle to exact "
                      f"float64 oracle {abs(rl[k] - exact[k]):.2e}; bound {bound:.2e}")
                assert abs(log[k] - rl[k]) <= bound, (k, log[k], rl[k], bound)
        if lam is not None:
            for k in ("coarse_density", "fine_density"):
                print(f"{tag} {k} {log[k]:.6f} / oracle {rl[k]:.6f} |d| {abs(log[k] - rl[k]):.2e}")
                assert abs(log[k] - rl[k]) < fam.density_tol(rl[k]), (k, log[k], rl[k])
        R.compare_gradient(loop, ref["grads"], fam.gtol, label=tag)
        print(f"{tag} grad_norm {log['grad_norm']:.5f} / {rl['grad_norm']:.5f}, param_norm {log['param_norm']:.5f} / "
              f"{rl['param_norm']:.5f}")
        assert abs(log["grad_norm"] - rl["grad_norm"]) < fam.gtol * rl["grad_norm"]
        assert abs(log["param_norm"] - rl["param_norm"]) < 1e-4 * rl["param_norm"]
        if check_adam:
            new_p, new_opt = R.oracle_adam(p, ref["grads"], opt, it + 1, lr, *adam)
            upd_err = (loop.flat.cpu().double() - torch.cat([t.reshape(-1) for t in new_p])).abs().max().item()
            m_rel = R.rel_l2(loop.state.opt_m.cpu(), torch.cat([t.reshape(-1) for t in new_opt["m"]]))
            print(f"{tag} Adam update max |d| {upd_err:.2e} (lr {lr:g}), opt_m rel L2 err {m_rel:.2e}")
            # Adam normalises the step to ~lr per entry; a sign flip of a tiny gradient bounds the error by 2 * lr
            assert upd_err <= 2.01 * lr
            assert m_rel < fam.gtol
    return refs


# ---------------------------------------------------------------- A: the default fused Ref-NeRF step
def test_fused_ref_nerf_step_matches_oracle():
    """TrainLoop(RefNERFModel(), RefNERFModel()) as bench.py and train_nerf.py run it, two steps.

    Measured on an MI355X, |device - bf16-operand oracle|, step 0 / step 1: coarse loss 4e-6 / 3e-6, fine loss 2e-5 / 2e-6;
    gradient relative L2, coarse slice 2.2e-3 / 4.5e-3, fine slice 4.3e-3 / 9.3e-3; coarse_normal_mse 3.1e-3 / 9.6e-4
    (bound 3.5e-3 / 2.9e-3), fine_normal_mse 2.3e-3 / 3.3e-4 (bound 7.4e-3 / 7.5e-3), *_neg_normal 1e-6..6e-5 (2e-3).  The
    aux bound is computed here from the two oracles (aux_bound): their distance was 2.1e-3 / 1.8e-3 for coarse_normal_mse,
    7.4e-3 / 7.5e-3 for fine_normal_mse and 2e-5..3e-4 for *_neg_normal."""
    fam = FAMILIES["refnerf-fused"]()
    loop = build_loop(fam, init_rng=8)
    for mdl in (loop.coarse, loop.fine):
        assert mdl._use_fused_trunk() and mdl._use_fused_dir() and mdl.precision == "bf16"
    assert loop.overlap_backward
    seen = capture_backward_contexts(loop)
    run_steps(loop, fam, steps=2, key0=100, label="fused ref-nerf")
    assert loop._side_stream is not None  # the coarse backward did run on the second stream
    for name in ("coarse", "fine"):
        assert len(seen[name]) == 2
        for ctx in seen[name]:  # the fused chain, not the dense GEMM path
            assert ctx["kind"] == "fused" and ctx["dsave"] is not None and ctx["hcol"] is None
    assert seen["coarse"][-1]["x"].shape[0] == N * TC and seen["fine"][-1]["x"].shape[0] == N * (TC + TF)


# ---------------------------------------------------------------- B: density penalty
def test_density_points_are_in_the_box_unit_and_keyed():
    fam = FAMILIES["nerf-fp32"]()
    loop = build_loop(fam, density_penalty=0.1, density_penalty_batch_size=PENALTY_POINTS)
    bmin, bmax = (-1.0, -0.5, -2.0), (1.0, 1.5, 0.5)
    key = R.step_keys(7)[2]
    x, d = loop.density_points(key, bmin, bmax)
    assert x.shape == d.shape == (PENALTY_POINTS, 3) and x.dtype == d.dtype == torch.float32
    assert x.is_contiguous() and d.is_contiguous()
    lo, hi = torch.tensor(bmin).cuda(), torch.tensor(bmax).cuda()
    assert bool((x >= lo).all()) and bool((x <= hi).all())
    # uniform over the whole box, not a corner of it: the sample range covers most of every axis
    assert bool(((x.max(0).values - x.min(0).values) > 0.9 * (hi - lo)).all())
    assert (d.norm(dim=-1) - 1).abs().max().item() < 1e-6
    x2, d2 = loop.density_points(key, bmin, bmax)
    assert torch.equal(x, x2) and torch.equal(d, d2)
    x3, d3 = loop.density_points(R.step_keys(8)[2], bmin, bmax)
    assert not torch.equal(x, x3) and not torch.equal(d, d3)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_density_penalty_step_matches_oracle(family):
    fam = FAMILIES[family]()
    lam = fam.lam
    loop = build_loop(fam, density_penalty=lam, density_penalty_batch_size=PENALTY_POINTS)
    key = 300
    points = capture_penalty_points(loop)

    # -- the no-gradient path (TrainLoop.losses) against the EXACT float64 oracle: it runs the exact-fp32 dense kernels or,
    # on the fused configurations, the split-precision kernels.  total = render terms + weighted aux + lam * densities.
    p = R.split_flat(loop)
    uc, uf = R.uniforms_for(key, N, TC, TF)
    coords, dirs = loop.density_points(R.step_keys(key)[2], BMIN, BMAX)
    ex = R.oracle_step(R.model_fn_factory(loop.coarse), R.model_fn_factory(loop.fine), p, batch(), TC, TF, uc, uf,
                       loss_weights=loop.loss_weights, penalty=(lam, coords.cpu(), dirs.cpu()), want_grad=False)
    total, ld = loop.losses(key, BMIN, BMAX, batch().cuda())
    ld = {k: float(v) for k, v in ld.items()}
    el = {k: float(v) for k, v in ex["log"].items()}
    assert set(ld) == set(el)
    total_bound, recomposed = 0.0, 0.0
    for k in sorted(el):
        name = k.split("_", 1)[1] if "_" in k else None
        if name is None:
            weight, tol = 1.0, 1e-4 * max(1.0, abs(el[k]))
        elif name == "density":
            weight, tol = lam, 1e-4 * max(1.0, abs(el[k]))
        else:
            weight, tol = loop.loss_weights[name], 2e-3 * abs(el[k])
        print(f"{family} losses(): {k} {ld[k]:.6f} / exact oracle {el[k]:.6f} |d| {abs(ld[k] - el[k]):.2e} (tol {tol:.1e})")
        assert abs(ld[k] - el[k]) <= tol, (k, ld[k], el[k])
        total_bound += weight * tol
        recomposed += weight * ld[k]
    assert abs(float(total) - recomposed) < 1e-5 * max(1.0, abs(recomposed))
    assert abs(float(total) - float(ex["total"])) <= total_bound + 1e-5

    # -- the training step against the oracle of its arithmetic
    (ref,) = run_steps(loop, fam, steps=1, key0=key, lam=lam, label=family)
    for i, name in enumerate(("coarse", "fine")):
        share = (ref["penalty_grads"][i].double().norm() / ref["grads"][i].double().norm()).item()
        print(f"{family} {name}: lambda {lam}: |lambda grad(mean density)| / |grad total| = {share:.3f} in the oracle")
        assert share >= 0.3, "the penalty must carry a visible share of the gradient or its loss would pass unseen"
    # both models were penalised at the same points, those of density_points for the step's density key; once without
    # (losses) and once with a backward
    for name in ("coarse", "fine"):
        assert len(points[name]) == 2
        for x, d in points[name]:
            assert torch.equal(x, coords) and torch.equal(d, dirs)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_backward_accumulates_into_a_filled_gradient(family):
    """ModelBase.backward: grad_flat += dL/dparams.  The buffer is pre-filled with a random vector c whose every leaf has
    the RMS of that leaf's oracle gradient; (buffer - c) must then be the oracle gradient within the family's bound.  An
    overwrite leaves -c (error of order 1), a double add a second gradient."""
    fam = FAMILIES[family]()
    model = fam.make("fine")
    m = PENALTY_POINTS
    params = model.init(dict(params=3))["params"]
    flat = model.flat(params)
    gen = torch.Generator().manual_seed(6)
    if fam.tables:
        _fill_tables(flat, model, gen)
    for _, leaf, lo, hi in R.leaf_ranges(model):
        if leaf == "bias":
            flat[lo:hi] += (torch.randn(hi - lo, generator=gen) * 0.1).cuda()
    x = (torch.rand(m, 3, generator=gen) * 2 - 1).float()
    d = torch.randn(m, 3, generator=gen)
    d = (d / d.norm(dim=-1, keepdim=True)).float()
    g_d = torch.randn(m, generator=gen).float()
    g_c = torch.randn(m, 3, generator=gen).float()
    g_a = {k: torch.rand(m, generator=gen).float() for k in model.AUX_NAMES}

    dt = fam.oracle_dtype
    f_ref = flat.cpu().to(dt).requires_grad_(True)
    rd, rr, raux = R.model_fn_factory(model, fam.rnd)(f_ref)(x.to(dt), d.to(dt))
    loss = (rd.reshape(-1) * g_d.to(dt)).sum() + (rr * g_c.to(dt)).sum() + sum((raux[k] * g_a[k].to(dt)).sum() for k in g_a)
    (g_ref,) = torch.autograd.grad(loss, f_ref)
    g_ref = g_ref.double()

    c = torch.zeros_like(g_ref)
    for _, _, lo, hi in R.leaf_ranges(model):
        c[lo:hi] = torch.randn(hi - lo, generator=gen, dtype=F64) * g_ref[lo:hi].pow(2).mean().sqrt()
    c32 = c.float()
    grad = c32.cuda().clone()
    _, _, _, ctx = model.forward_points(flat, x.cuda(), d.cuda(), save=True)
    model.backward(ctx, g_d.cuda(), g_c.cuda(), {k: v.cuda() for k, v in g_a.items()} if g_a else None, grad)
    if ctx.get("ls_scratch") is not None:
        from learn_nerf.model import ls_status

        assert ls_status(ctx) == 0
    added = grad.cpu().double() - c32.double()
    rel = R.rel_l2(added, g_ref)
    print(f"{family}: (buffer - prefill) vs oracle rel L2 err {rel:.2e}; prefill norm {c.norm().item():.3e}, gradient norm "
          f"{g_ref.norm().item():.3e}; per leaf: " + " ".join(f"{k}={v:.1e}" for k, v in R.per_layer_rel(model, added, g_ref)))
    assert c.norm() > 0.5 * g_ref.norm()
    assert rel < fam.gtol, (family, rel)


# ---------------------------------------------------------------- C: the two-stream backward
def test_ref_nerf_two_stream_backward_is_bit_identical_to_one_stream(monkeypatch):
    """The fused Ref-NeRF backward is bit-reproducible (test_ref_nerf_fused_backward_is_bit_reproducible), the coarse and
    the fine gradient slices are disjoint, and the background gradient is two addends into a zeroed word (the fold's last
    add is atomic, so their order does not matter): moving the coarse backward to the second stream changes no bit."""
    fam = FAMILIES["refnerf-fused"]()
    ends = {}
    for env in ("0", "1"):
        monkeypatch.setenv("LNRF_OVERLAP_BACKWARD", env)
        loop = build_loop(fam, init_rng=8)
        assert loop.overlap_backward == (env == "1")
        step = loop.step_fn(BMIN, BMAX)
        grads = []
        for it in range(2):
            step(100 + it, batch().cuda())
            grads.append(loop.grad.clone())
        torch.cuda.synchronize()
        assert (loop._side_stream is not None) == (env == "1")
        ends[env] = grads + [loop.flat.clone(), loop.state.opt_m.clone(), loop.state.opt_v.clone()]
    assert ends["0"][0].abs().max().item() > 0 and ends["0"][0][-3:].abs().min().item() > 0
    for name, a, b in zip(("grad step 0", "grad step 1", "flat", "opt_m", "opt_v"), ends["0"], ends["1"]):
        assert torch.equal(a[-3:], b[-3:]), (name, "background", a[-3:], b[-3:])
        assert torch.equal(a, b), name


def test_nerf_step_with_two_stream_backward_matches_oracle(monkeypatch):
    """LNRF_OVERLAP_BACKWARD=1 with fused NeRFModels: the paired layer-stationary launch gives way to one launch per model,
    each on its own stream with its own scratch block."""
    import learn_nerf.model as M

    monkeypatch.setenv("LNRF_OVERLAP_BACKWARD", "1")
    pair_calls = []
    monkeypatch.setattr(M, "backward_ls_pair", lambda *a, **k: pair_calls.append(a) or pytest.fail("pair launch taken"))
    fam = FAMILIES["nerf-fused-ls"]()
    loop = build_loop(fam)
    assert loop.overlap_backward and loop.coarse.backward_kernel == "ls"
    seen = capture_backward_contexts(loop)
    run_steps(loop, fam, steps=2, key0=100, label="nerf overlap")
    assert not pair_calls and loop._side_stream is not None
    assert len(seen["coarse"]) == len(seen["fine"]) == 2
    ctx_c, ctx_f = seen["coarse"][-1], seen["fine"][-1]
    assert ctx_c["kind"] == ctx_f["kind"] == "fused"
    assert ctx_c["ls_scratch"] is not None and ctx_f["ls_scratch"] is not None
    assert ctx_c["ls_scratch"].data_ptr() != ctx_f["ls_scratch"].data_ptr()
    assert M.ls_status(ctx_c) == 0 and M.ls_status(ctx_f) == 0


@pytest.mark.parametrize("family", ["ngp-fp32", "ngp-bf16"])
def test_ngp_step_with_two_stream_backward_matches_oracle(family, monkeypatch):
    monkeypatch.setenv("LNRF_OVERLAP_BACKWARD", "1")
    fam = FAMILIES[family]()
    loop = build_loop(fam, init_rng=4)
    assert loop.overlap_backward
    # the loss bounds of test_ngp_train_step_matches_oracle
    run_steps(loop, fam, steps=1, key0=77, ltol=1e-5 if fam.precision == "fp32" else 2e-4, label=f"{family} overlap")
    assert loop._side_stream is not None

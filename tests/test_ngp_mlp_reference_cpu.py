"""
CPU tests of tests/ngp_mlp_reference.py: the float64 emulation of the fused InstantNGP MLP kernels is tied to the oracle,
the safe-share condition holds for every parametrisation test_gpu_ngp_mlp_kernel.py runs, and the checker passes a CPU
fp32 simulation of the kernels' outputs but fails each of nine deliberate defects of it.
"""
import functools

import numpy as np
import pytest
import torch

import ngp_mlp_reference as R
from oracle import instant_ngp as ON
from oracle.model import bf16_round

SIM_WG = 3  # workgroups of the simulated persistent backward
SIM_M = 256 * (2 * SIM_WG + 3) - 5  # the GPU test's multi-group shape at 3 "CUs": 2 or 3 groups per workgroup, ragged


def _oracle(flat, enc, d, rnd=None):
    """oracle.instant_ngp.ngp_model with its hash-grid lookups replaced by columns of `enc` [m, lf] (a leaf)"""
    lf = enc.shape[1]
    calls = []

    def fake(x, table, g, t, bmin, bmax, smooth):
        calls.append(1)
        i = len(calls) - 1
        return enc[:, 2 * i:2 * i + 2]

    real = ON.hash_table_encoding
    ON.hash_table_encoding = fake
    try:
        return ON.ngp_model(flat, torch.zeros(enc.shape[0], 3, dtype=enc.dtype), d, [0] * (lf // 2), [2] * (lf // 2),
                            (0.0,) * 3, (1.0,) * 3, operand_round=rnd)[:2]
    finally:
        ON.hash_table_encoding = real


@pytest.mark.parametrize("lf", [2, 16, 18, 32])
def test_unrounded_emulation_is_the_oracle_model_and_its_autograd(lf):
    m = 97
    flat = R.flax_params(lf, 0, seed=lf, bias_std=0.1)
    enc_t, d, gd, gc = R.inputs(lf, m, seed=lf + 1)
    em = R.emulate(flat, 0, enc_t, d, gd, gc, rnd=lambda v: np.asarray(v, np.float64))
    f = torch.from_numpy(flat).double().requires_grad_(True)
    enc = torch.from_numpy(enc_t).double().t().contiguous().requires_grad_(True)
    dens, rgb = _oracle(f, enc, torch.from_numpy(d).double())
    assert np.abs(dens[:, 0].detach().numpy() - em["density"]).max() < 1e-12 * (1 + em["density"].max())
    assert np.abs(rgb.detach().numpy() - em["rgb"]).max() < 1e-12
    g_flat, g_enc = torch.autograd.grad((dens[:, 0] * torch.from_numpy(gd).double()).sum() +
                                        (rgb * torch.from_numpy(gc).double()).sum(), (f, enc))
    ours = R.dense_vector(R.wgrad_reference(em), lf)
    scale = 1 + np.abs(ours).max()
    assert np.abs(g_flat.numpy() - ours).max() < 1e-12 * scale
    assert np.abs(g_enc.numpy() - em["g_enc"]).max() < 1e-12 * scale


@pytest.mark.parametrize("lf", [2, 16, 18, 32])
def test_operand_rounding_only_is_the_bf16_operand_oracle(lf):
    m = 97
    flat = R.flax_params(lf, 0, seed=lf, bias_std=0.1)
    enc_t, d, gd, gc = R.inputs(lf, m, seed=lf + 1)
    via_f32 = lambda v: bf16_round(torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))).numpy()  # noqa: E731
    em = R.emulate(flat, 0, enc_t, d, gd, gc, rnd=via_f32)
    dens, rgb = _oracle(torch.from_numpy(flat).double(), torch.from_numpy(enc_t).double().t().contiguous(),
                        torch.from_numpy(d).double(), rnd=bf16_round)
    assert np.abs(dens[:, 0].numpy() - em["density"]).max() < 1e-12 * (1 + em["density"].max())
    assert np.abs(rgb.numpy() - em["rgb"]).max() < 1e-12


def test_layer_tables_match_the_host_build_of_ngp_layout():
    assert R.host_parts() == R.WGRAD_PARTS
    assert [R.dense_params(lf) for lf in (2, 16, 32)] == [2 * 64 + 64 + 64 * 16 + 16 + 40 * 64 + 64 + 64 * 64 + 64 + 64 * 3 + 3 +
                                                          (lf - 2) * 64 for lf in (2, 16, 32)]


def test_margin_is_the_distance_to_the_nearest_rounding_boundary():
    # bf16 spacing is 2^-7 above 1 and 2^-8 below it, 2^-6 in [2, 4), 2^-28 just below 2^-20
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 - 2.0 ** -12, -3.0, 2.0 ** -20])
    assert R.margin(v).tolist() == [2.0 ** -9, 0.0, 2.0 ** -12, 2.0 ** -7, 2.0 ** -29]
    assert R.margin(v, relu=True).tolist() == [2.0 ** -9, 0.0, 2.0 ** -12, 3.0, 2.0 ** -29]
    assert R.margin(np.array([0.0]), relu=True)[0] == 0.0
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-42, 3, 20000), [0.0, 2.0 ** -133, 2.0 ** -134, 2.0 ** -126],
                        np.ldexp(1.0, np.arange(-120, 8)) * (1 - 2.0 ** -9), np.ldexp(1.0, np.arange(-120, 8)) * (1 - 2.0 ** -10)])
    assert np.array_equal(R.round_margin(x)[0], R.bf16_rne(x)) and np.array_equal(R.round_margin(-x)[0], R.bf16_rne(-x))
    for x in rng.standard_normal(2000):
        mg = R.margin(np.array([x]))[0]
        assert R.bf16_rne(x - 0.999 * mg) == R.bf16_rne(x) == R.bf16_rne(x + 0.999 * mg)
        assert R.bf16_rne(x - 1.001 * mg) != R.bf16_rne(x) or R.bf16_rne(x + 1.001 * mg) != R.bf16_rne(x)


# ---- the safe-share condition, for every parametrisation of the GPU file ------------------------------------------------
@pytest.mark.parametrize("lf", [2, 16, 18, 32])
def test_safe_share_of_the_construction(lf):
    """20 000 evaluations, one seed, no retry: the share the construction gives (DESIGN.md quotes these)"""
    flat = R.sparse_params(lf, 6, seed=lf)
    enc_t, d, gd, gc = R.inputs(lf, 20000, seed=lf + 1)
    em = R.emulate(flat, 6, enc_t, d, gd, gc)
    share = em["safe"].mean()
    worst = {k: float(((mg > dl).reshape(em["m"], -1).all(1)).mean()) for k, (v, dl, mg, _) in em["points"].items()}
    print(f"lf={lf}: safe share {share:.3f}; per rounding point {worst}")
    assert share >= R.SAFE_SHARE_MIN


@pytest.mark.parametrize("case", R.gpu_cases(256), ids=lambda c: f"lf{c[0]}-m{c[1]}-off{c[2]}")
def test_safe_share_of_every_gpu_parametrisation(case):
    lf, m, off, seed = case
    *_, safe = R.safe_share_inputs(lf, m, off, seed)
    assert safe.mean() >= R.SAFE_SHARE_MIN and safe.sum() >= 1


# ---- the checker against the CPU fp32 simulation and its mutations ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sim_problem(lf):
    off = 6
    flat, enc_t, d, gd, gc, fw, safe = R.safe_share_inputs(lf, SIM_M, off, seed=5 * lf)
    em, safe, active, gd, gc = R.safe_problem(flat, off, enc_t, d, gd, gc, fw=fw, safe=safe)
    full = R.emulate(flat, off, enc_t, d, gd, gc)  # margins of the masked problem: no safe evaluation stops being safe
    assert (full["safe"] | ~safe).all() and active.sum() == safe.sum()
    return off, flat, enc_t, d, em, safe, active, gd, gc


def run_checker(lf, mutation=None, pick=None):
    off, flat, enc_t, d, em, safe, active, gd, gc = sim_problem(lf)
    out = R.simulate(flat, off, enc_t, d, gd, gc, SIM_WG, mutation=mutation, pick=pick)
    what = f"simulation lf={lf} m={SIM_M} mutation={mutation}"
    R.check_forward(em, out["density"], out["rgb"], R.LIBM_ALLOWANCE, R.LIBM_ALLOWANCE, what)
    return R.check_backward(em, active, SIM_WG, out["g_enc_t"], out["level_absmax"], out["dense_grad"], what)


@pytest.mark.parametrize("lf", [16, 32])
def test_checker_passes_the_fp32_simulation(lf):
    ratios = run_checker(lf)
    print({k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0


def _pick(lf, mutation):
    off, flat, enc_t, d, em, safe, active, gd, gc = sim_problem(lf)
    act = np.flatnonzero(active)
    if mutation == "drop_eval":
        return (int(act[len(act) // 2]),)
    if mutation == "relu_sign":  # an active evaluation and a unit with c2 == 0 whose unmasked gradient is the largest
        c2 = em["X"][4]
        un = np.abs(em["DY"][4] @ em["W"][4].T) * (c2 == 0) * active[:, None]
        e, u = np.unravel_index(un.argmax(), un.shape)
        assert un[e, u] > 0
        return int(e), int(u)
    return None


def test_simulation_roundings_are_the_reference_ones():
    x = torch.randn(4096, dtype=torch.float64) * 10.0 ** torch.randint(-6, 3, (4096,)).double()
    x32 = x.float()
    assert np.array_equal(R._bf(x32).double().numpy(), R.bf16_rne(x32.double().numpy()))
    assert np.array_equal(R._bf_trunc(x32).double().numpy(), R.bf16_trunc(x32.double().numpy()))


MUTATIONS = ["wacc_zeroed", "drop_eval", "drop_ragged_tile", "row_not_folded", "db_one_half", "dy_trunc", "relu_sign",
             "genc_swap", "lmax_last_group"]


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("lf", [16, 32])
def test_checker_fails_every_mutation(lf, mutation):
    off, flat, enc_t, d, em, safe, active, gd, gc = sim_problem(lf)
    assert active[SIM_M - SIM_M % 32:].any(), "the ragged tile must hold an evaluation with upstream gradient"
    with pytest.raises(AssertionError, match="gradient: |g_enc_t: |level_absmax "):
        run_checker(lf, mutation, _pick(lf, mutation))


def test_admissible_rounding_check_passes_the_simulation_and_sees_1e4():
    """the unsafe evaluations, tightly: the fp32 simulation matches the emulation under an admissible rounding of each
    evaluation's near-boundary points; an rgb of one unsafe evaluation moved by 1e-4 (far inside the 2e-3 gate) does not"""
    lf, off, m = 16, 6, 20000
    flat = R.sparse_params(lf, off, 3)
    enc_t, d, gd, gc = R.inputs(lf, m, 4)
    fw = R.forward(flat, off, enc_t, d)
    out = R.simulate(flat, off, enc_t, d, gd * 0, gc * 0, SIM_WG)
    args = (fw, flat, off, enc_t, d, out["density"], out["rgb"], R.LIBM_ALLOWANCE, R.LIBM_ALLOWANCE, "simulation")
    n, n_other, n_many = R.check_forward_admissible(*args)
    assert n == (~fw["safe"]).sum() > 1000 and n_many <= n // 100
    out["rgb"][np.flatnonzero(~fw["safe"])[5], 1] += 1e-4
    with pytest.raises(AssertionError, match="NO admissible rounding"):
        R.check_forward_admissible(*args)


def test_generated_inputs_carry_no_flip_hazard_and_keep_the_loose_gate_attainable():
    """Raw draws contain evaluations on which a correct kernel may miss the 2e-3 gate of the unsafe evaluations (about 1 %);
    the generator redraws exactly those.  What it returns has none, still has unsafe evaluations, and the fp32 simulation —
    which takes other admissible roundings than the emulation on some of them — stays inside the gate."""
    lf, off, m = 16, 6, 20000
    flat = R.sparse_params(lf, off, 9)
    enc_t, d, _, _ = R.inputs(lf, m, 10)
    raw = R.flip_hazard(R.forward(flat, off, enc_t, d), flat, off, enc_t, d)
    assert 0 < raw.mean() < 0.03
    flat, enc_t, d, gd, gc, fw, safe = R.safe_share_inputs(lf, m, off, seed=9)
    again = R.forward(flat, off, enc_t, d)  # the generator patches its forward block by block: it must be THE forward
    assert all(np.array_equal(fw[k], again[k]) for k in ("safe", "density", "rgb", "logit_delta", "a4_delta"))
    assert not R.flip_hazard(again, flat, off, enc_t, d).any()
    assert np.array_equal(R.backward(again, gd, gc)["safe"], safe) and safe.mean() >= R.SAFE_SHARE_MIN
    assert (~again["safe"]).mean() > 0.15
    out = R.simulate(flat, off, enc_t, d, gd * 0, gc * 0, SIM_WG)
    assert R.check_forward_unsafe(again, out["density"], out["rgb"], "simulation") == (~again["safe"]).sum()
    n, n_other, _ = R.check_forward_admissible(again, flat, off, enc_t, d, out["density"], out["rgb"], R.LIBM_ALLOWANCE,
                                               R.LIBM_ALLOWANCE, "simulation")
    print(f"{n} unsafe evaluations, the simulation rounds {n_other} of them another admissible way")

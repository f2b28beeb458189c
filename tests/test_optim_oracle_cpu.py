"""The float64 optimizer oracle (tests/optim_oracle.py) against torch.optim, and its power to
reject wrong updates on the exact inputs the GPU kernel tests (test_optim_gpu.py) use."""
import pytest
import torch

import optim_oracle as O

N = 1027  # the largest of the small sizes of test_optim_gpu.py


def _rel(a, b):
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("name", list(O.ALL_SGD_FLAGS))
def test_sgd_oracle_matches_torch(name):
    h = O.ALL_SGD_FLAGS[name]
    st = O.make_state(N, seed=11)
    p = st["p"].double()
    ref = p.clone().requires_grad_()
    opt = torch.optim.SGD([ref], lr=O.f32(h["lr"]), momentum=O.f32(h["momentum"]),
                          dampening=O.f32(h["dampening"]), weight_decay=O.f32(h["weight_decay"]),
                          nesterov=h["nesterov"], maximize=h["maximize"])
    buf = None
    for step in range(O.STEPS):
        g = O.make_grad(N, 11, step).double()
        ref.grad = g * O.f32(h["grad_scale"])
        opt.step()
        out, bound = O.sgd_step(p, g, buf, h, first_step=step == 0)
        p, buf = out["p"], out.get("buf")
        assert _rel(p, ref.detach()) <= 1e-12
        if h["momentum"]:
            assert _rel(buf, opt.state[ref]["momentum_buffer"]) <= 1e-12
        assert all(bool((b > 0).all()) for b in bound.values())


@pytest.mark.parametrize("name", list(O.ALL_ADAM_FLAGS))
def test_adam_oracle_matches_torch(name):
    h = O.ALL_ADAM_FLAGS[name]
    st = {k: t.double() for k, t in O.make_state(N, seed=12).items()}
    ref = st["p"].clone().requires_grad_()
    cls = torch.optim.AdamW if h["decoupled"] else torch.optim.Adam
    opt = cls([ref], lr=O.f32(h["lr"]), betas=(O.f32(h["beta1"]), O.f32(h["beta2"])),
              eps=O.f32(h["eps"]), weight_decay=O.f32(h["weight_decay"]), amsgrad=h["amsgrad"],
              maximize=h["maximize"], foreach=False)
    state = {"step": torch.tensor(float(O.ADAM_T0 - 1)), "exp_avg": st["m"].clone(),
             "exp_avg_sq": st["v"].clone()}
    if h["amsgrad"]:
        state["max_exp_avg_sq"] = st["vmax"].clone()
    opt.state[ref] = state
    p, m, v, vmax = st["p"], st["m"], st["v"], st["vmax"]
    for step in range(O.STEPS):
        g = O.make_grad(N, 12, step).double()
        ref.grad = g * O.f32(h["grad_scale"])
        opt.step()
        bc1, bc2s = O.bias_corrections(h["beta1"], h["beta2"], O.ADAM_T0 + step, True)
        out, bound = O.adam_step(p, g, m, v, vmax, h, bc1, bc2s)
        p, m, v = out["p"], out["m"], out["v"]
        assert _rel(p, ref.detach()) <= 1e-12
        assert _rel(m, opt.state[ref]["exp_avg"]) <= 1e-12
        assert _rel(v, opt.state[ref]["exp_avg_sq"]) <= 1e-12
        if h["amsgrad"]:
            vmax = out["vmax"]
            assert _rel(vmax, opt.state[ref]["max_exp_avg_sq"]) <= 1e-12
        assert all(bool((b > 0).all()) for b in bound.values())


def test_seeded_vmax_straddles_new_v():
    """amsgrad is only tested if max(vmax, v) takes both branches: about half each."""
    for name in ("amsgrad", "amsgrad_maximize_gscale"):
        h = O.ADAM_FLAGS[name]
        st = O.make_state(N, seed=12)
        bc1, bc2s = O.bias_corrections(h["beta1"], h["beta2"], O.ADAM_T0, False)
        out, _ = O.adam_step(st["p"], O.make_grad(N, 12, 0), st["m"], st["v"], st["vmax"], h,
                             bc1, bc2s)
        above = float((st["vmax"].double() > out["v"]).double().mean())
        assert 0.3 < above < 0.7, above


def test_one_minus_beta_is_exact_in_fp32():
    """The contract difference the oracle's docstring names: 1.f - beta2 is exact, and differs
    from torch's double 1 - 0.999 by 1.29e-5 relative (bounded by 2^-25 beta / (1 - beta))."""
    import numpy as np

    b = np.float32(0.999)
    assert float(np.float32(1) - b) == 1.0 - float(b)
    dev = abs((1.0 - float(b)) - (1.0 - 0.999)) / (1.0 - 0.999)
    assert 1.2e-5 < dev < 2.0 ** -25 * 0.999 / 0.001


# (mutant, optimizer, flag set, step at which it shows)
MUTANTS = [
    ("dampening_ignored", "sgd", "momentum_dampening", 1),
    ("nesterov_dropped", "sgd", "nesterov_wd", 0),
    ("buf_not_initialised", "sgd", "momentum_dampening", 0),
    ("maximize_ignored", "sgd", "maximize_gscale", 0),
    ("grad_scale_after_wd", "sgd", "maximize_gscale", 0),
    ("decay_swapped", "adam", "l2", 0),
    ("decay_swapped", "adam", "decoupled", 0),
    ("eps_inside_sqrt", "adam", "plain", 0),
    ("bc2_not_applied", "adam", "plain", 0),
    ("bc1_not_applied", "adam", "plain", 0),
    ("amsgrad_uses_v", "adam", "amsgrad", 0),
    ("maximize_ignored", "adam", "amsgrad_maximize_gscale", 0),
    ("grad_scale_after_wd", "adam", "amsgrad_maximize_gscale", 0),
    # the hyper-block tests' flag sets, on those tests' inputs (n = 1027, seeds 40 / 50)
    ("dampening_ignored", "sgd_hb", "hyper_block", 1),
    ("buf_not_initialised", "sgd_hb", "hyper_block", 0),
    ("maximize_ignored", "sgd_hb", "hyper_block", 0),
    ("grad_scale_after_wd", "sgd_hb", "hyper_block", 0),
    ("decay_swapped", "adam_hb", "hyper_block", 0),
    ("eps_inside_sqrt", "adam_hb", "hyper_block", 0),
    ("bc2_not_applied", "adam_hb", "hyper_block", 0),
    ("bc1_not_applied", "adam_hb", "hyper_block", 0),
    ("amsgrad_uses_v", "adam_hb", "hyper_block", 0),
    ("maximize_ignored", "adam_hb", "hyper_block", 0),
    ("grad_scale_after_wd", "adam_hb", "hyper_block", 0),
    # the GEMM epilogue's SGD flag sets, on its 132 x 68, K = 8 weight gradient A^T B
    # ("epi_no_momentum_wd" has no flag that a listed mutation touches)
    ("dampening_ignored", "sgd_epi", "epi_momentum_dampening_wd", 1),
    ("buf_not_initialised", "sgd_epi", "epi_momentum_dampening_wd", 0),
    ("nesterov_dropped", "sgd_epi", "epi_nesterov_wd_maximize", 0),
    ("maximize_ignored", "sgd_epi", "epi_nesterov_wd_maximize", 0),
]
EPI_M, EPI_N, EPI_K = 132, 68, 8  # the first ragged shape of the epilogue tests


def _mutant_inputs(kind):
    """(n, state, gradient(step)) as the GPU test of that family builds them."""
    if kind == "sgd_epi":
        n = EPI_M * EPI_N

        def grad(step):
            A, B = O.make_operands(EPI_M, EPI_N, EPI_K, O.EPI_SGD_SEED + step)
            return (A.double().t() @ B.double()).reshape(-1).float()  # exact in fp32

        return n, O.make_state(n, O.EPI_SGD_STATE_SEED), grad
    seed = {"sgd": 11, "adam": 12, "sgd_hb": O.HB_SGD_SEED, "adam_hb": O.HB_ADAM_SEED}[kind]
    return N, O.make_state(N, seed), lambda step: O.make_grad(N, seed, step)


@pytest.mark.parametrize("mutant,kind,name,step", MUTANTS)
def test_mutant_is_rejected(mutant, kind, name, step):
    """Each wrong update differs from the oracle by more than the bound on >= 1 % of the
    elements of the GPU tests' inputs (same seeds, flags, fp32 bias corrections)."""
    n, st, grad = _mutant_inputs(kind)
    if kind.startswith("sgd"):
        h = O.ALL_SGD_FLAGS[name]
        p, buf = st["p"], None
        for s in range(step):  # the kernel's state before `step`: the oracle's, rounded to fp32
            o, _ = O.sgd_step(p, grad(s), buf, h, s == 0)
            p, buf = o["p"].float(), o["buf"].float()
        args = (p, grad(step), buf, h, step == 0)
        out, bound = O.sgd_step(*args)
        bad, _ = O.sgd_step(*args, _mutant=mutant)
    else:
        h = O.ALL_ADAM_FLAGS[name]
        # by value the binding forms the bias corrections from its double betas; opt_step_begin
        # forms them from the hyper block's fp32 betas
        bc1, bc2s = (O.f32(x) for x in O.bias_corrections(h["beta1"], h["beta2"], O.ADAM_T0,
                                                          kind == "adam_hb"))
        args = (st["p"], grad(step), st["m"], st["v"], st["vmax"], h, bc1, bc2s)
        out, bound = O.adam_step(*args)
        bad, _ = O.adam_step(*args, _mutant=mutant)
    seen = torch.zeros(n, dtype=torch.bool)
    for k in out:
        seen |= ~((bad[k] - out[k]).abs() <= bound[k])
    assert float(seen.double().mean()) >= 0.01, (mutant, name, float(seen.double().mean()))
    # the rejection is by orders of magnitude, not marginal: the parameter alone shows it
    assert O.error_ratio(bad["p"], out["p"], bound["p"]) > 100.0

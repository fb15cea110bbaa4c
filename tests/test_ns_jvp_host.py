"""CPU: the truth behind the ns_step tangent-linear tests (`torch.func.jvp` of the restatement
against a central finite difference), the float32 noise floors behind the GPU tolerances of
tests/test_gpu_ns_jvp.py, `IncrementalFourDVar`'s host logic on the restatement and on a
linear model with a closed-form minimiser, and the argument checks of the new ABI calls."""
import pytest
import torch

import ns_jvp_ref as J
import ns_step_torch_ref as R
from conftest import record_err


def test_restatement_jvp_matches_a_central_difference_float64():
    """The project's gradcheck settings: eps 1e-7, atol 1e-5, rtol 1e-4."""
    fields = R.random_sign_fields(2, 5, 4, 11)
    tans = J.tangents((2, 5, 4))
    got = J.RefJvp.full_step_jvp(*fields, *tans, R.DT, R.DX)
    eps = 1e-7
    hi = R.full_step(*[f + eps * t for f, t in zip(fields, tans)], R.DT, R.DX)
    lo = R.full_step(*[f - eps * t for f, t in zip(fields, tans)], R.DT, R.DX)
    for name, a, p, m in zip(("dens", "vel", "pres"), got, hi, lo):
        fd = (p - m) / (2 * eps)
        print(name, float((a - fd).abs().max()), float(fd.abs().max()))
        assert torch.allclose(a, fd, atol=1e-5, rtol=1e-4), name


@pytest.mark.parametrize("op", J.OPS)
def test_float32_jvp_floor_is_logged(op):
    """The float32-vs-float64 JVP error of the restatement: the noise floor of an op; the GPU
    test's bound is BOUND_FACTOR x this."""
    floor = J.case_floor(op)
    record_err(f"ns jvp floor {op}", floor, J.BOUND_FACTOR * floor)
    print(f"floor {op}: {floor:.3e}")
    assert 1e-8 < floor < 1e-5  # the VJP floor's band


def test_rollout_jvp_floor_is_logged_and_chaining_is_the_rollout_jvp():
    floor = J.rollout_floor()
    record_err("ns jvp floor rollout4", floor, J.BOUND_FACTOR * floor)
    print(f"floor rollout4: {floor:.3e}")
    assert 1e-8 < floor < 1e-4
    # chaining step tangents over stored base states (what the device test and the inner loop
    # do) is the JVP of the whole rollout
    fields, tans = J.rollout_inputs()
    got = J.rollout_jvp(J.tangent_fn, R.step_fn, *fields, *tans)
    for a, b in zip(got, J.rollout_truth()):
        assert R.rel_err(a, b) <= 1e-12


def test_incremental_fourdvar_twin_experiment_on_the_restatement():
    r64 = J.twin_gn_truth64()
    r32 = J.twin_gn_run(J.restatement_gn(), torch.float32, torch.device("cpu"))
    for name, r in (("f64", r64), ("f32", r32)):
        print(name, {k: v for k, v in r.items() if k != "cg"}, "cg first/last", r["cg"][:, [0, -1]])
        J.check_twin(r)
    record_err("incremental fourdvar twin J f32 vs f64", abs(r32["J"] - r64["J"]) / r64["J"], 1e-3)
    assert abs(r32["J"] - r64["J"]) <= 1e-3 * r64["J"]


def test_incremental_fourdvar_linear_model_closed_form():
    """step = tangent = adjoint = a per-channel scaling a_c, uniform weights per channel: H is
    diagonal with at most four distinct eigenvalues, so four CG iterations reach
    x* = (w_b x_b + sum_t w a^t y_t) / (w_b + sum_t w a^2t); a second outer iteration starts
    from a vanishing right-hand side (the zero-curvature guard) and must leave x* alone."""
    from pinn_kalman.fourdvar import IncrementalFourDVar
    g = torch.Generator().manual_seed(0)
    B, H, W, T = 2, 5, 6, 3
    a = torch.tensor([0.9, 1.1, -0.7, 0.5], dtype=torch.float64).view(1, 4, 1, 1)
    w = torch.tensor([4.0, 0.0, 2.5, 1.0], dtype=torch.float64).view(1, 1, 4, 1, 1)
    wb = torch.tensor([1.0, 3.0, 0.5, 2.0], dtype=torch.float64).view(1, 4, 1, 1)
    obs = torch.randn(T, B, 4, H, W, generator=g, dtype=torch.float64)
    xb = torch.randn(B, 4, H, W, generator=g, dtype=torch.float64)
    ad, av, ap = a[:, 0:1], a[:, 1:3], a[:, 3:4]

    def step(d, v, p):
        return ad * d, av * v, ap * p

    def linear(d, v, p, v1, xd, xv, xp):
        return ad * xd, av * xv, ap * xp

    fd = IncrementalFourDVar(steps_per_frame=1, step_fn=step, tangent_fn=linear,
                             adjoint_fn=linear)
    num, den = wb * xb, wb.clone()
    for t in range(1, T + 1):
        num = num + w[0] * a ** t * obs[t - 1]
        den = den + w[0] * a ** (2 * t)
    want = num / den
    one = fd.fit(obs, w, xb, wb, outer=1, inner=4)
    two = fd.fit(obs, w, xb, wb, outer=2, inner=4)
    for res in (one, two):
        err = float((res.state0 - want).abs().max() / want.abs().max())
        print("closed form", err, res.cg_residuals[:, -1].tolist())
        assert torch.isfinite(res.state0).all() and torch.isfinite(res.cg_residuals).all()
        assert err <= 1e-10
    assert float((two.state0 - one.state0).abs().max() / want.abs().max()) <= 1e-10
    assert one.history.shape == (2, 3) and two.cg_residuals.shape == (2, 5)
    # an exactly zero right-hand side: p.Hp = 0 gives a zero update, not NaN
    zero = fd.fit(torch.zeros_like(obs), w, torch.zeros_like(xb), wb, outer=1, inner=2)
    assert float(zero.state0.abs().max()) == 0.0 and float(zero.cg_residuals.abs().max()) == 0.0


def test_incremental_fourdvar_refuses_empty_loops():
    fd = J.restatement_gn()
    _, obs, weights, bg, bw = R.twin_problem(torch.float64, torch.device("cpu"))
    with pytest.raises(ValueError):
        fd.fit(obs, weights, bg, bw, outer=0, inner=10)
    with pytest.raises(ValueError):
        fd.fit(obs, weights, bg, bw, outer=3, inner=0)


def test_jvp_argument_errors_are_reported_without_a_device():
    from op import _lib
    dll = _lib.lib.load()
    one = 1  # any non-NULL pointer: validation returns before it is used
    rc = dll.bpk_ns_full_step_jvp_f32(one, one, one, one, one, one, one, one, one, one, one, 2, 1,
                                      5, 0.1, 0.1, None)
    assert rc == 1 and b"planes" in dll.bpk_last_error()
    rc = dll.bpk_ns_full_step_jvp_f32(one, one, one, one, None, None, None, one, one, one, one, 2,
                                      4, 5, 0.1, 0.1, None)
    assert rc == 1 and b"tangent" in dll.bpk_last_error()
    rc = dll.bpk_ns_full_step_jvp_f32(one, one, one, one, one, None, None, one, one, one, None, 2,
                                      4, 5, 0.1, 0.1, None)
    assert rc == 1 and b"workspace" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_density_jvp_f32(one, one, None, None, one, one, 2, 4, 5, 0.1, 0.1, None)
    assert rc == 1 and b"tangent" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_density_jvp_f32(one, one, one, None, one, None, 2, 4, 5, 0.1, 0.1, None)
    assert rc == 1 and b"workspace" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_velocity_jvp_f32(one, one, one, one, one, one, 2, 4, 1, 0.1, 0.1, None)
    assert rc == 1 and b"planes" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_velocity_jvp_f32(one, one, None, None, one, one, 2, 4, 4, 0.1, 0.1,
                                            None)
    assert rc == 1 and b"tangent" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_velocity_jvp_f32(one, one, one, None, one, None, 2, 4, 4, 0.1, 0.1,
                                            None)
    assert rc == 1 and b"workspace" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_pressure_jvp_f32(one, None, None, one, 2, 4, 4, 0.1, 0.1, None)
    assert rc == 1 and b"tangent" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_pressure_jvp_f32(one, one, one, one, 2, 1, 4, 0.1, 0.1, None)
    assert rc == 1 and b"planes" in dll.bpk_last_error()
    for op in (0, 1, 3):
        assert dll.bpk_ns_jvp_workspace_bytes(op, 4, 8, 8) > 0
    assert dll.bpk_ns_jvp_workspace_bytes(2, 4, 8, 8) == 0
    assert dll.bpk_ns_jvp_workspace_bytes(1, 4, 8, 8) == 6 * 4 * 64 * 4
    assert len(R.refused_geometries(dll, lambda name: "_jvp_" in name)) == 4


def test_new_ops_refuse_cpu_tensors():
    from op import ns_step
    d, v, p = torch.zeros(1, 1, 8, 8), torch.ones(1, 2, 8, 8), torch.zeros(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.full_step_jvp(d, v, p, d, v, p, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.full_step_vjp(d, v, p, v, d, v, p, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.update_density_jvp(d, v, d, None, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.update_velocity_jvp(v, p, v, p, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.update_pressure_jvp(p, v, None, v, 0.1, 0.1)

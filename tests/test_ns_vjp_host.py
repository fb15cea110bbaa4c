"""CPU: the differentiable restatement of ns_step (tests/ns_step_torch_ref.py) against the C
oracle, its float64 gradcheck, the float32 noise floors behind the GPU tolerances of
tests/test_gpu_ns_vjp.py, the 4D-Var host logic on the restatement, and the argument checks
of the new ABI calls."""
import numpy as np
import pytest
import torch

import ns_step_torch_ref as R
from conftest import record_err
from oracle import ns_step_ref as O

ORACLE_BOUND = 1e-6  # of max|ref|


def _rel(a, ref):
    return float(np.abs(a.double().numpy() - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_restatement_matches_the_c_oracle(shape, dtype):
    (d, v, p), _ = R.case_inputs(shape)
    dn, vn, pn = d.numpy(), v.numpy(), p.numpy()
    d, v, p = d.to(dtype), v.to(dtype), p.to(dtype)
    pairs = {
        "update_density": (R.update_density(d, v, R.DT, R.DX),
                           O.update_density(dn, vn, R.DT, R.DX)),
        "update_velocity": (R.update_velocity(v, p, R.DT, R.DX),
                            O.update_velocity(vn, pn, R.DT, R.DX, compat=False)),
        "update_pressure": (R.update_pressure(p, v, R.DT, R.DX),
                            O.update_pressure(pn, vn, R.DT, R.DX)),
    }
    full = R.full_step(d, v, p, R.DT, R.DX)
    ref = O.full_step(dn, vn, pn, R.DT, R.DX, compat=False)
    for name, a, r in zip(("dens", "vel", "pres"), full, ref):
        pairs["full_step." + name] = (a, r)
    for name, (a, r) in pairs.items():
        assert a.dtype == dtype and tuple(a.shape) == r.shape
        err = _rel(a, r)
        record_err(f"ns restatement {name} {shape} {dtype}", err, ORACLE_BOUND)
        assert err <= ORACLE_BOUND, (name, err)


def test_restatement_gradcheck_float64():
    (d, v, p) = R.random_sign_fields(2, 5, 4, 11)
    ins = [t.clone().requires_grad_(True) for t in (d, v, p)]
    assert torch.autograd.gradcheck(lambda a, b, c: R.full_step(a, b, c, R.DT, R.DX), ins,
                                    eps=1e-7, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("case", R.CASES)
def test_float32_gradient_floor_is_logged(case):
    """The float32-vs-float64 gradient error of the restatement: the noise floor of a case
    class; the GPU test's bound is BOUND_FACTOR x this."""
    floor = R.case_floor(case)
    record_err(f"ns vjp floor {case}", floor, R.BOUND_FACTOR * floor)
    print(f"floor {case}: {floor:.3e}")
    # float32 rounding through a few dozen operations: anything outside this band means the
    # restatement (or the generator keeping velocities away from 0) broke
    assert 1e-8 < floor < 1e-5


def test_rollout_gradient_floor_is_logged():
    floor = R.rollout_floor()
    record_err("ns vjp floor rollout4", floor, R.BOUND_FACTOR * floor)
    print(f"floor rollout4: {floor:.3e}")
    assert 1e-8 < floor < 1e-4


def test_fourdvar_twin_experiment_on_the_restatement():
    from pinn_kalman.fourdvar import FourDVar
    r64 = R.twin_truth64()
    fd = FourDVar(steps_per_frame=1, dt=R.DT, dx=R.DX, step_fn=R.step_fn)
    r32 = R.twin_run(fd, torch.float32, torch.device("cpu"))
    for name, r in (("f64", r64), ("f32", r32)):
        print(name, r)
        assert r["J"] <= r["J0"] / 10, r
        assert r["err1"] <= r["err0"] / 2, r
        assert r["min_vel"] > 0.3, r  # the window never comes near a sign change
    assert abs(r32["J"] - r64["J"]) <= 1e-3 * r64["J"]


def test_fourdvar_cost_rollout_and_weights():
    from configs._configdict import ConfigDict
    from pinn_kalman import fourdvar
    fd = fourdvar.FourDVar(steps_per_frame=2, dt=R.DT, dx=R.DX, step_fn=R.step_fn)
    truth0, obs, weights, bg, bw = R.twin_problem(torch.float64, torch.device("cpu"))
    traj = fd.rollout(truth0, 2)
    assert traj.shape == (2, 2, 4, 16, 16)
    # frame t = state after (t + 1) * steps_per_frame steps: the twin observations are one
    # step apart
    assert torch.equal(traj[0], obs[1]) and torch.equal(traj[1], obs[3])
    one = fourdvar.FourDVar(steps_per_frame=1, dt=R.DT, dx=R.DX, step_fn=R.step_fn)
    J, j_obs, j_b = one.cost(truth0, obs, weights, bg, bw)
    assert float(j_obs) == 0.0 and float(J) == float(j_b) > 0
    want = 0.5 * float((bw * (truth0 - bg) ** 2).sum())
    assert abs(float(j_b) - want) <= 1e-12 * want
    with pytest.raises(ValueError):
        fd.rollout(truth0[:, :3], 1)
    with pytest.raises(ValueError):
        fourdvar.FourDVar(steps_per_frame=0)
    # weights helper: IdentityKFMeasure / InpaintKFMeasure conventions
    cfg = ConfigDict({"inverse": {"variance": 0.04}})
    mask = torch.zeros(4, 6)
    mask[1:3] = 1
    uf = torch.full((2, 2, 4, 6), 0.5)
    w = fourdvar.observation_weights(cfg, (2, 4, 6), mask=mask, uncer_flow=uf)
    assert w.shape == (1, 2, 4, 4, 6)
    assert torch.allclose(w[0, :, 0], (mask / 0.04).expand(2, 4, 6))
    assert torch.allclose(w[0, :, 1:3], torch.full((2, 2, 4, 6), 4.0))
    assert float(w[0, :, 3].abs().max()) == 0.0  # no pressure pseudo-observation given
    w = fourdvar.observation_weights(cfg, (2, 4, 6), uncer_pres=0.1)
    assert torch.allclose(w[0, :, 0], torch.full((2, 4, 6), 25.0))
    assert torch.allclose(w[0, :, 3], torch.full((2, 4, 6), 100.0))
    with pytest.raises(ValueError):
        fourdvar.observation_weights(cfg, (2, 4, 6), mask=torch.ones(3, 3))


def test_vjp_argument_errors_are_reported_without_a_device():
    from op import _lib
    dll = _lib.lib.load()
    one = 1  # any non-NULL pointer: validation returns before it is used
    rc = dll.bpk_ns_full_step_vjp_f32(one, one, one, one, one, one, one, one, one, one, one, 2, 1,
                                      5, 0.1, 0.1, None)
    assert rc == 1 and b"planes" in dll.bpk_last_error()
    rc = dll.bpk_ns_full_step_vjp_f32(one, one, one, one, None, None, None, one, one, one, one, 2,
                                      4, 5, 0.1, 0.1, None)
    assert rc == 1 and b"cotangent" in dll.bpk_last_error()
    rc = dll.bpk_ns_full_step_vjp_f32(one, one, one, one, one, None, None, one, one, one, None, 2,
                                      4, 5, 0.1, 0.1, None)
    assert rc == 1 and b"workspace" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_density_vjp_f32(one, one, one, None, None, None, one, 2, 4, 5, 0.1, 0.1,
                                           None)
    assert rc == 1 and b"no gradient" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_velocity_vjp_f32(one, one, one, one, one, one, 2, 4, 1, 0.1, 0.1, None)
    assert rc == 1 and b"planes" in dll.bpk_last_error()
    rc = dll.bpk_ns_update_pressure_vjp_f32(one, None, one, None, one, 2, 4, 4, 0.1, 0.1, None)
    assert rc == 1 and b"g_out" in dll.bpk_last_error()
    rc = dll.bpk_ns_cip_vjp_f32(one, 20, one, one, one, one, one, None, one, None, None, 2, 4, 5,
                                0.1, 0.1, None)
    assert rc == 1 and b"go together" in dll.bpk_last_error()
    rc = dll.bpk_ns_gradient_vjp_f32(one, one, None, None, 2, 4, 5, 0.1, 1.0, None)
    assert rc == 1 and b"required" in dll.bpk_last_error()
    assert dll.bpk_ns_vjp_workspace_bytes(0, 4, 8, 8) == 5 * 4 * 64 * 4
    assert dll.bpk_ns_vjp_workspace_bytes(1, 4, 8, 8) == 16 * 4 * 64 * 4
    assert dll.bpk_ns_vjp_workspace_bytes(2, 4, 8, 8) == 0
    assert dll.bpk_ns_vjp_workspace_bytes(3, 4, 8, 8) == 18 * 4 * 64 * 4
    # the forward's and the adjoint's entries share one geometry check: nx = 1, ny = 1, B = -1
    # and a plane of 2^31 sites, whose in-plane index no longer fits the kernels' int
    assert len(R.refused_geometries(dll, lambda name: "_jvp_" not in name)) == 16


def test_ops_keep_refusing_cpu_tensors_with_grad():
    from op import ns_step
    d = torch.zeros(1, 1, 8, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.full_step(d, torch.ones(1, 2, 8, 8), torch.zeros(1, 1, 8, 8), 0.1, 0.1,
                          compat=False)

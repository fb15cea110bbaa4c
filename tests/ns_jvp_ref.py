"""Test helper of the ns_step tangent-linear model (csrc/ns_step_jvp.hip): the JVP cases,
their float64 truth and float32 noise floor (computed once per session, never modified), the
restatement's linear models for `IncrementalFourDVar`, and its twin experiment.

Truth: `torch.func.jvp` of the float64 restatement (tests/ns_step_torch_ref.py) on the CPU.
Error: max|t - t64| / max|t64| per output tensor.  Floor: the same error of the restatement's
float32 CPU JVP, the largest over R.SHAPES and the output tensors of the op.
"""
import torch

import ns_step_torch_ref as R

OPS = ("full_step", "update_density", "update_velocity", "update_pressure")
BOUND_FACTOR = R.BOUND_FACTOR  # the adjoint's: same weights, sums of the same length, FMA
TANGENT_SEED = 5


def tangents(shape):
    """float64 (t_dens, t_vel, t_pres)."""
    B, H, W = shape
    return R.cotangents(B, H, W, TANGENT_SEED)


def op_jvp(ops, op, dens, vel, pres, t_dens, t_vel, t_pres, dt=R.DT, dx=R.DX):
    """Tangents of one op -> tuple of output tangents.  `ops` has
    full_step_jvp(d, v, p, td, tv, tp, dt, dx) and update_*_jvp in their ops' argument
    order."""
    if op == "full_step":
        return tuple(ops.full_step_jvp(dens, vel, pres, t_dens, t_vel, t_pres, dt, dx))
    if op == "update_density":
        return (ops.update_density_jvp(dens, vel, t_dens, t_vel, dt, dx),)
    if op == "update_velocity":
        return (ops.update_velocity_jvp(vel, pres, t_vel, t_pres, dt, dx),)
    if op == "update_pressure":
        return (ops.update_pressure_jvp(pres, vel, t_pres, t_vel, dt, dx),)
    raise KeyError(op)


def _jvp(fn, primals, tans):
    out = torch.func.jvp(fn, tuple(primals), tuple(tans))[1]
    return out if isinstance(out, tuple) else (out,)


class RefJvp:
    """`torch.func.jvp` of the restatement behind the call signatures of op.ns_step."""

    @staticmethod
    def full_step_jvp(d, v, p, td, tv, tp, dt, dx):
        return _jvp(lambda a, b, c: R.full_step(a, b, c, dt, dx), (d, v, p), (td, tv, tp))

    @staticmethod
    def update_density_jvp(d, v, td, tv, dt, dx):
        return _jvp(lambda a, b: R.update_density(a, b, dt, dx), (d, v), (td, tv))[0]

    @staticmethod
    def update_velocity_jvp(v, p, tv, tp, dt, dx):
        return _jvp(lambda a, b: R.update_velocity(a, b, dt, dx), (v, p), (tv, tp))[0]

    @staticmethod
    def update_pressure_jvp(p, v, tp, tv, dt, dx):
        return _jvp(lambda a, b: R.update_pressure(a, b, dt, dx), (p, v), (tp, tv))[0]


_CACHE = {}


def case_inputs(shape, dtype=torch.float64):
    """(fields, tangents) of a shape: the VJP cases' fields, tangents of seed 5."""
    fields, _ = R.case_inputs(shape, dtype)
    return fields, [t.to(dtype) for t in tangents(shape)]


def case_truth(op, shape):
    key = ("truth", op, shape)
    if key not in _CACHE:
        fields, tans = case_inputs(shape)
        _CACHE[key] = op_jvp(RefJvp, op, *fields, *tans)
    return _CACHE[key]


def case_errs(got, truth):
    return [R.rel_err(a, b) for a, b in zip(got, truth)]


def case_floor(op):
    key = ("floor", op)
    if key not in _CACHE:
        worst = 0.0
        for shape in R.SHAPES:
            fields, tans = case_inputs(shape, torch.float32)
            worst = max([worst] + case_errs(op_jvp(RefJvp, op, *fields, *tans),
                                            case_truth(op, shape)))
        _CACHE[key] = worst
    return _CACHE[key]


# ------------------------------------------------------------------ rollout case
def rollout_inputs(dtype=torch.float64):
    fields, _ = R.rollout_inputs(dtype)
    return fields, [t.to(dtype) for t in tangents(tuple(fields[0].shape[i] for i in (0, 2, 3)))]


def rollout_jvp(step_jvp, step, dens, vel, pres, td, tv, tp):
    """Tangents of the R.ROLLOUT_STEPS-step trajectories by chaining step tangents:
    step(d, v, p) -> (d1, v1, p1), step_jvp(d, v, p, v1, td, tv, tp) -> tangents."""
    out = []
    for _ in range(R.ROLLOUT_STEPS):
        d1, v1, p1 = step(dens, vel, pres)
        td, tv, tp = step_jvp(dens, vel, pres, v1, td, tv, tp)
        dens, vel, pres = d1, v1, p1
        out.append((td, tv, tp))
    return tuple(torch.stack(x) for x in zip(*out))


def _rollout_ref(dtype):
    fields, tans = rollout_inputs(dtype)
    return _jvp(lambda a, b, c: R.rollout(a, b, c, R.ROLLOUT_STEPS, R.DT, R.DX), fields, tans)


def rollout_truth():
    """`torch.func.jvp` of the restatement's whole rollout, float64."""
    if "rollout_truth" not in _CACHE:
        _CACHE["rollout_truth"] = _rollout_ref(torch.float64)
    return _CACHE["rollout_truth"]


def rollout_floor():
    if "rollout_floor" not in _CACHE:
        _CACHE["rollout_floor"] = max(case_errs(_rollout_ref(torch.float32), rollout_truth()))
    return _CACHE["rollout_floor"]


# ------------------------------------------------------------------ restatement linear models
def tangent_fn(d, v, p, v1, td, tv, tp):
    """`IncrementalFourDVar(tangent_fn=...)` signature (v1 is not needed here)."""
    return RefJvp.full_step_jvp(d, v, p, td, tv, tp, R.DT, R.DX)


def adjoint_fn(d, v, p, v1, gd1, gv1, gp1):
    """`IncrementalFourDVar(adjoint_fn=...)` signature."""
    _, pull = torch.func.vjp(lambda a, b, c: R.full_step(a, b, c, R.DT, R.DX), d, v, p)
    return pull((gd1, gv1, gp1))


def restatement_gn():
    from pinn_kalman.fourdvar import IncrementalFourDVar
    return IncrementalFourDVar(steps_per_frame=1, dt=R.DT, dx=R.DX, step_fn=R.step_fn,
                               tangent_fn=tangent_fn, adjoint_fn=adjoint_fn)


# ------------------------------------------------------------------ Gauss-Newton twin
TWIN_OUTER, TWIN_INNER = 3, 10


def twin_gn_run(fd, dtype, device):
    """R.twin_run for an `IncrementalFourDVar`: dict of host values read after the fit."""
    truth0, obs, weights, bg, bw = R.twin_problem(dtype, device)
    res = fd.fit(obs, weights, bg, bw, outer=TWIN_OUTER, inner=TWIN_INNER)
    assert res.history.shape == (TWIN_OUTER + 1, 3) and res.history.device == obs.device
    assert res.cg_residuals.shape == (TWIN_OUTER, TWIN_INNER + 1)
    assert res.cg_residuals.device == obs.device
    assert res.trajectory.shape == obs.shape and res.state0.shape == bg.shape
    hist = res.history.double().cpu()
    return dict(J0=float(hist[0, 0]), J=float(hist[-1, 0]), hist=hist[:, 0].tolist(),
                err0=float((bg[:, 0] - truth0[:, 0]).abs().mean()),
                err1=float((res.state0[:, 0] - truth0[:, 0]).abs().mean()),
                min_vel=float(res.trajectory[:, :, 1:3].abs().min()),
                cg=res.cg_residuals.double().cpu())


def twin_gn_truth64():
    """The float64 CPU Gauss-Newton run on the restatement (once per session)."""
    if "twin_gn64" not in _CACHE:
        _CACHE["twin_gn64"] = twin_gn_run(restatement_gn(), torch.float64, torch.device("cpu"))
    return _CACHE["twin_gn64"]


def check_twin(r):
    """The criteria of the Adam twin test (tests/test_ns_vjp_host.py) and monotone descent."""
    assert all(b <= a for a, b in zip(r["hist"], r["hist"][1:])), r["hist"]
    assert r["J"] <= r["J0"] / 10, r
    assert r["err1"] <= r["err0"] / 2, r
    assert r["min_vel"] > 0.3, r
    assert r["J"] <= R.twin_truth64()["J"], (r["J"], R.twin_truth64()["J"])

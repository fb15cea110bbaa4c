"""GPU: the HIP tangent-linear model of ns_step (csrc/ns_step_jvp.hip) behind
`op.ns_step.*_jvp`, the functional adjoint `full_step_vjp`, and `IncrementalFourDVar` on them.

Truth: `torch.func.jvp` of the float64 restatement on the CPU (tests/ns_jvp_ref.py).  The error
is max|t - t64| / max|t64| per output tensor; the bound of an op is BOUND_FACTOR (8) x the
float32 CPU JVP error of the same restatement (its noise floor, the one the host test logs).
The arithmetic is the adjoint's own -- the same weights, sums of the same length in another
order, FMA contraction -- so the factor is the adjoint's.

Shapes are R.SHAPES for the reasons in tests/test_gpu_ns_vjp.py: (2,7,5) non-square, (1,9,70)
a row wider than a 64-site tile with a ragged tail, (3,6,66) nothing far from a border,
(2,16,16) more than one 256-thread block; B >= 2 exercises the velocity planes 2b / 2b+1.
"""
import pytest
import torch

import ns_jvp_ref as J
import ns_step_torch_ref as R
from conftest import record_err

pytestmark = pytest.mark.gpu


class HipJvp:
    """op.ns_step's JVPs with the call signatures of J.RefJvp."""

    @staticmethod
    def full_step_jvp(d, v, p, td, tv, tp, dt, dx):
        from op import ns_step
        return ns_step.full_step_jvp(d, v, p, td, tv, tp, dt, dx)

    @staticmethod
    def update_density_jvp(d, v, td, tv, dt, dx):
        from op import ns_step
        return ns_step.update_density_jvp(d, v, td, tv, dt, dx)

    @staticmethod
    def update_velocity_jvp(v, p, tv, tp, dt, dx):
        from op import ns_step
        return ns_step.update_velocity_jvp(v, p, tv, tp, dt, dx)

    @staticmethod
    def update_pressure_jvp(p, v, tp, tv, dt, dx):
        from op import ns_step
        return ns_step.update_pressure_jvp(p, v, tp, tv, dt, dx)


def _hip_inputs(shape, hip):
    fields, tans = J.case_inputs(shape, torch.float32)
    return [t.to(hip) for t in fields], [t.to(hip) for t in tans]


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("op", J.OPS)
def test_jvp_parity_with_float64_jvp(hip, op, shape):
    fields, tans = _hip_inputs(shape, hip)
    truth = J.case_truth(op, shape)
    bound = J.BOUND_FACTOR * J.case_floor(op)
    errs = J.case_errs(J.op_jvp(HipJvp, op, *fields, *tans), truth)
    for i, e in enumerate(errs):
        record_err(f"ns jvp hip {op} {shape} out{i}", e, bound)
    print(op, shape, [f"{e:.2e}" for e in errs], f"bound {bound:.2e}")
    assert all(e <= bound for e in errs), (errs, bound)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_adjoint_identity_on_the_device(hip, shape):
    """<J t, w> = <t, J^T w> with full_step_jvp and full_step_vjp, dot products in float64.
    Each side is within its parity bound of the float64 value, so the two differ by at most
    e_J sum_k max|J t|_k ||w_k||_1 + e_A sum_k max|J^T w|_k ||t_k||_1 (maxima from the
    float64 truths)."""
    from op import ns_step
    fields, tans = _hip_inputs(shape, hip)
    _, cots = R.case_inputs(shape)
    w = [c.float().to(hip) for c in cots]
    v1 = ns_step.full_step(*fields, R.DT, R.DX, compat=False)[1]
    jt = ns_step.full_step_jvp(*fields, *tans, R.DT, R.DX, v1=v1)
    jtw = ns_step.full_step_vjp(*fields, v1, *w, R.DT, R.DX)
    lhs = sum(float((a.double() * b.double()).sum()) for a, b in zip(jt, w))
    rhs = sum(float((a.double() * b.double()).sum()) for a, b in zip(tans, jtw))
    e_j = J.BOUND_FACTOR * J.case_floor("full_step")
    e_a = R.BOUND_FACTOR * R.case_floor("full_step")
    jt64 = J.case_truth("full_step", shape)
    jtw64 = R.case_truth("full_step", shape)
    bound = (e_j * sum(float(a.abs().max()) * float(b.double().abs().sum())
                       for a, b in zip(jt64, w))
             + e_a * sum(float(jtw64[k].abs().max()) * float(t.double().abs().sum())
                         for k, t in zip(("dens", "vel", "pres"), tans)))
    record_err(f"ns jvp/vjp adjoint identity {shape}", abs(lhs - rhs), bound)
    print(shape, f"<Jt,w> {lhs:.9e} <t,JTw> {rhs:.9e} diff {abs(lhs - rhs):.2e} bound {bound:.2e}")
    assert abs(lhs - rhs) <= bound


def test_rollout_jvp(hip):
    from op import ns_step
    fields, tans = J.rollout_inputs(torch.float32)
    fields, tans = [t.to(hip) for t in fields], [t.to(hip) for t in tans]
    truth = J.rollout_truth()
    bound = J.BOUND_FACTOR * J.rollout_floor()
    got = J.rollout_jvp(
        lambda d, v, p, v1, td, tv, tp: ns_step.full_step_jvp(d, v, p, td, tv, tp, R.DT, R.DX,
                                                              v1=v1),
        lambda d, v, p: ns_step.full_step(d, v, p, R.DT, R.DX, compat=False), *fields, *tans)
    errs = J.case_errs(got, truth)
    for name, e in zip(("dens", "vel", "pres"), errs):
        record_err(f"ns jvp hip rollout4 t_{name}", e, bound)
    print("rollout4", [f"{e:.2e}" for e in errs], f"bound {bound:.2e}")
    assert all(e <= bound for e in errs), (errs, bound)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_structure(hip, shape):
    from op import ns_step
    (d, v, p), (td, tv, tp) = _hip_inputs(shape, hip)
    with torch.no_grad():
        before = ns_step.full_step(d, v, p, R.DT, R.DX, compat=False)
    full = ns_step.full_step_jvp(d, v, p, td, tv, tp, R.DT, R.DX)
    again = ns_step.full_step_jvp(d, v, p, td, tv, tp, R.DT, R.DX)
    given = ns_step.full_step_jvp(d, v, p, td, tv, tp, R.DT, R.DX, v1=before[1])
    with torch.no_grad():
        after = ns_step.full_step(d, v, p, R.DT, R.DX, compat=False)
    for a, b, c in zip(full, again, given):
        assert torch.equal(a, b) and torch.equal(a, c)  # same bits; v1=None == explicit v1
        assert not a.requires_grad
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    # a None tangent equals a zeros tangent bit for bit, in every op
    zd, zv, zp = torch.zeros_like(d), torch.zeros_like(v), torch.zeros_like(p)
    for some, zeros in (((td, None, None), (td, zv, zp)), ((None, tv, None), (zd, tv, zp)),
                        ((None, None, tp), (zd, zv, tp)), ((td, tv, None), (td, tv, zp))):
        for a, b in zip(ns_step.full_step_jvp(d, v, p, *some, R.DT, R.DX),
                        ns_step.full_step_jvp(d, v, p, *zeros, R.DT, R.DX)):
            assert torch.equal(a, b), some
    assert torch.equal(ns_step.update_density_jvp(d, v, td, None, R.DT, R.DX),
                       ns_step.update_density_jvp(d, v, td, zv, R.DT, R.DX))
    assert torch.equal(ns_step.update_density_jvp(d, v, None, tv, R.DT, R.DX),
                       ns_step.update_density_jvp(d, v, zd, tv, R.DT, R.DX))
    assert torch.equal(ns_step.update_velocity_jvp(v, p, tv, None, R.DT, R.DX),
                       ns_step.update_velocity_jvp(v, p, tv, zp, R.DT, R.DX))
    assert torch.equal(ns_step.update_velocity_jvp(v, p, None, tp, R.DT, R.DX),
                       ns_step.update_velocity_jvp(v, p, zv, tp, R.DT, R.DX))
    assert torch.equal(ns_step.update_pressure_jvp(p, v, tp, None, R.DT, R.DX),
                       ns_step.update_pressure_jvp(p, v, tp, zv, R.DT, R.DX))
    assert torch.equal(ns_step.update_pressure_jvp(p, v, None, tv, R.DT, R.DX),
                       ns_step.update_pressure_jvp(p, v, zp, tv, R.DT, R.DX))
    # the density moves nothing else
    t_d1, t_v1, t_p1 = ns_step.full_step_jvp(d, v, p, td, None, None, R.DT, R.DX)
    assert float(t_v1.abs().max()) == 0.0 and float(t_p1.abs().max()) == 0.0
    assert float(t_d1.abs().max()) > 0.0
    # inputs that require grad: the outputs still carry no graph
    out = ns_step.full_step_jvp(d.clone().requires_grad_(True), v, p,
                                td.clone().requires_grad_(True), tv, tp, R.DT, R.DX)
    assert all(not o.requires_grad for o in out)
    assert torch.equal(out[0], full[0])
    # the functional adjoint is the autograd backward's own call
    w = [c.float().to(hip) for c in R.case_inputs(shape)[1]]
    leaves = [t.clone().requires_grad_(True) for t in (d, v, p)]
    outs = ns_step.full_step(*leaves, R.DT, R.DX, compat=False)
    auto = torch.autograd.grad(outs, leaves, w)
    func = ns_step.full_step_vjp(d, v, p, before[1], *w, R.DT, R.DX)
    for a, b in zip(auto, func):
        assert torch.equal(a, b) and not b.requires_grad


def test_refusals(hip):
    from op import ns_step
    (d, v, p), (td, tv, tp) = _hip_inputs((2, 7, 5), hip)
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.full_step_jvp(d.cpu(), v.cpu(), p.cpu(), td.cpu(), None, None, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.full_step_jvp(d, v, p, td.cpu(), None, None, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="full_step_jvp.*float32"):
        ns_step.full_step_jvp(d, v, p, td.double(), tv, tp, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="update_velocity_jvp.*float32"):
        ns_step.update_velocity_jvp(v.double(), p, tv, tp, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="full_step_jvp.*shape"):
        ns_step.full_step_jvp(d, v, p, td, tv[:, :1], tp, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="update_density_jvp.*shape"):
        ns_step.update_density_jvp(d, v, td[:1], tv, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="update_pressure_jvp.*shape"):
        ns_step.update_pressure_jvp(p, v, tp, tv[:, :, :3], R.DT, R.DX)
    with pytest.raises(RuntimeError, match="full_step_jvp.*tangent"):
        ns_step.full_step_jvp(d, v, p, None, None, None, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="update_density_jvp.*tangent"):
        ns_step.update_density_jvp(d, v, None, None, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="full_step_vjp.*cotangent"):
        ns_step.full_step_vjp(d, v, p, v, None, None, None, R.DT, R.DX)
    with pytest.raises(RuntimeError, match="full_step_vjp.*shape"):
        ns_step.full_step_vjp(d, v, p, v[:, :1], td, tv, tp, R.DT, R.DX)


def test_incremental_fourdvar_twin_experiment_on_the_device(hip):
    from pinn_kalman.fourdvar import IncrementalFourDVar
    r64 = J.twin_gn_truth64()
    r = J.twin_gn_run(IncrementalFourDVar(steps_per_frame=1, dt=R.DT, dx=R.DX), torch.float32, hip)
    print("device", {k: v for k, v in r.items() if k != "cg"}, "float64 restatement J", r64["J"])
    record_err("incremental fourdvar twin final J vs float64", abs(r["J"] - r64["J"]) / r64["J"],
               1e-2)
    J.check_twin(r)
    assert abs(r["J"] - r64["J"]) <= 1e-2 * r64["J"], (r["J"], r64["J"])

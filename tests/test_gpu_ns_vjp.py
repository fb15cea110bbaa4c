"""GPU: the HIP adjoint of ns_step (csrc/ns_step_vjp.hip) behind `op.ns_step` autograd, the
differentiable `simulator.rollout` and `FourDVar` on the device.

Truth: float64 CPU autograd of the restatement (tests/ns_step_torch_ref.py).  The error is
max|g - g64| / max|g64| per input tensor; the bound of a case class is BOUND_FACTOR (8) x the
float32 CPU autograd error of the same restatement (its noise floor, computed here by the
same helper the host test logs): the factor covers a gather that sums up to ~40 terms in
another order and FMA contraction the restatement does not have.

Shapes (B, H, W): (2,7,5) non-square, (1,9,70) a row wider than a 64-site tile with a ragged
tail, (3,6,66) nothing far from a border, (2,16,16) more than one 256-thread block; B >= 2
exercises the velocity planes 2b / 2b+1.
"""
import pytest
import torch

import ns_step_torch_ref as R
from conftest import record_err

pytestmark = pytest.mark.gpu


class HipOps:
    """op.ns_step with the call signatures of R.RefOps (compat=False)."""

    @staticmethod
    def full_step(d, v, p, dt, dx):
        from op import ns_step
        return ns_step.full_step(d, v, p, dt, dx, compat=False)

    @staticmethod
    def update_density(d, v, dt, dx):
        from op import ns_step
        return ns_step.update_density(d, v, dt, dx)

    @staticmethod
    def update_velocity(v, p, dt, dx):
        from op import ns_step
        return ns_step.update_velocity(v, p, dt, dx, compat=False)

    @staticmethod
    def update_pressure(p, v, dt, dx):
        from op import ns_step
        return ns_step.update_pressure(p, v, dt, dx)


def _hip_inputs(shape, hip):
    fields, cots = R.case_inputs(shape, torch.float32)
    return [t.to(hip) for t in fields], cots


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("case", R.CASES)
def test_vjp_parity_with_float64_autograd(hip, case, shape):
    fields, cots = _hip_inputs(shape, hip)
    truth = R.case_truth(case, shape)
    bound = R.BOUND_FACTOR * R.case_floor(case)
    grads = R.case_grads(HipOps, case, *fields, cots)
    errs = {k: R.rel_err(grads[k], truth[k]) for k in truth}
    for k, e in errs.items():
        record_err(f"ns vjp hip {case} {shape} d/d{k}", e, bound)
    print(case, shape, {k: f"{e:.2e}" for k, e in errs.items()}, f"bound {bound:.2e}")
    assert all(e <= bound for e in errs.values()), (errs, bound)


def test_unused_outputs_and_inputs(hip):
    """Only the pressure output used: the density input gets no gradient, and a
    non-contiguous cotangent is accepted."""
    from op import ns_step
    (d, v, p), (gd, gv, gp) = _hip_inputs((2, 7, 5), hip)
    d, v, p = [t.requires_grad_(True) for t in (d, v, p)]
    d1, v1, p1 = ns_step.full_step(d, v, p, R.DT, R.DX, compat=False)
    g = torch.autograd.grad((p1 * gp.float().to(hip)).sum(), [d, v, p], allow_unused=True,
                            retain_graph=True)
    assert g[0] is None or float(g[0].abs().max()) == 0.0
    truth = R.case_truth("full_step_pres_only", (2, 7, 5))
    bound = R.BOUND_FACTOR * R.case_floor("full_step_pres_only")
    assert R.rel_err(g[1], truth["vel"]) <= bound and R.rel_err(g[2], truth["pres"]) <= bound
    # non-contiguous cotangent of the density output (a transposed view)
    cot = gd.float().to(hip).transpose(2, 3).contiguous().transpose(2, 3)
    assert not cot.is_contiguous()
    g2 = torch.autograd.grad(d1, [d, v, p], grad_outputs=cot)
    truth = R.case_truth("full_step_dens_only", (2, 7, 5))
    bound = R.BOUND_FACTOR * R.case_floor("full_step_dens_only")
    for a, k in zip(g2, ("dens", "vel", "pres")):
        assert R.rel_err(a, truth[k]) <= bound, k
    # only the density requires grad: the density-stage adjoint alone
    d3 = d.detach().clone().requires_grad_(True)
    d1b = ns_step.full_step(d3, v.detach(), p.detach(), R.DT, R.DX, compat=False)[0]
    g3, = torch.autograd.grad(d1b, d3, grad_outputs=cot)
    assert torch.equal(g3, g2[0])


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_forward_unchanged_and_backward_deterministic(hip, shape):
    from op import ns_step
    (d, v, p), cots = _hip_inputs(shape, hip)
    with torch.no_grad():
        plain = ns_step.full_step(d, v, p, R.DT, R.DX, compat=False)
        plain_ops = (ns_step.update_density(d, v, R.DT, R.DX),
                     ns_step.update_velocity(v, p, R.DT, R.DX, compat=False),
                     ns_step.update_pressure(p, v, R.DT, R.DX))
    dg, vg, pg = [t.clone().requires_grad_(True) for t in (d, v, p)]
    graph = ns_step.full_step(dg, vg, pg, R.DT, R.DX, compat=False)
    graph_ops = (ns_step.update_density(dg, vg, R.DT, R.DX),
                 ns_step.update_velocity(vg, pg, R.DT, R.DX, compat=False),
                 ns_step.update_pressure(pg, vg, R.DT, R.DX))
    for a, b in zip(plain + plain_ops, graph + graph_ops):
        assert b.requires_grad and not a.requires_grad
        assert torch.equal(a, b.detach())
    # compat=True builds no graph and is what it was
    with torch.no_grad():
        c_plain = ns_step.full_step(d, v, p, R.DT, R.DX, compat=True)
    c_graph = ns_step.full_step(dg, vg, pg, R.DT, R.DX, compat=True)
    for a, b in zip(c_plain, c_graph):
        assert not b.requires_grad and torch.equal(a, b)
    assert not ns_step.update_velocity(vg, pg, R.DT, R.DX, compat=True).requires_grad
    # two backward passes: identical bits
    first = R.case_grads(HipOps, "full_step", d, v, p, cots)
    second = R.case_grads(HipOps, "full_step", d, v, p, cots)
    for k in first:
        assert torch.equal(first[k], second[k]), k


def test_rollout_gradient(hip):
    from pinn_kalman import simulator
    fields, w = R.rollout_inputs(torch.float32)
    fields = [t.to(hip) for t in fields]
    truth = R.rollout_truth()
    bound = R.BOUND_FACTOR * R.rollout_floor()
    grads = R.rollout_grads(
        lambda d, v, p, n: simulator.rollout(d, v, p, n, dt=R.DT, dx=R.DX, compat=False),
        *fields, w)
    errs = {k: R.rel_err(grads[k], truth[k]) for k in truth}
    for k, e in errs.items():
        record_err(f"ns vjp hip rollout4 d/d{k}", e, bound)
    print("rollout4", {k: f"{e:.2e}" for k, e in errs.items()}, f"bound {bound:.2e}")
    assert all(e <= bound for e in errs.values()), (errs, bound)
    # stacked [steps, B, ...] trajectories, equal to repeated full_step calls
    from op import ns_step
    with torch.no_grad():
        fs, vs, ps = simulator.rollout(*fields, 2, dt=R.DT, dx=R.DX)
        s1 = ns_step.full_step(*fields, R.DT, R.DX, compat=False)
        s2 = ns_step.full_step(*s1, R.DT, R.DX, compat=False)
    assert fs.shape == (2, 2, 1, 16, 16) and vs.shape == (2, 2, 2, 16, 16)
    assert torch.equal(fs[1], s2[0]) and torch.equal(vs[0], s1[1]) and torch.equal(ps[1], s2[2])


def test_refusals(hip):
    from op import ns_step
    (d, v, p), _ = _hip_inputs((2, 7, 5), hip)
    dg = d.clone().requires_grad_(True)
    out = (torch.empty_like(d), torch.empty_like(v), torch.empty_like(p))
    with pytest.raises(RuntimeError, match="out="):
        ns_step.full_step(dg, v, p, R.DT, R.DX, compat=False, out=out)
    # out= keeps working where no gradient is required
    with torch.no_grad():
        got = ns_step.full_step(dg, v, p, R.DT, R.DX, compat=False, out=out)
    assert got[0] is out[0]
    d1 = ns_step.full_step(dg, v, p, R.DT, R.DX, compat=False)[0]
    g, = torch.autograd.grad(d1.sum(), dg, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        g.sum().backward()
    with pytest.raises(RuntimeError, match="HIP"):
        ns_step.full_step(d.cpu().requires_grad_(True), v.cpu(), p.cpu(), R.DT, R.DX,
                          compat=False)


def test_fourdvar_twin_experiment_on_the_device(hip):
    from pinn_kalman.fourdvar import FourDVar
    r64 = R.twin_truth64()
    r = R.twin_run(FourDVar(steps_per_frame=1, dt=R.DT, dx=R.DX), torch.float32, hip)
    print("device", r, "float64 restatement", r64)
    record_err("fourdvar twin final J vs float64", abs(r["J"] - r64["J"]) / r64["J"], 1e-2)
    assert r["J"] <= r["J0"] / 10, r
    assert r["err1"] <= r["err0"] / 2, r
    assert abs(r["J"] - r64["J"]) <= 1e-2 * r64["J"], (r, r64)

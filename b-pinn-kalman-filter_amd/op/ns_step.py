"""`op.ns_step` -- 2-D Navier-Stokes explicit step on the HIP stencil (csrc/ns_step.hip).

Reference API: op/ns_step.py:19-26 -> ns_step_forward.update_{density,velocity,
pressure}(tensor, tensor, float dt, float dx) (op/ns_step.cpp:45-102); forward
only and out-of-place there.  Here `update_density`, `update_pressure`,
`update_velocity(compat=False)` and `full_step(compat=False)` are also differentiable to
first order (HIP gather adjoints, csrc/ns_step_vjp.hip) when grad mode is on and an input
requires grad; without that they run exactly the forward launches.  A double backward
raises.  `compat=True` stays forward-only and builds no graph.  The linearized step is also
available as functional calls at a given base state: `full_step_jvp` / `update_*_jvp` (the
tangent-linear model, csrc/ns_step_jvp.hip) and `full_step_vjp` (its adjoint).

`compat=True` (default, = reference behaviour) reproduces the unbind-stride quirk
of update_velocity (op/ns_step.cpp:70): for batch >= 2 the u / v views of the
intermediate velocity are read with batch stride H*W, so sample b advects memory
plane b (u) / b+1 (v) of vel_n.  `compat=False` advects the intended planes.

Other reference properties kept: H == W is not required but the plane is indexed
as the reference does (contiguous axis = size(2)); a velocity component exactly
0 produces NaN (CIP divides by sign(u)); dt / dx are rounded to float32.
Lifted: the reference maps the batch to threadIdx.x (B <= 1024); any B works here.
"""
from __future__ import annotations

import functools

import torch

from ._lib import check, lib, ptr, require_hip, stream_ptr


def _check(name, *ts):
    require_hip(*ts, what=f"ns_step.{name}")
    for t in ts:
        if t.dtype != torch.float32:
            raise RuntimeError(f"ns_step.{name}: float32 tensors required, got {t.dtype}")
        if t.ndim != 4:
            raise RuntimeError(f"ns_step.{name}: expected [B, C, H, W] tensors")


def _geo(t):
    B, _, nx, ny = t.shape  # reference: gridDim.x = size(2), gridDim.y = size(3)
    return B, nx, ny


def _workspace(size_fn, op, B, nx, ny, device):
    """size_fn: bpk_ns_workspace_bytes, bpk_ns_vjp_workspace_bytes or bpk_ns_jvp_workspace_bytes
    (forward, adjoint, tangent)."""
    nbytes = size_fn(op, B, nx, ny)
    return torch.empty(max(nbytes // 4, 1), device=device, dtype=torch.float32)


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _cot(g):
    """Cotangent for the ABI: None stays None (NULL), anything else contiguous."""
    return None if g is None else g.contiguous()


def update_density(dens, vel, dt, dx):
    _check("update_density", dens, vel)
    dens, vel = dens.contiguous(), vel.contiguous()
    if _wants_grad(dens, vel):
        return _UpdateDensity.apply(dens, vel, float(dt), float(dx))
    return _update_density(dens, vel, dt, dx)


def _update_density(dens, vel, dt, dx):
    B, nx, ny = _geo(dens)
    out = torch.empty_like(dens)
    ws = _workspace(lib.bpk_ns_workspace_bytes, 0, B, nx, ny, dens.device)
    check(lib.bpk_ns_update_density_f32(dens.data_ptr(), vel.data_ptr(), out.data_ptr(),
                                        ws.data_ptr(), B, nx, ny, float(dt), float(dx),
                                        stream_ptr(dens.device)), "ns_step.update_density")
    return out


def update_velocity(vel, pres, dt, dx, compat=True):
    """compat=False is differentiable (first order); compat=True is the reference's
    forward-only op and builds no autograd graph."""
    _check("update_velocity", vel, pres)
    vel, pres = vel.contiguous(), pres.contiguous()
    if not compat and _wants_grad(vel, pres):
        return _UpdateVelocity.apply(vel, pres, float(dt), float(dx))
    return _update_velocity(vel, pres, dt, dx, compat)


def _update_velocity(vel, pres, dt, dx, compat):
    B, nx, ny = _geo(vel)
    out = torch.empty_like(vel)
    ws = _workspace(lib.bpk_ns_workspace_bytes, 1, B, nx, ny, vel.device)
    check(lib.bpk_ns_update_velocity_f32(vel.data_ptr(), pres.data_ptr(), out.data_ptr(),
                                         ws.data_ptr(), B, nx, ny, float(dt), float(dx),
                                         int(bool(compat)), stream_ptr(vel.device)),
          "ns_step.update_velocity")
    return out


def update_pressure(pres, vel, dt, dx):
    _check("update_pressure", pres, vel)
    pres, vel = pres.contiguous(), vel.contiguous()
    if _wants_grad(pres, vel):
        return _UpdatePressure.apply(pres, vel, float(dt), float(dx))
    return _update_pressure(pres, vel, dt, dx)


def _update_pressure(pres, vel, dt, dx):
    B, nx, ny = _geo(pres)
    out = torch.empty_like(pres)
    check(lib.bpk_ns_update_pressure_f32(pres.data_ptr(), vel.data_ptr(), out.data_ptr(), B, nx,
                                         ny, float(dt), float(dx), stream_ptr(pres.device)),
          "ns_step.update_pressure")
    return out


def full_step(dens, vel, pres, dt, dx, compat=True, out=None):
    """One simulator step (pinn_kalman/simulator.py:55-57) in two fused launches:
    vel' = update_velocity(vel, pres); pres' = update_pressure(pres, vel');
    dens' = update_density(dens, vel').  Bit-identical to the three calls.

    compat=False is differentiable to first order when grad mode is on and an input requires
    grad (backward: csrc/ns_step_vjp.hip; sgn(u), sgn(v) and the upwind indices are constants
    of the derivative); the forward launches and their results are the same with and without
    a graph.  `out=` buffers cannot be saved for backward, so `out=` with a required gradient
    raises.  compat=True is unchanged in every respect: the reference's forward-only op, it
    builds no autograd graph (its cross-sample plane mixing is a quirk nobody differentiates)."""
    _check("full_step", dens, vel, pres)
    dens, vel, pres = dens.contiguous(), vel.contiguous(), pres.contiguous()
    if not compat and _wants_grad(dens, vel, pres):
        if out is not None:
            raise RuntimeError("ns_step.full_step: out= buffers cannot be saved for backward; "
                               "drop out= or call under torch.no_grad()")
        return _FullStep.apply(dens, vel, pres, float(dt), float(dx))
    return _full_step(dens, vel, pres, dt, dx, compat, out)


def _full_step(dens, vel, pres, dt, dx, compat, out):
    B, nx, ny = _geo(dens)
    if out is None:
        out = (torch.empty_like(dens), torch.empty_like(vel), torch.empty_like(pres))
    d1, v1, p1 = out
    check(lib.bpk_ns_full_step_f32(dens.data_ptr(), vel.data_ptr(), pres.data_ptr(), d1.data_ptr(),
                                   v1.data_ptr(), p1.data_ptr(), None, B, nx, ny, float(dt),
                                   float(dx), int(bool(compat)), stream_ptr(dens.device)),
          "ns_step.full_step")
    return d1, v1, p1


# ---- autograd (compat=False): the forward is the launch above, the backward the gather
# adjoints of csrc/ns_step_vjp.hip.  First order only, in the manner of torch's
# once_differentiable but stricter: that decorator arms its error only when a cotangent
# requires grad, so torch.autograd.grad(..., create_graph=True) followed by a backward
# through the gradient would silently drop this op's second-order term.  Here every gradient
# produced under create_graph carries a node that raises when it is differentiated.
class _NoDoubleBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, what, *grads):
        ctx.what = what
        return tuple(g.view_as(g) for g in grads)

    @staticmethod
    def backward(ctx, *_):
        raise RuntimeError(f"{ctx.what}: double backward is not supported -- the backward is a "
                           "hand-written first-order HIP adjoint (once differentiable)")


def once_differentiable(what):
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(ctx, *cots):
            create_graph = torch.is_grad_enabled()
            with torch.no_grad():
                outs = fn(ctx, *cots)
            if not create_graph:
                return outs
            outs = list(outs)
            idx = [i for i, o in enumerate(outs) if o is not None]
            if idx:
                armed = _NoDoubleBackward.apply(
                    what, *[outs[i].detach().requires_grad_(True) for i in idx])
                for i, o in zip(idx, armed):
                    outs[i] = o
            return tuple(outs)
        return wrapper
    return deco


def _density_vjp(dens, vel, g, need_dens, need_vel, dt, dx, what):
    """Raw adjoint of update_density at (dens, vel): cotangent g -> (g_dens, g_vel), None
    where not needed."""
    B, nx, ny = _geo(dens)
    g_dens = torch.empty_like(dens) if need_dens else None
    g_vel = torch.empty_like(vel) if need_vel else None
    ws = _workspace(lib.bpk_ns_vjp_workspace_bytes, 0, B, nx, ny, dens.device)
    check(lib.bpk_ns_update_density_vjp_f32(dens.data_ptr(), vel.data_ptr(), g.data_ptr(),
                                            ptr(g_dens), None, ptr(g_vel), ws.data_ptr(), B, nx,
                                            ny, dt, dx, stream_ptr(dens.device)), what)
    return g_dens, g_vel


def _full_step_vjp(dens, vel, pres, v1, g_d1, g_v1, g_p1, need_dens, dt, dx, what):
    """Raw adjoint of full_step(compat=False): contiguous cotangents (None = zero) ->
    (g_dens or None, g_vel, g_pres); the velocity and pressure gradients come out of one pass
    over the velocity stage."""
    B, nx, ny = _geo(dens)
    g_dens = torch.empty_like(dens) if need_dens else None
    g_vel, g_pres = torch.empty_like(vel), torch.empty_like(pres)
    ws = _workspace(lib.bpk_ns_vjp_workspace_bytes, 3, B, nx, ny, dens.device)
    check(lib.bpk_ns_full_step_vjp_f32(dens.data_ptr(), vel.data_ptr(), pres.data_ptr(),
                                       v1.data_ptr(), ptr(g_d1), ptr(g_v1), ptr(g_p1),
                                       ptr(g_dens), g_vel.data_ptr(), g_pres.data_ptr(),
                                       ws.data_ptr(), B, nx, ny, dt, dx,
                                       stream_ptr(dens.device)), what)
    return g_dens, g_vel, g_pres


class _UpdateDensity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dens, vel, dt, dx):
        ctx.save_for_backward(dens, vel)
        ctx.dt, ctx.dx = dt, dx
        return _update_density(dens, vel, dt, dx)

    @staticmethod
    @once_differentiable("ns_step.update_density")
    def backward(ctx, g):
        dens, vel = ctx.saved_tensors
        g_dens, g_vel = _density_vjp(dens, vel, _cot(g), ctx.needs_input_grad[0],
                                     ctx.needs_input_grad[1], ctx.dt, ctx.dx,
                                     "ns_step.update_density backward")
        return g_dens, g_vel, None, None


class _UpdatePressure(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pres, vel, dt, dx):
        ctx.save_for_backward(vel)
        ctx.dt, ctx.dx = dt, dx
        return _update_pressure(pres, vel, dt, dx)

    @staticmethod
    @once_differentiable("ns_step.update_pressure")
    def backward(ctx, g):
        vel, = ctx.saved_tensors
        B, nx, ny = _geo(vel)
        g = _cot(g)
        g_pres = torch.empty_like(g) if ctx.needs_input_grad[0] else None
        g_vel = torch.empty_like(vel) if ctx.needs_input_grad[1] else None
        check(lib.bpk_ns_update_pressure_vjp_f32(vel.data_ptr(), g.data_ptr(), ptr(g_pres), None,
                                                 ptr(g_vel), B, nx, ny, ctx.dt, ctx.dx,
                                                 stream_ptr(vel.device)),
              "ns_step.update_pressure backward")
        return g_pres, g_vel, None, None


class _UpdateVelocity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vel, pres, dt, dx):
        ctx.save_for_backward(vel, pres)
        ctx.dt, ctx.dx = dt, dx
        return _update_velocity(vel, pres, dt, dx, False)

    @staticmethod
    @once_differentiable("ns_step.update_velocity")
    def backward(ctx, g):
        vel, pres = ctx.saved_tensors
        B, nx, ny = _geo(vel)
        g = _cot(g)
        g_vel = torch.empty_like(vel)  # the pressure gradient is computed from it
        g_pres = torch.empty_like(pres) if ctx.needs_input_grad[1] else None
        ws = _workspace(lib.bpk_ns_vjp_workspace_bytes, 1, B, nx, ny, vel.device)
        check(lib.bpk_ns_update_velocity_vjp_f32(vel.data_ptr(), pres.data_ptr(), g.data_ptr(),
                                                 g_vel.data_ptr(), ptr(g_pres), ws.data_ptr(), B,
                                                 nx, ny, ctx.dt, ctx.dx, stream_ptr(vel.device)),
              "ns_step.update_velocity backward")
        return (g_vel if ctx.needs_input_grad[0] else None), g_pres, None, None


class _FullStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dens, vel, pres, dt, dx):
        d1, v1, p1 = _full_step(dens, vel, pres, dt, dx, False, None)
        ctx.save_for_backward(dens, vel, pres, v1)
        ctx.set_materialize_grads(False)  # an unused output's cotangent stays None
        ctx.dt, ctx.dx = dt, dx
        return d1, v1, p1

    @staticmethod
    @once_differentiable("ns_step.full_step")
    def backward(ctx, g_d1, g_v1, g_p1):
        dens, vel, pres, v1 = ctx.saved_tensors
        g_d1, g_v1, g_p1 = _cot(g_d1), _cot(g_v1), _cot(g_p1)
        if g_d1 is None and g_v1 is None and g_p1 is None:
            return None, None, None, None, None
        need = ctx.needs_input_grad
        if not (need[1] or need[2]):  # dens' is the only output that depends on dens
            if g_d1 is None:
                return None, None, None, None, None
            g_dens, _ = _density_vjp(dens, v1, g_d1, True, False, ctx.dt, ctx.dx,
                                     "ns_step.full_step backward")
            return g_dens, None, None, None, None
        g_dens, g_vel, g_pres = _full_step_vjp(dens, vel, pres, v1, g_d1, g_v1, g_p1, need[0],
                                               ctx.dt, ctx.dx, "ns_step.full_step backward")
        return g_dens, (g_vel if need[1] else None), (g_pres if need[2] else None), None, None


# ---- functional linear models at a given base state (csrc/ns_step_jvp.hip and
# csrc/ns_step_vjp.hip), for callers that apply M or M^T many times at stored states (the
# inner loop of incremental 4D-Var).  compat=False only; outputs carry no autograd graph.
def _linear_args(name, primals, others, kind):
    """Check and detach the primals and their tangents / cotangents (`others`, aligned with
    `primals`, None = zero); at least one of `others` is required."""
    given = [t for t in others if t is not None]
    _check(name, *primals, *given)
    if not given:
        raise RuntimeError(f"ns_step.{name}: at least one {kind} is required (all are None)")
    for p, t in zip(primals, others):
        if t is not None and t.shape != p.shape:
            raise RuntimeError(f"ns_step.{name}: a {kind} must have the shape of its tensor, "
                               f"got {list(t.shape)} for {list(p.shape)}")
    return ([p.detach().contiguous() for p in primals],
            [None if t is None else t.detach().contiguous() for t in others])


def _base_v1(name, v1, vel):
    """The base step's velocity output as the linear models take it."""
    _check(name, v1)
    if v1.shape != vel.shape:
        raise RuntimeError(f"ns_step.{name}: v1 must have the shape of vel, got "
                           f"{list(v1.shape)} for {list(vel.shape)}")
    return v1.detach().contiguous()


def _same_geo(name, *ts):
    geo = {(t.shape[0],) + tuple(t.shape[2:]) for t in ts}
    if len(geo) != 1:
        raise RuntimeError(f"ns_step.{name}: tensors disagree on [B, ., H, W]: "
                           f"{[list(t.shape) for t in ts]}")


def update_density_jvp(dens, vel, t_dens, t_vel, dt, dx):
    """Tangent of update_density at (dens, vel): -> t_out.  A None tangent is zero."""
    (dens, vel), (t_dens, t_vel) = _linear_args("update_density_jvp", (dens, vel),
                                                (t_dens, t_vel), "tangent")
    _same_geo("update_density_jvp", dens, vel)
    B, nx, ny = _geo(dens)
    out = torch.empty_like(dens)
    ws = _workspace(lib.bpk_ns_jvp_workspace_bytes, 0, B, nx, ny, dens.device)
    check(lib.bpk_ns_update_density_jvp_f32(dens.data_ptr(), vel.data_ptr(), ptr(t_dens),
                                            ptr(t_vel), out.data_ptr(), ws.data_ptr(), B, nx, ny,
                                            float(dt), float(dx), stream_ptr(dens.device)),
          "ns_step.update_density_jvp")
    return out


def update_velocity_jvp(vel, pres, t_vel, t_pres, dt, dx):
    """Tangent of update_velocity(compat=False) at (vel, pres): -> t_out."""
    (vel, pres), (t_vel, t_pres) = _linear_args("update_velocity_jvp", (vel, pres),
                                                (t_vel, t_pres), "tangent")
    _same_geo("update_velocity_jvp", vel, pres)
    B, nx, ny = _geo(vel)
    out = torch.empty_like(vel)
    ws = _workspace(lib.bpk_ns_jvp_workspace_bytes, 1, B, nx, ny, vel.device)
    check(lib.bpk_ns_update_velocity_jvp_f32(vel.data_ptr(), pres.data_ptr(), ptr(t_vel),
                                             ptr(t_pres), out.data_ptr(), ws.data_ptr(), B, nx,
                                             ny, float(dt), float(dx), stream_ptr(vel.device)),
          "ns_step.update_velocity_jvp")
    return out


def update_pressure_jvp(pres, vel, t_pres, t_vel, dt, dx):
    """Tangent of update_pressure at (pres, vel): -> t_out (linear in pres, so only vel's
    values enter)."""
    (pres, vel), (t_pres, t_vel) = _linear_args("update_pressure_jvp", (pres, vel),
                                                (t_pres, t_vel), "tangent")
    _same_geo("update_pressure_jvp", pres, vel)
    B, nx, ny = _geo(pres)
    out = torch.empty_like(pres)
    check(lib.bpk_ns_update_pressure_jvp_f32(vel.data_ptr(), ptr(t_pres), ptr(t_vel),
                                             out.data_ptr(), B, nx, ny, float(dt), float(dx),
                                             stream_ptr(pres.device)),
          "ns_step.update_pressure_jvp")
    return out


def full_step_jvp(dens, vel, pres, t_dens, t_vel, t_pres, dt, dx, v1=None):
    """Tangent-linear model of full_step(compat=False) at the base state (dens, vel, pres):
    -> (t_d1, t_v1, t_p1).  A None tangent is zero; at least one is required.  v1: the base
    step's velocity output when the caller has it; None runs the forward launch to get it."""
    (dens, vel, pres), (t_dens, t_vel, t_pres) = _linear_args(
        "full_step_jvp", (dens, vel, pres), (t_dens, t_vel, t_pres), "tangent")
    _same_geo("full_step_jvp", dens, vel, pres)
    if v1 is None:
        v1 = _full_step(dens, vel, pres, dt, dx, False, None)[1]
    else:
        v1 = _base_v1("full_step_jvp", v1, vel)
    B, nx, ny = _geo(dens)
    t_d1, t_v1, t_p1 = torch.empty_like(dens), torch.empty_like(vel), torch.empty_like(pres)
    ws = _workspace(lib.bpk_ns_jvp_workspace_bytes, 3, B, nx, ny, dens.device)
    check(lib.bpk_ns_full_step_jvp_f32(dens.data_ptr(), vel.data_ptr(), pres.data_ptr(),
                                       v1.data_ptr(), ptr(t_dens), ptr(t_vel), ptr(t_pres),
                                       t_d1.data_ptr(), t_v1.data_ptr(), t_p1.data_ptr(),
                                       ws.data_ptr(), B, nx, ny, float(dt), float(dx),
                                       stream_ptr(dens.device)), "ns_step.full_step_jvp")
    return t_d1, t_v1, t_p1


def full_step_vjp(dens, vel, pres, v1, g_d1, g_v1, g_p1, dt, dx):
    """Adjoint of full_step(compat=False) at the base state (dens, vel, pres) with velocity
    output v1: cotangents of (d1, v1, p1) -> (g_dens, g_vel, g_pres).  A None cotangent is
    zero; at least one is required.  The call `_FullStep.backward` makes when every input
    needs its gradient, without a graph."""
    (dens, vel, pres), (g_d1, g_v1, g_p1) = _linear_args(
        "full_step_vjp", (dens, vel, pres), (g_d1, g_v1, g_p1), "cotangent")
    _same_geo("full_step_vjp", dens, vel, pres)
    v1 = _base_v1("full_step_vjp", v1, vel)
    return _full_step_vjp(dens, vel, pres, v1, g_d1, g_v1, g_p1, True, float(dt), float(dx),
                          "ns_step.full_step_vjp")


# low-level kernels (one launch each), exposed for tests and custom pipelines
def gradient(field, dx):
    _check("gradient", field)
    f = field.contiguous()
    if f.shape[1] != 1:
        raise RuntimeError("ns_step.gradient: expects a [B, 1, H, W] scalar field")
    B, nx, ny = _geo(f)
    fx, fy = torch.empty_like(f), torch.empty_like(f)
    check(lib.bpk_ns_gradient_f32(f.data_ptr(), nx * ny, fx.data_ptr(), fy.data_ptr(),
                                  B, nx, ny, float(dx), stream_ptr(f.device)), "ns_step.gradient")
    return fx, fy


def gradient_adjoint(gx, gy, dx):
    """Dx^T gx + Dy^T gy for the stencil of `gradient` (one launch)."""
    _check("gradient_adjoint", gx, gy)
    gx, gy = gx.contiguous(), gy.contiguous()
    B, nx, ny = _geo(gx)
    out = torch.empty_like(gx)
    check(lib.bpk_ns_gradient_adjoint_f32(gx.data_ptr(), gy.data_ptr(), out.data_ptr(), B, nx,
                                          ny, float(dx), stream_ptr(gx.device)),
          "ns_step.gradient_adjoint")
    return out


class _StencilGradient(torch.autograd.Function):
    """(fx, fy) = ns_step stencil gradient of a [B, 1, H, W] field, differentiable to any
    order (the stencil is linear; its backward is the adjoint kernel, whose own backward
    is the stencil again)."""

    @staticmethod
    def forward(ctx, f, dx):
        ctx.dx = dx
        return gradient(f, dx)

    @staticmethod
    def backward(ctx, gx, gy):
        if gx is None:
            gx = torch.zeros_like(gy)
        if gy is None:
            gy = torch.zeros_like(gx)
        return _StencilGradientAdjoint.apply(gx, gy, ctx.dx), None


class _StencilGradientAdjoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gx, gy, dx):
        ctx.dx = dx
        return gradient_adjoint(gx, gy, dx)

    @staticmethod
    def backward(ctx, g):
        fx, fy = _StencilGradient.apply(g, ctx.dx)
        return fx, fy, None


def stencil_gradient(field, dx):
    """Differentiable (d/dx, d/dy) of a [B, 1, H, W] field on the ns_step stencil."""
    return _StencilGradient.apply(field, dx)

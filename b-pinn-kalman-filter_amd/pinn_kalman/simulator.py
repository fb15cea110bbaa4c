"""Navier-Stokes / PINN rollouts (reference pinn_kalman/simulator.py:6-63).

`step(model, begin, t_range, stride)` advances B = 256 replicas of the 192x192 fields
of one snapshot with the ns_step stencil (dt = 0.0025, dx = 1/200), returning the
per-step density, velocity and pressure; `simulate(model, begin, ...)` rolls the PINN
forward (FlowNet flow -> `PINN.step` warp).  `begin` is the dataset array
[T, 6, H, W] (channels x, y, f, u, v, p), cropped as the reference does ([8:200, 4:-4]).

MI355X design: one simulator step is the fused `ns_step.full_step` (two launches,
bit-identical to the reference's three ops), the replicas stay resident in HBM, and the
reference's per-step `print(f)` (a device sync + host transfer of 9.4 M values) is dropped.
"""
from __future__ import annotations

import numpy as np
import torch

from op import ns_step

dt = 0.0005 * 5
dx = 1 / 200


# ---- the field state of the filters and the variational fits (UKF, LETKF, 4D-Var):
# [B, 4, H, W] with channels (f, u, v, p)
def split_state(x):
    """[B, 4, H, W] -> contiguous (f [B, 1, H, W], v [B, 2, H, W], p [B, 1, H, W])."""
    return x[:, 0:1].contiguous(), x[:, 1:3].contiguous(), x[:, 3:4].contiguous()


def join_state(f, v, p):
    """Inverse of `split_state`."""
    return torch.cat([f, v, p], dim=1)


def default_step(dt=dt, dx=dx):
    """step_fn(f, v, p) -> (f', v', p'): `ns_step.full_step(compat=False)`, the differentiable
    step (HIP tensors only)."""
    def step_fn(f, v, p):
        return ns_step.full_step(f, v, p, dt, dx, compat=False)
    return step_fn


def advance(step_fn, f, v, p, n, bases=None):
    """n steps of step_fn from (f, v, p), each on contiguous tensors -> (f, v, p).  bases: a
    list that receives every step's base state (f, v, p, v1), v1 being that step's velocity
    output -- what the step's tangent and adjoint take."""
    for _ in range(int(n)):
        f, v, p = f.contiguous(), v.contiguous(), p.contiguous()
        f1, v1, p1 = step_fn(f, v, p)
        if bases is not None:
            bases.append((f, v, p, v1))
        f, v, p = f1, v1, p1
    return f, v, p


def _prep(data, device):
    return torch.from_numpy(np.ascontiguousarray(data[:, 8:200, 4:-4])).to(device).unsqueeze(0)


def simulate(model, begin, t_range=(0, 100), stride=1):
    dev = model.mask_u.device
    t0, _ = t_range
    f1 = _prep(begin[0 + t0, 2:3], dev)
    f2 = _prep(begin[1 + t0, 2:3], dev)
    x = _prep(begin[0 + t0, 0:1], dev)
    y = _prep(begin[0 + t0, 1:2], dev)
    result, vel = [], []
    for t in torch.arange(*t_range, stride):
        t = t.unsqueeze(0).to(dev)
        flow, _ = model(f1, f2, x, y, t, size=(192, 192))
        f = model.step(f2, flow[-1])
        result.append(f)
        vel.append(flow[-1])
        f1, f2 = f2, f
    return result, vel


def rollout(f, v, p, steps, dt=dt, dx=dx, compat=False):
    """`steps` simulator steps from density f [B, 1, H, W], velocity v [B, 2, H, W] and
    pressure p [B, 1, H, W] -> stacked trajectories ([steps, B, 1, H, W], [steps, B, 2, H, W],
    [steps, B, 1, H, W]); entry k is the state after k + 1 steps.  With compat=False the
    rollout is differentiable with respect to f, v and p (`ns_step.full_step`'s HIP adjoint);
    compat=True is the reference's forward-only step and carries no graph."""
    fs, vs, ps = [], [], []
    for _ in range(int(steps)):
        f, v, p = ns_step.full_step(f, v, p, dt, dx, compat=compat)
        fs.append(f)
        vs.append(v)
        ps.append(p)
    return torch.stack(fs), torch.stack(vs), torch.stack(ps)


def step(model, begin, t_range=(0, 100), stride=1, replicas=256, device=None, ctx=None,
         compat=True):
    """ns_step rollout of `replicas` copies of snapshot t_range[0]; velocity channels are
    swapped into (v, u) order as the reference does (simulator.py:52-53).

    ctx (dist.DistContext): batch-sharded over the ranks, no collective -- rank r advances
    replicas [r * R, (r + 1) * R) with R = replicas / world and returns those.
    compat=False: replicas are independent and the shards equal the single-process rollout
    bit for bit.  compat=True (the reference's behaviour): update_velocity's unbind quirk
    (op/ns_step.cpp:70) makes sample b advect velocity planes b and b + 1, i.e. samples
    b / 2 and (b + 1) / 2, so the replicas diverge after the first step and a shard equals
    the reference's own rollout of R replicas -- reproducing the single-process batch would
    need every rank's velocities each step."""
    dev = device if device is not None else model.mask_u.device
    t0, _ = t_range
    if ctx is not None and ctx.enabled:
        if replicas % ctx.world_size:
            raise ValueError(f"replicas {replicas} do not split over {ctx.world_size} ranks")
        replicas //= ctx.world_size
    f = _prep(begin[0 + t0, 2:3], dev).repeat(replicas, 1, 1, 1)
    v = _prep(begin[0 + t0, 3:5], dev)
    v = torch.cat([v[:, 1:2], v[:, 0:1]], 1).repeat(replicas, 1, 1, 1)
    p = _prep(begin[0 + t0, 5:6], dev).repeat(replicas, 1, 1, 1)
    result, vel, pres = [], [], []
    for _ in torch.arange(*t_range, stride):
        f, v, p = ns_step.full_step(f, v, p, dt, dx, compat=compat)
        result.append(f)
        vel.append(v)
        pres.append(p)
    return result, vel, pres

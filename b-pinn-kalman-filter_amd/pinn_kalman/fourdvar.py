"""Strong-constraint 4D-Var on the differentiable simulator step.

The window's initial state x_0 [B, 4, H, W] (channels f, u, v, p as in `UKF`) is fitted to
all frames of the window through the dynamics:

    J(x_0) = 1/2 sum_t w_t (x_t - y_t)^2 + 1/2 w_b (x_0 - x_b)^2,   x_t = M^t(x_0), t = 1..T

where M is `steps_per_frame` simulator steps (`ns_step.full_step(compat=False)`, whose
backward is the HIP adjoint of csrc/ns_step_vjp.hip), `weights` the inverse observation
variances (0 = unobserved) and x_b / w_b the background and its inverse variance.  One
iteration costs one forward and one adjoint sweep over the window and works on the whole
field, where the patch UKF needs 2n + 1 = 129 simulator steps per filter step and treats
the patches as independent.

Everything stays on the device: Adam is written out on tensors and the cost history is a
device tensor, so `fit` never reads a value on the host.

`IncrementalFourDVar` minimises the same cost the way variational assimilation is normally
run: Gauss-Newton outer iterations around the current trajectory, conjugate gradients inside,
each Hessian product one tangent-linear (csrc/ns_step_jvp.hip) and one adjoint sweep.

No reference counterpart (the reference has no adjoint of its step).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from op import ns_step

from . import simulator


@dataclass
class FourDVarResult:
    state0: torch.Tensor      # [B, 4, H, W] fitted initial state
    trajectory: torch.Tensor  # [T, B, 4, H, W] frames of the fitted state
    history: torch.Tensor     # [iters + 1, 3] (J, J_obs, J_b) at iterates 0 .. iters


def observation_weights(config, shape, mask=None, uncer_flow=None, uncer_pres=None,
                        device=None):
    """Inverse-variance `weights` [1, B, 4, H, W] (broadcast over the frames) in the
    conventions of `IdentityKFMeasure` / `InpaintKFMeasure`: the density is observed with
    variance `config.inverse.variance` where `mask` (1 = observed pixel; [H, W] or
    [1, 1, H, W]; None = every pixel) is set, the B-PINN's flow / pressure pseudo-observations
    with variances uncer_flow^2 [B, 2, H, W] / uncer_pres^2 [B, 1, H, W] (standard
    deviations, as `update_uncertainty` takes them; a float applies to every site).  Unlike
    the Kalman measurement, which needs a noise level for every row, a channel whose
    uncertainty is None is unobserved here: weight 0.

    shape: (B, H, W)."""
    B, H, W = shape
    w = torch.zeros(1, B, 4, H, W, device=device)
    dens = torch.full((1, 1, H, W), 1.0 / float(config.inverse.variance), device=device)
    if mask is not None:
        mask = torch.as_tensor(mask, dtype=torch.float32, device=device)
        if mask.ndim == 2:
            mask = mask[None, None]
        if tuple(mask.shape) != (1, 1, H, W):
            raise ValueError(f"observation_weights: mask must be [{H}, {W}] or [1, 1, {H}, {W}], "
                             f"got {list(mask.shape)}")
        dens = dens * mask
    w[0, :, 0:1] = dens

    def inv_var(uncer, channels):
        if not torch.is_tensor(uncer):
            return 1.0 / float(uncer) ** 2
        if tuple(uncer.shape) != (B, channels, H, W):
            raise ValueError(f"observation_weights: uncertainty must be [{B}, {channels}, {H}, "
                             f"{W}], got {list(uncer.shape)}")
        return uncer.to(device=device, dtype=torch.float32) ** -2

    if uncer_flow is not None:
        w[0, :, 1:3] = inv_var(uncer_flow, 2)
    if uncer_pres is not None:
        w[0, :, 3:4] = inv_var(uncer_pres, 1)
    return w


class FourDVar:
    """steps_per_frame simulator steps of size dt between consecutive frames.
    step_fn(f, v, p) -> (f', v', p'): the step; default `ns_step.full_step(compat=False)`
    with this object's dt, dx (HIP tensors only).  A differentiable restatement can be passed
    to run the host logic on other devices or dtypes."""

    def __init__(self, steps_per_frame=1, dt=simulator.dt, dx=simulator.dx, step_fn=None):
        if int(steps_per_frame) < 1:
            raise ValueError("FourDVar: steps_per_frame must be >= 1")
        self.steps_per_frame = int(steps_per_frame)
        self.dt, self.dx = float(dt), float(dx)
        self.step_fn = simulator.default_step(self.dt, self.dx) if step_fn is None else step_fn

    def rollout(self, state0, T):
        """-> [T, B, 4, H, W]: frame t (0-based) is the state after (t + 1) * steps_per_frame
        steps; differentiable with respect to state0."""
        return self._frames(state0, T, None)

    def _frames(self, state0, T, bases):
        """`rollout`; bases: None, or a list that receives the base state (d, v, p, v1) of
        every sub-step in order (`simulator.advance`)."""
        if state0.ndim != 4 or state0.shape[1] != 4:
            raise ValueError(f"FourDVar: state must be [B, 4, H, W], got {list(state0.shape)}")
        fvp = simulator.split_state(state0)
        frames = []
        for _ in range(int(T)):
            fvp = simulator.advance(self.step_fn, *fvp, self.steps_per_frame, bases)
            frames.append(simulator.join_state(*fvp))
        return torch.stack(frames)

    def _cost(self, state0, obsv_seq, weights, background, background_weights):
        traj = self.rollout(state0, obsv_seq.shape[0])
        j_obs = 0.5 * (weights * (traj - obsv_seq) ** 2).sum()
        j_b = 0.5 * (background_weights * (state0 - background) ** 2).sum()
        return j_obs + j_b, j_obs, j_b, traj

    def cost(self, state0, obsv_seq, weights, background, background_weights):
        """-> (J, J_obs, J_b), 0-d tensors.  obsv_seq [T, B, 4, H, W]; weights broadcastable
        to it; background [B, 4, H, W]; background_weights broadcastable to it."""
        return self._cost(state0, obsv_seq, weights, background, background_weights)[:3]

    def fit(self, obsv_seq, weights, background, background_weights, iters=40, lr=5e-3,
            betas=(0.9, 0.999), eps=1e-8):
        """Adam from the background.  No host read: the history is a device tensor."""
        weights = torch.as_tensor(weights, dtype=obsv_seq.dtype, device=obsv_seq.device)
        background_weights = torch.as_tensor(background_weights, dtype=obsv_seq.dtype,
                                             device=obsv_seq.device)
        x = background.detach().clone()
        m, v = torch.zeros_like(x), torch.zeros_like(x)
        b1, b2 = betas
        history = []
        for k in range(1, int(iters) + 1):
            x.requires_grad_(True)
            with torch.enable_grad():
                J, j_obs, j_b, _ = self._cost(x, obsv_seq, weights, background,
                                              background_weights)
                g, = torch.autograd.grad(J, x)
            history.append(torch.stack([J.detach(), j_obs.detach(), j_b.detach()]))
            with torch.no_grad():
                m.mul_(b1).add_(g, alpha=1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                step = lr / (1 - b1 ** k)
                x = x.detach() - step * m / ((v / (1 - b2 ** k)).sqrt() + eps)
        with torch.no_grad():
            J, j_obs, j_b, traj = self._cost(x, obsv_seq, weights, background, background_weights)
        history.append(torch.stack([J, j_obs, j_b]))
        return FourDVarResult(state0=x, trajectory=traj, history=torch.stack(history))


@dataclass
class IncrementalResult(FourDVarResult):
    # history: [outer + 1, 3] nonlinear (J, J_obs, J_b) at outer iterates 0 .. outer
    cg_residuals: torch.Tensor = None  # [outer, inner + 1] |b - H dx| before / after each CG step


class IncrementalFourDVar(FourDVar):
    """Incremental (Gauss-Newton) 4D-Var: the same cost as `FourDVar`, minimised by an outer
    loop that re-linearizes the model around the current trajectory and an inner conjugate-
    gradient loop on the quadratic problem

        H dx = b,   H = B^-1 + sum_t M_t^T W_t M_t,   b = B^-1 (x_b - x_k) + sum_t M_t^T W_t d_t

    with d_t = y_t - x_t the innovations, M_t the tangent-linear model from x_0 to frame t and
    M_t^T its adjoint.  One Hessian product is one tangent-linear sweep forward over the stored
    states and one adjoint sweep back; no nonlinear forward runs inside the inner loop.

    tangent_fn(d, v, p, v1, td, tv, tp) -> (td1, tv1, tp1): the step's tangent at the base
    state (d, v, p) whose velocity output is v1; default `ns_step.full_step_jvp`.
    adjoint_fn(d, v, p, v1, gd1, gv1, gp1) -> (gd, gv, gp): its adjoint; default
    `ns_step.full_step_vjp`.  Both defaults take HIP tensors only; pass all three functions to
    run the host logic on a restatement."""

    def __init__(self, steps_per_frame=1, dt=simulator.dt, dx=simulator.dx, step_fn=None,
                 tangent_fn=None, adjoint_fn=None):
        super().__init__(steps_per_frame, dt, dx, step_fn)
        if tangent_fn is None:
            def tangent_fn(d, v, p, v1, td, tv, tp):
                return ns_step.full_step_jvp(d, v, p, td, tv, tp, self.dt, self.dx, v1=v1)
        if adjoint_fn is None:
            def adjoint_fn(d, v, p, v1, gd1, gv1, gp1):
                return ns_step.full_step_vjp(d, v, p, v1, gd1, gv1, gp1, self.dt, self.dx)
        self.tangent_fn, self.adjoint_fn = tangent_fn, adjoint_fn

    def _linearize(self, state0, T):
        """Nonlinear rollout from state0 -> (frames [T, B, 4, H, W], the base state
        (d, v, p, v1) of every sub-step in order)."""
        states = []
        return self._frames(state0, T, states), states

    def _tangent_sweep(self, states, dx0):
        """M_t dx0 for every frame t -> [T, B, 4, H, W]."""
        t = simulator.split_state(dx0)
        frames = []
        for i, base in enumerate(states):
            t = self.tangent_fn(*base, *t)
            if (i + 1) % self.steps_per_frame == 0:
                frames.append(simulator.join_state(*t))
        return torch.stack(frames)

    def _adjoint_sweep(self, states, cots):
        """sum_t M_t^T cots[t] -> [B, 4, H, W], accumulated backwards over the window."""
        lam = torch.zeros_like(cots[0])
        for i in range(len(states) - 1, -1, -1):
            if (i + 1) % self.steps_per_frame == 0:
                lam = lam + cots[(i + 1) // self.steps_per_frame - 1]
            lam = simulator.join_state(
                *self.adjoint_fn(*states[i], *simulator.split_state(lam)))
        return lam

    def fit(self, obsv_seq, weights, background, background_weights, outer=3, inner=10):
        """`outer` Gauss-Newton iterations from the background, each `inner` plain CG
        iterations from dx = 0 (a fixed count: no host read decides anything).  alpha, beta
        and the residual norms are 0-d device tensors; p.Hp = 0 (a converged system) yields a
        zero update."""
        if int(outer) < 1 or int(inner) < 1:
            raise ValueError("IncrementalFourDVar: outer and inner must be >= 1")
        weights = torch.as_tensor(weights, dtype=obsv_seq.dtype, device=obsv_seq.device)
        bw = torch.as_tensor(background_weights, dtype=obsv_seq.dtype, device=obsv_seq.device)
        T = obsv_seq.shape[0]
        zero, one = obsv_seq.new_zeros(()), obsv_seq.new_ones(())

        def nonlinear(x):
            traj, states = self._linearize(x, T)
            j_obs = 0.5 * (weights * (traj - obsv_seq) ** 2).sum()
            j_b = 0.5 * (bw * (x - background) ** 2).sum()
            return traj, states, torch.stack([j_obs + j_b, j_obs, j_b])

        def ratio(num, den):
            ok = den > 0
            return torch.where(ok, num / torch.where(ok, den, one), zero)

        with torch.no_grad():
            x = background.detach().clone()
            history, residuals = [], []
            for _ in range(int(outer)):
                traj, states, cost = nonlinear(x)
                history.append(cost)

                def hess(vec):
                    return bw * vec + self._adjoint_sweep(
                        states, weights * self._tangent_sweep(states, vec))

                b = bw * (background - x) + self._adjoint_sweep(
                    states, (weights * (obsv_seq - traj)).expand_as(traj))
                dx0, r, p = torch.zeros_like(x), b, b
                rs = (r * r).sum()
                res = [rs.sqrt()]
                for _ in range(int(inner)):
                    hp = hess(p)
                    alpha = ratio(rs, (p * hp).sum())
                    dx0 = dx0 + alpha * p
                    r = r - alpha * hp
                    rs_new = (r * r).sum()
                    p = r + ratio(rs_new, rs) * p
                    rs = rs_new
                    res.append(rs.sqrt())
                residuals.append(torch.stack(res))
                x = x + dx0
            traj, _, cost = nonlinear(x)
            history.append(cost)
        return IncrementalResult(state0=x, trajectory=traj, history=torch.stack(history),
                                 cg_residuals=torch.stack(residuals))

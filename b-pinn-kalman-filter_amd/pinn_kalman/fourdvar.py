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

No reference counterpart (the reference has no adjoint of its step).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

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
        if step_fn is None:
            from op import ns_step

            def step_fn(f, v, p):
                return ns_step.full_step(f, v, p, self.dt, self.dx, compat=False)
        self.step_fn = step_fn

    def rollout(self, state0, T):
        """-> [T, B, 4, H, W]: frame t (0-based) is the state after (t + 1) * steps_per_frame
        steps; differentiable with respect to state0."""
        if state0.ndim != 4 or state0.shape[1] != 4:
            raise ValueError(f"FourDVar: state must be [B, 4, H, W], got {list(state0.shape)}")
        f, v, p = state0[:, 0:1], state0[:, 1:3], state0[:, 3:4]
        frames = []
        for _ in range(int(T)):
            for _ in range(self.steps_per_frame):
                f, v, p = self.step_fn(f.contiguous(), v.contiguous(), p.contiguous())
            frames.append(torch.cat([f, v, p], dim=1))
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

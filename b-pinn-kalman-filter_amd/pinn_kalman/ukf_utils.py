"""UKF models on the ns_step stencil (reference pinn_kalman/ukf_utils.py:8-119).

What the square-root UKF (`pinn_kalman.ukf`, kernels in csrc/ukf.hip) calls on its hot path:
`patch` / `unpatch` (the state layout of p x p field patches), `NSDynamics.forward`, which
advances the unpatched fields by one simulator step -- update_velocity, update_pressure,
update_density (ukf_utils.py:109-111) -- here the fused `ns_step.full_step` (bit-identical to
the three calls), and returns the re-patched state with the reference's constant process
noise 1e-8 I, and `IdentityKFMeasure`, the identity observation model with per-channel noise
(`InpaintKFMeasure`: the same with the density channel seen through a pixel mask).
All are plain nn.Modules with the torchfilter model call contract (`state_dim`,
`forward(states, ...) -> (states, noise)`); the second value is consumed by the filter as a
lower-triangular square-root factor [rows, dim, dim].  The debug prints of the reference
(NaN/inf checks, each a device sync) are dropped.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from op import ns_step

from .simulator import join_state, split_state

DT = 0.0005 * 5  # reference ukf_utils.py:105-106 (the simulator's dt / dx)
DX = 1 / 200


def patch(x, p_size):
    """[B, C, H, W] -> [C * B * (H/p) * (W/p), p * p]: rows ordered (channel, sample,
    patch row, patch col) (reference ukf_utils.py:8-15)."""
    x = x.transpose(0, 1)
    x = x.unfold(2, p_size, p_size).unfold(3, p_size, p_size)
    return x.reshape(-1, p_size ** 2)


def unpatch(x, p_size, f_size, channel_num=6):
    """Inverse of `patch` (reference ukf_utils.py:17-22, which tiles the patches with
    torchvision's make_grid(nrow=f_size/p_size, padding=0)): -> [B, channel_num, f, f]."""
    num = f_size // p_size
    x = x.reshape(channel_num, -1, num, num, p_size, p_size)  # (c, b, i, j, a, b')
    x = x.permute(0, 1, 2, 4, 3, 5).reshape(channel_num, -1, f_size, f_size)
    return x.transpose(0, 1)


def valid_steps(valid, T, N):
    """The `valid` of `SquareRootUKF.filter` / `LETKF.filter` -> T entries, each True (plain
    update), False (skip) or a bool [N] device mask."""
    if valid is None:
        return [True] * T
    if torch.is_tensor(valid):
        if valid.dtype != torch.bool or valid.ndim not in (1, 2) or valid.shape[0] != T:
            raise ValueError(f"SquareRootUKF.filter: valid must be bool [{T}] or "
                             f"[{T}, {N}], got {valid.dtype} {list(valid.shape)}")
        if valid.ndim == 1 and not valid.is_cuda:
            valid = valid.tolist()
        elif valid.ndim == 1:  # on the device: never read, becomes a mask per step
            valid = valid.unsqueeze(1).expand(T, N)
    steps = []
    if len(valid) != T:
        raise ValueError(f"SquareRootUKF.filter: {len(valid)} valid entries for {T} "
                         "observations")
    for v in valid:
        if torch.is_tensor(v):
            steps.append(v if v.ndim else v.expand(N))
        else:
            steps.append(v is not None and bool(v))
    return steps


class NSDynamics(nn.Module):
    """Navier-Stokes dynamics of the patched UKF state (reference ukf_utils.py:85-119):
    channels (f, v, v, p) of [B, 4, S, S] fields, state rows of p * p values.

    `compat` is forwarded to `ns_step.full_step`.  The default (True) is the reference's
    arithmetic, including the unbind-stride quirk of update_velocity: for a batch of two or
    more fields, sample b advects memory planes b and b + 1 of the intermediate velocity.  The
    filter hands the model its sigma points as batch ((2n+1) * B fields), so under the quirk
    neighbouring sigma fields are mixed; `compat=False` advects each field by its own
    velocity and is the physically meaningful filter."""

    def __init__(self, config, compat=True):
        super().__init__()
        self.dim = config.kf.patch_size
        self.size = config.data.image_size
        assert self.size % self.dim == 0
        self.state_dim = self.dim ** 2
        self.compat = bool(compat)

    def unpatch(self, x):
        return unpatch(x, self.dim, self.size, 4)

    def forward(self, initial_states, controls=None):
        f, v, p = split_state(self.unpatch(initial_states))
        f, v, p = ns_step.full_step(f, v, p, DT, DX, compat=self.compat)
        state = patch(join_state(f, v, p), self.dim)
        # one 1e-8 I shared by every row (a stride-0 view: the sigma-point batch of the shipped
        # config has 297216 rows, 4.9 GB if repeated)
        uncer = (torch.eye(self.dim ** 2, device=state.device) * 1e-8).unsqueeze(0).expand(
            state.shape[0], -1, -1)
        return state, uncer


class IdentityKFMeasure(nn.Module):
    """Identity observation of the patched state with per-channel noise (reference
    ukf_utils.py:24-66).  Rows come in four equal channel blocks (f, u, v, p), each ordered
    (batch, patch); the batch is (sigma point, sample) when the filter calls the model.

    Returned factor [rows, dim, dim], as the reference builds it: `variance` * I on density
    rows, diag(uncer_flow)^2 on velocity rows and diag(uncer_pres)^2 on pressure rows, where
    the patched uncertainties ([2 * patches, dim] / [patches, dim], set by
    `update_uncertainty`; config.inverse.variance until then) are tiled over the batch with
    the reference's `repeat(N, 1)` -- whole (channel, patch) blocks one after the other, which
    lines up with the (channel, batch, patch) rows of u for every batch size and of v for an
    odd one (a single sample's 2n+1 sigma fields).

    `supports_factor_rows` tells `SquareRootUKF` that `forward(..., factor_rows=idx)` builds the
    factor for the rows it consumes only.

    `h(x) = x` is deterministic by default.  The reference adds a fresh randn draw to the
    states inside `forward`; inside a UKF that perturbs every sigma point differently and
    corrupts the propagated covariance, so it is offered only as `noisy=True`."""

    supports_factor_rows = True

    def __init__(self, config, noisy=False):
        super().__init__()
        self.dim = config.kf.patch_size
        self.size = config.data.image_size
        self.state_dim = self.observation_dim = self.dim ** 2
        self.var = config.inverse.variance
        self.uncer_flow = config.inverse.variance
        self.uncer_pres = config.inverse.variance
        self.noisy = bool(noisy)

    def update_uncertainty(self, uncer_flow, uncer_pres):
        assert uncer_flow.ndim == uncer_pres.ndim == 4
        assert uncer_flow.shape[1] == 2
        assert uncer_pres.shape[1] == 1
        self.uncer_flow = patch(uncer_flow, self.dim)
        self.uncer_pres = patch(uncer_pres, self.dim)

    def _tiled(self, uncer, rows, device):
        """uncer (float, or patched [channels * patches, dim]) -> [rows, dim] by repeat(N, 1)."""
        if not torch.is_tensor(uncer):
            return torch.full((1, self.dim ** 2), float(uncer), device=device).expand(rows, -1)
        assert rows % uncer.shape[0] == 0, "uncertainty rows do not tile the state rows"
        return uncer.to(device).repeat(rows // uncer.shape[0], 1)

    def forward(self, states, f_only=False, factor_rows=None):
        """-> (observations, factor).  `factor_rows` (int64 indices into the rows): build the
        factor for those rows only -- the filter consumes one factor per filter, and all
        (2n+1) * N of the shipped config would be 4.9 GB."""
        d, dev = self.dim ** 2, states.device
        if f_only:
            if self.noisy:
                states = states + torch.randn_like(states) * self.var ** 0.5
            rows = states.shape[0] if factor_rows is None else factor_rows.shape[0]
            eye = torch.eye(d, device=dev)
            return states, (eye * self.var).unsqueeze(0).expand(rows, -1, -1)
        assert states.shape[0] % 4 == 0
        q = states.shape[0] // 4
        flow = self._tiled(self.uncer_flow, 2 * q, dev)
        pres = self._tiled(self.uncer_pres, q, dev)
        if self.noisy:
            noise = torch.cat([torch.randn(q, d, device=dev) * self.var ** 0.5,
                               torch.randn(2 * q, d, device=dev) * flow,
                               torch.randn(q, d, device=dev) * pres], dim=0)
            states = states + noise
        # var * I, diag(uncer_flow)^2, diag(uncer_pres)^2: the diagonals first, [rows, dim]
        diag = torch.cat([torch.full((1, d), float(self.var), device=dev).expand(q, -1),
                          flow ** 2, pres ** 2], dim=0)
        if factor_rows is not None:
            diag = diag[factor_rows]
        return states, torch.diag_embed(diag)


class InpaintKFMeasure(IdentityKFMeasure):
    """Sparse observation of the density channel (the intent of reference ukf_utils.py:69-82,
    whose own version fails its operator's shape assert): `mask` [H, W] or [1, 1, H, W], 1 =
    observed pixel.  The density rows of `states` -- the first quarter of the rows, or all of
    them under `f_only` -- are multiplied by the patched mask tiled over the batch; the u, v and
    p rows and the returned factor are the parent's.  An unobserved pixel then has the same
    measurement (0) at every sigma point: zero measurement deviation, and with the observation
    masked the same way zero innovation, so the update leaves it to the dynamics."""

    def __init__(self, config, mask, noisy=False):
        super().__init__(config, noisy=noisy)
        mask = torch.as_tensor(mask, dtype=torch.float32)
        if mask.ndim == 2:
            mask = mask[None, None]
        if tuple(mask.shape) != (1, 1, self.size, self.size):
            raise ValueError(f"InpaintKFMeasure: mask must be [{self.size}, {self.size}] or "
                             f"[1, 1, {self.size}, {self.size}], got {list(mask.shape)}")
        self.mask_field = mask
        self.mask = patch(mask, self.dim).contiguous()  # [patches, dim]

    def forward(self, states, f_only=False, factor_rows=None):
        z, factor = super().forward(states, f_only=f_only, factor_rows=factor_rows)
        q = z.shape[0] if f_only else z.shape[0] // 4
        m = self._tiled(self.mask, q, z.device)
        if f_only:
            return z * m, factor
        return torch.cat([z[:q] * m, z[q:]], dim=0), factor

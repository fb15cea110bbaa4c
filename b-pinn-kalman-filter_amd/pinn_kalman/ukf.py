"""Square-root unscented Kalman filter over field patches (reference pinn_kalman/ukf.py:9-44).

The reference wraps `torchfilter.filters.SquareRootUnscentedKalmanFilter` with
`MerweSigmaPointStrategy(alpha=1, beta=0, kappa=0)`; torchfilter is not pinned by the reference
and is absent here, so `SquareRootUKF` implements the standard algorithm (Van der Merwe & Wan
2001) on the `op.ukf` kernels.  Two points of its contract cannot be confirmed against
torchfilter here and are fixed as follows:

  * the second value returned by a dynamics / measurement model is consumed as a
    lower-triangular square-root factor (torchfilter's model contract), one per row of the
    sigma-point batch; the filter uses the factor of each filter's sigma point 0 (a tensor with
    one factor per filter is accepted as well, and a measurement model with
    `supports_factor_rows` is asked for those rows only).  `NSDynamics`' 1e-8 I passes through
    as it is.
  * sigma points are handed to the models as 2-D [groups * (2n+1) * N / groups, dim] with rows
    ordered (g, s, r) (see `op.ukf`), not in torchfilter's (filter, sigma) flattening: with
    groups = 4 channels `unpatch` then sees (2n+1) * B whole fields, each assembled from every
    patch's s-th sigma point, where the flattening would scramble patches across fields.

One filter step is predict (sigma points -> dynamics -> unscented root) followed by update
(sigma points redrawn from the prior -> measurement -> unscented root -> Kalman update); only
libbpk.so kernels, the models and element-wise glue run on it.  `PINN_KF` (needs B_PINN ->
bayesian_torch) and `InpaintKFMeasure` are not built.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from op import ukf as K

from .ukf_utils import IdentityKFMeasure, NSDynamics, patch, unpatch


class SquareRootUKF(nn.Module):
    """N independent square-root UKFs sharing a dynamics and a measurement model.

    Attributes after `initialize_beliefs`: `belief_mean` [N, n], `belief_scale_tril`
    [N, n, n] (lower triangular, P = S S^T) and `status` (int32 [N] on the device, OR-ed over
    every kernel since initialisation, never read on the host: 1 where a Cholesky downdate lost
    positive definiteness, see `op.ukf`)."""

    def __init__(self, dynamics, measurement, alpha=1., beta=0., kappa=0., groups=1):
        super().__init__()
        self.dynamics_model = dynamics
        self.measurement_model = measurement
        self.alpha, self.beta, self.kappa = float(alpha), float(beta), float(kappa)
        self.groups = int(groups)
        self.belief_mean = self.belief_scale_tril = self.status = None

    def initialize_beliefs(self, mean, covariance=None, scale_tril=None):
        if (covariance is None) == (scale_tril is None):
            raise ValueError("SquareRootUKF: give exactly one of covariance / scale_tril")
        if mean.ndim != 2:
            raise ValueError("SquareRootUKF: mean must be [N, n]")
        N, n = mean.shape
        if N % self.groups:
            raise ValueError(f"SquareRootUKF: groups = {self.groups} does not divide N = {N}")
        if scale_tril is None:  # general covariance: factored on the host in float64, once
            scale_tril = torch.linalg.cholesky(covariance.detach().double().cpu())
        if tuple(scale_tril.shape) != (N, n, n):
            raise ValueError(f"SquareRootUKF: factor must be [{N}, {n}, {n}]")
        self.weights = K.merwe_weights(n, self.alpha, self.beta, self.kappa)
        self.belief_mean = mean.detach().float().contiguous()
        dev = self.belief_mean.device
        self.belief_scale_tril = scale_tril.detach().to(dev, torch.float32).tril().contiguous()
        self.status = torch.zeros(N, device=dev, dtype=torch.int32)
        self._rows0 = K.point_rows(N, n, self.groups, device=dev)[:, 0].contiguous()

    def _noise(self, factor):
        """Per-filter noise factor from a model's second return value."""
        N = self.belief_mean.shape[0]
        if factor.shape[0] == N:
            return factor
        return factor[self._rows0]

    def _points(self):
        return K.sigma_points(self.belief_mean, self.belief_scale_tril, self.weights[0],
                              self.groups)

    def predict(self, controls=None):
        n = self.belief_mean.shape[1]
        _, wm0, wc0, wi = self.weights
        y, q = self.dynamics_model(self._points(), controls)
        self.belief_mean, self.belief_scale_tril, st = K.unscented_root(
            y, self._noise(q), n, wm0, wc0, wi, self.groups)
        self.status |= st

    def update(self, observations):
        n = self.belief_mean.shape[1]
        _, wm0, wc0, wi = self.weights
        x = self._points()
        if getattr(self.measurement_model, "supports_factor_rows", False):
            z, r = self.measurement_model(x, factor_rows=self._rows0)
        else:
            z, r = self.measurement_model(x)
        z_mean, z_tril, st = K.unscented_root(z, self._noise(r), n, wm0, wc0, wi, self.groups)
        self.status |= st
        self.belief_mean, self.belief_scale_tril, st = K.kalman_update(
            self.belief_mean, self.belief_scale_tril, x, z, z_mean, z_tril, observations, wc0, wi,
            self.groups)
        self.status |= st

    @torch.no_grad()
    def forward(self, observations, controls=None):
        """One filter step; returns the posterior mean [N, n]."""
        if self.belief_mean is None:
            raise RuntimeError("SquareRootUKF: call initialize_beliefs first")
        self.predict(controls)
        self.update(observations)
        return self.belief_mean


class UKF(nn.Module):
    """The reference's patch filter (pinn_kalman/ukf.py:9-44): state = the p x p patches of the
    (f, u, v, p) fields, one filter per (channel, sample, patch) row, `NSDynamics` +
    `IdentityKFMeasure`, Merwe points (1, 0, 0), groups = 4 channels.  `compat` is NSDynamics'
    (True = the reference's stencil arithmetic; False = the physically meaningful filter).

    `initialize(x0, var)`: the reference passes `eye * var` as torchfilter's `covariance`;
    whether it meant a covariance or a factor cannot be settled without torchfilter, so it is
    taken at its word: the initial scale_tril is sqrt(var) I."""

    def __init__(self, config, compat=True):
        super().__init__()
        self.dim = config.kf.patch_size
        self.size = config.data.image_size
        self.device = config.device
        self.dynamic = NSDynamics(config, compat=compat)
        self.measurement = IdentityKFMeasure(config)
        self.ukf = SquareRootUKF(self.dynamic, self.measurement, alpha=1.0, beta=0.0, kappa=0.0,
                                 groups=4)

    def initialize(self, x0=None, var=0.01):
        d = self.dim ** 2
        if x0 is None:
            N = (self.size // self.dim) ** 2 * 4
            mean = torch.full((N, d), 0.1, device=self.device)
            var = 0.01
        else:
            mean = x0.to(self.device)
            N = mean.shape[0]
        tril = (torch.eye(d, device=self.device) * float(var) ** 0.5).unsqueeze(0).expand(N, -1, -1)
        self.ukf.initialize_beliefs(mean=mean, scale_tril=tril)

    def forward(self, obsv):
        """obsv [B, 4, H, W] -> filtered fields [B, 4, H, W]."""
        pred = self.ukf(patch(obsv, self.dim))
        return unpatch(pred, self.dim, self.size, 4)

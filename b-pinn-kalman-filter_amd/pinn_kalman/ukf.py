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
libbpk.so kernels, the models and element-wise glue run on it.

Offline use (the reference filters a recorded sequence, pinn_kalman/ukf.py:85-138):
`SquareRootUKF.filter` runs the forward steps over a whole sequence and keeps each step's
posterior and prediction; `SquareRootUKF.smooth` then runs the unscented Rauch-Tung-Striebel
recursion backwards over that history (`op.ukf.rts_smooth`), so the estimate at frame t also
uses the frames after t.  `UKF.filter` / `UKF.smooth` are the same on fields, and
`UKF(mask=...)` observes the density channel through `InpaintKFMeasure` (sparse pixels).

`PINN_KF` (reference :46-82) couples the filter to a `B_PINN`: each step the Monte-Carlo mean
of the predicted flow and pressure is the pseudo-observation of (u, v, p) and their standard
deviation the observation's uncertainty (`IdentityKFMeasure.update_uncertainty`).

Consistency (`diagnostics=True`, `gate=...`, `valid=...`; all off by default, and then every
launch and result is what it was without them).  An update then also calls
`op.ukf.innovation` on the (z_mean, z_tril) it already has and keeps, per filter, the
normalized innovation squared `nis` = e^T e with e = S_z^-1 (z - zhat) and the innovation
log-likelihood `loglik` = log N(z; zhat, S_z S_z^T).  A consistent filter has nis ~ chi-square
with dz degrees of freedom (mean dz), and the logliks of a sequence add up to the evidence of
the noise choices (initial variance, process noise, observation factor) -- the number to
compare when tuning them.  `gate` (a float, e.g. a chi-square quantile for dz degrees of
freedom; the caller computes it, no scipy here) keeps filters with nis > gate (or NaN) out of
the update; `valid` (bool [N]) marks filters that have no observation at this step.  Both
leave the rejected filters' predicted belief untouched, bit for bit, by a `torch.where` over
the outputs of the one update kernel.  Nothing is read on the host: `valid`, `accepted` and
the statistics stay on the device.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from op import ukf as K

from .pinn import B_PINN
from .simulator import join_state
from .ukf_utils import (IdentityKFMeasure, InpaintKFMeasure, NSDynamics, patch, unpatch,
                        valid_steps)


class FilterHistory:
    """What `SquareRootUKF.filter` keeps of T steps, on the device: `means` [T+1, N, n] and
    `scale_trils` [T+1, N, n, n] (index 0: the belief before the first step, index t + 1: the
    posterior of step t), `pred_means` [T, N, n] and `pred_trils` [T, N, n, n] (the prediction
    of step t) and `controls` (a list of length T).  When the filter kept innovation statistics
    (diagnostics, a gate or a `valid` argument): `nis`, `logliks` [T, N] (NaN where a filter had
    no observation) and `accepted` (bool [T, N]: the update was applied); else None."""

    def __init__(self, means, scale_trils, pred_means, pred_trils, controls, *, nis=None,
                 logliks=None, accepted=None):
        self.means, self.scale_trils = means, scale_trils
        self.pred_means, self.pred_trils = pred_means, pred_trils
        self.controls = controls
        self.nis, self.logliks, self.accepted = nis, logliks, accepted

    def __len__(self):
        return self.pred_means.shape[0]


class SquareRootUKF(nn.Module):
    """N independent square-root UKFs sharing a dynamics and a measurement model.

    Attributes after `initialize_beliefs`: `belief_mean` [N, n], `belief_scale_tril`
    [N, n, n] (lower triangular, P = S S^T) and `status` (int32 [N] on the device, OR-ed over
    every kernel since initialisation, never read on the host: 1 where a Cholesky downdate lost
    positive definiteness, see `op.ukf`).

    `diagnostics=True`: every update also stores `nis`, `loglik` (float32 [N]) and `accepted`
    (bool [N]) of that step (module docstring).  `gate`: the NIS threshold above which a
    filter's update is rejected; implies the statistics.  With neither (and no `valid`
    argument) the three stay None and the filter runs exactly the launches it ran without
    them."""

    def __init__(self, dynamics, measurement, alpha=1., beta=0., kappa=0., groups=1,
                 diagnostics=False, gate=None):
        super().__init__()
        self.dynamics_model = dynamics
        self.measurement_model = measurement
        self.alpha, self.beta, self.kappa = float(alpha), float(beta), float(kappa)
        self.groups = int(groups)
        self.diagnostics = bool(diagnostics)
        self.gate = None if gate is None else float(gate)
        self.nis = self.loglik = self.accepted = None
        self.belief_mean = self.belief_scale_tril = self.status = None
        self._filtered = False

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

    def update(self, observations, valid=None, statistics=False):
        """Measurement update.  `valid` (bool [N] on the device, False = this filter has no
        observation at this step) and the gate decide which filters are *accepted*: valid and
        nis <= gate (a NaN nis compares False and is rejected).  Accepted filters get exactly
        what `kalman_update` returns, rejected ones keep the predicted belief bit for bit (and
        the update's status is not held against them); `nis` / `loglik` are NaN where `valid`
        is False.  `statistics=True` asks for the statistics of this call alone (`filter` does,
        for the observed steps of a sequence with gaps)."""
        n = self.belief_mean.shape[1]
        _, wm0, wc0, wi = self.weights
        x = self._points()
        if getattr(self.measurement_model, "supports_factor_rows", False):
            z, r = self.measurement_model(x, factor_rows=self._rows0)
        else:
            z, r = self.measurement_model(x)
        z_mean, z_tril, st = K.unscented_root(z, self._noise(r), n, wm0, wc0, wi, self.groups)
        self.status |= st
        mean, tril, st = K.kalman_update(
            self.belief_mean, self.belief_scale_tril, x, z, z_mean, z_tril, observations, wc0, wi,
            self.groups)
        if statistics or self.diagnostics or self.gate is not None or valid is not None:
            _, nis, loglik, ist = K.innovation(z_mean, z_tril, observations, white=False)
            self.status |= ist
            accepted = None
            if valid is not None:
                if valid.dtype != torch.bool or tuple(valid.shape) != nis.shape:
                    raise ValueError(f"SquareRootUKF.update: valid must be bool "
                                     f"[{nis.shape[0]}], got {valid.dtype} {list(valid.shape)}")
                accepted = valid = valid.to(nis.device)
                nan = torch.full_like(nis, float("nan"))
                nis, loglik = torch.where(valid, nis, nan), torch.where(valid, loglik, nan)
            if self.gate is not None:
                inside = nis <= self.gate
                accepted = inside if accepted is None else accepted & inside
            if accepted is None:
                accepted = torch.ones_like(nis, dtype=torch.bool)
            else:
                mean = torch.where(accepted.unsqueeze(1), mean, self.belief_mean)
                tril = torch.where(accepted.view(-1, 1, 1), tril, self.belief_scale_tril)
                st = torch.where(accepted, st, torch.zeros_like(st))
            self.nis, self.loglik, self.accepted = nis, loglik, accepted
        self.belief_mean, self.belief_scale_tril = mean, tril
        self.status |= st

    def _skip(self):
        """A step without an observation: the prediction stands, the statistics are NaN."""
        N, dev = self.belief_mean.shape[0], self.belief_mean.device
        self.nis = torch.full((N,), float("nan"), device=dev)
        self.loglik = self.nis.clone()
        self.accepted = torch.zeros(N, device=dev, dtype=torch.bool)

    def _measure(self, observations, valid, statistics=False):
        """The second half of a step: `valid` is None / True (update), False (a missing frame)
        or a bool [N] device mask."""
        if valid is None or valid is True:
            self.update(observations, statistics=statistics)
        elif valid is False:
            self._skip()
        else:
            self.update(observations, valid)

    @torch.no_grad()
    def forward(self, observations, controls=None, valid=None):
        """One filter step; returns the posterior mean [N, n].  `valid`: None (every filter
        observes), bool [N] on the device (see `update`), or a Python False (a missing frame:
        predict only, the measurement model is not called)."""
        if self.belief_mean is None:
            raise RuntimeError("SquareRootUKF: call initialize_beliefs first")
        self.predict(controls)
        self._measure(observations, valid)
        return self.belief_mean

    @torch.no_grad()
    def filter(self, observations, controls=None, valid=None):
        """T `forward` steps from the current belief over `observations` ([T, N, dz] or a
        sequence of T tensors [N, dz]) and `controls` (None or a sequence of length T);
        bit-identical to T calls of `forward`.  Returns the `FilterHistory` `smooth` needs.

        `valid`: None, or T entries, one per step -- a sequence (or a host tensor [T]) of
        Python bools / None / bool [N] device tensors, or a device tensor [T] or [T, N].  A
        step whose entry is a Python False or None is a missing frame: predict only, neither
        the measurement model nor the update runs (its observation is not looked at and may be
        None), and its statistics are NaN.  Entries on the device are never read on the host:
        they go to `update` as masks."""
        if self.belief_mean is None:
            raise RuntimeError("SquareRootUKF: call initialize_beliefs first")
        T = len(observations)
        controls = [None] * T if controls is None else list(controls)
        if len(controls) != T:
            raise ValueError(f"SquareRootUKF.filter: {len(controls)} controls for {T} observations")
        N, n = self.belief_mean.shape
        dev = self.belief_mean.device
        steps = valid_steps(valid, T, N)
        keep = self.diagnostics or self.gate is not None or valid is not None
        means, trils, pmeans, ptrils = [self.belief_mean], [self.belief_scale_tril], [], []
        nis, logliks, accepted = [], [], []
        for t in range(T):
            self.predict(controls[t])
            pmeans.append(self.belief_mean)
            ptrils.append(self.belief_scale_tril)
            self._measure(None if steps[t] is False else observations[t], steps[t], keep)
            means.append(self.belief_mean)
            trils.append(self.belief_scale_tril)
            if keep:
                nis.append(self.nis)
                logliks.append(self.loglik)
                accepted.append(self.accepted)
        self._filtered = True
        stats = {}
        if keep:
            stats = dict(
                nis=torch.stack(nis) if T else torch.empty(0, N, device=dev),
                logliks=torch.stack(logliks) if T else torch.empty(0, N, device=dev),
                accepted=torch.stack(accepted) if T else torch.empty(0, N, device=dev,
                                                                     dtype=torch.bool))
        return FilterHistory(torch.stack(means), torch.stack(trils),
                             torch.stack(pmeans) if T else torch.empty(0, N, n, device=dev),
                             torch.stack(ptrils) if T else torch.empty(0, N, n, n, device=dev),
                             controls, **stats)

    _valid_steps = staticmethod(valid_steps)  # its earlier home; `LETKF.filter` shares it

    @torch.no_grad()
    def smooth(self, history):
        """Unscented Rauch-Tung-Striebel smoother over a `filter` history -> (means_s
        [T+1, N, n], scale_trils_s [T+1, N, n, n]); index T is the filtered posterior itself.

        For t = T-1 .. 0 the sigma points of the posterior at t are redrawn and propagated
        through the dynamics model again, then `op.ukf.rts_smooth` combines them with the
        stored prediction and the smoothed belief at t + 1.  Redrawing instead of storing
        keeps a step's history at 2 (N n^2 + N n) floats (76 MB at 2304 filters of n = 64,
        against 228 MB with both point sets), and requires a deterministic dynamics model:
        the second call must return the points the prediction was made from.  `NSDynamics`
        is one.  Statuses are OR-ed into `self.status`.

        A gated, invalid or skipped step needs nothing special: its posterior is its
        prediction, so its entry of `history.means` equals that of `history.pred_means`, and
        the backward recursion treats it like any other step (the step carried no
        information; the smoothed belief there comes from the dynamics and the later
        frames)."""
        if self.belief_mean is None or not self._filtered:
            raise RuntimeError("SquareRootUKF: call filter before smooth")
        if not isinstance(history, FilterHistory):
            raise ValueError("SquareRootUKF.smooth: history must come from filter()")
        N, n = self.belief_mean.shape
        T = len(history)
        if (tuple(history.means.shape) != (T + 1, N, n)
                or tuple(history.scale_trils.shape) != (T + 1, N, n, n)
                or tuple(history.pred_means.shape) != (T, N, n)
                or tuple(history.pred_trils.shape) != (T, N, n, n)
                or len(history.controls) != T):
            raise ValueError(f"SquareRootUKF.smooth: history is not one of {N} filters of "
                             f"dimension {n}")
        gamma, _, wc0, wi = self.weights
        ms, Ss = [None] * (T + 1), [None] * (T + 1)
        ms[T], Ss[T] = history.means[T], history.scale_trils[T]
        for t in range(T - 1, -1, -1):
            m, S = history.means[t], history.scale_trils[t]
            x = K.sigma_points(m, S, gamma, self.groups)
            y = self.dynamics_model(x, history.controls[t])[0]
            ms[t], Ss[t], st = K.rts_smooth(m, S, x, y, history.pred_means[t],
                                            history.pred_trils[t], ms[t + 1], Ss[t + 1], wc0, wi,
                                            self.groups)
            self.status |= st
        return torch.stack(ms), torch.stack(Ss)


class UKF(nn.Module):
    """The reference's patch filter (pinn_kalman/ukf.py:9-44): state = the p x p patches of the
    (f, u, v, p) fields, one filter per (channel, sample, patch) row, `NSDynamics` +
    `IdentityKFMeasure`, Merwe points (1, 0, 0), groups = 4 channels.  `compat` is NSDynamics'
    (True = the reference's stencil arithmetic; False = the physically meaningful filter).

    `initialize(x0, var)`: the reference passes `eye * var` as torchfilter's `covariance`;
    whether it meant a covariance or a factor cannot be settled without torchfilter, so it is
    taken at its word: the initial scale_tril is sqrt(var) I.

    `mask` ([H, W] or [1, 1, H, W], 1 = observed; None = every pixel, the reference's filter):
    the density channel is observed through `InpaintKFMeasure` and the density channel of
    every observation is multiplied by the mask, so an unobserved pixel has zero measurement
    deviation and zero innovation and is left to the dynamics.

    `filter(obsv_seq)` / `smooth(obsv_seq)` process a recorded sequence [T, B, 4, H, W];
    `smooth` needs a deterministic dynamics model (see `SquareRootUKF.smooth`).

    `diagnostics` / `gate` are `SquareRootUKF`'s.  `valid` (`forward`: bool [B]; `filter`:
    [T] or [T, B]) marks whole frames of a sample as present; it is expanded to the filter rows
    in `patch`'s (channel, sample, patch) order.  After `filter`, `nis_maps()` and
    `log_likelihood()` read the statistics of `self.history`.  Under `mask`, an unobserved
    density pixel has zero deviation and zero innovation, and S_z is block diagonal there with
    the measurement model's own factor entry r on the diagonal (`IdentityKFMeasure` hands the
    filter `config.inverse.variance` as that factor entry, so the pixel's innovation variance
    is r^2): the pixel adds zero to the NIS and the constant -0.5 log(2 pi r^2) to the
    log-likelihood."""

    def __init__(self, config, compat=True, mask=None, diagnostics=False, gate=None):
        super().__init__()
        self.dim = config.kf.patch_size
        self.size = config.data.image_size
        self.device = config.device
        self.dynamic = NSDynamics(config, compat=compat)
        self.mask = None
        if mask is None:
            self.measurement = IdentityKFMeasure(config)
        else:
            self.measurement = InpaintKFMeasure(config, mask)
            self.mask = self.measurement.mask_field.to(self.device)
        self.ukf = SquareRootUKF(self.dynamic, self.measurement, alpha=1.0, beta=0.0, kappa=0.0,
                                 groups=4, diagnostics=diagnostics, gate=gate)
        self.history = None

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

    def forward(self, obsv, valid=None):
        """obsv [B, 4, H, W] -> filtered fields [B, 4, H, W].  `valid`: None, bool [B] on the
        device (samples whose frame is present) or a Python False (no frame: predict only)."""
        if valid is None:
            pred = self.ukf(self._observation(obsv))
        elif valid is False:
            pred = self.ukf(None, valid=False)
        else:
            pred = self.ukf(self._observation(obsv), valid=self._valid_rows(valid))
        return unpatch(pred, self.dim, self.size, 4)

    def _valid_rows(self, valid):
        """bool [..., B] (frames of a sample) -> bool [..., N]: filter rows are (channel,
        sample, patch)."""
        if not torch.is_tensor(valid) or valid.dtype != torch.bool or valid.ndim < 1:
            raise ValueError("UKF: valid must be a bool tensor over the samples")
        patches = (self.size // self.dim) ** 2
        lead, B = valid.shape[:-1], valid.shape[-1]
        v = valid.reshape(*lead, 1, B, 1).expand(*lead, 4, B, patches)
        return v.reshape(*lead, 4 * B * patches)

    def _observation(self, obsv):
        """[B, 4, H, W] -> the filters' observation rows (density masked under `mask`)."""
        if self.mask is not None:
            obsv = torch.cat([obsv[:, :1] * self.mask, obsv[:, 1:]], dim=1)
        return patch(obsv, self.dim)

    def _fields(self, means):
        """[T, N, n] -> [T, B, 4, H, W]."""
        return torch.stack([unpatch(m, self.dim, self.size, 4) for m in means])

    def filter(self, obsv_seq, valid=None):
        """obsv_seq [T, B, 4, H, W] -> filtered fields [T, B, 4, H, W]: T `forward` steps.
        `valid`: None, [T] (whole steps; host bools make a False step predict-only, see
        `SquareRootUKF.filter`) or a bool tensor [T, B] (frames of single samples)."""
        if torch.is_tensor(valid) and valid.ndim == 2:
            valid = self._valid_rows(valid)
        self.history = self.ukf.filter([self._observation(o) for o in obsv_seq], valid=valid)
        return self._fields(self.history.means[1:])

    def _statistic(self, name):
        h = self.history
        if h is None or getattr(h, name) is None:
            raise RuntimeError("UKF: no innovation statistics: build the filter with "
                               "diagnostics=True (or a gate / valid) and call filter() first")
        v = getattr(h, name)
        num = self.size // self.dim
        return v.reshape(v.shape[0], 4, -1, num, num).transpose(1, 2)  # [T, B, 4, H/p, W/p]

    def nis_maps(self):
        """[T, B, 4, H/p, W/p]: the NIS of every (channel, patch) filter at every step of the
        last `filter` (NaN where a frame was missing); a consistent filter has mean p^2."""
        return self._statistic("nis")

    def log_likelihood(self):
        """[T, B]: the innovation log-likelihood of every frame of the last `filter`, summed
        over channels and patches (the filters are independent, so their evidences add); NaN
        where the frame was missing."""
        return self._statistic("logliks").sum(dim=(2, 3, 4))

    def smooth(self, obsv_seq, valid=None):
        """obsv_seq [T, B, 4, H, W] -> (filtered, smoothed), both [T, B, 4, H, W]: `filter`,
        then the backward pass; smoothed[T-1] is filtered[T-1]."""
        filtered = self.filter(obsv_seq, valid=valid)
        means_s, _ = self.ukf.smooth(self.history)
        return filtered, self._fields(means_s[1:])


class PINN_KF(nn.Module):
    """B-PINN pseudo-observations filtered by the patch UKF (reference pinn_kalman/ukf.py:46-82).

    `initialize(f, v, p, var=1e-2)`: the filter starts at the patched fields [f, v, p] with
    scale sqrt(var) I, and f becomes the previous frame.  It loads no checkpoint: the reference
    hard-codes a path (and uses names it never defines); loading the B_PINN's weights
    (`self.pinn`, e.g. utils.load_checkpoint) is the caller's job.

    `forward(x, y, t, f, n=8)`, without autograd: n Monte-Carlo forwards of the B_PINN on
    (previous frame, f); mean and unbiased std of the full-size flow and of the pressure; the
    stds go to `measurement.update_uncertainty`; the observation cat[f, flow mean, pressure
    mean] goes through one `UKF.forward`.  Returns the filtered fields [B, 4, H, W].
    `mask` / `compat` / `diagnostics` / `gate` are the UKF's: with diagnostics on,
    `self.ukf.ukf.nis`, `.loglik` and `.accepted` describe the step `forward` just made (how
    well the B-PINN's Monte-Carlo std explains its own pseudo-observation)."""

    def __init__(self, config, compat=True, mask=None, diagnostics=False, gate=None):
        super().__init__()
        self.device = config.device
        self.patch_size = config.kf.patch_size
        self.ukf = UKF(config, compat=compat, mask=mask, diagnostics=diagnostics,
                       gate=gate).to(self.device)
        self.pinn = B_PINN(config).to(self.device)
        self.f_prev = None

    def initialize(self, f, v, p, var=1e-2):
        state = patch(join_state(f, v, p), self.patch_size)
        self.ukf.initialize(state, var)
        self.f_prev = f

    @torch.no_grad()
    def forward(self, x, y, t, f, n=8):
        if self.f_prev is None:
            self.f_prev = torch.ones_like(f) * 0.1
        t = t.to(self.device)
        flow, pres = self.pinn.sample_uvp(self.f_prev, f, x, y, t, n=n,
                                          size=(self.ukf.size, self.ukf.size))
        flow, pres = torch.stack(flow, dim=0), torch.stack(pres, dim=0)
        flow_uncer, pres_uncer = flow.std(dim=0), pres.std(dim=0)
        flow, pres = flow.mean(dim=0), pres.mean(dim=0)
        self.f_prev = f
        self.ukf.measurement.update_uncertainty(flow_uncer, pres_uncer)
        return self.ukf(torch.cat([f, flow, pres], dim=1))

"""Local ensemble transform Kalman filter (Hunt, Kostelich & Szunyogh 2007) on the simulator.

An ensemble [B, m, 4, H, W] (channels f, u, v, p as in `UKF` / `FourDVar`) is a batch of
B * m simulator replicas that differ.  One filter step is

  forecast  `steps_per_frame` simulator steps of every member (`ns_step.full_step(compat=False)`
            on the B * m planes: the replicas are independent there), and
  analysis  `op.letkf.analysis`: every grid point fits the ensemble to the observations of its
            (2R+1)^2 window, weighted by a localization taper, and transforms the members so
            that mean and sample covariance are the Kalman update's (csrc/letkf.hip).

Next to the patch UKF (129 simulator steps per filter step, no covariance across a patch
border) this costs m simulator steps per frame, its covariances are the flow's own and cross
any border, and unlike `FourDVar` it is sequential and returns a spread next to the mean.
By default the observation is the masked identity: `weights` are the inverse variances of
`fourdvar.observation_weights` (0 = unobserved).

With `observe` the filter assimilates observations on a grid of their own behind any operator
the members can be passed through, e.g. `blur_observation`: a blurred, low-resolution image of
some channels (`op.letkf.analysis_obs`).  An observation is localized at its sampling point
(`obs_stride * i + obs_offset`), so the operator's footprint (K // 2 for a K-tap blur) should
be small against the radius R.  With a window that sees every observation at full weight the
analysis is the exact Kalman update for any linear operator.

Everything stays on the device: `filter` never reads a value on the host, and the number of
grid points the analysis flagged is summed per frame into a device tensor.

No reference counterpart (the reference has no ensemble filter).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import simulator
from .ukf_utils import valid_steps


@dataclass
class EnsembleHistory:
    means: torch.Tensor           # [T, B, 4, H, W] analysis means
    spreads: torch.Tensor         # [T, B, 4, H, W] analysis spreads (unbiased std over members)
    forecast_means: torch.Tensor  # [T, B, 4, H, W]
    flagged: torch.Tensor         # [T] int64: grid points whose analysis status was not 0
    forecast_ensembles: Optional[torch.Tensor] = None  # [T, B, m, 4, H, W] (keep_ensembles)
    analysis_ensembles: Optional[torch.Tensor] = None  # [T, B, m, 4, H, W] (keep_ensembles)

    def __len__(self):
        return self.means.shape[0]


def blur_observation(taps, stride=1, channels=None):
    """The observation operator x [N, C, H, W] -> `op.blur.blur2d(x[:, channels], taps, stride)`
    (all channels with channels=None): `channels=[0]` is a blurred, low-resolution density
    image.  Pass it as `LETKF(..., observe=..., obs_stride=stride)`; blur2d samples at
    stride * i + (stride - 1) // 2, the default `obs_offset`.  The footprint of an observation
    is len(taps) // 2 grid points around its sampling point, where the filter localizes it:
    keep it small against the radius R."""
    from op import blur
    idx = None if channels is None else [int(c) for c in channels]

    def observe(x):
        return blur.blur2d(x if idx is None else x[:, idx].contiguous(), taps, stride)
    return observe


class LETKF:
    """members: ensemble size m (2..64).  radius: window half-width R in grid points (0..8).
    taper: "gaspari_cohn" (with `cutoff`, default (R + 1) / 2), "boxcar", or a [2R+1, 2R+1]
    table.  inflation: multiplicative covariance inflation applied in every analysis.
    step_fn(f, v, p) -> (f', v', p') on [B * m] planes; default `ns_step.full_step(compat=False)`
    with this object's dt, dx (HIP tensors only).  analysis_fn(ens, obs, prec, taper, inflation)
    -> (ens_out, status); default `op.letkf.analysis` (HIP, float32).  Restatements of both can
    be passed to run the host logic on other devices or dtypes.

    observe: None (the masked identity: nothing below applies), or a map of planes
    [N, C, H, W] -> [N, Cy, Hy, Wy] such as `blur_observation`.  Observation (i, j) is localized
    at state grid point (obs_stride i + obs_offset, obs_stride j + obs_offset); obs_offset=None:
    (obs_stride - 1) // 2.  Its footprint should be small against R; with a window that sees
    everything the analysis is the exact Kalman update for any linear `observe`.
    obs_analysis_fn(ens, yens, obs, prec, taper, inflation, stride, offset) -> (ens_out, status);
    default `op.letkf.analysis_obs`."""

    def __init__(self, members, radius, cutoff=None, inflation=1.0, taper="gaspari_cohn",
                 steps_per_frame=1, dt=simulator.dt, dx=simulator.dx, step_fn=None,
                 analysis_fn=None, observe=None, obs_stride=1, obs_offset=None,
                 obs_analysis_fn=None):
        from op import letkf as K
        if not 2 <= int(members) <= K.MAX_MEMBERS:
            raise ValueError(f"LETKF: members = {members} out of range [2, {K.MAX_MEMBERS}]")
        if int(steps_per_frame) < 1:
            raise ValueError("LETKF: steps_per_frame must be >= 1")
        if not float(inflation) > 0:
            raise ValueError(f"LETKF: inflation = {inflation} must be positive")
        self.members, self.steps_per_frame = int(members), int(steps_per_frame)
        self.inflation = float(inflation)
        self.dt, self.dx = float(dt), float(dx)
        if torch.is_tensor(taper):
            R = int(radius)
            if tuple(taper.shape) != (2 * R + 1, 2 * R + 1):
                raise ValueError(f"LETKF: taper must be [{2 * R + 1}, {2 * R + 1}], got "
                                 f"{list(taper.shape)}")
            self.taper = taper.detach().clone()
        elif taper == "gaspari_cohn":
            self.taper = K.gaspari_cohn_taper(radius, cutoff)
        elif taper == "boxcar":
            self.taper = K.boxcar_taper(radius)
        else:
            raise ValueError(f"LETKF: unknown taper {taper!r}")
        self.radius = self.taper.shape[0] // 2
        self.step_fn = simulator.default_step(self.dt, self.dx) if step_fn is None else step_fn
        self.analysis_fn = K.analysis if analysis_fn is None else analysis_fn
        self.observe = observe
        self.obs_stride = int(obs_stride)
        if self.obs_stride != obs_stride or self.obs_stride < 1:
            raise ValueError(f"LETKF: obs_stride = {obs_stride} must be an integer >= 1")
        self.obs_offset = (self.obs_stride - 1) // 2 if obs_offset is None else int(obs_offset)
        if not 0 <= self.obs_offset < self.obs_stride:
            raise ValueError(f"LETKF: obs_offset = {obs_offset} out of range "
                             f"[0, obs_stride = {self.obs_stride})")
        self.obs_analysis_fn = K.analysis_obs if obs_analysis_fn is None else obs_analysis_fn
        self.ens = None

    # ------------------------------------------------------------------------------------
    def initialize(self, mean, perturbations=None, std=None, length=None, generator=None):
        """Ensemble = mean [B, C, H, W] + centred perturbations (C = 4, channels f, u, v, p,
        with the default step; an injected step and analysis may carry any C).  Given
        `perturbations` [B, m, C, H, W], their member mean is removed.  Otherwise white noise
        from `generator` is smoothed with `op.blur`'s Gaussian (`gaussian_taps(length, K)`,
        `length` being the variance of the Gaussian in grid points squared; HIP only;
        length=None: no smoothing), scaled so that every channel's standard deviation is
        `std` (a float or C values), and centred."""
        if mean.ndim != 4:
            raise ValueError(f"LETKF: mean must be [B, C, H, W], got {list(mean.shape)}")
        B, C, H, W = mean.shape
        m = self.members
        if perturbations is None:
            if std is None:
                raise ValueError("LETKF.initialize: give perturbations or std")
            gdev = mean.device if generator is None else generator.device
            noise = torch.randn(B, m, C, H, W, generator=generator, device=gdev,
                                dtype=mean.dtype).to(mean.device)
            if length is not None:
                from op import blur
                half = min(blur.MAX_TAPS // 2, H, W, max(1, math.ceil(3 * math.sqrt(length))))
                taps = blur.gaussian_taps(length, 2 * half + 1)
                noise = blur.blur2d(noise.view(B * m, C, H, W), taps).view(B, m, C, H, W)
            std = torch.as_tensor(std, dtype=mean.dtype, device=mean.device).expand(C)
            scale = std / noise.std(dim=(0, 1, 3, 4))
            perturbations = noise * scale.view(1, 1, C, 1, 1)
        elif tuple(perturbations.shape) != (B, m, C, H, W):
            raise ValueError(f"LETKF: perturbations must be {[B, m, C, H, W]}, got "
                             f"{list(perturbations.shape)}")
        perturbations = perturbations - perturbations.mean(1, keepdim=True)
        self.ens = (mean.unsqueeze(1) + perturbations).contiguous()
        return self.ens

    def _need(self):
        if self.ens is None:
            raise RuntimeError("LETKF: initialize() first")
        return self.ens

    def mean(self):
        return self._need().mean(1)

    def spread(self):
        """Unbiased standard deviation over the members at every site."""
        return self._need().std(1, unbiased=True)

    @torch.no_grad()
    def observation_shape(self):
        """(B, Cy, Hy, Wy): what `observe` makes of one member of every sample ((B, C, H, W)
        without `observe`)."""
        ens = self._need()
        B, m, C, H, W = ens.shape
        if self.observe is None:
            return (B, C, H, W)
        return (B,) + tuple(self.observe(ens[:, 0].contiguous()).shape[1:])

    @torch.no_grad()
    def forecast(self):
        """`steps_per_frame` simulator steps of every member."""
        ens = self._need()
        B, m, C, H, W = ens.shape
        fvp = simulator.split_state(ens.view(B * m, C, H, W))
        fvp = simulator.advance(self.step_fn, *fvp, self.steps_per_frame)
        self.ens = simulator.join_state(*fvp).view(B, m, C, H, W)
        return self.ens

    @torch.no_grad()
    def analyze(self, obs, weights, valid=None):
        """obs [B, 4, H, W] ([B, Cy, Hy, Wy] with `observe`); weights: inverse variances
        broadcastable to it (0 = unobserved; obs may hold anything there).  valid: None, or a
        bool [B] device mask -- a sample that is not valid keeps its forecast bit for bit (no
        analysis, no inflation).
        -> status int32 [B, H, W] (0 for samples that are not valid)."""
        ens = self._need()
        B, m, C, H, W = ens.shape
        yens = None
        if self.observe is not None:
            yens = self.observe(ens.reshape(B * m, C, H, W))
            yens = yens.reshape(B, m, *yens.shape[1:]).contiguous()
        oshape = (B, C, H, W) if yens is None else (B,) + tuple(yens.shape[2:])
        if tuple(obs.shape) != oshape:
            raise ValueError(f"LETKF: obs must be {list(oshape)}, got {list(obs.shape)}")
        prec = torch.as_tensor(weights, dtype=ens.dtype, device=ens.device)
        if prec.ndim == 5 and prec.shape[0] == 1:  # observation_weights' frame axis
            prec = prec[0]
        prec = prec.expand(oshape)
        if valid is not None:
            prec = prec * valid.view(B, 1, 1, 1).to(ens.dtype)
        if yens is None:
            out, status = self.analysis_fn(ens.contiguous(), obs.contiguous(), prec.contiguous(),
                                           self.taper, self.inflation)
        else:
            out, status = self.obs_analysis_fn(ens.contiguous(), yens, obs.contiguous(),
                                               prec.contiguous(), self.taper, self.inflation,
                                               self.obs_stride, self.obs_offset)
        if valid is not None:
            out = torch.where(valid.view(B, 1, 1, 1, 1), out, ens)
            status = status * valid.view(B, 1, 1).to(status.dtype)
        self.ens = out
        return status

    @torch.no_grad()
    def filter(self, obsv_seq, weights, valid=None, keep_ensembles=False):
        """Forecast + analysis for every frame of obsv_seq [T, B, 4, H, W] ([T, B, Cy, Hy, Wy]
        with `observe`) from the current ensemble.  weights: as `analyze` (broadcast over the
        frames).  valid: None, bool [T] or bool [T, B] as `UKF.filter` takes it; a missing frame
        is forecast only.
        -> EnsembleHistory."""
        ens = self._need()
        if self.observe is not None:
            want = self.observation_shape()
            if obsv_seq.ndim != 5 or tuple(obsv_seq.shape[1:]) != want:
                raise ValueError(f"LETKF.filter: obsv_seq must be [T, B, Cy, Hy, Wy] with "
                                 f"[B, Cy, Hy, Wy] = {list(want)}, the observed ensemble's, got "
                                 f"{list(obsv_seq.shape)}")
        elif obsv_seq.ndim != 5 or tuple(obsv_seq.shape[1:]) != (ens.shape[0],) + tuple(ens.shape[2:]):
            raise ValueError(f"LETKF.filter: obsv_seq must be [T, B, C, H, W] of the ensemble, got "
                             f"{list(obsv_seq.shape)}")
        T, B = obsv_seq.shape[:2]
        steps = valid_steps(valid, T, B)
        means, spreads, fmeans, flagged, fens, aens = [], [], [], [], [], []
        for t in range(T):
            self.forecast()
            fmeans.append(self.mean())
            if keep_ensembles:
                fens.append(self.ens)
            if steps[t] is False:
                flagged.append(torch.zeros((), dtype=torch.int64, device=ens.device))
            else:
                status = self.analyze(obsv_seq[t], weights,
                                      None if steps[t] is True else steps[t])
                flagged.append((status != 0).sum())
            means.append(self.mean())
            spreads.append(self.spread())
            if keep_ensembles:
                aens.append(self.ens)
        return EnsembleHistory(torch.stack(means), torch.stack(spreads), torch.stack(fmeans),
                               torch.stack(flagged),
                               torch.stack(fens) if keep_ensembles else None,
                               torch.stack(aens) if keep_ensembles else None)

"""`op.ukf` -- square-root unscented Kalman filter steps on HIP (csrc/ukf.hip).

The reference delegates its filter to `torchfilter` (pinn_kalman/ukf.py:4-23), which it does
not pin and which is absent here; these ops implement the standard square-root UKF (Van der
Merwe & Wan 2001) with Merwe scaled sigma points for N independent filters of state dimension
n <= 64, float32 -- the forward filter steps and the backward step of the unscented
Rauch-Tung-Striebel smoother:

  sigma_points    X_0 = m, X_i = m + gamma S[:, i-1], X_{n+i} = m - gamma S[:, i-1]
  unscented_root  weighted mean and square-root covariance of propagated points + noise factor
  kalman_update   cross covariance, gain by triangular solves, mean update, rank-1 downdates
  rts_smooth      state / propagated-state cross covariance, smoother gain by triangular
                  solves, smoothed mean, rank-1 updates then downdates of the posterior factor

Row layout.  Filters are rows i = g * (N / groups) + r.  Every sigma-point tensor is 2-D
[groups * (2n+1) * N / groups, dim] with rows ordered (g, s, r) -- `point_rows` gives the
index.  With groups = 4 this is what `pinn_kalman.ukf_utils.unpatch(..., channel_num=4)`
reads as (2n+1) * B whole 4-channel fields, field (s, b) being assembled from every patch's
s-th sigma point.  This differs from torchfilter's (filter, sigma) flattening, which would
scramble patches across fields.

Factors are lower triangular; only the lower triangle of a noise factor is read.  `status`
(int32 [N]) is 1 where a rank-1 downdate lost positive definiteness (that filter's outputs are
finite but otherwise unspecified; the others are unaffected), else 0.

Consistency.  `innovation` reports what an update's innovation says about the filter: the
whitened innovation e = S_z^-1 (z - zhat) (the very vector `kalman_update` applies), the
normalized innovation squared nis = e^T e (chi-square with dz degrees of freedom when the
filter's covariances are right) and the innovation log-likelihood
-0.5 (nis + 2 sum_i log S_z[i,i] + dz log(2 pi)) = log N(z; zhat, S_z S_z^T).  Its `status` is 1
where z_tril's diagonal is not positive and finite; that filter's statistics are NaN.  The
reference has no counterpart (torchfilter reports none); the truth is the closed-form Gaussian
evidence in float64.
"""
from __future__ import annotations

import math

import torch

from ._lib import check, lib, require_hip, stream_ptr

MAX_DIM = 64


def merwe_weights(n, alpha=1., beta=0., kappa=0.):
    """(gamma, wm0, wc0, wi) of the Merwe scaled sigma points: lam = alpha^2 (n + kappa) - n,
    gamma = sqrt(n + lam), wm0 = lam / (n + lam), wc0 = wm0 + 1 - alpha^2 + beta,
    wi = 1 / (2 (n + lam)).  Pure Python."""
    n = int(n)
    if n < 1:
        raise ValueError(f"merwe_weights: n = {n} must be >= 1")
    lam = alpha * alpha * (n + kappa) - n
    if n + lam <= 0:
        raise ValueError(f"merwe_weights: n + lambda = {n + lam} must be positive "
                         f"(alpha={alpha}, kappa={kappa})")
    wm0 = lam / (n + lam)
    return math.sqrt(n + lam), wm0, wm0 + 1. - alpha * alpha + beta, 1. / (2. * (n + lam))


def point_rows(N, n, groups=1, device=None):
    """int64 [N, 2n+1]: row of filter i's sigma point s in the (g, s, r) order."""
    if groups < 1 or N % groups:
        raise ValueError(f"ukf: groups = {groups} does not divide N = {N}")
    ng = N // groups
    i = torch.arange(N, device=device).unsqueeze(1)
    s = torch.arange(2 * n + 1, device=device).unsqueeze(0)
    return ((i // ng) * (2 * n + 1) + s) * ng + i % ng


def _f32(what, *ts):
    require_hip(*ts, what=what)
    for t in ts:
        if t.dtype != torch.float32:
            raise RuntimeError(f"{what}: float32 tensors required, got {t.dtype}")


def _shape(what, name, t, shape):
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: {name} must be {list(shape)}, got {list(t.shape)}")


def _geo(what, N, n, groups, **dims):
    for k, v in dict(n=n, **dims).items():
        if not 1 <= v <= MAX_DIM:
            raise RuntimeError(f"{what}: {k} = {v} out of range [1, {MAX_DIM}]")
    if groups < 1 or N % groups:
        raise RuntimeError(f"{what}: groups = {groups} does not divide N = {N}")


def sigma_points(mean, scale_tril, gamma, groups=1):
    """mean [N, n], scale_tril [N, n, n] -> points [(2n+1) N, n], rows (g, s, r)."""
    what = "ukf.sigma_points"
    _f32(what, mean, scale_tril)
    if mean.ndim != 2:
        raise RuntimeError(f"{what}: mean must be [N, n]")
    N, n = mean.shape
    _shape(what, "scale_tril", scale_tril, (N, n, n))
    _geo(what, N, n, groups)
    mean, scale_tril = mean.contiguous(), scale_tril.contiguous()
    out = torch.empty((2 * n + 1) * N, n, device=mean.device, dtype=torch.float32)
    check(lib.bpk_ukf_sigma_points_f32(mean.data_ptr(), scale_tril.data_ptr(), out.data_ptr(), N,
                                       n, float(gamma), int(groups), stream_ptr(mean.device)),
          what)
    return out


def unscented_root(points, noise_tril, n, wm0, wc0, wi, groups=1):
    """points [(2n+1) N, d] in (g, s, r) order, noise_tril [N, d, d] ->
    (mean [N, d], scale_tril [N, d, d], status int32 [N])."""
    what = "ukf.unscented_root"
    _f32(what, points, noise_tril)
    if points.ndim != 2 or noise_tril.ndim != 3:
        raise RuntimeError(f"{what}: points must be 2-D and noise_tril 3-D")
    N, d = noise_tril.shape[0], points.shape[1]
    _shape(what, "noise_tril", noise_tril, (N, d, d))
    _shape(what, "points", points, ((2 * n + 1) * N, d))
    _geo(what, N, n, groups, d=d)
    points, noise_tril = points.contiguous(), noise_tril.contiguous()
    mean = torch.empty(N, d, device=points.device, dtype=torch.float32)
    tril = torch.empty(N, d, d, device=points.device, dtype=torch.float32)
    status = torch.empty(N, device=points.device, dtype=torch.int32)
    check(lib.bpk_ukf_root_f32(points.data_ptr(), noise_tril.data_ptr(), mean.data_ptr(),
                               tril.data_ptr(), status.data_ptr(), N, int(n), d, float(wm0),
                               float(wc0), float(wi), int(groups), stream_ptr(points.device)),
          what)
    return mean, tril, status


def kalman_update(mean, scale_tril, x_points, z_points, z_mean, z_tril, obs, wc0, wi, groups=1):
    """Prior (mean [N, n], scale_tril [N, n, n]), its sigma points x_points [(2n+1) N, n], their
    measurements z_points [(2n+1) N, dz] with (z_mean [N, dz], z_tril [N, dz, dz]) from
    `unscented_root`, and obs [N, dz] -> posterior (mean, scale_tril, status)."""
    what = "ukf.kalman_update"
    _f32(what, mean, scale_tril, x_points, z_points, z_mean, z_tril, obs)
    if mean.ndim != 2 or z_mean.ndim != 2:
        raise RuntimeError(f"{what}: mean and z_mean must be 2-D")
    (N, n), dz = mean.shape, z_mean.shape[1]
    _shape(what, "scale_tril", scale_tril, (N, n, n))
    _shape(what, "x_points", x_points, ((2 * n + 1) * N, n))
    _shape(what, "z_points", z_points, ((2 * n + 1) * N, dz))
    _shape(what, "z_mean", z_mean, (N, dz))
    _shape(what, "z_tril", z_tril, (N, dz, dz))
    _shape(what, "obs", obs, (N, dz))
    _geo(what, N, n, groups, dz=dz)
    mean, scale_tril, x_points, z_points, z_mean, z_tril, obs = (
        t.contiguous() for t in (mean, scale_tril, x_points, z_points, z_mean, z_tril, obs))
    m1 = torch.empty_like(mean)
    s1 = torch.empty_like(scale_tril)
    status = torch.empty(N, device=mean.device, dtype=torch.int32)
    check(lib.bpk_ukf_update_f32(mean.data_ptr(), scale_tril.data_ptr(), x_points.data_ptr(),
                                 z_points.data_ptr(), z_mean.data_ptr(), z_tril.data_ptr(),
                                 obs.data_ptr(), m1.data_ptr(), s1.data_ptr(), status.data_ptr(),
                                 N, n, dz, float(wc0), float(wi), int(groups),
                                 stream_ptr(mean.device)), what)
    return m1, s1, status


def rts_smooth(mean, scale_tril, x_points, y_points, pred_mean, pred_tril, next_mean, next_tril,
               wc0, wi, groups=1):
    """One backward step t+1 -> t of the unscented Rauch-Tung-Striebel smoother.  Posterior at t
    (mean [N, n], scale_tril [N, n, n]), its sigma points x_points [(2n+1) N, n] and their
    images y_points [(2n+1) N, n] under the dynamics, the prediction at t+1 (pred_mean [N, n],
    pred_tril [N, n, n]: `unscented_root` of y_points) and the smoothed belief at t+1
    (next_mean, next_tril) -> smoothed belief at t (mean, scale_tril, status).

    C = sum_s wc_s (X_s - m)(Y_s - m-)^T, G = C P-^-1, m^s = m + G (m^s_+ - m-),
    P^s = P + G P^s_+ G^T - G P- G^T: n rank-1 updates of S by the columns of G S^s_+, then n
    rank-1 downdates by the columns of G S- (updates first: every intermediate then dominates
    P^s, where downdates first would pass through the nearly singular P - C P-^-1 C^T)."""
    what = "ukf.rts_smooth"
    _f32(what, mean, scale_tril, x_points, y_points, pred_mean, pred_tril, next_mean, next_tril)
    if mean.ndim != 2:
        raise RuntimeError(f"{what}: mean must be 2-D")
    N, n = mean.shape
    _shape(what, "scale_tril", scale_tril, (N, n, n))
    _shape(what, "x_points", x_points, ((2 * n + 1) * N, n))
    _shape(what, "y_points", y_points, ((2 * n + 1) * N, n))
    _shape(what, "pred_mean", pred_mean, (N, n))
    _shape(what, "pred_tril", pred_tril, (N, n, n))
    _shape(what, "next_mean", next_mean, (N, n))
    _shape(what, "next_tril", next_tril, (N, n, n))
    _geo(what, N, n, groups)
    mean, scale_tril, x_points, y_points, pred_mean, pred_tril, next_mean, next_tril = (
        t.contiguous() for t in (mean, scale_tril, x_points, y_points, pred_mean, pred_tril,
                                 next_mean, next_tril))
    m1 = torch.empty_like(mean)
    s1 = torch.empty_like(scale_tril)
    status = torch.empty(N, device=mean.device, dtype=torch.int32)
    check(lib.bpk_ukf_smooth_f32(mean.data_ptr(), scale_tril.data_ptr(), x_points.data_ptr(),
                                 y_points.data_ptr(), pred_mean.data_ptr(), pred_tril.data_ptr(),
                                 next_mean.data_ptr(), next_tril.data_ptr(), m1.data_ptr(),
                                 s1.data_ptr(), status.data_ptr(), N, n, float(wc0), float(wi),
                                 int(groups), stream_ptr(mean.device)), what)
    return m1, s1, status


def innovation(z_mean, z_tril, obs, white=True):
    """(z_mean [N, dz], z_tril [N, dz, dz]) from `unscented_root` of the measured points and
    obs [N, dz] -> (white [N, dz], nis [N], loglik [N], status int32 [N]); `white=False` skips
    the whitened innovation (None is returned in its place)."""
    what = "ukf.innovation"
    _f32(what, z_mean, z_tril, obs)
    if z_mean.ndim != 2:
        raise RuntimeError(f"{what}: z_mean must be [N, dz]")
    N, dz = z_mean.shape
    _shape(what, "z_tril", z_tril, (N, dz, dz))
    _shape(what, "obs", obs, (N, dz))
    _geo(what, N, 1, 1, dz=dz)
    z_mean, z_tril, obs = z_mean.contiguous(), z_tril.contiguous(), obs.contiguous()
    dev = z_mean.device
    e = torch.empty(N, dz, device=dev, dtype=torch.float32) if white else None
    nis = torch.empty(N, device=dev, dtype=torch.float32)
    loglik = torch.empty(N, device=dev, dtype=torch.float32)
    status = torch.empty(N, device=dev, dtype=torch.int32)
    check(lib.bpk_ukf_innovation_f32(z_mean.data_ptr(), z_tril.data_ptr(), obs.data_ptr(),
                                     None if e is None else e.data_ptr(), nis.data_ptr(),
                                     loglik.data_ptr(), status.data_ptr(), N, dz,
                                     stream_ptr(dev)), what)
    return e, nis, loglik, status

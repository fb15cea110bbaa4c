"""`op.letkf` -- the analysis step of the local ensemble transform Kalman filter on HIP
(csrc/letkf.hip; Hunt, Kostelich & Szunyogh 2007): `analysis` for an identity observation of
the state, `analysis_obs` for observations on a grid of their own behind any operator.

For an ensemble ens [B, m, C, H, W] (2 <= m <= 64 members, 1 <= C <= 8 channels), an
observation obs [B, C, H, W] with inverse variances prec [B, C, H, W] (0 = unobserved) and a
table of localization weights taper [2R+1, 2R+1] (0 <= R <= 8), every grid point (b, y0, x0)
solves its own m x m problem over the window |y - y0| <= R, |x - x0| <= R (clipped at the
domain edge), with xbar the member mean, dX_k = ens_k - xbar and rho_j = taper * prec_j:

    A    = (m-1)/inflation I + sum_j rho_j dX_j dX_j^T,    g = sum_j rho_j dX_j (obs_j - xbar_j)
    A    = Q L Q^T
    wbar = Q L^-1 Q^T g,    Wa = sqrt(m-1) Q L^-1/2 Q^T     (symmetric root: mean preserving)
    ens_out[i, :, y0, x0] = xbar + sum_k dX_k[:, y0, x0] (wbar_k + Wa[k, i])

Entries with rho_j == 0 are skipped, so obs may hold anything (NaN included) where prec == 0:
the masked-frame convention of the other Kalman code.  `status` (int32 [B, H, W]) is 1 where
the eigen-iteration hit its sweep cap or the result is not finite; ens_out there is the
background with its perturbations scaled by sqrt(inflation).

`analysis_obs` takes the members in observation space as well, yens [B, m, Cy, Hy, Wy] =
h(ens_k) for any operator h the caller applies (`op.blur.blur2d` for a blurred, low-resolution
image), with obs / prec [B, Cy, Hy, Wy] on that grid.  Observation (i, j) is localized at state
grid point (stride i + offset, stride j + offset); A and g are formed from ybar, dY_k =
yens_k - ybar over the observations whose position lies in the window, and the transform is
applied to the state perturbations dX as above.  With yens = ens, stride 1, offset 0 it gives
`analysis`'s bits.

float32, HIP tensors only, no CPU path and no autograd.  The reference project has no ensemble
filter; the truth is the float64 restatements tests/letkf_ref.py and tests/letkf_obs_ref.py.
"""
from __future__ import annotations

import math

import torch

from ._lib import check, lib, require_hip, stream_ptr

MAX_MEMBERS = 64
MAX_CHANNELS = 8
MAX_RADIUS = 8


def _radius(radius):
    R = int(radius)
    if R != radius or not 0 <= R <= MAX_RADIUS:
        raise ValueError(f"letkf: radius = {radius} must be an integer in [0, {MAX_RADIUS}]")
    return R


def gaspari_cohn(z):
    """The fifth-order piecewise rational function of Gaspari & Cohn 1999 (eq. 4.10) of
    z = distance / cutoff, a float64 tensor: 1 at 0, 0 for z >= 2."""
    z = torch.as_tensor(z, dtype=torch.float64).abs()
    inner = ((((-0.25 * z + 0.5) * z + 0.625) * z - 5.0 / 3.0) * z * z) + 1.0
    zs = z.clamp(min=1.0)  # the outer branch divides by z; it is only used for z >= 1
    outer = (((((zs / 12.0 - 0.5) * zs + 0.625) * zs + 5.0 / 3.0) * zs - 5.0) * zs + 4.0
             - 2.0 / (3.0 * zs))
    out = torch.where(z <= 1.0, inner, outer.clamp(min=0.0))
    return torch.where(z >= 2.0, torch.zeros_like(out), out)


def gaspari_cohn_taper(radius, cutoff=None):
    """CPU float32 [2R+1, 2R+1]: Gaspari-Cohn of the Euclidean grid distance / cutoff, computed
    in float64 and rounded once.  Default cutoff = (R + 1) / 2: the support (2 cutoff = R + 1)
    ends just past the midpoints of the window's edges."""
    R = _radius(radius)
    cutoff = (R + 1) / 2.0 if cutoff is None else float(cutoff)
    if not cutoff > 0:
        raise ValueError(f"letkf: cutoff = {cutoff} must be positive")
    d = torch.arange(-R, R + 1, dtype=torch.float64)
    dist = (d[:, None] ** 2 + d[None, :] ** 2).sqrt()
    return gaspari_cohn(dist / cutoff).to(torch.float32)


def boxcar_taper(radius):
    """CPU float32 [2R+1, 2R+1] of ones: every observation of the window at full weight."""
    R = _radius(radius)
    return torch.ones(2 * R + 1, 2 * R + 1, dtype=torch.float32)


def analysis(ens, obs, prec, taper, inflation=1.0):
    """ens [B, m, C, H, W], obs / prec [B, C, H, W], taper [2R+1, 2R+1] (any device; it is
    moved to ens's) -> (ens_out [B, m, C, H, W], status int32 [B, H, W])."""
    what = "letkf.analysis"
    require_hip(ens, obs, prec, what=what)
    for name, t in (("ens", ens), ("obs", obs), ("prec", prec), ("taper", taper)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{what}: float32 tensors required, {name} is {t.dtype}")
        if torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError(f"{what}: not differentiable ({name} requires grad)")
    if ens.ndim != 5:
        raise RuntimeError(f"{what}: ens must be [B, m, C, H, W], got {list(ens.shape)}")
    B, m, C, H, W = ens.shape
    if not 2 <= m <= MAX_MEMBERS:
        raise RuntimeError(f"{what}: m = {m} out of range [2, {MAX_MEMBERS}]")
    if not 1 <= C <= MAX_CHANNELS:
        raise RuntimeError(f"{what}: C = {C} out of range [1, {MAX_CHANNELS}]")
    for name, t in (("obs", obs), ("prec", prec)):
        if tuple(t.shape) != (B, C, H, W):
            raise RuntimeError(f"{what}: {name} must be {[B, C, H, W]}, got {list(t.shape)}")
    if taper.ndim != 2 or taper.shape[0] != taper.shape[1] or taper.shape[0] % 2 == 0:
        raise RuntimeError(f"{what}: taper must be [2R+1, 2R+1], got {list(taper.shape)}")
    R = taper.shape[0] // 2
    if R > MAX_RADIUS:
        raise RuntimeError(f"{what}: R = {R} out of range [0, {MAX_RADIUS}]")
    inflation = float(inflation)
    if not (inflation > 0 and math.isfinite(inflation)):
        raise RuntimeError(f"{what}: inflation = {inflation} must be positive and finite")
    for name, t in (("ens", ens), ("obs", obs), ("prec", prec)):
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be contiguous")
    dev = ens.device
    taper = taper.to(dev).contiguous()
    out = torch.empty_like(ens)
    status = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    nbytes = lib.bpk_letkf_workspace_bytes(B, m, C, H, W)
    if nbytes < 0:
        raise RuntimeError(f"{what}: B * H * W = {B * H * W} out of range (< 2^31)")
    ws = torch.empty(max(int(nbytes), 4) // 4, device=dev, dtype=torch.float32)
    check(lib.bpk_letkf_analysis_f32(ens.data_ptr(), obs.data_ptr(), prec.data_ptr(),
                                     taper.data_ptr(), out.data_ptr(), status.data_ptr(),
                                     ws.data_ptr(), B, m, C, H, W, R, inflation, stream_ptr(dev)),
          what)
    return out, status


def analysis_obs(ens, yens, obs, prec, taper, inflation=1.0, stride=1, offset=None):
    """ens [B, m, C, H, W], yens [B, m, Cy, Hy, Wy] (the members in observation space),
    obs / prec [B, Cy, Hy, Wy], taper [2R+1, 2R+1] in state-grid units (any device; it is moved
    to ens's).  Observation (i, j) sits at state grid point (stride i + offset,
    stride j + offset); offset=None: (stride - 1) // 2, the sampling of `op.blur.blur2d`.
    -> (ens_out [B, m, C, H, W], status int32 [B, H, W])."""
    what = "letkf.analysis_obs"
    require_hip(ens, yens, obs, prec, what=what)
    for name, t in (("ens", ens), ("yens", yens), ("obs", obs), ("prec", prec), ("taper", taper)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{what}: float32 tensors required, {name} is {t.dtype}")
        if torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError(f"{what}: not differentiable ({name} requires grad)")
    if ens.ndim != 5:
        raise RuntimeError(f"{what}: ens must be [B, m, C, H, W], got {list(ens.shape)}")
    B, m, C, H, W = ens.shape
    if not 2 <= m <= MAX_MEMBERS:
        raise RuntimeError(f"{what}: m = {m} out of range [2, {MAX_MEMBERS}]")
    if not 1 <= C <= MAX_CHANNELS:
        raise RuntimeError(f"{what}: C = {C} out of range [1, {MAX_CHANNELS}]")
    if yens.ndim != 5 or tuple(yens.shape[:2]) != (B, m):
        raise RuntimeError(f"{what}: yens must be [{B}, {m}, Cy, Hy, Wy], got {list(yens.shape)}")
    Cy, Hy, Wy = yens.shape[2:]
    if not 1 <= Cy <= MAX_CHANNELS:
        raise RuntimeError(f"{what}: Cy = {Cy} out of range [1, {MAX_CHANNELS}]")
    if Hy < 1 or Wy < 1:
        raise RuntimeError(f"{what}: Hy = {Hy}, Wy = {Wy} must be >= 1")
    for name, t in (("obs", obs), ("prec", prec)):
        if tuple(t.shape) != (B, Cy, Hy, Wy):
            raise RuntimeError(f"{what}: {name} must be {[B, Cy, Hy, Wy]}, got {list(t.shape)}")
    if taper.ndim != 2 or taper.shape[0] != taper.shape[1] or taper.shape[0] % 2 == 0:
        raise RuntimeError(f"{what}: taper must be [2R+1, 2R+1], got {list(taper.shape)}")
    R = taper.shape[0] // 2
    if R > MAX_RADIUS:
        raise RuntimeError(f"{what}: R = {R} out of range [0, {MAX_RADIUS}]")
    inflation = float(inflation)
    if not (inflation > 0 and math.isfinite(inflation)):
        raise RuntimeError(f"{what}: inflation = {inflation} must be positive and finite")
    if int(stride) != stride or int(stride) < 1:
        raise RuntimeError(f"{what}: stride = {stride} must be an integer >= 1")
    stride = int(stride)
    if offset is None:
        offset = (stride - 1) // 2
    if int(offset) != offset or not 0 <= int(offset) < stride:
        raise RuntimeError(f"{what}: offset = {offset} out of range [0, stride = {stride})")
    offset = int(offset)
    for name, n, N in (("Hy", Hy, H), ("Wy", Wy, W)):
        if stride * (n - 1) + offset > N - 1:
            raise RuntimeError(f"{what}: {name} = {n} does not fit: stride * ({name} - 1) + offset "
                               f"= {stride * (n - 1) + offset} > {name[0]} - 1 = {N - 1}")
    for name, t in (("ens", ens), ("yens", yens), ("obs", obs), ("prec", prec)):
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be contiguous")
    dev = ens.device
    taper = taper.to(dev).contiguous()
    out = torch.empty_like(ens)
    status = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    nbytes = lib.bpk_letkf_obs_workspace_bytes(B, m, C, H, W, Cy, Hy, Wy)
    if nbytes < 0:
        raise RuntimeError(f"{what}: B * H * W = {B * H * W}, B * Hy * Wy = {B * Hy * Wy} out of "
                           "range (< 2^31)")
    ws = torch.empty(max(int(nbytes), 4) // 4, device=dev, dtype=torch.float32)
    check(lib.bpk_letkf_analysis_obs_f32(ens.data_ptr(), yens.data_ptr(), obs.data_ptr(),
                                         prec.data_ptr(), taper.data_ptr(), out.data_ptr(),
                                         status.data_ptr(), ws.data_ptr(), B, m, C, H, W, Cy, Hy,
                                         Wy, stride, offset, R, inflation, stream_ptr(dev)),
          what)
    return out, status

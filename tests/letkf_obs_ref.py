"""NumPy restatement of the LETKF analysis with observations on a grid of their own behind any
operator (include/bpk.h, section "letkf", bpk_letkf_analysis_obs_f32), in the two forms of
tests/letkf_ref.py:

  truth(...)   float64, np.linalg.eigh
  ref32(...)   every operation in float32, the eigenproblem by letkf_ref.jacobi_eigh

The caller passes the members in observation space, yens [B, m, Cy, Hy, Wy]; observation (i, j)
sits at state grid point (stride i + offset, stride j + offset).  With ybar / dY the member mean
and perturbations of yens and xbar / dX those of ens, for every grid point (b, y0, x0):

    A    = (m-1)/inflation I + sum_j rho_j dY_j dY_j^T,   g = sum_j rho_j dY_j (obs_j - ybar_j)
    A    = Q L Q^T,   wbar = Q L^-1 Q^T g,   Wa = sqrt(m-1) Q L^-1/2 Q^T
    out[i, c, y0, x0] = xbar_c + sum_k dX_k[c, y0, x0] (wbar_k + Wa[k, i])

over the observations j whose position lies in the window |y - y0| <= R, |x - x0| <= R (clipped
at the domain edge, all Cy channels), rho_j = taper[y - y0 + R, x - x0 + R] * prec_j, entries
with rho_j == 0 skipped (obs may be NaN there).  Status and fall-back as the kernel's contract.
The observations are scattered to their positions on the state grid (precision 0 everywhere
else) and the window is then walked exactly as letkf_ref.system walks it.  The reference project
has no ensemble filter; nothing here is derived from it.
"""
import numpy as np

from letkf_ref import jacobi_eigh


def scatter(v, H, W, stride, offset):
    """v [..., Hy, Wy] -> [..., H, W]: v at (stride i + offset, stride j + offset), 0 elsewhere."""
    Hy, Wy = v.shape[-2:]
    assert stride >= 1 and 0 <= offset < stride
    assert stride * (Hy - 1) + offset <= H - 1 and stride * (Wy - 1) + offset <= W - 1
    out = np.zeros(v.shape[:-2] + (H, W), v.dtype)
    out[..., offset:offset + stride * Hy:stride, offset:offset + stride * Wy:stride] = v
    return out


def system(ens, yens, obs, prec, taper, inflation, stride, offset, dtype):
    """-> xbar [B, C, H, W], dX [B, m, C, H, W], A [B, H, W, m, m], g [B, H, W, m]."""
    dt = np.dtype(dtype)
    ens, yens, prec, taper = (np.asarray(v, dt) for v in (ens, yens, prec, taper))
    obs = np.asarray(obs, dt)
    B, m, C, H, W = ens.shape
    Cy, Hy, Wy = yens.shape[2:]
    R = taper.shape[0] // 2
    assert taper.shape == (2 * R + 1, 2 * R + 1) and yens.shape[:2] == (B, m)
    assert obs.shape == prec.shape == (B, Cy, Hy, Wy)
    xbar = (ens.sum(1, dtype=dt) / dt.type(m)).astype(dt)
    dX = ens - xbar[:, None]
    ybar = (yens.sum(1, dtype=dt) / dt.type(m)).astype(dt)
    with np.errstate(invalid="ignore"):
        innov = np.where(prec != 0, obs - ybar, 0).astype(dt)  # skipped, not multiplied
    dY = scatter(yens - ybar[:, None], H, W, stride, offset)   # [B, m, Cy, H, W]
    prec = scatter(prec, H, W, stride, offset)                  # [B, Cy, H, W]
    innov = scatter(innov, H, W, stride, offset)
    A = np.zeros((B, H, W, m, m), dt)
    g = np.zeros((B, H, W, m), dt)
    A[..., np.arange(m), np.arange(m)] = dt.type(m - 1) / dt.type(inflation)
    for dy in range(-R, R + 1):
        ys = slice(max(0, -dy), min(H, H - dy))           # centres y0
        yw = slice(max(0, -dy) + dy, min(H, H - dy) + dy)  # window rows y = y0 + dy
        if ys.start >= ys.stop:
            continue
        for dx in range(-R, R + 1):
            xs = slice(max(0, -dx), min(W, W - dx))
            xw = slice(max(0, -dx) + dx, min(W, W - dx) + dx)
            if xs.start >= xs.stop or taper[dy + R, dx + R] == 0:
                continue
            rho = taper[dy + R, dx + R] * prec[:, :, yw, xw]           # [B, Cy, h, w]
            d = dY[:, :, :, yw, xw]                                    # [B, m, Cy, h, w]
            v = np.where(rho != 0, innov[:, :, yw, xw], 0).astype(dt)
            A[:, ys, xs] += np.einsum("bkcyx,bcyx,blcyx->byxkl", d, rho, d).astype(dt)
            g[:, ys, xs] += np.einsum("bkcyx,bcyx->byxk", d, rho * v).astype(dt)
    assert A.dtype == dt and g.dtype == dt
    return xbar, dX, A, g


def analysis(ens, yens, obs, prec, taper, inflation=1.0, stride=1, offset=None,
             dtype=np.float64, solver="eigh"):
    """-> (ens_out [B, m, C, H, W] in `dtype`, status int32 [B, H, W]).  offset=None:
    (stride - 1) // 2.  status / fall-back as the kernel's contract: 1 where the Jacobi
    iteration was capped or the result is not finite, and the output there is
    xbar + sqrt(inflation) dX."""
    dt = np.dtype(dtype)
    offset = (stride - 1) // 2 if offset is None else offset
    xbar, dX, A, g = system(ens, yens, obs, prec, taper, inflation, stride, offset, dt)
    B, m, C, H, W = dX.shape
    flat = A.reshape(-1, m, m)
    if solver == "eigh":
        lam, Q = np.linalg.eigh(flat)
        capped = np.zeros(len(flat), bool)
    elif solver == "jacobi":
        lam, Q, _, capped = jacobi_eigh(flat)
    else:
        raise ValueError(solver)
    lam, Q = lam.astype(dt).reshape(B, H, W, m), Q.astype(dt).reshape(B, H, W, m, m)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.einsum("byxkl,byxk->byxl", Q, g) / lam
        wbar = np.einsum("byxkl,byxl->byxk", Q, z)
        Wa = np.einsum("byxkl,byxl,byxil->byxki", Q, np.sqrt(dt.type(m - 1)) / np.sqrt(lam), Q)
        T = (wbar[..., None] + Wa).astype(dt)
        out = xbar[:, None] + np.einsum("bkcyx,byxki->bicyx", dX, T)
    out = out.astype(dt)
    status = capped.reshape(B, H, W) | ~np.isfinite(out).all(axis=(1, 2))
    fallback = xbar[:, None] + np.sqrt(dt.type(inflation)) * dX
    out = np.where(status[:, None, None], fallback, out).astype(dt)
    return out, status.astype(np.int32)


def truth(ens, yens, obs, prec, taper, inflation=1.0, stride=1, offset=None):
    return analysis(ens, yens, obs, prec, taper, inflation, stride, offset, np.float64, "eigh")


def ref32(ens, yens, obs, prec, taper, inflation=1.0, stride=1, offset=None):
    return analysis(ens, yens, obs, prec, taper, inflation, stride, offset, np.float32, "jacobi")


def kalman_update_linear(ens, Hmat, obs, prec):
    """The textbook update of one sample's whole state through a dense linear observation
    operator (float64): ens [m, n], Hmat [p, n], obs / prec [p] (prec 0 = unobserved), Y = H X
    -> (mean [n], cov [n, n]) with mean = xbar + K (y - H xbar), cov = (I - K H) Pb,
    Pb = dX dX^T / (m - 1), K = Pb H^T (H Pb H^T + R)^-1 over the observed rows of H."""
    ens = np.asarray(ens, np.float64)
    m, n = ens.shape
    xbar = ens.mean(0)
    dX = ens - xbar
    Pb = dX.T @ dX / (m - 1)
    sel = np.flatnonzero(np.asarray(prec) != 0)
    Hm = np.asarray(Hmat, np.float64)[sel]
    Rm = np.diag(1.0 / np.asarray(prec, np.float64)[sel])
    K = Pb @ Hm.T @ np.linalg.inv(Hm @ Pb @ Hm.T + Rm)
    mean = xbar + K @ (np.asarray(obs, np.float64)[sel] - Hm @ xbar)
    return mean, (np.eye(n) - K @ Hm) @ Pb


def binomial_blur(x):
    """The 3-tap binomial blur (1, 2, 1) / 4 along the last two axes with symmetric boundary
    (edge sample repeated), in x's dtype."""
    for ax in (-2, -1):
        p = np.concatenate([np.take(x, [0], ax), x, np.take(x, [-1], ax)], ax)
        n = x.shape[ax]
        lo, mid, hi = (np.take(p, np.arange(k, k + n), ax) for k in range(3))
        x = 0.25 * lo + 0.5 * mid + 0.25 * hi
    return x

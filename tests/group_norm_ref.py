"""GroupNorm (+ per-(n, c) bias before the norm, + SiLU after) as plain float64 (helper, not a
test): the truth the tests of csrc/group_norm.hip are held against, written from the definition

    h = x + b[n, c],   mean, var over the (C / G) H W elements of a (sample, group),
    y = act((h - mean) rstd gamma[c] + beta[c]),   rstd = (var + eps)^-1/2,

with the closed-form backward, the (s, t) table of the conv prologue, the equal-count partial
statistics, and -- as yardsticks, not truth -- the reference's own float32 arithmetic
(fp32_chain: torch.native_group_norm, F.silu and autograd on the CPU) and a numpy float32
emulation of the summation orders the kernels document (emulate_f32: two-pass statistics, Chan's
combination of chunk partials in chunk order, the equal-count combination of producer partials).
Nothing here imports op.*.

The case table (CASES, VARIANTS) is shared by the host test, which measures the gate's factor
on the emulation, and the GPU test, which applies it.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -20  # exact in float32; rstd of a constant group is exactly 1024

# id -> (N, C, G, H, W): the smallest shapes that enter each dispatch path of group_norm.hip
CASES = {
    "a": (2, 8, 4, 2, 2),       # S 8: resident 256x1; backward segment mode, L = 1
    "b": (2, 6, 3, 1, 1),       # S 2: one pixel per plane, scalar path, segment mode
    "c": (1, 8, 2, 5, 5),       # S 100: scalar, backward LDS-atomic mode
    "d": (2, 32, 8, 16, 16),    # S 1024: L = 64, slice mode, one slice per channel
    "e": (1, 16, 1, 24, 24),    # S 9216: G = 1, 512x8 rung, L = 144: atomic mode at W = 4
    "f": (3, 16, 16, 16, 16),   # S 256: one channel per group
    "g": (1, 32, 4, 64, 64),    # S 32768: last backward resident rung, 16 slices per channel
    "h": (1, 8, 2, 128, 128),   # S 65536: last forward rung; backward split, one slice / channel
    "i": (1, 64, 2, 48, 48),    # S 73728: ragged 4.5th forward chunk; backward planes 7,7,7,7,4
    "j": (1, 6, 2, 160, 160),   # S 76800: backward split, slices 16384 + 9216 per channel
    "k": (1, 32, 8, 65, 65),    # S 16900: scalar slab above the scalar forward ladder
    "l": (1, 32, 4, 45, 45),    # S 16200: scalar, last forward rung, above the backward ladder
    "m": (1, 64, 2, 33, 33),    # S 34848: scalar split both ways; backward planes 3,...,3,2
}
# n: d and g again with x, dy, addend as contiguous views one float into their storage
MISALIGNED = {"nd": "d", "ng": "g"}

MODES = ("plain", "offset", "constant", "saturated")
# backward forms: full = every gradient; add_bnc = addend with d bias_nc wanted (the wrapper
# adds it after the kernel); add = addend fused into the kernel; dx = dx alone (NULL partials)
BWD = ("full", "add_bnc", "add", "dx")


def _v(case, mode="plain", act=1, bnc=True, affine=True, bwd="full"):
    return (case, mode, act, bnc, affine, bwd)


# every case: plain, act = 1, bias_nc, affine, every gradient; the other variants are spread so
# that each is seen on a resident, a split and a scalar (W = 1) case
VARIANTS = [_v(c) for c in list(CASES) + list(MISALIGNED)] + [
    _v("d", act=0), _v("i", act=0), _v("k", act=0), _v("b", act=0),
    _v("a", bnc=False), _v("j", bnc=False), _v("l", bnc=False),
    _v("e", affine=False), _v("h", affine=False), _v("m", affine=False), _v("c", affine=False),
    _v("a", "offset"), _v("d", "offset"), _v("g", "offset"), _v("i", "offset"),
    _v("k", "offset"), _v("ng", "offset"),
    _v("d", "constant"), _v("j", "constant"), _v("m", "constant"), _v("c", "constant", act=0),
    _v("g", "saturated"), _v("i", "saturated"), _v("l", "saturated"), _v("c", "saturated"),
    _v("d", bwd="add_bnc"), _v("h", bwd="add_bnc"), _v("k", bwd="add_bnc"),
    _v("d", bwd="add"), _v("h", bwd="add"), _v("k", bwd="add"), _v("nd", bwd="add"),
    _v("a", bwd="dx"), _v("j", bwd="dx"), _v("m", bwd="dx"), _v("e", bwd="dx"),
]


def variant_id(v):
    case, mode, act, bnc, affine, bwd = v
    return "-".join([case, mode, f"act{act}"] + ([] if bnc else ["nobnc"])
                    + ([] if affine else ["noaffine"]) + [bwd])


def shape_of(case):
    return CASES[MISALIGNED.get(case, case)]


# ------------------------------------------------------------------ float64 truth
def _d(t):
    return None if t is None else t.detach().double().cpu()


def _silu(z):
    return z * torch.sigmoid(z)


def _dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _stats(x, bias_nc, G, eps):
    N, C = x.shape[:2]
    h = x if bias_nc is None else x + bias_nc[:, :, None, None]
    hg = h.reshape(N, G, -1)
    mean = hg.mean(2)
    var = ((hg - mean[:, :, None]) ** 2).mean(2)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((hg - mean[:, :, None]) * rstd[:, :, None]).reshape(x.shape)
    return mean, rstd, xhat


def _per_channel(p, C, G):
    """[N, G] -> [N, C]: the group's value for each of its channels."""
    return p.repeat_interleave(C // G, dim=1)


def forward(x, bias_nc, gamma, beta, G, eps, act):
    """(y, mean [N, G], rstd [N, G]) in float64."""
    x, bias_nc, gamma, beta = _d(x), _d(bias_nc), _d(gamma), _d(beta)
    mean, rstd, z = _stats(x, bias_nc, G, eps)
    if gamma is not None:
        z = z * gamma[None, :, None, None]
    if beta is not None:
        z = z + beta[None, :, None, None]
    return (_silu(z) if act else z), mean, rstd


def affine_table(x, bias_nc, gamma, beta, G, eps):
    """(s, t) [N, C] each: act(GN(x + b)) == act(x s + t)."""
    x, bias_nc, gamma, beta = _d(x), _d(bias_nc), _d(gamma), _d(beta)
    N, C = x.shape[:2]
    mean, rstd, _ = _stats(x, bias_nc, G, eps)
    s = _per_channel(rstd, C, G) * (1.0 if gamma is None else gamma[None, :])
    b = 0.0 if bias_nc is None else bias_nc
    t = (0.0 if beta is None else beta[None, :]) + (b - _per_channel(mean, C, G)) * s
    return s, t


def backward(dy, x, bias_nc, gamma, beta, G, eps, act, addend=None):
    """dict(dx, d_bnc, dgamma, dbeta, dgamma_nc, dbeta_nc) in closed form, float64.  With
    z = xhat gamma + beta and dz = dy act'(z):  dgamma_nc = sum_hw dz xhat, dbeta_nc = sum_hw dz,
    dxhat = dz gamma, dx = rstd (dxhat - <dxhat> - xhat <dxhat xhat>) (<.> the group mean),
    d_bnc = sum_hw dx; then dx += addend (d_bnc stays the GroupNorm part alone)."""
    dy, x, bias_nc, gamma, beta, addend = (_d(t) for t in (dy, x, bias_nc, gamma, beta, addend))
    N, C = x.shape[:2]
    _, rstd, xhat = _stats(x, bias_nc, G, eps)
    ga = torch.ones(C, dtype=torch.float64) if gamma is None else gamma
    be = torch.zeros(C, dtype=torch.float64) if beta is None else beta
    z = xhat * ga[None, :, None, None] + be[None, :, None, None]
    dz = dy * _dsilu(z) if act else dy
    dgamma_nc = (dz * xhat).sum((2, 3))
    dbeta_nc = dz.sum((2, 3))
    dxhat = dz * ga[None, :, None, None]
    A = dxhat.reshape(N, G, -1).mean(2)
    B = (dxhat * xhat).reshape(N, G, -1).mean(2)
    bc = lambda p: _per_channel(p, C, G)[:, :, None, None]  # noqa: E731
    dx = bc(rstd) * (dxhat - bc(A) - xhat * bc(B))
    if C == G:  # the plane is the whole group and dx sums to zero over a group, identically
        dx_sum = torch.zeros(N, C, dtype=torch.float64)
    else:
        dx_sum = dx.sum((2, 3))
    out = {"d_bnc": dx_sum, "dgamma": dgamma_nc.sum(0), "dbeta": dbeta_nc.sum(0),
           "dgamma_nc": dgamma_nc, "dbeta_nc": dbeta_nc}
    out["dx"] = dx if addend is None else dx + addend
    return out


def partials(x, cnt):
    """[N, C, R, 2] (mean, M2) of each run of cnt consecutive pixels, float64."""
    x = _d(x)
    N, C = x.shape[:2]
    r = x.reshape(N, C, -1, cnt)
    m = r.mean(3)
    return torch.stack([m, ((r - m[..., None]) ** 2).sum(3)], 3)


def combine_equal_count(part, cnt, bias_nc, G, eps):
    """(mean, rstd) [N, G] of GroupNorm(x + b) from equal-count partials [N, C, R, 2], in the
    dtype of part: the group mean is the mean of the (biased) partial means, and
    M2 = sum(M2_i + cnt (mean_i + b_c - mean)^2)."""
    N, C, R, _ = part.shape
    m = part[..., 0] if bias_nc is None else part[..., 0] + bias_nc.to(part.dtype)[:, :, None]
    mg = m.reshape(N, G, -1)
    mean = mg.mean(2)
    m2 = (part[..., 1].reshape(N, G, -1) + cnt * (mg - mean[:, :, None]) ** 2).sum(2)
    return mean, 1.0 / torch.sqrt(m2 / (mg.shape[2] * cnt) + eps)


def table_from_stats(mean, rstd, bias_nc, gamma, beta, C):
    """(s, t) [N, C] from group statistics [N, G], in their dtype."""
    G = mean.shape[1]
    dt = mean.dtype
    s = _per_channel(rstd, C, G) * (1.0 if gamma is None else gamma.to(dt)[None, :])
    b = 0.0 if bias_nc is None else bias_nc.to(dt)
    t = (0.0 if beta is None else beta.to(dt)[None, :]) + (b - _per_channel(mean, C, G)) * s
    return s, t


def affine_silu(x, ss):
    """silu(x s + t) for ss [N, C, 2], exact z sigmoid(z) in float64; also returns z."""
    x, ss = _d(x), _d(ss)
    z = x * ss[:, :, 0, None, None] + ss[:, :, 1, None, None]
    return _silu(z), z


# ------------------------------------------------------------------ float32 yardstick
def fp32_chain(x, bias_nc, gamma, beta, G, eps, act, dy=None, addend=None):
    """The reference arithmetic in float32 on the CPU: torch.native_group_norm (y, mean, rstd),
    F.silu, autograd, and the table formed from its statistics in float32.  One sample at a
    time, so the per-sample dgamma_nc / dbeta_nc are autograd's own."""
    x = x.detach().float().cpu()
    N, C = x.shape[:2]
    HW = x[0, 0].numel()
    ys, means, rstds, g = [], [], [], {k: [] for k in ("dx", "d_bnc", "dgamma_nc", "dbeta_nc")}
    for n in range(N):
        xn = x[n:n + 1].clone().requires_grad_()
        bn = None if bias_nc is None else bias_nc[n:n + 1].detach().float().clone().requires_grad_()
        ga = None if gamma is None else gamma.detach().float().clone().requires_grad_()
        be = None if beta is None else beta.detach().float().clone().requires_grad_()
        h = xn if bn is None else xn + bn[:, :, None, None]
        out, m, r = torch.native_group_norm(h, ga, be, 1, C, HW, G, eps)
        y = F.silu(out) if act else out
        ys.append(y.detach()), means.append(m.detach().reshape(1, G))
        rstds.append(r.detach().reshape(1, G))
        if dy is not None:
            leaves = {k: t for k, t in zip(g, (xn, bn, ga, be)) if t is not None}
            grads = torch.autograd.grad(y, list(leaves.values()),
                                        dy[n:n + 1].detach().float().cpu())
            for k, gr in zip(leaves, grads):
                g[k].append(gr if k == "dx" else gr.reshape(1, C))
    res = {"y": torch.cat(ys), "mean": torch.cat(means), "rstd": torch.cat(rstds)}
    res["s"], res["t"] = table_from_stats(
        res["mean"], res["rstd"], None if bias_nc is None else bias_nc.detach().float().cpu(),
        None if gamma is None else gamma.detach().float().cpu(),
        None if beta is None else beta.detach().float().cpu(), C)
    if dy is not None:
        for k, v in g.items():
            if v:
                res[k] = torch.cat(v)
        if addend is not None:
            res["dx"] = addend.detach().float().cpu() + res["dx"]
        if "dgamma_nc" in res:
            res["dgamma"], res["dbeta"] = res["dgamma_nc"].sum(0), res["dbeta_nc"].sum(0)
    return res


# ------------------------------------------------------------------ float32 emulation
f32 = np.float32
FWD_LADDER = ((256, 1), (256, 2), (256, 4), (256, 8), (512, 8), (1024, 8), (1024, 16))
BWD_LADDER = FWD_LADDER[:-1]
SPLIT_CHUNK = 256 * 16 * 4  # floats per split-path chunk at W = 4; a quarter of it at W = 1


def plan(S, HW, aligned, ladder):
    """(W, (T, VPT) or None, chunk): the documented dispatch.  W = 4 for 4-aligned planes behind
    16-byte aligned pointers, else 1; the resident rung is the first of the ladder holding
    ceil(S / W) units of W floats, None (split path, chunks of `chunk` floats) above it."""
    W = 4 if (HW % 4 == 0 and aligned) else 1
    units = -(-S // W)
    rung = next(((T, V) for T, V in ladder if units <= T * V), None)
    return W, rung, SPLIT_CHUNK // (4 // W)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _block_sum(per_thread):
    """Butterfly over each 64-lane wave, then the waves in order."""
    w = per_thread.astype(f32).reshape(-1, 64)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, idx ^ off]
    r = f32(0)
    for i in range(w.shape[0]):
        r = f32(r + w[i, 0])
    return r


def _two_pass(v, T, VPT, W):
    """(mean, M2) of the float32 vector v as a block of T threads holding VPT units of W
    consecutive floats each computes them: per-thread sums in (k, q) order, block_sum."""
    n = v.size
    pad = np.zeros(T * VPT * W, f32)
    pad[:n] = v
    live = np.zeros(T * VPT * W, bool)
    live[:n] = True
    a, live = pad.reshape(VPT, T, W), live.reshape(VPT, T, W)
    ls = np.zeros(T, f32)
    for k in range(VPT):
        for q in range(W):
            ls = ls + a[k, :, q]
    mean = f32(_block_sum(ls) / f32(n))
    lm = np.zeros(T, f32)
    for k in range(VPT):
        for q in range(W):
            d = (a[k, :, q] - mean).astype(f32)
            lm = np.where(live[k, :, q], _fma(d, d, lm), lm)
    return mean, _block_sum(lm)


def _chan(parts):
    """Chan's combination of (count, mean, M2) float32 triples in list order."""
    count, mean, m2 = parts[0]
    for nb, mb, m2b in parts[1:]:
        nn = f32(count + nb)
        d = f32(mb - mean)
        mean = f32(mean + f32(d * f32(nb / nn)))
        m2 = f32(m2 + f32(m2b + f32(f32(d * d) * f32(f32(count * nb) / nn))))
        count = nn
    return count, mean, m2


def _rstd32(var, eps):
    return f32(f32(1) / np.sqrt(f32(var + f32(eps)), dtype=f32))


def _exp32(z):
    with np.errstate(over="ignore"):
        return np.exp(z.astype(np.float64)).astype(f32)


def emulate_f32(x, bias_nc, gamma, beta, G, eps, act, dy=None, addend=None, aligned=True):
    """numpy float32 emulation of the kernels' documented arithmetic, as a dict like
    fp32_chain's: y / mean_saved / rstd_saved by the forward's plan (resident two-pass, or
    chunk partials combined by Chan in chunk order); mean / rstd / s / t as the statistics pass
    of the table computes them (always chunk partials); gradients from the saved statistics
    with float32 sums."""
    x = x.detach().float().cpu().numpy()
    N, C = x.shape[:2]
    HW = x[0, 0].size
    cpg = C // G
    S = cpg * HW
    b = np.zeros((N, C), f32) if bias_nc is None else bias_nc.detach().float().cpu().numpy()
    ga = np.ones(C, f32) if gamma is None else gamma.detach().float().cpu().numpy()
    be = np.zeros(C, f32) if beta is None else beta.detach().float().cpu().numpy()
    h = (x.reshape(N, C, HW) + b[:, :, None]).astype(f32)
    W, rung, chunk = plan(S, HW, aligned, FWD_LADDER)

    def split_stats(v):
        parts = []
        for e0 in range(0, S, chunk):
            c = v[e0:e0 + chunk]
            m, m2 = _two_pass(c, 256, 16, W)
            parts.append((f32(c.size), m, m2))
        count, mean, m2 = _chan(parts)
        return mean, _rstd32(f32(m2 / count), eps)

    mean_s, rstd_s, mean_t, rstd_t = (np.zeros((N, G), f32) for _ in range(4))
    for n in range(N):
        for g in range(G):
            v = h[n, g * cpg:(g + 1) * cpg].reshape(-1)
            mean_t[n, g], rstd_t[n, g] = split_stats(v)
            if rung is None:
                mean_s[n, g], rstd_s[n, g] = mean_t[n, g], rstd_t[n, g]
            else:
                m, m2 = _two_pass(v, rung[0], rung[1], W)
                mean_s[n, g], rstd_s[n, g] = m, _rstd32(f32(m2 / f32(S)), eps)
    pc = lambda p: np.repeat(p, cpg, axis=1)[:, :, None]  # noqa: E731
    xhat = ((h - pc(mean_s)).astype(f32) * pc(rstd_s)).astype(f32)
    z = _fma(xhat, ga[None, :, None], be[None, :, None])
    sig = (f32(1) / (f32(1) + _exp32(-z))).astype(f32)
    y = (z * sig).astype(f32) if act else z
    sc = (np.repeat(rstd_t, cpg, axis=1) * ga[None, :]).astype(f32)
    t = _fma((b - np.repeat(mean_t, cpg, axis=1)).astype(f32), sc, be[None, :])
    res = {"y": y.reshape(x.shape), "mean": mean_t, "rstd": rstd_t, "s": sc, "t": t,
           "mean_saved": mean_s, "rstd_saved": rstd_s}
    if dy is not None:
        gv = dy.detach().float().cpu().numpy().reshape(N, C, HW)
        dz = (gv * (sig * (f32(1) + z * (f32(1) - sig))).astype(f32)).astype(f32) if act else gv
        dgn = (dz * xhat).astype(f32).sum(2, dtype=f32)
        dbn = dz.sum(2, dtype=f32)
        dxh = (dz * ga[None, :, None]).astype(f32)
        A = (dxh.reshape(N, G, -1).sum(2, dtype=f32) / f32(S)).astype(f32)
        B = ((dxh * xhat).astype(f32).reshape(N, G, -1).sum(2, dtype=f32) / f32(S)).astype(f32)
        dx = (pc(rstd_s) * (dxh - pc(A) - (xhat * pc(B)).astype(f32)).astype(f32)).astype(f32)
        res.update(d_bnc=dx.sum(2, dtype=f32), dgamma_nc=dgn, dbeta_nc=dbn,
                   dgamma=dgn.sum(0, dtype=f32), dbeta=dbn.sum(0, dtype=f32))
        if addend is not None:
            dx = (addend.detach().float().cpu().numpy().reshape(N, C, HW) + dx).astype(f32)
        res["dx"] = dx.reshape(x.shape)
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in res.items()}


def emulate_partials_f32(part, cnt, bias_nc, G, eps):
    """(mean, rstd) float32 [N, G] by the equal-count combination as one block of 256 threads
    runs it: thread i sums partials i, i + 256, ... in order, block_sum, two passes."""
    p = part.detach().float().cpu().numpy()
    N, C, R, _ = p.shape
    cpg = C // G
    K = cpg * R
    b = np.zeros((N, C), f32) if bias_nc is None else bias_nc.detach().float().cpu().numpy()
    m = (p[..., 0] + b[:, :, None]).astype(f32).reshape(N, G, K)
    q = p[..., 1].reshape(N, G, K)
    mean, rstd = np.zeros((N, G), f32), np.zeros((N, G), f32)
    passes = -(-K // 256)
    for n in range(N):
        for g in range(G):
            pm, pq = np.zeros(passes * 256, f32), np.zeros(passes * 256, f32)
            pm[:K], pq[:K] = m[n, g], q[n, g]
            live = (np.arange(passes * 256) < K).reshape(passes, 256)
            pm, pq = pm.reshape(passes, 256), pq.reshape(passes, 256)
            ls = np.zeros(256, f32)
            for k in range(passes):
                ls = ls + pm[k]
            mu = f32(_block_sum(ls) / f32(K))
            lm = np.zeros(256, f32)
            for k in range(passes):
                d = (pm[k] - mu).astype(f32)
                lm = np.where(live[k], (lm + _fma(f32(cnt) * d, d, pq[k])).astype(f32), lm)
            mean[n, g] = mu
            rstd[n, g] = _rstd32(f32(_block_sum(lm) / f32(f32(K) * f32(cnt))), eps)
    return torch.from_numpy(mean), torch.from_numpy(rstd)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(shape, mode, seed):
    """Seeded float32 CPU dict(x, bnc, gamma, beta, dy, addend) for (N, C, G, H, W) (cached: read
    only).  plain: x = 2 randn + 0.5.  offset: x = 100 + randn and bias_nc = +-50 (1 + 0.1 u),
    sign alternating over channels and samples, so the group variance is the between-channel
    term.  constant: group 0 of every sample has x = 0.5 and bias -0.5, so x + b = 0 in every
    element once the bias is added and y = act(beta) exactly, in the reference's float32 chain
    too (a non-zero constant is not reproduced exactly by either: aten folds the mean into a
    per-channel shift, beta - mean rstd gamma, that rounds at the scale of 1024 mean, and a
    sum-based mean of a constant that is not dyadic is off by an ulp, which rstd = 1024 turns
    into 1e-4 -- true of any float32 GroupNorm, and no bug); the other groups plain.  saturated: |gamma| about 30, so |z| reaches 100 where |xhat| passes 3.3."""
    assert mode in MODES
    N, C, G, H, W = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x, bnc = r(N, C, H, W) * 2 + 0.5, r(N, C)
    gamma, beta = 1 + 0.5 * r(C), 0.5 * r(C)
    dy, addend = r(N, C, H, W), r(N, C, H, W)
    if C // G * H * W == 2:
        # two elements per group: xhat = +-(1 + eps / var)^-1/2, and with var >> eps both are
        # +-1 and dx = rstd (dxhat - <dxhat> - xhat <dxhat xhat>) cancels to a residue of order
        # eps / var, which no float32 arithmetic resolves.  Scaled (exactly) to a spread of the
        # order of sqrt(eps), the case is as well conditioned as the others.
        x, bnc = x * 2.0 ** -10, bnc * 2.0 ** -10
    if mode == "offset":
        x = 100 + r(N, C, H, W)
        sign = 1.0 - 2.0 * ((torch.arange(C)[None, :] + torch.arange(N)[:, None]) % 2)
        bnc = 50 * sign * (1 + 0.1 * torch.rand(N, C, generator=g))
    elif mode == "constant":
        assert G >= 2
        x[:, :C // G] = 0.5
        bnc[:, :C // G] = -0.5
    elif mode == "saturated":
        sign = 1.0 - 2.0 * (torch.arange(C) % 2)
        gamma = 30 * sign * (1 + 0.1 * torch.rand(C, generator=g))
    return {"x": x.contiguous(), "bnc": bnc.contiguous(), "gamma": gamma, "beta": beta,
            "dy": dy, "addend": addend}


def variant_inputs(v):
    """The tensors variant v runs on (absent ones None) and its (G, act, bwd, aligned)."""
    case, mode, act, bnc, affine, bwd = v
    shape = shape_of(case)
    seed = 1000 + 16 * list(CASES).index(MISALIGNED.get(case, case)) + MODES.index(mode)
    d = dict(inputs(shape, mode, seed))
    if not bnc:
        d["bnc"] = None
    if not affine:
        d["gamma"] = d["beta"] = None
    if bwd not in ("add", "add_bnc"):
        d["addend"] = None
    return d, shape[2], act, bwd, case not in MISALIGNED


# Tensor groups sharing one yardstick E.  The gradients are two groups: dx and its plane sums
# d_bnc cancel within a group (sum over a group of dx = 0), the parameter gradients do not, and
# one must not be judged by the other's error.
GROUPS = {"forward": ("y",),
          "statistics": ("mean", "rstd", "s", "t", "mean_saved", "rstd_saved"),
          "input gradients": ("dx", "dx_fused", "d_bnc"),
          "parameter gradients": ("dgamma", "dbeta", "dgamma_nc", "dbeta_nc"),
          "zero d_bnc": ()}
E_CEILING = 1e-4  # a float32 chain further than this from the truth is no yardstick


def groups_of(truth):
    """GROUPS for one variant: where d_bnc is identically zero (C == G) its error is absolute
    and gets a yardstick of its own instead of entering a maximum of relative errors."""
    if truth["d_bnc"].abs().max().item() > 0:
        return {g: n for g, n in GROUPS.items() if n}
    g = dict(GROUPS)
    g["input gradients"] = ("dx", "dx_fused")
    g["zero d_bnc"] = ("d_bnc",)
    return g


@functools.lru_cache(maxsize=None)
def reference(v):
    """(inputs, truth, chain) of variant v: truth in float64, chain = fp32_chain, as dicts over
    the names of GROUPS (cached, read only)."""
    d, G, act, bwd, _ = variant_inputs(v)
    y, mean, rstd = forward(d["x"], d["bnc"], d["gamma"], d["beta"], G, EPS, act)
    s, t = affine_table(d["x"], d["bnc"], d["gamma"], d["beta"], G, EPS)
    truth = {"y": y, "mean": mean, "rstd": rstd, "s": s, "t": t, "mean_saved": mean,
             "rstd_saved": rstd}
    truth.update(backward(d["dy"], d["x"], d["bnc"], d["gamma"], d["beta"], G, EPS, act,
                          d["addend"]))
    truth["dx_fused"] = truth["dx"]
    chain = fp32_chain(d["x"], d["bnc"], d["gamma"], d["beta"], G, EPS, act, d["dy"], d["addend"])
    chain["mean_saved"], chain["rstd_saved"] = chain["mean"], chain["rstd"]
    chain["dx_fused"] = chain["dx"]
    return d, truth, chain


def err(t, truth):
    """max|t - truth| / max|truth|; the absolute error where the truth is identically zero."""
    t, truth = t.detach().double().cpu().reshape(-1), truth.double().reshape(-1)
    a = (t - truth).abs().max().item()
    m = truth.abs().max().item()
    return a / m if m > 0 else a


def yardsticks(truth, chain):
    """E per tensor group: the largest error of the float32 chain over the group's tensors
    (groups the variant has no tensor of are absent)."""
    return {grp: max(err(chain[k], truth[k]) for k in names if k in chain)
            for grp, names in groups_of(truth).items() if any(k in chain for k in names)}


# ------------------------------------------------------------------ tables from partials
# (C / G, R, cnt) with N = G = 2: K = C / G * R partials per group against the block's 256 threads
PART_CASES = ((2, 1, 128),    # K = 2
              (4, 64, 128),   # K = 256: exactly one pass of the block
              (6, 50, 64))    # K = 300: ragged second pass


@functools.lru_cache(maxsize=None)
def partials_reference(pc, with_bnc):
    """(part float32 [N, C, R, 2], inputs, truth, chain) for one of PART_CASES in mode offset.
    part is the float32 cast of the float64 partials of x, and the truth is the float64
    equal-count combination of exactly those float32 numbers (what the entry point is given);
    chain is the same combination evaluated by torch in float32."""
    cpg, R, cnt = pc
    N, G = 2, 2
    C = G * cpg
    d = dict(inputs((N, C, G, R, cnt), "offset", 2000 + PART_CASES.index(pc)))
    if not with_bnc:
        d["bnc"] = None
    part = partials(d["x"], cnt).float().contiguous()
    out = []
    for p in (part.double(), part):
        mean, rstd = combine_equal_count(p, cnt, d["bnc"], G, EPS)
        s, t = table_from_stats(mean, rstd, d["bnc"], d["gamma"], d["beta"], C)
        out.append({"mean": mean, "rstd": rstd, "s": s, "t": t})
    return part, d, out[0], out[1]


# The gate: every native error <= FACTOR x E.  FACTOR is twice the worst err(emulate_f32) / E
# over VARIANTS and PART_CASES, rounded up to the next of 2, 4, 8 (test_group_norm_ref_host.py
# measures it and asserts that this constant is that value).
FACTOR = 8.0


# ------------------------------------------------------------------ chunk partials, param grads
CHUNK_CASES = tuple((s, m) for s in ((3, 1, 8, 16), (2, 5, 16, 24)) for m in ("plain", "offset"))


def _butterfly(w):
    """xor butterfly over the last axis (64 lanes), float32: every lane ends with the sum."""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = (w + w[..., idx ^ off]).astype(f32)
    return w[..., 0]


@functools.lru_cache(maxsize=None)
def chunk_reference(shape, mode):
    """(x, truth, chain, emulation) of the (mean, M2) of every run of 128 pixels of x [N, C, H, W]:
    float64; torch float32 (mean(), sum((x - m)^2)); and numpy float32 as one wave computes them
    (two values per lane, xor butterflies)."""
    N, C, H, W = shape
    x = inputs((N, C, 1, H, W), mode, 31)["x"]
    r = x.reshape(N, C, -1, 128)
    m = r.mean(3)
    chain = torch.stack([m, ((r - m[..., None]) ** 2).sum(3)], 3)
    v = r.numpy().reshape(N, C, -1, 64, 2)
    mean = (_butterfly((v[..., 0] + v[..., 1]).astype(f32)) * f32(1 / 128)).astype(f32)
    a = (v[..., 0] - mean[..., None]).astype(f32)
    b = (v[..., 1] - mean[..., None]).astype(f32)
    m2 = _butterfly(_fma(b, b, (a * a).astype(f32)))
    emu = torch.from_numpy(np.stack([mean, m2], -1))
    return x, partials(x, 128), chain, emu


PG_N, PG_C = (1, 3, 4, 9), (1, 64, 65, 130)
PG_HW = ((1, False), (25, False), (64, False), (64, True))  # (H W, dx misaligned)


@functools.lru_cache(maxsize=None)
def param_grads_reference(N, C, HW, misaligned=False):
    """(inputs (dx [N, C, HW], dgamma_nc, dbeta_nc [N, C]), truth, chain, emulation) of
    d_bnc = sum_hw dx, dgamma = sum_n dgamma_nc, dbeta = sum_n dbeta_nc: float64; torch float32
    sums; and numpy float32 in the kernel's documented order (a row by 256 threads, four floats
    at a time on aligned 4-multiple rows, then block_sum; a channel by four waves taking a
    quarter of the samples each in order, then the four partials in wave order)."""
    g = torch.Generator().manual_seed(5000 + 1000 * N + 4 * C + HW)
    dx = torch.randn(N, C, HW, generator=g)
    dg, db = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g) + 1.0
    names = ("d_bnc", "dgamma", "dbeta")
    truth = dict(zip(names, (dx.double().sum(2), dg.double().sum(0), db.double().sum(0))))
    chain = dict(zip(names, (dx.sum(2), dg.sum(0), db.sum(0))))
    rows = dx.numpy().reshape(N * C, HW)
    per = np.zeros((N * C, 256), f32)
    if HW % 4 == 0 and not misaligned:
        q = rows.reshape(N * C, HW // 4, 4)
        per[:, :HW // 4] = ((q[..., 0] + q[..., 1]).astype(f32) + (q[..., 2] + q[..., 3]).astype(f32))
    else:
        per[:, :HW] = rows
    waves = _butterfly(per.reshape(N * C, 4, 64))
    d_bnc = np.zeros(N * C, f32)
    for w in range(4):
        d_bnc = (d_bnc + waves[:, w]).astype(f32)

    def over_n(t):
        t, nq = t.numpy(), (N + 3) // 4
        part = np.zeros((4, C), f32)
        for w in range(4):
            for n in range(w * nq, min(N, (w + 1) * nq)):
                part[w] = (part[w] + t[n]).astype(f32)
        return (((part[0] + part[1]).astype(f32) + part[2]).astype(f32) + part[3]).astype(f32)
    emu = dict(zip(names, (torch.from_numpy(d_bnc.reshape(N, C)), torch.from_numpy(over_n(dg)),
                           torch.from_numpy(over_n(db)))))
    return (dx, dg, db), truth, chain, emu

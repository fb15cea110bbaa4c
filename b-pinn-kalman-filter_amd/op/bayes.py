"""Reparameterized Gaussian weights of a whole network and their KL in one launch
(csrc/bayes.hip; include/bpk.h section "bayes").

`sample_kl(mu, rho, table, seed, step) -> (W, kl)`: mu, rho flat float32 [P] (all kernels and
biases of one network), `table` float64 [S, 4] from `make_table` -- (offset, numel, prior_mu,
prior_sigma) per segment.  W = mu + softplus(rho) * eps with eps the Philox normal of
`op.sde_kernels.philox_normal((1, P), seed, step, draw=0)`; kl = the sum over segments of the
segment mean of KL(N(mu, sigma) || N(prior_mu, prior_sigma)), i.e. bayesian_torch's
`kl_div(...).mean()` per kernel / bias summed by `get_kl_loss`.  W is a fresh tensor per call
(never a rewritten buffer: op.conv caches filter transforms per weight tensor and version).
The backward is one launch that draws eps again from (seed, step); first order only.

BPK_BAYES_FUSED=0: the same arithmetic as an aten composition on the same Philox noise
(softplus, mul, add, the per-element KL term weighted by 1 / numel of its segment and summed;
float32 throughout, plain torch.nn.functional.softplus -- valid for rho >= -80 or so, where
float32 sigma has not yet underflowed).  Read once at import; tests flip `_FUSED`.
"""
from __future__ import annotations

import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import check, lib, require_hip, stream_ptr

_FUSED = os.environ.get("BPK_BAYES_FUSED", "1") == "1"


def make_table(segments, device):
    """float64 [S, 4] device table from [(offset, numel, prior_mu, prior_sigma), ...]; the
    segments must tile [0, P) in order (checked here: the kernel trusts the table)."""
    segments = [(int(o), int(n), float(pm), float(ps)) for o, n, pm, ps in segments]
    if not segments:
        raise ValueError("bayes.make_table: no segments")
    at = 0
    for o, n, _pm, ps in segments:
        if o != at or n < 1:
            raise ValueError(f"bayes.make_table: segment (offset {o}, numel {n}) does not "
                             f"continue the tiling at {at}")
        if not ps > 0:
            raise ValueError(f"bayes.make_table: prior_sigma {ps} must be positive")
        at += n
    return torch.tensor(segments, dtype=torch.float64).to(device)


def _check(mu, rho, table):
    require_hip(mu, rho, table, what="bayes.sample_kl")
    if mu.dtype != torch.float32 or rho.dtype != torch.float32 or table.dtype != torch.float64:
        raise RuntimeError("bayes.sample_kl: mu, rho float32 and table float64 expected")
    if mu.dim() != 1 or mu.shape != rho.shape or table.dim() != 2 or table.shape[1] != 4:
        raise RuntimeError(f"bayes.sample_kl: mu {tuple(mu.shape)}, rho {tuple(rho.shape)}, "
                           f"table {tuple(table.shape)}: flat [P], [P] and [S, 4] expected")
    if not (mu.is_contiguous() and rho.is_contiguous() and table.is_contiguous()):
        raise RuntimeError("bayes.sample_kl: contiguous tensors expected")


class _SampleKL(Function):
    @staticmethod
    def forward(ctx, mu, rho, table, seed, step):
        P, S = mu.numel(), table.shape[0]
        W = torch.empty_like(mu)
        kl = torch.empty((), dtype=torch.float32, device=mu.device)
        ws = torch.empty(max(1, lib.bpk_bayes_workspace_bytes(P) // 8), dtype=torch.float64,
                         device=mu.device)
        check(lib.bpk_bayes_sample_kl_f32(mu.data_ptr(), rho.data_ptr(), table.data_ptr(), S, P,
                                          seed, step, W.data_ptr(), kl.data_ptr(), ws.data_ptr(),
                                          stream_ptr(mu.device)), "bayes.sample_kl")
        ctx.save_for_backward(mu, rho, table)
        ctx.key = (seed, step)
        ctx.set_materialize_grads(False)
        return W, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, gW, gkl):
        mu, rho, table = ctx.saved_tensors
        if gW is None and gkl is None:
            return None, None, None, None, None
        if gW is not None:
            gW = gW.contiguous()
        if gkl is not None:
            gkl = gkl.contiguous()
        gmu, grho = torch.empty_like(mu), torch.empty_like(rho)
        seed, step = ctx.key
        check(lib.bpk_bayes_sample_kl_bwd_f32(
            mu.data_ptr(), rho.data_ptr(), table.data_ptr(), table.shape[0], mu.numel(), seed,
            step, None if gW is None else gW.data_ptr(), None if gkl is None else gkl.data_ptr(),
            gmu.data_ptr(), grho.data_ptr(), stream_ptr(mu.device)), "bayes.sample_kl backward")
        return gmu, grho, None, None, None


def _expanded(table):
    """per-element (prior_mu, prior_sigma, 1 / numel) float32 [P] of a table, kept on it"""
    e = getattr(table, "_bpk_expanded", None)
    if e is None:
        t = table.cpu()
        n = t[:, 1].long()
        e = tuple(torch.repeat_interleave(v.float(), n).to(table.device)
                  for v in (t[:, 2], t[:, 3], 1.0 / t[:, 1]))
        table._bpk_expanded = e
    return e


def noise(P, seed, step, device):
    """eps of `sample_kl` as a tensor [P] (the kernels never store it)."""
    from . import sde_kernels
    st = torch.tensor([step], dtype=torch.int32, device=device)
    return sde_kernels.philox_normal((1, P), seed, st, 0, device=device).view(P)


def sample_kl_aten(mu, rho, table, seed, step):
    """`sample_kl` as an aten composition on the same noise (autograd's own backward)."""
    _check(mu, rho, table)
    pm, ps, invn = _expanded(table)
    eps = noise(mu.numel(), seed, step, mu.device)
    sigma = torch.nn.functional.softplus(rho)
    W = mu + sigma * eps
    term = torch.log(ps / sigma) + (sigma ** 2 + (mu - pm) ** 2) / (2 * ps ** 2) - 0.5
    return W, (term * invn).sum()


def sample_kl(mu, rho, table, seed, step):
    """(W [P], kl []) -- see the module docstring.  `seed`, `step`: host integers."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & 0x7FFFFFFF
    if not _FUSED:
        return sample_kl_aten(mu, rho, table, seed, step)
    _check(mu, rho, table)
    return _SampleKL.apply(mu, rho, table, seed, step)

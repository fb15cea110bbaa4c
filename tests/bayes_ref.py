"""Plain-torch restatement of the Bayesian weight sampler (csrc/bayes.hip, op/bayes.py), meant
to be run in float64: the truth the kernel tests compare against.  The KL formula itself is
anchored to torch.distributions in test_bayes_host.py."""
import torch


def softplus(rho):
    """log(1 + exp(rho)) without overflow or cancellation at either end:
    max(rho, 0) + log1p(exp(-|rho|)), with -|rho| written rho - 2 max(rho, 0) so that autograd
    gives sigmoid(rho) everywhere, rho = 0 included."""
    p = rho.clamp(min=0)
    return p + torch.log1p(torch.exp(rho - 2 * p))


def sample(mu, rho, eps):
    """W = mu + softplus(rho) * eps."""
    return mu + softplus(rho) * eps


def kl(mu, rho, prior_mu, prior_sigma, segments):
    """Sum over segments [(offset, numel), ...] of the segment mean of
    KL(N(mu, softplus(rho)) || N(prior_mu, prior_sigma)); prior_mu / prior_sigma: numbers, or
    one per segment."""
    sigma = softplus(rho)
    total = mu.new_zeros(())
    for i, (off, n) in enumerate(segments):
        pm = prior_mu[i] if hasattr(prior_mu, "__len__") else prior_mu
        ps = prior_sigma[i] if hasattr(prior_sigma, "__len__") else prior_sigma
        m, s = mu[off:off + n], sigma[off:off + n]
        term = torch.log(ps / s) + (s ** 2 + (m - pm) ** 2) / (2 * ps ** 2) - 0.5
        total = total + term.mean()
    return total


def moped_rho(w, delta):
    """rho with softplus(rho) = delta |w| (bayesian_torch's MOPED: log(expm1(delta |w|) + 1e-20))."""
    return torch.log(torch.expm1(delta * w.abs()) + 1e-20)

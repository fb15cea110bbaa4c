"""Bayesian (mean-field Gaussian, reparameterized) conv layers for FlowNet / PressureNet.

The reference converts its nets with `bayesian_torch.models.dnn_to_bnn.dnn_to_bnn`
(pinn_kalman/pinn.py:144-145): every Conv2d / ConvTranspose2d becomes a
Conv2dReparameterization / ConvTranspose2dReparameterization holding mu_kernel, rho_kernel,
mu_bias, rho_bias, and each layer call draws w = mu + log1p(exp(rho)) * eps and returns its KL
to the prior.  bayesian_torch is not pinned by the reference and is not available here, so its
few formulas are restated (as pinn_kalman/ukf.py does for torchfilter) from the library's
documentation; the two initialisations below in particular could not be confirmed against it:

  * default: mu ~ N(posterior_mu_init, 0.1), rho ~ N(posterior_rho_init, 0.1);
  * MOPED (`moped_enable`, Krishnan et al. 2020): mu = w, rho = log(expm1(delta |w|) + 1e-20),
    the same for biases, w the deterministic net's weights.

Layout: a converted net owns ONE flat `mu` and ONE flat `rho` Parameter (`net.bayes`, a
`BayesParams`) in the order of the deterministic net's `parameters()`, plus the segment table
of `op.bayes`.  Adam, clip_grad_norm_, the EMA and the gradient all-reduce then touch 2 tensors
per net instead of ~260, and one `op.bayes.sample_kl` launch draws every weight of the net and
reduces its KL.  The flat sample W is cut into per-layer views by one `op.channels.split` node
(backward: one concatenation).

One draw per network forward (a forward pre-hook on the net), in train() and eval() alike:
every layer of one forward -- both frames of FlowNet's shared feature extractor, PressureNet's
repeated `flow_feature` -- sees ONE consistent network, i.e. one Monte-Carlo run is one sample
of the weight posterior.  bayesian_torch draws per layer call, so the reference's two frames
see different extractor weights; which of the two the authors meant cannot be settled here, and
parity with the library's noise cannot be pinned either way.

Noise: `(seed, step)` of the Philox stream; `step` is a host counter advanced by every draw,
`reseed(seed, step=0)` resets it.  Nothing depends on the rank: a sharded batch sees the same
weights as the single process.

Every draw's weights are fresh tensors (outputs of the sampling Function), never a buffer
rewritten in place: op.conv keeps a conv's filter transform on the weight tensor, keyed by its
version counter.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from op import bayes as bayes_op
from op import channels
from op import conv as conv_op

from . import layers

DEFAULT_PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0,
                 "posterior_rho_init": -3.0, "type": "Reparameterization",
                 "moped_enable": False, "moped_delta": 0.5}

_CONV_ATTRS = ("in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation",
               "groups", "padding_mode", "output_padding")


def moped_rho(w, delta):
    """rho with softplus(rho) = delta |w| (up to the 1e-20 guard), float64 inside."""
    return torch.log(torch.expm1(delta * w.detach().double().abs()) + 1e-20).to(w.dtype)


class BayesParams(nn.Module):
    """The flat variational parameters of one net, its segment table and its noise stream.

    `segments`: [(name, shape)] in flat order, name = '<layer>.weight' / '<layer>.bias'.
    After `draw()`: `sample` (per-segment weight views of this forward's W) and `kl`."""

    def __init__(self, segments, mu, rho, prior_mu, prior_sigma, seed=0):
        super().__init__()
        self.segments = [(n, tuple(s)) for n, s in segments]
        self.sizes = [int(math.prod(s)) for _, s in self.segments]
        self.numel = sum(self.sizes)
        assert mu.shape == rho.shape == (self.numel,)
        self.prior_mu, self.prior_sigma = float(prior_mu), float(prior_sigma)
        self.mu = nn.Parameter(mu)
        self.rho = nn.Parameter(rho)
        rows, at = [], 0
        for n in self.sizes:
            rows.append((at, n, self.prior_mu, self.prior_sigma))
            at += n
        self.rows = rows
        self.register_buffer("table", bayes_op.make_table(rows, mu.device), persistent=False)
        self.seed, self.step = int(seed), 0
        self.sample, self.kl = None, None

    def reseed(self, seed, step=0):
        self.seed, self.step = int(seed), int(step)

    def draw(self):
        """One sample of every weight of the net (and its KL); advances `step`."""
        W, kl = bayes_op.sample_kl(self.mu, self.rho, self.table, self.seed, self.step)
        self.step += 1
        pieces = channels.split(W, self.sizes, 0)
        self.sample = [p.view(s) for p, (_, s) in zip(pieces, self.segments)]
        self.kl = kl
        return W, kl

    def kl_loss(self):
        """KL of the last draw (bayesian_torch.get_kl_loss of the net)."""
        if self.kl is None:
            raise RuntimeError("kl_loss: no forward (draw) has run yet")
        return self.kl


class _BayesConvBase(nn.Module):
    """What layers.conv2d / layers.ConvTranspose2d.forward / ResidualBlock read of a conv
    module; `weight` and `bias` are this forward's sample (views of the net's flat W)."""

    def __init__(self, conv, store, iw, ib):
        super().__init__()
        for a in _CONV_ATTRS:
            setattr(self, a, getattr(conv, a))
        self._store = (store,)  # in a tuple: a reference, not a registered submodule
        self._iw, self._ib = iw, ib

    def _get(self, i):
        sample = self._store[0].sample
        if sample is None:
            raise RuntimeError("Bayesian layer read before its net's forward drew the weights")
        return sample[i]

    @property
    def weight(self):
        return self._get(self._iw)

    @property
    def bias(self):
        return None if self._ib is None else self._get(self._ib)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, "
                f"stride={self.stride}, padding={self.padding}, groups={self.groups}, "
                f"bias={self._ib is not None}")


class BayesConv2d(_BayesConvBase):
    def forward(self, x):
        return layers.conv2d(x, self)


class BayesConvTranspose2d(_BayesConvBase):
    def forward(self, x):
        if not layers._WINO_ENABLED:  # the A/B switch of layers.ConvTranspose2d: MIOpen
            return torch.nn.functional.conv_transpose2d(
                x, self.weight, self.bias, self.stride, self.padding, self.output_padding,
                self.groups, self.dilation)
        return conv_op.conv_transpose2d_general(x, self.weight, self.bias, self.stride,
                                                self.padding, self.output_padding, self.groups,
                                                self.dilation)


_KINDS = {layers.Conv2d: BayesConv2d, nn.Conv2d: BayesConv2d,
          layers.ConvTranspose2d: BayesConvTranspose2d,
          nn.ConvTranspose2d: BayesConvTranspose2d}


def _draw_hook(net, args):
    net.bayes.draw()


def dnn_to_bnn(net, prior, seed=0):
    """Convert `net` (a FlowNet or PressureNet) in place: every layers.Conv2d / nn.Conv2d /
    layers.ConvTranspose2d / nn.ConvTranspose2d becomes a Bayesian stand-in reading the net's
    flat sample; any other layer type with parameters raises.  `prior`: bayesian_torch's
    dictionary (prior_mu, prior_sigma, posterior_mu_init, posterior_rho_init, type,
    moped_enable, moped_delta).  Adds `net.bayes` (BayesParams), `net.kl_loss()` and the
    pre-hook that draws once per forward.  Returns the net."""
    prior = {**DEFAULT_PRIOR, **dict(prior)}
    if prior["type"] != "Reparameterization":
        raise NotImplementedError(f"dnn_to_bnn: type {prior['type']!r} (only Reparameterization)")
    if hasattr(net, "bayes"):
        raise RuntimeError("dnn_to_bnn: the net is converted already")
    if isinstance(net, (nn.Sequential, nn.ModuleList, nn.ModuleDict)):
        raise TypeError("dnn_to_bnn: the net gains a child module (`bayes`), which a bare "
                        f"{type(net).__name__} would take for one of its layers")
    found = []
    for name, m in net.named_modules():
        own = list(m.named_parameters(recurse=False))
        if not own:
            continue
        if type(m) not in _KINDS:
            raise NotImplementedError(
                f"dnn_to_bnn: {name or type(net).__name__} is a {type(m).__name__} with "
                "parameters; only Conv2d / ConvTranspose2d layers are converted")
        if m.padding_mode != "zeros" or isinstance(m.padding, str):
            raise NotImplementedError(f"dnn_to_bnn: {name}: padding {m.padding_mode!r} / "
                                      f"{m.padding!r}")
        found.append((name, m))
    if not found:
        raise RuntimeError("dnn_to_bnn: no convolution layers")
    segments, values = [], []
    for name, m in found:
        segments.append((name + ".weight", m.weight.shape))
        values.append(m.weight.detach().reshape(-1))
        if m.bias is not None:
            segments.append((name + ".bias", m.bias.shape))
            values.append(m.bias.detach().reshape(-1))
    w = torch.cat(values)
    if prior["moped_enable"]:
        mu = w.clone()
        rho = moped_rho(w, float(prior["moped_delta"]))
    else:
        mu = torch.empty(w.shape).normal_(float(prior["posterior_mu_init"]), 0.1).to(w)
        rho = torch.empty(w.shape).normal_(float(prior["posterior_rho_init"]), 0.1).to(w)
    store = BayesParams(segments, mu, rho, prior["prior_mu"], prior["prior_sigma"], seed)
    index = {n: i for i, (n, _) in enumerate(segments)}
    for name, m in found:
        parent = net
        *path, leaf = name.split(".")
        for p in path:
            parent = getattr(parent, p)
        parent._modules[leaf] = _KINDS[type(m)](m, store, index[name + ".weight"],
                                                index.get(name + ".bias"))
    net.bayes = store
    net.kl_loss = store.kl_loss
    net.register_forward_pre_hook(_draw_hook)
    return net


def _lib_key(name):
    layer, kind = name.rsplit(".", 1)
    return layer, ("kernel" if kind == "weight" else "bias")


def to_layerwise_state_dict(net):
    """bayesian_torch's keys: '<layer>.mu_kernel', '<layer>.rho_kernel', '<layer>.mu_bias',
    '<layer>.rho_bias' (copies, in the layers' shapes)."""
    b, out, at = net.bayes, {}, 0
    for (name, shape), n in zip(b.segments, b.sizes):
        layer, kind = _lib_key(name)
        out[f"{layer}.mu_{kind}"] = b.mu.detach()[at:at + n].clone().view(shape)
        out[f"{layer}.rho_{kind}"] = b.rho.detach()[at:at + n].clone().view(shape)
        at += n
    return out


def load_layerwise_state_dict(net, sd):
    """Inverse of `to_layerwise_state_dict` (every key required, shapes checked)."""
    b, at = net.bayes, 0
    with torch.no_grad():
        for (name, shape), n in zip(b.segments, b.sizes):
            layer, kind = _lib_key(name)
            for flat, key in ((b.mu, f"{layer}.mu_{kind}"), (b.rho, f"{layer}.rho_{kind}")):
                if key not in sd:
                    raise KeyError(f"load_layerwise_state_dict: missing {key}")
                if tuple(sd[key].shape) != shape:
                    raise RuntimeError(f"load_layerwise_state_dict: {key} has shape "
                                       f"{tuple(sd[key].shape)}, expected {shape}")
                flat[at:at + n].copy_(sd[key].reshape(-1))
            at += n
    return net

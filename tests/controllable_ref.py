"""Test helper: the reference's conditional PC samplers (controllable_generation.py:8-181)
restated in float32 torch-CPU with the reference's operation order and INJECTED noise.

`project_inpaint` / `project_colorize` are the data-consistency projections (:48-51, :140-143),
`init_inpaint` / `init_colorize` the initial states (:73, :170-172), `pc_conditional` the whole
loop on top of oracle.score_sde_ref's predictor / corrector restatements.  Serves the kernel
tests on every SDE kind (the fixtures are VP only) and replays tests/golden/ctrl_*.npz.
"""
from __future__ import annotations

import json

import torch

from oracle import score_sde_ref

FIXTURES = ["inpaint_em_langevin", "inpaint_anc_none", "colorize_rd_ald"]  # golden/ctrl_<name>.npz


def fixture_net(d):
    """(config, {name: tensor}) of a fixture's score network: a stored net_<name>.npz, or the
    weights the fixture carries."""
    from conftest import net_fixture, to_attr
    if "net" in d.files:
        cfg, sd, *_ = net_fixture(str(d["net"]))
    else:
        cfg = to_attr(json.loads(str(d["config_json"])))
        sd = {k[2:]: d[k] for k in d.files if k.startswith("p:")}
    return cfg, {k: torch.tensor(v) for k, v in sd.items()}


DATA_DRAW = 0x100  # the engine's draw id of a projection's data noise: DATA_DRAW + update draw id

# controllable_generation.py:107-111
M = torch.tensor([[5.7735014e-01, -8.1649649e-01, 4.7008697e-08],
                  [5.7735026e-01, 4.0824834e-01, 7.0710671e-01],
                  [5.7735026e-01, 4.0824822e-01, -7.0710683e-01]])
INV_M = torch.inverse(M)


def decouple(x):
    return torch.einsum('bihw,ij->bjhw', x, M)


def couple(x):
    return torch.einsum('bihw,ij->bjhw', x, INV_M)


def color_mask(x):
    return torch.cat([torch.ones_like(x[:, :1]), torch.zeros_like(x[:, 1:])], dim=1)


def marginal(spec, t):
    """(mean coefficient or None, std) of marginal_prob (sde_lib.py:174-178, :226-230,
    :284-287); None: the VE mean is x itself, no multiplication."""
    if spec.kind == "ve":
        return None, spec.marginal_std(t)
    return spec.marginal_mean_coef(t), spec.marginal_std(t)


def _bc(v, x):
    return v.reshape((-1,) + (1,) * (x.dim() - 1))


def _mean(mc, data):
    return data if mc is None else _bc(mc, data) * data


def project_inpaint(x, data, mask, mc, sd, z2):
    md_mean = _mean(mc, data)
    md = md_mean + z2 * _bc(sd, x)
    x = x * (1. - mask) + md * mask
    return x, x * (1. - mask) + md_mean * mask


def project_colorize(x, gray, mc, sd, z2):
    """z2: a full-shape draw, or its channel 0 [B, 1, H, W] (the others meet a zero mask)."""
    mask = color_mask(x)
    if z2.shape[1] == 1:
        z2 = torch.cat([z2, torch.zeros_like(x[:, 1:])], dim=1)
    md_mean = _mean(mc, decouple(gray))
    md = md_mean + z2 * _bc(sd, x)
    x = couple(decouple(x) * (1. - mask) + md * mask)
    return x, couple(decouple(x) * (1. - mask) + md_mean * mask)


def init_inpaint(data, mask, prior):
    return data * mask + prior * (1. - mask)


def init_colorize(gray, prior):
    mask = color_mask(gray)
    return couple(decouple(gray) * mask + decouple(prior * (1. - mask)))


def pc_conditional(model_fn, spec, condition, prior, data, mask, predictor, corrector, snr,
                   n_steps, continuous, draws, draws2, denoise=True, eps=1e-3):
    """pc_inpainter / pc_colorizer (:59-80, :156-179).  `draws`: the update draws in order,
    `draws2`: the projections' data draws in order (two per iteration)."""
    score = score_sde_ref.make_score(model_fn, spec, continuous)
    it, it2 = iter(draws), iter(draws2)

    def project(x, t):
        mc, sd = marginal(spec, t)
        if condition == "inpaint":
            return project_inpaint(x, data, mask, mc, sd, next(it2))
        return project_colorize(x, data, mc, sd, next(it2))

    x = init_inpaint(data, mask, prior) if condition == "inpaint" else init_colorize(data, prior)
    ts = torch.linspace(spec.T, eps, spec.N)
    with torch.no_grad():
        for i in range(spec.N):
            t = torch.ones(x.shape[0]) * ts[i]
            x, x_mean = score_sde_ref._corrector(corrector, spec, score, x, t, snr, n_steps,
                                                 lambda: next(it))
            x, x_mean = project(x, t)
            x, x_mean = score_sde_ref._predictor(predictor, spec, score, x, t, lambda: next(it))
            x, x_mean = project(x, t)
    return x_mean if denoise else x


def engine_noise_table(draws, draws2, N, predictor, corrector, n_steps):
    """{(step, draw id): tensor} for PCEngine's noise_fn from the two ordered lists: update draws
    under 1 + j (corrector) and 0 (predictor), data draws under DATA_DRAW + the id of the update
    they follow (a None corrector counts as draw 1)."""
    n_corr = n_steps if corrector != "none" else 0
    order = [1 + j for j in range(n_corr)] + ([0] if predictor != "none" else [])
    table = {}
    for i in range(N):
        for k, d in enumerate(order):
            table[(i, d)] = draws[i * len(order) + k]
        table[(i, DATA_DRAW + (n_corr if n_corr else 1))] = draws2[2 * i]
        table[(i, DATA_DRAW)] = draws2[2 * i + 1]
    return table

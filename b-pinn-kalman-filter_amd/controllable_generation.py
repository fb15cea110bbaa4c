"""Conditional PC sampling on MI355X: inpainting and colorization (reference:
controllable_generation.py:8-181).

Public surface kept from the reference: `get_pc_inpainter(...)` -> `pc_inpainter(model, data,
mask)` and `get_pc_colorizer(...)` -> `pc_colorizer(model, gray_scale_img)`, with the
reference's arguments, defaults, `M` matrix and return value (`inverse_scaler(x_mean if denoise
else x)`).

Execution: the built-in predictor / corrector pairs run on `sampling.PCEngine(condition=...)`,
whose update kernels apply the data-consistency projection in their store (csrc/sampler.hip),
one captured graph per PC step.  The shape is only known at call time, so the engine is built
at the first call and cached per (shape, device); later calls with new data / mask of the same
shape reuse its graph.  Pairs the engine has no fused step for (user-registered classes,
`probability_flow=True`) run the reference's loop with torch ops on the device.  Inputs must be
HIP tensors: there is no CPU path.
"""
from __future__ import annotations

import functools

import torch

import sampling
from op import sde_kernels as K
from op._lib import require_hip
from sampling import (NoneCorrector, NonePredictor, PCEngine, shared_corrector_update_fn,
                      shared_predictor_update_fn)


def _canon(cls, none_cls):
    return none_cls if cls is None else cls


def _marginal(sde, t, B, device):
    """(mean coefficient [B,1,1,1], std [B]) of sde.marginal_prob at the scalar time t, from
    the host float32 expressions the engine's table is built with."""
    row = sampling.marginal_rows(sde, torch.ones(1) * t)[0]
    return (row[0].to(device).expand(B)[:, None, None, None], row[1].to(device).expand(B))


def _get_runner(condition, sde, predictor, corrector, snr, n_steps, probability_flow, continuous,
                denoise, eps, engine_kwargs):
    """fn(model, data, mask) -> (x, x_mean) after the N conditioned steps."""
    pred_cls, corr_cls = _canon(predictor, NonePredictor), _canon(corrector, NoneCorrector)
    fused = PCEngine.supports(sde, pred_cls, corr_cls, probability_flow)
    engines = {}

    def run_engine(model, data, mask):
        key = (tuple(data.shape), data.device)
        if key not in engines:
            engines[key] = PCEngine(sde, data.shape, pred_cls, corr_cls, snr, n_steps, continuous,
                                    denoise, eps, data.device, condition=condition,
                                    **engine_kwargs)
        return engines[key].run(model, data=data.contiguous(),
                                mask=None if mask is None else mask.contiguous())

    pred_fn = functools.partial(shared_predictor_update_fn, sde=sde, predictor=predictor,
                                probability_flow=probability_flow, continuous=continuous)
    corr_fn = functools.partial(shared_corrector_update_fn, sde=sde, corrector=corrector,
                                continuous=continuous, snr=snr, n_steps=n_steps)
    M, invM = K.color_mats()

    def project(x, data, mask, t):
        # reference :48-51 (inpaint) and :140-143 (colorize: data is the decoupled gray image)
        mc, std = _marginal(sde, t, x.shape[0], x.device)
        md_mean = mc * data
        md = md_mean + torch.randn_like(x) * std[:, None, None, None]
        if condition == "inpaint":
            x = x * (1. - mask) + md * mask
            return x, x * (1. - mask) + md_mean * mask
        x = sampling.decouple(sampling.decouple(x, M) * (1. - mask) + md * mask, invM)
        return x, sampling.decouple(sampling.decouple(x, M) * (1. - mask) + md_mean * mask, invM)

    def run_loop(model, data, mask):
        dev, shape = data.device, data.shape
        prior = sde.prior_sampling(shape).to(dev)
        if condition == "inpaint":
            x = data * mask + prior * (1. - mask)
            known = data
        else:
            mask = torch.cat([torch.ones_like(data[:, :1]), torch.zeros_like(data[:, 1:])], dim=1)
            known = sampling.decouple(data, M)
            x = sampling.decouple(known * mask + sampling.decouple(prior * (1. - mask), M), invM)
        timesteps = sampling.pc_timesteps(sde, eps)
        x_mean = x
        for i in range(sde.N):
            t = timesteps[i]
            vec_t = torch.ones(shape[0], device=dev) * t
            x, x_mean = corr_fn(x, vec_t, model=model)
            x, x_mean = project(x, known, mask, t)
            x, x_mean = pred_fn(x, vec_t, model=model)
            x, x_mean = project(x, known, mask, t)
        return x, x_mean

    runner = run_engine if fused else run_loop
    runner.engines = engines
    runner.fused = fused
    return runner


def get_pc_inpainter(sde, predictor, corrector, inverse_scaler, snr, n_steps=1,
                     probability_flow=False, continuous=False, denoise=True, eps=1e-5,
                     **engine_kwargs):
    """Reference controllable_generation.py:8-82.  `engine_kwargs` (seed, use_graph, dist_ctx,
    noise_fn) go to PCEngine."""
    runner = _get_runner("inpaint", sde, predictor, corrector, snr, n_steps, probability_flow,
                         continuous, denoise, eps, engine_kwargs)

    def pc_inpainter(model, data, mask):
        """data: [B, C, H, W] images; mask: same shape, 1 = known pixel, 0 = to inpaint."""
        require_hip(data, mask, what="pc_inpainter")
        with torch.no_grad():
            x, x_mean = runner(model, data.to(torch.float32), mask.to(torch.float32))
            return inverse_scaler(x_mean if denoise else x)

    pc_inpainter.engines, pc_inpainter.fused = runner.engines, runner.fused
    return pc_inpainter


def get_pc_colorizer(sde, predictor, corrector, inverse_scaler, snr, n_steps=1,
                     probability_flow=False, continuous=False, denoise=True, eps=1e-5,
                     **engine_kwargs):
    """Reference controllable_generation.py:85-181."""
    runner = _get_runner("colorize", sde, predictor, corrector, snr, n_steps, probability_flow,
                         continuous, denoise, eps, engine_kwargs)

    def pc_colorizer(model, gray_scale_img):
        """gray_scale_img: [B, 3, H, W], the three channels holding the same values."""
        require_hip(gray_scale_img, what="pc_colorizer")
        if gray_scale_img.dim() != 4 or gray_scale_img.shape[1] != 3:
            raise ValueError(f"pc_colorizer needs [B, 3, H, W], got {tuple(gray_scale_img.shape)}")
        with torch.no_grad():
            x, x_mean = runner(model, gray_scale_img.to(torch.float32), None)
            return inverse_scaler(x_mean if denoise else x)

    pc_colorizer.engines, pc_colorizer.fused = runner.engines, runner.fused
    return pc_colorizer

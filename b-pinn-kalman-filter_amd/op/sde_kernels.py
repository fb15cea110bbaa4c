"""Thin wrappers over the PC-sampler kernels of csrc/sampler.hip (see include/bpk.h).

All tensors are float32 on the HIP device.  `coef` is a [n_rows, coef_bdim, 8]
table (or [coef_bdim, 8] for a single step), `step` a 1-element int32 device
tensor holding the row index (so captured graphs can advance it on device).

Conditional sampling (reference controllable_generation.py): `cond=` COND_INPAINT /
COND_COLORIZE on `predictor` / `langevin_update` applies the data-consistency projection in
the update's store, `project` is the projection alone.  `mtab` is the [n_rows, bdim, 2]
(mean coefficient, std) table of sde.marginal_prob read at the same `step`, `mats` the
colorizer's (M, inverse(M)) pair from `color_mats()`, `noise2` an explicit data draw (else
the Philox stream under draw id DATA_DRAW + draw).
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import check, lib, require_hip, stream_ptr

COEF_STRIDE = 8
C_SDIV, C_DRIFT, C_DIFF, C_DT, C_SQRT_MDT, C_ALPHA, C_AUX = range(7)

PRED_EM, PRED_RD, PRED_ANC_VP, PRED_ANC_VE = 0, 1, 2, 3
SCORE_DIV, SCORE_RAW = 0, 1
COND_NONE, COND_INPAINT, COND_COLORIZE = 0, 1, 2
DATA_DRAW = 0x100  # draw id of the projection's data noise: DATA_DRAW + the update's draw id


def _p(t):
    return None if t is None else t.data_ptr()


def _bd(coef, B):
    bdim = coef.shape[-2]
    if bdim not in (1, B):
        raise RuntimeError(f"coef table batch dim {bdim} must be 1 or {B}")
    return bdim


def color_mats():
    """(M, invM) of the colorizer, float32 on the host: the reference's orthonormal matrix that
    puts the gray-scale image into channel 0 and its torch.inverse (controllable_generation.py
    :105-111)."""
    M = torch.tensor([[5.7735014e-01, -8.1649649e-01, 4.7008697e-08],
                      [5.7735026e-01, 4.0824834e-01, 7.0710671e-01],
                      [5.7735026e-01, 4.0824822e-01, -7.0710683e-01]])
    return M, torch.inverse(M)


def _cond_args(cond, x, data, mask, mtab, mats, noise2, what):
    """(noise2, data, mask, mtab, mtab_bdim, mats, C) arguments of the C ABI; the host array
    behind `mats` is returned too so it outlives the call."""
    if cond == COND_NONE:
        return (None, None, None, None, 1, None, 1), None
    require_hip(x, data, mask, mtab, noise2, what=what)
    B = x.shape[0]
    for name, t in (("data", data), ("mask", mask), ("noise2", noise2)):
        if t is not None and (t.shape != x.shape or t.dtype != torch.float32
                              or not t.is_contiguous()):
            raise RuntimeError(f"{what}: {name} must be contiguous float32 of shape "
                               f"{tuple(x.shape)}, got {t.dtype} {tuple(t.shape)}")
    if mtab is None or mtab.shape[-1] != 2 or mtab.shape[-2] not in (1, B):
        raise RuntimeError(f"{what}: mtab must be [n_rows, 1 or {B}, 2]")
    C, host = 1, None
    if cond == COND_COLORIZE:
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"{what}: colorization needs [B, 3, H, W], got {tuple(x.shape)}")
        C = 3
        M, invM = mats if mats is not None else color_mats()
        vals = [float(v) for v in torch.cat([M.reshape(-1), invM.reshape(-1)]).tolist()]
        host = (ctypes.c_float * 18)(*vals)
    return (_p(noise2), _p(data), _p(mask), mtab.data_ptr(), mtab.shape[-2],
            None if host is None else ctypes.addressof(host), C), host


def project(cond, x, mtab, step, *, x_out, x_mean=None, data, mask=None, mats=None, noise2=None,
            seed=0, draw=0, sample_offset=0):
    """The projection alone: x_out, x_mean = project((x, x)) (a None predictor / corrector)."""
    require_hip(x, x_out, x_mean, step, what="pc_project")
    (n2, dp, mp, tp, tb, hp, C), host = _cond_args(cond, x, data, mask, mtab, mats, noise2,
                                                  "pc_project")
    B = x.shape[0]
    D = x.numel() // max(B, 1)
    check(lib.bpk_pc_project_f32(cond, x.data_ptr(), n2, x_out.data_ptr(), _p(x_mean), dp, mp, tp,
                                 tb, hp, B, C, D, sample_offset, step.data_ptr(),
                                 seed & (2 ** 64 - 1), draw, stream_ptr(x.device)), "pc_project")
    del host


def philox_normal(shape, seed, step, draw, sample_offset=0, device=None):
    out = torch.empty(shape, device=device, dtype=torch.float32)
    B = shape[0]
    D = out.numel() // max(B, 1)
    check(lib.bpk_philox_normal_f32(out.data_ptr(), B, D, sample_offset, seed & (2 ** 64 - 1),
                                    _p(step), draw, stream_ptr(out.device)), "philox_normal")
    return out


def predictor(kind, x, model_out, coef, step, *, x_out, x_mean=None, noise=None, score_mode=0,
              drift_mul_x=1, seed=0, draw=0, sample_offset=0, cond=COND_NONE, data=None,
              mask=None, mtab=None, mats=None, noise2=None):
    require_hip(x, model_out, coef, step, what="pc_predictor")
    B = x.shape[0]
    D = x.numel() // max(B, 1)
    if cond != COND_NONE:
        (n2, dp, mp, tp, tb, hp, C), host = _cond_args(cond, x, data, mask, mtab, mats, noise2,
                                                      "pc_predictor")
        check(lib.bpk_pc_predictor_cond_f32(cond, kind, x.data_ptr(), model_out.data_ptr(),
                                            _p(noise), n2, x_out.data_ptr(), _p(x_mean), dp, mp,
                                            tp, tb, hp, B, C, D, sample_offset, coef.data_ptr(),
                                            _bd(coef, B), step.data_ptr(), score_mode,
                                            drift_mul_x, seed & (2 ** 64 - 1), draw,
                                            stream_ptr(x.device)), "pc_predictor")
        del host
        return
    check(lib.bpk_pc_predictor_f32(kind, x.data_ptr(), model_out.data_ptr(), _p(noise),
                                   x_out.data_ptr(), _p(x_mean), B, D, sample_offset,
                                   coef.data_ptr(), _bd(coef, B), step.data_ptr(), score_mode,
                                   drift_mul_x, seed & (2 ** 64 - 1), draw,
                                   stream_ptr(x.device)), "pc_predictor")


def langevin_workspace(B, D, device):
    nb = lib.bpk_langevin_workspace_bytes(B, D)
    return torch.empty(max(nb // 4, 1), device=device, dtype=torch.float32)


def langevin_norms(model_out, coef, step, workspace, red, *, noise=None, score_mode=0, seed=0,
                   draw=0, sample_offset=0):
    """red[0] = sum_b ||score_b||, red[1] = sum_b ||noise_b|| over the local batch."""
    B = model_out.shape[0]
    D = model_out.numel() // max(B, 1)
    st = stream_ptr(model_out.device)
    check(lib.bpk_langevin_partial_f32(model_out.data_ptr(), _p(noise), workspace.data_ptr(), B, D,
                                       sample_offset, coef.data_ptr(), _bd(coef, B),
                                       step.data_ptr(), score_mode, seed & (2 ** 64 - 1), draw,
                                       st), "langevin_partial")
    check(lib.bpk_langevin_reduce_f32(workspace.data_ptr(), red.data_ptr(), B, D, st),
          "langevin_reduce")


def langevin_update(mode, x, model_out, coef, step, red, *, x_out, x_mean=None, noise=None,
                    B_global=None, score_mode=0, snr=0.16, seed=0, draw=0, sample_offset=0,
                    cond=COND_NONE, data=None, mask=None, mtab=None, mats=None, noise2=None):
    B = x.shape[0]
    D = x.numel() // max(B, 1)
    if cond != COND_NONE:
        require_hip(x, model_out, coef, step, what="langevin_update")
        (n2, dp, mp, tp, tb, hp, C), host = _cond_args(cond, x, data, mask, mtab, mats, noise2,
                                                      "langevin_update")
        check(lib.bpk_langevin_update_cond_f32(cond, mode, x.data_ptr(), model_out.data_ptr(),
                                               _p(noise), n2, _p(red), x_out.data_ptr(),
                                               _p(x_mean), dp, mp, tp, tb, hp, B, C, D,
                                               B_global or B, sample_offset, coef.data_ptr(),
                                               _bd(coef, B), step.data_ptr(), score_mode,
                                               float(snr), seed & (2 ** 64 - 1), draw,
                                               stream_ptr(x.device)), "langevin_update")
        del host
        return
    check(lib.bpk_langevin_update_f32(mode, x.data_ptr(), model_out.data_ptr(), _p(noise),
                                      _p(red), x_out.data_ptr(), _p(x_mean), B, D,
                                      B_global or B, sample_offset, coef.data_ptr(),
                                      _bd(coef, B), step.data_ptr(), score_mode, float(snr),
                                      seed & (2 ** 64 - 1), draw, stream_ptr(x.device)),
          "langevin_update")


def step_increment(step):
    check(lib.bpk_step_increment(step.data_ptr(), stream_ptr(step.device)), "step_increment")


def fill_from_table(out, table, step):
    check(lib.bpk_fill_step_scalar_f32(out.data_ptr(), out.numel(), table.data_ptr(),
                                       step.data_ptr(), stream_ptr(out.device)),
          "fill_step_scalar")

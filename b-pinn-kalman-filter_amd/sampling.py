"""Predictor-Corrector sampling on MI355X (reference: sampling.py).

Plugin surface kept from the reference:
  * `register_predictor` / `register_corrector` registries, `get_predictor`,
    `get_corrector` (sampling.py:30-77);
  * `Predictor(sde, score_fn, probability_flow)` / `Corrector(sde, score_fn, snr,
    n_steps)` with `update_fn(x, t) -> (x, x_mean)` (sampling.py:126-173);
  * `get_sampling_fn(config, sde, shape, inverse_scaler, eps)` -> fn(model) ->
    (samples, nfe) (sampling.py:80-123), `get_pc_sampler`, `get_ode_sampler`.

Execution (the MI355X part):
  * the built-in predictors (euler_maruyama, reverse_diffusion,
    ancestral_sampling) and correctors (langevin, ald) run as fused HIP update
    kernels (csrc/sampler.hip) that read the raw model output and fold
    "score = -model/std" into the update;
  * per-step scalars are precomputed once on the host with the reference's float32
    expressions (bit-identical to the reference CPU path) into a device table, and
    the step index lives in device memory;
  * one whole PC step (time-label fill, corrector score eval + Langevin update,
    predictor score eval + update, step increment) is captured in a hipGraph and
    replayed N times -- no per-step Python, object rebuilding or launch gaps (the
    reference rebuilds score_fn and predictor objects every step,
    sampling.py:333-352);
  * batch-sharded multi-GPU: each rank owns samples [r*B, (r+1)*B); the only
    exchange is a 2-float all-reduce per Langevin step (the batch-mean norms of
    sampling.py:276-277); noise is Philox keyed by the global sample index, so
    results do not depend on the number of ranks;
  * conditional sampling (`PCEngine(condition="inpaint" | "colorize")`, public API in
    controllable_generation.py): the reference's data-consistency projection after every
    corrector and predictor half-step sits in the update kernels' store, so the conditioned
    step is the same launch sequence and the same single graph.
User-registered predictors/correctors fall back to the reference-style loop.
"""
from __future__ import annotations

import abc
import functools
import os

import numpy as np
import torch

import sde_lib
from models import utils as mutils
from models.utils import from_flattened_numpy, get_score_fn, to_flattened_numpy
from op import sde_kernels as K

_CORRECTORS: dict = {}
_PREDICTORS: dict = {}


def _make_register(table):
    def register(cls=None, *, name=None):
        def _reg(c):
            key = c.__name__ if name is None else name
            if key in table:
                raise ValueError(f"Already registered model with name: {key}")
            table[key] = c
            return c

        return _reg if cls is None else _reg(cls)

    return register


register_predictor = _make_register(_PREDICTORS)
register_corrector = _make_register(_CORRECTORS)


def get_predictor(name):
    return _PREDICTORS[name]


def get_corrector(name):
    return _CORRECTORS[name]


def get_sampling_fn(config, sde, shape, inverse_scaler, eps, **engine_kwargs):
    name = config.sampling.method.lower()
    if name == "ode":
        return get_ode_sampler(sde=sde, shape=shape, inverse_scaler=inverse_scaler,
                               denoise=config.sampling.noise_removal, eps=eps,
                               device=config.device)
    if name == "pc":
        return get_pc_sampler(sde=sde, shape=shape,
                              predictor=get_predictor(config.sampling.predictor.lower()),
                              corrector=get_corrector(config.sampling.corrector.lower()),
                              inverse_scaler=inverse_scaler, snr=config.sampling.snr,
                              n_steps=config.sampling.n_steps_each,
                              probability_flow=config.sampling.probability_flow,
                              continuous=config.training.continuous,
                              denoise=config.sampling.noise_removal, eps=eps,
                              device=config.device, **engine_kwargs)
    raise ValueError(f"Sampler name {name} unknown.")


# ---------------------------------------------------------------------------
# per-step coefficient rows (float32, reference expressions)
# ---------------------------------------------------------------------------

def _score_divisor(sde, continuous, t):
    if isinstance(sde, sde_lib.VESDE):
        return torch.ones_like(t)
    if continuous or isinstance(sde, sde_lib.subVPSDE):
        return sde.marginal_coef(t)[1]
    return sde.sqrt_1m_alphas_cumprod.to(t.device)[(t * (sde.N - 1)).long()]


def coef_rows(sde, t, continuous, predictor_kind=None, probability_flow=False):
    """[len(t), 8] float32 coefficient rows for the fused kernels (see include/bpk.h)."""
    t = t.to(torch.float32)
    rows = torch.zeros((t.shape[0], K.COEF_STRIDE), dtype=torch.float32, device=t.device)
    rows[:, K.C_SDIV] = _score_divisor(sde, continuous, t)
    if predictor_kind == K.PRED_EM:
        dc, diff = sde.coefficient(t)
        dt = -1. / sde.N
        rows[:, K.C_DRIFT] = dc
        rows[:, K.C_DIFF] = diff
        rows[:, K.C_DT] = torch.tensor(dt, dtype=torch.float32)
        rows[:, K.C_SQRT_MDT] = torch.tensor(np.sqrt(-dt), dtype=torch.float32)
    elif predictor_kind == K.PRED_RD:
        ts = sde.timestep_index(t)
        if isinstance(sde, sde_lib.VPSDE):
            rows[:, K.C_DRIFT] = torch.sqrt(sde.alphas.to(t.device)[ts])
            rows[:, K.C_DIFF] = torch.sqrt(sde.discrete_betas.to(t.device)[ts])
        else:
            rows[:, K.C_DIFF] = sde.discretize(torch.zeros_like(t), t)[1]
    elif predictor_kind == K.PRED_ANC_VP:
        beta = sde.discrete_betas.to(t.device)[sde.timestep_index(t)]
        rows[:, K.C_DRIFT] = beta
        rows[:, K.C_DIFF] = torch.sqrt(1. - beta)
        rows[:, K.C_SQRT_MDT] = torch.sqrt(beta)
    elif predictor_kind == K.PRED_ANC_VE:
        ts = sde.timestep_index(t)
        sig = sde.discrete_sigmas.to(t.device)[ts]
        adj = torch.where(ts == 0, torch.zeros_like(t), sde.discrete_sigmas.to(t.device)[ts - 1])
        rows[:, K.C_DRIFT] = sig ** 2 - adj ** 2
        rows[:, K.C_DIFF] = torch.sqrt((adj ** 2 * (sig ** 2 - adj ** 2)) / (sig ** 2))
    # corrector fields
    if isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE)):
        if hasattr(sde, "alphas"):
            rows[:, K.C_ALPHA] = sde.alphas.to(t.device)[sde.timestep_index(t)]
        else:
            # subVPSDE has no alphas: never read, the correctors refuse sub-VP
            # (PCEngine.supports, _FusedCorrector.update_fn)
            rows[:, K.C_ALPHA] = float("nan")
    else:
        rows[:, K.C_ALPHA] = 1.0
    rows[:, K.C_AUX] = sde.marginal_coef(t)[1]
    return rows


def _fusable_sde(sde):
    return isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE, sde_lib.VESDE))


def _score_parts(score_fn, x, t):
    """(model_out, score_mode, coef_rows-capable?) for a score function."""
    if isinstance(score_fn, mutils.ScoreFn):
        return score_fn.model_fn(x, score_fn.labels(t)), (K.SCORE_DIV if score_fn.divides
                                                           else K.SCORE_RAW)
    return score_fn(x, t), K.SCORE_RAW


def _zero_step(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


# ---------------------------------------------------------------------------
# Predictors / correctors
# ---------------------------------------------------------------------------

class Predictor(abc.ABC):
    """Abstract predictor (reference sampling.py:126-149)."""

    def __init__(self, sde, score_fn, probability_flow=False):
        super().__init__()
        self.sde = sde
        self.rsde = sde.reverse(score_fn, probability_flow)
        self.score_fn = score_fn
        self.probability_flow = probability_flow

    @abc.abstractmethod
    def update_fn(self, x, t):
        """One predictor update -> (x, x_mean)."""


class Corrector(abc.ABC):
    """Abstract corrector (reference sampling.py:152-173)."""

    def __init__(self, sde, score_fn, snr, n_steps):
        super().__init__()
        self.sde = sde
        self.score_fn = score_fn
        self.snr = snr
        self.n_steps = n_steps

    @abc.abstractmethod
    def update_fn(self, x, t):
        """One corrector update -> (x, x_mean)."""


class _FusedPredictor(Predictor):
    _kind = None  # set by subclasses

    def fused_kind(self):
        return self._kind

    def _fusable(self, x):
        return (x.is_cuda and x.dtype == torch.float32 and _fusable_sde(self.sde)
                and not self.probability_flow and self.fused_kind() is not None)

    def update_fn(self, x, t, noise=None):
        if not self._fusable(x):
            return self.torch_update_fn(x, t)
        continuous = getattr(self.score_fn, "continuous", True)
        m, mode = _score_parts(self.score_fn, x, t)
        rows = coef_rows(self.sde, t, continuous, self.fused_kind())
        xo, xm = torch.empty_like(x), torch.empty_like(x)
        if noise is None:
            noise = torch.randn_like(x)
        K.predictor(self.fused_kind(), x.contiguous(), m.contiguous(), rows[None], _zero_step(x.device),
                    x_out=xo, x_mean=xm, noise=noise.contiguous(), score_mode=mode,
                    drift_mul_x=int(not isinstance(self.sde, sde_lib.VESDE)))
        return xo, xm

    @abc.abstractmethod
    def torch_update_fn(self, x, t):
        """Reference-style torch implementation (fallback for non-fusable cases)."""


@register_predictor(name="euler_maruyama")
class EulerMaruyamaPredictor(_FusedPredictor):
    """Reference sampling.py:176-187 (z drawn before the score evaluation)."""
    _kind = K.PRED_EM

    def torch_update_fn(self, x, t):
        dt = -1. / self.rsde.N
        z = torch.randn_like(x)
        drift, diffusion = self.rsde.sde(x, t)
        x_mean = x + drift * dt
        if torch.is_tensor(diffusion):
            x = x_mean + diffusion[:, None, None, None] * np.sqrt(-dt) * z
        else:
            x = x_mean + diffusion * np.sqrt(-dt) * z
        return x, x_mean


@register_predictor(name="reverse_diffusion")
class ReverseDiffusionPredictor(_FusedPredictor):
    """Reference sampling.py:190-200."""

    def fused_kind(self):
        return K.PRED_RD if isinstance(self.sde, (sde_lib.VPSDE, sde_lib.VESDE)) else None

    def torch_update_fn(self, x, t):
        f, G = self.rsde.discretize(x, t)
        z = torch.randn_like(x)
        x_mean = x - f
        return x_mean + G[:, None, None, None] * z, x_mean


@register_predictor(name="ancestral_sampling")
class AncestralSamplingPredictor(_FusedPredictor):
    """Reference sampling.py:203-239 (VP / VE only)."""

    def __init__(self, sde, score_fn, probability_flow=False):
        super().__init__(sde, score_fn, probability_flow)
        if not isinstance(sde, (sde_lib.VPSDE, sde_lib.VESDE)):
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
        assert not probability_flow, "Probability flow not supported by ancestral sampling"

    def fused_kind(self):
        return K.PRED_ANC_VE if isinstance(self.sde, sde_lib.VESDE) else K.PRED_ANC_VP

    def torch_update_fn(self, x, t):
        sde = self.sde
        ts = sde.timestep_index(t)
        score = self.score_fn(x, t)
        if isinstance(sde, sde_lib.VESDE):
            sigma = sde.discrete_sigmas.to(t.device)[ts]
            adj = torch.where(ts == 0, torch.zeros_like(t), sde.discrete_sigmas.to(t.device)[ts - 1])
            x_mean = x + score * (sigma ** 2 - adj ** 2)[:, None, None, None]
            std = torch.sqrt((adj ** 2 * (sigma ** 2 - adj ** 2)) / (sigma ** 2))
            return x_mean + std[:, None, None, None] * torch.randn_like(x), x_mean
        beta = sde.discrete_betas.to(t.device)[ts]
        x_mean = (x + beta[:, None, None, None] * score) / torch.sqrt(1. - beta)[:, None, None, None]
        return x_mean + torch.sqrt(beta)[:, None, None, None] * torch.randn_like(x), x_mean


@register_predictor(name="none")
class NonePredictor(Predictor):
    def __init__(self, sde, score_fn, probability_flow=False):
        pass

    def update_fn(self, x, t):
        return x, x


class _FusedCorrector(Corrector):
    _mode = None

    def __init__(self, sde, score_fn, snr, n_steps):
        super().__init__(sde, score_fn, snr, n_steps)
        if not isinstance(sde, (sde_lib.VPSDE, sde_lib.VESDE, sde_lib.subVPSDE)):
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")

    def update_fn(self, x, t, noise_fn=None):
        if not (x.is_cuda and x.dtype == torch.float32):
            return self.torch_update_fn(x, t)
        if not isinstance(self.sde, sde_lib.VESDE):
            # sub-VP has no alphas table: AttributeError, as torch_update_fn and the reference
            getattr(self.sde, "alphas")
        continuous = getattr(self.score_fn, "continuous", True)
        rows = coef_rows(self.sde, t, continuous)[None]
        step = _zero_step(x.device)
        B = x.shape[0]
        D = x.numel() // B
        ws = K.langevin_workspace(B, D, x.device)
        red = torch.zeros(2, device=x.device, dtype=torch.float32)
        x = x.contiguous()
        x_mean = x
        for i in range(self.n_steps):
            m, mode = _score_parts(self.score_fn, x, t)
            m = m.contiguous()
            noise = noise_fn(i) if noise_fn is not None else torch.randn_like(x)
            if self._mode == 0:
                K.langevin_norms(m, rows, step, ws, red, noise=noise, score_mode=mode)
            xo, xm = torch.empty_like(x), torch.empty_like(x)
            K.langevin_update(self._mode, x, m, rows, step, red, x_out=xo, x_mean=xm, noise=noise,
                              score_mode=mode, snr=self.snr)
            x, x_mean = xo, xm
        return x, x_mean


@register_corrector(name="langevin")
class LangevinCorrector(_FusedCorrector):
    """Reference sampling.py:253-282 (noise drawn after the score; batch-mean norms)."""
    _mode = 0

    def torch_update_fn(self, x, t):
        sde = self.sde
        if isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE)):
            alpha = sde.alphas.to(t.device)[sde.timestep_index(t) if hasattr(sde, "timestep_index")
                                            else (t * (sde.N - 1) / sde.T).long()]
        else:
            alpha = torch.ones_like(t)
        x_mean = x
        for _ in range(self.n_steps):
            grad = self.score_fn(x, t)
            noise = torch.randn_like(x)
            gn = torch.norm(grad.reshape(grad.shape[0], -1), dim=-1).mean()
            nn_ = torch.norm(noise.reshape(noise.shape[0], -1), dim=-1).mean()
            step = (self.snr * nn_ / gn) ** 2 * 2 * alpha
            x_mean = x + step[:, None, None, None] * grad
            x = x_mean + torch.sqrt(step * 2)[:, None, None, None] * noise
        return x, x_mean


@register_corrector(name="ald")
class AnnealedLangevinDynamics(_FusedCorrector):
    """Reference sampling.py:285-319."""
    _mode = 1

    def torch_update_fn(self, x, t):
        sde = self.sde
        if isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE)):
            alpha = sde.alphas.to(t.device)[(t * (sde.N - 1) / sde.T).long()]
        else:
            alpha = torch.ones_like(t)
        std = sde.marginal_prob(x, t)[1]
        x_mean = x
        for _ in range(self.n_steps):
            grad = self.score_fn(x, t)
            noise = torch.randn_like(x)
            step = (self.snr * std) ** 2 * 2 * alpha
            x_mean = x + step[:, None, None, None] * grad
            x = x_mean + noise * torch.sqrt(step * 2)[:, None, None, None]
        return x, x_mean


@register_corrector(name="none")
class NoneCorrector(Corrector):
    def __init__(self, sde, score_fn, snr, n_steps):
        pass

    def update_fn(self, x, t):
        return x, x


def shared_predictor_update_fn(x, t, sde, model, predictor, probability_flow, continuous):
    score_fn = get_score_fn(sde, model, train=False, continuous=continuous)
    obj = NonePredictor(sde, score_fn, probability_flow) if predictor is None \
        else predictor(sde, score_fn, probability_flow)
    return obj.update_fn(x, t)


def shared_corrector_update_fn(x, t, sde, model, corrector, continuous, snr, n_steps):
    score_fn = get_score_fn(sde, model, train=False, continuous=continuous)
    obj = NoneCorrector(sde, score_fn, snr, n_steps) if corrector is None \
        else corrector(sde, score_fn, snr, n_steps)
    return obj.update_fn(x, t)


# ---------------------------------------------------------------------------
# PC sampler engine
# ---------------------------------------------------------------------------

def pc_timesteps(sde, eps):
    """The reference's time grid, float32 CPU algorithm (sampling.py:401)."""
    return torch.linspace(sde.T, eps, sde.N)


def marginal_rows(sde, t):
    """[len(t), 2] float32 (mean coefficient, std) of sde.marginal_prob at t: the scalars of
    the conditional samplers' projection (reference controllable_generation.py:48, :140).
    The mean coefficient is marginal_prob's mean of a unit input, so a user SDE with a linear
    mean needs nothing beyond the reference's interface."""
    t = t.to(torch.float32)
    mean, std = sde.marginal_prob(torch.ones((t.shape[0], 1, 1, 1), dtype=torch.float32,
                                             device=t.device), t)
    return torch.stack([mean.reshape(-1).to(torch.float32), std.to(torch.float32)], dim=1)


_CONDITIONS = {None: K.COND_NONE, "inpaint": K.COND_INPAINT, "colorize": K.COND_COLORIZE}


def decouple(x, M):
    """Reference controllable_generation.py:114-115 (couple: the same with inverse(M))."""
    return torch.einsum('bihw,ij->bjhw', x, M.to(x.device))


def _graph_collective(ctx) -> bool:
    """Capture the sharded PC step's RCCL all-reduce inside the step graph (opt-in,
    BPK_PC_GRAPH_ALLREDUCE=1): one graph replay per step instead of segments with a
    host-issued all-reduce between them.  Off by default: the split form is what the 8-GPU
    runs have exercised; tests/test_gpu_dist.py checks RCCL capture on one device."""
    import torch.distributed as tdist
    if os.environ.get("BPK_PC_GRAPH_ALLREDUCE", "0") != "1" or ctx is None:
        return False
    return tdist.is_initialized() and tdist.get_backend(ctx.group) == "nccl"


class PCEngine:
    """Fused, graph-captured PC sampler for the built-in predictor/corrector pairs.

    shape is the LOCAL (per-rank) batch shape.  `dist_ctx` (dist.DistContext) makes
    it batch-sharded: rank r owns global samples [r*B, (r+1)*B).
    """

    def __init__(self, sde, shape, predictor, corrector, snr, n_steps=1, continuous=False,
                 denoise=True, eps=1e-3, device="cuda", seed=None, use_graph=True, dist_ctx=None,
                 noise_fn=None, condition=None):
        if condition not in _CONDITIONS:
            raise ValueError(f"condition must be None, 'inpaint' or 'colorize', got {condition!r}")
        if condition == "colorize" and tuple(shape)[1] != 3:
            raise ValueError(f"colorization needs 3 channels, got shape {tuple(shape)}")
        if not self.supports(sde, predictor, corrector, False):
            raise NotImplementedError(
                f"PCEngine has no fused step for {sde.__class__.__name__} with "
                f"{getattr(predictor, '__name__', predictor)} / "
                f"{getattr(corrector, '__name__', corrector)}; get_pc_sampler runs such pairs "
                "on the reference loop")
        self.sde, self.shape = sde, tuple(shape)
        self.predictor, self.corrector = predictor, corrector
        self.snr, self.n_steps = float(snr), int(n_steps)
        self.continuous, self.denoise, self.eps = continuous, denoise, eps
        self.device = torch.device(device)
        from op import _hipenv
        # hipGraph replays only with the runtime setting of op/_hipenv.py proven in effect
        # (else, warned once, the eager step runs)
        self.use_graph = (use_graph and noise_fn is None
                          and _hipenv.graphs_allowed("PCEngine(use_graph=True)"))
        self.noise_fn = noise_fn
        self.dist = dist_ctx
        self.world = dist_ctx.world_size if dist_ctx is not None else 1
        self.rank = dist_ctx.rank if dist_ctx is not None else 0
        self.B = self.shape[0]
        self.D = int(np.prod(self.shape[1:]))
        self.B_global = self.B * self.world
        self.sample_offset = self.rank * self.B
        self.seed = seed
        self.graph = None
        self._filters = []  # Winograd filter transforms the step graph reads (conv.static_filters)
        self._graph_key = None
        self.pred_kind = self._pred_kind()
        self.corr_mode = {LangevinCorrector: 0, AnnealedLangevinDynamics: 1}.get(corrector, None)
        self.condition = condition
        self.cond = _CONDITIONS[condition]
        self._build_tables()

    # which built-in kernels apply
    def _pred_kind(self):
        p = self.predictor
        if p is EulerMaruyamaPredictor:
            return K.PRED_EM
        if p is ReverseDiffusionPredictor:
            return K.PRED_RD if isinstance(self.sde, (sde_lib.VPSDE, sde_lib.VESDE)) else None
        if p is AncestralSamplingPredictor:
            return K.PRED_ANC_VE if isinstance(self.sde, sde_lib.VESDE) else K.PRED_ANC_VP
        return None

    @staticmethod
    def supports(sde, predictor, corrector, probability_flow):
        if probability_flow or not _fusable_sde(sde):
            return False
        # sub-VP has no DDPM tables (discrete_betas / alphas): the reference's ancestral
        # predictor raises NotImplementedError on it and both Langevin correctors
        # AttributeError; those pairs go to the reference loop, which raises the same
        tables = isinstance(sde, (sde_lib.VPSDE, sde_lib.VESDE))
        ok_p = predictor in (EulerMaruyamaPredictor, NonePredictor) or (
            predictor in (ReverseDiffusionPredictor, AncestralSamplingPredictor) and tables)
        ok_c = corrector is NoneCorrector or (
            corrector in (LangevinCorrector, AnnealedLangevinDynamics) and tables)
        return ok_p and ok_c

    def _build_tables(self):
        sde = self.sde
        ts = pc_timesteps(sde, self.eps)
        self.timesteps = ts
        rows, labels = [], []
        dummy = mutils.ScoreFn(sde, torch.nn.Identity(), continuous=self.continuous)
        for i in range(sde.N):
            vec = torch.ones(1) * ts[i]
            rows.append(coef_rows(sde, vec, self.continuous, self.pred_kind))
            labels.append(dummy.labels(vec).to(torch.float32))
        self.coef = torch.stack(rows).to(self.device)  # [N, 1, 8]
        self.label_table = torch.cat(labels).to(self.device)  # [N]
        self.step = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.labels = torch.empty(self.B, dtype=torch.float32, device=self.device)
        self.red = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.ws = K.langevin_workspace(self.B, self.D, self.device)
        if self.cond != K.COND_NONE:
            # static buffers of the projection: the graph reads them, reset() rewrites them
            self.mtab = torch.stack([marginal_rows(sde, torch.ones(1) * ts[i])
                                     for i in range(sde.N)]).to(self.device)  # [N, 1, 2]
            self.cdata = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
            self.cmask = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
            self.mats = K.color_mats() if self.cond == K.COND_COLORIZE else None

    def _cond_kw(self, i, draw):
        """Keywords that put the projection into an update kernel's store (none when
        unconditioned); the data draw of the update with draw id `draw`."""
        if self.cond == K.COND_NONE:
            return {}
        return dict(cond=self.cond, data=self.cdata, mask=self.cmask, mtab=self.mtab,
                    mats=self.mats,
                    noise2=self._noise(i, K.DATA_DRAW + draw) if i is not None else None)

    def _project(self, x, x_mean, i, draw):
        """A None half-step of a conditioned run: (x, x) projected with fresh data noise."""
        kw = self._cond_kw(i, draw)
        K.project(kw.pop("cond"), x, kw.pop("mtab"), self.step, x_out=x, x_mean=x_mean,
                  seed=self.seed, draw=draw, sample_offset=self.sample_offset, **kw)

    def _noise(self, i, draw):
        if self.noise_fn is None:
            return None
        return self.noise_fn(i, draw).to(self.device, torch.float32).contiguous()

    def _segments(self, model, x, x_mean, i=None):
        """One PC iteration on the static buffers x / x_mean, as a generator that yields at
        every cross-rank exchange point (the Langevin norm all-reduce, only when sharded).
        The code between two yields is a graph-capturable launch sequence."""
        sde_vp_like = not isinstance(self.sde, sde_lib.VESDE)
        mode = K.SCORE_DIV if sde_vp_like else K.SCORE_RAW
        K.fill_from_table(self.labels, self.label_table, self.step)
        labels = self.labels if sde_vp_like or self.continuous else self.labels.long()
        if self.corr_mode is not None:
            for j in range(self.n_steps):
                m = model(x, labels).contiguous()
                nz = self._noise(i, 1 + j) if i is not None else None
                if self.corr_mode == 0:
                    K.langevin_norms(m, self.coef, self.step, self.ws, self.red, noise=nz,
                                     score_mode=mode, seed=self.seed, draw=1 + j,
                                     sample_offset=self.sample_offset)
                    if self.world > 1:
                        yield "all_reduce"  # red <- sum over ranks
                # the reference projects once per corrector call, after its last Langevin step
                ckw = self._cond_kw(i, 1 + j) if j == self.n_steps - 1 else {}
                K.langevin_update(self.corr_mode, x, m, self.coef, self.step, self.red, x_out=x,
                                  x_mean=x_mean, noise=nz, B_global=self.B_global, score_mode=mode,
                                  snr=self.snr, seed=self.seed, draw=1 + j,
                                  sample_offset=self.sample_offset, **ckw)
        elif self.cond != K.COND_NONE:
            self._project(x, x_mean, i, 1)
        if self.pred_kind is not None:
            m = model(x, labels).contiguous()
            nz = self._noise(i, 0) if i is not None else None
            K.predictor(self.pred_kind, x, m, self.coef, self.step, x_out=x, x_mean=x_mean,
                        noise=nz, score_mode=mode, drift_mul_x=int(sde_vp_like), seed=self.seed,
                        draw=0, sample_offset=self.sample_offset, **self._cond_kw(i, 0))
        elif self.cond != K.COND_NONE:
            self._project(x, x_mean, i, 0)
        elif self.corr_mode is not None:
            # NonePredictor returns (x, x): the step's x_mean is the corrector's noisy x, not
            # its x_mean (reference sampling.py:249-250, :405-406)
            x_mean.copy_(x)
        K.step_increment(self.step)

    def _pc_step(self, model, x, x_mean, i=None):
        for _ in self._segments(model, x, x_mean, i):
            self.dist.all_reduce_sum_(self.red)

    def init_state(self, x_init=None):
        if x_init is None:
            full = (self.B_global,) + self.shape[1:]
            x_full = self.sde.prior_sampling(full)
            x_init = x_full[self.sample_offset:self.sample_offset + self.B]
        if self.seed is None:
            self.seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        x = x_init.to(self.device, torch.float32).contiguous().clone()
        return x, x.clone()

    def _set_condition(self, x, data, mask):
        """Load data / mask into the static buffers and turn the prior x into the reference's
        initial state (controllable_generation.py:73, :168-172); once per run, torch ops."""
        if data is None:
            raise ValueError(f"PCEngine(condition={self.condition!r}).reset needs data=")
        for name, t in (("data", data), ("mask", mask)):
            if t is not None and not t.is_cuda:
                raise RuntimeError(f"PCEngine.reset: {name} must be a HIP (cuda) tensor, got "
                                   f"device {t.device}")
        self.cdata.copy_(data.to(torch.float32))
        if self.cond == K.COND_INPAINT:
            if mask is None:
                raise ValueError("PCEngine(condition='inpaint').reset needs mask=")
            self.cmask.copy_(mask.to(torch.float32))
            return self.cdata * self.cmask + x * (1. - self.cmask)
        self.cmask.zero_()
        self.cmask[:, :1] = 1.  # get_mask: channel 0 of the decoupled image is the known one
        M, invM = self.mats
        return decouple(decouple(self.cdata, M) * self.cmask + decouple(x * (1. - self.cmask), M),
                        invM).contiguous()

    @torch.no_grad()
    def reset(self, model, x_init=None, data=None, mask=None):
        """Draw / load the prior, (re)capture the step graph if needed, zero the step counter.
        A conditioned engine takes the known image (`data`, the gray image for colorize) and,
        for inpainting, the 0/1 `mask` of this rank's samples; x_init is then the prior the
        initial state is built from.  New data / mask of the same shape reuse the graph."""
        x, x_mean = self.init_state(x_init)
        if self.cond != K.COND_NONE:
            x = self._set_condition(x, data, mask)
            x_mean = x.clone()
        elif data is not None or mask is not None:
            raise ValueError("data= / mask= need PCEngine(condition=...)")
        self.step.zero_()
        if self.use_graph:
            key = (self.seed, id(model))
            if self.graph is None or self._graph_key != key:
                self._capture(model, x, x_mean)
                self._graph_key = key
        if self.use_graph:
            self._gx.copy_(x)
            self._gxm.copy_(x)
            self.step.zero_()
            self._x, self._xm = self._gx, self._gxm
        else:
            self._x, self._xm = x, x_mean
        self._model = model
        self._done = 0

    @torch.no_grad()
    def advance(self, n, progress=None):
        """Run n more PC steps on the current state (no host sync)."""
        if self._done + n > self.sde.N:
            raise ValueError(f"only {self.sde.N - self._done} steps left on the time grid")
        if self.use_graph and self._filters:
            # the step graph reads the cached Winograd filter transforms (conv.static_filters):
            # rewrite those whose weights changed since the capture (EMA copy_to, a load)
            from op import conv as conv_op
            conv_op.refresh_filters(self._filters)
        for k in range(n):
            if self.use_graph:
                for gi, g in enumerate(self.graph):
                    if gi:
                        self.dist.all_reduce_sum_(self.red)
                    g.replay()
            else:
                i = self._done if self.noise_fn is not None else None
                self._pc_step(self._model, self._x, self._xm, i=i)
            self._done += 1
            if progress is not None:
                progress(self._done)
        return self._x, self._xm

    @torch.no_grad()
    def run(self, model, x_init=None, n_iters=None, progress=None, data=None, mask=None):
        """Run n_iters (default N) PC steps from the prior; returns (x, x_mean)."""
        self.reset(model, x_init, data=data, mask=mask)
        x, xm = self.advance(self.sde.N if n_iters is None else n_iters, progress)
        return x.clone(), xm.clone()

    def _capture(self, model, x, x_mean):
        from op import conv as conv_op
        self._filters = []
        with conv_op.static_filters(self._filters):
            self._capture_graphs(model, x, x_mean)

    def _capture_graphs(self, model, x, x_mean):
        # static buffers owned by the graph
        self._gx = x.clone()
        self._gxm = x_mean.clone()
        # warm-up on a side stream (kernel selection, allocator)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(2):
                self._pc_step(model, self._gx, self._gxm)
        torch.cuda.current_stream(self.device).wait_stream(s)
        self.step.zero_()
        try:
            if self.world > 1 and _graph_collective(self.dist):
                # the whole PC step as ONE graph, the Langevin norm all-reduce (RCCL) captured
                # inside it (BPK_PC_GRAPH_ALLREDUCE=1; needs the nccl backend, whose
                # communicator the warm-up above has initialised)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in self._segments(model, self._gx, self._gxm):
                        self.dist.all_reduce_sum_(self.red)
                self.graph = [g]
                return
            # one graph per segment between exchange points (a single graph when unsharded);
            # the segments share one memory pool and the generator keeps the tensors that
            # cross a segment boundary (the model output) alive
            graphs, pool = [], None
            gen = self._segments(model, self._gx, self._gxm)
            done = False
            while not done:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool):
                    try:
                        next(gen)
                    except StopIteration:
                        done = True
                pool = g.pool()
                graphs.append(g)
            self._gen = gen
            self.graph = graphs
        except Exception as e:  # capture unsupported by some library call: run eagerly
            self.use_graph = False
            self.graph = None
            self.capture_error = repr(e)
            torch.cuda.synchronize(self.device)

    def __call__(self, model, inverse_scaler=lambda v: v, x_init=None, data=None, mask=None):
        x, x_mean = self.run(model, x_init, data=data, mask=mask)
        out = x_mean if self.denoise else x
        return inverse_scaler(out), self.sde.N * (self.n_steps + 1)


def get_pc_sampler(sde, shape, predictor, corrector, inverse_scaler, snr, n_steps=1,
                   probability_flow=False, continuous=False, denoise=True, eps=1e-3,
                   device="cuda", **engine_kwargs):
    """Reference sampling.py:355-411.  Built-in predictor/corrector pairs run on the
    fused / graph-captured engine; anything else runs the reference loop."""
    if PCEngine.supports(sde, predictor, corrector, probability_flow) and \
            torch.device(device).type == "cuda":
        engine = PCEngine(sde, shape, predictor, corrector, snr, n_steps, continuous, denoise,
                          eps, device, **engine_kwargs)

        def pc_sampler(model):
            return engine(model, inverse_scaler)

        pc_sampler.engine = engine
        return pc_sampler

    pred_fn = functools.partial(shared_predictor_update_fn, sde=sde, predictor=predictor,
                                probability_flow=probability_flow, continuous=continuous)
    corr_fn = functools.partial(shared_corrector_update_fn, sde=sde, corrector=corrector,
                                continuous=continuous, snr=snr, n_steps=n_steps)

    def pc_sampler(model):
        with torch.no_grad():
            x = sde.prior_sampling(shape).to(device)
            timesteps = pc_timesteps(sde, eps).to(device)
            x_mean = x
            for i in range(sde.N):
                vec_t = torch.ones(shape[0], device=device) * timesteps[i]
                x, x_mean = corr_fn(x, vec_t, model=model)
                x, x_mean = pred_fn(x, vec_t, model=model)
            return inverse_scaler(x_mean if denoise else x), sde.N * (n_steps + 1)

    return pc_sampler


def get_ode_sampler(sde, shape, inverse_scaler, denoise=False, rtol=1e-5, atol=1e-5,
                    method="RK45", eps=1e-3, device="cuda"):
    """Probability-flow ODE sampler (reference sampling.py:414-485).  The reference runs
    scipy's RK45 on a host copy of the batch; here the identical controller
    (inverse.ode.solve_ivp_rk, same accepted steps and nfev as scipy) runs on the device
    state, so no per-evaluation host round trip."""
    from inverse.ode import solve_ivp_rk

    def denoise_update_fn(model, x):
        score_fn = get_score_fn(sde, model, train=False, continuous=True)
        pred = ReverseDiffusionPredictor(sde, score_fn, probability_flow=False)
        vec_eps = torch.ones(x.shape[0], device=x.device) * eps
        _, x = pred.update_fn(x, vec_eps)
        return x

    def drift_fn(model, x, t):
        score_fn = get_score_fn(sde, model, train=False, continuous=True)
        return sde.reverse(score_fn, probability_flow=True).sde(x, t)[0]

    def ode_sampler(model, z=None):
        with torch.no_grad():
            x = sde.prior_sampling(shape).to(device) if z is None else z

            def ode_func(t, y):
                y = y.reshape(shape).to(torch.float32)
                vec_t = torch.ones(shape[0], device=y.device) * t
                return drift_fn(model, y, vec_t)

            sol = solve_ivp_rk(ode_func, (sde.T, eps), x.reshape(-1), rtol=rtol, atol=atol,
                               method=method)
            x = sol.y.reshape(shape).to(torch.float32)
            if denoise:
                x = denoise_update_fn(model, x)
            return inverse_scaler(x), sol.nfev

    return ode_sampler

"""GPU: the HIP blur measurement operator (csrc/blur.hip, op.blur) against the float64
restatement tests/blur_ref.py, its adjoint / autograd properties, the operator class, and
the DPS drift with it.

Tolerances.  float64: 1e-13 of max|input|.  float32: 4 K 2^-24 max|input| -- two passes of
K fused multiply-adds with non-negative weights summing to 1 (each pass: K roundings of a
running sum bounded by max|input|, plus the taps' own rounding to float32).  The inputs are
float32-representable, so both precisions see the same data and the same reference.
Dot-product identity: on positive data (no cancellation, so 'relative' is well defined)
both sides carry the element-wise relative error 2 (K + 1) 2^-24 <= 4 K 2^-24, together
8 K 2^-24; float64 1e-12.  The sums themselves are taken in float64 on the host.
DPS drifts: 1e-4 of max|ref|, the tolerance of test_gpu_dps.py.
"""
import functools

import numpy as np
import pytest
import torch

import blur_ref
from conftest import load_golden, net_fixture, product_config

pytestmark = pytest.mark.gpu

KS = [(1, 1), (3, 1), (5, 2), (13, 1), (13, 4), (33, 3)]
PLANES = [(1, 1), (1, 3), (17, 1)]
ASYM5 = (0.5, 0.3, 0.1, 0.07, 0.03)          # pins the flip (convolution, not correlation)


def _sizes(K):
    from op.blur import TILE_H as TH, TILE_W as TW
    p = K // 2
    cand = [(2, 5), (7, 9), (TH + 1, TW - 1), (2 * TH - 1, TW + 1), (p, p + 3)]
    return [(H, W) for H, W in dict.fromkeys(cand) if H >= 1 and p <= min(H, W)]


def _taps(K):
    return tuple(blur_ref.taps(max(K / 4.0, 0.5), K))


@functools.lru_cache(maxsize=None)
def _case(taps, s, H, W, planes, positive=False):
    """Inputs (float32-representable) and the float64 reference, computed once and shared by
    the float32 / float64 and forward / adjoint tests."""
    rng = np.random.default_rng([len(taps), s, H, W, planes[0] * planes[1]])
    Ho, Wo = blur_ref.out_size(H, s), blur_ref.out_size(W, s)
    draw = (lambda sh: rng.uniform(0.5, 1.5, sh)) if positive else rng.standard_normal
    x = draw(planes + (H, W)).astype(np.float32).astype(np.float64)
    y = draw(planes + (Ho, Wo)).astype(np.float32).astype(np.float64)
    out = dict(x=x, y=y, Ax=blur_ref.forward(x, taps, s), ATy=blur_ref.adjoint(y, taps, s, (H, W)))
    for v in out.values():
        v.setflags(write=False)
    return out


def _tol(dtype, K, scale):
    return (1e-13 if dtype == torch.float64 else 4 * K * 2.0 ** -24) * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("K,s", KS + [(5, 1), (5, 3)])
def test_forward_and_adjoint_match_the_restatement(hip, K, s, dtype):
    from op.blur import blur2d, blur2d_adjoint
    taps_list = [_taps(K)] if (K, s) in KS else []
    if K == 5:
        taps_list.append(ASYM5)
    n = 0
    for taps in taps_list:
        for H, W in _sizes(K):
            for planes in PLANES:
                c = _case(taps, s, H, W, planes)
                x = torch.tensor(c["x"], device=hip, dtype=dtype)
                y = torch.tensor(c["y"], device=hip, dtype=dtype)
                Ax = blur2d(x, taps, s)
                ATy = blur2d_adjoint(y, taps, s, (H, W))
                assert Ax.shape == c["Ax"].shape and Ax.dtype == dtype
                assert ATy.shape == x.shape and ATy.dtype == dtype
                e = np.abs(Ax.double().cpu().numpy() - c["Ax"]).max()
                ea = np.abs(ATy.double().cpu().numpy() - c["ATy"]).max()
                what = f"K={K} s={s} {H}x{W} planes={planes}"
                assert e <= _tol(dtype, K, np.abs(c["x"]).max()), f"forward {what}: {e:.3e}"
                assert ea <= _tol(dtype, K, np.abs(c["y"]).max()), f"adjoint {what}: {ea:.3e}"
                n += 1
    assert n >= 9


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_single_tap_returns_the_input_bit_for_bit(hip, dtype):
    from op.blur import blur2d
    for H, W in _sizes(1):
        x = torch.tensor(_case((1.0,), 1, H, W, (1, 3))["x"], device=hip, dtype=dtype)
        out = blur2d(x, [1.0], 1)
        assert out.data_ptr() != x.data_ptr() and torch.equal(out, x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("K,s", KS)
def test_adjoint_identity_and_reproducibility_on_the_device(hip, K, s, dtype):
    from op.blur import blur2d, blur2d_adjoint
    taps = _taps(K)
    rel = 1e-12 if dtype == torch.float64 else 8 * K * 2.0 ** -24
    for H, W in _sizes(K):
        c = _case(taps, s, H, W, (1, 3), positive=True)
        x = torch.tensor(c["x"], device=hip, dtype=dtype)
        y = torch.tensor(c["y"], device=hip, dtype=dtype)
        Ax = blur2d(x, taps, s)
        ATy = blur2d_adjoint(y, taps, s, (H, W))
        lhs = float(np.sum(Ax.double().cpu().numpy() * c["y"]))
        rhs = float(np.sum(c["x"] * ATy.double().cpu().numpy()))
        assert abs(lhs - rhs) <= rel * max(abs(lhs), abs(rhs)), (K, s, H, W, lhs, rhs)
        assert torch.equal(ATy, blur2d_adjoint(y, taps, s, (H, W)))


@pytest.mark.parametrize("K,s", [(3, 2), (5, 1)])
def test_gradcheck_and_gradgradcheck(hip, K, s):
    from op.blur import blur2d, gaussian_taps
    taps = gaussian_taps(1.0, K)
    x = torch.tensor(_case(tuple(taps.tolist()), s, 5, 6, (1, 2))["x"], device=hip,
                     requires_grad=True)
    assert x.dtype == torch.float64 and x.shape == (1, 2, 5, 6)
    f = lambda t: blur2d(t, taps, s)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x,))
    assert torch.autograd.gradgradcheck(f, (x,))


def test_non_contiguous_input_is_taken_as_its_contiguous_copy(hip):
    from op.blur import blur2d, blur2d_adjoint
    taps = _taps(5)
    base = torch.tensor(_case(taps, 2, 9, 7, (1, 3))["x"], device=hip, dtype=torch.float32)
    xt = base.transpose(2, 3)
    assert not xt.is_contiguous()
    assert torch.equal(blur2d(xt, taps, 2), blur2d(xt.contiguous(), taps, 2))
    y = blur2d(xt, taps, 2).transpose(2, 3).contiguous().transpose(2, 3)
    assert not y.is_contiguous()
    size = (y.shape[2] * 2, y.shape[3] * 2)
    assert torch.equal(blur2d_adjoint(y, taps, 2, size),
                       blur2d_adjoint(y.contiguous(), taps, 2, size))


def test_operator_contract_and_observe_sampling(hip):
    import sde_lib
    from configs._configdict import ConfigDict
    from inverse.conditional_sampling import get_controlled_sampler
    from inverse.operators import GaussianBlurOperator
    op = GaussianBlurOperator(std=2.0, size=5, factor=2)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 9, 12, generator=g).to(hip)
    y = op(x)
    assert y.shape == (2, 3, 5, 6) == op.out_shape(x.shape)
    y0 = op(x, keep_shape=False)
    assert y0.shape == (2, 3, 30) and torch.equal(y0, y.reshape(2, 3, 30))
    ref = blur_ref.forward(x.double().cpu().numpy(), blur_ref.taps(2.0, 5), 2)
    assert np.abs(y.double().cpu().numpy() - ref).max() <= _tol(torch.float32, 5, float(x.abs().max()))
    xt = op.transpose(y0, x.shape)
    assert xt.shape == x.shape and torch.equal(xt, op.transpose(y, x.shape))
    op.next()
    assert torch.equal(op(x), y)
    with pytest.raises(ValueError):
        op(x, invert=True)
    obs = sde_lib.LOBSVSDE(sde_lib.VPSDE(0.1, 20.0, 1000), y0, op)
    z = torch.randn(2, 3, 9, 12, generator=g).to(hip)
    t = torch.tensor([0.3, 0.7], device=hip)
    yt = obs.observe_sampling(z, t)
    assert yt.shape == (2, 3, 30)
    alpha, beta = obs.state_sde.marginal_coef(t)
    want = alpha[:, None, None] * y0 + beta[:, None, None] * op(z, keep_shape=False)
    assert torch.allclose(yt, want, rtol=1e-6, atol=1e-6)
    with pytest.raises(NotImplementedError, match="GaussianBlurOperator"):
        get_controlled_sampler(ConfigDict(dict(device=hip)), obs, tuple(x.shape), lambda t: 1.0 - t)


# --- DPS with the blur operator, on the net of tests/golden/dps.npz (setup as test_gpu_dps._setup)

class _AtenBlur:
    """The same operator from aten ops: index-gather symmetric pad, F.conv2d with the taps as
    a column then as a row, strided slice."""

    def __init__(self, taps, s):
        self.taps, self.s = torch.as_tensor(taps, dtype=torch.float64), s

    def next(self):
        pass

    @staticmethod
    def _symm(n, p, device):
        i = torch.arange(-p, n + p, device=device)
        return torch.where(i < 0, -1 - i, torch.where(i >= n, 2 * n - 1 - i, i))

    def __call__(self, x, keep_shape=True, invert=False):
        import torch.nn.functional as F
        K, s = self.taps.numel(), self.s
        p, o = K // 2, (s - 1) // 2
        B, C, H, W = x.shape
        xp = x[:, :, self._symm(H, p, x.device)][:, :, :, self._symm(W, p, x.device)]
        g = self.taps.flip(0).to(x)                    # conv2d correlates
        t = F.conv2d(xp.reshape(B * C, 1, H + 2 * p, W + 2 * p), g.view(1, 1, K, 1))
        t = F.conv2d(t, g.view(1, 1, 1, K))
        y = t[:, :, o::s, o::s]
        y = y.reshape(B, C, y.shape[2], y.shape[3])
        return y if keep_shape else y.reshape(B, C, -1)


def _dps_setup(hip, operators, max_steps=None):
    """One model, and one DPS sampler per operator, all seeing the same observation noise."""
    import models  # noqa: F401
    import sde_lib
    from configs._configdict import ConfigDict
    from inverse.conditional_sampling import get_dps_sampler
    from models import utils as mutils
    d = load_golden("dps.npz")
    cfg, sd, *_ = net_fixture("ddpm_a")
    c = product_config(cfg, hip)
    c.inverse = ConfigDict(dict(operator="gaussian_blur", sampler="dps",
                                variance=float(d["variance"]), solver="RK45"))
    if max_steps is not None:
        c.inverse.max_steps = max_steps
    model = mutils.create_model(c, wrap=False)
    model.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    model.eval()
    origin = torch.tensor(d["origin"], device=hip)
    sde = sde_lib.VPSDE(c.model.beta_min, c.model.beta_max, c.model.num_scales)
    shape = tuple(d["prior"].shape)
    samplers, noise = [], None
    for op in operators:
        y0 = op(origin, keep_shape=False)
        if noise is None:
            noise = torch.randn(y0.shape, generator=torch.Generator().manual_seed(5)).to(hip)
        assert y0.shape == noise.shape
        obs = sde_lib.LOBSVSDE(sde, y0, op)
        samplers.append(get_dps_sampler(c, obs, shape, eps=float(d["eps"]), noise=noise))
    return d, model, samplers


def _drifts_agree(hip, d, model, samplers):
    x = torch.tensor(d["prior"], device=hip).reshape(-1).to(torch.float64)
    fa, fb = (s.make_ode_func(model) for s in samplers)
    for tp in d["t_probe"]:
        ref = fa(float(tp), x).reshape(-1).double().cpu().numpy()
        out = fb(float(tp), x).reshape(-1).double().cpu().numpy()
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0
        err = np.abs(out - ref).max() / np.abs(ref).max()
        assert err < 1e-4, f"t={tp}: rel err {err:.2e}"


def test_dps_drift_single_tap_blur_equals_all_ones_inpainting(hip):
    from inverse.operators import GaussianBlurOperator, InpaintOperator
    shape = tuple(load_golden("dps.npz")["prior"].shape)
    ops = [InpaintOperator(mask=[torch.ones(shape, device=hip)]),
           GaussianBlurOperator(size=1, factor=1)]
    d, model, samplers = _dps_setup(hip, ops)
    _drifts_agree(hip, d, model, samplers)


def test_dps_drift_and_short_solve_match_the_aten_operator(hip):
    from inverse.conditional_sampling import get_solver
    from inverse.operators import GaussianBlurOperator
    op = GaussianBlurOperator(std=2.0, size=5, factor=2)
    d, model, samplers = _dps_setup(hip, [_AtenBlur(op.taps, 2), op], max_steps=2)
    _drifts_agree(hip, d, model, samplers)
    z = torch.tensor(d["prior"], device=hip)
    outs, nfev = [], []
    for s in samplers:
        outs.append(s(model, z=z.clone()))
        nfev.append(get_solver.last_nfe)
    assert all(torch.isfinite(o).all() for o in outs)
    assert nfev[0] == nfev[1] > 0


@pytest.mark.parametrize("module", ["nc_ddpmpp_deblur_dps", "nc_ddpmpp_sr_dps"])
def test_new_configs_run_the_dps_sampler(hip, module):
    """get_operator -> LOBSVSDE -> get_dps_sampler -> a one-step RK45 solve, at a reduced
    image size and batch (seeded weights)."""
    import importlib
    import models  # noqa: F401
    from conftest import seeded_fill_
    from inverse import inverse_lib
    from inverse.conditional_sampling import get_sampler, get_solver
    from inverse.operators import get_operator
    from models import utils as mutils
    c = importlib.import_module(f"configs.inverse.{module}").get_config()
    c.device = hip
    c.model.dropout = 0.0
    c.data.image_size = 32
    c.training.batch_size = 2
    c.inverse.max_steps = 1
    model = seeded_fill_(mutils.create_model(c, wrap=False), 3).eval()
    op = get_operator(c)
    shape = (2, c.data.num_channels, 32, 32)
    g = torch.Generator().manual_seed(1)
    y0 = op(torch.rand(shape, generator=g).to(hip), keep_shape=False)
    side = 32 if module.endswith("deblur_dps") else 8
    assert y0.shape == (2, c.data.num_channels, side * side)
    obs, eps = inverse_lib.get_obsvsde(c, y0, op)
    sampler = get_sampler(c, obs, shape, eps=eps)
    out = sampler(model, z=torch.randn(shape, generator=g).to(hip))
    assert out.shape == shape and torch.isfinite(out).all() and get_solver.last_nfe > 0

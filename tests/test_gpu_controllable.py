"""GPU: conditional PC sampling (inpainting, colorization) -- the projection kernels of
csrc/sampler.hip, the conditioned PCEngine and controllable_generation.py against the CPU
restatement tests/controllable_ref.py and the reference's recorded runs
(tests/golden/ctrl_*.npz).  Shapes are the smallest that reach each path: D = 35 is odd, not a
multiple of 4, and its sample boundaries fall inside a Philox block."""
import inspect

import numpy as np
import pytest
import torch

import controllable_ref as cref
from conftest import load_golden, product_config, record_err
from oracle import score_sde_ref
from controllable_ref import FIXTURES, fixture_net

pytestmark = pytest.mark.gpu

# whole recorded trajectories, relative to max(1, max|ref|): the tolerance of the existing PC
# fixtures (tests/test_gpu_models.py; they measure 2e-7 .. 2e-6)
PC_RTOL = 2e-4
# one colorize projection: each 3-term float32 dot has error <= 3 * 2^-24 * sum|terms| <=
# 3 * 2^-24 * sqrt(3) * max|in| = 3.1e-7 * max|in|, at most three transforms are chained
COLORIZE_TOL = 4e-6

SHAPE = (3, 1, 5, 7)
T3 = torch.tensor([0.9, 0.4567, 0.003])
PRED_NAMES = {"em": "euler_maruyama", "rd": "reverse_diffusion", "anc": "ancestral_sampling"}


def _step(hip, v=0):
    return torch.tensor([v], dtype=torch.int32, device=hip)


def _sde(kind, N=1000):
    import sde_lib
    sde = {"vp": lambda: sde_lib.VPSDE(0.1, 20., N), "subvp": lambda: sde_lib.subVPSDE(0.1, 20., N),
           "ve": lambda: sde_lib.VESDE(0.01, 50., N)}[kind]()
    return score_sde_ref.SDESpec(kind, N), sde


def _pred_kind(pred, kind):
    from op import sde_kernels as K
    if pred == "anc":
        return K.PRED_ANC_VE if kind == "ve" else K.PRED_ANC_VP
    return {"em": K.PRED_EM, "rd": K.PRED_RD}[pred]


def _padded(rows, hip):
    """`rows` [bdim, k] in row 2 of a 3-row table whose rows 0 and 1 are NaN; step = 2."""
    full = torch.full((3,) + tuple(rows.shape), float("nan"))
    full[2] = rows
    return full.to(hip)


def _times(bdim):
    return T3 if bdim == "B" else T3[1:2].expand(3).contiguous()


def _marginal_table(spec, sde, t, bdim, hip):
    """Product table rows == the restatement's (mean coefficient, std), then padded."""
    import sampling
    rows = sampling.marginal_rows(sde, t)
    mc, sd = cref.marginal(spec, t)
    assert torch.equal(rows[:, 1], sd)
    assert torch.equal(rows[:, 0], torch.ones_like(sd) if mc is None else mc)
    return _padded(rows if bdim == "B" else rows[:1], hip), mc, sd


def _masks(shape, g):
    mixed = (torch.rand(shape, generator=g) < 0.5).float()
    assert 0 < mixed.sum() < mixed.numel()
    return {"all0": torch.zeros(shape), "all1": torch.ones(shape), "mixed": mixed}


def _nan_like(x):
    return torch.full_like(x, float("nan"))


# ------------------------------------------------------------------ 1. inpaint, bit for bit

PRED_CASES = [("em", "vp"), ("em", "subvp"), ("em", "ve"), ("rd", "vp"), ("rd", "ve"),
              ("anc", "vp"), ("anc", "ve")]


@pytest.mark.parametrize("bdim", ["one", "B"])
@pytest.mark.parametrize("pred,kind", PRED_CASES)
def test_predictor_inpaint_bit_exact(hip, pred, kind, bdim):
    """Fused predictor + inpaint projection == the CPU restatement (oracle predictor, then
    controllable_ref.project_inpaint) == the unfused kernel followed by K.project, bit for bit:
    all four predictor kinds on VP / sub-VP / VE tables, bdim 1 and B, row 2 of NaN-padded
    tables, masks all-0 / all-1 / mixed, x_mean NULL."""
    import sampling
    from op import sde_kernels as K
    spec, sde = _sde(kind)
    g = torch.Generator().manual_seed(5)
    x, m, z, z2, data = (torch.randn(SHAPE, generator=g) for _ in range(5))
    t = _times(bdim)
    with torch.no_grad():
        ux, _ = score_sde_ref._predictor(
            PRED_NAMES[pred], spec, score_sde_ref.make_score(lambda x_, l_: m, spec, True), x, t,
            lambda: z)
    pk = _pred_kind(pred, kind)
    rows = sampling.coef_rows(sde, t, True, pk)
    coef = _padded(rows if bdim == "B" else rows[:1], hip)
    mtab, mc, sd = _marginal_table(spec, sde, t, bdim, hip)
    st = _step(hip, 2)
    kw = dict(noise=z.to(hip), score_mode=K.SCORE_RAW if kind == "ve" else K.SCORE_DIV,
              drift_mul_x=int(kind != "ve"))
    xd, md = x.to(hip), m.to(hip)
    uo = _nan_like(xd)
    K.predictor(pk, xd, md, coef, st, x_out=uo, x_mean=_nan_like(xd), **kw)
    assert torch.equal(uo.cpu(), ux)
    for name, mask in _masks(SHAPE, g).items():
        ref_x, ref_mean = cref.project_inpaint(ux, data, mask, mc, sd, z2)
        assert torch.isfinite(ref_x).all() and torch.isfinite(ref_mean).all()
        ckw = dict(data=data.to(hip), mask=mask.to(hip), noise2=z2.to(hip))
        fo, fm = _nan_like(xd), _nan_like(xd)
        K.predictor(pk, xd, md, coef, st, x_out=fo, x_mean=fm, cond=K.COND_INPAINT, mtab=mtab,
                    **ckw, **kw)
        assert torch.equal(fo.cpu(), ref_x), name
        assert torch.equal(fm.cpu(), ref_mean), name
        po, pm = _nan_like(xd), _nan_like(xd)
        K.project(K.COND_INPAINT, uo, mtab, st, x_out=po, x_mean=pm, **ckw)
        assert torch.equal(po, fo) and torch.equal(pm, fm), name
        # x_mean NULL, in place (what the engine passes)
        xi = xd.clone()
        K.predictor(pk, xi, md, coef, st, x_out=xi, x_mean=None, cond=K.COND_INPAINT, mtab=mtab,
                    **ckw, **kw)
        assert torch.equal(xi, fo), name
        pi = uo.clone()
        K.project(K.COND_INPAINT, pi, mtab, st, x_out=pi, x_mean=None, **ckw)
        assert torch.equal(pi, fo), name
        if name == "all1":  # every pixel known: the perturbed data and its mean
            assert torch.equal(fm.cpu(), cref._mean(mc, data))
        if name == "all0":  # nothing known: the plain update, and x_mean' = x' (the quirk)
            assert torch.equal(fo.cpu(), ux) and torch.equal(fm, fo)


def _langevin_expect(mode, x, m, z, rows, red, B_global, snr, divides):
    """The oracle's float32 expression order (score_sde_ref._corrector) given the reduced norms;
    sqrt(step * 2) in float64 rounded once = the correctly rounded float32 square root that the
    device returns (see tests/test_gpu_sampler.py)."""
    from op import sde_kernels as K
    bc = (slice(None),) + (None,) * (x.dim() - 1)
    g = -m / rows[:, K.C_SDIV][bc] if divides else m
    alpha = rows[:, K.C_ALPHA]
    r = snr * (red[1] / B_global) / (red[0] / B_global) if mode == 0 else snr * rows[:, K.C_AUX]
    step = r * r * 2 * alpha
    x_mean = x + step[bc] * g
    return x_mean + torch.sqrt((step * 2).double()).float()[bc] * z


@pytest.mark.parametrize("bdim", ["one", "B"])
@pytest.mark.parametrize("mode,kind", [(0, "vp"), (0, "ve"), (1, "vp"), (1, "ve")])
def test_langevin_inpaint_bit_exact(hip, mode, kind, bdim):
    import sampling
    from op import sde_kernels as K
    spec, sde = _sde(kind)
    g = torch.Generator().manual_seed(6)
    x, m, z, z2, data = (torch.randn(SHAPE, generator=g) for _ in range(5))
    t = _times(bdim)
    rows = sampling.coef_rows(sde, t, True)
    red = torch.tensor([1.37, 0.91]) * 3 * float(np.sqrt(35))
    snr = 0.16
    ux = _langevin_expect(mode, x, m, z, rows, red, 3, snr, kind != "ve")
    coef = _padded(rows if bdim == "B" else rows[:1], hip)
    mtab, mc, sd = _marginal_table(spec, sde, t, bdim, hip)
    st = _step(hip, 2)
    args = (mode, x.to(hip), m.to(hip), coef, st, red.to(hip))
    kw = dict(noise=z.to(hip), snr=snr, score_mode=K.SCORE_RAW if kind == "ve" else K.SCORE_DIV)
    uo = _nan_like(args[1])
    K.langevin_update(*args, x_out=uo, x_mean=_nan_like(uo), **kw)
    assert torch.equal(uo.cpu(), ux)
    for name, mask in _masks(SHAPE, g).items():
        ref_x, ref_mean = cref.project_inpaint(ux, data, mask, mc, sd, z2)
        ckw = dict(data=data.to(hip), mask=mask.to(hip), noise2=z2.to(hip))
        fo, fm = _nan_like(uo), _nan_like(uo)
        K.langevin_update(*args, x_out=fo, x_mean=fm, cond=K.COND_INPAINT, mtab=mtab, **ckw, **kw)
        assert torch.equal(fo.cpu(), ref_x) and torch.equal(fm.cpu(), ref_mean), name
        po, pm = _nan_like(uo), _nan_like(uo)
        K.project(K.COND_INPAINT, uo, mtab, st, x_out=po, x_mean=pm, **ckw)
        assert torch.equal(po, fo) and torch.equal(pm, fm), name
        xi = args[1].clone()
        K.langevin_update(mode, xi, *args[2:], x_out=xi, x_mean=None, cond=K.COND_INPAINT,
                          mtab=mtab, **ckw, **kw)
        assert torch.equal(xi, fo), name


# ------------------------------------------------------------------ 2. colorize kernel

def _rel(a, ref):
    return (a.cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("kind", ["vp", "ve"])
def test_colorize_kernels_vs_restatement(hip, kind):
    """B = 2, 3 x 5 x 7: the stand-alone projection and both fused forms against the restatement;
    fused == unfused then projected, bit for bit (same kernel arithmetic)."""
    import sampling
    from op import sde_kernels as K
    shape = (2, 3, 5, 7)
    spec, sde = _sde(kind)
    g = torch.Generator().manual_seed(7)
    x, m, z, z2 = (torch.randn(shape, generator=g) for _ in range(4))
    gray = torch.rand((2, 1, 5, 7), generator=g).repeat(1, 3, 1, 1).contiguous()
    t = torch.tensor([0.8, 0.01])
    mtab, mc, sd = _marginal_table(spec, sde, t, "B", hip)
    st = _step(hip, 2)
    ckw = dict(data=gray.to(hip), mtab=mtab, noise2=z2.to(hip))
    ref_x, ref_mean = cref.project_colorize(x, gray, mc, sd, z2)
    po, pm = _nan_like(x.to(hip)), _nan_like(x.to(hip))
    K.project(K.COND_COLORIZE, x.to(hip), mtab, st, x_out=po, x_mean=pm, data=gray.to(hip),
              noise2=z2.to(hip))
    for what, err in (("x", _rel(po, ref_x)), ("x_mean", _rel(pm, ref_mean))):
        print(f"colorize project {kind} {what}: err {err:.3e}")
        record_err(f"colorize project {kind} {what}", err, COLORIZE_TOL)
        assert err <= COLORIZE_TOL
    # only channel 0 of the data draw is consumed
    z2b = z2.clone()
    z2b[:, 1:] = 7.0
    qo = _nan_like(po)
    K.project(K.COND_COLORIZE, x.to(hip), mtab, st, x_out=qo, data=gray.to(hip),
              noise2=z2b.to(hip))
    assert torch.equal(qo, po)
    # fused predictor / Langevin == the unfused kernel then the projection
    pk = _pred_kind("rd", kind)
    coef = _padded(sampling.coef_rows(sde, t, True, pk), hip)
    kw = dict(noise=z.to(hip), score_mode=K.SCORE_RAW if kind == "ve" else K.SCORE_DIV)
    red = (torch.tensor([1.37, 0.91]) * 2 * float(np.sqrt(105))).to(hip)
    for launch in (
            lambda **k: K.predictor(pk, x.to(hip), m.to(hip), coef, st, drift_mul_x=int(kind != "ve"),
                                    **kw, **k),
            lambda **k: K.langevin_update(1, x.to(hip), m.to(hip), coef, st, red, snr=0.16, **kw, **k)):
        uo = _nan_like(po)
        launch(x_out=uo, x_mean=_nan_like(po))
        eo, em = _nan_like(po), _nan_like(po)
        K.project(K.COND_COLORIZE, uo, mtab, st, x_out=eo, x_mean=em, data=gray.to(hip),
                  noise2=z2.to(hip))
        fo, fm = _nan_like(po), _nan_like(po)
        launch(x_out=fo, x_mean=fm, cond=K.COND_COLORIZE, **ckw)
        assert torch.isfinite(fo).all() and not torch.equal(fo, uo)
        assert torch.equal(fo, eo) and torch.equal(fm, em)
        rx, rm = cref.project_colorize(uo.cpu(), gray, mc, sd, z2)
        assert _rel(fo, rx) <= COLORIZE_TOL and _rel(fm, rm) <= COLORIZE_TOL


@pytest.mark.parametrize("cond", ["inpaint", "colorize"])
def test_projection_grid_stride_second_pass(hip, cond):
    """More threads than the 8192 x 256 of one pass (elements for inpaint, pixels for colorize),
    odd sizes: the fused predictor equals the unfused kernel followed by the projection bit for
    bit, in place too, and the restatement on every element, the tail included."""
    import sampling
    from op import sde_kernels as K
    shape = (3, 1, 1, 700001) if cond == "inpaint" else (1, 3, 1, 2100001)
    assert shape[0] * shape[3] > 8192 * 256
    spec, sde = _sde("vp")
    g = torch.Generator().manual_seed(14)
    x, m, z, z2, data = (torch.randn(shape, generator=g) for _ in range(5))
    mask = (torch.rand(shape, generator=g) < 0.5).float()
    t = T3[:shape[0]]
    coef = _padded(sampling.coef_rows(sde, t, True, K.PRED_EM), hip)
    mtab, mc, sd = _marginal_table(spec, sde, t, "B", hip)
    st = _step(hip, 2)
    ck = K.COND_INPAINT if cond == "inpaint" else K.COND_COLORIZE
    xd, md, zd = x.to(hip), m.to(hip), z.to(hip)
    ckw = dict(data=data.to(hip), mask=mask.to(hip), noise2=z2.to(hip))
    uo = _nan_like(xd)
    K.predictor(K.PRED_EM, xd, md, coef, st, x_out=uo, noise=zd)
    po, pm = _nan_like(xd), _nan_like(xd)
    K.project(ck, uo, mtab, st, x_out=po, x_mean=pm, **ckw)
    fo, fm = _nan_like(xd), _nan_like(xd)
    K.predictor(K.PRED_EM, xd, md, coef, st, x_out=fo, x_mean=fm, noise=zd, cond=ck, mtab=mtab,
                **ckw)
    assert torch.isfinite(fo).all() and torch.isfinite(fm).all()
    assert torch.equal(fo, po) and torch.equal(fm, pm)
    xi = xd.clone()
    K.predictor(K.PRED_EM, xi, md, coef, st, x_out=xi, x_mean=None, noise=zd, cond=ck, mtab=mtab,
                **ckw)
    assert torch.equal(xi, fo)
    if cond == "inpaint":
        rx, rm = cref.project_inpaint(uo.cpu(), data, mask, mc, sd, z2)
        assert torch.equal(fo.cpu(), rx) and torch.equal(fm.cpu(), rm)
    else:
        rx, rm = cref.project_colorize(uo.cpu(), data, mc, sd, z2)
        assert _rel(fo, rx) <= COLORIZE_TOL and _rel(fm, rm) <= COLORIZE_TOL
        assert _rel(fo[..., -8:], rx[..., -8:]) <= COLORIZE_TOL


def test_colorize_binding_refuses_other_channel_counts(hip):
    from op import sde_kernels as K
    st = _step(hip)
    mtab = torch.ones(1, 1, 2, device=hip)
    for C in (1, 2, 4):
        x = torch.zeros(2, C, 5, 7, device=hip)
        out = torch.zeros_like(x)
        with pytest.raises(RuntimeError):
            K.project(K.COND_COLORIZE, x, mtab, st, x_out=out, data=x, noise2=x)
        with pytest.raises(RuntimeError):
            K.predictor(0, x, x, torch.ones(1, 1, 8, device=hip), st, x_out=out, noise=x,
                        cond=K.COND_COLORIZE, data=x, mtab=mtab, noise2=x)
        assert torch.equal(out, torch.zeros_like(x))
    # the C ABI itself refuses as well (D = 3 * HW, but C = 1)
    from op._lib import lib
    x = torch.zeros(2, 1, 3, 7, device=hip)
    rc = lib.bpk_pc_project_f32(K.COND_COLORIZE, x.data_ptr(), None, x.data_ptr(), None,
                                x.data_ptr(), None, mtab.data_ptr(), 1, None, 2, 1, 21, 0,
                                st.data_ptr(), 0, 0, None)
    assert rc != 0
    # a CPU tensor is refused
    with pytest.raises(RuntimeError):
        K.project(K.COND_INPAINT, torch.zeros(2, 1, 5, 7), mtab, st,
                  x_out=torch.zeros(2, 1, 5, 7, device=hip), data=x, mask=x)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. noise sites, sharding

@pytest.mark.parametrize("cond", ["inpaint", "colorize"])
def test_data_noise_is_the_philox_stream_under_its_own_draw_id(hip, cond):
    from op import sde_kernels as K
    B, off, seed, step, draw = 3, 6, 2 ** 40 + 3, 4, 2
    shape = (B, 1, 5, 7) if cond == "inpaint" else (B, 3, 5, 7)
    g = torch.Generator().manual_seed(3)
    x, m, data = (torch.randn(shape, generator=g).to(hip) for _ in range(3))
    mask = (torch.rand(shape, generator=g) < 0.5).float().to(hip)
    coef = (0.1 + torch.rand(5, B, 8, generator=g)).to(hip)
    mtab = (0.1 + torch.rand(5, B, 2, generator=g)).to(hip)
    st = _step(hip, step)
    ck = K.COND_INPAINT if cond == "inpaint" else K.COND_COLORIZE
    z_data = K.philox_normal(shape, seed, st, K.DATA_DRAW + draw, sample_offset=off, device=hip)
    z_upd = K.philox_normal(shape, seed, st, draw, sample_offset=off, device=hip)
    red = torch.tensor([3.0, 2.0], device=hip)
    launches = {
        "project": lambda n2, o, om: K.project(ck, x, mtab, st, x_out=o, x_mean=om, data=data,
                                               mask=mask, noise2=n2, seed=seed, draw=draw,
                                               sample_offset=off),
        "predictor": lambda n2, o, om: K.predictor(0, x, m, coef, st, x_out=o, x_mean=om, cond=ck,
                                                   data=data, mask=mask, mtab=mtab, noise2=n2,
                                                   seed=seed, draw=draw, sample_offset=off),
        "langevin": lambda n2, o, om: K.langevin_update(0, x, m, coef, st, red, x_out=o, x_mean=om,
                                                        cond=ck, data=data, mask=mask, mtab=mtab,
                                                        noise2=n2, seed=seed, draw=draw,
                                                        sample_offset=off)}
    for name, launch in launches.items():
        outs = []
        for n2 in (None, z_data, z_upd):
            o, om = _nan_like(x), _nan_like(x)
            launch(n2, o, om)
            outs.append((o, om))
        assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all(), name
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), name
        assert not torch.equal(outs[0][0], outs[2][0]), name


class _Toy(torch.nn.Module):
    """Elementwise score-net stand-ins that keep a run bounded: VP / sub-VP (score =
    -out / std) 0.5 x + 0.001 label, VE (score = out, label = sigma) -x / (1 + sigma^2)."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind

    def forward(self, x, lab):
        if self.kind == "ve":
            return -x / (1 + lab * lab)[:, None, None, None]
        return 0.5 * x + 0.001 * lab[:, None, None, None]


_toy_model = _Toy("vp")

# VP runs with a Langevin corrector need every DDPM beta = 20 / N below 1 (alpha > 0)
N_SMALL = 25


def test_inpaint_engine_is_shard_invariant(hip):
    """One eager engine at B = 4 (ALD corrector, EM predictor) == two engines at B = 2 with
    sample_offset 0 and 2 on the halves: the data draws follow the global sample index."""
    import sampling
    from dist import DistContext
    _, sde = _sde("vp", N_SMALL)
    shape = (4, 1, 5, 7)
    g = torch.Generator().manual_seed(8)
    prior, data = torch.randn(shape, generator=g), torch.rand(shape, generator=g)
    mask = (torch.rand(shape, generator=g) < 0.5).float()

    def run(sl, ctx):
        eng = sampling.PCEngine(sde, (sl.stop - sl.start,) + shape[1:],
                                sampling.EulerMaruyamaPredictor,
                                sampling.AnnealedLangevinDynamics, 0.16, 2, continuous=True,
                                device=hip, seed=77, use_graph=False, dist_ctx=ctx,
                                condition="inpaint")
        assert eng.sample_offset == sl.start
        return eng.run(_toy_model, prior[sl], data=data[sl].to(hip), mask=mask[sl].to(hip))

    x, xm = run(slice(0, 4), None)
    assert torch.isfinite(x).all() and not torch.equal(x, xm)
    for r in (0, 1):
        xr, xmr = run(slice(2 * r, 2 * r + 2), DistContext(rank=r, world_size=2))
        assert torch.equal(xr, x[2 * r:2 * r + 2]) and torch.equal(xmr, xm[2 * r:2 * r + 2])


# ------------------------------------------------------------------ 4. trajectories vs reference

def _product_model(d, hip):
    import models  # noqa: F401
    from models import utils as mutils
    cfg, params = fixture_net(d)
    model = mutils.create_model(product_config(cfg, hip), wrap=False)
    model.load_state_dict(params, strict=True)
    return model.eval()


@pytest.mark.parametrize("name", FIXTURES)
def test_engine_replays_the_reference_run(hip, name):
    import sampling
    import sde_lib
    d = load_golden(f"ctrl_{name}.npz")
    model = _product_model(d, hip)
    cond, N, n_steps = str(d["condition"]), int(d["N"]), int(d["n_steps"])
    pred, corr = str(d["predictor"]), str(d["corrector"])
    shape = tuple(d["prior"].shape)
    draws2 = torch.tensor(d["draws2"])
    if cond == "colorize":  # channel 0 is stored, the engine takes full-shape draws
        draws2 = torch.cat([draws2, torch.zeros(draws2.shape[:2] + (2,) + shape[2:])], dim=2)
    table = cref.engine_noise_table(torch.tensor(d["draws"]), draws2, N, pred, corr, n_steps)
    asked = set()

    def noise_fn(i, draw):
        asked.add((i, draw))
        return table[(i, draw)]

    eng = sampling.PCEngine(sde_lib.VPSDE(0.1, 20., N), shape, sampling.get_predictor(pred),
                            sampling.get_corrector(corr), float(d["snr"]), n_steps,
                            continuous=bool(d["continuous"]), eps=float(d["eps"]), device=hip,
                            noise_fn=noise_fn, use_graph=False, condition=cond)
    out, nfe = eng(model, x_init=torch.tensor(d["prior"]), data=torch.tensor(d["data"]).to(hip),
                   mask=torch.tensor(d["mask"]).to(hip))
    assert asked == set(table)
    ref = torch.tensor(d["out"])
    err = _rel(out, ref)
    print(f"ctrl {name}: engine vs reference err {err:.3e} (max|ref| {ref.abs().max().item():.3g})")
    record_err(f"ctrl engine {name}", err, PC_RTOL)
    assert err <= PC_RTOL


# ------------------------------------------------------------------ 5. exact invariant

def _last_mean_coef(sde, eps, B):
    import sampling
    t = sampling.pc_timesteps(sde, eps)[-1]
    return sampling.marginal_rows(sde, torch.ones(1) * t)[0, 0]


@pytest.mark.parametrize("kind,pred,corr", [("vp", "euler_maruyama", "langevin"),
                                            ("ve", "reverse_diffusion", "none"),
                                            ("ve", "none", "ald"),
                                            ("subvp", "euler_maruyama", "none")])
def test_known_pixels_of_the_denoised_output_are_the_scaled_data(hip, kind, pred, corr):
    """x_mean' at mask == 1 is 0 * x' + mc * data: with denoise=True the returned known pixels
    equal mc(t_last) * data bit for bit (VE: the data itself)."""
    import sampling
    _, sde = _sde(kind, N_SMALL)
    g = torch.Generator().manual_seed(9)
    data = torch.rand(SHAPE, generator=g)
    mask = (torch.rand(SHAPE, generator=g) < 0.5).float()
    eng = sampling.PCEngine(sde, SHAPE, sampling.get_predictor(pred), sampling.get_corrector(corr),
                            0.16, 2, continuous=True, eps=1e-3, device=hip, seed=5,
                            use_graph=False, condition="inpaint")
    out, _ = eng(_Toy(kind), data=data.to(hip), mask=mask.to(hip))
    out = out.cpu()
    assert torch.isfinite(out).all()
    mc = _last_mean_coef(sde, 1e-3, SHAPE[0])
    want = data if kind == "ve" else mc * data
    assert kind != "ve" or mc.item() == 1.0
    assert torch.equal(out[mask == 1], want[mask == 1])
    assert not torch.equal(out[mask == 0], want[mask == 0])


# ------------------------------------------------------------------ 6. graph

def test_inpaint_graph_equals_eager_and_is_reused_for_new_data(hip):
    import sampling
    import sde_lib
    from conftest import net_fixture
    import models  # noqa: F401
    from models import utils as mutils
    cfg, sd, *_ = net_fixture("ncsnpp_a")
    model = mutils.create_model(product_config(cfg, hip), wrap=False)
    model.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    model.eval()
    sde = sde_lib.VPSDE(0.1, 20., 25)
    shape = (2, 1, 32, 32)
    g = torch.Generator().manual_seed(10)
    prior = torch.randn(shape, generator=g)
    cases = [(torch.rand(shape, generator=g).to(hip),
              (torch.rand(shape, generator=g) < p).float().to(hip)) for p in (0.5, 0.2)]
    mk = lambda graph: sampling.PCEngine(sde, shape, sampling.EulerMaruyamaPredictor,
                                         sampling.LangevinCorrector, 0.075, 1, continuous=True,
                                         device=hip, seed=1234, use_graph=graph,
                                         condition="inpaint")
    graph = mk(True)
    assert graph.use_graph  # op._hipenv.graphs_allowed: the runtime setting is in effect
    xg, xmg = graph.run(model, prior, n_iters=5, data=cases[0][0], mask=cases[0][1])
    assert graph.graph is not None, getattr(graph, "capture_error", "")
    captured = list(graph.graph)
    xe, xme = mk(False).run(model, prior, n_iters=5, data=cases[0][0], mask=cases[0][1])
    assert torch.isfinite(xe).all()
    assert torch.equal(xg, xe) and torch.equal(xmg, xme)
    # new data / mask of the same shape: the same graph objects, a fresh engine's result
    xg2, xmg2 = graph.run(model, prior, n_iters=5, data=cases[1][0], mask=cases[1][1])
    assert len(graph.graph) == len(captured) and all(a is b for a, b in zip(graph.graph, captured))
    xe2, xme2 = mk(False).run(model, prior, n_iters=5, data=cases[1][0], mask=cases[1][1])
    assert not torch.equal(xe2, xe)
    assert torch.equal(xg2, xe2) and torch.equal(xmg2, xme2)


# ------------------------------------------------------------------ 7. public API

def test_public_api_signatures_shapes_and_refusals(hip):
    import controllable_generation as cg
    import sampling
    want = ["sde", "predictor", "corrector", "inverse_scaler", "snr", "n_steps",
            "probability_flow", "continuous", "denoise", "eps"]
    for get in (cg.get_pc_inpainter, cg.get_pc_colorizer):
        sig = inspect.signature(get)
        assert list(sig.parameters)[:len(want)] == want
        defaults = {k: v.default for k, v in sig.parameters.items() if k in want[5:]}
        assert defaults == dict(n_steps=1, probability_flow=False, continuous=False, denoise=True,
                                eps=1e-5)
    _, sde = _sde("vp", N_SMALL)
    g = torch.Generator().manual_seed(12)
    inpaint = cg.get_pc_inpainter(sde, sampling.EulerMaruyamaPredictor,
                                  sampling.LangevinCorrector, lambda v: 2 * v, 0.16,
                                  continuous=True, seed=3)
    assert list(inspect.signature(inpaint).parameters) == ["model", "data", "mask"]
    assert inpaint.fused
    data = torch.rand(SHAPE, generator=g)
    mask = (torch.rand(SHAPE, generator=g) < 0.5).float()
    out = inpaint(_toy_model, data.to(hip), mask.to(hip))
    assert out.shape == SHAPE and torch.isfinite(out).all()
    assert len(inpaint.engines) == 1
    inpaint(_toy_model, data.to(hip), (1 - mask).to(hip))
    assert len(inpaint.engines) == 1  # cached per (shape, device)
    with pytest.raises(RuntimeError):
        inpaint(_toy_model, data, mask)
    colorize = cg.get_pc_colorizer(sde, sampling.ReverseDiffusionPredictor,
                                   sampling.AnnealedLangevinDynamics, lambda v: v, 0.16,
                                   n_steps=2, continuous=True, seed=3)
    assert list(inspect.signature(colorize).parameters) == ["model", "gray_scale_img"]
    gray = torch.rand((2, 1, 5, 7), generator=g).repeat(1, 3, 1, 1)
    out = colorize(_toy_model, gray.to(hip))
    assert out.shape == (2, 3, 5, 7) and torch.isfinite(out).all()
    # the known channel of the decoupled output is the decoupled gray image, scaled
    mc = _last_mean_coef(sde, 1e-5, 2)
    got, ref = cref.decouple(out.cpu())[:, 0], mc * cref.decouple(gray)[:, 0]
    assert _rel(got, ref) <= COLORIZE_TOL
    with pytest.raises(RuntimeError):
        colorize(_toy_model, gray)
    with pytest.raises(ValueError):
        colorize(_toy_model, gray[:, :1].to(hip))


def test_user_predictor_runs_the_loop_fallback_and_keeps_the_invariant(hip):
    import controllable_generation as cg
    import sampling

    class HalfStepPredictor(sampling.Predictor):  # not one of the fused classes
        def update_fn(self, x, t):
            x_mean = x + 0.01 * self.score_fn(x, t)
            return x_mean + 0.01 * torch.randn_like(x), x_mean

    _, sde = _sde("vp", N_SMALL)
    g = torch.Generator().manual_seed(13)
    data = torch.rand(SHAPE, generator=g)
    mask = (torch.rand(SHAPE, generator=g) < 0.5).float()
    inpaint = cg.get_pc_inpainter(sde, HalfStepPredictor, sampling.LangevinCorrector,
                                  lambda v: v, 0.16, continuous=True, eps=1e-3)
    assert not inpaint.fused and not inpaint.engines
    out = inpaint(_toy_model, data.to(hip), mask.to(hip)).cpu()
    assert out.shape == SHAPE and torch.isfinite(out).all()
    want = _last_mean_coef(sde, 1e-3, SHAPE[0]) * data
    assert torch.equal(out[mask == 1], want[mask == 1])
    assert not torch.equal(out[mask == 0], want[mask == 0])

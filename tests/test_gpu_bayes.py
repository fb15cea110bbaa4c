"""GPU: the fused Bayesian weight sampler (csrc/bayes.hip, op.bayes), the Bayesian layers on
it (models/bayesian.py), B_PINN, its train step and PINN_KF.

Gate of every float comparison against the float64 restatement tests/bayes_ref.py: the same
restatement run with aten in float32 on the same inputs gives the yardstick E (max error
against float64, normalised by max|ref|); the kernel passes at max(4 E, 2 ulp_f32) of the same
normalisation.  Everything else is exact (bitwise)."""
import functools

import pytest
import torch

import bayes_ref
from conftest import build_pinn_weights, full_pinn_config, make_pinn_inputs, record_err

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 32, 56448, 2, 149760, 5]
PRIOR_MU = [0.0, 0.05, -0.1, 0.0, 0.2, 0.0, 0.01]
PRIOR_SIGMA = [0.1, 0.01, 1.0, 0.1, 0.5, 0.01, 0.3]
SEED, STEP = 0x1234_5678_9ABC, 7
ULP = 2.0 ** -23


def _gate(what, got, ref64, ref32):
    scale = float(ref64.abs().max())
    err = float((got.detach().double().cpu() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    tol = max(4 * e32, 2 * ULP)
    record_err(what, err, tol)
    print(f"{what}: err {err:.3e}  float32 restatement E {e32:.3e}  tol {tol:.3e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e} (float32 restatement {e32:.3e})"


def _segments():
    out, at = [], 0
    for n in SIZES:
        out.append((at, n))
        at += n
    return out


@functools.lru_cache(maxsize=None)
def _case(hip):
    """Inputs of (a)-(c) with the restatement's float64 and float32 results (computed once,
    never modified): misaligned segments crossing Philox blocks and workgroups, rho from
    {-30, -3, 0, 25} mixed with random values."""
    from op import bayes
    g = torch.Generator().manual_seed(21)
    P = sum(SIZES)
    mu = 0.3 * torch.randn(P, generator=g)
    rho = 2 * torch.randn(P, generator=g) - 2
    pick = torch.randint(0, 8, (P,), generator=g)
    for k, v in enumerate((-30.0, -3.0, 0.0, 25.0)):
        rho[pick == k] = v
    G = torch.randn(P, generator=g)
    c = 0.37
    segs = _segments()
    table = bayes.make_table([(o, n, pm, ps) for (o, n), pm, ps in
                              zip(segs, PRIOR_MU, PRIOR_SIGMA)], hip)
    eps = bayes.noise(P, SEED, STEP, hip).cpu()
    out = dict(P=P, mu=mu, rho=rho, G=G, c=c, table=table, eps=eps)
    for key, dt in (("64", torch.float64), ("32", torch.float32)):
        m, r = mu.to(dt).requires_grad_(), rho.to(dt).requires_grad_()
        W = bayes_ref.sample(m, r, eps.to(dt))
        kl = bayes_ref.kl(m, r, PRIOR_MU, PRIOR_SIGMA, segs)
        gm, gr = torch.autograd.grad((W * G.to(dt)).sum() + c * kl, (m, r))
        out[key] = dict(W=W.detach(), kl=kl.detach().reshape(1), gmu=gm, grho=gr)
    return out


def test_a_forward_matches_restatement(hip):
    from op import bayes
    d = _case(hip)
    assert torch.isfinite(d["eps"]).all() and 0.99 < float(d["eps"].std()) < 1.01
    W, _ = bayes.sample_kl(d["mu"].to(hip), d["rho"].to(hip), d["table"], SEED, STEP)
    _gate("bayes W", W, d["64"]["W"], d["32"]["W"])


def test_b_kl_matches_restatement_and_is_reproducible(hip):
    from op import bayes
    d = _case(hip)
    mu, rho = d["mu"].to(hip), d["rho"].to(hip)
    _, kl = bayes.sample_kl(mu, rho, d["table"], SEED, STEP)
    _gate("bayes KL", kl.reshape(1), d["64"]["kl"], d["32"]["kl"])
    _, kl2 = bayes.sample_kl(mu, rho, d["table"], SEED, STEP)
    assert torch.equal(kl, kl2)
    for v in (-100.0, 30.0):
        W, k = bayes.sample_kl(mu, torch.full_like(rho, v), d["table"], SEED, STEP)
        assert torch.isfinite(k) and torch.isfinite(W).all(), v


def test_c_backward_matches_restatement(hip):
    from op import bayes
    d = _case(hip)
    mu, rho = d["mu"].to(hip).requires_grad_(), d["rho"].to(hip).requires_grad_()
    W, kl = bayes.sample_kl(mu, rho, d["table"], SEED, STEP)
    gmu, grho = torch.autograd.grad((W * d["G"].to(hip)).sum() + d["c"] * kl, (mu, rho))
    _gate("bayes d/dmu", gmu, d["64"]["gmu"], d["32"]["gmu"])
    _gate("bayes d/drho", grho, d["64"]["grho"], d["32"]["grho"])
    # the ends of the documented rho range: finite gradients
    for v in (-100.0, 30.0):
        r = torch.full_like(rho, v).requires_grad_()
        W, kl = bayes.sample_kl(mu, r, d["table"], SEED, STEP)
        ga, gb = torch.autograd.grad(W.sum() + kl, (mu, r))
        assert torch.isfinite(ga).all() and torch.isfinite(gb).all(), v


def test_c_aten_composition_agrees(hip):
    """BPK_BAYES_FUSED=0: the same arithmetic on the same noise."""
    from op import bayes
    d = _case(hip)
    mu, rho = d["mu"].to(hip).requires_grad_(), d["rho"].to(hip).requires_grad_()
    W, kl = bayes.sample_kl_aten(mu, rho, d["table"], SEED, STEP)
    _gate("bayes W (aten composition)", W.detach(), d["64"]["W"], d["32"]["W"])
    gmu, grho = torch.autograd.grad((W * d["G"].to(hip)).sum() + d["c"] * kl, (mu, rho))
    # the switch's own gradients and KL: float32 aten, a blocked sum of 2e5 terms (a few
    # 1e-7 relative at most); 1e-5 leaves room for nothing but a wrong formula
    scale = float(d["64"]["grho"].abs().max())
    assert float((grho.double().cpu() - d["64"]["grho"]).abs().max()) / scale < 1e-5
    assert abs(float(kl.detach()) / float(d["64"]["kl"]) - 1) < 1e-5
    assert torch.isfinite(gmu).all()


def test_d_noise_stream(hip):
    from op import bayes
    d = _case(hip)
    mu = torch.zeros(d["P"], device=hip)  # W - mu = sigma * eps exactly
    rho = d["rho"].to(hip)
    W0, _ = bayes.sample_kl(mu, rho, d["table"], SEED, STEP)
    W1, _ = bayes.sample_kl(mu, rho, d["table"], SEED, STEP)
    assert torch.equal(W0, W1) and W0.data_ptr() != W1.data_ptr()
    W2, _ = bayes.sample_kl(mu, rho, d["table"], SEED, STEP + 1)
    sigma = bayes_ref.softplus(rho)
    assert (sigma > 0).all()
    assert bool(((W2 - mu) != (W0 - mu)).all())
    W3, _ = bayes.sample_kl(mu, rho, d["table"], SEED + 1, STEP)
    assert float(((W3 - mu) != (W0 - mu)).float().mean()) > 0.999


def _layer_case(kind):
    from models import layers
    if kind == "3x3":
        return (lambda: layers.Conv2d(16, 16, 3, padding=1)), (2, 16, 16, 16)
    if kind == "1x1":
        return (lambda: layers.Conv2d(32, 16, 1)), (2, 32, 16, 16)
    return (lambda: layers.ConvTranspose2d(2, 2, kernel_size=4, stride=2, padding=1, bias=False,
                                           groups=2)), (2, 2, 16, 16)


@pytest.mark.parametrize("kind", ["3x3", "1x1", "convT_g2"])
def test_e_no_stale_filter_cache(hip, kind):
    """Two forwards under no_grad draw two networks (op.conv's per-weight filter cache must not
    serve the first draw's transform), each the deterministic layer on that draw's weights."""
    import torch.nn as nn
    from models.bayesian import dnn_to_bnn

    class One(nn.Module):
        def __init__(self, layer):
            super().__init__()
            self.layer = layer

        def forward(self, x):
            return self.layer(x)

    make, shape = _layer_case(kind)
    torch.manual_seed(3)
    net = dnn_to_bnn(One(make()).to(hip), {"prior_sigma": 0.1, "posterior_rho_init": -3.0},
                     seed=4)
    det = make().to(hip)
    x = torch.randn(shape, device=hip)
    outs = []
    with torch.no_grad():
        for _ in range(2):
            y = net(x)
            det.weight.copy_(net.layer.weight)
            if det.bias is not None:
                det.bias.copy_(net.layer.bias)
            else:
                assert net.layer.bias is None
            assert torch.equal(y, det(x))
            outs.append(y)
    assert net.bayes.step == 2
    assert not torch.equal(outs[0], outs[1])
    assert float((outs[0] - outs[1]).abs().max()) > 1e-3


@functools.lru_cache(maxsize=None)
def _pinn_case(hip):
    """The shipped 64 x 64 config at B = 2 on the device, seeded inputs and a B_PINN initialised
    by MOPED from seeded deterministic weights (activations of a sane scale)."""
    from configs.pinn import pinn_pde
    from pinn_kalman.pinn import B_PINN, PINN
    c = full_pinn_config(pinn_pde.get_config)
    batch = tuple(v.to(hip) for v in make_pinn_inputs(c, 1))
    c.device = hip
    bp = B_PINN(c, build_pinn_weights(PINN, c))
    return c, bp, batch


def _load_sample(pinn, bp):
    """Copy each layer's exposed sample of the last draws into a plain PINN."""
    with torch.no_grad():
        for net, bnet in ((pinn.flownet, bp.flownet), (pinn.pressurenet, bp.pressurenet)):
            params = dict(net.named_parameters())
            assert list(params) == [n for n, _ in bnet.bayes.segments]
            for (name, _), w in zip(bnet.bayes.segments, bnet.bayes.sample):
                params[name].copy_(w)
            for name, m in bnet.named_modules():
                if hasattr(m, "_iw"):
                    assert torch.equal(m.weight, params[name + ".weight"])


def test_f_forward_plumbing_bit_identical(hip):
    from pinn_kalman.pinn import PINN
    c, bp, (f1, f2, x, y, t, _) = _pinn_case(hip)
    bp.reseed(1)
    with torch.no_grad():
        flows, pres = bp(f1, f2, x, y, t)
        det = PINN(c)
        _load_sample(det, bp)
        flows_d, pres_d = det(f1, f2, x, y, t)
    assert len(flows) == len(flows_d) == 6 and tuple(pres.shape) == (2, 1, 64, 64)
    assert all(torch.isfinite(f).all() for f in flows) and torch.isfinite(pres).all()
    for a, b in zip(flows, flows_d):
        assert torch.equal(a, b)
    assert torch.equal(pres, pres_d)
    assert bp.flownet.bayes.step == bp.pressurenet.bayes.step == 1
    assert torch.isfinite(bp.flownet.kl_loss()) and float(bp.pressurenet.kl_loss()) > 0


def _chain(bayes_mod, gW, coef, eps, dt):
    """(gmu, grho) of sum(W gW) + coef KL through the restatement in dtype dt (on the CPU)."""
    m = bayes_mod["mu"].to(dt).requires_grad_()
    r = bayes_mod["rho"].to(dt).requires_grad_()
    W = bayes_ref.sample(m, r, eps.to(dt))
    kl = bayes_ref.kl(m, r, bayes_mod["pm"], bayes_mod["ps"], bayes_mod["segs"])
    return torch.autograd.grad((W * gW.to(dt)).sum() + coef * kl, (m, r))


def test_g_prelim_train_step(hip):
    import losses
    from inverse.operators import InpaintOperator
    from models.ema import ExponentialMovingAverage
    from op import bayes
    from pinn_kalman.pinn import PINN
    c, bp, batch = _pinn_case(hip)
    f1, f2, x, y, t, target = batch
    B = c.training.batch_size
    bp.reseed(5)
    before = {k: dict(mu=n.bayes.mu.detach().clone(), rho=n.bayes.rho.detach().clone())
              for k, n in (("f", bp.flownet), ("p", bp.pressurenet))}
    state = dict(optimizer=(losses.get_optimizer(c, bp.flownet.parameters(), is_bpinn=True),
                            losses.get_optimizer(c, bp.pressurenet.parameters(), 0.05,
                                                 is_bpinn=True)),
                 model=bp, ema=ExponentialMovingAverage(bp.parameters(), c.model.ema_rate),
                 step=50)
    real_opt = losses.optimization_manager(c, is_bpinn=True)
    seen = []

    def optimize_fn(opt, params, step):
        params = list(params)
        seen.append([p.grad.detach().clone() for p in params])  # before clipping
        real_opt(opt, params, step=step)

    g = torch.Generator().manual_seed(8)
    mask = (torch.rand(f1.shape, generator=g) < 0.1).float().to(hip)
    z = [torch.randn(f1.shape, generator=g).to(hip) for _ in range(2)]
    op = InpaintOperator(mask=[mask])
    step_fn = losses.get_prelim_step_fn(c, True, optimize_fn, is_bpinn=True)
    real, it = torch.randn_like, iter(z)
    torch.randn_like = lambda v, *a, **k: next(it).clone()
    try:
        loss, v_loss, p_loss = step_fn(state, op, batch)
    finally:
        torch.randn_like = real
    assert state["step"] == 51 and torch.equal(loss, v_loss + p_loss)
    assert len(seen) == 2 and all(len(s) == 2 for s in seen)

    # the same losses and weight gradients from a plain PINN on the same sampled weights
    det = PINN(c)
    error_fn = torch.nn.MSELoss()
    for key, net, dnet, grads, coef in (("f", bp.flownet, det.flownet, seen[0], 0.1),
                                        ("p", bp.pressurenet, det.pressurenet, seen[1], 0.01)):
        b = net.bayes
        W, kl = bayes.sample_kl(before[key]["mu"], before[key]["rho"], b.table, b.seed, 0)
        assert torch.equal(kl, b.kl_loss().detach())
        params = dict(dnet.named_parameters())
        with torch.no_grad():
            for (name, shape), w in zip(b.segments, torch.split(W, b.sizes)):
                params[name].copy_(w.view(shape))
        if key == "f":
            o1 = losses._observe(c, op, f1, z[0])
            o2 = losses._observe(c, op, f2, z[1])
            data = dnet.multiscale_data_mse(dnet(o1, o2, x, y, t), target, error_fn=error_fn)
            got = v_loss
        else:
            pyramid = [target[:, 0:2]]
            for _ in range(len(c.model.feature_nums)):
                fl = pyramid[-1]
                pyramid.append(torch.nn.functional.interpolate(
                    fl, size=(fl.shape[2] // 2, fl.shape[3] // 2), mode="bilinear",
                    align_corners=False))
            data = dnet.data_mse(dnet(pyramid[::-1], x, y, t), target, error_fn=error_fn)
            got = p_loss
        assert torch.isfinite(data) and float(kl) > 0
        assert torch.equal(got, data + kl / B * coef), (float(got), float(data), float(kl))
        data.backward()
        # a weight the forward never used (the coarsest level's flow upsampler): zero gradient
        gW = torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad).reshape(-1)
                        for p in dnet.parameters()]).cpu()
        assert torch.isfinite(gW).all() and float(gW.abs().max()) > 0
        mod = dict(mu=before[key]["mu"].cpu(), rho=before[key]["rho"].cpu(), pm=b.prior_mu,
                   ps=b.prior_sigma, segs=[(o, n) for o, n, _, _ in b.rows])
        eps = bayes.noise(b.numel, b.seed, 0, hip).cpu()
        g64 = _chain(mod, gW, coef / B, eps, torch.float64)
        g32 = _chain(mod, gW, coef / B, eps, torch.float32)
        _gate(f"B-PINN prelim step d/dmu ({key})", grads[0], g64[0], g32[0])
        _gate(f"B-PINN prelim step d/drho ({key})", grads[1], g64[1], g32[1])
        # the step moved both vectors
        assert float((b.mu.detach() != before[key]["mu"]).float().mean()) > 0.9
        assert float((b.rho.detach() != before[key]["rho"]).float().mean()) > 0.9
        assert torch.isfinite(b.mu).all() and torch.isfinite(b.rho).all()
        assert b.step == 1


def test_h_monte_carlo_outputs(hip):
    c, bp, (f1, f2, x, y, t, _) = _pinn_case(hip)
    with torch.no_grad():
        bp.reseed(3)
        flows, press = bp.sample_uvp(f1, f2, x, y, t, n=4)
        assert len(flows) == len(press) == 4
        fs, ps = torch.stack(flows), torch.stack(press)
        for s in (fs.std(0), ps.std(0)):
            assert torch.isfinite(s).all() and (s > 0).all()
        steps = torch.stack([bp.step(f2, f) for f in flows])
        bp.reseed(3)
        out = bp.predict(f1, f2, x, y, t, n=4)
    shapes = [(2, 2, 64, 64), (2, 1, 64, 64), (2, 1, 64, 64)]
    assert [tuple(o.shape) for o in out] == shapes + shapes
    want = (fs.mean(0), ps.mean(0), steps.mean(0), fs.std(0), ps.std(0), steps.std(0))
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    assert bp.flownet.bayes.step == 4


def test_i_pinn_kf_step(hip):
    """One PINN_KF step.  The measurement factor is std^2 (the reference's construction), so a
    filter's posterior variance is ~ std^4 against the prior variance 1e-2 of `initialize`: the
    float32 square-root downdates keep status 0 only while std^4 >> 64 eps_f32 1e-2, i.e. the
    Monte-Carlo std of EVERY pixel >> 0.014 (and std^2 far from overflow).  With n = 4 the
    smallest of the 12288 per-pixel stds is ~ 0.05 of the typical one, so the typical std must
    be of the order of the fields: the B_PINN is initialised by MOPED with delta = 2 from the
    seeded weights.  Measured on the MI355X (per-pixel std, min .. max): delta 0.01 -> flow
    5.6e-5 .. 2.2e-3 (192 of 256 filters flagged), 0.5 -> 4.0e-3 .. 0.10 (9 flagged), 2 ->
    0.09 .. 3.5, pressure 0.05 .. 10 (none); the default initialisation of an untrained net
    overflows PressureNet (std ~ 1e17)."""
    from configs.pinn import pinn_pde
    from pinn_kalman.pinn import B_PINN, PINN
    from pinn_kalman.ukf import PINN_KF, UKF
    from pinn_kalman.ukf_utils import patch
    c = full_pinn_config(pinn_pde.get_config)
    f1, f2, x, y, t, _ = (v.to(hip) for v in make_pinn_inputs(c, 1))
    c.device = hip
    c.model.bpinn_moped_delta = 2.0
    bp = B_PINN(c, build_pinn_weights(PINN, c))
    assert c.kf.patch_size == 8
    f0, f, xs, ys, ts = f1[:1], f2[:1], x[:1], y[:1], t[:1]
    g = torch.Generator().manual_seed(4)
    v0 = (0.1 * torch.randn(1, 2, 64, 64, generator=g)).to(hip)
    p0 = (0.1 * torch.randn(1, 1, 64, 64, generator=g)).to(hip)
    kf = PINN_KF(c)
    kf.pinn.load_state_dict(bp.state_dict())  # loading weights is the caller's job
    kf.pinn.reseed(6)
    kf.initialize(f0, v0, p0)
    out = kf(xs, ys, ts, f, n=4)
    assert kf.pinn.flownet.bayes.step == 4 and kf.f_prev is f
    # the same composition by hand
    with torch.no_grad():
        bp.reseed(6)
        flows, press = bp.sample_uvp(f0, f, xs, ys, ts, n=4, size=(64, 64))
        fs, ps = torch.stack(flows), torch.stack(press)
        print(f"PINN_KF: flow std {float(fs.std(0).min()):.3e} .. {float(fs.std(0).max()):.3e}, "
              f"pressure std {float(ps.std(0).min()):.3e} .. {float(ps.std(0).max()):.3e}")
        ukf = UKF(c).to(hip)
        ukf.initialize(patch(torch.cat([f0, v0, p0], dim=1), 8), 1e-2)
        ukf.measurement.update_uncertainty(fs.std(0), ps.std(0))
        want = ukf(torch.cat([f, fs.mean(0), ps.mean(0)], dim=1))
    assert tuple(out.shape) == (1, 4, 64, 64) and torch.isfinite(out).all()
    assert int(kf.ukf.ukf.status.abs().sum()) == 0
    assert torch.equal(out, want)
    # a sparse density observation
    mask = (torch.rand(64, 64, generator=g) < 0.3).float()
    kfm = PINN_KF(c, compat=False, mask=mask)
    kfm.pinn.load_state_dict(bp.state_dict())
    kfm.initialize(f0, v0, p0)
    outm = kfm(xs, ys, ts, f, n=4)
    assert tuple(outm.shape) == (1, 4, 64, 64) and torch.isfinite(outm).all()

"""GPU parity of the PINN path (HIP correlation + grid_sample grad2 inside FlowNet /
PressureNet, equation_mse, the PINN and preliminary train steps) against the oracle and
the reference-generated fixtures (tests/golden/make_golden_pinn.py).

Tolerances (fp32, different summation orders / conv algorithms): correlation 1e-5
absolute on O(1) data; network outputs 1e-4 relative to max|ref|; equation_mse values and
their input / parameter sensitivities 2e-3 relative (they are products and sums of
first and second derivatives through ~30 layers); the parameter gradients of
equation_mse against the reference's float64 truth, no worse than the reference's own
float32 error up to a factor 2 (conftest.param_grads_vs_truth); post-step parameters 1e-5 absolute
(Adam moves each parameter by <= lr)."""

import numpy as np
import pytest
import torch

from conftest import (build_pinn_weights, load_golden, param_grads_vs_truth, record_err,
                      sample_idx, small_config)
from oracle import correlation_ref as cr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,s", [((2, 16, 32, 32), 1), ((3, 5, 9, 13), 1),
                                     ((2, 4, 10, 7), 2), ((1, 128, 2, 2), 1),
                                     ((0, 3, 4, 4), 1)])
def test_correlation_matches_oracle(hip, shape, s):
    from op.correlation import FunctionCorrelation
    g = torch.Generator().manual_seed(0)
    a = torch.randn(*shape, generator=g)
    b = torch.randn(*shape, generator=g)
    ad, bd = a.to(hip).requires_grad_(), b.to(hip).requires_grad_()
    out = FunctionCorrelation(ad, bd, s)
    ref = cr.forward(a.numpy(), b.numpy(), s)
    assert out.shape == ref.shape
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    if a.numel() == 0:
        return
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(hip))
    gf, gs = cr.backward(a.numpy(), b.numpy(), go.numpy(), s)
    np.testing.assert_allclose(ad.grad.cpu().numpy(), gf, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(bd.grad.cpu().numpy(), gs, rtol=1e-5, atol=1e-5)


def test_correlation_rejects_cpu_tensors():
    from op.correlation import FunctionCorrelation
    with pytest.raises(RuntimeError, match="HIP"):
        FunctionCorrelation(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), 1)


def _model(dev):
    from configs.pinn import pinn_pde
    from pinn_kalman.pinn import PINN
    c = small_config(pinn_pde.get_config)
    m = build_pinn_weights(PINN, c).to(dev)
    c.device = dev
    return c, m


def _close(a, ref, rel, what, floor=1e-30):
    """max|a - ref| <= rel * max(max|ref|, floor); `floor` covers tensors whose exact
    gradient is zero (e.g. conv biases feeding an InstanceNorm) and hold only rounding."""
    a = np.asarray(a, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(a - ref).max() / max(np.abs(ref).max(), floor)
    assert err <= rel, f"{what}: rel err {err:.3e} > {rel}"


def test_pinn_forward_and_residual_match_reference(hip):
    d = load_golden("pinn_fwd.npz")
    c, m = _model(hip)
    m.train()
    T = lambda k: torch.tensor(d[k], device=hip)
    x, y, t = (T(k).requires_grad_() for k in ("x", "y", "t"))
    flows, pres = m(T("f1"), T("f2"), x, y, t)
    assert len(flows) == int(d["n_flows"])
    for i, fl in enumerate(flows):
        _close(fl.detach().cpu(), d[f"flow{i}"], 1e-4, f"flow{i}")
    _close(pres.detach().cpu(), d["pres"], 1e-4, "pressure")
    eq7 = m.equation_mse(x, y, t, flows[-1], pres, 10000000.0)
    _close(eq7.item(), d["eq7"], 2e-3, "equation_mse Re=1e7")
    m.zero_grad()
    eq50 = m.equation_mse(x, y, t, flows[-1], pres, 50.0)
    _close(eq50.item(), d["eq50"], 2e-3, "equation_mse Re=50")
    gx, gy, gt = torch.autograd.grad(eq50, (x, y, t), retain_graph=True)
    for name, v in (("gx", gx), ("gy", gy), ("gt", gt)):
        _close(v.cpu(), d[name], 2e-3, name)
    eq50.backward()
    worst, wname, n = param_grads_vs_truth(m, d, load_golden("pinn_fwd_f64.npz"))
    record_err(f"pinn16 residual param grads vs float64 truth, fraction of the limit "
               f"(worst tensor: {wname})", worst, 1.0)
    assert n > 50


@pytest.mark.parametrize("fixture,factory", [("pinn_step.npz", "get_pinn_step_fn"),
                                             ("prelim_step.npz", "get_prelim_step_fn")])
def test_pinn_train_steps_match_reference(hip, fixture, factory):
    import losses
    from inverse.operators import InpaintOperator
    from models.ema import ExponentialMovingAverage
    d = load_golden(fixture)
    c, m = _model(hip)
    em = ExponentialMovingAverage(m.parameters(), decay=c.model.ema_rate)
    opt_f = losses.get_optimizer(c, m.flownet.parameters())
    opt_p = losses.get_optimizer(c, m.pressurenet.parameters(), 0.001)
    state = dict(optimizer=(opt_f, opt_p), model=m, ema=em, step=50)
    step_fn = getattr(losses, factory)(c, train=True, optimize_fn=losses.optimization_manager(c))
    T = lambda k: torch.tensor(d[k], device=hip)
    batch = (T("f1"), T("f2"), T("x").requires_grad_(), T("y").requires_grad_(),
             T("t").requires_grad_(), T("target"))
    op = InpaintOperator(mask=[T("mask")])
    draws = [T(k) for k in sorted((k for k in d.files if k.startswith("noise")),
                                  key=lambda s: int(s[5:]))]
    real = torch.randn_like
    it = iter(draws)
    torch.randn_like = lambda v, *a, **k: next(it).clone()
    grads = {}
    for opt, pref in ((opt_f, "flownet."), (opt_p, "pressurenet.")):
        net = getattr(m, pref[:-1])

        def capture(*a, _real=opt.step, _net=net, _pref=pref, **k):
            # after this net's clip_grad_norm_, as the fixture generator records it
            for kk, p in _net.named_parameters():
                if p.grad is not None:
                    grads[_pref + kk] = p.grad.detach().clone()
            return _real(*a, **k)

        opt.step = capture
    try:
        out = step_fn(state, op, batch)
    finally:
        torch.randn_like = real
    np.testing.assert_allclose([o.item() for o in out], d["losses"], rtol=2e-4, atol=1e-9)
    assert state["step"] == int(d["step1"])
    gscale = max(np.abs(d[k]).max() for k in d.files if k.startswith("g:"))
    # parameters whose exact gradient is zero (conv biases feeding an InstanceNorm) hold
    # rounding noise only, which Adam normalises to steps of up to lr: allow lr there
    lr = c.optim.lr * min(50 / c.optim.warmup, 1.0)
    atol = {}
    for k, p in m.named_parameters():
        noise_only = "g:" + k in d.files and np.abs(d["g:" + k]).max() <= 1e-4 * gscale
        atol[k] = 2 * lr if noise_only else 1e-5
        if "g:" + k in d.files:
            g = grads[k].reshape(-1).cpu().numpy()
            _close(g[sample_idx(g.size)], d["g:" + k], 5e-3, "grad " + k, 1e-4 * gscale)
        v = p.detach().reshape(-1).cpu().numpy()
        np.testing.assert_allclose(v[sample_idx(v.size)], d["p1:" + k], atol=atol[k],
                                   err_msg="param " + k)
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    for k, s in zip(names, em.shadow_params):
        v = s.reshape(-1).cpu().numpy()
        np.testing.assert_allclose(v[sample_idx(v.size)], d["ema:" + k], atol=atol[k])


def test_simulator_step_rollout_bit_exact(hip):
    """pinn_kalman.simulator.step (fused ns_step rollout of replicated snapshots) equals the
    reference's three-op sequence per step (C oracle), bit for bit."""
    from oracle import ns_step_ref
    from pinn_kalman import simulator
    rng = np.random.default_rng(0)
    begin = np.zeros((2, 6, 200, 200), np.float32)
    begin[:, 2] = rng.uniform(0.1, 1.0, (2, 200, 200))
    begin[:, 3:5] = rng.uniform(0.05, 0.5, (2, 2, 200, 200)) * rng.choice([-1, 1], (2, 2, 200, 200))
    begin[:, 5] = rng.normal(0, 0.01, (2, 200, 200))
    res, vel, pres = simulator.step(None, begin, t_range=(0, 3), replicas=2, device=hip)
    f = np.repeat(begin[0, 2:3, 8:200, 4:-4][None], 2, 0)
    v = begin[0, 3:5, 8:200, 4:-4][None][:, ::-1]
    v = np.ascontiguousarray(np.repeat(v, 2, 0))
    p = np.repeat(begin[0, 5:6, 8:200, 4:-4][None], 2, 0)
    for i in range(3):
        v = ns_step_ref.update_velocity(v, p, simulator.dt, simulator.dx, True)
        p = ns_step_ref.update_pressure(p, v, simulator.dt, simulator.dx)
        f = ns_step_ref.update_density(f, v, simulator.dt, simulator.dx)
        np.testing.assert_array_equal(vel[i].cpu().numpy(), v)
        np.testing.assert_array_equal(pres[i].cpu().numpy(), p)
        np.testing.assert_array_equal(res[i].cpu().numpy(), f)


def test_stencil_gradient_forward_exact_and_adjoint(hip):
    """ns_step stencil gradient == C oracle bit for bit; its backward is the exact adjoint
    (<D f, g> = <f, D^T g>) and second derivatives flow through it."""
    from op.ns_step import stencil_gradient
    from oracle import ns_step_ref
    rng = np.random.default_rng(0)
    f = rng.standard_normal((3, 1, 20, 20)).astype(np.float32)
    ft = torch.tensor(f, device=hip, requires_grad=True)
    fx, fy = stencil_gradient(ft, 0.05)
    rx, ry = ns_step_ref.gradient(f, 0.05)
    np.testing.assert_array_equal(fx.detach().cpu().numpy(), rx)
    np.testing.assert_array_equal(fy.detach().cpu().numpy(), ry)
    gx = torch.randn_like(fx)
    gy = torch.randn_like(fy)
    (gf,) = torch.autograd.grad((fx * gx).sum() + (fy * gy).sum(), ft, create_graph=True)
    lhs = float((fx.detach().double() * gx.double()).sum() + (fy.detach().double() * gy.double()).sum())
    rhs = float((gf.double() * ft.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs))
    # d/df of sum(Dx(Dx f) * w) through the stencil twice == Dx^T Dx^T w
    w = torch.randn_like(fx)
    (g2,) = torch.autograd.grad((stencil_gradient(fx, 0.05)[0] * w).sum(), ft)
    from op.ns_step import gradient_adjoint
    z = torch.zeros_like(w)
    ref2 = gradient_adjoint(gradient_adjoint(w, z, 0.05), z, 0.05)
    np.testing.assert_allclose(g2.cpu().numpy(), ref2.cpu().numpy(), rtol=1e-5, atol=1e-3)


def test_pinn_stencil_residual_step_runs(hip):
    import losses
    from inverse.operators import InpaintOperator
    from models.ema import ExponentialMovingAverage
    d = load_golden("pinn_step.npz")
    c, m = _model(hip)
    c.training.pinn_residual = "stencil"
    em = ExponentialMovingAverage(m.parameters(), decay=c.model.ema_rate)
    state = dict(optimizer=(losses.get_optimizer(c, m.flownet.parameters()),
                            losses.get_optimizer(c, m.pressurenet.parameters(), 0.001)),
                 model=m, ema=em, step=50)
    step_fn = losses.get_pinn_step_fn(c, train=True, optimize_fn=losses.optimization_manager(c))
    T = lambda k: torch.tensor(d[k], device=hip)
    batch = (T("f1"), T("f2"), T("x").requires_grad_(), T("y").requires_grad_(),
             T("t").requires_grad_(), T("target"))
    loss, pinn_loss, data_loss = step_fn(state, InpaintOperator(mask=[T("mask")]), batch)
    assert torch.isfinite(loss) and float(pinn_loss) > 0 and state["step"] == 51


def test_ns_dynamics_bit_exact_vs_oracle(hip):
    """UKF NSDynamics.forward (reference ukf_utils.py:95-119) on the fused ns_step == the
    oracle's unpatch -> three C ns_step ops (compat quirk on) -> patch, bit for bit; the
    process covariance is the reference's 1e-8 I per state row."""
    from configs.pinn import pinn_pde
    from oracle import pinn_fd_ref
    from pinn_kalman.ukf_utils import NSDynamics, patch
    c = pinn_pde.get_config()
    assert c.kf.patch_size == 8 and c.data.image_size == 64
    rng = np.random.default_rng(4)
    B, n = 2, 64
    fields = np.concatenate([
        rng.uniform(0.1, 1.0, (B, 1, n, n)),
        rng.uniform(0.05, 0.5, (B, 2, n, n)) * rng.choice([-1, 1], (B, 2, n, n)),
        rng.normal(0, 0.01, (B, 1, n, n))], 1).astype(np.float32)
    states = patch(torch.from_numpy(fields), 8).numpy()
    dyn = NSDynamics(c)
    st, cov = dyn(torch.from_numpy(states).to(hip), None)
    ref_st, ref_cov = pinn_fd_ref.ns_dynamics(states, 8, 64)
    np.testing.assert_array_equal(st.cpu().numpy(), ref_st)
    np.testing.assert_array_equal(cov.cpu().numpy(), ref_cov)


def test_stencil_residual_matches_cpu_oracle(hip):
    """PINN.equation_mse_fd (the residual on the ns_step stencil kernel) == the float64
    oracle residual of the same fields and time derivatives (oracle/pinn_fd_ref.py);
    float32 vs float64: 1e-5 relative.  The fields and u_t / v_t come from the build's
    forward (checked against the reference elsewhere); the oracle recomputes every
    spatial derivative and the residual."""
    from oracle import pinn_fd_ref
    d = load_golden("pinn_fwd.npz")
    c, m = _model(hip)
    m.train()
    T = lambda k: torch.tensor(d[k], device=hip)
    x, y, t = (T(k).requires_grad_() for k in ("x", "y", "t"))
    flows, pres = m(T("f1"), T("f2"), x, y, t)
    h = float((x[:, :, :, -1] - x[:, :, :, 0]).mean()) / (x.shape[-1] - 1)
    for Re in (50.0, 1e7):
        val = m.equation_mse_fd(x, y, t, flows[-1], pres, Re, h=h)
        u = (m.mask_u * flows[-1]).sum(1, keepdim=True)
        v = (m.mask_v * flows[-1]).sum(1, keepdim=True)
        u_t = torch.autograd.grad(u.sum(), t, retain_graph=True)[0]
        v_t = torch.autograd.grad(v.sum(), t, retain_graph=True)[0]
        ref = pinn_fd_ref.fd_residual_mse(u.detach().cpu().numpy(), v.detach().cpu().numpy(),
                                          pres.detach().cpu().numpy(), u_t.cpu().numpy(),
                                          v_t.cpu().numpy(), h, Re)
        assert abs(float(val) - ref) <= 1e-5 * abs(ref), (Re, float(val), ref)


def test_pinn_step_hip_graph_replays_match_eager(hip):
    """get_pinn_step_fn(graph=True): the forward + residual derivatives + backward captured
    once and replayed for 8 steps (new batch and observation mask each step, optimizer steps
    and EMA in between) == the eager step from the same state on the configs[3] 64x64
    network: losses at every step and the final parameters / EMA (both run the same native
    kernels).  The observation noise (variance 0.01, as
    configured) comes from the same seeded generator in both runs: the graph step draws it
    into static buffers in the eager step's order."""
    import copy

    import losses
    from configs.pinn import pinn_pde
    from inverse.operators import InpaintOperator
    from models.ema import ExponentialMovingAverage
    from pinn_kalman.pinn import PINN
    c = pinn_pde.get_config()
    c.device = hip
    torch.manual_seed(0)
    m0 = PINN(c)
    B, n = 4, c.data.image_size
    g = torch.Generator().manual_seed(1)
    lin = torch.linspace(0.05, 1.0, n)
    batches = []
    for _ in range(8):
        f1, f2 = torch.rand(B, 1, n, n, generator=g), torch.rand(B, 1, n, n, generator=g)
        x = lin.view(1, 1, 1, n) + 0.01 * torch.rand(B, 1, n, n, generator=g)
        y = lin.view(1, 1, n, 1) + 0.01 * torch.rand(B, 1, n, n, generator=g)
        t = torch.randint(300, 900, (B,), generator=g).float()
        target = torch.randn(B, 3, n, n, generator=g) * 0.5
        batches.append([v.to(hip) for v in (f1, f2, x, y, t, target)])
    masks = [(torch.rand(1, 1, n, n, generator=g) > 0.3).float().expand(B, 1, n, n).contiguous()
             for _ in range(3)]  # CPU masks, as random_mask_source gives them

    def run(graph):
        m = copy.deepcopy(m0).to(hip)
        ema = ExponentialMovingAverage(m.parameters(), decay=c.model.ema_rate)
        state = dict(optimizer=(losses.get_optimizer(c, m.flownet.parameters()),
                                losses.get_optimizer(c, m.pressurenet.parameters(), 0.005)),
                     model=m, ema=ema, step=c.training.n_iters)
        step_fn = losses.get_pinn_step_fn(c, train=True, graph=graph,
                                          optimize_fn=losses.optimization_manager(c))
        op = InpaintOperator(mask=masks)
        out = []
        torch.manual_seed(123)
        for bt in batches:
            x, y, t = (v.clone().requires_grad_() for v in bt[2:5])
            out.append([float(v.detach()) for v in step_fn(state, op, (bt[0], bt[1], x, y, t, bt[5]))])
        if graph:
            assert step_fn.graph is not None
        return out, [p.detach().clone() for p in m.parameters()], \
            [p.clone() for p in ema.shadow_params], state["step"]
    lg, pg, eg, sg = run(True)
    le, pe, ee, se = run(False)
    assert sg == se
    lg, le = np.array(lg), np.array(le)  # columns: loss, pinn_loss, data_loss
    np.testing.assert_allclose(lg[:, [0, 2]], le[:, [0, 2]], rtol=1e-5, atol=0)
    # the residual term (~1e-5, sums of products of second derivatives) at the residual
    # tolerance of the fixtures above
    np.testing.assert_allclose(lg[:, 1], le[:, 1], rtol=2e-3, atol=0)
    # parameters: grid_sample's backward accumulates with atomics, so two eager runs differ
    # in the last bits too, and Adam turns the rounding noise of (mathematically) zero
    # gradients -- the conv biases in front of an InstanceNorm -- into sign-random moves of
    # up to lr per step in either run; the losses above are the tight check (each depends on
    # every earlier update), the parameters are bounded by 10 % of the 8 x 5e-3 an 8-step Adam
    # run can move a PressureNet parameter: a stale input, mask or gradient buffer moves
    # every parameter by O(lr) per step
    for a, b in zip(pg + eg, pe + ee):
        assert (a - b).abs().max().item() <= 4e-3


@pytest.mark.parametrize("k,ties", [(1, False), (2, False), (4, True)])
def test_spatial_embedding_native_matches_aten_chain(hip, k, ties):
    """op.embedding (the PINN nets' spatial embedding with its first and second derivatives as
    native launches) vs the reference's aten op chain (layers.get_spatial_embedding with the
    fused path off), k stacked copies with a per-copy max (layers.spatial_groups): forward bit
    for bit; then the residual's derivative pattern -- first derivatives w.r.t. x, y with
    create_graph, second derivatives w.r.t. x, y of a weighted sum of them, and that sum's
    gradient w.r.t. an upstream weight W (the path the final backward takes to the
    parameters) -- within 2e-5 of each tensor's max.  ties: the max repeated inside a copy
    (its gradient is shared evenly, as max() does)."""
    import models.layers as layers
    g = torch.Generator().manual_seed(10 * k + ties)
    B, n = 2 * k, 64
    lin = torch.linspace(0.05, 1.0, n)
    x0 = lin.view(1, 1, 1, n) + 0.01 * torch.rand(B, 1, n, n, generator=g)
    y0 = lin.view(1, 1, n, 1) + 0.01 * torch.rand(B, 1, n, n, generator=g)
    if ties:
        x0[0, 0, 3, 5] = x0[0, 0, 7, 9] = x0.view(k, -1)[0].max() + 0.01
    w0 = torch.randn(B, 1, n, n, generator=g)
    a0, b0 = torch.randn(B, 1, n, n, generator=g), torch.randn(B, 1, n, n, generator=g)
    x0, y0, w0, a0, b0 = (v.to(hip) for v in (x0, y0, w0, a0, b0))

    def run(fused):
        old = layers._SEMB_FUSED
        layers._SEMB_FUSED = fused
        try:
            x, y, W = (v.clone().requires_grad_() for v in (x0, y0, w0))
            with layers.spatial_groups(k):
                e = layers.get_spatial_embedding(x, y, 3.0, 2.5)
            gx, gy = torch.autograd.grad((e * W).sum(), (x, y), create_graph=True)
            l2 = (gx * a0 + gy * b0).sum()
            d2x, d2y, dW = torch.autograd.grad(l2, (x, y, W))
        finally:
            layers._SEMB_FUSED = old
        return [t.detach() for t in (e, gx, gy, d2x, d2y, dW)]
    fz, ref = run(True), run(False)
    assert torch.equal(fz[0], ref[0]), "forward not bit-identical"
    for name, a, b in zip(("gx", "gy", "d2x", "d2y", "dW"), fz[1:], ref[1:]):
        err = (a - b).abs().max().item() / b.abs().max().item()
        assert err <= 2e-5, f"{name}: {err:.3e}"

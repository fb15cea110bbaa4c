"""Both candidates of every timed kernel choice of op/conv.py against float64.

op.conv times two native kernels at six sites (`_pick_any`: f3, d3, w3, dsc, wsc, w2) on the
first eager call of a key and keeps the faster, so a test that merely calls conv3x3() checks
whichever kernel won on that machine.  Here every candidate of every site is forced
(tests/conv_pick.py) and compared with a float64 computation on the CPU of the fp32 inputs cast
to double: F.conv2d, torch.nn.grad.conv2d_input / conv2d_weight, or double autograd.  What
is pinned is the glue at each site -- argument order, the flip versus the adjoint, the bias
column and want_b, the residual tail and div, whose bias gradient a two-source launch returns.
Inputs and weights are seeded randn (no symmetric taps: a missing flip or transposition is an
O(1) error).  Every test asserts that the site it names was consulted, with two candidates;
tests/test_conv_pick_host.py shows the same from the library's predicates without a device.
(The dsc site: test_gpu_ops.py::test_conv2d_input_select_small_cin_candidates.)

Bounds.  First-order results keep the bound the igemm, Winograd and two-source kernel tests
use: 2e-5 * max(1, max|truth|).  The second-order and GroupNorm-prologue cases have no such
number; they allow max(2e-5 * scale, 2 x the error of the same construction on F.conv2d in fp32
on the device against the same truth) -- no worse than plain fp32 arithmetic up to a factor 2
(conftest.param_grads_vs_truth's convention).  Every error and bound goes to record_err.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_pick as cp
from conftest import record_err

pytestmark = pytest.mark.gpu

DIV = float(np.float32(cp.SQRT2))  # the kernels take div as a float


def _scale(truth):
    return max(1.0, float(truth.abs().max()))


def _check(what, got, truth, tol=None):
    """|got - truth| <= tol (default: the first-order bound), logged with its bound"""
    assert tuple(got.shape) == tuple(truth.shape), f"{what}: {tuple(got.shape)} vs {tuple(truth.shape)}"
    err = float((got.detach().double().cpu() - truth).abs().max())
    tol = 2e-5 * _scale(truth) if tol is None else tol
    record_err(f"conv_pick {what}", err, tol)
    print(f"conv_pick {what}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _filt(g, cout, cin, k=3):
    return _randn(g, cout, cin, k, k) / (cin * k * k) ** 0.5


# ------------------------------------------------------------------------------------ f3
@functools.lru_cache(maxsize=None)
def _f3_data(case):
    N, cin, cout, H, W = case
    g = torch.Generator().manual_seed(1000 + sum(case))
    x, w, b, skip = _randn(g, N, cin, H, W), _filt(g, cout, cin), _randn(g, cout), _randn(g, N, cout, H, W)
    y = F.conv2d(x.double(), w.double(), padding=1)
    yb = y + b.double().view(1, -1, 1, 1)
    return x, w, b, skip, {"plain": y, "bias": yb, "bias_skip": (skip.double() + yb) / DIV}


def _f3_args(hip, case, variant):
    x, w, b, skip, truth = _f3_data(case)
    bias = b.to(hip) if variant != "plain" else None
    sk = skip.to(hip) if variant == "bias_skip" else None
    key = ("f3", tuple(x.shape), tuple(w.shape), bias is not None, sk is not None)
    return (x.to(hip), w.to(hip), bias, sk, DIV if sk is not None else 1.0), key, truth[variant]


@pytest.mark.parametrize("candidate", [0, 1])
@pytest.mark.parametrize("variant", cp.F3_VARIANTS)
@pytest.mark.parametrize("case", cp.F3_CASES, ids=cp.case_id)
def test_f3_forward_winograd_and_igemm(hip, monkeypatch, case, variant, candidate):
    """conv._fwd_impl: Winograd with the fused bias / skip / div tail, and implicit GEMM followed
    by _residual_tail; (bias, skip) are part of the key, so the three variants are three keys."""
    from op import conv
    log = cp.forced(monkeypatch, {"f3": candidate})
    args, key, truth = _f3_args(hip, case, variant)
    got = conv._fwd_impl(*args)
    assert cp.reached(log, "f3") == [key] and len(log) == 1, log
    _check(f"f3[{candidate}] {case} {variant}", got, truth)


@pytest.mark.parametrize("candidate", [0, 1])
def test_f3_through_conv3x3(hip, monkeypatch, candidate):
    """the same site through the public conv3x3() (the padded-cout shape with the residual tail)"""
    from op import conv
    log = cp.forced(monkeypatch, {"f3": candidate})
    args, key, truth = _f3_args(hip, cp.F3_CASES[1], "bias_skip")
    got = conv.conv3x3(*args[:3], skip=args[3], div=args[4])
    assert cp.reached(log, "f3") == [key] and len(log) == 1, log
    _check(f"f3[{candidate}] conv3x3() {cp.F3_CASES[1]} bias_skip", got, truth)


def test_f3_boundary_image_above_the_limit_consults_nothing(hip, monkeypatch):
    from op import conv
    log = cp.forced(monkeypatch, {})
    for variant in cp.F3_VARIANTS:
        args, _, truth = _f3_args(hip, cp.F3_BOUNDARY, variant)
        _check(f"f3 boundary {cp.F3_BOUNDARY} {variant}", conv._fwd_impl(*args), truth)
    assert log == []


# ------------------------------------------------------------------------------------ d3
@functools.lru_cache(maxsize=None)
def _d3_data(case):
    N, c0, c1, H, W = case
    g = torch.Generator().manual_seed(2000 + sum(case))
    x, w = _randn(g, N, c0, H, W), _filt(g, c0, c1)
    truth = torch.nn.grad.conv2d_input((N, c1, H, W), w.double(), x.double(), padding=1)
    return x, w, truth


@pytest.mark.parametrize("candidate", [0, 1])
@pytest.mark.parametrize("case", cp.D3_CASES, ids=cp.case_id)
def test_d3_backward_data_flip_and_adjoint(hip, monkeypatch, case, candidate):
    """conv._fwd_ft_impl(x, w) = conv3x3(x, flip_t(w)): Winograd with the flip and transposition
    in its filter transform, and the implicit GEMM's adjoint (no flip), with Cin != Cout so the
    two cannot be exchanged unseen."""
    from op import conv
    log = cp.forced(monkeypatch, {"d3": candidate})
    x, w, truth = _d3_data(case)
    got = conv._fwd_ft_impl(x.to(hip), w.to(hip))
    assert cp.reached(log, "d3") == [("d3", tuple(x.shape), tuple(w.shape))] and len(log) == 1, log
    _check(f"d3[{candidate}] {case}", got, truth)


def test_d3_boundary_image_above_the_limit_consults_nothing(hip, monkeypatch):
    from op import conv
    log = cp.forced(monkeypatch, {})
    x, w, truth = _d3_data(cp.D3_BOUNDARY)
    _check(f"d3 boundary {cp.D3_BOUNDARY}", conv._fwd_ft_impl(x.to(hip), w.to(hip)), truth)
    assert log == []


# ------------------------------------------------------------------------------------ w3
@functools.lru_cache(maxsize=None)
def _w3_data(case):
    N, cin, cout, H, W = case
    g = torch.Generator().manual_seed(3000 + sum(case))
    x, gy = _randn(g, N, cin, H, W), _randn(g, N, cout, H, W)
    dw = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), gy.double(), padding=1)
    return x, gy, dw, gy.double().sum((0, 2, 3))


@pytest.mark.parametrize("candidate", [0, 1])
@pytest.mark.parametrize("want_b", [True, False])
@pytest.mark.parametrize("case", cp.W3_CASES, ids=cp.case_id)
def test_w3_weight_gradient_and_bias_column(hip, monkeypatch, case, want_b, candidate):
    """conv._wgrad_impl: the Winograd weight gradient and the implicit GEMM's, both with the
    bias column; db is handed out with want_b only."""
    from op import conv
    log = cp.forced(monkeypatch, {"w3": candidate})
    x, gy, dw_t, db_t = _w3_data(case)
    wshape = tuple(dw_t.shape)
    dw, db = conv._wgrad_impl(x.to(hip), gy.to(hip), wshape, want_b)
    assert cp.reached(log, "w3") == [("w3", tuple(x.shape), wshape)] and len(log) == 1, log
    _check(f"w3[{candidate}] {case} dw (want_b={want_b})", dw, dw_t)
    if want_b:
        _check(f"w3[{candidate}] {case} db", db, db_t)
    else:
        assert db is None


def test_w3_boundary_large_image_full_cout_blocks_consults_nothing(hip, monkeypatch):
    from op import conv
    log = cp.forced(monkeypatch, {})
    x, gy, dw_t, db_t = _w3_data(cp.W3_BOUNDARY)
    dw, db = conv._wgrad_impl(x.to(hip), gy.to(hip), tuple(dw_t.shape), True)
    assert log == []
    _check(f"w3 boundary {cp.W3_BOUNDARY} dw", dw, dw_t)
    _check(f"w3 boundary {cp.W3_BOUNDARY} db", db, db_t)


# ----------------------------------------------------------------------------------- wsc
@functools.lru_cache(maxsize=None)
def _wsc_data(case):
    N, cin, cout, H, W, K = case
    g = torch.Generator().manual_seed(4000 + sum(case))
    x, gy = _randn(g, N, cin, H, W), _randn(g, N, cout, H, W)
    dw = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, K, K), gy.double(), padding=K // 2)
    return x, gy, dw, gy.double().sum((0, 2, 3))


@pytest.mark.parametrize("candidate", [0, 1])
@pytest.mark.parametrize("bias_grad", [True, False])
@pytest.mark.parametrize("case", cp.WSC_CASES, ids=cp.case_id)
def test_wsc_small_cout_weight_gradient(hip, monkeypatch, case, bias_grad, candidate):
    """conv.conv2d_weight_select into Cout <= 4: the streaming kernel and the implicit GEMM"""
    from op import conv
    log = cp.forced(monkeypatch, {"wsc": candidate})
    x, gy, dw_t, db_t = _wsc_data(case)
    K = case[5]
    wshape = tuple(dw_t.shape)
    dw, db = conv.conv2d_weight_select(x.to(hip), wshape, gy.to(hip), 1, K // 2, bias_grad)
    key = ("wsc", tuple(x.shape), wshape, (1, 1), (K // 2, K // 2), bias_grad)
    assert cp.reached(log, "wsc") == [key] and len(log) == 1, log
    _check(f"wsc[{candidate}] {case} dw (bias_grad={bias_grad})", dw, dw_t)
    if bias_grad:
        _check(f"wsc[{candidate}] {case} db", db, db_t)
    else:
        assert db is None


def test_wsc_and_dsc_boundaries_five_channels_consult_nothing(hip, monkeypatch):
    from op import conv
    log = cp.forced(monkeypatch, {})
    x, gy, dw_t, db_t = _wsc_data(cp.WSC_BOUNDARY)
    dw, db = conv.conv2d_weight_select(x.to(hip), tuple(dw_t.shape), gy.to(hip), 1, 1, True)
    _check(f"wsc boundary {cp.WSC_BOUNDARY} dw", dw, dw_t)
    _check(f"wsc boundary {cp.WSC_BOUNDARY} db", db, db_t)
    N, cin, cout, H, W = cp.DSC_BOUNDARY
    g = torch.Generator().manual_seed(4500)
    w, gy = _filt(g, cout, cin), _randn(g, N, cout, H, W)
    truth = torch.nn.grad.conv2d_input((N, cin, H, W), w.double(), gy.double(), padding=1)
    got = conv.conv2d_input_select((N, cin, H, W), w.to(hip), gy.to(hip), 1, 1)
    _check(f"dsc boundary {cp.DSC_BOUNDARY}", got, truth)
    assert log == []


# ------------------------------------------------------------------------------------ w2
@functools.lru_cache(maxsize=None)
def _w2_data(name):
    _, kind, how, N1, N2, cin, cout, H, W, k, s, p = next(c for c in cp.W2_CASES if c[0] == name)
    g = torch.Generator().manual_seed(5000 + N1 + 3 * N2 + cin + cout + H + k)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x1, x2 = _randn(g, N1, cin, H, W), _randn(g, N2, cin, H, W)
    g1, g2 = _randn(g, N1, cout, Ho, Wo), _randn(g, N2, cout, Ho, Wo)
    wshape = (cout, cin, k, k)
    dw = (torch.nn.grad.conv2d_weight(x1.double(), wshape, g1.double(), stride=s, padding=p)
          + torch.nn.grad.conv2d_weight(x2.double(), wshape, g2.double(), stride=s, padding=p))
    return kind, wshape, (x1, g1, x2, g2), dw, g1.double().sum((0, 2, 3))


def _w2_params():
    out = []
    for case in cp.W2_CASES:
        name, nested = case[0], cp.W2_NESTED[case[0]]
        for c in cp.W2_CANDIDATES.get(name, (0, 1)):
            for n in ((0, 1) if (c == 1 and nested) else (None,)):
                out.append(pytest.param(name, c, n, id=f"{name}-w2_{c}" + ("" if n is None else f"-{nested}_{n}")))
    return out


@pytest.mark.parametrize("name,candidate,nested", _w2_params())
def test_w2_two_sources_in_one_launch_and_in_two(hip, monkeypatch, name, candidate, nested):
    """conv._wgrad_pairs: one two-source launch (Winograd or implicit GEMM), and two launches
    plus an add (which reach w3 / wsc in turn: both of its values).  Unequal sources, the bias
    flag on the first pair only: dw is the sum over both, db the first source's."""
    from op import conv
    kind, wshape, (x1, g1, x2, g2), dw_t, db_t = _w2_data(name)
    tag = cp.W2_NESTED[name]
    picks = {"w2": candidate}
    if nested is not None:
        picks[tag] = nested
    log = cp.forced(monkeypatch, picks)
    d = [t.to(hip) for t in (x1, g1, x2, g2)]
    with torch.no_grad():
        dw, db = conv._wgrad_pairs(kind, wshape, [(d[0], d[1], True), (d[2], d[3], False)])
    key = ("w2", kind[0], tuple(x1.shape), tuple(x2.shape), tuple(g1.shape), wshape,
           kind[1] if kind[0] == "gen" else None, True)
    assert cp.reached(log, "w2") == [key], log
    if nested is None:
        assert len(log) == 1, log
    else:  # one nested choice per source, the bias with the first
        keys = cp.reached(log, tag)
        assert [k[1] for k in keys] == [tuple(x1.shape), tuple(x2.shape)] and len(log) == 3, log
        if tag == "wsc":
            assert [k[-1] for k in keys] == [True, False]
    what = f"w2[{candidate}] {name}" + ("" if nested is None else f" {tag}[{nested}]")
    _check(what + " dw", dw, dw_t)
    _check(what + " db", db, db_t)


def test_w2_pairs_of_different_spatial_shape_consult_nothing(hip, monkeypatch):
    from op import conv
    log = cp.forced(monkeypatch, {})
    g = torch.Generator().manual_seed(5900)
    wshape = (32, 49, 3, 3)
    x1, g1 = _randn(g, 2, 49, 8, 8), _randn(g, 2, 32, 8, 8)
    x2, g2 = _randn(g, 3, 49, 4, 8), _randn(g, 3, 32, 4, 8)
    truth = (torch.nn.grad.conv2d_weight(x1.double(), wshape, g1.double(), padding=1)
             + torch.nn.grad.conv2d_weight(x2.double(), wshape, g2.double(), padding=1))
    with torch.no_grad():
        dw, db = conv._wgrad_pairs(("3x3",), wshape, [(x1.to(hip), g1.to(hip), True),
                                                     (x2.to(hip), g2.to(hip), False)])
    assert log == []
    _check("w2 different spatial shapes dw", dw, truth)
    _check("w2 different spatial shapes db", db, g1.double().sum((0, 2, 3)))


# ------------------------------------------------- second order: shared truth and fp32 error
def _aten_bound(name, build):
    """{i: (truth, tol)} for the tensors build(device, dtype, conv) returns: truth from float64
    on the CPU, tol = max(2e-5 * scale, 2 x the error of the same construction on F.conv2d in
    fp32 on the device).  Computed once per name."""
    if name not in _BOUNDS:
        dev = torch.device("cuda:0")
        truth = [None if t is None else t.detach() for t in build("cpu", torch.float64, _aten_conv)]
        aten = build(dev, torch.float32, _aten_conv)
        out = []
        for i, (t, a) in enumerate(zip(truth, aten)):
            if t is None:
                out.append(None)
                continue
            e = float((a.detach().double().cpu() - t).abs().max())
            tol = max(2e-5 * _scale(t), 2 * e)
            record_err(f"conv_pick {name} fp32 F.conv2d [{i}]", e, tol)
            out.append((t, tol))
        _BOUNDS[name] = out
    return _BOUNDS[name]


_BOUNDS = {}


def _aten_conv(x, w, b):
    return F.conv2d(x, w, b, padding=1)


@functools.lru_cache(maxsize=None)
def _second_inputs():
    N, cin, cout, H, W = cp.SECOND_ORDER_CASE
    g = torch.Generator().manual_seed(6000)
    return (_randn(g, N, cin, H, W), _filt(g, cout, cin), _randn(g, cout),
            _randn(g, N, cout, H, W), _randn(g, N, cin, H, W))


def _second(dev, dtype, conv_fn):
    """the construction of test_conv3x3_double_backward_any_shape: gradients w.r.t. (x, w, b)
    of a function of (dL/dx, dL/dw) -- f3, d3 and w3 in one graph"""
    x0, w0, b0, go, v = (t.to(dev, dtype) for t in _second_inputs())
    x, w, b = x0.requires_grad_(), w0.requires_grad_(), b0.requires_grad_()
    y = conv_fn(torch.tanh(x), w, b)
    gx, gw = torch.autograd.grad(y, (x, w), go, create_graph=True)
    return (gx, gw) + torch.autograd.grad((gx * v).sum() + (gw * gw).sum() + (gx * gx).sum(),
                                          (x, w, b), allow_unused=True)


@pytest.mark.parametrize("w3", [0, 1])
@pytest.mark.parametrize("d3", [0, 1])
@pytest.mark.parametrize("f3", [0, 1])
def test_all_sites_under_autograd_to_second_order(hip, monkeypatch, f3, d3, w3):
    """conv3x3() differentiated twice: forward (f3), backward-data (d3) and the weight gradient
    (w3) and their own derivatives in one graph, for all eight combinations of the choices."""
    from op import conv
    bounds = _aten_bound("second order", _second)
    log = cp.forced(monkeypatch, {"f3": f3, "d3": d3, "w3": w3})
    got = _second(hip, torch.float32, lambda x, w, b: conv.conv3x3(x, w, b))
    for tag in ("f3", "d3", "w3"):
        assert cp.reached(log, tag), (tag, log)
    for i, (name, a, tb) in enumerate(zip(("dL/dx", "dL/dw", "d2/dx", "d2/dw", "d2/db"), got, bounds)):
        if tb is None:  # the bias does not reach (dL/dx, dL/dw)
            assert i == 4 and (a is None or float(a.abs().max()) == 0.0)
            continue
        _check(f"second order f3={f3} d3={d3} w3={w3} {name}", a, tb[0], tb[1])


# -------------------------------------------------------------- GroupNorm + SiLU prologue
@functools.lru_cache(maxsize=None)
def _gn_inputs():
    N, cin, cout, H, W = cp.GN_CASE
    g = torch.Generator().manual_seed(7000)
    return (_randn(g, N, cin, H, W) * 1.5 + 0.3, _randn(g, N, cin) * 0.5, 1 + 0.2 * _randn(g, cin),
            0.2 * _randn(g, cin), _filt(g, cout, cin), _randn(g, cout), _randn(g, N, cout, H, W))


def _gn(dev, dtype, conv_fn):
    """conv_fn(x, bias_nc, gamma, beta, w, b) and its gradients for the output gradient go"""
    *leaves, go = (t.to(dev, dtype) for t in _gn_inputs())
    leaves = [t.requires_grad_() for t in leaves]
    y = conv_fn(*leaves)
    return (y,) + torch.autograd.grad(y, leaves, go)


def _gn_aten(x, bnc, gamma, beta, w, b):
    h = F.group_norm(x + bnc[:, :, None, None], cp.GN_GROUPS, gamma, beta, 1e-6)
    return F.conv2d(F.silu(h), w, b, padding=1)


@pytest.mark.parametrize("w3", [0, 1])
@pytest.mark.parametrize("d3", [0, 1])
def test_gn_silu_conv3x3_ad_backward_candidates(hip, monkeypatch, d3, w3):
    """gn_silu_conv3x3_ad (GroupNorm + SiLU in the Winograd conv's input load): the forward has
    no choice; its backward reaches d3 (the activation's gradient) and, at small images, w3 on
    the materialised activation.  Output and the gradients of x, bias_nc, gamma, beta, weight
    and bias against the double composition."""
    from op import conv
    bounds = _aten_bound("gn_silu", lambda dev, dt, _: _gn(dev, dt, _gn_aten))
    log = cp.forced(monkeypatch, {"d3": d3, "w3": w3})
    got = _gn(hip, torch.float32, lambda x, bnc, gamma, beta, w, b: conv.gn_silu_conv3x3_ad(
        x, cp.GN_GROUPS, gamma, beta, 1e-6, w, b, bias_nc=bnc))
    assert cp.reached(log, "d3") and cp.reached(log, "w3") and not cp.reached(log, "f3"), log
    names = ("y", "dx", "dbias_nc", "dgamma", "dbeta", "dw", "db")
    for name, a, (t, tol) in zip(names, got, bounds):
        _check(f"gn_silu d3={d3} w3={w3} {name}", a, t, tol)


# --------------------------------------------------------------- deferred_weight_grads()
@functools.lru_cache(maxsize=None)
def _net_inputs():
    g = torch.Generator().manual_seed(8000)
    return (_randn(g, 2, 32, 8, 16), _filt(g, 64, 32), 0.5 * _randn(g, 64), _filt(g, 32, 64),
            0.5 * _randn(g, 32), _randn(g, 2, 32, 8, 16))


def _net(dev, dtype, conv_fn, around_backward=None):
    """.grad of the four parameters of a two-conv net after the backward of a loss of the
    output and of the input gradient (create_graph): every weight is reached twice, through its
    forward conv and through the backward-data conv the first pass recorded."""
    import contextlib
    x0, w1, b1, w2, b2, go = (t.to(dev, dtype) for t in _net_inputs())
    x = x0.requires_grad_()
    params = [t.requires_grad_() for t in (w1, b1, w2, b2)]
    h = conv_fn(torch.tanh(conv_fn(x, params[0], params[1])), params[2], params[3])
    gx, = torch.autograd.grad((h * go).sum(), x, create_graph=True)
    loss = (gx ** 2).sum() + (h ** 2).sum()
    with (around_backward() if around_backward else contextlib.nullcontext()):
        loss.backward(inputs=params)
    return tuple(p.grad for p in params)


@pytest.mark.parametrize("other", [0, 1])
@pytest.mark.parametrize("w2", [0, 1])
def test_w2_through_deferred_weight_grads(hip, monkeypatch, w2, other):
    """the public deferred_weight_grads() around loss.backward(): both weights' two pairs run as
    one two-source launch (w2 = 0) or as two launches and an add (w2 = 1); `other` is the
    candidate of f3 / d3 / w3 along the way."""
    from op import conv
    bounds = _aten_bound("two-conv net", lambda dev, dt, fn: _net(dev, dt, fn))
    log = cp.forced(monkeypatch, {"f3": other, "d3": other, "w3": other, "w2": w2})
    got = _net(hip, torch.float32, lambda x, w, b: conv.conv3x3(x, w, b), conv.deferred_weight_grads)
    keys = cp.reached(log, "w2")
    assert sorted(k[5] for k in keys) == [(32, 64, 3, 3), (64, 32, 3, 3)], log
    assert all(k[1] == "3x3" and k[-1] is True for k in keys)
    assert bool(cp.reached(log, "w3")) == (w2 == 1)  # only the separate launches get there
    for name, a, (t, tol) in zip(("w1", "b1", "w2", "b2"), got, bounds):
        _check(f"deferred w2={w2} f3/d3/w3={other} {name}.grad", a, t, tol)

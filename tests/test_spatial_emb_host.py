"""tests/emb_ref.py -- the float64 truth of the spatial-embedding tests -- checked on the CPU
against things that do not share its autograd: central finite differences, an explicit loop
over the copies with a hand-built evenly shared maximum, and models.layers' aten chain."""
import pytest
import torch

import emb_ref


def _f64(case):
    return tuple(v.double() for v in emb_ref.inputs(*case))


@pytest.mark.parametrize("omega,s", emb_ref.OMEGAS)
def test_chain_first_derivatives_match_finite_differences(omega, s):
    """gx, gy of the float64 chain vs central differences (h = 1e-6) of the float64 forward,
    L = sum(e W), at a 16 x 16 case of two copies: 1e-6 of max|g|.  (Truncation h^2 w^3 / 6 and
    rounding 1e-16 |L| / h are both below 1e-8 of it at omega = 100.)  The probes lie
    off the argmax sets: moving an argmax element moves the maximum for its whole copy, which
    a one-element difference quotient of a tied set does not describe."""
    k = 2
    x, y, W, a, b = _f64((k, 1, 16, 16, 11, "jitter"))
    _, gx, gy, _, _, _ = emb_ref.chain(x, y, W, a, b, k, omega, s)
    mask = emb_ref.argmax_mask(x, y, k).reshape(-1)
    probes = [0, 17, 100, 255, 256, 300, 391, 500]
    assert not mask[probes].any()
    h = 1e-6

    def L(xx, yy):
        return (emb_ref.forward(xx, yy, k, omega, s) * W).sum().item()
    for v, gv, name in ((x, gx, "gx"), (y, gy, "gy")):
        for i in probes:
            d = torch.zeros_like(v).reshape(-1)
            d[i] = h
            d = d.view_as(v)
            fd = ((L(x + d, y) - L(x - d, y)) if name == "gx" else
                  (L(x, y + d) - L(x, y - d))) / (2 * h)
            err = abs(fd - gv.reshape(-1)[i].item()) / gv.abs().max().item()
            assert err <= 1e-6, f"{name}[{i}]: {err:.3e}"


@pytest.mark.parametrize("case", [(4, 1, 16, 16, 12, "column_ties"), (2, 3, 16, 16, 13, "column_ties"),
                                  (3, 2, 16, 16, 14, "jitter")])
def test_chain_copy_max_and_tie_sharing_match_explicit_loop(case):
    """The stacked float64 chain vs a Python loop over the copies in which the maximum is built
    by hand as the mean of the tied elements (so autograd shares its gradient evenly by
    construction, whatever amax's backward does): all six tensors to 1e-12 of their maximum.
    Also pins the tie counts the cases are meant to have."""
    k, cb, h, w = case[:4]
    omega, s = 3.0, 2.5
    x, y, W, a, b = _f64(case)
    got = emb_ref.chain(x, y, W, a, b, k, omega, s)
    outs = []
    for c in range(k):
        sl = slice(c * cb, (c + 1) * cb)
        xc, yc, Wc = (v[sl].clone().requires_grad_() for v in (x, y, W))
        tx, ty = xc.detach() == xc.max().item(), yc.detach() == yc.max().item()
        assert int(tx.sum()) == (cb * h if case[5] == "column_ties" else 1) and int(ty.sum()) == 1
        mx, my = xc[tx].sum() / tx.sum(), yc[ty].sum() / ty.sum()
        e = (torch.sin(omega * torch.sqrt(xc ** 2 + yc ** 2))
             + torch.sin(omega * torch.sqrt((mx - xc) ** 2 + (my - yc) ** 2))) / s
        gx, gy = torch.autograd.grad((e * Wc).sum(), (xc, yc), create_graph=True)
        d2 = torch.autograd.grad((gx * a[sl] + gy * b[sl]).sum(), (xc, yc, Wc))
        outs.append([t.detach() for t in (e, gx, gy) + tuple(d2)])
    for i, name in enumerate(("e", "gx", "gy", "d2x", "d2y", "dW")):
        ref = torch.cat([o[i] for o in outs])
        err = (got[i] - ref).abs().max().item() / ref.abs().max().item()
        assert err <= 1e-12, f"{name}: {err:.3e}"
    # the copies' maxima differ grossly (a kernel using copy 0's would be far off)
    m = emb_ref.copy_max(x, k).reshape(-1)
    assert all(m[c + 1] >= 1.15 * m[c] for c in range(k - 1))


@pytest.mark.parametrize("k,case", [(1, (1, 2, 16, 16, 15, "jitter")), (1, (1, 3, 16, 16, 16, "column_ties")),
                                    (2, (2, 1, 16, 16, 17, "jitter")), (2, (2, 2, 16, 16, 18, "column_ties"))])
@pytest.mark.parametrize("omega,s", emb_ref.OMEGAS)
def test_layers_aten_chain_equals_ref_chain_bit_for_bit(k, case, omega, s):
    """models.layers.get_spatial_embedding on CPU tensors (the aten chain) == emb_ref.chain in
    float32, all six tensors bit for bit, for one copy and for two under spatial_groups."""
    import models.layers as layers
    x0, y0, W0, a, b = emb_ref.inputs(*case)
    ref = emb_ref.chain(x0, y0, W0, a, b, k, omega, s)
    x, y, W = (v.clone().requires_grad_() for v in (x0, y0, W0))
    with layers.spatial_groups(k):
        e = layers.get_spatial_embedding(x, y, omega, s)
    gx, gy = torch.autograd.grad((e * W).sum(), (x, y), create_graph=True)
    d2 = torch.autograd.grad((gx * a + gy * b).sum(), (x, y, W))
    for name, t, r in zip(("e", "gx", "gy", "d2x", "d2y", "dW"), (e, gx, gy) + tuple(d2), ref):
        assert torch.equal(t.detach(), r), name


def test_inputs_refuses_nan_truth(monkeypatch):
    """inputs() asserts its truth finite: an exact mesh in both coordinates puts both maxima on
    one element (r2 = 0) and must be refused, not returned."""
    real = torch.rand
    monkeypatch.setattr(torch, "rand", lambda *a, **k: 0.0 * real(*a, **k))
    emb_ref.inputs.cache_clear()
    try:
        with pytest.raises(AssertionError, match="not finite"):
            emb_ref.inputs(1, 1, 16, 16, 99, "jitter")
    finally:
        emb_ref.inputs.cache_clear()

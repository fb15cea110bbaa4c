"""csrc/group_norm.hip -- every entry point, every dispatch path -- against the float64 truth of
tests/group_norm_ref.py: the forward and backward (resident rungs, split paths, the float4 and
the scalar form, misaligned views, an empty batch), the (s, t) tables from a statistics pass and
from producer partials, chunk_partials, affine_silu and the parameter-gradient reduction.

Tolerance rule.  err(t) = max|t - truth| / max|truth| per tensor (the absolute error where the
truth is identically zero).  E = the largest such error of the reference's own float32 arithmetic
(group_norm_ref.fp32_chain: torch.native_group_norm, F.silu and autograd on the CPU) over the
tensors of a group -- forward; statistics and tables; dx with its plane sums; the parameter
gradients -- for the variant; every native error must be <= FACTOR x E, FACTOR = 8.  The factor is twice the worst ratio of a CPU float32
emulation of the kernels' documented summation orders to E (3.43: the statistics of g-plain,
where E = 6e-8 is one rounding), rounded up to the next of 2, 4, 8
(test_group_norm_ref_host.py).  E is 4e-8...5e-7 for the well-conditioned variants.
On an MI355X the worst native / E was 3.43 as well (mean saved by the forward of g-plain: the
emulation reproduces that sum bit for bit), 2.91 forward (y of l-plain-nobnc),
2.28 input gradients (d_bnc of e-plain), 2.78 parameter gradients (dgamma of e-plain, LDS-atomic
mode), 1.94 tables from partials (t of (6, 50, 64) with bias), 1.04 chunk partials, 3.00
param_grads (dgamma at N = 9, C = 1: one sum of nine terms).
chunk_partials and param_grads go by the same rule, with torch's float32 mean / sum over the same
numbers as the chain (group_norm_ref.chunk_reference, param_grads_reference), and are held to
the worst-case bound of float32 summation as well.  affine_silu is bounded per element, see
test_affine_silu.
"""
import functools

import pytest
import torch

import group_norm_ref as R
from conftest import record_err

pytestmark = pytest.mark.gpu

FACTOR = R.FACTOR
VIDS = [R.variant_id(v) for v in R.VARIANTS]
DEV = "cuda:0"


def _off1(t):
    """t on the device as a contiguous view one float into its storage (no 16-byte alignment)."""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _p(t):
    return None if t is None else t.data_ptr()


def _native(v):
    """Every tensor the variant produces on the native kernels, as a dict over R.GROUPS' names."""
    from op import norm_act
    from op._lib import check, lib, stream_ptr
    d, G, act, bwd, aligned = R.variant_inputs(v)
    dev = torch.device(DEV)
    big = (lambda t: None if t is None else t.to(dev)) if aligned else \
        (lambda t: None if t is None else _off1(t))
    x, dy, addend = big(d["x"]), big(d["dy"]), big(d["addend"])
    bnc, gamma, beta = (None if d[k] is None else d[k].to(dev) for k in ("bnc", "gamma", "beta"))
    N, C = x.shape[:2]
    HW = x[0, 0].numel()
    out = {}
    y = norm_act.group_norm_act_f(x.requires_grad_(), G, gamma, beta, R.EPS, act, bnc)
    out["y"] = y.detach()
    sx, _, _, _, mean, rstd = y.grad_fn.saved_tensors
    assert sx.data_ptr() == x.data_ptr()
    out["mean_saved"], out["rstd_saved"] = mean, rstd
    x = x.detach()
    ss, out["mean"], out["rstd"] = norm_act.group_norm_affine_stats(x, G, gamma, beta, R.EPS, bnc)
    out["s"], out["t"] = ss[..., 0], ss[..., 1]
    # the wrapper, as autograd calls it
    affine = gamma is not None
    want_bnc = bnc is not None and bwd in ("full", "add_bnc")
    want_p = affine and bwd != "dx"
    dx, d_bnc, dw, dbeta = norm_act.group_norm_act_backward(
        dy, x, bnc, gamma, beta, mean, rstd, G, act, want_bnc, want_p, want_p, addend=addend)
    assert (d_bnc is None) == (not want_bnc) and (dw is None) == (dbeta is None) == (not want_p)
    out["dx"] = dx
    out.update({k: t for k, t in (("d_bnc", d_bnc), ("dgamma", dw), ("dbeta", dbeta))
                if t is not None})
    # the kernel itself, the way the wrapper calls it: the addend fused, the per-sample partials
    dxf = torch.empty_like(x)
    dg = torch.full((N, C), float("nan"), device=dev) if want_p else None
    db = torch.full((N, C), float("nan"), device=dev) if want_p else None
    ws = norm_act._ws(N, C, HW, G, dev)
    check(lib.bpk_group_norm_bwd_add_f32(
        dy.data_ptr(), x.data_ptr(), _p(bnc), _p(gamma), _p(beta), mean.data_ptr(),
        rstd.data_ptr(), _p(addend), dxf.data_ptr(), _p(dg), _p(db), _p(ws), N, C, HW, G, act,
        stream_ptr(dev)), "group_norm_bwd_add")
    out["dx_fused"] = dxf
    if want_p:
        out["dgamma_nc"], out["dbeta_nc"] = dg, db
    torch.cuda.synchronize()
    return out


_eval = functools.lru_cache(maxsize=None)(_native)


@pytest.mark.parametrize("v", R.VARIANTS, ids=VIDS)
def test_against_float64_truth(hip, v):
    """Forward, statistics and table, and every gradient of the variant by the module's rule
    (all tensors checked before failing)."""
    _, truth, chain = R.reference(v)
    native = _eval(v)
    E = R.yardsticks(truth, chain)
    what, bad = R.variant_id(v), []
    _, _, _, bnc, affine, bwd = v
    want = {"y", "mean", "rstd", "s", "t", "mean_saved", "rstd_saved", "dx", "dx_fused"}
    want |= {"d_bnc"} if bnc and bwd in ("full", "add_bnc") else set()
    want |= {"dgamma", "dbeta", "dgamma_nc", "dbeta_nc"} if affine and bwd != "dx" else set()
    assert set(native) == want
    for grp, names in R.groups_of(truth).items():
        for k in names:
            if k not in want:
                continue
            assert 0 < E[grp] < R.E_CEILING
            assert native[k].shape == truth[k].shape, k
            en = R.err(native[k], truth[k])
            print(f"{what} {k}: native {en:.3e} E {E[grp]:.3e} ratio {en / E[grp]:.2f}")
            record_err(f"group_norm {what} {k} native vs float64", en, FACTOR * E[grp])
            if not en <= FACTOR * E[grp]:
                bad.append(f"{k}: {en:.3e} > {FACTOR} x {E[grp]:.3e}")
    assert not bad, f"{what}: {bad}"
    if v[1] == "constant":  # rstd = eps^-1/2 = 1024 there, exactly (and y = beta without act)
        cpg = truth["y"].shape[1] // truth["mean"].shape[1]
        assert torch.equal(native["rstd_saved"][:, 0].cpu(), torch.full((truth["y"].shape[0],), 1024.0))
        assert torch.equal(native["rstd"][:, 0].cpu(), torch.full((truth["y"].shape[0],), 1024.0))
        if v[2] == 0:
            assert torch.equal(native["y"][:, :cpg].double().cpu(), truth["y"][:, :cpg])


@pytest.mark.parametrize("case", ["d", "g", "h", "i", "j", "m"])
def test_run_to_run_bit_identical(hip, case):
    """Slice / segment / split modes sum in a fixed order: a second evaluation gives the same bits
    in every tensor.  (Not asserted for c and e: LDS-atomic mode is order-dependent.)"""
    v = R._v(case)
    first, again = _eval(v), _native(v)
    assert first.keys() == again.keys()
    for k in first:
        assert torch.equal(first[k], again[k]), k


def test_empty_batch(hip):
    """N = 0: empty outputs of the right shapes, zero parameter gradients, no launch error."""
    from op import norm_act
    N, C, G = 0, 8, 4
    x = torch.empty(N, C, 4, 4, device=hip).requires_grad_()
    bnc, gamma, beta = (torch.randn(s, device=hip) for s in ((N, C), (C,), (C,)))
    y = norm_act.group_norm_act_f(x, G, gamma, beta, R.EPS, 1, bnc)
    assert y.shape == x.shape
    mean, rstd = y.grad_fn.saved_tensors[4:]
    assert mean.shape == rstd.shape == (N, G)
    ss, m2, r2 = norm_act.group_norm_affine_stats(x.detach(), G, gamma, beta, R.EPS, bnc)
    assert ss.shape == (N, C, 2) and m2.shape == r2.shape == (N, G)
    dx, d_bnc, dw, db = norm_act.group_norm_act_backward(
        torch.empty_like(y), x.detach(), bnc, gamma, beta, mean, rstd, G, 1, True, True, True)
    assert dx.shape == x.shape and d_bnc.shape == (N, C)
    assert torch.equal(dw, torch.zeros(C, device=hip)) and torch.equal(db, torch.zeros(C, device=hip))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ partial statistics
def _sum_bound(terms, dim):
    """The error bound of a float32 sum of n terms in any order: (n - 1) 2^-24 sum|terms| (first
    order; 1.01 x for the higher ones), per output element, float64."""
    n = terms.shape[dim]
    return 1.01 * (n - 1) * 2.0 ** -24 * terms.double().abs().sum(dim)


@pytest.mark.parametrize("shape,mode", R.CHUNK_CASES,
                         ids=["-".join(map(str, sh)) + "-" + m for sh, m in R.CHUNK_CASES])
def test_chunk_partials(hip, shape, mode):
    """ensure_gn_partials / bpk_group_norm_chunk_partials_f32: (mean, M2) of every run of 128
    pixels against float64 by the module's rule, E from torch's float32 mean and sum((x - m)^2)
    of the same runs.  3 x 1 x 128: three chunks, a block whose fourth wave exits.  Also within the
    worst-case bounds: the mean that of a 128-term float32 sum; M2 -- sum (x - m')^2 about the
    float32 mean m' = m + e is M2 + 128 e^2 exactly, and the float32 evaluation adds one rounding
    of x - m' (entering twice), one of the square and the 128-term sum's -- relative to
    sum (|x - m| + |e|)^2."""
    from op.conv import ensure_gn_partials, gn_partials
    N, C, H, W = shape
    x, truth, chain, _ = R.chunk_reference(shape, mode)
    xg = x.to(hip)
    assert gn_partials(xg) is None
    part, Rr, cnt = ensure_gn_partials(xg)
    assert (Rr, cnt) == (H * W // 128, 128) and part.shape == (N, C, Rr, 2)
    assert gn_partials(xg)[0] is part
    got = part.double().cpu()
    E = max(R.err(chain[..., i], truth[..., i]) for i in (0, 1))
    assert 0 < E < R.E_CEILING
    bad = []
    for i, name in enumerate(("mean", "M2")):
        en = R.err(got[..., i], truth[..., i])
        print(f"chunk_partials {shape} {mode} {name}: native {en:.3e} E {E:.3e} ratio {en / E:.2f}")
        record_err(f"group_norm chunk_partials {shape} {mode} {name} native vs float64", en,
                   FACTOR * E)
        if not en <= FACTOR * E:
            bad.append(f"{name}: {en:.3e} > {FACTOR} x {E:.3e}")
    assert not bad, bad
    runs = x.double().reshape(N, C, Rr, 128)
    e_mean = (got[..., 0] - truth[..., 0]).abs()
    b_mean = _sum_bound(runs, 3) / 128 + 2.0 ** -24 * truth[..., 0].abs()
    sq = ((runs - truth[..., 0, None]).abs() + b_mean[..., None]) ** 2
    b_m2 = _sum_bound(sq, 3) + 1.01 * 3 * 2.0 ** -24 * sq.sum(3) + 128 * b_mean ** 2
    e_m2 = (got[..., 1] - truth[..., 1]).abs()
    assert (e_mean <= b_mean).all() and (e_m2 <= b_m2).all()


def _gn(C, G, gamma, beta):
    gn = torch.nn.GroupNorm(G, C, eps=R.EPS).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(gamma), gn.bias.copy_(beta)
    return gn


@pytest.mark.parametrize("pc", R.PART_CASES, ids=[f"{a}-{b}-{c}" for a, b, c in R.PART_CASES])
@pytest.mark.parametrize("with_bnc", [True, False], ids=["bnc", "nobnc"])
def test_affine_partials(hip, pc, with_bnc):
    """group_norm_affine_partials[_stats] fed float32 casts of truth partials (the test owns R
    and cnt): s, t, mean, rstd against the float64 combination of the same numbers, by the
    module's rule with the float32 torch combination as the yardstick; the table of the stats
    entry == the plain entry's, bit for bit."""
    from op import norm_act
    from op._lib import check, lib, stream_ptr
    cpg, Rr, cnt = pc
    N, G, C = 2, 2, 2 * cpg
    part, d, truth, chain = R.partials_reference(pc, with_bnc)
    pg = part.to(hip)
    bnc = None if d["bnc"] is None else d["bnc"].to(hip)
    gn = _gn(C, G, d["gamma"], d["beta"])
    ss = norm_act.group_norm_affine_partials((pg, Rr, cnt), N, C, gn, bnc)
    ss2, mean, rstd = (torch.empty_like(ss), torch.empty(N, G, device=hip),
                       torch.empty(N, G, device=hip))
    check(lib.bpk_group_norm_affine_partials_stats_f32(
        pg.data_ptr(), Rr, cnt, _p(bnc), gn.weight.data_ptr(), gn.bias.data_ptr(), ss2.data_ptr(),
        mean.data_ptr(), rstd.data_ptr(), N, C, G, R.EPS, stream_ptr(hip)), "partials_stats")
    assert torch.equal(ss, ss2)
    native = {"mean": mean, "rstd": rstd, "s": ss[..., 0], "t": ss[..., 1]}
    E = max(R.err(chain[k], truth[k]) for k in native)
    assert E > 0
    bad = []
    for k, t in native.items():
        en = R.err(t, truth[k])
        print(f"affine_partials {pc} bnc={with_bnc} {k}: native {en:.3e} E {E:.3e}")
        record_err(f"group_norm affine_partials {pc} bnc={with_bnc} {k} native vs float64", en,
                   FACTOR * E)
        if not en <= FACTOR * E:
            bad.append(f"{k}: {en:.3e} > {FACTOR} x {E:.3e}")
    assert not bad, bad


@pytest.mark.parametrize("C1", [4, 6])
@pytest.mark.parametrize("with_bnc", [True, False], ids=["bnc", "nobnc"])
def test_affine_partials_two_sources(hip, C1, with_bnc):
    """The two-source entry (C = 12, G = 2: C1 = 4 splits group 0 between the sources, C1 = 6
    does not) == the single-source entry on the concatenated partials, bit for bit (the header's
    promise) -- which test_affine_partials holds against truth."""
    from op import norm_act
    pc = R.PART_CASES[2]
    part, d, _, _ = R.partials_reference(pc, with_bnc)
    pg = part.to(hip)
    bnc = None if d["bnc"] is None else d["bnc"].to(hip)
    gn = _gn(12, 2, d["gamma"], d["beta"])
    one = norm_act.group_norm_affine_partials((pg, pc[1], pc[2]), 2, 12, gn, bnc)
    two = norm_act.group_norm_affine_partials(
        (pg[:, :C1].contiguous(), pc[1], pc[2]), 2, 12, gn, bnc,
        part2=(pg[:, C1:].contiguous(), pc[1], pc[2]))
    assert torch.equal(one, two)


# ------------------------------------------------------------------ affine_silu
def _silu_bound(z, y):
    """(|z| + 4) 2^-23 |silu(z)| + |z| 2^-126 + 2^-149 per element.  The relative term: one FMA,
    the log2(e) scaling inside __expf (its error grows with |z|), v_exp_f32 and v_rcp_f32 at
    about an ulp each, one multiply.  The absolute terms: v_rcp_f32 returns no denormals, so
    once 1 + exp(-z) reaches 2^126 (z <= -87.34) the reciprocal -- below 2^-126 -- is flushed to
    zero and the result, z times it, with it: an error of up to |z| 2^-126 (the result's own
    subnormal range adds 2^-149).  Measured on an MI355X with the relative term and 2^-149 alone:
    exceeded only there, worst at z = -87.377, where the kernel returns 0 for a truth of
    -9.87e-37 (91790 x that bound); above z = -87.34 the error stays below 0.77 of the
    relative term (largest relative error 6.2e-6)."""
    return (z.abs() + 4) * 2.0 ** -23 * y.abs() + z.abs() * 2.0 ** -126 + 2.0 ** -149


@pytest.mark.parametrize("form", ["scalar-2-3-5-7", "float4-2-4-8-8", "misaligned-2-4-8-8"])
def test_affine_silu(hip, form):
    """silu(x s + t) with z spanning [-100, 100], finite everywhere and within _silu_bound of
    the exact z sigmoid(z) (z itself exact in float64 from the float32 x, s, t)."""
    from op import norm_act
    shape = (2, 3, 5, 7) if form.startswith("scalar") else (2, 4, 8, 8)
    g = torch.Generator().manual_seed(41)
    N, C = shape[:2]
    x = torch.rand(shape, generator=g) * 2 - 1
    x.view(-1)[:4] = torch.tensor([1.0, -1.0, 0.0, 0.5])
    ss = torch.stack([torch.full((N, C), 100.0), torch.zeros(N, C)], 2)
    ss[0, 1:] = torch.stack([torch.rand(C - 1, generator=g) * 47 + 50,
                             torch.rand(C - 1, generator=g) * 4 - 2], 1)
    xg = _off1(x) if form.startswith("misaligned") else x.to(hip)
    y = norm_act.affine_silu(xg, ss.to(hip))
    truth, z = R.affine_silu(x, ss)
    assert z.min().item() == -100.0 and z.max().item() == 100.0
    assert torch.isfinite(y).all()
    e = (y.double().cpu() - truth).abs()
    ratio = e / _silu_bound(z, truth)
    i = ratio.argmax()
    print(f"affine_silu {form}: worst {ratio.max().item():.3f} of its bound at z = "
          f"{z.reshape(-1)[i].item():.6g} (err {e.reshape(-1)[i].item():.3e}); "
          f"max rel err {(e / truth.abs().clamp_min(1e-30)).max().item():.3e}")
    live = z > -87.34
    rel = (e / ((z.abs() + 4) * 2.0 ** -23 * truth.abs() + 2.0 ** -149))[live].max().item()
    print(f"affine_silu {form}: worst {rel:.3f} of the relative term above z = -87.34")
    record_err(f"group_norm affine_silu {form} err / bound", ratio.max().item(), 1.0)
    record_err(f"group_norm affine_silu {form} err / relative term, z > -87.34", rel, 1.0)
    assert ratio.max().item() <= 1.0, f"z = {z.reshape(-1)[i].item()!r}: {e.reshape(-1)[i].item():.3e}"


# ------------------------------------------------------------------ param_grads
@pytest.mark.parametrize("N", R.PG_N)
def test_param_grads(hip, N):
    """bpk_group_norm_param_grads_f32 alone: d_bias_nc = the plane sums of dx, dgamma / dbeta =
    the sums over n of the per-sample partials, against float64 by the module's rule with torch's
    float32 sums as the chain (E = 0, sums of one term: exact), and within the bound of a
    float32 sum in any order.  N covers the per-wave quarter tail and the 8-wide unroll tail, C
    the 64-channel blocks with a ragged last one, H W the float4 and scalar row forms (one row
    misaligned).  Every combination of NULL outputs the ABI allows -- with all three inputs
    given, as the wrapper calls it, and with the inputs of the outputs not asked for NULL too --
    gives the same bits in the outputs asked for and touches no other."""
    from op._lib import check, lib, stream_ptr
    for C in R.PG_C:
        for HW, mis in R.PG_HW:
            (dx, dg, db), truth, chain, _ = R.param_grads_reference(N, C, HW, mis)
            ins = [_off1(dx) if mis else dx.to(hip), dg.to(hip), db.to(hip)]
            outs = {}
            for mask in range(8):
                want = [bool(mask & (1 << j)) for j in range(3)]
                for all_inputs in (True, False):
                    o = [torch.full(sh, 7.0, device=hip) for sh in ((N, C), (C,), (C,))]
                    check(lib.bpk_group_norm_param_grads_f32(
                        *(t.data_ptr() if (w or all_inputs) else None for t, w in zip(ins, want)),
                        *(t.data_ptr() if w else None for t, w in zip(o, want)),
                        N, C, HW, stream_ptr(hip)), "param_grads")
                    outs[mask, all_inputs] = o
            full = outs[7, True]
            for (mask, _), o in outs.items():
                for j in range(3):
                    ref = full[j] if mask & (1 << j) else torch.full_like(o[j], 7.0)
                    assert torch.equal(o[j], ref), (C, HW, mis, mask, j)
            got = dict(zip(("d_bnc", "dgamma", "dbeta"), full))
            E = max(R.err(chain[k], truth[k]) for k in truth)
            assert E < R.E_CEILING and (E > 0 or (N == 1 and HW == 1))
            what = f"N{N} C{C} HW{HW}{'m' if mis else ''}"
            for (k, t), terms, dim in zip(got.items(), (dx, dg, db), (2, 0, 0)):
                en = R.err(t, truth[k])
                record_err(f"group_norm param_grads {what} {k} native vs float64", en, FACTOR * E)
                assert en <= FACTOR * E, (what, k, en, E)
                e = (t.double().cpu() - truth[k]).abs()
                assert (e <= _sum_bound(terms, dim)).all(), (what, k, e.max().item())

"""GPU: every kernel path of csrc/sampler.hip against CPU restatements.

The Philox generator against oracle/philox_ref.py (float64 transcendentals), the predictor
and Langevin update kernels bit for bit against the float32 expressions of
oracle/score_sde_ref.py, the Langevin norms against float64 sums, and the VE / sub-VP engine
against oracle.score_sde_ref.pc_sample.  Shapes are the smallest that reach each loop, tail
and counter word of the kernels."""
import numpy as np
import pytest
import torch

from conftest import record_err
from oracle import philox_ref, score_sde_ref

pytestmark = pytest.mark.gpu

# Device Philox normals vs the float64 restatement, max |device - ref| / max(1, |ref|).  Not
# bit-exact: the device's logf / sincosf are not correctly rounded and every intermediate is
# rounded to float32.  Measured on MI355X over the 24 parametrized cases and the 2.1 M draw
# below: 1.77e-7 (about 3 float32 ulp at |z| = 1).  The tolerance is 8 x the measured value
# and may never exceed 1e-4: an indexing, constant or counter error moves most elements by
# O(1).
PHILOX_MEASURED = 1.77e-7
PHILOX_TOL = 8 * PHILOX_MEASURED
assert PHILOX_TOL <= 1e-4
# Langevin norms vs float64, relative: non-negative terms through at most 16 + 6 + 4 + chunks
# + 256 float32 additions and one square root, ~290 * 2^-24 = 1.7e-5 worst case, ~1e-6 typical
# (measured on MI355X over the cases below: at most 3.3e-7)
NORM_RTOL = 1e-5
# PC trajectories after the whole run, relative to max(1, max|ref|) (tests/test_gpu_models.py:
# measured 2e-7 .. 2e-6 on MI355X; the five VE / sub-VP cases below: 0 .. 1.4e-7)
PC_RTOL = 2e-4

PRED_NAMES = {"em": "euler_maruyama", "rd": "reverse_diffusion", "anc": "ancestral_sampling"}


def _step(hip, v=0):
    return torch.tensor([v], dtype=torch.int32, device=hip)


def _sde(kind, N=1000):
    """(oracle SDESpec, product SDE) of one kind."""
    import sde_lib
    sde = {"vp": lambda: sde_lib.VPSDE(0.1, 20., N), "subvp": lambda: sde_lib.subVPSDE(0.1, 20., N),
           "ve": lambda: sde_lib.VESDE(0.01, 50., N)}[kind]()
    return score_sde_ref.SDESpec(kind, N), sde


def _pred_kind(pred, kind):
    from op import sde_kernels as K
    if pred == "anc":
        return K.PRED_ANC_VE if kind == "ve" else K.PRED_ANC_VP
    return {"em": K.PRED_EM, "rd": K.PRED_RD}[pred]


def _table(rows, hip, padded):
    """(coef table, step): `rows` [B, 8] as a one-row table at step 0, or in row 2 of a 3-row
    table whose rows 0 and 1 are NaN, with step = 2."""
    if not padded:
        return rows[None].contiguous().to(hip), _step(hip, 0)
    full = torch.full((3,) + tuple(rows.shape), float("nan"))
    full[2] = rows
    return full.to(hip), _step(hip, 2)


# ------------------------------------------------------------------ 2. device Philox

def _philox_err(dev, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(dev.double().cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))).max())


@pytest.mark.parametrize("step,draw", [(0, 0), (7, 1), (999, 5)])
@pytest.mark.parametrize("seed", [0, 2 ** 63 + 12345])
@pytest.mark.parametrize("B,D,off", [(3, 10, 0), (4, 7, 0), (2, 7, 2), (2, 8, 2 ** 33 + 1)])
def test_philox_matches_restatement(hip, B, D, off, seed, step, draw):
    """Round count, multipliers, counter word order (q_lo, q_hi, step, draw), both key words,
    the Box-Muller layout and the sample_offset / D indexing; the last shape has q_hi != 0."""
    from op import sde_kernels as K
    dev = K.philox_normal((B, D), seed, _step(hip, step), draw, sample_offset=off, device=hip)
    err = _philox_err(dev, philox_ref.normal(B, D, off, seed, step, draw))
    print(f"philox B={B} D={D} off={off} seed={seed} step={step} draw={draw}: err {err:.3e}")
    record_err(f"philox {B}x{D}+{off} seed {seed} step {step} draw {draw}", err, PHILOX_TOL)
    assert err <= PHILOX_TOL


def test_philox_streams_differ_by_step_and_draw(hip):
    from op import sde_kernels as K
    z = {sd: K.philox_normal((4, 7), 99, _step(hip, sd[0]), sd[1], device=hip)
         for sd in [(7, 1), (7, 2), (8, 1)]}
    keys = list(z)
    for i in range(3):
        for j in range(i + 1, 3):
            assert not (z[keys[i]] == z[keys[j]]).any(), (keys[i], keys[j])
    # step_ptr NULL means step 0
    assert torch.equal(K.philox_normal((4, 7), 99, None, 1, device=hip),
                       K.philox_normal((4, 7), 99, _step(hip, 0), 1, device=hip))


def test_philox_large_odd_draw(hip):
    """2.1 M values: the grid-stride loop (8192 x 256 threads) runs a second pass, D is odd so
    every sample boundary falls inside a Philox block."""
    from op import sde_kernels as K
    B, D, off, seed, step, draw = 3, 700001, 5, 2 ** 40 + 3, 3, 1
    n = B * D
    assert n > 8192 * 256
    dev = K.philox_normal((B, D), seed, _step(hip, step), draw, sample_offset=off, device=hip)
    assert torch.isfinite(dev).all()
    assert dev.abs().max().item() <= 5.77  # sqrt(-2 ln 2^-24) = 5.768
    idx = np.unique(np.concatenate([np.linspace(0, n - 1, 4096 - 8).astype(np.int64),
                                    np.arange(n - 8, n)]))
    b, e = idx // D, idx % D
    ref = philox_ref.normal_at((off + b) * D + e, seed, step, draw)
    err = _philox_err(dev.reshape(-1)[torch.from_numpy(idx).to(hip)], ref)
    print(f"philox large: err {err:.3e}")
    record_err("philox 3x700001+5 sampled", err, PHILOX_TOL)
    assert err <= PHILOX_TOL
    v = dev.double()
    assert abs(v.mean().item()) <= 5 / np.sqrt(n)
    assert abs(v.var().item() - 1) <= 5 * np.sqrt(2 / n)


# ------------------------------------------------------------------ 3. in-kernel noise sites

def _noise_site_setup(hip):
    torch.manual_seed(3)
    B, D, off, seed, step = 3, 35, 6, 2 ** 40 + 3, 4
    x, m = torch.randn(B, D).to(hip), torch.randn(B, D).to(hip)
    coef = (0.1 + torch.rand(5, B, 8)).to(hip)  # 5 rows, coef_bdim = B, all positive
    return B, D, off, seed, step, x, m, coef


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_predictor_in_kernel_noise_is_the_philox_stream(hip, kind):
    from op import sde_kernels as K
    B, D, off, seed, step, x, m, coef = _noise_site_setup(hip)
    st = _step(hip, step)
    z = K.philox_normal((B, D), seed, st, 0, sample_offset=off, device=hip)
    outs = []
    for noise in (None, z):
        xo, xm = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        K.predictor(kind, x, m, coef, st, x_out=xo, x_mean=xm, noise=noise, seed=seed, draw=0,
                    sample_offset=off)
        outs.append((xo, xm))
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[0][1])  # the noise term is there


@pytest.mark.parametrize("mode", [0, 1])
def test_langevin_in_kernel_noise_is_the_philox_stream(hip, mode):
    from op import sde_kernels as K
    B, D, off, seed, step, x, m, coef = _noise_site_setup(hip)
    st = _step(hip, step)
    z = K.philox_normal((B, D), seed, st, 2, sample_offset=off, device=hip)
    outs = []
    for noise in (None, z):
        ws = K.langevin_workspace(B, D, hip).fill_(float("nan"))
        red = torch.full((2,), float("nan"), device=hip)
        K.langevin_norms(m, coef, st, ws, red, noise=noise, seed=seed, draw=2, sample_offset=off)
        xo, xm = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        K.langevin_update(mode, x, m, coef, st, red, x_out=xo, x_mean=xm, noise=noise,
                          seed=seed, draw=2, sample_offset=off)
        outs.append((red, xo, xm))
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][1], outs[0][2])


# ------------------------------------------------------------------ 4. predictor, bit-exact

PRED_CASES = [("em", "vp", True), ("em", "vp", False), ("em", "subvp", True), ("em", "ve", True),
              ("rd", "vp", True), ("rd", "vp", False), ("rd", "ve", True),
              ("anc", "vp", True), ("anc", "vp", False), ("anc", "ve", True)]


def _predictor_case(hip, pred, kind, continuous, shape, padded, seed=0):
    """Device (x_out, x_mean) and the oracle's, for the same model output m and noise z."""
    import sampling
    from op import sde_kernels as K
    spec, sde = _sde(kind)
    g = torch.Generator().manual_seed(seed)
    x, m, z = (torch.randn(shape, generator=g) for _ in range(3))
    t = torch.tensor([0.9, 0.4567, 0.003])
    with torch.no_grad():
        ref_x, ref_mean = score_sde_ref._predictor(
            PRED_NAMES[pred], spec, score_sde_ref.make_score(lambda x_, l_: m, spec, continuous),
            x, t, lambda: z)
    pk = _pred_kind(pred, kind)
    rows = sampling.coef_rows(sde, t, continuous, pk)
    assert rows.shape == (3, K.COEF_STRIDE)
    assert not torch.equal(rows[0], rows[1]) and not torch.equal(rows[1], rows[2])
    coef, st = _table(rows, hip, padded)
    xd = x.to(hip)
    xo, xm = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    K.predictor(pk, xd, m.to(hip), coef, st, x_out=xo, x_mean=xm, noise=z.to(hip),
                score_mode=K.SCORE_RAW if kind == "ve" else K.SCORE_DIV,
                drift_mul_x=int(kind != "ve"))
    return (xo, xm), (ref_x, ref_mean), (xd, m.to(hip), z.to(hip), coef, st, pk)


@pytest.mark.parametrize("padded", [False, True], ids=["row0", "row2of3"])
@pytest.mark.parametrize("pred,kind,continuous", PRED_CASES)
def test_predictor_bit_exact_vs_oracle(hip, pred, kind, continuous, padded):
    """All four predictor kinds, both score modes and drift_mul_x values, per-sample t
    (coef_bdim = B with distinct rows), step 0 and step 2 of a table whose other rows are
    NaN: x_out and x_mean equal the oracle's float32 expressions bit for bit."""
    (xo, xm), (ref_x, ref_mean), _ = _predictor_case(hip, pred, kind, continuous, (3, 1, 5, 7),
                                                     padded)
    assert torch.isfinite(ref_x).all() and not torch.equal(ref_x, ref_mean)
    assert torch.equal(xm.cpu(), ref_mean)
    assert torch.equal(xo.cpu(), ref_x)


# ------------------------------------------------------------------ 5. Langevin norms

@pytest.mark.parametrize("bdim", ["one", "B"])
@pytest.mark.parametrize("score_mode", [0, 1])
@pytest.mark.parametrize("B,D", [(1, 1), (3, 63), (3, 4096), (3, 4097), (2, 3 * 4096 + 5),
                                 (257, 4097)])
def test_langevin_norms_vs_float64(hip, B, D, score_mode, bdim):
    """Chunk tail (D % 4096 != 0), chunks > 1, B > 256 (the b += 256 loop of the reduce), both
    score modes; per-sample C_SDIV in row 2 of a 3-row table (rows 0, 1 NaN) when
    coef_bdim = B.  The workspace and the result start as NaN."""
    from op import sde_kernels as K
    g = torch.Generator().manual_seed(B * 100003 + D)
    m, z = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    if bdim == "one":
        sdiv = torch.tensor([0.37])
        rows = torch.zeros(1, K.COEF_STRIDE)
        rows[:, K.C_SDIV] = sdiv
        coef, st = _table(rows, hip, False)
    else:
        sdiv = torch.linspace(0.05, 1.0, B) if B > 1 else torch.tensor([0.05])
        rows = torch.zeros(B, K.COEF_STRIDE)
        rows[:, K.C_SDIV] = sdiv
        coef, st = _table(rows, hip, True)
    score = (-m.double() / sdiv.double()[:, None]) if score_mode == 0 else m.double()
    ref = torch.stack([score.norm(dim=1).sum(), z.double().norm(dim=1).sum()])
    ws = K.langevin_workspace(B, D, hip).fill_(float("nan"))
    red = torch.full((2,), float("nan"), device=hip)
    K.langevin_norms(m.to(hip), coef, st, ws, red, noise=z.to(hip), score_mode=score_mode)
    err = ((red.double().cpu() - ref).abs() / ref).max().item()
    print(f"langevin norms B={B} D={D} mode={score_mode} bdim={bdim}: rel err {err:.3e}")
    record_err(f"langevin norms {B}x{D} score_mode {score_mode} bdim {bdim}", err, NORM_RTOL)
    assert err <= NORM_RTOL


# ------------------------------------------------------------------ 6. Langevin update, bit-exact

def _langevin_expect(mode, x, m, z, rows, red, B_global, snr, divides):
    """The oracle's float32 expression order (score_sde_ref._corrector) given the reduced
    norms `red` = (sum_b ||g_b||, sum_b ||z_b||) and the batch size they were summed over.

    sqrt(step * 2) is taken in float64 and rounded once, which is the correctly rounded
    float32 square root (53 >= 2 * 24 + 2 bits) the device's sqrtf returns.  torch.sqrt on a
    float32 CPU tensor is not correctly rounded on every host: on one MI355X node's CPU it gave
    0x3e59a40d for sqrt(0x3d390786), one ulp above the exact rounding 0x3e59a40c that the
    kernel (and numpy) return, which made vp / mode 0 differ in 8 of 105 elements."""
    from op import sde_kernels as K
    bc = (slice(None),) + (None,) * (x.dim() - 1)
    g = -m / rows[:, K.C_SDIV][bc] if divides else m
    alpha = rows[:, K.C_ALPHA]
    if mode == 0:
        gn, nn_ = red[0] / B_global, red[1] / B_global
        r = snr * nn_ / gn
    else:
        r = snr * rows[:, K.C_AUX]
    step = r * r * 2 * alpha
    x_mean = x + step[bc] * g
    nscale = torch.sqrt((step * 2).double()).float()
    return x_mean + nscale[bc] * z, x_mean


def _langevin_case(hip, mode, kind, shape, B_global, seed=1):
    import sampling
    from op import sde_kernels as K
    _, sde = _sde(kind)
    g = torch.Generator().manual_seed(seed)
    x, m, z = (torch.randn(shape, generator=g) for _ in range(3))
    B = shape[0]
    t = torch.tensor([0.9, 0.4567, 0.003])
    rows = sampling.coef_rows(sde, t, True)
    assert torch.isfinite(rows).all()
    assert bool((rows[:, K.C_ALPHA] == 1).all()) == (kind == "ve")
    # the norms a batch of B_global samples of this size would reduce to (any positive pair)
    red = torch.tensor([1.37, 0.91]) * (B_global or B) * float(np.sqrt(x[0].numel()))
    snr = 0.16
    ref_x, ref_mean = _langevin_expect(mode, x, m, z, rows, red, B_global or B, snr, kind != "ve")
    coef, st = _table(rows, hip, True)
    args = (mode, x.to(hip), m.to(hip), coef, st, red.to(hip))
    kw = dict(noise=z.to(hip), B_global=B_global, snr=snr,
              score_mode=K.SCORE_RAW if kind == "ve" else K.SCORE_DIV)
    xo, xm = torch.full_like(args[1], float("nan")), torch.full_like(args[1], float("nan"))
    K.langevin_update(*args, x_out=xo, x_mean=xm, **kw)
    return (xo, xm), (ref_x, ref_mean), (args, kw)


@pytest.mark.parametrize("mode,kind,B_global", [(0, "vp", None), (0, "vp", 6), (0, "ve", None),
                                                (1, "vp", None), (1, "ve", None)])
def test_langevin_update_bit_exact_given_red(hip, mode, kind, B_global):
    (xo, xm), (ref_x, ref_mean), _ = _langevin_case(hip, mode, kind, (3, 1, 5, 7), B_global)
    assert torch.isfinite(ref_x).all() and not torch.equal(ref_x, ref_mean)
    assert torch.equal(xm.cpu(), ref_mean)
    assert torch.equal(xo.cpu(), ref_x)


# ------------------------------------------------------------------ 7. in place, large launches

LARGE = (3, 1, 1, 700001)  # 2.1 M elements: second grid-stride pass; odd D


def test_predictor_in_place_and_grid_stride(hip):
    """x_out = x (what PCEngine passes every step) equals the out-of-place result, which
    equals the oracle on every element, the tail included."""
    from op import sde_kernels as K
    (xo, xm), (ref_x, ref_mean), (x, m, z, coef, st, pk) = _predictor_case(
        hip, "em", "vp", True, LARGE, True)
    assert x.numel() > 8192 * 256
    assert torch.equal(xm.cpu(), ref_mean) and torch.equal(xo.cpu(), ref_x)
    xi, xmi = x.clone(), torch.full_like(x, float("nan"))
    K.predictor(pk, xi, m, coef, st, x_out=xi, x_mean=xmi, noise=z)
    assert torch.equal(xi, xo) and torch.equal(xmi, xm)
    # and with the in-kernel noise
    outs = []
    for inplace in (False, True):
        xin = x.clone()
        out = xin if inplace else torch.full_like(x, float("nan"))
        K.predictor(pk, xin, m, coef, st, x_out=out, x_mean=None, seed=5, draw=0, sample_offset=2)
        outs.append(out)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_langevin_update_in_place_and_grid_stride(hip):
    from op import sde_kernels as K
    (xo, xm), (ref_x, ref_mean), (args, kw) = _langevin_case(hip, 0, "vp", LARGE, None)
    assert torch.equal(xm.cpu(), ref_mean) and torch.equal(xo.cpu(), ref_x)
    mode, x, m, coef, st, red = args
    xi, xmi = x.clone(), torch.full_like(x, float("nan"))
    K.langevin_update(mode, xi, m, coef, st, red, x_out=xi, x_mean=xmi, **kw)
    assert torch.equal(xi, xo) and torch.equal(xmi, xm)


# ------------------------------------------------------------------ 8. small kernels, refusals

@pytest.mark.parametrize("step", [0, 11])
@pytest.mark.parametrize("B", [1, 257, 1000])
def test_fill_from_table(hip, B, step):
    from op import sde_kernels as K
    table = torch.arange(12, dtype=torch.float32, device=hip) * 0.25 + 3
    out = torch.full((B,), float("nan"), device=hip)
    K.fill_from_table(out, table, _step(hip, step))
    assert torch.equal(out, table[step].expand(B))


def test_step_increment(hip):
    from op import sde_kernels as K
    st = _step(hip, 0)
    for _ in range(3):
        K.step_increment(st)
    assert st.item() == 3


def test_bad_arguments_are_refused_before_any_launch(hip):
    from op import sde_kernels as K
    x = torch.zeros(3, 8, device=hip)
    coef = torch.ones(1, 1, 8, device=hip)
    st = _step(hip)
    red = torch.ones(2, device=hip)
    out = torch.zeros_like(x)
    with pytest.raises(RuntimeError):
        K.predictor(4, x, x, coef, st, x_out=out, noise=x)
    with pytest.raises(RuntimeError):
        K.predictor(0, x, x, coef, st, x_out=out, noise=x, score_mode=2)
    with pytest.raises(RuntimeError):
        K.langevin_update(2, x, x, coef, st, red, x_out=out, noise=x)
    big = torch.zeros(65536, 1, device=hip)
    with pytest.raises(RuntimeError):
        K.langevin_norms(big, coef, st, K.langevin_workspace(65536, 1, hip), red, noise=big)
    with pytest.raises(RuntimeError):
        K.predictor(0, x, x, torch.ones(1, 2, 8, device=hip), st, x_out=out, noise=x)
    assert torch.equal(out, torch.zeros_like(x))
    # empty batches / samples are no-ops
    for shape in [(0, 8), (3, 0)]:
        e = torch.zeros(shape, device=hip)
        K.predictor(0, e, e, coef, st, x_out=e.clone(), x_mean=e.clone(), noise=e)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 9. engine: VE and sub-VP

def _engine_model(kind, continuous, sde):
    """Plain callables of elementwise torch arithmetic: the same function on CPU and GPU."""
    if kind == "subvp":
        return lambda x, lab: 0.5 * x + 0.001 * lab[:, None, None, None]
    if continuous:
        return lambda x, lab: -x / (1 + lab * lab)[:, None, None, None]

    def discrete(x, lab):
        sig = sde.discrete_sigmas.to(x.device).flip(0)[lab]
        return -x / (1 + sig * sig)[:, None, None, None]

    return discrete


ENGINE_CASES = [("ve", "euler_maruyama", "langevin", True),
                ("ve", "reverse_diffusion", "ald", False),
                ("ve", "ancestral_sampling", "none", False),
                ("ve", "none", "langevin", True),
                ("subvp", "euler_maruyama", "none", True)]


@pytest.mark.parametrize("kind,pred,corr,continuous", ENGINE_CASES)
def test_engine_ve_subvp_matches_oracle_with_injected_noise(hip, kind, pred, corr, continuous):
    import sampling
    N, n_steps, snr, shape = 12, 2, 0.16, (3, 1, 5, 7)
    spec, sde = _sde(kind, N)
    g = torch.Generator().manual_seed(11)
    prior = torch.randn(shape, generator=g) * (50.0 if kind == "ve" else 1.0)
    n_corr = n_steps if corr != "none" else 0
    order = [1 + j for j in range(n_corr)] + ([0] if pred != "none" else [])
    draws = [torch.randn(shape, generator=g) for _ in range(N * len(order))]
    model = _engine_model(kind, continuous, sde)
    ref, nfe_ref = score_sde_ref.pc_sample(model, spec, prior, pred, corr, snr, n_steps,
                                           continuous, draws=draws)
    assert torch.isfinite(ref).all()
    # the oracle's sequential draw order mapped onto the engine's (step, draw id)
    table = {(i, d): draws[i * len(order) + k] for i in range(N) for k, d in enumerate(order)}
    eng = sampling.PCEngine(sde, shape, sampling.get_predictor(pred), sampling.get_corrector(corr),
                            snr, n_steps, continuous=continuous, device=hip,
                            noise_fn=lambda i, d: table[(i, d)])
    out, nfe = eng(model, x_init=prior)
    assert nfe == nfe_ref
    if pred == "none":  # NonePredictor returns (x, x): no denoised mean after the corrector
        assert torch.equal(eng._x, eng._xm)
    scale = max(1.0, ref.abs().max().item())
    err = (out.cpu() - ref).abs().max().item() / scale
    print(f"engine {kind} {pred} {corr} continuous={continuous}: err {err:.3e} (max|ref| "
          f"{ref.abs().max().item():.3g})")
    record_err(f"pc engine {kind} {pred}/{corr} continuous={continuous}", err, PC_RTOL)
    assert err <= PC_RTOL


def test_engine_seeded_noise_is_the_philox_stream(hip):
    """The eager engine's in-kernel noise (draw ids 1 + j for the corrector, 0 for the
    predictor, the device step counter) is K.philox_normal of the same (seed, step, draw)."""
    import sampling
    from op import sde_kernels as K
    shape = (3, 1, 5, 7)
    _, sde = _sde("ve", 12)
    model = _engine_model("ve", True, sde)
    prior = torch.randn(shape, generator=torch.Generator().manual_seed(12)) * 50.0
    mk = lambda **kw: sampling.PCEngine(sde, shape, sampling.EulerMaruyamaPredictor,
                                        sampling.LangevinCorrector, 0.16, 2, continuous=True,
                                        device=hip, use_graph=False, **kw)
    xs, xms = mk(seed=77).run(model, prior)
    xn, xmn = mk(seed=77, noise_fn=lambda i, d: K.philox_normal(
        shape, 77, _step(hip, i), d, sample_offset=0, device=hip)).run(model, prior)
    assert torch.isfinite(xs).all() and not torch.equal(xs, xms)
    assert torch.equal(xs, xn) and torch.equal(xms, xmn)


def test_subvp_pairs_the_reference_raises_on_do_not_reach_the_kernels(hip):
    import sampling
    import sde_lib
    sub = sde_lib.subVPSDE(0.1, 20., 12)
    model = _engine_model("subvp", True, sub)
    sampler = sampling.get_pc_sampler(sub, (2, 1, 5, 7), sampling.AncestralSamplingPredictor,
                                      sampling.NoneCorrector, lambda v: v, 0.16, continuous=True,
                                      device=hip)
    with pytest.raises(NotImplementedError):
        sampler(model)
    x, t = torch.randn(2, 1, 5, 7, device=hip), torch.full((2,), 0.5, device=hip)
    for corr in (sampling.LangevinCorrector, sampling.AnnealedLangevinDynamics):
        fused = corr(sub, lambda x_, t_: x_, 0.16, 1)
        with pytest.raises(AttributeError):
            fused.update_fn(x, t)
        sampler = sampling.get_pc_sampler(sub, (2, 1, 5, 7), sampling.EulerMaruyamaPredictor, corr,
                                          lambda v: v, 0.16, continuous=True, device=hip)
        with pytest.raises(AttributeError):
            sampler(model)

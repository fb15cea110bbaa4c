"""Test helper: the ns_step step (compat=False) restated in plain differentiable torch ops,
for any dtype and device, and the field generators of the ns_step VJP tests.

Tensors are [B, C, S2, S3] as the ops take them.  A plane is indexed as the reference does,
f[y * nx + x] with nx = S2 and ny = S3: the plane's memory is viewed as [ny, nx] with x
fastest (for a square plane x is the last axis).  Signs and upwind indices are detached: the
derivative is piecewise, like the function.

Also here, shared by tests/test_ns_vjp_host.py and tests/test_gpu_ns_vjp.py: the VJP cases,
their float64 truth and float32 noise floor (computed once per session), and the 4D-Var twin
experiment.
"""
import math

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------ plane views
def _planes(t):
    """[B, C, S2, S3] -> [B, C, ny, nx] view of the same memory (ny = S3, nx = S2)."""
    B, C, nx, ny = t.shape
    return t.contiguous().view(B, C, ny, nx)


def _tensor(t, like):
    B, C, nx, ny = like.shape
    return t.reshape(B, -1, nx, ny)


def _mirror(i, n):
    i = torch.where(i < 0, -i, i)
    return torch.where(i > n - 1, 2 * n - 2 - i, i)


# ------------------------------------------------------------------ plane ops ([.., ny, nx])
def _diff_last(f, dx):
    lo = (f[..., 1:2] - f[..., 0:1]) / dx
    mid = (f[..., 2:] - f[..., :-2]) / dx / 2
    hi = (f[..., -1:] - f[..., -2:-1]) / dx
    return torch.cat([lo, mid, hi], dim=-1)


def _grad_planes(f, dx):
    fx = _diff_last(f, dx)
    fy = _diff_last(f.transpose(-1, -2), dx).transpose(-1, -2)
    return fx, fy


def _take(f, yi, xi):
    nx = f.shape[-1]
    idx = (yi * nx + xi).flatten(-2)
    return f.flatten(-2).gather(-1, idx).view(f.shape)


def _cip_planes(f, fx, fy, u, v, dt, dx):
    """CIP advection of plane f (with gradients fx, fy) by (u, v); all [B, 1, ny, nx]."""
    ny, nx = f.shape[-2:]
    sx, sy = torch.sign(u).detach(), torch.sign(v).detach()
    xi = torch.arange(nx, device=f.device).view(1, 1, 1, nx).expand_as(f)
    yi = torch.arange(ny, device=f.device).view(1, 1, ny, 1).expand_as(f)
    xm = _mirror(xi - sx.long(), nx)
    ym = _mirror(yi - sy.long(), ny)
    f_c, f_xm, f_ym, f_xy = f, _take(f, yi, xm), _take(f, ym, xi), _take(f, ym, xm)
    fx_c, fx_xm, fx_ym = fx, _take(fx, yi, xm), _take(fx, ym, xi)
    fy_c, fy_xm, fy_ym = fy, _take(fy, yi, xm), _take(fy, ym, xi)
    tmp1 = f_c - f_ym - f_xm + f_xy
    tmp2 = f_xm - f_c
    tmp3 = f_ym - f_c
    xd, yd = sx * dx * dx * dx, sy * dx * dx * dx
    a = (sx * (fx_xm + fx_c) * dx + 2 * tmp2) / xd
    b = (sy * (fy_ym + fy_c) * dx + 2 * tmp3) / yd
    c = (-tmp1 - sx * (fx_ym - fx_c) * dx) / yd
    d = (-tmp1 - sy * (fy_xm - fy_c) * dx) / xd
    e = (3 * tmp2 + sx * (fx_xm + 2 * fx_c) * dx) / dx / dx
    ff = (3 * tmp3 + sy * (fy_ym + 2 * fy_c) * dx) / dx / dx
    g = (-(fy_xm - fy_c) + c * dx * dx) / (sx * dx)
    X, Y = -u * dt, -v * dt
    return (((a * X + c * Y + e) * X + g * Y + fx_c) * X
            + ((b * Y + d * X + ff) * Y + fy_c) * Y + f_c)


def _pressure_planes(p, u, v, dt, dx):
    ny, nx = p.shape[-2:]
    ax = torch.arange(nx, device=p.device)
    ay = torch.arange(ny, device=p.device)
    xu, xd = _mirror(ax + 1, nx), _mirror(ax - 1, nx)
    yu, yd = _mirror(ay + 1, ny), _mirror(ay - 1, ny)
    sel = torch.index_select
    sxx = sel(u, -1, xu) - sel(u, -1, xd)
    sxy = sel(v, -1, xu) - sel(v, -1, xd)
    syx = sel(u, -2, yu) - sel(u, -2, yd)
    syy = sel(v, -2, yu) - sel(v, -2, yd)
    aver = 0.25 * (sel(p, -1, xd) + sel(p, -1, xu) + sel(p, -2, yd) + sel(p, -2, yu))
    return aver + (sxx * sxx + syy * syy + syx * sxy) / 8 - dx * (sxx + syy) / (8 * dt)


# ------------------------------------------------------------------ the ops ([B, C, S2, S3])
def grad_xy(f, dx):
    fx, fy = _grad_planes(_planes(f), dx)
    return _tensor(fx, f), _tensor(fy, f)


def cip(f, vel, dt, dx):
    """CIP advection of the [B, 1, ..] field f (with its stencil gradient) by vel [B, 2, ..]."""
    fp, vp = _planes(f), _planes(vel)
    fx, fy = _grad_planes(fp, dx)
    return _tensor(_cip_planes(fp, fx, fy, vp[:, 0:1], vp[:, 1:2], dt, dx), f)


def update_density(dens, vel, dt, dx):
    return cip(dens, vel, dt, dx)


def pressure(pres, vel, dt, dx):
    vp = _planes(vel)
    return _tensor(_pressure_planes(_planes(pres), vp[:, 0:1], vp[:, 1:2], dt, dx), pres)


update_pressure = pressure


def update_velocity(vel, pres, dt, dx):
    vp, pp = _planes(vel), _planes(pres)
    px, py = _grad_planes(pp, dx)
    un, vn = vp[:, 0:1] - px * dt, vp[:, 1:2] - py * dt
    out = []
    for fld in (un, vn):
        fx, fy = _grad_planes(fld, dx)
        out.append(_cip_planes(fld, fx, fy, un, vn, dt, dx))
    return _tensor(torch.cat(out, dim=1), vel)


def full_step(dens, vel, pres, dt, dx):
    v1 = update_velocity(vel, pres, dt, dx)
    p1 = pressure(pres, v1, dt, dx)
    d1 = update_density(dens, v1, dt, dx)
    return d1, v1, p1


def rollout(dens, vel, pres, steps, dt, dx):
    ds, vs, ps = [], [], []
    for _ in range(steps):
        dens, vel, pres = full_step(dens, vel, pres, dt, dx)
        ds.append(dens), vs.append(vel), ps.append(pres)
    return torch.stack(ds), torch.stack(vs), torch.stack(ps)


# ------------------------------------------------------------------ field generators (CPU)
DT, DX = 0.0025, 0.005
SHAPES = [(2, 7, 5), (1, 9, 70), (3, 6, 66), (2, 16, 16)]  # (B, H, W)


def smooth(shape, seed):
    """Seeded randn, three 3x3 avg_pool2d passes (stride 1, pad 1), divided by its max abs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    for _ in range(3):
        x = F.avg_pool2d(x, 3, stride=1, padding=1)
    return x / x.abs().max()


def random_sign_fields(B, H, W, seed):
    """float64 (dens, vel, pres): both signs and every mirrored border are exercised, and
    dt |grad p| << 0.3 keeps every velocity component away from 0."""
    g = torch.Generator().manual_seed(seed + 1000)
    dens = 0.5 + 0.2 * smooth((B, 1, H, W), seed)
    mag = 0.3 + 0.7 * torch.rand(B, 2, H, W, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(B, 2, H, W, generator=g) < 0.5, -1.0, 1.0).double()
    pres = 0.002 * smooth((B, 1, H, W), seed + 1)
    return dens, mag * sign, pres


def cotangents(B, H, W, seed):
    g = torch.Generator().manual_seed(seed + 2000)
    return (torch.randn(B, 1, H, W, generator=g, dtype=torch.float64),
            torch.randn(B, 2, H, W, generator=g, dtype=torch.float64),
            torch.randn(B, 1, H, W, generator=g, dtype=torch.float64))


def twin_fields(B=2, n=16, seed=0):
    """Twin experiment: float64 truth (dens, vel, pres) and background (dens_b, vel_b)."""
    lin = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    wave = (torch.sin(2 * math.pi * xx) * torch.cos(2 * math.pi * yy)).expand(B, 1, n, n)
    dens = 0.5 + 0.3 * wave + 0.05 * smooth((B, 1, n, n), seed)
    base = torch.tensor([0.6, -0.5], dtype=torch.float64).view(1, 2, 1, 1)
    vel = base + 0.1 * smooth((B, 2, n, n), seed + 1)
    pres = 0.002 * smooth((B, 1, n, n), seed + 2)
    dens_b = dens + 0.05 * smooth((B, 1, n, n), seed + 3)
    vel_b = vel + 0.1 * smooth((B, 2, n, n), seed + 4)
    return (dens, vel, pres), (dens_b, vel_b)


def step_fn(dens, vel, pres, dt=DT, dx=DX):
    """`FourDVar(step_fn=...)` signature."""
    return full_step(dens, vel, pres, dt, dx)


def rel_err(g, truth):
    """max|g - truth| / max|truth| (truth float64)."""
    truth = truth.double()
    return float((g.detach().double().cpu() - truth.cpu()).abs().max() / truth.abs().max())


# ------------------------------------------------------------------ VJP cases
class RefOps:
    """The restatement behind the call signatures the tests use for both sides."""
    update_density = staticmethod(update_density)
    update_pressure = staticmethod(update_pressure)
    update_velocity = staticmethod(update_velocity)
    full_step = staticmethod(full_step)


CASES = ("full_step", "full_step_dens_only", "full_step_pres_only", "update_density",
         "update_velocity", "update_pressure")
BOUND_FACTOR = 8.0  # gather sums ~40 terms in another order + FMA contraction


def case_grads(ops, case, dens, vel, pres, cots, dt=DT, dx=DX):
    """Gradients of <outputs, cotangents> of one case -> {input name: grad}.  `ops` has
    full_step(d, v, p, dt, dx) and update_*(.., dt, dx); unused outputs get no cotangent."""
    gd, gv, gp = [c.to(dens.dtype).to(dens.device) for c in cots]
    d, v, p = [t.detach().clone().requires_grad_(True) for t in (dens, vel, pres)]
    if case.startswith("full_step"):
        d1, v1, p1 = ops.full_step(d, v, p, dt, dx)
        if case == "full_step":
            loss, ins = (d1 * gd).sum() + (v1 * gv).sum() + (p1 * gp).sum(), dict(dens=d, vel=v, pres=p)
        elif case == "full_step_dens_only":
            loss, ins = (d1 * gd).sum(), dict(dens=d, vel=v, pres=p)
        else:
            loss, ins = (p1 * gp).sum(), dict(vel=v, pres=p)
    elif case == "update_density":
        loss, ins = (ops.update_density(d, v, dt, dx) * gd).sum(), dict(dens=d, vel=v)
    elif case == "update_velocity":
        loss, ins = (ops.update_velocity(v, p, dt, dx) * gv).sum(), dict(vel=v, pres=p)
    elif case == "update_pressure":
        loss, ins = (ops.update_pressure(p, v, dt, dx) * gp).sum(), dict(pres=p, vel=v)
    else:
        raise KeyError(case)
    grads = torch.autograd.grad(loss, list(ins.values()))
    return dict(zip(ins.keys(), grads))


_CACHE = {}


def case_inputs(shape, dtype=torch.float64):
    key = ("in", shape)
    if key not in _CACHE:
        B, H, W = shape
        _CACHE[key] = (random_sign_fields(B, H, W, 7), cotangents(B, H, W, 3))
    fields, cots = _CACHE[key]
    return [t.to(dtype) for t in fields], cots


def case_truth(case, shape):
    """float64 CPU autograd of the restatement (computed once, never modified)."""
    key = ("truth", case, shape)
    if key not in _CACHE:
        fields, cots = case_inputs(shape)
        _CACHE[key] = case_grads(RefOps, case, *fields, cots)
    return _CACHE[key]


def case_floor(case):
    """Noise floor of a case class: the largest float32-vs-float64 gradient error of the
    restatement's CPU autograd over the shapes and input tensors."""
    key = ("floor", case)
    if key not in _CACHE:
        worst = 0.0
        for shape in SHAPES:
            fields, cots = case_inputs(shape, torch.float32)
            g32 = case_grads(RefOps, case, *fields, cots)
            truth = case_truth(case, shape)
            worst = max(worst, max(rel_err(g32[k], truth[k]) for k in truth))
        _CACHE[key] = worst
    return _CACHE[key]


# ------------------------------------------------------------------ rollout case
ROLLOUT_STEPS = 4


def rollout_inputs(dtype=torch.float64):
    (d, v, p), _ = twin_fields()
    g = torch.Generator().manual_seed(4000)
    w = torch.randn(ROLLOUT_STEPS, *d.shape, generator=g, dtype=torch.float64)
    return [t.to(dtype) for t in (d, v, p)], w


def rollout_grads(rollout_fn, dens, vel, pres, w):
    """Gradient of sum(w * density frames) of a 4-step rollout; rollout_fn(d, v, p, steps)
    -> (dens_traj, vel_traj, pres_traj)."""
    d, v, p = [t.detach().clone().requires_grad_(True) for t in (dens, vel, pres)]
    traj = rollout_fn(d, v, p, ROLLOUT_STEPS)[0]
    grads = torch.autograd.grad((traj * w.to(traj.dtype).to(traj.device)).sum(), [d, v, p])
    return dict(zip(("dens", "vel", "pres"), grads))


def rollout_truth():
    if "rollout_truth" not in _CACHE:
        fields, w = rollout_inputs()
        _CACHE["rollout_truth"] = rollout_grads(
            lambda d, v, p, n: rollout(d, v, p, n, DT, DX), *fields, w)
    return _CACHE["rollout_truth"]


def rollout_floor():
    if "rollout_floor" not in _CACHE:
        fields, w = rollout_inputs(torch.float32)
        g32 = rollout_grads(lambda d, v, p, n: rollout(d, v, p, n, DT, DX), *fields, w)
        truth = rollout_truth()
        _CACHE["rollout_floor"] = max(rel_err(g32[k], truth[k]) for k in truth)
    return _CACHE["rollout_floor"]


# ------------------------------------------------------------------ 4D-Var twin experiment
TWIN_T, TWIN_ITERS, TWIN_LR = 4, 40, 5e-3
TWIN_OBS_VAR, TWIN_BG_VAR = 1e-4, 1e-2


def twin_problem(dtype, device):
    """(truth0, obsv_seq, weights, background, background_weights): the observations are the
    float64 restatement's rollout of the truth (density frames only carry weight)."""
    if "twin" not in _CACHE:
        (d, v, p), (db, vb) = twin_fields()
        ds, vs, ps = rollout(d, v, p, TWIN_T, DT, DX)
        _CACHE["twin"] = (torch.cat([d, v, p], 1), torch.cat([ds, vs, ps], 2),
                          torch.cat([db, vb, p], 1))
    truth0, obs, bg = [t.to(dtype).to(device) for t in _CACHE["twin"]]
    weights = torch.zeros(1, 1, 4, 1, 1, dtype=dtype, device=device)
    weights[:, :, 0] = 1.0 / TWIN_OBS_VAR
    bw = torch.full((1, 4, 1, 1), 1.0 / TWIN_BG_VAR, dtype=dtype, device=device)
    return truth0, obs, weights, bg, bw


def twin_run(fd, dtype, device):
    """Run the twin experiment with the FourDVar `fd` -> dict of host floats (read after the
    fit): J0, J, density error of the initial state before / after, min |velocity|."""
    truth0, obs, weights, bg, bw = twin_problem(dtype, device)
    res = fd.fit(obs, weights, bg, bw, iters=TWIN_ITERS, lr=TWIN_LR)
    assert res.history.shape == (TWIN_ITERS + 1, 3) and res.history.device == obs.device
    assert res.trajectory.shape == obs.shape and res.state0.shape == bg.shape
    hist = res.history.double().cpu()
    return dict(J0=float(hist[0, 0]), J=float(hist[-1, 0]),
                err0=float((bg[:, 0] - truth0[:, 0]).abs().mean()),
                err1=float((res.state0[:, 0] - truth0[:, 0]).abs().mean()),
                min_vel=float(res.trajectory[:, :, 1:3].abs().min()))


def twin_truth64():
    """The float64 CPU run of the twin experiment on the restatement (once per session)."""
    if "twin64" not in _CACHE:
        from pinn_kalman.fourdvar import FourDVar
        fd = FourDVar(steps_per_frame=1, dt=DT, dx=DX, step_fn=step_fn)
        _CACHE["twin64"] = twin_run(fd, torch.float64, torch.device("cpu"))
    return _CACHE["twin64"]


# ------------------------------------------------------------------ C ABI geometry refusals
BAD_GEOMETRIES = [(2, 1, 5), (2, 4, 1), (-1, 4, 5), (2, 65536, 32768)]  # (B, nx, ny)


def refused_geometries(dll, select):
    """Call every compute entry `int bpk_ns_*` of include/bpk.h whose name `select` accepts
    with each of BAD_GEOMETRIES and dummy non-NULL pointers (validation returns before a
    pointer or the device is touched): status 1 and a message naming the planes.
    -> the names called."""
    import re

    from op import _lib
    with open(_lib.HEADER_PATH) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    names = []
    for ret, name, args in _lib._PROTO_RE.findall(text):
        if ret != "int" or not name.startswith("bpk_ns_") or not select(name):
            continue
        params = [" ".join(a.split()) for a in args.split(",")]
        for B, nx, ny in BAD_GEOMETRIES:
            geo, vals = {"B": B, "nx": nx, "ny": ny}, []
            for prm in params:
                pname = prm.rsplit(" ", 1)[1]
                if pname == "stream":
                    vals.append(None)
                elif "*" in prm:
                    vals.append(1)
                elif pname in geo:
                    vals.append(geo[pname])
                else:  # dt, dx, scale; a plane stride; compat
                    vals.append(0.1 if prm.startswith("float") else 0)
            rc = getattr(dll, name)(*vals)
            assert rc == 1 and b"planes" in dll.bpk_last_error(), (name, B, nx, ny)
        names.append(name)
    return names

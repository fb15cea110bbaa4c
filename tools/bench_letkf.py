"""Time of one LETKF analysis (`op.letkf.analysis`, csrc/letkf.hip) at the simulator's shape:
192 x 192, C = 4, B = 1, for m in {16, 32, 64} members and R in {2, 4}, and of one forecast
step (`ns_step.full_step(compat=False)`) of the same ensemble for scale.  Two observation
patterns: "density" (channel 0 under a random half mask, sigma = 0.02 -- what
`fourdvar.observation_weights` gives for an inpainting mask) and "all" (every channel, every
pixel).  HIP-event times; after --warmup calls of every shape the configurations are visited
round-robin --reps times (so drift of the box hits all of them alike) and the medians reported.

Comparison basis: the same analysis composed from PyTorch ops on the same device -- unfold the
windows, einsum the m x m systems, batched `torch.linalg.eigh`, einsum the transform -- timed
the same way with --basis-reps visits; it is skipped, and the output says so, where it fails
(memory, an unsupported batch) or where one call took longer than --basis-budget seconds at a
smaller shape.  The basis is never an earlier state of the kernel.

With --obs-stride S [S ...] the same shapes are also timed through `op.letkf.analysis_obs`: the
density (channel 0) observed through a 5-tap Gaussian blur (`op.blur.blur2d`, variance 1) and
decimated at each stride S, under a random half mask on the observation grid, sigma = 0.02.  The
members' images yens are formed once outside the timed call (the time of that blur is reported
as observe_ms).  --obs-identity adds `analysis_obs` with yens = ens, stride 1 on the "density"
pattern: the work of `analysis` plus one launch.  These lines say "letkf.analysis_obs" and
carry no basis.

The kernel does not report its sweep count; with --ref-sweeps the float32 restatement
tests/letkf_ref.py (same rotation order and threshold, on the CPU) counts sweeps on a
12 x 12 crop of the same inputs.

Prints one JSON line per configuration and a last line with the device name.

    python tools/bench_letkf.py [--size 192] [--reps 20] [--warmup 3] [--basis-reps 3]
                                [--no-basis] [--ref-sweeps] [--obs-stride S [S ...]]
                                [--obs-identity] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-pinn-kalman-filter_amd"), os.path.join(REPO, "tests"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from op import letkf as K  # noqa: E402
from op import ns_step  # noqa: E402
from pinn_kalman import simulator  # noqa: E402


def make_inputs(size, m, pattern, dev):
    """A smooth 4-channel state, an ensemble of spread ~0.03 around it with errors correlated
    over a few pixels, and noisy observations of the state."""
    g = torch.Generator().manual_seed(1000 * m + size)
    y, x = torch.meshgrid(torch.linspace(0, 1, size), torch.linspace(0, 1, size), indexing="ij")
    base = torch.stack([torch.exp(-((x - 0.4) ** 2 + (y - 0.5) ** 2) / 0.05),
                        0.3 * torch.sin(6.28 * y), 0.3 * torch.cos(6.28 * x), 0.1 * x * y])

    def smooth(t):
        k = torch.tensor([1., 4., 6., 4., 1.]) / 16
        k2 = torch.outer(k, k)[None, None]
        flat = t.reshape(-1, 1, size, size)
        for _ in range(2):
            flat = F.conv2d(F.pad(flat, (2, 2, 2, 2), mode="reflect"), k2)
        return (flat / flat.std()).reshape(t.shape)
    pert = 0.03 * smooth(torch.randn(1, m, 4, size, size, generator=g))
    ens = (base[None, None] + pert - pert.mean(1, keepdim=True)).contiguous()
    sigma = 0.02
    obs = base[None] + sigma * torch.randn(1, 4, size, size, generator=g)
    prec = torch.zeros(1, 4, size, size)
    if pattern == "density":
        prec[:, 0] = (torch.rand(size, size, generator=g) < 0.5).float() / sigma ** 2
        obs[prec == 0] = float("nan")
    else:
        prec[:] = 1 / sigma ** 2
    return ens.to(dev), obs.to(dev), prec.to(dev)


def make_obs_inputs(size, m, stride, dev):
    """The ensemble of make_inputs(..., "density"), its density observed through a 5-tap
    Gaussian blur at `stride`: (ens, yens [1, m, 1, Hy, Wy], obs, prec [1, 1, Hy, Wy])."""
    from op import blur
    ens = make_inputs(size, m, "density", dev)[0]
    taps = blur.gaussian_taps(1.0, 5)
    g = torch.Generator().manual_seed(7000 * m + size + stride)
    yens = blur.blur2d(ens[0, :, 0:1].contiguous(), taps, stride).unsqueeze(0).contiguous()
    sigma = 0.02
    shape = (1,) + tuple(yens.shape[2:])
    obs = yens.mean(1) + (sigma * torch.randn(shape, generator=g)).to(dev)
    prec = ((torch.rand(shape, generator=g) < 0.5).float() / sigma ** 2).to(dev)
    obs[prec == 0] = float("nan")
    return ens, yens, obs, prec, taps


def composition(ens, obs, prec, taper, inflation):
    """The analysis from PyTorch ops: unfold + einsum + batched eigh."""
    B, m, C, H, W = ens.shape
    k = taper.shape[0]
    R, HW = k // 2, H * W
    xbar = ens.mean(1)
    dX = ens - xbar[:, None]
    dXu = F.unfold(dX.reshape(B, m * C, H, W), k, padding=R).view(B, m, C * k * k, HW)
    rho = F.unfold(prec, k, padding=R).view(B, C, k * k, HW) * taper.reshape(1, 1, k * k, 1)
    rho = rho.view(B, C * k * k, HW)
    innov = torch.where(prec != 0, obs - xbar, torch.zeros_like(xbar))
    innu = F.unfold(innov, k, padding=R)
    A = torch.einsum("bkjn,bjn,bljn->bnkl", dXu, rho, dXu)
    A = A + torch.eye(m, device=ens.device) * ((m - 1) / inflation)
    g = torch.einsum("bkjn,bjn->bnk", dXu, rho * innu)
    lam, Q = torch.linalg.eigh(A)
    z = torch.einsum("bnkl,bnk->bnl", Q, g) / lam
    wbar = torch.einsum("bnkl,bnl->bnk", Q, z)
    Wa = torch.einsum("bnkl,bnl,bnil->bnki", Q, math.sqrt(m - 1) / lam.sqrt(), Q)
    T = wbar[..., None] + Wa
    upd = torch.einsum("bkcn,bnki->bicn", dX.reshape(B, m, C, HW), T)
    return xbar[:, None] + upd.view(B, m, C, H, W)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--members", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--radii", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--patterns", nargs="+", default=["density", "all"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--basis-reps", type=int, default=3)
    ap.add_argument("--basis-budget", type=float, default=5.0)
    ap.add_argument("--no-basis", action="store_true")
    ap.add_argument("--ref-sweeps", action="store_true")
    ap.add_argument("--inflation", type=float, default=1.05)
    ap.add_argument("--obs-stride", type=int, nargs="*", default=[])
    ap.add_argument("--obs-identity", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")  # no fall-back: a timing needs the device
    cfgs = []
    for pattern in a.patterns:
        for m in a.members:
            data = make_inputs(a.size, m, pattern, dev)
            for R in a.radii:
                cfgs.append(dict(m=m, R=R, pattern=pattern, data=data,
                                 taper=K.gaspari_cohn_taper(R).to(dev), t=[], tf=[], tb=[],
                                 basis=None))
    no_basis = "not run (the basis restates the identity observation only)"
    for m in a.members:
        obs_data = [(s, "blur5") + make_obs_inputs(a.size, m, s, dev) for s in a.obs_stride]
        if a.obs_identity:
            ens, obs, prec = make_inputs(a.size, m, "density", dev)
            obs_data.append((1, "ens", ens, ens, obs, prec, None))
        for s, yname, ens, yens, obs, prec, taps in obs_data:
            for R in a.radii:
                cfgs.append(dict(m=m, R=R, pattern="density", data=(ens, yens, obs, prec),
                                 obs_stride=s, yens=yname, taps=taps,
                                 taper=K.gaspari_cohn_taper(R).to(dev), t=[], tf=[], tb=[], to=[],
                                 basis=no_basis))

    def analysis(c):
        if "obs_stride" in c:
            return K.analysis_obs(*c["data"], c["taper"], a.inflation, c["obs_stride"])
        return K.analysis(*c["data"], c["taper"], a.inflation)

    def observe(c):
        from op import blur
        return blur.blur2d(c["data"][0][0, :, 0:1].contiguous(), c["taps"], c["obs_stride"])

    def forecast(c):
        p = c["data"][0][0]
        return ns_step.full_step(p[:, 0:1].contiguous(), p[:, 1:3].contiguous(),
                                 p[:, 3:4].contiguous(), simulator.dt, simulator.dx, compat=False)

    for c in cfgs:
        for _ in range(a.warmup):
            out, status = analysis(c)
            forecast(c)
        torch.cuda.synchronize()
        c["flagged"] = int((status != 0).sum())
        c["finite"] = bool(torch.isfinite(out).all())
        c["out"] = out
    for _ in range(a.reps):
        for c in cfgs:
            c["t"].append(timed(lambda: analysis(c))[0])
            c["tf"].append(timed(lambda: forecast(c))[0])
            if c.get("taps") is not None:
                c["to"].append(timed(lambda: observe(c))[0])

    if not a.no_basis:
        # a small shape first: if one call there is already over budget, the full one is not tried
        small = make_inputs(48, 16, "all", dev)
        tp = K.gaspari_cohn_taper(2).to(dev)
        try:
            composition(*small, tp, a.inflation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            composition(*small, tp, a.inflation)
            torch.cuda.synchronize()
            probe = time.perf_counter() - t0
            scale = (a.size / 48) ** 2
        except Exception as e:  # the leg is optional; say why it is missing
            probe, scale = None, None
            for c in cfgs:
                c["basis"] = f"skipped: {type(e).__name__}: {str(e)[:120]}"
        for c in cfgs:
            if c["basis"] is not None:
                continue
            if probe * scale * (c["m"] / 16) ** 2 > a.basis_budget:  # m^2 entries per system at least
                c["basis"] = (f"skipped: {probe * 1e3:.0f} ms at 48 x 48, m = 16, R = 2 "
                              f"extrapolates past the budget of {a.basis_budget:.0f} s")
                continue
            try:
                ms, ref = timed(lambda: composition(*c["data"], c["taper"], a.inflation))  # warm
                if ms * 1e-3 > a.basis_budget:
                    c["basis"] = f"one call took {ms:.0f} ms; not repeated"
                    c["tb"] = [ms]
                ok = c["out"].isfinite() & ref.isfinite()
                c["basis_max_diff"] = float((c["out"] - ref)[ok].abs().max())
                del ref
            except Exception as e:
                c["basis"] = f"skipped: {type(e).__name__}: {str(e)[:120]}"
                torch.cuda.empty_cache()
        for _ in range(a.basis_reps):
            for c in cfgs:
                if c["basis"] is None:
                    c["tb"].append(timed(lambda: composition(*c["data"], c["taper"], a.inflation))[0])

    med = lambda v: round(statistics.median(v), 4)
    lines = []
    for c in cfgs:
        sites = a.size * a.size
        res = {"what": "letkf.analysis", "size": a.size, "C": 4, "m": c["m"], "R": c["R"],
               "pattern": c["pattern"], "analysis_ms": med(c["t"]),
               "analysis_ms_min": round(min(c["t"]), 4), "analysis_ms_max": round(max(c["t"]), 4),
               "us_per_grid_point": round(1e3 * statistics.median(c["t"]) / sites, 4),
               "forecast_step_ms": med(c["tf"]), "flagged": c["flagged"], "finite": c["finite"],
               "reps": a.reps}
        if "obs_stride" in c:
            res.update({"what": "letkf.analysis_obs", "obs_stride": c["obs_stride"],
                        "yens": c["yens"], "obs_grid": list(c["data"][1].shape[3:])})
            if c["to"]:
                res["observe_ms"] = med(c["to"])
        if a.no_basis and "obs_stride" not in c:
            res["basis"] = "not run (--no-basis)"
        elif c["tb"]:
            res["basis"] = {"what": "torch: unfold + einsum + batched linalg.eigh, same device",
                            "ms": med(c["tb"]), "reps": len(c["tb"]),
                            "note": c["basis"], "max_diff_vs_kernel": c.get("basis_max_diff")}
            res["speedup_vs_basis"] = round(statistics.median(c["tb"]) / statistics.median(c["t"]), 1)
        else:
            res["basis"] = c["basis"]
        if a.ref_sweeps and "obs_stride" not in c:
            import letkf_ref
            ens, obs, prec = (v[..., :12, :12].cpu().numpy() for v in c["data"])
            _, st, sw = letkf_ref.ref32(ens, obs, prec, c["taper"].cpu().numpy(), a.inflation, True)
            res["ref32_sweeps_12x12_crop"] = {"max": int(sw.max()), "median": float(np.median(sw)),
                                              "capped": int(st.sum())}
        lines.append(json.dumps(res))
    lines.append(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                             "hip": torch.version.hip}))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""GPU: the Winograd F(2x4,3x3) form of the 16-cin conv kernel (csrc/conv_winograd.hip
k16_item24, csrc/wino_f24.h) against a float64 direct convolution on the CPU, at the smallest
shapes that reach each of its code paths.  Bound: 1e-5 of max|ref|, the gate of every Winograd
op test (the form's own fp32 error is ~1.2e-6, tests/test_wino_f24_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_pick
from conftest import PKG, REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _first_conv_candidate(monkeypatch):
    """Every timed kernel choice of op.conv (tests/conv_pick.py) runs its first candidate in
    this module -- the Winograd kernels these tests are about -- with no timing and no choice
    inherited from an earlier test.  Both candidates of every choice against float64:
    tests/test_gpu_conv_pick.py."""
    conv_pick.first_only(monkeypatch)

TOL = 1e-5
NET_RTOL = 1e-4


def _inputs(N, cin, cout, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = F.silu(torch.randn(N, cin, H, W, generator=g))
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g)
    return x, w, b


def _ref(x, w, b=None, pre=None, skip=None, div=1.0):
    a = x.double()
    if pre is not None:
        a = F.silu(a * pre[..., 0].double()[:, :, None, None] + pre[..., 1].double()[:, :, None, None])
    y = F.conv2d(a, w.double(), None if b is None else b.double(), padding=1)
    if skip is not None:
        y = (skip.double() + y) / div
    return y


def _check(out, ref, what):
    from op import conv as conv_op
    assert conv_op.last_form == 24, f"{what}: ran the {conv_op.last_form}-point form"
    scale = ref.abs().max().item()
    err = (out.double().cpu() - ref).abs().max().item()
    print(f"{what}: max err / max|ref| = {err / scale:.3e}")
    assert err <= TOL * scale, f"{what}: {err / scale:.3e}"


def _check_stats(out, what):
    """the epilogue's GroupNorm partials vs the statistics of the returned output itself"""
    from op.conv import gn_partials
    part, R, cnt = gn_partials(out)
    N, C, H, W = out.shape
    assert R == (H // 8) * (W // 16) and cnt == 128
    o = out.double().reshape(N, C, H // 8, 8, W // 16, 16)
    m = o.mean((3, 5), keepdim=True)
    m2 = ((o - m) ** 2).sum((3, 5)).reshape(N, C, R)
    m = m.reshape(N, C, R)
    scale = out.abs().max().item()
    assert (part[..., 0].double() - m).abs().max().item() <= TOL * scale, what
    assert (part[..., 1].double() - m2).abs().max().item() <= TOL * m2.max().item(), what


@pytest.mark.parametrize("N,cin,cout,H,W", [
    (1, 16, 128, 8, 16),    # one chunk, one region: prologue-only pipeline, all four borders
    (2, 32, 128, 8, 16),    # two chunks: both LDS buffers, U refill across the chunk edge
    (1, 48, 256, 16, 32),   # odd chunk count (tail step), two cout blocks, interior halos
])
def test_f24_plain_conv(hip, N, cin, cout, H, W):
    from op.conv import conv3x3_fwd_raw
    x, w, b = _inputs(N, cin, cout, H, W)
    with torch.no_grad():
        out = conv3x3_fwd_raw(x.to(hip), w.to(hip))
    _check(out, _ref(x, w), f"plain {cin}->{cout} {H}x{W}")


@pytest.mark.parametrize("form", ["bias", "pre", "skip", "stats", "all"])
def test_f24_epilogue_and_prologue_forms(hip, form):
    from op.conv import conv3x3_fwd_raw
    N, cin, cout, H, W = 2, 32, 128, 16, 32
    x, w, b = _inputs(N, cin, cout, H, W, seed=1)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, cin, H, W, generator=g) * 2 + 0.5 if form in ("pre", "all") else x
    pre = torch.stack([torch.rand(N, cin, generator=g) + 0.5, torch.randn(N, cin, generator=g)], -1) \
        if form in ("pre", "all") else None
    skip = torch.randn(N, cout, H, W, generator=g) * 3 + 1 if form in ("skip", "all") else None
    div = 2 ** 0.5 if skip is not None else 1.0
    bias = None if form in ("pre", "skip", "stats") else b
    stats = form in ("stats", "all")
    with torch.no_grad():
        out = conv3x3_fwd_raw(x.to(hip), w.to(hip), None if bias is None else bias.to(hip),
                              skip=None if skip is None else skip.to(hip), div=div,
                              pre=None if pre is None else pre.to(hip), stats=stats)
    _check(out, _ref(x, w, bias, pre, skip, div), f"form {form}")
    if stats:
        _check_stats(out, f"form {form}")


def test_f24_two_sources_with_prologue(hip):
    """the source switch mid-walk: channels [0, 16) from x, [16, 48) from x2"""
    from op.conv import conv3x3_fwd_raw
    N, cin, cout, H, W = 2, 48, 128, 16, 32
    _, w, b = _inputs(N, cin, cout, H, W, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, cin, H, W, generator=g) * 2 + 0.5
    pre = torch.stack([torch.rand(N, cin, generator=g) + 0.5, torch.randn(N, cin, generator=g)], -1)
    with torch.no_grad():
        out = conv3x3_fwd_raw(x[:, :16].contiguous().to(hip), w.to(hip), b.to(hip),
                              pre=pre.to(hip), x2=x[:, 16:].contiguous().to(hip))
    _check(out, _ref(x, w, b, pre), "two sources")


def test_f24_nearest_up2(hip):
    """half-resolution patch addressing, through conv3x3_up2"""
    from op.conv import conv3x3_up2
    x, w, b = _inputs(1, 32, 128, 8, 16, seed=5)
    with torch.no_grad():
        out = conv3x3_up2(x.to(hip), w.to(hip), b.to(hip))
    _check(out, _ref(F.interpolate(x, scale_factor=2, mode="nearest"), w, b), "up2")


@pytest.mark.parametrize("c", [128, 256])
def test_f24_split_k(hip, c):
    """N = 1 at 16 x 16: ksplit > 1 and the reduce kernel, with the residual tail and stats"""
    from op._lib import lib
    from op.conv import conv3x3_fwd_raw
    N, H, W = 1, 16, 16
    assert lib.bpk_conv3x3_wino_splitk_bytes(N, c, c, c, H, W) > 0
    x, w, b = _inputs(N, c, c, H, W, seed=6)
    skip = torch.randn(N, c, H, W, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        out = conv3x3_fwd_raw(x.to(hip), w.to(hip), b.to(hip), skip=skip.to(hip), div=2 ** 0.5,
                              stats=True)
    _check(out, _ref(x, w, b, None, skip, 2 ** 0.5), f"split-K {c}")
    _check_stats(out, f"split-K {c}")


def test_f24_persistent_walk(hip):
    """320 items on at most one workgroup per CU: the item loop, the XCD remap and the
    barrier between items"""
    from op.conv import conv3x3_fwd_raw
    x, w, b = _inputs(5, 16, 256, 64, 64, seed=8)
    with torch.no_grad():
        out = conv3x3_fwd_raw(x.to(hip), w.to(hip), b.to(hip), stats=True)
    _check(out, _ref(x, w, b), "persistent walk")
    _check_stats(out, "persistent walk")


_CHILD = """
import sys
import numpy as np
import torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from op import conv as conv_op
d = np.load(sys.argv[3])
dev = torch.device("cuda:0")
with torch.no_grad():
    y = conv_op.conv3x3_fwd_raw(torch.tensor(d["x"], device=dev), torch.tensor(d["w"], device=dev),
                                torch.tensor(d["b"], device=dev))
np.save(sys.argv[4], y.cpu().numpy())
print("form", conv_op.last_form)
"""


def test_f24_switch_off_in_a_fresh_process(hip, tmp_path, monkeypatch):
    """BPK_WINO_F24=0 (read at import): the same conv runs the 16-point form and gives the
    16-point result of this process"""
    from op import conv as conv_op
    x, w, b = _inputs(2, 32, 128, 16, 32, seed=9)
    np.savez(tmp_path / "in.npz", x=x.numpy(), w=w.numpy(), b=b.numpy())
    p = subprocess.run([sys.executable, "-c", _CHILD, PKG, REPO, str(tmp_path / "in.npz"),
                        str(tmp_path / "out.npy")], env=dict(os.environ, BPK_WINO_F24="0"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "form 16" in p.stdout
    child = torch.tensor(np.load(tmp_path / "out.npy"))
    ref = _ref(x, w, b)
    scale = ref.abs().max().item()
    assert (child.double() - ref).abs().max().item() <= TOL * scale
    monkeypatch.setattr(conv_op, "_F24", False)
    with torch.no_grad():
        y16 = conv_op.conv3x3_fwd_raw(x.to(hip), w.to(hip), b.to(hip)).cpu()
    assert conv_op.last_form == 16
    assert (child - y16).abs().max().item() <= TOL * scale
    monkeypatch.setattr(conv_op, "_F24", True)
    with torch.no_grad():
        y24 = conv_op.conv3x3_fwd_raw(x.to(hip), w.to(hip), b.to(hip)).cpu()
    assert conv_op.last_form == 24
    assert (y24 - y16).abs().max().item() <= TOL * scale


def test_f24_bench_model_matches_16_point_path(hip, monkeypatch):
    """The full 128 x 128 benchmark network at B = 2: 24-point convs vs the 16-point path of
    the same process (NET_RTOL of max|ref|), with the 24-point kernel counted by op.flops."""
    from bench import build_model
    from op import conv as conv_op
    from op import flops
    c, model = build_model(hip)
    model.eval()
    g = torch.Generator().manual_seed(10)
    x = torch.rand(2, 1, 128, 128, generator=g).to(hip)
    t = (torch.tensor([0.3, 0.9]) * 999).to(hip)
    with torch.no_grad():
        with flops.counting(aten=False) as tally:
            y24 = model(x, t)
        monkeypatch.setattr(conv_op, "_F24", False)
        with flops.counting(aten=False) as tally16:
            y16 = model(x, t)
    kinds, kinds16 = tally.summary()["native"], tally16.summary()["native"]
    assert kinds["wino_fwd24"]["launches"] > 0 and "wino_fwd24" not in kinds16
    assert kinds["wino_fwd24"]["executed"] == pytest.approx(kinds["wino_fwd24"]["direct"] / 3)
    scale = max(1.0, y16.abs().max().item())
    err = (y24 - y16).abs().max().item()
    print(f"bench model 24 vs 16 points: {err / scale:.3e}")
    assert err <= NET_RTOL * scale


def test_f24_pc_graph_equals_eager_and_refreshes_filters(hip):
    """3 PC steps of the bench config (B = 2) from one prior: step graph on == eager, bit for
    bit -- the graph reads the registered U24 transforms (conv.static_filters) -- and again
    after every conv weight has changed in place (refresh_filters rewrites the U24s)."""
    import sampling
    import sde_lib
    from bench import build_model
    c, model = build_model(hip)
    model.eval()
    sde = sde_lib.VPSDE(c.model.beta_min, c.model.beta_max, c.model.num_scales)
    prior = torch.randn(2, 1, 128, 128, generator=torch.Generator().manual_seed(5))
    w0 = [p.detach().clone() for p in model.parameters()]
    outs = []
    for use_graph in (True, False):
        with torch.no_grad():
            for p, v in zip(model.parameters(), w0):
                p.copy_(v)
        eng = sampling.PCEngine(sde, (2, 1, 128, 128), sampling.EulerMaruyamaPredictor,
                                sampling.LangevinCorrector, c.sampling.snr, 1, continuous=True,
                                device=hip, seed=1234, use_graph=use_graph)
        eng.reset(model, x_init=prior)
        eng.advance(3)
        first = eng._xm.clone()
        if use_graph:
            assert eng.graph is not None, getattr(eng, "capture_error", None)
            assert any(e[4] == 24 for e in eng._filters)
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() == 4:  # the conv weights (as EMA copy_to rewrites them)
                    p.mul_(1.05)
        eng.advance(2)
        torch.cuda.synchronize()
        outs.append((first, eng._xm.clone()))
        del eng
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[0][1])

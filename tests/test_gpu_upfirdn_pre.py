"""upfirdn2d with GroupNorm + SiLU applied while loading (bpk_upfirdn2d_pre_f32,
op.upfirdn2d.upfirdn2d_pre): the kernel convolves silu(x * s + t), and a tap outside the plane
contributes 0 -- zero AFTER the activation, not silu(t).

Reference: oracle.upfirdn2d_ref.upfirdn2d_np on float64 silu(x * s + t).  The table has shift
t = 1 (silu(1) = 0.73: an activated padding tap would show at every border and corner) and
scales of both signs.  Gate: the existing upfirdn2d GPU tests' 2e-6 x max(1, max |ref|).

Shapes: per kernel template that gained a PRE form, the smallest H = W (rows of 4 k floats) at
which the dispatcher (bpk_upfirdn2d_pre_f32, as try_stream / try_roll) selects it, plus one
shape that fills the segment and spans several strips:
  up 2, pad (2, 1): upfirdn2d_stream<2, 1, 2, 16, SEGW, 4, false, true>, SEGW by out_w / 4 lanes
  down 2, pad (1, 1): upfirdn2d_roll<2, 1, SEGW, 2, false, 0, true>, SEGW by out_w / 2 lanes
"""
import numpy as np
import pytest
import torch

from oracle.upfirdn2d_ref import upfirdn2d_np

pytestmark = pytest.mark.gpu

K = np.outer([1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 3.0, 1.0]) / 64.0
CASES = {
    # up 2: out_w = 2 W, lanes = out_w / 4
    "up_stream_seg8_W4": ("up", 4),        # 2 lanes of an 8-lane segment
    "up_stream_seg8_W16": ("up", 16),      # the segment full, 2 strips of 16 rows
    "up_stream_seg16_W20": ("up", 20),     # 10 lanes: first width past 8
    "up_stream_seg32_W36": ("up", 36),     # 18 lanes: first width past 16
    "up_stream_seg64_W68": ("up", 68),     # 34 lanes: first width past 32
    # down 2: out_w = W / 2, lanes = out_w / 2
    "down_roll_seg8_W4": ("down", 4),      # one lane
    "down_roll_seg8_W32": ("down", 32),    # the segment full
    "down_roll_seg16_W36": ("down", 36),   # 9 lanes: first width past 8
    "down_roll_seg32_W68": ("down", 68),   # 17 lanes: first width past 16
    "down_roll_seg64_W132": ("down", 132),  # 33 lanes: first width past 32
}


def _args(kind):
    if kind == "up":
        return dict(up=2, down=1, pad=(2, 1)), 4.0 * K, ((2, 2), (1, 1), (2, 1, 2, 1))
    return dict(up=1, down=2, pad=(1, 1)), K, ((1, 1), (2, 2), (1, 1, 1, 1))


def _table(N, C, seed):
    """(s, t): t = 1 everywhere, |s| in [0.5, 1.5] with both signs"""
    g = torch.Generator().manual_seed(seed)
    s = (torch.rand(N, C, generator=g) + 0.5) * torch.where(torch.rand(N, C, generator=g) < 0.5,
                                                            -1.0, 1.0)
    s[0, 0], s[-1, -1] = 1.25, -1.25
    return torch.stack([s, torch.ones(N, C)], -1).contiguous()


def _ref(x, pre, kind):
    _, k, (up, down, pad) = _args(kind)
    z = x.double() * pre[..., 0].double()[:, :, None, None] + pre[..., 1].double()[:, :, None, None]
    a = z * torch.sigmoid(z)
    return upfirdn2d_np(a.numpy(), k, up, down, pad)


@pytest.mark.parametrize("C", [3, 16])
@pytest.mark.parametrize("name", list(CASES))
def test_upfirdn2d_pre_matches_float64_activation_then_fir(hip, name, C):
    from op.upfirdn2d import upfirdn2d_pre, upfirdn2d_pre_supported
    kind, W = CASES[name]
    kw, k, _ = _args(kind)
    g = torch.Generator().manual_seed(W * 7 + C)
    x = torch.randn(2, C, W, W, generator=g)
    pre = _table(2, C, W + C)
    kt = torch.tensor(k, dtype=torch.float32, device=hip)
    assert upfirdn2d_pre_supported(x.to(hip), kt, pre.to(hip), **kw)
    y = upfirdn2d_pre(x.to(hip), pre.to(hip), kt, **kw).cpu().numpy()
    ref = _ref(x, pre, kind)
    assert y.shape == ref.shape
    err = np.abs(y - ref)
    gate = 2e-6 * max(1.0, float(np.abs(ref).max()))
    border = max(err[..., 0, :].max(), err[..., -1, :].max(), err[..., :, 0].max(),
                 err[..., :, -1].max())
    print(f"{name} C={C}: worst error {err.max():.3e} (borders {border:.3e}), gate {gate:.3e}")
    assert err.max() <= gate


def test_upfirdn2d_pre_empty_batch(hip):
    from op.upfirdn2d import upfirdn2d_pre
    for kind, shape in (("up", (0, 3, 16, 16)), ("down", (0, 3, 4, 4))):
        kw, k, _ = _args(kind)
        y = upfirdn2d_pre(torch.zeros(0, 3, 8, 8, device=hip), torch.zeros(0, 3, 2, device=hip),
                          torch.tensor(k, dtype=torch.float32, device=hip), **kw)
        assert tuple(y.shape) == shape


def test_unsupported_form_is_refused_and_the_block_falls_back(hip):
    """A row length that is no multiple of 4 has no PRE form: the query says so, the op raises,
    and the resample block takes the materialised-activation path (same result as with the
    switch off, no raise)."""
    import models.layerspp as lpp
    from op.upfirdn2d import upfirdn2d_pre, upfirdn2d_pre_supported
    kw, k, _ = _args("up")
    kt = torch.tensor(k, dtype=torch.float32, device=hip)
    x = torch.randn(2, 32, 10, 10, generator=torch.Generator().manual_seed(1)).to(hip)
    pre = _table(2, 32, 5).to(hip)
    assert not upfirdn2d_pre_supported(x, kt, pre, **kw)
    assert not upfirdn2d_pre_supported(x[:, :, :8, :8].contiguous(), kt, pre, up=1, down=1, pad=(2, 2))
    with pytest.raises(RuntimeError):
        upfirdn2d_pre(x, pre, kt, **kw)
    torch.manual_seed(2)
    blk = lpp.ResnetBlockBigGANpp(act=torch.nn.SiLU(), in_ch=32, out_ch=32, temb_dim=64, up=True,
                                  fir=True, skip_rescale=True, init_scale=1.).to(hip).eval()
    temb = torch.randn(2, 64, generator=torch.Generator().manual_seed(3)).to(hip)
    with torch.no_grad():
        got = blk(x, temb)
        old = lpp._FIR_PRE
        lpp._FIR_PRE = False
        try:
            want = blk(x, temb)
        finally:
            lpp._FIR_PRE = old
    assert torch.equal(got, want)

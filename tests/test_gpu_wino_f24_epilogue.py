"""GPU: the epilogue of the Winograd F(2x4,3x3) 16-cin kernel (csrc/conv_winograd.hip
k16_item24) with the couts on the MFMA's rows: lane (kq, 4 tty + ttx), register r owns tile
(tty, ttx) of cout 16 wave + 4 kq + r, and the GroupNorm records are chained inside a quad.

Shapes: the smallest at which that indexing can go wrong -- N = 2, one region (8 x 16) and
2 x 2 regions (16 x 32), one and two cout blocks (128, 256), an even chunk count (Cin = 32, the
kernel's TAILK form) and an odd one (Cin = 48).  Every output against a float64 direct
convolution at 1e-5 of max|ref|, the gate of every Winograd op test; every record against the
float64 (mean, M2) of the stored output at the tolerance of tests/test_gpu_wino_f24.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_pick

pytestmark = pytest.mark.gpu

TOL = 1e-5
SHAPES = [(H, W, cout, cin) for (H, W) in ((8, 16), (16, 32)) for cout in (128, 256)
          for cin in (32, 48)]
N = 2


@pytest.fixture(autouse=True)
def _first_conv_candidate(monkeypatch):
    """the Winograd candidate of every timed choice (tests/conv_pick.py), with no timing"""
    conv_pick.first_only(monkeypatch)


@functools.lru_cache(maxsize=None)
def _case(H, W, cout, cin):
    """inputs of one shape and the float64 convolutions every form's reference starts from
    (computed once, never written to)"""
    g = torch.Generator().manual_seed(1000 * cin + cout + H)
    x = torch.randn(N, cin, H, W, generator=g) * 2 + 0.5
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 2
    pre = torch.stack([torch.rand(N, cin, generator=g) + 0.5, torch.randn(N, cin, generator=g)], -1)
    skip = torch.randn(N, cout, H, W, generator=g) * 3 + 1  # unrelated to the output
    xh = torch.randn(N, cin, H // 2, W // 2, generator=g)
    a = F.silu(x.double() * pre[..., 0].double()[:, :, None, None]
               + pre[..., 1].double()[:, :, None, None])
    return dict(x=x, w=w, b=b, pre=pre, skip=skip, xh=xh,
                plain=F.conv2d(x.double(), w.double(), None, padding=1),
                pre_conv=F.conv2d(a, w.double(), None, padding=1),
                up=F.conv2d(F.interpolate(xh.double(), scale_factor=2, mode="nearest"),
                            w.double(), None, padding=1))


def _bias(ref, b):
    return ref + b.double()[None, :, None, None]


def _check(out, ref, what):
    from op import conv as conv_op
    assert conv_op.last_form == 24, f"{what}: ran the {conv_op.last_form}-point form"
    scale = ref.abs().max().item()
    err = (out.double().cpu() - ref).abs().max().item()
    print(f"{what}: max err / max|ref| = {err / scale:.3e}")
    assert err <= TOL * scale, f"{what}: {err / scale:.3e}"


def _check_records(out, what):
    """the (mean, M2) record of every (image, cout, region) against float64 statistics of the
    128 stored values it covers"""
    from op.conv import gn_partials
    part, R, cnt = gn_partials(out)
    n, C, H, W = out.shape
    assert R == (H // 8) * (W // 16) and cnt == 128 and tuple(part.shape) == (n, C, R, 2)
    o = out.double().cpu().reshape(n, C, H // 8, 8, W // 16, 16)
    m = o.mean((3, 5), keepdim=True)
    m2 = ((o - m) ** 2).sum((3, 5)).reshape(n, C, R)
    m = m.reshape(n, C, R)
    part = part.double().cpu()
    scale = out.abs().max().item()
    em = (part[..., 0] - m).abs().max().item()
    e2 = (part[..., 1] - m2).abs().max().item()
    print(f"{what}: record mean err {em / scale:.3e} of max|y|, M2 err {e2 / m2.max().item():.3e}")
    assert em <= TOL * scale, what
    assert e2 <= TOL * m2.max().item(), what


def _ids(s):
    return "%dx%d-cout%d-cin%d" % s


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_plain(hip, shape):
    from op.conv import conv3x3_fwd_raw
    c = _case(*shape)
    with torch.no_grad():
        out = conv3x3_fwd_raw(c["x"].to(hip), c["w"].to(hip))
    _check(out, c["plain"], f"plain {_ids(shape)}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_prologue_with_bias(hip, shape):
    from op.conv import conv3x3_fwd_raw
    c = _case(*shape)
    with torch.no_grad():
        out = conv3x3_fwd_raw(c["x"].to(hip), c["w"].to(hip), c["b"].to(hip), pre=c["pre"].to(hip))
    _check(out, _bias(c["pre_conv"], c["b"]), f"pre + bias {_ids(shape)}")


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_residual_tail(hip, shape, pre):
    """(skip + (conv + bias)) / sqrt 2: the skip loads have the stores' addresses"""
    from op.conv import conv3x3_fwd_raw
    c = _case(*shape)
    div = 2 ** 0.5
    with torch.no_grad():
        out = conv3x3_fwd_raw(c["x"].to(hip), c["w"].to(hip), c["b"].to(hip),
                              skip=c["skip"].to(hip), div=div,
                              pre=c["pre"].to(hip) if pre else None)
    ref = (c["skip"].double() + _bias(c["pre_conv" if pre else "plain"], c["b"])) / div
    _check(out, ref, f"residual tail {_ids(shape)}")


@pytest.mark.parametrize("form", ["bias", "pre_skip"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_statistics_records(hip, shape, form):
    """records of a biased output (every cout its own mean), and of the sampler's form:
    prologue, bias, residual tail and statistics in one launch"""
    from op.conv import conv3x3_fwd_raw
    c = _case(*shape)
    full = form == "pre_skip"
    div = 2 ** 0.5 if full else 1.0
    with torch.no_grad():
        out = conv3x3_fwd_raw(c["x"].to(hip), c["w"].to(hip), c["b"].to(hip),
                              skip=c["skip"].to(hip) if full else None, div=div,
                              pre=c["pre"].to(hip) if full else None, stats=True)
    ref = _bias(c["pre_conv" if full else "plain"], c["b"])
    if full:
        ref = (c["skip"].double() + ref) / div
    _check(out, ref, f"stats {form} {_ids(shape)}")
    _check_records(out, f"stats {form} {_ids(shape)}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_two_sources(hip, shape):
    """channels [0, 16) from x, the rest from x2, with the prologue and statistics"""
    from op.conv import conv3x3_fwd_raw
    c = _case(*shape)
    with torch.no_grad():
        out = conv3x3_fwd_raw(c["x"][:, :16].contiguous().to(hip), c["w"].to(hip), c["b"].to(hip),
                              pre=c["pre"].to(hip), x2=c["x"][:, 16:].contiguous().to(hip),
                              stats=True)
    _check(out, _bias(c["pre_conv"], c["b"]), f"two sources {_ids(shape)}")
    _check_records(out, f"two sources {_ids(shape)}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_up_form(hip, shape):
    """conv of the nearest x2 upsample of a half-resolution input"""
    from op.conv import conv3x3_up2
    c = _case(*shape)
    with torch.no_grad():
        out = conv3x3_up2(c["xh"].to(hip), c["w"].to(hip), c["b"].to(hip))
    _check(out, _bias(c["up"], c["b"]), f"up {_ids(shape)}")


@pytest.mark.parametrize("cout", [128, 256])
def test_split_k_workspace(hip, cout):
    """128 input channels at 16 x 16, N = 2: the split-K rule slices the chunks, so the kernel
    writes raw partial slabs (ks_idx in the store address) and the reduce kernel finishes"""
    from op._lib import lib
    from op.conv import conv3x3_fwd_raw
    cin, H, W = 128, 16, 16
    assert lib.bpk_conv3x3_wino_splitk_bytes(N, cin, cin, cout, H, W) > 0
    g = torch.Generator().manual_seed(77 + cout)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 2
    skip = torch.randn(N, cout, H, W, generator=g) * 3 + 1
    with torch.no_grad():
        out = conv3x3_fwd_raw(x.to(hip), w.to(hip), b.to(hip), skip=skip.to(hip), div=2 ** 0.5,
                              stats=True)
    ref = (skip.double() + F.conv2d(x.double(), w.double(), b.double(), padding=1)) / 2 ** 0.5
    _check(out, ref, f"split-K cout {cout}")
    _check_records(out, f"split-K cout {cout}")


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
def test_lane_to_output_mapping(hip, pre):
    """Cin = Cout = 128, the filter's centre tap the identity: output plane c is input plane c.
    The input is c + (pixel index) + n / 2, so a cout, tile, row or image permutation is an
    error of at least 1/2 against a rounding error of 1e-5 * 640; the records of the planes are
    those of the pixel ramp shifted by c."""
    from op.conv import conv3x3_fwd_raw
    C, H, W = 128, 16, 32
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    x = (torch.arange(C, dtype=torch.float32)[None, :, None, None]
         + torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
         + 0.5 * torch.arange(N, dtype=torch.float32)[:, None, None, None]).contiguous()
    # with the prologue: scale 1, shift 40, so silu(x + 40) == x + 40 in float32 (x >= 0)
    p = torch.tensor([1.0, 40.0]).expand(N, C, 2).contiguous() if pre else None
    with torch.no_grad():
        out = conv3x3_fwd_raw(x.to(hip), w.to(hip), pre=None if p is None else p.to(hip),
                              stats=True)
    ref = x.double() + (40.0 if pre else 0.0)
    err = (out.double().cpu() - ref).abs()
    bad = (err > 0.25).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} outputs in the wrong place, first (n, cout, y, x) = "
                              f"{bad[0].tolist()}: got {out[tuple(bad[0])].item()}, "
                              f"want {ref[tuple(bad[0])].item()}")
    _check(out, ref, "mapping")
    _check_records(out, "mapping")

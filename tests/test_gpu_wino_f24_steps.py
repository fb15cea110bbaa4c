"""GPU: the chunk loop of the Winograd F(2x4,3x3) kernel (csrc/conv_winograd.hip k16_item24,
`step`): the two-step loop body (6 or more chunks per workgroup), the odd-count loop with its
last step (5 or more) and the peeled tail steps behind a loop that has run -- the schedules the
other F(2x4) tests, which stop at 4 chunks, never execute.

Chunks per workgroup = Cin / 16 / S, S the library's split-K factor.  A launch of at most half
as many items as CUs whose chunk count is even is split (wino_splits), so the one-image shapes
run Cin = 80, 96, 112, 128, 160 as 5, 3, 7, 2 and 5 chunks per slice; the same shapes at N = 129
(129 items: not split, one item per workgroup) run 5, 6, 7, 8 and 10: the odd loop once with
its last step, the even (TAILK) loop once, the odd loop twice, the even loop twice and three
times.  Each case is checked against the float64 direct convolution at 1e-5 of max|ref| (the
gate of every Winograd op test; the form measures 1e-7 - 1.2e-6), its statistics records against
float64 (mean, M2) of the stored output, and bit for bit against a second run of itself."""
import pytest
import torch

import conv_pick
from test_gpu_wino_f24 import _check, _check_stats, _inputs, _ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _first_conv_candidate(monkeypatch):
    """the small images here reach a timed choice of op.conv: run its first candidate, the
    Winograd kernel (tests/conv_pick.py), as tests/test_gpu_wino_f24.py does"""
    conv_pick.first_only(monkeypatch)


def _case(N, cin, cout, H, W, seed, pre=False, skip=False, c1=None):
    x, w, b = _inputs(N, cin, cout, H, W, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    d = dict(x=x, w=w, b=b, pre=None, skip=None, div=1.0, c1=c1)
    if pre:  # a different (s, t) per image and channel
        d["x"] = torch.randn(N, cin, H, W, generator=g) * 2 + 0.5
        d["pre"] = torch.stack([torch.rand(N, cin, generator=g) + 0.5,
                                torch.randn(N, cin, generator=g)], -1)
    if skip:
        d["skip"] = torch.randn(N, cout, H, W, generator=g) * 3 + 1
        d["div"] = 2 ** 0.5
    return d


def _run(hip, d, stats, lo=None, hi=None):
    """the conv of images [lo, hi) of case d -> (output, its statistics partials or None)"""
    from op.conv import conv3x3_fwd_raw, gn_partials
    s = slice(lo, hi)
    dev = lambda t: None if t is None else t[s].contiguous().to(hip)  # noqa: E731
    x, c1 = d["x"], d["c1"]
    kw = {}
    if c1 is not None:
        kw["x2"] = x[s, c1:].contiguous().to(hip)
        x = x[:, :c1]
    with torch.no_grad():
        out = conv3x3_fwd_raw(x[s].contiguous().to(hip), d["w"].to(hip),
                              None if d["b"] is None else d["b"].to(hip), skip=dev(d["skip"]),
                              div=d["div"], pre=dev(d["pre"]), stats=stats, **kw)
    return out, (gn_partials(out)[0].clone() if stats else None)


def _chunks(d):
    """chunks per workgroup of case d's launch, by the library's own split rule"""
    from op._lib import lib
    N, cin, H, W = d["x"].shape
    cout = d["w"].shape[0]
    c1 = cin if d["c1"] is None else d["c1"]
    nbytes = lib.bpk_conv3x3_wino_splitk_bytes(N, cin, c1, cout, H, W)
    S = max(1, nbytes // (N * cout * H * W * 4))
    return cin // 16 // S


def _check_twice(hip, d, what, stats):
    out, part = _run(hip, d, stats)
    _check(out, _ref(d["x"], d["w"], d["b"], d["pre"], d["skip"], d["div"]), what)
    if stats:
        _check_stats(out, what)
    again, part2 = _run(hip, d, stats)
    assert torch.equal(out, again), f"{what}: two runs differ"
    if stats:
        assert torch.equal(part, part2), f"{what}: statistics of two runs differ"
    return out, part


# N = 1: the launch is split where the rule says so; N = 129: never, so nch = Cin / 16
CHUNKS = {(1, 80): 5, (1, 96): 3, (1, 112): 7, (1, 128): 2, (1, 160): 5,
          (129, 80): 5, (129, 96): 6, (129, 112): 7, (129, 128): 8, (129, 160): 10}


@pytest.mark.parametrize("form", ["plain", "all"])
@pytest.mark.parametrize("cin", [80, 96, 112, 128, 160])
@pytest.mark.parametrize("N", [1, 129])
def test_steps_chunk_counts(hip, N, cin, form):
    """Cout = 128 at 8 x 16: one region per image, all four borders.  plain: the kernel's
    form without the prologue; all: prologue + bias + residual tail + statistics."""
    full = form == "all"
    d = _case(N, cin, 128, 8, 16, seed=40 + cin + N, pre=full, skip=full)
    if not full:
        d["b"] = None
    assert _chunks(d) == CHUNKS[N, cin]
    _check_twice(hip, d, f"steps N={N} {cin}->128 {form} ({CHUNKS[N, cin]} chunks)", stats=full)


@pytest.mark.parametrize("c1", [48, 32])
def test_steps_two_sources_switch_inside_the_loop(hip, c1):
    """Cin = 96 as channels [0, c1) from x and [c1, 96) from x2, Cout = 256 (two cout blocks) at
    16 x 32, N = 17 (136 items: six chunks per workgroup, not split): the source changes at
    chunk 3, between the loop's two steps, and at chunk 2, inside the pair"""
    d = _case(17, 96, 256, 16, 32, seed=60 + c1, pre=True, c1=c1)
    assert _chunks(d) == 6
    _check_twice(hip, d, f"steps two sources C1={c1}", stats=True)


def test_steps_two_items_per_workgroup(hip):
    """N = 5, 96 -> 128 at 64 x 128, prologue + statistics: 320 items of six chunks, so 64
    workgroups walk two items with the filter carried and the table kept or reloaded.  Bit for
    bit against launches of three images (192 items, one per workgroup, the same arithmetic: a
    launch of one image, 64 items, would be split into two K slices and sum in another order);
    the float64 check of _check_twice covers every image, image 0 among them."""
    d = _case(5, 96, 128, 64, 128, seed=70, pre=True)
    assert _chunks(d) == 6
    out, part = _check_twice(hip, d, "steps N=5 96->128 64x128", stats=True)
    from op._lib import lib
    assert lib.bpk_conv3x3_wino_splitk_bytes(3, 96, 96, 128, 64, 128) == 0
    for lo in (0, 2):
        sub, psub = _run(hip, d, True, lo, lo + 3)
        assert torch.equal(out[lo:lo + 3], sub), f"images {lo}..{lo + 2} differ from their launch"
        assert torch.equal(part[lo:lo + 3], psub), f"statistics of images {lo}..{lo + 2}"

"""GPU: the item boundary of the Winograd F(2x4,3x3) kernel (csrc/conv_winograd.hip k16_item24):
the ordered prologue, the peeled tail steps, the filter k-steps fetched for the workgroup's next
item and the GroupNorm table kept while the image stays the same.

Small shapes give fewer items than CUs, so every workgroup runs one item and none of that code
runs.  These are the smallest shapes with more than 256 items (one workgroup per CU walks 2 or 3
of them).  Each case is checked against the float64 direct convolution (1e-5 of max|ref|, the
gate of every Winograd op test), bit for bit against the same call made per image (N = 1: at
most 256 items, one per workgroup; Cin <= 48 is never split, so both sides run the same
arithmetic) and bit for bit against a second run of itself."""
import pytest
import torch

from test_gpu_wino_f24 import _check, _check_stats, _inputs, _ref

pytestmark = pytest.mark.gpu

H, W = 64, 128  # 8 x 8 regions of 8 x 16 pixels per image and cout block


def _case(N, cin, cout, seed, pre=False, skip=False, c1=None):
    x, w, b = _inputs(N, cin, cout, H, W, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    d = dict(x=x, w=w, b=b, pre=None, skip=None, div=1.0, c1=c1)
    if pre:  # a different (s, t) per image and channel: a table left from another image shows
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
        out = conv3x3_fwd_raw(x[s].contiguous().to(hip), d["w"].to(hip), d["b"].to(hip),
                              skip=dev(d["skip"]), div=d["div"], pre=dev(d["pre"]), stats=stats,
                              **kw)
    return out, (gn_partials(out)[0].clone() if stats else None)


def _check_case(hip, d, what, stats=False, per_image=True):
    from op import conv as conv_op
    out, part = _run(hip, d, stats)
    _check(out, _ref(d["x"], d["w"], d["b"], d["pre"], d["skip"], d["div"]), what)
    if stats:
        _check_stats(out, what)
    again, part2 = _run(hip, d, stats)
    assert torch.equal(out, again), f"{what}: two runs differ"
    if stats:
        assert torch.equal(part, part2), f"{what}: statistics of two runs differ"
    if per_image:
        for i in range(d["x"].shape[0]):
            one, p1 = _run(hip, d, stats, i, i + 1)
            assert conv_op.last_form == 24
            assert torch.equal(out[i:i + 1], one), f"{what}: image {i} differs from its own launch"
            if stats:
                assert torch.equal(part[i:i + 1], p1), f"{what}: statistics of image {i}"


def test_items_one_chunk(hip):
    """320 items of one chunk: FIRST and the last step are the same step"""
    _check_case(hip, _case(5, 16, 128, seed=20), "items 16->128")


@pytest.mark.parametrize("cin", [32, 48])
def test_items_two_and_three_chunks_all_forms(hip, cin):
    """nch = 2 and 3 with bias, prologue, residual tail and statistics together"""
    _check_case(hip, _case(5, cin, 128, seed=21 + cin, pre=True, skip=True), f"items {cin}->128",
                stats=True)


def test_items_three_per_workgroup_across_images(hip):
    """576 items: some workgroups walk 3 items and pass from one image to the next"""
    _check_case(hip, _case(9, 32, 128, seed=23, pre=True), "items N=9 32->128", stats=True)


def test_items_two_cout_blocks_two_sources(hip):
    """384 items over two cout blocks; channels [0, 16) from x, [16, 48) from x2"""
    _check_case(hip, _case(3, 48, 256, seed=24, pre=True, c1=16), "items 48->256 two sources")


def test_items_four_chunk_loop(hip):
    """nch = 4: the first full step and the three peeled tail steps, 384 items (float64 only: a
    per-image call may split K)"""
    _check_case(hip, _case(3, 64, 256, seed=25, pre=True, skip=True), "items 64->256", stats=True,
                per_image=False)


def test_items_split_k_slices(hip):
    """a shape that wino_splits does split (the existing split-K test's): slices as items"""
    from op._lib import lib
    from op.conv import conv3x3_fwd_raw
    N, c, h, w_ = 1, 128, 16, 16
    assert lib.bpk_conv3x3_wino_splitk_bytes(N, c, c, c, h, w_) > 0
    x, w, b = _inputs(N, c, c, h, w_, seed=26)
    skip = torch.randn(N, c, h, w_, generator=torch.Generator().manual_seed(27))
    with torch.no_grad():
        out = conv3x3_fwd_raw(x.to(hip), w.to(hip), b.to(hip), skip=skip.to(hip), div=2 ** 0.5,
                              stats=True)
    _check(out, _ref(x, w, b, None, skip, 2 ** 0.5), "items split-K")
    _check_stats(out, "items split-K")

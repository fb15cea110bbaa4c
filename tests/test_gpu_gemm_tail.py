"""The 1x1-conv GEMM's fused store (bpk_gemm_nchw_ex_f32, op.conv.conv1x1(skip=, div=, stats=)):
the residual tail (skip + (W X + bias)) / div and the GroupNorm partial statistics of the
stored values, in the GEMM's epilogue and, under split-K, in its reduce launch.

Gates
  * output: bit-identical to conv1x1 followed by residual_rescale;
  * partial records: float64 mean / M2 of each 128-pixel record.  float32 arithmetic over a
    128-term tree: the mean within 1e-5 of max |y|, M2 (a sum of squares, every term >= 0)
    within 1e-5 of itself;
  * (scale, shift) table built from the records vs the table from ensure_gn_partials on the
    same tensor: TABLE_GATE = 4 x the worst difference the two existing statistic paths
    (group_norm_affine's own pass, and ensure_gn_partials + group_norm_affine_partials) show on
    these same tensors, as a fraction of max |table|.  Measured on MI355X over the five shapes
    below: 9.6e-8, 1.99e-7, 1.60e-7, 1.53e-7, 1.47e-7 -> TABLE_PATHS_WORST = 1.99e-7 (per shape
    it is printed by the test before the assertion; the records' own tables measured
    9.6e-8 .. 1.99e-7 from the chunk-partials table).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, M, P = H x W, K1, K2)
SHAPES = {
    "one_tile": (2, 128, (8, 16), 16, 0),
    "m144_guarded_rows": (2, 144, (16, 16), 48, 0),
    "two_sources": (2, 128, (16, 16), 32, 16),
    "splitk": (2, 128, (8, 16), 128, 0),          # smallest shape the split-K form takes
    "splitk_two_sources_m144": (2, 144, (16, 16), 64, 64),
}
SPLIT = {"splitk", "splitk_two_sources_m144"}
DIV = float(np.sqrt(2.0))
TABLE_PATHS_WORST = 1.99e-7   # measured: see the module docstring
TABLE_GATE = 4 * TABLE_PATHS_WORST

_CASES = {}


def _case(hip, name):
    """Inputs, the unfused result and the fused results of one shape (computed once)."""
    if name in _CASES:
        return _CASES[name]
    from op.conv import conv1x1, gn_partials
    from op.norm_act import residual_rescale
    N, M, (H, W), K1, K2 = SHAPES[name]
    g = torch.Generator().manual_seed(1000 + M + K1 + 7 * K2 + H)
    x1 = torch.randn(N, K1, H, W, generator=g).to(hip)
    x2 = torch.randn(N, K2, H, W, generator=g).to(hip) if K2 else None
    w = (torch.randn(M, K1 + K2, 1, 1, generator=g) / (K1 + K2) ** 0.5).to(hip)
    b = torch.randn(M, generator=g).to(hip)
    skip = (torch.randn(N, M, H, W, generator=g) + 0.5).to(hip)
    with torch.no_grad():
        plain = conv1x1(x1, w, b, x2)
        unfused = residual_rescale(skip, plain, None, DIV)
        fused = conv1x1(x1, w, b, x2, skip=skip, div=DIV, stats=True)
        again = conv1x1(x1, w, b, x2, skip=skip, div=DIV, stats=True)
        stats_only = conv1x1(x1, w, b, x2, stats=True)
        skip_only = conv1x1(x1, w, b, x2, skip=skip, div=DIV)
    c = dict(N=N, M=M, P=H * W, plain=plain, unfused=unfused, fused=fused, again=again,
             stats_only=stats_only, skip_only=skip_only, part=gn_partials(fused),
             part_again=gn_partials(again), part_stats_only=gn_partials(stats_only))
    _CASES[name] = c
    return c


def _records64(y):
    """float64 (mean, M2) of every 128 consecutive pixels of every row: [N, M, R]"""
    N, M = y.shape[:2]
    v = y.double().cpu().reshape(N, M, -1, 128)
    mean = v.mean(-1)
    return mean, ((v - mean[..., None]) ** 2).sum(-1)


def _check_records(y, part):
    pt, R, cnt = part
    assert cnt == 128 and R == y.shape[2] * y.shape[3] // 128
    assert tuple(pt.shape) == (y.shape[0], y.shape[1], R, 2)
    mean, m2 = _records64(y)
    got = pt.double().cpu()
    e_mean = ((got[..., 0] - mean).abs().max() / y.double().abs().max()).item()
    e_m2 = ((got[..., 1] - m2).abs() / m2).max().item()
    print(f"partials: mean err / max|y| = {e_mean:.3e}, worst relative M2 err = {e_m2:.3e}")
    assert e_mean <= 1e-5 and e_m2 <= 1e-5


@pytest.mark.parametrize("name", list(SHAPES))
def test_split_form_is_the_one_named(hip, name):
    from op.conv import lib
    N, M, (H, W), K1, K2 = SHAPES[name]
    assert (lib.bpk_gemm_nchw_splitk_bytes(N, M, H * W, K1, K2) > 0) == (name in SPLIT)


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_tail_bit_identical_to_conv1x1_then_residual_rescale(hip, name):
    c = _case(hip, name)
    assert torch.equal(c["fused"], c["unfused"])
    assert torch.equal(c["skip_only"], c["unfused"])      # skip without stats
    assert torch.equal(c["stats_only"], c["plain"])       # stats without skip
    assert c["part"] is not None and c["part_stats_only"] is not None
    from op.conv import gn_partials
    assert gn_partials(c["skip_only"]) is None


@pytest.mark.parametrize("name", list(SHAPES))
def test_partial_records_match_float64(hip, name):
    c = _case(hip, name)
    _check_records(c["fused"], c["part"])
    _check_records(c["stats_only"], c["part_stats_only"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_runs_bit_identical(hip, name):
    c = _case(hip, name)
    assert torch.equal(c["fused"], c["again"])
    assert torch.equal(c["part"][0], c["part_again"][0])


@pytest.mark.parametrize("name", list(SHAPES))
def test_affine_table_from_records_matches_chunk_partials(hip, name):
    from op.conv import ensure_gn_partials
    from op.norm_act import group_norm_affine, group_norm_affine_partials
    c = _case(hip, name)
    N, M = c["N"], c["M"]
    gn = torch.nn.GroupNorm(32 if M % 32 == 0 else 16, M, eps=1e-6).to(hip)
    with torch.no_grad():
        gn.weight.copy_(1 + 0.1 * torch.randn(M, generator=torch.Generator().manual_seed(M)))
        gn.bias.copy_(0.05 * torch.randn(M, generator=torch.Generator().manual_seed(M + 1)))
        y = c["fused"].clone()                      # no records attached
        own_pass = group_norm_affine(y, gn)         # existing path 1: its own statistics pass
        chunk = group_norm_affine_partials(ensure_gn_partials(y), N, M, gn)  # existing path 2
        ours = group_norm_affine_partials(c["part"], N, M, gn)
    scale = chunk.abs().max().item()
    paths = (own_pass - chunk).abs().max().item() / scale
    err = (ours - chunk).abs().max().item() / scale
    print(f"table: existing paths differ by {paths:.3e} of max |table|, records vs "
          f"ensure_gn_partials {err:.3e} (gate {TABLE_GATE:.3e})")
    assert err <= TABLE_GATE

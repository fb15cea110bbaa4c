"""Which launches each residual block issues, per regime.

The float64 truth tests cannot see a block that silently falls back to its unfused
composition: it computes the same numbers.  Here every `bpk_*` symbol a block calls through
`op._lib.lib` -- kernels, `*_supported` and `*_bytes` queries alike, names only -- is recorded in
order, for the forward and for each backward, and compared against tests/golden/block_paths.json.

The expected lists were recorded from the commit before the blocks were split into one method
per regime (`python tests/test_gpu_block_paths.py --record PATH` on that commit's files), so a
restructuring that changes a launch, drops a fusion or reorders two attempts fails here.

Blocks: N = 2, 32 x 32 planes, temb_dim 64, SiLU (score-net blocks); ELU + InstanceNorm
(`layers.ResidualBlock`).  At this size every eval / no_grad list of a score-net block holds a
Winograd conv behind a GroupNorm prologue table (`bpk_group_norm_affine*` then
`bpk_conv3x3_wino*`), no standalone GroupNorm launch, and for the FIR blocks the FIR-prologue
resampler: test_golden_pins_the_fused_kernels checks that of the committed file.
"""
import contextlib
import json
import os
import sys

import pytest
import torch

import conv_pick

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_paths.json")

# name: (class, constructor arguments, forward_pair?)
SCORE_BLOCKS = {
    "biggan_32_32": ("biggan", dict(in_ch=32, out_ch=32), False),
    "biggan_32_64": ("biggan", dict(in_ch=32, out_ch=64), False),
    "biggan_fir_up": ("biggan", dict(in_ch=32, out_ch=32, up=True, fir=True), False),
    "biggan_fir_down": ("biggan", dict(in_ch=32, out_ch=32, down=True, fir=True), False),
    "biggan_pair_32_32_32": ("biggan", dict(in_ch=64, out_ch=32), True),
    "ddpm_32_32": ("ddpm", dict(in_ch=32, out_ch=32), False),
    "ddpm_32_64_nin": ("ddpm", dict(in_ch=32, out_ch=64), False),
    "ddpm_32_64_conv_shortcut": ("ddpm", dict(in_ch=32, out_ch=64, conv_shortcut=True), False),
    "ddpm_pair_32_32_32": ("ddpm", dict(in_ch=64, out_ch=32), True),
}
SCORE_MODES = ("no_grad", "frozen", "grad", "higher_order", "train_dropout", "train_no_dropout")
# Conv_0 on the small-channel kernel (Cin <= 4), which has no GroupNorm prologue: gn_silu_conv
# declines, and with grad mode on and nothing requiring a gradient the block asks for the
# autograd form of the fusion next -- an ordering of attempts that is behaviour
SMALL_CIN = ("biggan_4_32", ("biggan", dict(in_ch=4, out_ch=32), False))
RESIDUAL_BLOCKS = {"residual_16_32": (16, 32), "residual_32_32": (32, 32)}
RESIDUAL_MODES = ("no_grad", "grad", "create_graph")
CASES = ([(b, m) for b in SCORE_BLOCKS for m in SCORE_MODES]
         + [(SMALL_CIN[0], m) for m in ("no_grad", "frozen")]
         + [(b, m) for b in RESIDUAL_BLOCKS for m in RESIDUAL_MODES])


def _recorder(monkeypatch):
    """The list that every `bpk_*` call through op._lib.lib appends its symbol name to."""
    from op import _lib
    orig, names = _lib._Lib.__getattr__, []

    def getattr_(self, name):
        fn = orig(self, name)
        if name == "bpk_last_error":
            return fn

        def call(*args):
            names.append(name)
            return fn(*args)
        return call

    monkeypatch.setattr(_lib._Lib, "__getattr__", getattr_)
    return names


def _perturb(module):
    with torch.no_grad():
        for p in module.parameters():
            p.add_(torch.randn_like(p) * 0.05)


def _take(names):
    out = list(names)
    del names[:]
    return out


def _run_score_block(hip, names, block, mode):
    from models import layers, layerspp
    kind, kw, pair = SMALL_CIN[1] if block == SMALL_CIN[0] else SCORE_BLOCKS[block]
    cls = layerspp.ResnetBlockBigGANpp if kind == "biggan" else layers.ResnetBlockDDPM
    torch.manual_seed(5)
    blk = cls(act=torch.nn.SiLU(), temb_dim=64, dropout=0.0 if mode == "train_no_dropout" else 0.1,
              **kw).to(hip)
    _perturb(blk)
    blk.train(mode.startswith("train"))
    if mode == "frozen":
        blk.requires_grad_(False)
    g = torch.Generator().manual_seed(6)
    backward = mode not in ("no_grad", "frozen")
    xs = [torch.randn(2, kw["in_ch"] // 2 if pair else kw["in_ch"], 32, 32, generator=g).to(hip)
          .requires_grad_(backward) for _ in range(2 if pair else 1)]
    temb = torch.randn(2, 64, generator=g).to(hip)
    ctx = (torch.no_grad() if mode == "no_grad" else layers.higher_order_autograd()
           if mode == "higher_order" else contextlib.nullcontext())
    got = {}
    with ctx:
        _take(names)
        out = (blk.forward_pair if pair else blk)(*xs, temb)
        got["forward"] = _take(names)
        if backward:
            (out ** 2).sum().backward()
            got["backward"] = _take(names)
    return got


def _run_residual_block(hip, names, block, mode):
    from models import layers
    torch.manual_seed(7)
    blk = layers.ResidualBlock(*RESIDUAL_BLOCKS[block]).to(hip)
    _perturb(blk)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, RESIDUAL_BLOCKS[block][0], 32, 32, generator=g).to(hip)
    x.requires_grad_(mode != "no_grad")
    got = {}
    with torch.no_grad() if mode == "no_grad" else contextlib.nullcontext():
        _take(names)
        out = blk(x)
        got["forward"] = _take(names)
        if mode == "grad":
            (out ** 2).sum().backward()
            got["backward"] = _take(names)
        elif mode == "create_graph":
            gx, = torch.autograd.grad(out.sum(), x, create_graph=True)
            got["backward"] = _take(names)
            ((gx ** 2).sum() + (out ** 2).sum()).backward()
            got["second_backward"] = _take(names)
    return got


def _run(hip, monkeypatch, block, mode):
    from op import conv
    conv_pick.first_only(monkeypatch)
    # the one memo of op.conv that outlives a module: without this a case's list would depend
    # on which shapes earlier tests of the process had asked about
    conv._igemm_shape_ok.cache_clear()
    names = _recorder(monkeypatch)
    run = _run_residual_block if block in RESIDUAL_BLOCKS else _run_score_block
    got = run(hip, names, block, mode)
    torch.cuda.synchronize()
    return got


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@gpu
@pytest.mark.parametrize("block,mode", CASES, ids=[f"{b}-{m}" for b, m in CASES])
def test_block_issues_the_recorded_launches(hip, monkeypatch, block, mode):
    want = _golden()[f"{block}/{mode}"]
    got = _run(hip, monkeypatch, block, mode)
    assert got.keys() == want.keys()
    for phase in want:
        assert got[phase] == want[phase], f"{block}, {mode}, {phase}"


def test_golden_pins_the_fused_kernels():
    """A golden in which the fused kernels do not occur pins nothing."""
    gold = _golden()
    assert sorted(gold) == sorted(f"{b}/{m}" for b, m in CASES)
    for block in SCORE_BLOCKS:
        fwd = gold[f"{block}/no_grad"]["forward"]
        table = [i for i, n in enumerate(fwd) if n.startswith("bpk_group_norm_affine")]
        wino = [i for i, n in enumerate(fwd)
                if n.startswith("bpk_conv3x3_wino") and n.endswith("splitk_f32")]
        assert table and wino and wino[-1] > table[0], block
        assert "bpk_group_norm_fwd_f32" not in fwd, block
        if "_fir_" in block:
            assert "bpk_upfirdn2d_pre_f32" in fwd, block
    # small Cin: with grad mode on, the autograd form's two shape queries follow the decline of
    # gn_silu_conv (its two small-kernel queries), and nothing else differs
    off, on = (gold[f"{SMALL_CIN[0]}/{m}"]["forward"] for m in ("no_grad", "frozen"))
    assert off[:2] == ["bpk_conv3x3_small_supported"] * 2
    asked = ["bpk_conv3x3_wino_supported", "bpk_conv3x3_wino_pair_supported"]
    assert on == off[:2] + asked + off[2:]


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_block_paths.py --record PATH")
    import conftest  # noqa: F401  (puts the package on sys.path)
    dev, rec = torch.device("cuda:0"), {}
    for blk_, mode_ in CASES:
        with pytest.MonkeyPatch.context() as mp:
            rec[f"{blk_}/{mode_}"] = _run(dev, mp, blk_, mode_)
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sys.argv[2]}: {len(rec)} cases, "
          f"{sum(len(v) for c in rec.values() for v in c.values())} calls")

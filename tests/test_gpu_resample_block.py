"""The inference paths around the 3x3 convs of the NCSN++ resample and attention blocks:
GroupNorm_0 + SiLU inside the FIR resampler's loads (upfirdn2d_pre), the up block's skip
projection before the FIR upsample, Conv_0's GroupNorm partials in the
resample blocks, the attention block's residual tail + partials in the NIN_3 GEMM's store, and
the weight-only tensors kept between forwards (op.conv.weight_derived).

Reference: the blocks restated in float64 torch on the CPU in the reference's op order
(GroupNorm+SiLU, FIR resample of h and x, Conv_0, + Dense_0(SiLU(temb)), GroupNorm+SiLU,
Conv_1, Conv_2 on the resampled x, (x + h) / sqrt 2; oracle.upfirdn2d_ref for the FIR).
Gate 1e-5 of max |ref|, with every switch on and with each one off.
"""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_pick

gpu = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _first_conv_candidate(monkeypatch):
    """Every timed kernel choice of op.conv (tests/conv_pick.py) runs its first candidate in
    this module -- the Winograd kernels of the blocks -- with no timing and no choice
    inherited from an earlier test.  Both candidates of every choice against float64:
    tests/test_gpu_conv_pick.py."""
    conv_pick.first_only(monkeypatch)
RTOL = 1e-5
K1D = np.array([1.0, 3.0, 3.0, 1.0])


def _fir64(t, up):
    from oracle.upfirdn2d_ref import upfirdn2d_np
    k = np.outer(K1D, K1D) / 64.0
    if up:
        return torch.from_numpy(upfirdn2d_np(t.numpy(), 4.0 * k, (2, 2), (1, 1), (2, 1, 2, 1)))
    return torch.from_numpy(upfirdn2d_np(t.numpy(), k, (1, 1), (2, 2), (1, 1, 1, 1)))


def _p64(m):
    return {k: v.detach().double().cpu() for k, v in m.state_dict().items()}


def _gn64(x, p, name, groups):
    return F.group_norm(x, groups, p[name + ".weight"], p[name + ".bias"], 1e-6)


def _resblock_ref(blk, x, temb, up):
    p = _p64(blk)
    x, temb = x.double().cpu(), temb.double().cpu()
    h = F.silu(_gn64(x, p, "GroupNorm_0", blk.GroupNorm_0.num_groups))
    h, x = _fir64(h, up), _fir64(x, up)
    h = F.conv2d(h, p["Conv_0.weight"], p["Conv_0.bias"], padding=1)
    h = h + F.linear(F.silu(temb), p["Dense_0.weight"], p["Dense_0.bias"])[:, :, None, None]
    h = F.silu(_gn64(h, p, "GroupNorm_1", blk.GroupNorm_1.num_groups))
    h = F.conv2d(h, p["Conv_1.weight"], p["Conv_1.bias"], padding=1)
    x = F.conv2d(x, p["Conv_2.weight"], p["Conv_2.bias"])
    return (x + h) / np.sqrt(2.0)


def _attn_ref(blk, x):
    p = _p64(blk)
    x = x.double().cpu()
    B, C, H, W = x.shape
    h = _gn64(x, p, "GroupNorm_0", blk.GroupNorm_0.num_groups)
    nin = lambda t, n: torch.einsum("bchw,co->bohw", t, p[n + ".W"]) + p[n + ".b"][None, :, None, None]
    q, k, v = nin(h, "NIN_0"), nin(h, "NIN_1"), nin(h, "NIN_2")
    w = torch.einsum("bchw,bcij->bhwij", q, k) * (int(C) ** (-0.5))
    w = F.softmax(w.reshape(B, H, W, H * W), dim=-1).reshape(B, H, W, H, W)
    h = nin(torch.einsum("bhwij,bcij->bchw", w, v), "NIN_3")
    return (x + h) / np.sqrt(2.0)


@contextlib.contextmanager
def _switch(name, value):
    import models.layers as layers
    import models.layerspp as lpp
    from op import conv as conv_op
    mod = {"_GEMM_TAIL": lpp, "_UP_SKIP_FIRST": lpp, "_RESAMPLE_STATS": lpp, "_FIR_PRE": lpp,
           "_WEIGHT_CACHE": conv_op, "_TEMB_FOLD": layers}[name]
    old = getattr(mod, name)
    setattr(mod, name, value)
    try:
        yield
    finally:
        setattr(mod, name, old)


def _make_resblock(hip, up):
    import models.layerspp as lpp
    torch.manual_seed(3 + up)
    blk = lpp.ResnetBlockBigGANpp(act=torch.nn.SiLU(), in_ch=32, out_ch=32, temb_dim=64, up=up,
                                  down=not up, fir=True, skip_rescale=True, init_scale=0.,
                                  dropout=0.1).to(hip).eval()
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    g = torch.Generator().manual_seed(11 + up)
    x = (torch.randn(2, 32, 16, 16, generator=g) * 1.5 + 0.3).to(hip)
    temb = torch.randn(2, 64, generator=g).to(hip)
    return blk, x, temb


@gpu
@pytest.mark.parametrize("kind", ["up", "down"])
def test_resample_block_matches_float64_reference_with_every_switch(hip, kind):
    from op import conv as conv_op
    up = kind == "up"
    blk, x, temb = _make_resblock(hip, up)
    ref = _resblock_ref(blk, x, temb, up)
    scale = ref.abs().max().item()
    errs = {}
    with torch.no_grad():
        errs["fused"] = blk(x.clone(), temb)
        xp = x.clone()
        assert conv_op.ensure_gn_partials(xp) is not None  # input carrying partial statistics
        errs["fused, input with partials"] = blk(xp, temb)
        for sw in ("_FIR_PRE", "_UP_SKIP_FIRST", "_RESAMPLE_STATS", "_WEIGHT_CACHE"):
            with _switch(sw, False):
                errs[sw + "=0"] = blk(x.clone(), temb)
    # the switches change the path: the reordered projection rounds differently
    if up:
        assert not torch.equal(errs["fused"], errs["_UP_SKIP_FIRST=0"])
    assert torch.equal(errs["fused"], errs["_WEIGHT_CACHE=0"])
    assert not torch.equal(errs["fused"], errs["_FIR_PRE=0"])
    for what, y in errs.items():
        if up:  # 32 x 32 output: Conv_1's epilogue writes the partials, as before
            assert conv_op.gn_partials(y) is not None, what
        e = (y.double().cpu() - ref).abs().max().item() / scale
        print(f"{kind} block, {what}: {e:.3e} of max |ref|")
        assert e <= RTOL, what


def _make_attn(hip):
    import models.layerspp as lpp
    torch.manual_seed(9)
    blk = lpp.AttnBlockpp(32, skip_rescale=True, init_scale=0.).to(hip).eval()
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    x = torch.randn(2, 32, 16, 16, generator=torch.Generator().manual_seed(4)).to(hip)
    return blk, x


@gpu
def test_attention_block_matches_float64_reference_with_every_switch(hip):
    from op import conv as conv_op
    blk, x = _make_attn(hip)
    ref = _attn_ref(blk, x)
    scale = ref.abs().max().item()
    outs = {}
    with torch.no_grad():
        assert blk._qkv_ok(x)
        outs["fused"] = blk(x)
        for sw in ("_GEMM_TAIL", "_WEIGHT_CACHE"):
            with _switch(sw, False):
                outs[sw + "=0"] = blk(x)
    # the tail in the GEMM's store is the same arithmetic: bit-identical to the separate launch
    assert torch.equal(outs["fused"], outs["_GEMM_TAIL=0"])
    assert torch.equal(outs["fused"], outs["_WEIGHT_CACHE=0"])
    assert conv_op.gn_partials(outs["fused"]) is not None
    assert conv_op.gn_partials(outs["_GEMM_TAIL=0"]) is None
    for what, y in outs.items():
        e = (y.double().cpu() - ref).abs().max().item() / scale
        print(f"attention block, {what}: {e:.3e} of max |ref|")
        assert e <= RTOL, what


# ------------------------------------------------------------------ weight-derived tensors

def test_weight_derived_rebuilds_after_every_kind_of_weight_change():
    """Host side: the cached tensor follows an in-place write, an optimizer step and
    load_state_dict; an untouched weight is not rebuilt; nothing is cached under autograd."""
    from op import conv as conv_op
    lin = torch.nn.Linear(4, 3)
    calls = []

    def build():
        calls.append(1)
        return lin.weight.t().contiguous() * 2.0

    def get():
        return conv_op.weight_derived(lin, "wt2", [lin.weight], build)

    with torch.no_grad():
        a = get()
        assert get() is a and len(calls) == 1
        lin.weight.add_(1.0)                                   # in place
        b = get()
        assert len(calls) == 2 and torch.equal(b, lin.weight.t() * 2.0)
    opt = torch.optim.SGD(lin.parameters(), lr=0.5)
    lin(torch.ones(2, 4)).sum().backward()
    opt.step()                                                 # optimizer step
    with torch.no_grad():
        c = get()
        assert len(calls) == 3 and torch.equal(c, lin.weight.t() * 2.0)
        sd = {k: v + 3.0 for k, v in lin.state_dict().items()}
        lin.load_state_dict(sd)                                # load_state_dict
        d = get()
        assert len(calls) == 4 and torch.equal(d, lin.weight.t() * 2.0)
        assert get() is d and len(calls) == 4
    n = len(calls)
    e = get()                                                  # grad mode on: never cached
    assert e.requires_grad and len(calls) == n + 1
    get()
    assert len(calls) == n + 2
    with torch.no_grad(), _switch("_WEIGHT_CACHE", False):
        get()
        get()
    assert len(calls) == n + 4


def test_temb_bank_sees_a_weight_changed_in_place():
    """Host side: the TembBank that keeps its concatenated weights on the model and folds
    Conv_0.bias in returns, after an in-place weight and bias change, what a bank built from
    scratch returns."""
    from models import layers
    torch.manual_seed(0)

    class Blk(torch.nn.Module):
        def __init__(self, c):
            super().__init__()
            self.Dense_0 = torch.nn.Linear(8, c)
            self.Conv_0 = torch.nn.Conv2d(c, c, 3, padding=1)

    owner = torch.nn.Module()
    owner.blocks = torch.nn.ModuleList([Blk(4), Blk(6)])
    act = torch.nn.SiLU()
    temb = torch.randn(3, 8)

    def biases(folded):
        ds = [b.Dense_0 for b in owner.blocks]
        if folded:
            bank = layers.TembBank(temb, act, ds, owner=owner,
                                   conv_biases=[b.Conv_0.bias for b in owner.blocks])
        else:
            bank = layers.TembBank(temb, act, ds)
        return [layers.conv_temb_bias(b, act, bank, 3) for b in owner.blocks]

    with torch.no_grad():
        for _ in range(2):
            for got, want in zip(biases(True), biases(False)):
                assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()
            first = [t.clone() for t in biases(True)]
            owner.blocks[1].Dense_0.weight.mul_(1.5)
            owner.blocks[0].Conv_0.bias.add_(0.25)
        for got, old in zip(biases(True), first):
            assert not torch.equal(got, old)
        with pytest.raises(RuntimeError):
            bank = layers.TembBank(temb, act, [b.Dense_0 for b in owner.blocks], owner=owner,
                                   conv_biases=[b.Conv_0.bias for b in owner.blocks])
            layers.temb_proj(owner.blocks[0].Dense_0, act, bank)


@gpu
def test_attention_block_sees_a_weight_changed_in_place(hip):
    blk, x = _make_attn(hip)
    with torch.no_grad():
        before = blk(x)
        blk.NIN_3.W.mul_(1.25)
        blk.NIN_0.b.add_(0.5)
        after = blk(x)
        with _switch("_WEIGHT_CACHE", False):
            fresh = blk(x)
    assert torch.equal(after, fresh)
    assert not torch.equal(after, before)


@gpu
def test_pc_step_graph_refreshes_weight_derived_tensors(hip):
    """The PC step graph reads the cached weight-derived tensors (registered beside the filter
    transforms): after every parameter has changed in place, graph replays == eager steps."""
    import models  # noqa: F401
    import sampling
    import sde_lib
    from configs.vp import nc_ncsnpp_128
    from models import utils as mutils
    c = nc_ncsnpp_128.get_config()
    c.model.nf = 32
    c.data.image_size = 32
    c.device = hip
    torch.manual_seed(0)
    model = mutils.create_model(c, wrap=False).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    sde = sde_lib.VPSDE(0.1, 20., 1000)
    prior = torch.randn(2, 1, 32, 32, generator=torch.Generator().manual_seed(5))
    w0 = [p.detach().clone() for p in model.parameters()]
    outs = []
    for use_graph in (True, False):
        with torch.no_grad():
            for p, v in zip(model.parameters(), w0):
                p.copy_(v)
        eng = sampling.PCEngine(sde, (2, 1, 32, 32), sampling.EulerMaruyamaPredictor,
                                sampling.LangevinCorrector, 0.075, 1, continuous=True,
                                device=hip, seed=1234, use_graph=use_graph)
        eng.reset(model, x_init=prior)
        eng.advance(2)
        first = eng._xm.clone()
        if use_graph:
            assert eng.graph is not None, getattr(eng, "capture_error", None)
            assert any(e[4] == "derived" for e in eng._filters)
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(1.05)
        eng.advance(2)
        torch.cuda.synchronize()
        outs.append((first, eng._xm.clone()))
        del eng
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[0][1])

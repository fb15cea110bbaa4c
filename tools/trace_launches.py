"""Launch trace of one tree: every `bpk_*` call of `op._lib.lib` (symbol, each non-pointer
argument, null / non-null for each pointer argument, the returned status or byte count), per
workload, plus the tensors each workload produced.

    BPK_CONV_PICK=first python tools/trace_launches.py ROOT OUT.pt

ROOT: the repository root to trace (this tree, or an export of the parent commit; BPK_LIB names
the libbpk.so when ROOT has none built).  One fresh process per run; compare_traces.py reads
the OUT files.

Workloads: one training step per train fixture (`train_*`), a DPS-style input gradient through
`ncsnpp_a` (`dps_*`), the same inside `higher_order_autograd()` (`higher_*`), one `no_grad`
forward of every net fixture (`infer_*`), one forward of `ncsnpp_a` with grad enabled and all
parameters frozen (`frozen_*`), one eager PINN training step (`pinn`), and a double backward
outside `deferred_weight_grads()` (`nodefer`)."""
import contextlib
import ctypes
import os
import sys

ROOT, OUT = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("BPK_CONV_PICK", "first")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402,F401
import conftest as cf  # noqa: E402  (puts ROOT's package on sys.path)
from op import _lib  # noqa: E402

TRACE, TENSORS, SECTION = [], {}, ["start"]
_orig, _wrapped = _lib._Lib.__getattr__, {}


def _wrap(name, fn):
    is_ptr = [a is ctypes.c_void_p for a in fn.argtypes]

    def call(*args):
        r = fn(*args)
        shown = [("nil" if a in (None, 0) else "ptr") if p else a for a, p in zip(args, is_ptr)]
        TRACE.append(f"{SECTION[0]} {name}({', '.join(map(str, shown))}) -> {r}")
        return r
    return call


def _getattr(self, name):
    fn = _orig(self, name)
    if name == "bpk_last_error":
        return fn
    if name not in _wrapped:
        _wrapped[name] = _wrap(name, fn)
    return _wrapped[name]


_lib._Lib.__getattr__ = _getattr
hip = torch.device("cuda", 0)


def keep(name, t):
    TENSORS[f"{SECTION[0]}/{name}"] = t.detach().cpu().clone()


def score_model(name):
    import models  # noqa: F401
    from models import utils as mutils
    cfg, sd, x, labels, y = cf.net_fixture(name)
    model = mutils.create_model(cf.product_config(cfg, hip), wrap=False)
    model.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    return cfg, model.eval(), x, labels


def train_step(name):
    """the body of tests/test_gpu_models.py::test_train_step_matches_reference"""
    import losses
    import sde_lib
    from models.ema import ExponentialMovingAverage
    SECTION[0] = f"train_{name}"
    d = cf.load_golden(f"train_{name}.npz")
    cfg, model, *_ = score_model(str(d["net"]))
    c = cf.product_config(cfg, hip)
    model.train()
    rng = [(k.split("_", 1)[1], torch.tensor(d[k])) for k in sorted(
        (k for k in d.files if k.startswith("rng")), key=lambda s: int(s[3:].split("_")[0]))]
    it = iter(rng)
    real = {k: getattr(torch, k) for k in ("rand", "randn_like", "randint")}
    for k in real:
        setattr(torch, k, lambda *a, **kw: next(it)[1].to(hip))
    try:
        sde = sde_lib.VPSDE(c.model.beta_min, c.model.beta_max, c.model.num_scales)
        opt = losses.get_optimizer(c, model.parameters())
        ema = ExponentialMovingAverage(model.parameters(), decay=c.model.ema_rate)
        state = dict(optimizer=opt, model=model, ema=ema, step=int(d["step0"]))
        real_step = opt.step

        def capture(*a, **kw):
            for k, p in model.named_parameters():
                if p.grad is not None:
                    keep("g:" + k, p.grad)
            return real_step(*a, **kw)

        opt.step = capture
        step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(c),
                                     reduce_mean=c.training.reduce_mean,
                                     continuous=bool(d["continuous"]))
        keep("loss", step_fn(state, torch.tensor(d["batch"], device=hip)))
    finally:
        for k, v in real.items():
            setattr(torch, k, v)
    for k, p in model.named_parameters():
        keep("p1:" + k, p)


def dps_input_gradient(name="ncsnpp_a"):
    SECTION[0] = f"dps_{name}"
    _, model, x, labels = score_model(name)
    x = torch.tensor(x, device=hip).requires_grad_()
    out = model(x, torch.tensor(labels, device=hip))
    gx, = torch.autograd.grad((out ** 2).sum(), x)
    keep("out", out)
    keep("gx", gx)


def higher_order_input_gradient(name="ncsnpp_a"):
    from models import layers
    SECTION[0] = f"higher_{name}"
    _, model, x, labels = score_model(name)
    x = torch.tensor(x, device=hip).requires_grad_()
    with layers.higher_order_autograd():
        out = model(x, torch.tensor(labels, device=hip))
        gx, = torch.autograd.grad((out ** 2).sum(), x)
    keep("out", out)
    keep("gx", gx)


def inference(name, frozen=False):
    """one forward without an autograd graph: under no_grad, or (frozen) with grad enabled and
    no parameter requiring a gradient"""
    SECTION[0] = f"{'frozen' if frozen else 'infer'}_{name}"
    _, model, x, labels = score_model(name)
    with contextlib.nullcontext() if frozen else torch.no_grad():
        keep("out", model.requires_grad_(not frozen)(torch.tensor(x, device=hip),
                                                     torch.tensor(labels, device=hip)))


def pinn_step(batch=4):
    """one eager training step of the shipped PINN configuration (deferred weight gradients)"""
    import losses
    from configs.pinn import pinn_pde
    from inverse.operators import InpaintOperator
    from models.ema import ExponentialMovingAverage
    from pinn_kalman.pinn import PINN
    SECTION[0] = "pinn"
    c = cf.full_pinn_config(pinn_pde.get_config, batch)
    m = cf.build_pinn_weights(PINN, c).to(hip)
    c.device = hip
    em = ExponentialMovingAverage(m.parameters(), decay=c.model.ema_rate)
    opt_f = losses.get_optimizer(c, m.flownet.parameters())
    opt_p = losses.get_optimizer(c, m.pressurenet.parameters(), 0.001)
    state = dict(optimizer=(opt_f, opt_p), model=m, ema=em, step=50)
    step_fn = losses.get_pinn_step_fn(c, train=True, optimize_fn=losses.optimization_manager(c))
    f1, f2, x, y, t, target = (v.to(hip) for v in cf.make_pinn_inputs(c, 7))
    n = c.data.image_size
    mask = (torch.rand(1, 1, n, n, generator=torch.Generator().manual_seed(8)) <= 0.9).float()
    mask = mask.expand(batch, 1, n, n).contiguous()
    torch.manual_seed(9)
    out = step_fn(state, InpaintOperator(mask=[mask.to(hip)]),
                  (f1, f2, x.requires_grad_(), y.requires_grad_(), t.requires_grad_(), target))
    for i, o in enumerate(out):
        keep(f"loss{i}", o)
    for k, p in m.named_parameters():
        keep("p:" + k, p)
        if p.grad is not None:
            keep("g:" + k, p.grad)


def double_backward_not_deferred():
    """the body of tests/test_gpu_ops.py::test_deferred_weight_grads_match_autograd, defer=False"""
    from models import layers
    from op import conv as conv_op
    from op.fused_act import leaky_relu
    SECTION[0] = "nodefer"
    torch.manual_seed(3)
    net = torch.nn.ModuleList([
        layers.Conv2d(16, 32, 3, padding=1), layers.Conv2d(32, 32, 3, padding=1),
        layers.Conv2d(32, 16, 3, stride=2, padding=1),
        layers.ConvTranspose2d(16, 16, 2, stride=2),
        layers.ResidualBlock(16, 32), layers.ResidualBlock(32, 32),
        layers.Conv2d(32, 8, 1)]).to(hip)
    x = torch.randn(8, 16, 16, 16, device=hip, requires_grad=True)
    prev, layers._IN_FANOUT = layers._IN_FANOUT, False
    try:
        h = x
        for i, m in enumerate(net):
            h = m(h)
            if i < 3:
                h = leaky_relu(h, 0.1)
        gx, = torch.autograd.grad(h.sum(), x, create_graph=True)
        loss = (gx ** 2).sum() + (h ** 2).sum()
        with conv_op.deferred_weight_grads(False):
            loss.backward(inputs=list(net.parameters()))
    finally:
        layers._IN_FANOUT = prev
    for k, p in net.named_parameters():
        keep("g:" + k, p.grad)


for name in ("dsm_ncsnpp", "dsm_fourier", "ddpm_discrete"):
    train_step(name)
dps_input_gradient()
higher_order_input_gradient()
for name in ("ncsnpp_a", "ncsnpp_b", "ncsnpp_c", "ddpm_a"):
    inference(name)
inference("ncsnpp_a", frozen=True)
pinn_step()
double_backward_not_deferred()
torch.cuda.synchronize()
torch.save({"trace": TRACE, "tensors": TENSORS}, OUT)
print(f"{OUT}: {len(TRACE)} calls, {len(TENSORS)} tensors, "
      f"finite: {all(bool(np.isfinite(t.numpy()).all()) for t in TENSORS.values())}")

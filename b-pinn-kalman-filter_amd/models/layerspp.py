"""NCSN++ layers on the gfx950 path (reference: models/layerspp.py).

Module / parameter names are the reference's (GroupNorm_0, Conv_0, Dense_0,
GroupNorm_1, Conv_1, Conv_2, NIN_*, Conv2d_0, W) so reference state dicts load.
Per block the arithmetic is re-scheduled for the GPU:
  GroupNorm_0+SiLU                  -> 1 fused launch
  FIR up/down of h and x            -> upfirdn2d HIP kernel
  Conv_0 (no bias)                  -> conv
  + Conv_0.bias + Dense_0(SiLU(temb)), GroupNorm_1, SiLU -> 1 fused launch
  Conv_1 (no bias), + Conv_1.bias + skip, / sqrt(2)      -> conv + 1 fused launch
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from op import conv as conv_op
from op.norm_act import residual_rescale

from . import layers, up_or_down_sampling

# Test seams of the inference paths outside the 3x3 convs: plain constants, all on; a test sets
# one to False to run the unfused composition beside the fused path.
_ATTN_FUSED = True      # softmax(q^T k) v as one kernel, False: bmm + softmax + bmm (test_gpu_ops)
_GEMM_TAIL = True       # attention: residual tail + GroupNorm partials in the NIN_3 GEMM's store
_UP_SKIP_FIRST = True   # up blocks: the 1x1 skip projection before the FIR upsample
_FIR_PRE = True         # up / down blocks: GroupNorm_0 + SiLU inside the FIR resampler's loads
_RESAMPLE_STATS = True  # up / down blocks: Conv_0 writes GroupNorm_1's partial statistics
# (the last four: test_gpu_resample_block; _FIR_PRE also test_gpu_upfirdn_pre)

conv1x1 = layers.ddpm_conv1x1
conv3x3 = layers.ddpm_conv3x3
NIN = layers.NIN
default_init = layers.default_init
gn_act = layers.gn_act
conv_nobias = layers.conv_nobias


class GaussianFourierProjection(nn.Module):
    """Random Fourier features of log-sigma (reference :32-41)."""

    def __init__(self, embedding_size=256, scale=1.0):
        super().__init__()
        self.W = nn.Parameter(torch.randn(embedding_size) * scale, requires_grad=False)

    def forward(self, x):
        proj = x[:, None] * self.W[None, :] * 2 * np.pi
        return torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1)


class Combine(nn.Module):
    """1x1 conv of x then concat/sum with y (reference :44-59)."""

    def __init__(self, dim1, dim2, method="cat"):
        super().__init__()
        self.Conv_0 = conv1x1(dim1, dim2)
        self.method = method

    def forward(self, x, y):
        h = self.Conv_0(x)
        if self.method == "cat":
            return torch.cat([h, y], dim=1)
        if self.method == "sum":
            return h + y
        raise ValueError(f"Method {self.method} not recognized.")


class AttnBlockpp(nn.Module):
    """Channel self-attention over H*W positions (reference :62-91)."""

    def __init__(self, channels, skip_rescale=False, init_scale=0.):
        super().__init__()
        self.GroupNorm_0 = nn.GroupNorm(num_groups=min(channels // 4, 32), num_channels=channels,
                                        eps=1e-6)
        self.NIN_0 = NIN(channels, channels)
        self.NIN_1 = NIN(channels, channels)
        self.NIN_2 = NIN(channels, channels)
        self.NIN_3 = NIN(channels, channels, init_scale=init_scale)
        self.skip_rescale = skip_rescale

    def forward(self, x):
        h = gn_act(x, self.GroupNorm_0, None)
        div = np.sqrt(2.) if self.skip_rescale else 1.0
        if not torch.is_grad_enabled() and self._qkv_ok(h):
            return self._forward_qkv(h, x, div)
        h = self.NIN_3(layers._attention(h, self.NIN_0, self.NIN_1, self.NIN_2))
        return residual_rescale(x, h, None, div)

    def _qkv_ok(self, h):
        N, C, H, W = h.shape
        return (h.is_cuda and h.dtype == torch.float32
                and bool(conv_op.lib.bpk_gemm_nchw_supported(N, 3 * C, H * W, C, 0))
                and bool(conv_op.lib.bpk_gemm_nchw_supported(N, C, H * W, C, 0)))

    def _forward_qkv(self, h, skip=None, div=1.0):
        """Inference: q, k, v as ONE MFMA GEMM over the stacked NIN weights, NIN_3 as another
        (op.conv.conv1x1), the 1/sqrt(C) scale folded into q's weights when it is a power of
        two (exact: C = 4^k, e.g. 256) and applied to the logits otherwise.  With `skip` the
        result is the block's output (skip + NIN_3(...)) / div: the residual tail and the
        output's GroupNorm partial statistics in the NIN_3 GEMM's store (_GEMM_TAIL off: the
        separate residual_rescale launch, no statistics).  The stacked / transposed weights
        are kept between forwards (op.conv.weight_derived)."""
        B, C, H, W = h.shape
        s = float(int(C) ** (-0.5))
        fold = math.frexp(s)[0] == 0.5  # s is a power of two
        sq = s if fold else 1.0
        n0, n1, n2, n3 = self.NIN_0, self.NIN_1, self.NIN_2, self.NIN_3
        wqkv = conv_op.weight_derived(
            self, "wqkv", [n0.W, n1.W, n2.W],
            lambda: torch.cat([n0.W.t() * sq, n1.W.t(), n2.W.t()], 0))
        bqkv = conv_op.weight_derived(
            self, "bqkv", [n0.b, n1.b, n2.b], lambda: torch.cat([n0.b * sq, n1.b, n2.b], 0))
        w3 = conv_op.weight_derived(self, "w3", [n3.W], lambda: n3.W.t().contiguous())
        qkv = conv_op.conv1x1(h, wqkv, bqkv).reshape(B, 3, C, H * W)
        from op import attention as attn_op
        if _ATTN_FUSED and attn_op.supported(qkv):
            out = attn_op.attention(qkv, 1.0 if fold else s).reshape(B, C, H, W)
        else:
            q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
            w = torch.bmm(q.transpose(1, 2), k)
            if not fold:
                w = w * s
            w = torch.softmax(w, dim=-1)
            out = torch.bmm(v, w.transpose(1, 2)).reshape(B, C, H, W)
        if skip is None:
            return conv_op.conv1x1(out, w3, n3.b)
        if _GEMM_TAIL:
            return conv_op.conv1x1(out, w3, n3.b, skip=skip, div=div, stats=True)
        return residual_rescale(skip, conv_op.conv1x1(out, w3, n3.b), None, div)


class Upsample(nn.Module):
    """x2 upsampling: nearest(+conv) or FIR(+fused conv) (reference :94-126)."""

    def __init__(self, in_ch=None, out_ch=None, with_conv=False, fir=False,
                 fir_kernel=(1, 3, 3, 1)):
        super().__init__()
        out_ch = out_ch if out_ch else in_ch
        if not fir:
            if with_conv:
                self.Conv_0 = conv3x3(in_ch, out_ch)
        elif with_conv:
            self.Conv2d_0 = up_or_down_sampling.Conv2d(in_ch, out_ch, kernel=3, up=True,
                                                       resample_kernel=fir_kernel, use_bias=True,
                                                       kernel_init=default_init())
        self.fir, self.with_conv = fir, with_conv
        self.fir_kernel = fir_kernel
        self.out_ch = out_ch

    def forward(self, x):
        B, C, H, W = x.shape
        if not self.fir:
            # the reference passes 'nearest' positionally as scale_factor (layerspp.py:117),
            # which raises; the intended nearest-neighbour upsample is used here
            h = F.interpolate(x, (H * 2, W * 2), mode="nearest")
            return self.Conv_0(h) if self.with_conv else h
        if not self.with_conv:
            return up_or_down_sampling.upsample_2d(x, self.fir_kernel, factor=2)
        return self.Conv2d_0(x)


class Downsample(nn.Module):
    """/2 downsampling: strided conv / avg-pool or FIR(+fused conv) (reference :129-163)."""

    def __init__(self, in_ch=None, out_ch=None, with_conv=False, fir=False,
                 fir_kernel=(1, 3, 3, 1)):
        super().__init__()
        out_ch = out_ch if out_ch else in_ch
        if not fir:
            if with_conv:
                self.Conv_0 = conv3x3(in_ch, out_ch, stride=2, padding=0)
        elif with_conv:
            self.Conv2d_0 = up_or_down_sampling.Conv2d(in_ch, out_ch, kernel=3, down=True,
                                                       resample_kernel=fir_kernel, use_bias=True,
                                                       kernel_init=default_init())
        self.fir, self.with_conv = fir, with_conv
        self.fir_kernel = fir_kernel
        self.out_ch = out_ch

    def forward(self, x):
        if not self.fir:
            if self.with_conv:
                return self.Conv_0(F.pad(x, (0, 1, 0, 1)))
            return F.avg_pool2d(x, 2, stride=2)
        if not self.with_conv:
            return up_or_down_sampling.downsample_2d(x, self.fir_kernel, factor=2)
        return self.Conv2d_0(x)


class ResnetBlockDDPMpp(nn.Module):
    """DDPM++ residual block (reference :166-209)."""

    def __init__(self, act, in_ch, out_ch=None, temb_dim=None, conv_shortcut=False,
                 dropout=0.1, skip_rescale=False, init_scale=0.):
        super().__init__()
        out_ch = out_ch if out_ch else in_ch
        self.GroupNorm_0 = nn.GroupNorm(num_groups=min(in_ch // 4, 32), num_channels=in_ch, eps=1e-6)
        self.Conv_0 = conv3x3(in_ch, out_ch)
        if temb_dim is not None:
            self.Dense_0 = nn.Linear(temb_dim, out_ch)
            self.Dense_0.weight.data = default_init()(self.Dense_0.weight.data.shape)
            nn.init.zeros_(self.Dense_0.bias)
        self.GroupNorm_1 = nn.GroupNorm(num_groups=min(out_ch // 4, 32), num_channels=out_ch,
                                        eps=1e-6)
        self.Dropout_0 = nn.Dropout(dropout)
        self.Conv_1 = conv3x3(out_ch, out_ch, init_scale=init_scale)
        if in_ch != out_ch:
            if conv_shortcut:
                self.Conv_2 = conv3x3(in_ch, out_ch)
            else:
                self.NIN_0 = NIN(in_ch, out_ch)
        self.skip_rescale = skip_rescale
        self.act = act
        self.out_ch = out_ch
        self.conv_shortcut = conv_shortcut

    def forward(self, x, temb=None):
        h, x = layers.gn_act_fanout(x, self.GroupNorm_0, self.act)
        h = conv_nobias(h, self.Conv_0)
        bias_nc = layers.conv_temb_bias(self, self.act, temb, x.shape[0])
        h = gn_act(h, self.GroupNorm_1, self.act, bias_nc)
        h = self.Dropout_0(h)
        if x.shape[1] != self.out_ch:
            x = self.Conv_2(x) if self.conv_shortcut else self.NIN_0(x)
        return layers.conv_residual(h, self.Conv_1, self.Conv_1.bias, x,
                                    np.sqrt(2.) if self.skip_rescale else 1.0)


class ResnetBlockBigGANpp(nn.Module):
    """BigGAN residual block with optional FIR up/down (reference :212-274)."""

    def __init__(self, act, in_ch, out_ch=None, temb_dim=None, up=False, down=False,
                 dropout=0.1, fir=False, fir_kernel=(1, 3, 3, 1), skip_rescale=True,
                 init_scale=0.):
        super().__init__()
        out_ch = out_ch if out_ch else in_ch
        self.GroupNorm_0 = nn.GroupNorm(num_groups=min(in_ch // 4, 32), num_channels=in_ch, eps=1e-6)
        self.up, self.down = up, down
        self.fir, self.fir_kernel = fir, fir_kernel
        self.Conv_0 = conv3x3(in_ch, out_ch)
        if temb_dim is not None:
            self.Dense_0 = nn.Linear(temb_dim, out_ch)
            self.Dense_0.weight.data = default_init()(self.Dense_0.weight.shape)
            nn.init.zeros_(self.Dense_0.bias)
        self.GroupNorm_1 = nn.GroupNorm(num_groups=min(out_ch // 4, 32), num_channels=out_ch,
                                        eps=1e-6)
        self.Dropout_0 = nn.Dropout(dropout)
        self.Conv_1 = conv3x3(out_ch, out_ch, init_scale=init_scale)
        if in_ch != out_ch or up or down:
            self.Conv_2 = conv1x1(in_ch, out_ch)
        self.skip_rescale = skip_rescale
        self.act = act
        self.in_ch, self.out_ch = in_ch, out_ch

    def _resample(self, t):
        if self.up:
            return (up_or_down_sampling.upsample_2d(t, self.fir_kernel, factor=2) if self.fir
                    else up_or_down_sampling.naive_upsample_2d(t, factor=2))
        if self.down:
            return (up_or_down_sampling.downsample_2d(t, self.fir_kernel, factor=2) if self.fir
                    else up_or_down_sampling.naive_downsample_2d(t, factor=2))
        return t

    def _bias12(self):
        """Conv_1.bias + Conv_2.bias (inference: kept between forwards)"""
        b1, b2 = self.Conv_1.bias, self.Conv_2.bias
        return conv_op.weight_derived(self, "bias12", [b1, b2], lambda: b1 + b2)

    @property
    def _div(self):
        return np.sqrt(2.) if self.skip_rescale else 1.0

    def forward(self, x, temb=None):
        if not layers.fused_inference_ok(self, x, self.act):
            return self._autograd(x, temb)
        if self.up or self.down:
            return self._inference_resample(x, temb)
        return self._inference_plain(x, temb)

    def forward_pair(self, x1, x2, temb=None):
        """forward(torch.cat([x1, x2], 1), temb) -- the up path's skip concatenation -- at
        inference without building the concatenation: GroupNorm_0 from the parts' partial
        statistics, Conv_0 reading both sources (layers.pair_conv0), the 1x1 skip projection as
        one two-source MFMA GEMM.  Falls back to the concatenation when a piece does not fit."""
        conv2 = getattr(self, "Conv_2", None)
        ok = (layers.fused_inference_ok(self, x1, self.act) and not (self.up or self.down)
              and conv2 is not None)
        h = layers.pair_conv0(self, x1, x2, ok, conv2)
        if h is None:
            return self.forward(layers.cat_channels(x1, x2), temb)
        bias_nc = layers.conv_temb_bias(self, self.act, temb, h.shape[0])
        bias = self._bias12()
        skip = conv_op.conv1x1(x1, self.Conv_2.weight, None, x2)
        return layers.inference_tail(self, h, bias_nc, bias, skip, self._div, stats=True)

    def _inference_plain(self, x, temb):
        """GroupNorm_0 + SiLU applied inside Conv_0's input load"""
        h = layers.gn_silu_conv(x, self.GroupNorm_0, self.Conv_0)
        if h is None:
            # a Conv_0 without the prologue form; with grad mode on (and nothing requiring a
            # gradient) the autograd form of the same fusion is tried next
            h = layers.gn_silu_conv_ad_1(self, x, self.GroupNorm_0, self.Conv_0, self.act)
        if h is None:
            h = self._conv0_stats(gn_act(x, self.GroupNorm_0, self.act))
        return self._shortcut_and_tail(h, x, temb)

    def _inference_resample(self, x, temb):
        """FIR up / down block: GroupNorm_0 + SiLU inside the FIR resampler's loads (the table
        from the input's partial statistics when its producer wrote them), no activated tensor
        written and read back"""
        if (_FIR_PRE and self.fir
                and up_or_down_sampling.resample_2d_pre_supported(x, self.fir_kernel, self.up)):
            ss = layers.group_norm_affine(x, self.GroupNorm_0)
            h = up_or_down_sampling.resample_2d_pre(x, ss, self.fir_kernel, self.up)
        else:
            h = self._resample(gn_act(x, self.GroupNorm_0, self.act))
        # the 1x1 projection mixes channels, the FIR upsample acts per channel -- they commute,
        # and projecting first runs the GEMM on a quarter of the pixels (down blocks project
        # at the low resolution already)
        first = self.up and _UP_SKIP_FIRST and x.is_cuda
        x = self._resample(conv_nobias(x, self.Conv_2) if first else x)
        return self._shortcut_and_tail(self._conv0_stats(h), x, temb, projected=first)

    def _conv0_stats(self, h):
        """Conv_0 without bias, GroupNorm_1's statistics from its epilogue"""
        if _RESAMPLE_STATS and layers._wino_eligible(h, self.Conv_0):
            return conv_op.conv3x3(h, self.Conv_0.weight, None, stats=True)
        return conv_nobias(h, self.Conv_0)

    def _shortcut_and_tail(self, h, x, temb, projected=False):
        """GroupNorm_1 (+ time bias) + SiLU + Conv_1 + residual tail; the 1x1 skip conv's bias
        joins Conv_1's in the fused residual (no separate full-tensor bias add after the GEMM)"""
        bias_nc = layers.conv_temb_bias(self, self.act, temb, h.shape[0])
        bias = self.Conv_1.bias
        if hasattr(self, "Conv_2"):
            if not projected:
                x = conv_nobias(x, self.Conv_2)
            bias = self._bias12()
        return layers.inference_tail(self, h, bias_nc, bias, x, self._div, stats=True)

    def _autograd(self, x, temb):
        """training, and eval-mode gradients (DPS): there the plain block's convs take the fused
        first-order Function, its backward recomputing the normalization"""
        if self.up or self.down:
            h, x = layers.gn_act_fanout(x, self.GroupNorm_0, self.act)
            h, x = self._resample(h), self._resample(x)
            h, link = conv_nobias(h, self.Conv_0), None
        else:
            h, x, link = layers.autograd_conv0(self, x)
        bias_nc = layers.conv_temb_bias(self, self.act, temb, h.shape[0])
        bias = self.Conv_1.bias
        if hasattr(self, "Conv_2"):
            x = conv_nobias(x, self.Conv_2)
            bias = bias + self.Conv_2.bias
        return layers.autograd_tail(self, h, bias_nc, bias, x, self._div, link)

"""SincNet stream: SincConv front end on the HIP kernel + the residual 2-D encoder.

Reference: CONV (src/models/DualStreamSEMamba.py:49-138), Residual_block (:144-200) and
SincNetEncoder (:206-270), themselves taken from AASIST (models/AASIST.py:325-466).
"""
import os
import random
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

import torch.nn.functional as F

from . import sinc_x3
from .ops import (HALF, SCONV_CH, SCONV_POOL_DEFAULT, Block0Convs, Block0Front, Block0Fused, BnSelu, BnSeluSConv,
                  ResBlock, ResTail, SConv, SConvBnSelu, SConvBnSeluSConv, _frozen_invstd, sconv_enabled,
                  sincconv_absmaxpool)


def _half_autocast(x):
    """CUDA autocast to bf16 or fp16: the 16-bit NHWC kernels (libradhip.so / libradhip_f16.so) apply."""
    return x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") in HALF


def mel_edges(out_channels, sample_rate, nfft=512):
    """Band edges equally spaced on the mel scale over 0..fs/2 (CONV.__init__ :95-101)."""
    f = int(sample_rate / 2) * np.linspace(0, 1, int(nfft / 2) + 1)
    mel = 2595 * np.log10(1 + f / 700)
    m = np.linspace(np.min(mel), np.max(mel), out_channels + 1)
    return 700 * (10 ** (m / 2595) - 1)


def sinc_bank(out_channels=70, kernel_size=129, sample_rate=16000):
    """[C, K] float32 Hamming-windowed band-pass bank. Follows the reference's numeric path exactly
    (float32 tap grid, numpy sinc on it, float32 window x float32 ideal response; :104-117) so the
    bank is bit-identical to the reference's `band_pass` (checked against tests/golden)."""
    K = kernel_size
    edges = mel_edges(out_channels, sample_rate)
    n = torch.arange(-(K - 1) / 2, (K - 1) / 2 + 1, device="cpu")   # float32 grid, as the reference
    win = torch.from_numpy(np.hamming(K)).float()
    rows = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        h = (2 * hi / sample_rate) * np.sinc(2 * hi * n / sample_rate)
        l = (2 * lo / sample_rate) * np.sinc(2 * lo * n / sample_rate)
        rows.append(win * torch.from_numpy(np.asarray(h - l)).float())
    return torch.stack(rows)


class CONV(nn.Module):
    """Drop-in of the reference CONV: fixed (non-learnable) sinc filter bank. `forward` keeps the
    reference's API (x [B,1,T] -> [B,C,T-K+1]) for callers that need the raw conv; SincNetEncoder uses
    `absmaxpool`, the fused HIP path that never materialises the [B, 70, 64472] conv output."""

    def __init__(self, out_channels, kernel_size, sample_rate=16000, in_channels=1, stride=1, padding=0,
                 dilation=1, bias=False, groups=1, mask=False):
        super().__init__()
        if in_channels != 1:
            raise ValueError("SincConv only support one input channel (here, in_channels = {%i})" % in_channels)
        if bias:
            raise ValueError("SincConv does not support bias.")
        if groups > 1:
            raise ValueError("SincConv does not support groups.")
        self.out_channels = out_channels
        self.kernel_size = kernel_size + 1 if kernel_size % 2 == 0 else kernel_size
        self.sample_rate = sample_rate
        self.stride, self.padding, self.dilation, self.mask = stride, padding, dilation, mask
        self.register_buffer("band_pass", sinc_bank(out_channels, self.kernel_size, sample_rate), persistent=False)
        # HIP-graph mode: when set (int32 [2] on the device), the Freq_aug mask is read from here at
        # execution time; the trainer draws it on the host (same RNG order) before each replay.
        self.mask_dev = None

    def draw_mask(self):
        """Freq_aug: zero A = int(U(0,20)) consecutive filters at A0 = randint(0, C-A) (:121-125),
        numpy then python RNG, exactly as the reference draws them."""
        A = int(np.random.uniform(0, 20))
        A0 = random.randint(0, self.out_channels - A)
        return A0, A0 + A

    def forward(self, x, mask=False):
        w = self.band_pass.clone()
        if mask:
            lo, hi = self.draw_mask()
            w[lo:hi] = 0
        return torch.nn.functional.conv1d(x, w.view(self.out_channels, 1, self.kernel_size), stride=self.stride,
                                          padding=self.padding, dilation=self.dilation)

    def absmaxpool(self, x, mask=False):
        """max_pool2d(|conv(x)|, (3,3)) on the HIP kernel: x [B, T] -> [B, C//3, (T-K+1)//3]."""
        if mask and self.mask_dev is not None:
            return sincconv_absmaxpool(x, self.band_pass, mask_dev=self.mask_dev)
        lo, hi = self.draw_mask() if mask else (0, 0)
        return sincconv_absmaxpool(x, self.band_pass, lo, hi)


class Residual_block(nn.Module):
    """Same parameters and forward as the reference block. The reference computes bn1+selu and then
    discards them (`out = self.conv1(x)`, :189); here only bn1's running-stat side effect is kept
    (when bn1 is in training mode), without the dead activation."""

    def __init__(self, nb_filts, first=False):
        super().__init__()
        self.first = first
        if not self.first:
            self.bn1 = nn.BatchNorm2d(num_features=nb_filts[0])
        self.conv1 = nn.Conv2d(nb_filts[0], nb_filts[1], kernel_size=(2, 3), padding=(1, 1), stride=1)
        self.selu = nn.SELU(inplace=True)
        self.bn2 = nn.BatchNorm2d(num_features=nb_filts[1])
        self.conv2 = nn.Conv2d(nb_filts[1], nb_filts[1], kernel_size=(2, 3), padding=(0, 1), stride=1)
        self.downsample = nb_filts[0] != nb_filts[1]
        if self.downsample:
            self.conv_downsample = nn.Conv2d(nb_filts[0], nb_filts[1], padding=(0, 1), kernel_size=(1, 3), stride=1)
        self.mp = nn.MaxPool2d((1, 3))

    def dead_parameters(self):
        """bn1's affine weights: the reference's forward discards bn1's output, so they never receive a
        gradient there (AdamW skips them, weight decay included); radhip.train leaves them out likewise."""
        return [] if self.first else list(self.bn1.parameters())

    def _fused_ok(self, x):
        return (x.is_cuda and not self.bn2.training and x.dim() == 4 and x.shape[1] == self.conv1.in_channels
                and x.is_contiguous(memory_format=torch.channels_last) and self.conv2.out_channels % 8 == 0)

    def forward(self, x):
        if not self.first and self.bn1.training:
            with torch.no_grad():
                self.bn1(x)
        if not self._fused_ok(x):
            out = self.conv1(x)
            out = self.selu(self.bn2(out))
            out = self.conv2(out)
            identity = self.conv_downsample(x) if self.downsample else x
            return self.mp(out + identity)
        # NHWC fused epilogues (csrc/sincnet.hip): conv1's bias is folded into the frozen-BN+SELU pass, conv2 /
        # conv_downsample biases into the add + MaxPool2d((1,3)) pass. Under bf16 / fp16 autocast the 32/64-channel
        # convolutions run on csrc/sconv.hip (conv1 with the BN+SELU in its epilogue). _route names the ops.
        c1, c2, bn = self.conv1, self.conv2, self.bn2
        cd = self.conv_downsample if self.downsample else None
        w1, w2, wd = c1.weight, c2.weight, cd.weight if cd is not None else None
        bnp = (c1.bias, bn.running_mean, _frozen_invstd(bn), bn.weight, bn.bias)
        a = c = out = None
        idn = x
        for op in _route(self.first, self.downsample, x.shape[1], c1.out_channels, x.shape[3], _half_autocast(x),
                         _switches()):
            if op == "Block0Fused":
                return Block0Fused.apply(x, w1, wd, *bnp, w2, c2.bias, cd.bias)
            if op == "ResBlock":
                return ResBlock.apply(x, w1, *bnp, w2, c2.bias + cd.bias if cd is not None else c2.bias, wd)
            if op == "ResTail":
                return ResTail.apply(a, idn, c2.bias + cd.bias if cd is not None else c2.bias)
            if op == "Block0Front":
                a, idn = Block0Front.apply(x, w1, wd, *bnp, w2)
            elif op == "Block0Convs":
                c, idn = Block0Convs.apply(x, w1, wd)
            elif op == "BnSeluSConv":
                a = BnSeluSConv.apply(c, *bnp, w2)
            elif op == "conv1":
                c = F.conv2d(x, w1, None, c1.stride, c1.padding)
            elif op == "BnSelu":
                out = BnSelu.apply(c, *bnp)
            elif op == "SConvBnSeluSConv":
                a = SConvBnSeluSConv.apply(x, w1, 1, *bnp, w2)
            elif op == "SConvBnSelu":
                out = SConvBnSelu.apply(x, w1, 1, *bnp)
            elif op == "SConv2":
                a = SConv.apply(out, w2, 0)
            elif op == "conv2":
                a = F.conv2d(out, w2, None, c2.stride, c2.padding)
            elif op == "SConvDown":
                idn = SConv.apply(x, wd, 0)
            elif op == "convDown":
                idn = F.conv2d(x, wd, None, cd.stride, cd.padding)
        raise AssertionError("radhip: a residual block's route ends in an op that returns")


Switches = namedtuple("Switches", "sconv pair b0x fused_b0 b0_fwd res_fused pool")


def _switches():
    """The residual stack's routing switches (RADHIP_<NAME>=0 takes the path the named one replaced); all default
    to on. RADHIP_SCONV_POOL also takes fwd / bwd (radhip.ops.sconv_pool_ok): only 0 changes the route."""
    on = lambda name, default="1": os.environ.get(name, default) != "0"
    return Switches(sconv=sconv_enabled(), pair=on("RADHIP_SCONV_PAIR"), b0x=on("RADHIP_B0X"),
                    fused_b0=on("RADHIP_FUSED_B0"), b0_fwd=on("RADHIP_B0_FWD"), res_fused=on("RADHIP_RES_FUSED"),
                    pool=on("RADHIP_SCONV_POOL", SCONV_POOL_DEFAULT))


def _route(first, down, ci, co, W, half, sw):
    """The ops of a fused residual block, in the order Residual_block.forward runs them: first / down: the block's
    flags, ci -> co its channels, W the input's width, half: 16-bit autocast, sw: _switches(). Names of radhip.ops
    classes, and conv1 / conv2 / convDown for torch's conv2d, SConv2 / SConvDown for SConv as conv2 / conv_downsample.
    Every chain ends in an op that produces the block's output."""
    def sconv(a, b):                       # csrc/sconv.hip has the convolution a -> b channels
        return half and sw.sconv and a in SCONV_CH and b in SCONV_CH
    pair = sconv(co, co) and sw.pair       # conv1 -> bn2 -> selu -> conv2 as one autograd op
    conv2 = ("SConv2" if sconv(co, co) else "conv2",)
    if first and down and ci == 1 and half:
        if pair and W >= 3 and co == 32 and sw.b0x:
            return ("Block0Fused",)        # the whole block in one HIP pass each way
        if sw.fused_b0:                    # one input channel: conv1 and conv_downsample in one HIP pass each way
            if pair and sw.b0_fwd:
                return ("Block0Front", "ResTail")
            return ("Block0Convs",) + (("BnSeluSConv",) if pair else ("BnSelu",) + conv2) + ("ResTail",)
    if sconv(ci, co):
        if pair and sw.res_fused and (sw.pool or not down):
            return ("ResBlock",)           # the whole block as one autograd op (RADHIP_SCONV_POOL=0: not block 2)
        front = ("SConvBnSeluSConv",) if pair else ("SConvBnSelu",) + conv2
    else:
        front = ("conv1", "BnSelu") + conv2
    return front + (("SConvDown" if sconv(ci, co) else "convDown",) if down else ()) + ("ResTail",)


class SincNetEncoder(nn.Module):
    def __init__(self, sinc_channels=70, sinc_kernel=128):
        super().__init__()
        filts = [sinc_channels, [1, 32], [32, 32], [32, 64], [64, 64]]
        self.conv_time = CONV(out_channels=filts[0], kernel_size=sinc_kernel, in_channels=1)
        self.first_bn = nn.BatchNorm2d(num_features=1)
        self.selu = nn.SELU(inplace=True)
        self.encoder = nn.Sequential(
            nn.Sequential(Residual_block(nb_filts=filts[1], first=True)),
            nn.Sequential(Residual_block(nb_filts=filts[2])),
            nn.Sequential(Residual_block(nb_filts=filts[3])),
            nn.Sequential(Residual_block(nb_filts=filts[4])),
            nn.Sequential(Residual_block(nb_filts=filts[4])),
            nn.Sequential(Residual_block(nb_filts=filts[4])))
        self.out_dim = filts[-1][-1]
        # NHWC activations for the residual Conv2d stack: MIOpen's NHWC implicit-GEMM solvers are
        # ~1.4x faster than its NCHW path on these [B, C, 23, T] shapes (measured on MI355X).
        self.channels_last = True

    def forward(self, x, freq_aug=False):
        """x [B, T] -> e_T [B, T', 64] (SincNetEncoder.forward :238-270)."""
        if sinc_x3.eligible(self, x, freq_aug):
            # the fp32 scoring pass on the split-precision kernels (radhip/sinc_x3.py)
            return sinc_x3.forward(self, x)
        x = self.conv_time.absmaxpool(x.float(), mask=freq_aug).unsqueeze(1)    # [B, 1, 23, T/3]
        x = self.selu(self.first_bn(x))
        if self.channels_last and x.is_cuda:
            x = x.contiguous()
            # C == 1: NCHW memory is already NHWC, but torch keeps the NCHW strides and its layout
            # heuristic would then run block 0's convs in NCHW (and copy every gradient back and forth).
            # Restride to the channels_last form (same bytes) so MIOpen picks its NHWC kernels.
            N, C, H, W = x.shape
            x = x.as_strided((N, C, H, W), (C * H * W, 1, W * C, C)) if C == 1 else \
                x.contiguous(memory_format=torch.channels_last)
        e = self.encoder(x)
        e_T, _ = torch.max(torch.abs(e), dim=2)
        return e_T.transpose(1, 2)

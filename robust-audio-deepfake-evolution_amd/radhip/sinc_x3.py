"""The SincNet stream of the fp32 scoring pass on split-precision ("x3") kernels.

Beside the WavLM stream (radhip/wavlm_x3.py), the scoring pass runs SincNetEncoder (radhip/sinc.py; reference
src/models/DualStreamSEMamba.py:206-270) in eval mode without autocast. Its residual convolutions used to take MIOpen
fp32; here they take csrc/sconv_x3.hip, with the conventions of the WavLM stream: an fp32 operand is two bf16 planes
hi = bf16(x), lo = bf16(x - hi), a product is x_hi w_hi + x_lo w_hi + x_hi w_lo on the bf16 MFMA with fp32 accumulation.
  * SincConv + |.| + 3x3 max pool: the exact fp32 kernel (radhip.ops.sincconv_absmaxpool), as before;
  * block 0 (one input channel): rdx_x3_b0x_fwd, one pass from the raw SincConv output (first_bn + SELU folded into its
    staging) to the pooled block output, no full-size intermediate;
  * blocks 1-5: conv1 with bn2 + SELU in its epilogue, conv2 and conv_downsample on rdx_x3_sconv_fwd (fp32 NHWC in
    and out, split on staging), then the fp32 rdx_res_tail_fwd (a + identity + bias, MaxPool2d((1, 3)));
  * max |.| over the 23 filter rows in torch; the NHWC output is already [B, T', 64].

Enabled inside `wavlm_x3.scoring()`; RADHIP_X3_SINC=0 (or RADHIP_X3=0) keeps the module path.

In order, not beside the WavLM stream. models/DualStreamSEMamba.py runs an eligible pass on the current stream after
the WavLM stream instead of on its side stream. With these kernels on the side stream, the first batched CNN GEMM of
the WavLM stream (rdx_hgemm_x3, batch > 1, overlapping A rows) returned different values from pass to pass (about 3 %
of its elements, up to 0.15 absolute; logits moved by up to 4e-3 at |logit| 10), while every stage of this stream stayed
bit-identical; in order, both streams are bit-identical from pass to pass. Why that GEMM depends on what runs beside it
is open. The overlap bought nothing here: 25.3 ms per batch of 32 beside each other, against 20.3 ms for
the WavLM stream plus 5.0 ms for this one.

When the planes are rebuilt. The planes, BN tables and summed biases (`_x3w` on the SincNetEncoder) are a cache of
trained weights, keyed by `wavlm_x3._src(enc)`: the `invalidate()` epoch plus `(data_ptr, _version)` of every parameter
and buffer of the encoder. The rules are those of the WavLM planes and need no call site of their own:
radhip.optim.AdamW.step, radhip.train.EMA.swap and FGM.attack / FGM.restore write through raw pointers or `p.data` and
call `wavlm_x3.invalidate()`; `load_state_dict`, `copy_` and other in-place ops bump `_version`;
`radhip.infer.produce_evaluation_file_sharded` calls `wavlm_x3.drop(model)`, which pops `_x3w` from every submodule,
this encoder included, before and after a scoring pass.
"""
import os

import torch

from ._lib import check, lib
from .ops import _p, _stream, _timed, sincconv_absmaxpool
from . import _lib, wavlm_x3

# (ci, co, downsample) of blocks 1-5 behind block 0 (1 -> 32)
_LAYOUT = [(32, 32, False), (32, 64, True), (64, 64, False), (64, 64, False), (64, 64, False)]


def _conv_is(c, ci, co, k, pad):
    return (isinstance(c, torch.nn.Conv2d) and c.in_channels == ci and c.out_channels == co
            and tuple(c.kernel_size) == k and tuple(c.padding) == pad and tuple(c.stride) == (1, 1)
            and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.bias is not None)


def _block_is(blk, ci, co, first, down):
    return (blk.first == first and blk.downsample == down and _conv_is(blk.conv1, ci, co, (2, 3), (1, 1))
            and _conv_is(blk.conv2, co, co, (2, 3), (0, 1))
            and (not down or _conv_is(blk.conv_downsample, ci, co, (1, 3), (0, 1))))


def standard_layout(enc):
    """1 -> 32, 32 -> 32, 32 -> 64, 64 -> 64 x 3 with the (2, 3) / (2, 3) / (1, 3) kernels of Residual_block."""
    seq = list(enc.encoder)
    if len(seq) != 6 or any(len(s) != 1 for s in seq):
        return False
    blocks = [s[0] for s in seq]
    if not _block_is(blocks[0], 1, 32, True, True):
        return False
    return all(_block_is(b, ci, co, False, down) for b, (ci, co, down) in zip(blocks[1:], _LAYOUT))


def widths(enc, L):
    """Input width of each of the six blocks for L samples."""
    w = (L - enc.conv_time.kernel_size + 1) // 3
    out = []
    for _ in range(6):
        out.append(w)
        w //= 3
    return out


def eligible(enc, x, freq_aug=False):
    """Inside `wavlm_x3.scoring()` unless RADHIP_X3_SINC=0: a 2-D CUDA input, no autocast, no grad, the
    whole encoder in eval mode, no band mask, the standard block layout and every block at least 3 positions wide.
    Anything else takes the module path."""
    if not (wavlm_x3.active() and os.environ.get("RADHIP_X3_SINC", "1") != "0"):
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2) or freq_aug:
        return False
    if torch.is_autocast_enabled("cuda") or torch.is_grad_enabled():
        return False
    if any(m.training for m in enc.modules()):
        return False
    return standard_layout(enc) and enc.conv_time.out_channels >= 3 and min(widths(enc, x.shape[1])) >= 3


def tap_major(w):
    """Conv2d weight [co, ci, kh, 3] -> [kh * 3][co][ci] fp32, the layout csrc/sconv_x3.hip reads."""
    co, ci, kh, kw = w.shape
    return w.detach().float().permute(2, 3, 0, 1).reshape(kh * kw, co, ci).contiguous()


def bn_table(conv_bias, bn):
    """[4][C]: conv bias, running mean, invstd * gamma, beta of a frozen BatchNorm2d behind a convolution."""
    s = torch.rsqrt(bn.running_var.detach().float() + bn.eps) * bn.weight.detach().float()
    return torch.stack([conv_bias.detach().float(), bn.running_mean.detach().float(), s,
                        bn.bias.detach().float()]).contiguous()


class SincX3Weights:
    """Planes and fp32 tables of one SincNetEncoder for the x3 stream."""

    def __init__(self, enc):
        f = lambda t: t.detach().float().contiguous()   # noqa: E731
        with torch.no_grad():
            fb = enc.first_bn
            sc = torch.rsqrt(fb.running_var.detach().float() + fb.eps) * fb.weight.detach().float()
            self.fbn = torch.cat([sc, fb.bias.detach().float() - fb.running_mean.detach().float() * sc]).contiguous()
            b0 = enc.encoder[0][0]
            self.b0 = dict(w1=f(b0.conv1.weight.reshape(32, 6)), wd=f(b0.conv_downsample.weight.reshape(32, 3)),
                           bn=bn_table(b0.conv1.bias, b0.bn2), w2=wavlm_x3.planes(tap_major(b0.conv2.weight)),
                           bias=f(b0.conv2.bias + b0.conv_downsample.bias))
            self.blocks = []
            for seq in list(enc.encoder)[1:]:
                b = seq[0]
                d = dict(w1=wavlm_x3.planes(tap_major(b.conv1.weight)), bn=bn_table(b.conv1.bias, b.bn2),
                         w2=wavlm_x3.planes(tap_major(b.conv2.weight)), wd=None, bias=f(b.conv2.bias))
                if b.downsample:
                    d["wd"] = wavlm_x3.planes(tap_major(b.conv_downsample.weight))
                    d["bias"] = f(b.conv2.bias + b.conv_downsample.bias)
                self.blocks.append(d)


def weights(enc):
    key = wavlm_x3._src(enc)
    cur = enc.__dict__.get("_x3w")
    if cur is None or cur[0] != key:
        cur = (key, SincX3Weights(enc))
        enc.__dict__["_x3w"] = cur
    return cur[1]


def b0x(x, fbn, w1, wd, bn, w2, bias):
    """Block 0 on rdx_x3_b0x_fwd: x fp32 [N, H, W] -> fp32 NHWC [N, H, W // 3, 32]."""
    N, H, W = x.shape
    y = torch.empty(N, H, W // 3, 32, device=x.device, dtype=torch.float32)
    # conv2's three products dominate: 2 * 6 taps * 32 * 32 per position, x 3
    with _timed("x3_b0x_fwd", x, 3 * 2.0 * N * H * W * 6 * 32 * 32, shape=(N, H, W)):
        check(lib().rdx_x3_b0x_fwd(_p(x), _p(fbn) if fbn is not None else None, _p(w1), _p(wd), _p(bn), _p(w2[0]),
                                   _p(w2[1]), _p(bias), _p(y), N, H, W, _stream(x)), "x3_b0x_fwd")
    return y


def sconv(x, w, kh, ph, bn=None):
    """x fp32 NHWC [N, H, W, ci], w the (hi, lo) planes [kh * 3][co][ci] -> fp32 NHWC [N, H + 2 ph - kh + 1, W, co];
    bn [4][co]: selu(bn(acc + conv bias))."""
    N, H, W, ci = x.shape
    co = w[0].shape[1]
    Ho = H + 2 * ph - kh + 1
    y = torch.empty(N, Ho, W, co, device=x.device, dtype=torch.float32)
    with _timed("x3_sconv", x, 3 * 2.0 * N * Ho * W * kh * 3 * ci * co, shape=(N, H, W, ci, co, kh)):
        check(lib().rdx_x3_sconv_fwd(_p(x), _p(w[0]), _p(w[1]), _p(bn) if bn is not None else None, _p(y), N, H, W,
                                     ci, co, kh, ph, _stream(x)), "x3_sconv_fwd")
    return y


def res_tail(a, idn, bias):
    """MaxPool2d((1, 3))(a + idn + bias) on fp32 NHWC tensors (rdx_res_tail_fwd; its argmax bytes are not kept)."""
    N, H, W, C = a.shape
    y = torch.empty(N, H, W // 3, C, device=a.device, dtype=torch.float32)
    arg = torch.empty(N, H, W // 3, C, device=a.device, dtype=torch.uint8)
    check(lib().rdx_res_tail_fwd(_lib.RDX_F32, _p(a), _p(idn), _p(bias), _p(y), _p(arg), N * H, W, C, _stream(a)),
          "res_tail_fwd")
    return y


@torch.no_grad()
def forward(enc, x):
    """SincNetEncoder.forward (eval, no band mask) on the x3 kernels: x [B, L] -> e_T [B, T', 64] fp32."""
    W = weights(enc)
    p = sincconv_absmaxpool(x.float(), enc.conv_time.band_pass)            # [B, 23, L'] raw (before first_bn)
    b = W.b0
    h = b0x(p, W.fbn, b["w1"], b["wd"], b["bn"], b["w2"], b["bias"])       # [B, 23, L' // 3, 32]
    for b in W.blocks:
        a = sconv(sconv(h, b["w1"], 2, 1, bn=b["bn"]), b["w2"], 2, 0)
        idn = sconv(h, b["wd"], 1, 0) if b["wd"] is not None else h
        h = res_tail(a, idn, b["bias"])
    return h.abs().amax(dim=1)

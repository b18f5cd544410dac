"""Rounding-faithful fp64 restatement of the fused head ops (csrc/head.hip, radhip/head.py): squeeze-excitation over
time, attention pooling, and the align-and-concat of DualStreamFusion (reference src/models/DualStreamSEMamba.py
:492-531, :700-770, :537-637), forward AND backward, hand-written in plain torch on the CPU.

TEST INFRASTRUCTURE. Every function takes `rnd`, applied exactly where csrc/head.hip's header comments say a value is
rounded to the 16-bit storage type (where autocast's op would round it). `rounder(dtype)` gives the rounding of a
storage type, `identity` the exact operation; with `identity` the hand-written backward equals autograd through the
plain formula (tests/test_head_ref_cpu.py). All sums are fp64, so against a kernel the only differences left are the
order of its fp32 sums and the `__expf` of the SE gate's sigmoid.

Inputs are fp64 tensors holding values the storage type represents (the 16-bit tensors the kernel is given, widened).
For every gradient the kernels sum in fp32 (dW1, dW2, the pooling dw / db) the result carries `A`, the per-element sum
of the absolute values of the terms added: the scale a sum's rounding error is measured against.
"""
import numpy as np
import torch
import torch.nn.functional as F


def identity(v):
    return v


def rounder(dt):
    """Round-to-nearest-even to the storage type dt, kept in fp64."""
    return lambda v: v.to(dt).to(torch.float64)


def se(x, w1, w2, dy, rnd=identity):
    """y = x * sigmoid(relu(mean_t(x) W1^T) W2^T) for x, dy [B, T, C], w1 [R, C], w2 [C, R].

    Roundings, forward: m, h (before the relu), z, s, y. Backward: every product dy x before the sum over t and the sum
    itself (autocast's sum writes 16 bits; the kernel rounds it before the sigmoid's derivative), dz, dh, dm and dm / T
    (the mean's backward is a 16-bit division), round(dy s), and the 16-bit add of the two branches into dx.
    Returns a dict: y, m, h, s, dx and its two branches dx1, dx2, dw1 [R, C], dw2 [C, R], A1, A2.
    """
    T = x.shape[1]
    m = rnd(x.sum(1) / T)
    h = torch.relu(rnd(m @ w1.t()))
    z = rnd(h @ w2.t())
    s = rnd(torch.sigmoid(z))
    y = rnd(x * s[:, None, :])
    ds = rnd(rnd(dy * x).sum(1))
    dz = rnd(ds * (s * (1.0 - s)))
    dh = rnd(dz @ w2) * (h > 0)
    dm = rnd(rnd(dh @ w1) / T)
    dx1, dx2 = rnd(dy * s[:, None, :]), dm[:, None, :].expand_as(x)
    dx = rnd(dx1 + dx2)
    return {"y": y, "m": m, "h": h, "s": s, "dx": dx, "dx1": dx1, "dx2": dx2,
            "dw1": torch.einsum("br,bc->rc", dh, m), "A1": torch.einsum("br,bc->rc", dh.abs(), m.abs()),
            "dw2": torch.einsum("bc,br->cr", dz, h), "A2": torch.einsum("bc,br->cr", dz.abs(), h.abs())}


def se_plain(x, w1, w2):
    """The unrounded formula, for autograd."""
    return x * torch.sigmoid(torch.relu(x.mean(1) @ w1.t()) @ w2.t())[:, None, :]


def pool(f, w, b, dfeat, rnd=identity):
    """feat = softmax_t(f w + b)^T f for f [B, T, C], w [C], b a 0-dim tensor or None, dfeat [B, C].

    Roundings, forward: the scores z, a16 = round(a), feat. The softmax a is what the kernel and autocast hold in fp32:
    the fp64 softmax rounded to fp32 (whatever `rnd` is; with `identity` it stays exact).
    Backward: da = round(f dfeat), df1 = round(a16 dfeat), dz = round(a (da - sum_t a da)) on the fp32 a,
    df2 = round(dz w), df = round(df1 + df2).
    Returns a dict: feat, a, z, df and its two branches df1, df2, dw [C], db (0-dim), Aw, Ab.
    """
    z = f @ w
    if b is not None:
        z = z + b
    z = rnd(z)
    a = torch.softmax(z, 1)
    if rnd is not identity:
        a = a.float().double()
    a16 = rnd(a)
    feat = rnd(torch.einsum("bt,btc->bc", a16, f))
    da = rnd(torch.einsum("btc,bc->bt", f, dfeat))
    df1 = rnd(a16[:, :, None] * dfeat[:, None, :])
    dz = rnd(a * (da - (a * da).sum(1, keepdim=True)))
    df2 = rnd(dz[:, :, None] * w)
    df = rnd(df1 + df2)
    return {"feat": feat, "a": a, "z": z, "df": df, "df1": df1, "df2": df2,
            "dw": torch.einsum("bt,btc->c", dz, f), "Aw": torch.einsum("bt,btc->c", dz.abs(), f.abs()),
            "db": dz.sum(), "Ab": dz.abs().sum()}


def pool_plain(f, w, b):
    z = f @ w
    if b is not None:
        z = z + b
    return torch.einsum("bt,btc->bc", torch.softmax(z, 1), f)


def nearest_index(T1, T2):
    """F.interpolate(mode='nearest') source frame of each of T1 output frames: min(floor(t * scale), T2 - 1), the scale
    T2 / T1 and the product in fp32 as torch computes them."""
    scale = np.float32(T2) / np.float32(T1)
    idx = np.floor(np.arange(T1, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, T2 - 1))


def upcat(fw, fs, dout, rnd=identity):
    """out = cat([fw, fs[:, idx]], -1) for fw [B, T1, C], fs [B, T2, C], dout [B, T1, 2 C]; the forward copies values,
    the SincNet half's gradient is the sum of dout over the frames that read each source frame, rounded once; the WavLM
    half's is dout's first half.
    Returns a dict: out, dfw, dfs.
    """
    C = fw.shape[2]
    idx = nearest_index(fw.shape[1], fs.shape[1])
    out = torch.cat([fw, fs[:, idx]], -1)
    dfs = torch.zeros_like(fs).index_add_(1, idx, dout[..., C:])
    return {"out": out, "dfw": dout[..., :C], "dfs": rnd(dfs)}


def upcat_plain(fw, fs):
    up = F.interpolate(fs.permute(0, 2, 1), size=fw.shape[1], mode="nearest").permute(0, 2, 1)
    return torch.cat([fw, up], -1)


# ---- the error metric of tests/test_head_edges_gpu.py
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}            # unit roundoff
_EMIN = {torch.bfloat16: -126, torch.float16: -14}                       # exponent of the smallest normal


def ulp(v, dt):
    """Spacing of the storage type dt at |v| (fp64 tensor in, fp64 out; the subnormal spacing below the normals)."""
    e = torch.frexp(v.abs())[1].to(torch.float64) - 1.0                   # floor(log2 |v|); frexp(0) gives 0
    e = torch.where(v == 0, torch.full_like(e, _EMIN[dt]), e).clamp_min(_EMIN[dt])
    return torch.exp2(e) * (2.0 * EPS[dt])


def ulp_floored(ref, dt):
    """ulp(ref), floored at the spacing at 2^-14 max |ref| so that exact zeros do not make a bound vacuous."""
    return torch.maximum(ulp(ref, dt), ulp(ref.abs().max() * 2.0 ** -14, dt))


def dist16(got, ref, dt):
    """max over every element of |got - ref| / ulp_floored(ref): a 16-bit result's distance in ulps."""
    return float(((got - ref).abs() / ulp_floored(ref, dt)).max())


def dist16_sum(got, ref, branches, dt):
    """dist16 for a 16-bit sum of two 16-bit branches (dx, df): each element is measured in the largest of the spacings
    at the sum and at its branches. Where the branches cancel, one ulp of a branch is many ulps of the sum; against
    this scale a one-ulp flip of a branch reads as about 1 however far the sum cancels."""
    scale = ulp_floored(ref, dt)
    for b in branches:
        scale = torch.maximum(scale, ulp(b, dt))
    return float(((got - ref).abs() / scale).max())


def dist32(got, ref, A, dt):
    """max over every element of |got - ref| / (eps_dt A): an fp32-summed gradient's distance in units of one 16-bit
    rounding of its terms. Where no term was added (A == 0) anything but equality is infinitely far."""
    d = (got - ref).abs()
    r = torch.where(A > 0, d / (EPS[dt] * A).clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d),
                                                                             torch.full_like(d, float("inf"))))
    return float(r.max())

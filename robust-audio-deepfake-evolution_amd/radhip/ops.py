"""PyTorch-facing wrappers of the libradhip.so C ABI (device memory, streams and autograd only).

Every op here runs the hand-written HIP kernel on the tensor's current HIP stream; there is no CPU
path. Tensors must live on a ROCm device.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr_array

# 16-bit storage: bf16 on libradhip.so, fp16 on libradhip_f16.so (the same kernels built with -DRDX_F16,
# csrc/common.h); the dtype code 1 (RDX_BF16) names the library's 16-bit storage type in both
HALF = (torch.bfloat16, torch.float16)
_DT = {torch.float32: _lib.RDX_F32, torch.bfloat16: _lib.RDX_BF16, torch.float16: _lib.RDX_BF16}


def _L(*xs):
    """The library whose 16-bit storage type is that of the tensors / dtypes xs: libradhip_f16.so for fp16,
    libradhip.so otherwise (one call never mixes bf16 and fp16)."""
    dts = {x if isinstance(x, torch.dtype) else x.dtype for x in xs}
    if torch.float16 in dts:
        if torch.bfloat16 in dts:
            raise TypeError("radhip: one launch cannot mix bf16 and fp16 tensors")
        return _lib.lib16()
    return lib()


def half_dtype():
    """The 16-bit storage dtype of a fused op's forward: the CUDA autocast dtype (bf16 or fp16) when autocast
    is on, else bf16. Backward passes take it from their saved tensors."""
    if torch.is_autocast_enabled("cuda"):
        d = torch.get_autocast_dtype("cuda")
        if d in HALF:
            return d
    return torch.bfloat16

# Optional live timing: when TIMING is a dict, every C-ABI launch below is bracketed by two HIP events
# recorded on the stream it is launched on; TIMING[name] collects (start, end, work) tuples, where
# `work` is the launch's algorithmic bytes or FLOPs (bench.py turns these into the roofline line).
# Inside a HIP graph capture, events cannot become graph nodes on ROCm, so CAPTURE_TIMING (a
# GraphTimer) brackets each launch with two captured device-clock stamp kernels (rdx_timestamp_acc)
# that accumulate the launch's duration and count over every replay.
TIMING = None
CAPTURE_TIMING = None


class GraphTimer:
    """Per-launch-site accumulators [ticks, count] in device memory, filled by captured stamps. Only the
    first `per_graph` launch sites of each kernel in each captured graph are stamped (every stamp is
    itself a ~4.5 us graph node); the sites of one kernel in one graph have the same shape (e.g. the 24
    WavLM layers), so each sampled site stands for total / sampled of them and rows() scales its count
    and time by that factor: launches and total_ms are per-replay totals over ALL sites."""

    def __init__(self, device, capacity=1024, per_graph=2):
        self.device = torch.device(device)
        self.acc = torch.zeros(capacity, 2, dtype=torch.int64, device=self.device)
        self.sites = []                       # (name, work, group) per slot
        self.per_graph = per_graph
        self._in_graph = {}                   # name -> group record {"total", "sampled"} of this graph
        # one empty bracket (two back-to-back stamps) per graph: the stamps' own cost, subtracted from every
        # bracketed launch in rows() (a bracket holds the opening stamp kernel and the launch gaps around the kernel)
        self.calib = torch.zeros(64, 2, dtype=torch.int64, device=self.device)
        self._ncalib = 0

    def new_graph(self):
        """Call before capturing each graph."""
        self._in_graph = {}

    def calibrate(self, t):
        """Inside a capture: the graph's empty bracket, once per graph (before its first stamped launch)."""
        if self._in_graph.get("__calib__") or self._ncalib >= self.calib.shape[0]:
            return
        self._in_graph["__calib__"] = True
        site = self.calib[self._ncalib]
        self._ncalib += 1
        check(lib().rdx_timestamp_acc(_p(site), -1, _stream(t)), "timestamp")
        check(lib().rdx_timestamp_acc(_p(site), 1, _stream(t)), "timestamp")

    def overhead_ticks(self):
        """Average ticks of an empty bracket (0 before any calibrated replay)."""
        c = self.calib[:self._ncalib].cpu().numpy()
        n = int(c[:, 1].sum()) if len(c) else 0
        return float(c[:, 0].sum()) / n if n else 0.0

    def slot(self, name, work, shape=None):
        """shape: an extra key for kernels whose launch sites differ in size within one graph (the SincNet
        blocks, the CNN layers): sites are grouped (sampled and scaled) per (name, shape), reported per name."""
        grp = self._in_graph.setdefault((name, shape), {"total": 0, "sampled": 0})
        grp["total"] += 1
        if grp["sampled"] >= self.per_graph:
            return None
        grp["sampled"] += 1
        if len(self.sites) >= self.acc.shape[0]:
            raise RuntimeError("GraphTimer: out of slots")
        self.sites.append((name, float(work), grp, shape))
        return self.acc[len(self.sites) - 1]

    def reset(self):
        self.acc.zero_()
        self.calib.zero_()

    def rows(self, by_shape=False):
        """{name: {launches, total_ms, avg_ms, avg_work, sampled_launches}} over everything replayed since
        reset(): launches / total_ms count every launch site of the graphs (sampled sites scaled). by_shape:
        keyed "name[shape]" for the sites that carry a shape key (one row per (kernel, shape))."""
        khz = lib().rdx_wallclock_khz(self.device.index or 0)
        if khz <= 0:
            raise RuntimeError("rdx_wallclock_khz failed")
        acc = self.acc.cpu().numpy()
        ovh = self.overhead_ticks()
        out = {}
        for i, (name, work, grp, shape) in enumerate(self.sites):
            ticks, cnt = int(acc[i, 0]), int(acc[i, 1])
            if cnt == 0:
                continue
            ticks = max(ticks - ovh * cnt, 0.0)
            mult = grp["total"] / grp["sampled"]
            key = name if not by_shape or shape is None else f"{name}{list(shape)}"
            r = out.setdefault(key, {"launches": 0.0, "total_ms": 0.0, "work_sum": 0.0, "sampled_launches": 0})
            r["launches"] += cnt * mult
            r["total_ms"] += ticks / khz * mult
            r["work_sum"] += work * cnt * mult
            r["sampled_launches"] += cnt
        for r in out.values():
            r["avg_ms"] = r["total_ms"] / r["launches"]
            r["avg_work"] = r.pop("work_sum") / r["launches"]
            r["launches"] = int(round(r["launches"]))
        return out


class _timed:
    __slots__ = ("name", "t", "work", "ev", "reg", "site", "shape")

    def __init__(self, name, t, work=0.0, shape=None):
        self.name, self.t, self.work, self.shape = name, t, work, shape
        self.reg = self.site = None

    def __enter__(self):
        if CAPTURE_TIMING is not None and torch.cuda.is_current_stream_capturing():
            CAPTURE_TIMING.calibrate(self.t)
            self.site = CAPTURE_TIMING.slot(self.name, self.work, self.shape)   # None: not a sampled site
            if self.site is not None:
                check(lib().rdx_timestamp_acc(_p(self.site), -1, _stream(self.t)), "timestamp")
        elif TIMING is not None:
            self.reg = TIMING
            s = torch.cuda.current_stream(self.t.device)
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record(s)
        return self

    def __exit__(self, *exc):
        if self.site is not None:
            check(lib().rdx_timestamp_acc(_p(self.site), 1, _stream(self.t)), "timestamp")
        elif self.reg is not None:
            self.ev[1].record(torch.cuda.current_stream(self.t.device))
            self.reg.setdefault(self.name, []).append((self.ev[0], self.ev[1], self.work))
        return False


def event_rows(timing):
    """TIMING dict -> {name: {launches, total_ms, avg_ms, avg_work}} (call after synchronising)."""
    rows = {}
    for name, evs in timing.items():
        ms = [s.elapsed_time(e) for s, e, _ in evs]
        rows[name] = {"launches": len(ms), "total_ms": float(sum(ms)), "avg_ms": float(sum(ms) / len(ms)),
                      "avg_work": float(sum(w for _, _, w in evs) / len(evs))}
    return rows


def sinc_flops(B, C, K, L):
    """Algorithmic FLOPs of one fused SincConv launch: 2*K MACs for every conv output the 3x3 pool reads."""
    return 2.0 * K * B * (3 * (C // 3)) * (3 * ((L - K + 1) // 3))


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _dtype_code(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"radhip: unsupported dtype {t.dtype} (float32 / bfloat16 / float16 only)")


def _require_gpu(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("radhip ops run on the GPU only (tensor on %s)" % t.device)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------------- SincConv ----
def sinc_mfma_enabled(C, K):
    """The f16 MFMA SincConv under CUDA fp16 autocast (the reference's autocast runs this conv in fp16: the same
    input rounding), for banks of <= 80 channels x 160 taps. bf16 autocast and fp32 keep the fp32 kernel (rounding
    the conv's inputs to fp16 there would add an error the reference's fp16 run has but a bf16 run has no reason
    to carry); RADHIP_SINC_MFMA=0 keeps the fp32 kernel everywhere (A/B measurement)."""
    return (torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16
            and C <= 80 and K <= 160 and os.environ.get("RADHIP_SINC_MFMA", "1") != "0")


def sincconv_absmaxpool(x, filters, mask_lo=0, mask_hi=0, mask_dev=None):
    """|conv1d(x, filters)| max-pooled 3x3 over (channel, time): [B, L] -> [B, C//3, (L-K+1)//3].

    Replaces CONV.forward + F.max_pool2d(torch.abs(.), (3, 3))
    (reference src/models/DualStreamSEMamba.py:119-138, :250-253).
    """
    _require_gpu(x, filters)
    x = x.contiguous().float()
    filters = filters.contiguous().float()
    B, L = x.shape
    C, K = filters.shape
    out = torch.empty(B, C // 3, (L - K + 1) // 3, device=x.device, dtype=torch.float32)
    if sinc_mfma_enabled(C, K):
        # fp16 autocast (the training step, fp16 eval): the reference's conv1d runs in fp16 there
        # (src/main.py:1049) -> the f16 MFMA form; the other paths keep the exact fp32 kernel below
        per_utt = mask_dev is not None and mask_dev.dim() == 2
        if mask_dev is not None:
            assert mask_dev.dtype == torch.int32 and mask_dev.is_cuda and mask_dev.is_contiguous()
            assert (mask_dev.shape == (B, 2)) if per_utt else mask_dev.numel() >= 2
        with _timed("sincconv_mfma", x, sinc_flops(B, C, K, L)):
            check(lib().rdx_sincconv_absmaxpool_f16mfma(_p(x), B, L, _p(filters), C, K, int(mask_lo), int(mask_hi),
                                                        _p(mask_dev) if mask_dev is not None else None,
                                                        2 if per_utt else 0, _p(out), _stream(x)),
                  "sincconv_absmaxpool_f16mfma")
        return out
    with _timed("sincconv_absmaxpool", x, sinc_flops(B, C, K, L)):
        if mask_dev is not None:
            # int32 [2] (one mask for the batch) or [B, 2] (one per utterance)
            per_utt = mask_dev.dim() == 2
            assert mask_dev.dtype == torch.int32 and mask_dev.is_cuda and mask_dev.is_contiguous()
            assert (mask_dev.shape == (B, 2)) if per_utt else mask_dev.numel() >= 2
            check(lib().rdx_sincconv_absmaxpool_fwd_devmask(_p(x), B, L, _p(filters), C, K, _p(mask_dev),
                                                            2 if per_utt else 0, _p(out), _stream(x)),
                  "sincconv_absmaxpool_fwd_devmask")
        else:
            check(lib().rdx_sincconv_absmaxpool_fwd(_p(x), B, L, _p(filters), C, K, int(mask_lo), int(mask_hi),
                                                    _p(out), _stream(x)), "sincconv_absmaxpool_fwd")
    return out


def sincconv_abspool1d(x, filters, mask_lo=0, mask_hi=0):
    """|conv1d(x, filters)| max-pooled over 3 conv times per channel: [B, L] -> [B, C, (L-K+1)//3].

    Replaces RawNet2's SincConv.forward + F.max_pool1d(torch.abs(.), 3)
    (reference models/RawNet2Spoof.py:77-103, :244-245)."""
    _require_gpu(x, filters)
    x = x.contiguous().float()
    filters = filters.contiguous().float()
    B, L = x.shape
    C, K = filters.shape
    out = torch.empty(B, C, (L - K + 1) // 3, device=x.device, dtype=torch.float32)
    with _timed("sincconv_abspool1d", x, 2.0 * K * B * C * 3 * ((L - K + 1) // 3)):
        check(lib().rdx_sincconv_abspool1d_fwd(_p(x), B, L, _p(filters), C, K, int(mask_lo), int(mask_hi),
                                               _p(out), _stream(x)), "sincconv_abspool1d_fwd")
    return out


# ------------------------------------------------------------------------------ Bi-Mamba -------
def _rowview_ld(x):
    """x: [B, L, D] view with unit inner stride and rows of stride ld; returns ld."""
    B, L, D = x.shape
    if x.stride(2) != 1 or x.stride(0) != L * x.stride(1):
        raise ValueError("radhip: expected a [B, L, D] row view (inner stride 1, batch stride L*ld)")
    return x.stride(1)


class DWConvBidir(torch.autograd.Function):
    """Depthwise causal conv + SiLU for both scan directions (mamba causal_conv1d stage)."""

    @staticmethod
    def forward(ctx, x, weight, bias, dirs):
        _require_gpu(x)
        B, L, D = x.shape
        ldx = _rowview_ld(x)
        w = weight.reshape(D, -1).contiguous().float()
        b = bias.contiguous().float()
        K = w.shape[1]
        u = torch.empty(dirs, B, L, D, device=x.device, dtype=x.dtype)
        check(_L(x).rdx_dwconv_bidir_fwd(_dtype_code(x), _p(x), ldx, _p(w), _p(b), _p(u), B, L, D, K, dirs,
                                         _stream(x)), "dwconv_bidir_fwd")
        ctx.save_for_backward(x, w, b)
        ctx.dirs = dirs
        ctx.wshape = weight.shape
        return u

    @staticmethod
    def backward(ctx, du):
        x, w, b = ctx.saved_tensors
        B, L, D = x.shape
        K = w.shape[1]
        du = du.contiguous().to(x.dtype)
        dx = torch.empty(B, L, D, device=x.device, dtype=x.dtype)
        parts = lib().rdx_dwconv_bidir_bwd_parts(L) * B
        # weight and bias partials packed into one [parts][D*K + D] buffer: one reduction launch for both
        part = torch.empty(parts, D * K + D, device=x.device, dtype=torch.float32)
        check(_L(x).rdx_dwconv_bidir_bwd(_dtype_code(x), _p(x), _rowview_ld(x), _p(w), _p(b), _p(du), _p(dx), D,
                                         _p(part), ctypes.c_void_p(part.data_ptr() + 4 * D * K), D * K + D,
                                         B, L, D, K, ctx.dirs, _stream(x)),
              "dwconv_bidir_bwd")
        tot = part.sum(0)
        return dx, tot[:D * K].view(ctx.wshape), tot[D * K:], None


def scan2_enabled():
    """The chunked two-level scan (csrc/scan2.hip) by default; RADHIP_SCAN2=0 runs csrc/bimamba.hip's segmented
    kernels (A/B measurement, parity tests of both)."""
    return os.environ.get("RADHIP_SCAN2", "1") != "0"


class SelectiveScan(torch.autograd.Function):
    """y[dir] = scan(u[dir], softplus(delta[dir] + dt_bias), A = -exp(A_log), B, C) + D*u[dir]."""

    @staticmethod
    def forward(ctx, u, delta, A_log, Bm, Cm, Dp, dt_bias):
        _require_gpu(u)
        dirs, B, L, D = u.shape
        N = A_log.shape[1]
        dt = u.dtype
        u = u.contiguous()
        delta = delta.contiguous().to(dt)
        if Bm.dtype != dt:
            Bm, Cm = Bm.to(dt), Cm.to(dt)
        ldbc = Bm.stride(2)
        if Bm.stride(3) != 1 or Cm.stride(2) != ldbc or Bm.stride(1) != L * ldbc or Bm.stride(0) != B * L * ldbc:
            raise ValueError("radhip: B / C must be column slices of one [dirs, B, L, R+2N] tensor")
        A_log = A_log.contiguous().float()
        Dp = Dp.contiguous().float()
        dt_bias = dt_bias.contiguous().float()
        y = torch.empty(dirs, B, L, D, device=u.device, dtype=torch.float32)
        ck = torch.empty(lib().rdx_scan_ckpt_elems(B, L, D, N, dirs), device=u.device, dtype=torch.float32)
        es = u.element_size()
        chunked = scan2_enabled()
        if chunked:     # csrc/scan2.hip: per-chunk decay products P are kept for the backward
            nrec = int(lib().rdx_scan2_rec_elems(B, L, D, N, dirs))
            P = torch.empty(nrec, device=u.device, dtype=torch.float32)
            hloc = torch.empty(nrec, device=u.device, dtype=torch.float32)
            with _timed("selective_scan_fwd", u, dirs * B * L * (D * (2 * es + 4) + 2 * N * es)):
                check(_L(u).rdx_scan2_fwd(_dtype_code(u), _p(u), _p(delta), _p(A_log), _p(Bm), _p(Cm), ldbc, _p(Dp),
                                          _p(dt_bias), _p(y), _p(ck), _p(P), _p(hloc), B, L, D, N, dirs, _stream(u)),
                      "scan2_fwd")
        else:
            P = torch.empty(0, device=u.device, dtype=torch.float32)
            with _timed("selective_scan_fwd", u, dirs * B * L * (D * (2 * es + 4) + 2 * N * es)):
                check(_L(u).rdx_selective_scan_fwd(_dtype_code(u), _p(u), _p(delta), _p(A_log), _p(Bm), _p(Cm),
                                                   ldbc, _p(Dp), _p(dt_bias), _p(y), _p(ck), B, L, D, N, dirs,
                                                   _stream(u)), "selective_scan_fwd")
        ctx.save_for_backward(u, delta, A_log, Bm, Cm, Dp, dt_bias, ck, P)
        ctx.ldbc = ldbc
        ctx.chunked = chunked
        return y

    @staticmethod
    def backward(ctx, dy):
        u, delta, A_log, Bm, Cm, Dp, dt_bias, ck, P = ctx.saved_tensors
        dirs, B, L, D = u.shape
        N = A_log.shape[1]
        dy = dy.float()
        if dirs > 1 and dy.stride(0) == 0 and dy[0].is_contiguous():
            dy_stride = 0
        else:
            dy = dy.contiguous()
            dy_stride = B * L * D
        du = torch.empty_like(u)
        ddelta = torch.empty_like(u)
        # dB | dC, accumulated atomically: scan2 zeroes it itself, the segmented kernels need it zeroed
        dBC = (torch.empty if ctx.chunked else torch.zeros)(dirs, B, L, 2 * N, device=u.device, dtype=torch.float32)
        es = u.element_size()
        if ctx.chunked:
            # dA_log / D / dt_bias partials of every (dir, b, chunk) packed into one [parts][D*N + 2D] buffer:
            # one reduction launch for the three
            parts = dirs * B * int(lib().rdx_scan2_chunks(L))
            part = torch.empty(parts, D * N + 2 * D, device=u.device, dtype=torch.float32)
            base = part.data_ptr()
            gloc = torch.empty(int(lib().rdx_scan2_rec_elems(B, L, D, N, dirs)), device=u.device, dtype=torch.float32)
            with _timed("selective_scan_bwd", u, dirs * B * L * (D * (4 * es + 4) + 2 * N * es)):
                check(_L(u).rdx_scan2_bwd(_dtype_code(u), _p(u), _p(delta), _p(A_log), _p(Bm), _p(Cm), ctx.ldbc,
                                          _p(Dp), _p(dt_bias), _p(ck), _p(P), _p(dy), dy_stride, _p(du), _p(ddelta),
                                          _p(dBC), ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * D * N),
                                          ctypes.c_void_p(base + 4 * (D * N + D)), D * N + 2 * D, _p(gloc), B, L, D,
                                          N, dirs, _stream(u)),
                      "scan2_bwd")
            tot = part.sum(0)
            dBC = dBC.to(Bm.dtype)
            return (du, ddelta, tot[:D * N].view(D, N), dBC[..., :N], dBC[..., N:], tot[D * N:D * N + D],
                    tot[D * N + D:])
        else:
            parts = dirs * B
            dA = torch.empty(parts, D, N, device=u.device, dtype=torch.float32)
            dD = torch.empty(parts, D, device=u.device, dtype=torch.float32)
            dbias = torch.empty(parts, D, device=u.device, dtype=torch.float32)
            with _timed("selective_scan_bwd", u, dirs * B * L * (D * (4 * es + 4) + 2 * N * es)):
                check(_L(u).rdx_selective_scan_bwd(_dtype_code(u), _p(u), _p(delta), _p(A_log), _p(Bm), _p(Cm),
                                                   ctx.ldbc, _p(Dp), _p(dt_bias), _p(ck), _p(dy), dy_stride, _p(du),
                                                   _p(ddelta), _p(dBC), _p(dA), _p(dD), _p(dbias), B, L, D, N, dirs,
                                                   _stream(u)), "selective_scan_bwd")
        dBC = dBC.to(Bm.dtype)
        return du, ddelta, dA.sum(0), dBC[..., :N], dBC[..., N:], dD.sum(0), dbias.sum(0)


class BiGate(torch.autograd.Function):
    """g = (sum over directions of y) * silu(z)."""

    @staticmethod
    def forward(ctx, y, z):
        _require_gpu(y, z)
        dirs, B, L, D = y.shape
        y = y.contiguous()
        ldz = _rowview_ld(z)
        g = torch.empty(B, L, D, device=z.device, dtype=z.dtype)
        ysum = torch.empty(B, L, D, device=z.device, dtype=torch.float32)
        check(_L(z).rdx_bigate_fwd(_dtype_code(z), _p(y), dirs, _p(z), ldz, _p(g), _p(ysum), B, L, D, _stream(z)),
              "bigate_fwd")
        ctx.save_for_backward(z, ysum)
        ctx.dirs = dirs
        return g

    @staticmethod
    def backward(ctx, dg):
        z, ysum = ctx.saved_tensors
        B, L, D = z.shape
        dg = dg.contiguous().to(z.dtype)
        dy = torch.empty(B, L, D, device=z.device, dtype=torch.float32)
        dz = torch.empty(B, L, D, device=z.device, dtype=z.dtype)
        check(_L(z).rdx_bigate_bwd(_dtype_code(z), _p(dg), _p(z), _rowview_ld(z), _p(ysum), _p(dy), _p(dz), D, B, L,
                                   D, _stream(z)), "bigate_bwd")
        return dy.unsqueeze(0).expand(ctx.dirs, B, L, D), dz


# ------------------------------------------------------------------- layer-weighted sum ------
class LayerWeightedSum(torch.autograd.Function):
    """sum_l softmax(w)_l * h_l over the WavLM hidden states, without stacking them.

    `deferred` (radhip.wavlm_fused.EncoderChain, or None): states whose gradient softmax(w)_l * g the backward
    does NOT write; it leaves g and softmax(w) on the object instead, and the fused layer that takes that state
    as its input adds the term inside its LN1 backward (rdx_wl_ln1_bwd_ex), so no [M, E] gradient is written
    and no autograd add runs per layer."""

    @staticmethod
    def forward(ctx, w, deferred, *hs):
        _require_gpu(w, *hs)
        h0 = hs[0]
        dt = h0.dtype
        hs = tuple(h if (h.dtype == dt and h.is_contiguous()) else h.to(dt).contiguous() for h in hs)
        wf = w.detach().contiguous().float()
        out = torch.empty_like(hs[0])
        with _timed("layer_wsum_fwd", out, (len(hs) + 1) * out.numel() * out.element_size()):
            check(_L(h0).rdx_layer_wsum_fwd(_dtype_code(h0), len(hs), ptr_array([h.data_ptr() for h in hs]), _p(wf),
                                           _p(out), out.numel(), _stream(out)), "layer_wsum_fwd")
        ctx.save_for_backward(wf, *hs)
        ctx.deferred = deferred
        return out

    @staticmethod
    def backward(ctx, g):
        wf, *hs = ctx.saved_tensors
        dfr = ctx.deferred
        skip = dfr.indices if dfr is not None and g.dtype == torch.float32 and hs[0].dtype == torch.float32 else ()
        g = g.contiguous().to(hs[0].dtype)
        dhs = [None if l in skip else torch.empty_like(h) for l, h in enumerate(hs)]
        n = g.numel()
        nblk = lib().rdx_layer_wsum_nblk(n)
        dots = torch.empty(nblk, len(hs), device=g.device, dtype=torch.float32)
        nwrite = sum(d is not None for d in dhs)
        with _timed("layer_wsum_bwd", g, (len(hs) + nwrite + 1) * n * g.element_size()):
            check(_L(g).rdx_layer_wsum_bwd(_dtype_code(g), len(hs), ptr_array([h.data_ptr() for h in hs]), _p(wf),
                                           _p(g), ptr_array([d.data_ptr() if d is not None else 0 for d in dhs]),
                                           _p(dots), n, _stream(g)), "layer_wsum_bwd")
        dots = dots.sum(0)
        p = torch.softmax(wf, 0)
        if skip:
            dfr.g, dfr.p = g, p.contiguous()
        dw = p * (dots - (p * dots).sum())
        return (dw, None, *dhs)


def layer_weighted_sum(hidden_states, layer_weights, deferred=None):
    return LayerWeightedSum.apply(layer_weights, deferred, *hidden_states)


class SplitLast(torch.autograd.Function):
    """x[..., a:b] views of consecutive last-dim ranges whose backward is ONE concatenation of the parts'
    gradients, instead of one zero-fill + copy per slice and an add per extra slice (SliceBackward)."""

    @staticmethod
    def forward(ctx, x, *sizes):
        ctx.sizes, ctx.dtype = sizes, x.dtype
        outs, o = [], 0
        for n in sizes:
            outs.append(x.narrow(-1, o, n))
            o += n
        if o != x.shape[-1]:
            raise ValueError("SplitLast: the sizes must cover the last dimension")
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        return (torch.cat([g.to(ctx.dtype) for g in grads], dim=-1),) + (None,) * len(ctx.sizes)


# ----------------------------------------------------------------------------------- loss ----
class MixupFocal(torch.autograd.Function):
    """scale * sum_b [lam_b focal(z_b, ya_b) + (1 - lam_b) focal(z_b, yb_b)] on csrc/loss.hip: the value and
    d/dlogits in one launch, the backward in one more (lam_b = lam[b // rows_per_lam], a device tensor)."""

    @staticmethod
    def forward(ctx, logits, ya, yb, lam, rows_per_lam, alpha, gamma, mode, scale):
        _require_gpu(logits, ya)
        if logits.dim() != 2 or logits.dtype not in (*HALF, torch.float32) or logits.stride(1) != 1:
            raise ValueError("mixup focal: [B, C] bf16/fp16/fp32 logits with unit column stride required")
        B, C = logits.shape
        ya = ya.contiguous()
        yb = yb.contiguous() if yb is not None else None
        lam = lam.contiguous().float() if lam is not None else None
        if ya.dtype != torch.int64 or ya.numel() != B or (yb is not None and (yb.dtype != torch.int64 or yb.numel() != B)):
            raise ValueError("mixup focal: int64 labels of B entries required")
        if lam is not None and lam.numel() * rows_per_lam < B:
            raise ValueError("mixup focal: lam has too few entries for the rows")
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        d32 = torch.empty(B, C, device=logits.device, dtype=torch.float32)
        check(_L(logits).rdx_focal_mixup_fwd(_p(logits), int(logits.dtype in HALF), logits.stride(0), B, C, _p(ya),
                                        _p(yb) if yb is not None else None, _p(lam) if lam is not None else None,
                                        int(rows_per_lam), float(alpha), float(gamma), int(mode), float(scale),
                                        _p(loss), _p(d32), _stream(logits)), "focal_mixup_fwd")
        ctx.save_for_backward(d32)
        ctx.out_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        d32, = ctx.saved_tensors
        g = g.float().contiguous()
        out = torch.empty(d32.shape, device=d32.device, dtype=ctx.out_dtype)
        check(_L(ctx.out_dtype).rdx_focal_mixup_bwd(_p(g), _p(d32), _p(out), int(ctx.out_dtype in HALF), d32.numel(),
                                        _stream(d32)), "focal_mixup_bwd")
        return out, None, None, None, None, None, None, None, None


def mixup_focal(logits, ya, yb, lam, rows_per_lam, focal, divisor):
    """The mixup focal criterion of a pass, divided by `divisor` (the accumulation steps), for a
    radhip.train.FocalLoss `focal`: per_class mode averages each micro-batch of rows_per_lam rows over its
    rows * C elements, scalar mode over its rows."""
    C = logits.shape[1]
    mode = 0 if focal.alpha_mode == "per_class" else 1
    scale = 1.0 / (rows_per_lam * (C if mode == 0 else 1) * divisor)
    alpha = -1.0 if focal.alpha is None else float(focal.alpha)
    return MixupFocal.apply(logits, ya, yb, lam, rows_per_lam, alpha, float(focal.gamma), mode, scale)


def ocsupcon_eligible(feats, rows_per_lam, center=None):
    """True when csrc/ocsupcon.hip takes these features (and centre): a [R, D] bf16 / fp16 / fp32 device tensor with
    unit column stride and the shape limits the library states (rdx_ocsupcon_eligible: 2 <= B <= 64, D <= 256,
    R % B == 0, 16-byte-aligned base), the centre a contiguous fp32 device tensor of D elements. Callers take the
    module path (radhip.train.OCSoftmax / SupConLoss) otherwise."""
    if not (torch.is_tensor(feats) and feats.is_cuda and feats.dim() == 2 and feats.dtype in (*HALF, torch.float32)
            and feats.stride(1) == 1 and feats.shape[0] > 0):
        return False
    if center is not None and not (center.is_cuda and center.dtype == torch.float32 and center.is_contiguous()
                                   and center.numel() == feats.shape[1]):
        return False
    return bool(_L(feats).rdx_ocsupcon_eligible(_p(feats), feats.stride(0), feats.shape[0], feats.shape[1],
                                                int(rows_per_lam)))


class MixupOcSupcon(torch.autograd.Function):
    """scale * sum_k [lam_k L_k(ya) + (1 - lam_k) L_k(yb)], L = OC-Softmax(feats, center) + lambda * SupCon(feats),
    on csrc/ocsupcon.hip: the value, d/dfeats and each micro-batch's d/dcenter in one launch, the backward in one
    more (lam_k = lam[k], a device tensor; micro-batch k = rows [k * rows_per_lam, (k + 1) * rows_per_lam)).
    center None: SupCon alone. The centre is read through its own storage (no copy), so a captured launch sees
    every later optimizer update. Shapes outside ocsupcon_eligible raise (the C entry's RDX_EUNSUPPORTED)."""

    @staticmethod
    def forward(ctx, feats, center, ya, yb, lam, rows_per_lam, r_real, r_fake, alpha, lambda_supcon, temperature,
                base_temperature, scale):
        _require_gpu(feats, ya)
        if feats.dim() != 2 or feats.dtype not in (*HALF, torch.float32) or feats.stride(1) != 1:
            raise ValueError("mixup ocsupcon: [R, D] bf16/fp16/fp32 features with unit column stride required")
        R, D = feats.shape
        B = int(rows_per_lam)
        if center is not None and not (center.is_cuda and center.dtype == torch.float32 and center.is_contiguous()
                                       and center.numel() == D):
            raise ValueError("mixup ocsupcon: the centre must be a contiguous fp32 device tensor of D elements")
        ya = ya.contiguous()
        yb = yb.contiguous() if yb is not None else None
        lam = lam.contiguous().float() if lam is not None else None
        if ya.dtype != torch.int64 or ya.numel() != R or (yb is not None and (yb.dtype != torch.int64 or yb.numel() != R)):
            raise ValueError("mixup ocsupcon: int64 labels of R entries required")
        if lam is not None and B > 0 and lam.numel() * B < R:
            raise ValueError("mixup ocsupcon: lam has too few entries for the rows")
        K = R // B if B > 0 and R % B == 0 else 1
        dev = feats.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        parts = torch.empty(K, device=dev, dtype=torch.float32) if K > 1 else None
        d32 = torch.empty(R, D, device=dev, dtype=torch.float32)
        dcp = torch.empty(K, D, device=dev, dtype=torch.float32) if center is not None else None
        check(_L(feats).rdx_ocsupcon_mixup_fwd(
            _p(feats), int(feats.dtype in HALF), feats.stride(0), R, D, _p(center) if center is not None else None,
            _p(ya), _p(yb) if yb is not None else None, _p(lam) if lam is not None else None, B, float(r_real),
            float(r_fake), float(alpha), float(lambda_supcon), float(temperature), float(base_temperature),
            float(scale), _p(loss), _p(parts) if parts is not None else None, _p(d32),
            _p(dcp) if dcp is not None else None, _stream(feats)), "ocsupcon_mixup_fwd")
        ctx.save_for_backward(d32, dcp)
        ctx.out_dtype = feats.dtype
        ctx.center_shape = center.shape if center is not None else None
        return loss

    @staticmethod
    def backward(ctx, g):
        d32, dcp = ctx.saved_tensors
        g = g.float().contiguous()
        out = torch.empty(d32.shape, device=d32.device, dtype=ctx.out_dtype)
        dc = torch.empty(ctx.center_shape, device=d32.device, dtype=torch.float32) if dcp is not None else None
        check(_L(ctx.out_dtype).rdx_ocsupcon_mixup_bwd(
            _p(g), _p(d32), _p(out), int(ctx.out_dtype in HALF), d32.numel(), _p(dcp) if dcp is not None else None,
            dcp.shape[0] if dcp is not None else 0, d32.shape[1], _p(dc) if dc is not None else None, _stream(d32)),
            "ocsupcon_mixup_bwd")
        return (out, dc) + (None,) * 11


def mixup_ocsupcon(feats, ya, yb, lam, rows_per_lam, oc, supcon, lambda_supcon, divisor):
    """The feature-side criteria of a pass, divided by `divisor` (the accumulation steps): `oc` a
    radhip.train.OCSoftmax or None, `supcon` a radhip.train.SupConLoss or None (then lambda_supcon is ignored); each
    micro-batch of rows_per_lam rows is averaged over its rows."""
    if oc is None and supcon is None:
        raise ValueError("mixup ocsupcon: neither OC-Softmax nor SupCon given")
    lsc = float(lambda_supcon) if supcon is not None else 0.0
    if oc is None and lsc == 0.0:
        return feats.float().sum() * 0.0        # SupCon alone at weight 0: no criterion left to launch
    return MixupOcSupcon.apply(feats, oc.center if oc is not None else None, ya, yb, lam, rows_per_lam,
                               oc.r_real if oc is not None else 0.0, oc.r_fake if oc is not None else 0.0,
                               oc.alpha if oc is not None else 0.0, lsc,
                               supcon.temperature if supcon is not None else 1.0,
                               supcon.base_temperature if supcon is not None else 1.0, 1.0 / divisor)


# ------------------------------------------------------------------------ graph attention ----
def gat_eligible(x, att_proj, att_weight, temp=1.0):
    """True when csrc/gat.hip takes this graph-attention layer: x a [B, N, Din] bf16 / fp16 / fp32 device tensor
    (GatAtt casts it to contiguous fp32), att_proj a Linear(Din, Dout) with a bias, att_weight of Dout elements, and
    the shape limits the library states (rdx_gat_eligible: N <= 32, Din <= 64, Dout <= 64, temp > 0). Callers take
    the module path otherwise (CPU tensors, float64, larger graphs)."""
    W, b = att_proj.weight, att_proj.bias
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.dtype in (*HALF, torch.float32) and x.numel() > 0):
        return False
    if b is None or not (W.is_cuda and W.dim() == 2 and W.shape[1] == x.shape[2] and att_weight.is_cuda
                         and att_weight.numel() == W.shape[0] and b.numel() == W.shape[0]):
        return False
    # the alignment rule is checked on a buffer of the allocator x's fp32 copy would come from
    probe = x if x.dtype == torch.float32 and x.is_contiguous() else W
    return bool(lib().rdx_gat_eligible(_p(probe), x.shape[1], x.shape[2], W.shape[0], float(temp)))


class GatAtt(torch.autograd.Function):
    """(agg, att) of one graph-attention layer on csrc/gat.hip, one workgroup per utterance:
    att[b] = softmax_j((tanh(W (x_i * x_j) + bias) . w) / temp), agg[b] = att[b] @ x[b]. x [B, N, Din], W [Dout, Din],
    bias [Dout], w [Dout], all contiguous fp32 on the device (gat_att prepares them); att is returned for inspection
    and takes no gradient. The backward recomputes tanh from the saved att, writes each utterance's dW / dbias / dw
    to its own slot and adds the slots with torch.sum over dim 0 (a fixed order): no atomics, the same bits every
    time. Shapes outside gat_eligible raise (the C entry's RDX_EUNSUPPORTED)."""

    @staticmethod
    def forward(ctx, x, W, bias, w, temp):
        _require_gpu(x, W, bias, w)
        for t, what in ((x, "x"), (W, "W"), (bias, "bias"), (w, "w")):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"gat: {what} must be a contiguous fp32 tensor")
        if x.dim() != 3 or W.dim() != 2 or W.shape[1] != x.shape[2] or bias.numel() != W.shape[0] or \
                w.numel() != W.shape[0] or x.numel() == 0:
            raise ValueError(f"gat: x [B, N, Din], W [Dout, Din], bias [Dout], w [Dout] required, got "
                             f"{tuple(x.shape)}, {tuple(W.shape)}, {tuple(bias.shape)}, {tuple(w.shape)}")
        if not float(temp) > 0:
            raise ValueError("gat: the temperature must be positive")
        B, N, Din = x.shape
        att = torch.empty(B, N, N, device=x.device, dtype=torch.float32)
        agg = torch.empty(B, N, Din, device=x.device, dtype=torch.float32)
        check(lib().rdx_gat_att_fwd(_p(x), _p(W), _p(bias), _p(w), float(temp), B, N, Din, W.shape[0], _p(att),
                                    _p(agg), _stream(x)), "gat_att_fwd")
        ctx.save_for_backward(x, W, bias, w, att)
        ctx.temp = float(temp)
        ctx.mark_non_differentiable(att)
        return agg, att

    @staticmethod
    def backward(ctx, dagg, _datt):
        x, W, bias, w, att = ctx.saved_tensors
        B, N, Din = x.shape
        Dout = W.shape[0]
        dagg = dagg.float().contiguous()
        dx = torch.empty_like(x)
        parts = any(ctx.needs_input_grad[1:4])
        dWp = torch.empty(B, Dout, Din, device=x.device, dtype=torch.float32) if parts else None
        dbp = torch.empty(B, Dout, device=x.device, dtype=torch.float32) if parts else None
        dwp = torch.empty(B, Dout, device=x.device, dtype=torch.float32) if parts else None
        q = lambda t: _p(t) if t is not None else None
        check(lib().rdx_gat_att_bwd(_p(dagg), _p(x), _p(W), _p(bias), _p(w), ctx.temp, _p(att), B, N, Din, Dout,
                                    _p(dx), q(dWp), q(dbp), q(dwp), _stream(x)), "gat_att_bwd")
        need = ctx.needs_input_grad
        return (dx if need[0] else None, dWp.sum(0) if need[1] else None,
                dbp.sum(0).view_as(bias) if need[2] else None, dwp.sum(0).view_as(w) if need[3] else None, None)


def gat_att(x, att_proj, att_weight, temp=1.0):
    """GatAtt over a layer's own tensors: x may be a transposed view or a 16-bit autocast tensor (made contiguous
    fp32 here, whatever autocast says), att_weight is the layer's [Dout, 1] parameter. Returns (agg, att) in fp32."""
    if x.dim() != 3:
        raise ValueError(f"gat: x must be [B, N, Din], got {tuple(x.shape)}")
    if att_proj.bias is None:
        raise ValueError("gat: att_proj needs a bias")
    return GatAtt.apply(x.float().contiguous(), att_proj.weight.float().contiguous(),
                        att_proj.bias.float().contiguous(), att_weight.float().reshape(-1), temp)


# --------------------------------------------------------------------------- multi-tensor cast ----
def cast_many(srcs, dsts):
    """dsts[k] = srcs[k] rounded to the dsts' 16-bit dtype (bf16 or fp16), fp32 contiguous sources, one launch per
    64 tensors (csrc/layersum.hip rdx_cast_f32_many)."""
    if not srcs:
        return
    dt = dsts[0].dtype
    if dt not in HALF or len(srcs) != len(dsts):
        raise ValueError("radhip cast_many: 16-bit destinations, one per source")
    for a, b in zip(srcs, dsts):
        if (a.dtype != torch.float32 or b.dtype != dt or a.numel() != b.numel() or not a.is_contiguous()
                or not b.is_contiguous() or not a.is_cuda or a.device != b.device):
            raise ValueError("radhip cast_many: contiguous fp32 -> 16-bit tensors of equal size on one device")
    for i in range(0, len(srcs), 64):
        s, d = srcs[i:i + 64], dsts[i:i + 64]
        check(_L(dt).rdx_cast_f32_many(len(s), ptr_array([t.data_ptr() for t in s]),
                                       ptr_array([t.data_ptr() for t in d]),
                                       (ctypes.c_int64 * len(s))(*[t.numel() for t in s]), _stream(s[0])),
              "cast_f32_many")


def add_many(dsts, srcs, copy=False):
    """dsts[k] += srcs[k] (copy: dsts[k] = srcs[k]) for contiguous fp32 tensors, one launch per 64 pairs
    (csrc/layersum.hip rdx_add_f32_many; the same fp32 adds as torch._foreach_add_)."""
    if len(dsts) != len(srcs):
        raise ValueError("radhip add_many: one source per destination")
    if not dsts:
        return
    _require_gpu(*dsts)
    for d, s in zip(dsts, srcs):
        if (d.dtype != torch.float32 or s.dtype != torch.float32 or d.numel() != s.numel() or not d.is_contiguous()
                or not s.is_contiguous() or d.device != s.device):
            raise ValueError("radhip add_many: contiguous fp32 tensors of equal size on one device")
    for i in range(0, len(dsts), 64):
        d, s = dsts[i:i + 64], srcs[i:i + 64]
        check(lib().rdx_add_f32_many(len(d), ptr_array([t.data_ptr() for t in d]), ptr_array([t.data_ptr() for t in s]),
                                     (ctypes.c_int64 * len(d))(*[t.numel() for t in d]), int(bool(copy)),
                                     _stream(d[0])), "add_f32_many")


# ------------------------------------------------------------------------------------ FGM ----
def fgm_attack(params, grads, backups, eps):
    """backup <- p; p += eps * g / ||g|| per tensor (skip when the norm is 0 or NaN). fp32 tensors."""
    assert len(params) == len(grads) == len(backups) and len(params) > 0
    _require_gpu(*params)
    for p, g, b in zip(params, grads, backups):
        assert p.dtype == g.dtype == b.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous()
    ws = torch.empty(len(params) * 256, device=params[0].device, dtype=torch.float64)
    n = len(params)
    numels = (ctypes.c_int64 * n)(*[p.numel() for p in params])
    check(lib().rdx_fgm_attack(n, ptr_array([p.data_ptr() for p in params]), ptr_array([g.data_ptr() for g in grads]),
                               ptr_array([b.data_ptr() for b in backups]), numels, float(eps), _p(ws),
                               _stream(params[0])), "fgm_attack")


# ---------------------------------------------------------------------------- augmentation ----
def rawboost_batch(x_flat, records, noise_isd=None, noise_ssi=None):
    """Apply RawBoost to every utterance of a flat fp32 buffer; records: list of RawboostUtt."""
    _require_gpu(x_flat)
    x_flat = x_flat.contiguous().float()
    out = torch.empty_like(x_flat)
    n = len(records)
    for r in records:
        if r.offset < 0 or r.len <= 0 or r.offset + r.len > x_flat.numel():
            raise ValueError(f"rawboost record [{r.offset}, +{r.len}) outside the {x_flat.numel()}-sample buffer")
        if noise_isd is not None and r.offset + r.len > noise_isd.numel():
            raise ValueError("noise_isd shorter than the records")
        if noise_ssi is not None and r.offset + r.len > noise_ssi.numel():
            raise ValueError("noise_ssi shorter than the records")
    arr = (_lib.RawboostUtt * n)(*records)
    total = int(sum(r.len for r in records))
    wsb = lib().rdx_rawboost_workspace_bytes(n, max(total, 1))
    ws = torch.empty(max(wsb, 8), device=x_flat.device, dtype=torch.uint8)
    ni = _p(noise_isd) if noise_isd is not None else None
    ns = _p(noise_ssi) if noise_ssi is not None else None
    with _timed("rawboost_batch", x_flat, 8.0 * total):
        check(lib().rdx_rawboost_batch(_p(x_flat), _p(out), arr, n, _p(ws), ni, ns, _stream(x_flat)),
              "rawboost_batch")
    return out


def resample_kernel(orig_freq, new_freq, lowpass_width=6, rolloff=0.99):
    """Host fp32 kernel [new_g, 2*width+orig_g] (torchaudio sinc_interp_hann restatement)."""
    w = ctypes.c_int()
    og = ctypes.c_int()
    ng = ctypes.c_int()
    check(lib().rdx_resample_kernel(orig_freq, new_freq, lowpass_width, rolloff, None, 0, ctypes.byref(w),
                                    ctypes.byref(og), ctypes.byref(ng)), "resample_kernel")
    kw = 2 * w.value + og.value
    buf = (ctypes.c_float * (ng.value * kw))()
    check(lib().rdx_resample_kernel(orig_freq, new_freq, lowpass_width, rolloff, buf, len(buf), ctypes.byref(w),
                                    ctypes.byref(og), ctypes.byref(ng)), "resample_kernel")
    t = torch.tensor(list(buf), dtype=torch.float32).view(ng.value, kw)
    return t, w.value, og.value, ng.value


def resample_batch(x_flat, out_flat, kernels_dev, jobs):
    _require_gpu(x_flat, out_flat, kernels_dev)
    for j in jobs:
        kw = 2 * j.width + j.orig_g
        if (j.in_offset < 0 or j.in_offset + j.in_len > x_flat.numel() or j.out_offset < 0
                or j.out_offset + j.out_len > out_flat.numel() or j.kern_offset + j.new_g * kw > kernels_dev.numel()
                or j.out_len > -(-j.new_g * j.in_len // j.orig_g)):
            raise ValueError("resample job outside its buffers")
    arr = (_lib.ResampleJob * len(jobs))(*jobs)
    check(lib().rdx_resample_batch(_p(x_flat), _p(out_flat), _p(kernels_dev), arr, len(jobs), _stream(x_flat)),
          "resample_batch")


def pad_mixup(sig_flat, offsets, lens, starts, max_len, perm=None, lam=1.0, out=None):
    """[nutt, max_len] batch: crop (len >= max_len, at starts[b]) or tile, then mixup with perm."""
    _require_gpu(sig_flat)
    n = len(offsets)
    for o, L, st in zip(offsets, lens, starts):
        if o < 0 or L <= 0 or o + L > sig_flat.numel():
            raise ValueError(f"pad_mixup: utterance [{o}, +{L}) outside the {sig_flat.numel()}-sample buffer")
        if L >= max_len and (st < 0 or st + max_len > L):
            raise ValueError("pad_mixup: crop start outside the utterance")
    if perm is not None and sorted(perm) != list(range(n)):
        raise ValueError("pad_mixup: perm is not a permutation")
    if out is None:
        out = torch.empty(n, max_len, device=sig_flat.device, dtype=torch.float32)
    assert out.shape == (n, max_len) and out.dtype == torch.float32 and out.is_contiguous()
    I64 = ctypes.c_int64 * n
    pa = (ctypes.c_int * n)(*perm) if perm is not None else None
    check(lib().rdx_pad_mixup(_p(sig_flat), I64(*offsets), I64(*lens), I64(*starts), n, int(max_len), pa, float(lam),
                              _p(out), _stream(sig_flat)), "pad_mixup")
    return out


def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def window_gather(sig_flat, offsets, lens, rec, start, win, out=None):
    """[nwin, win] model inputs cut from packed recordings: window w is recording rec[w] from sample start[w], or the
    whole recording tiled when it is no longer than win (rdx_window_gather; radhip.recordings.window_table makes
    the table). offsets / lens per recording, rec / start per window: host integer sequences."""
    _require_gpu(sig_flat)
    if sig_flat.dtype != torch.float32 or not sig_flat.is_contiguous():
        raise TypeError("window_gather: sig must be a contiguous float32 tensor")
    (offsets, po), (lens, pl), (rec, pr), (start, ps) = _i64(offsets), _i64(lens), _i64(rec), _i64(start)
    nwin, win = rec.size, int(win)
    if offsets.size != lens.size or start.size != nwin:
        raise ValueError("window_gather: offsets / lens and rec / start must pair up")
    if nwin and (rec.min() < 0 or rec.max() >= lens.size):
        raise ValueError("window_gather: rec names a recording outside the table")
    if lens.size and (offsets.min() < 0 or lens.min() <= 0 or (offsets + lens).max() > sig_flat.numel()):
        raise ValueError(f"window_gather: a recording lies outside the {sig_flat.numel()}-sample buffer")
    if out is None:
        out = torch.empty(nwin, win, device=sig_flat.device, dtype=torch.float32)
    if out.shape != (nwin, win) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"window_gather: out must be a contiguous float32 [{nwin}, {win}] device tensor")
    check(lib().rdx_window_gather(_p(sig_flat), po, pl, pr, ps, nwin, win, _p(out), _stream(sig_flat)),
          "window_gather")
    return out


def segment_reduce(scores, seg):
    """(mean, min, max [fp32 n], argmin [int64 n]) of scores[seg[r]:seg[r + 1]] for the n = len(seg) - 1 non-empty
    segments, on the device (rdx_segment_reduce): fixed accumulation order, argmin = the first index inside the
    segment that attains the minimum. seg: host integer prefix offsets."""
    _require_gpu(scores)
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        raise TypeError("segment_reduce: scores must be a contiguous float32 tensor")
    seg, _ = _i64(seg)
    n = seg.size - 1
    if n < 1 or seg[0] < 0 or seg[-1] > scores.numel() or (seg[1:] <= seg[:-1]).any():
        raise ValueError("segment_reduce: seg must be increasing prefix offsets inside scores (no empty segment)")
    seg_dev = torch.from_numpy(seg).to(scores.device)
    f = torch.empty(3, n, device=scores.device, dtype=torch.float32)
    arg = torch.empty(n, device=scores.device, dtype=torch.int64)
    check(lib().rdx_segment_reduce(_p(scores), _p(seg_dev), n, _p(f[0]), _p(f[1]), _p(f[2]), _p(arg),
                                   _stream(scores)), "segment_reduce")
    return f[0], f[1], f[2], arg


def ingest_taps(orig_freq, new_freq=16000, lowpass_width=6, rolloff=0.99):
    """The compact taps of the resampling filter (rdx_ingest_taps, host): (first int32 [new_g], taps float32
    [ntap, new_g] tap-major, width, orig_g, new_g)."""
    nt, w, og, ng = (ctypes.c_int() for _ in range(4))
    refs = [ctypes.byref(v) for v in (nt, w, og, ng)]
    check(lib().rdx_ingest_taps(int(orig_freq), int(new_freq), int(lowpass_width), float(rolloff), None, None, 0,
                                *refs), "ingest_taps")
    first = np.empty(ng.value, dtype=np.int32)
    taps = np.empty((nt.value, ng.value), dtype=np.float32)
    check(lib().rdx_ingest_taps(int(orig_freq), int(new_freq), int(lowpass_width), float(rolloff), first.ctypes.data,
                                taps.ctypes.data, taps.size, *refs), "ingest_taps")
    return first, taps, w.value, og.value, ng.value


def ingest_plan(orig_g, new_g, ntap, channels=1):
    """(outputs per workgroup, LDS bytes, taps staged in LDS) of rdx_ingest_resample for one rate and channel count."""
    ob, lds, in_lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().rdx_ingest_plan(int(orig_g), int(new_g), int(ntap), int(channels), ctypes.byref(ob), ctypes.byref(lds),
                                ctypes.byref(in_lds)), "ingest_plan")
    return ob.value, lds.value, bool(in_lds.value)


def ingest_out_len(frames, orig_freq, new_freq=16000):
    """ceil(new_freq * frames / orig_freq): the length rdx_ingest_resample writes (torchaudio's rule)."""
    return -(-int(new_freq) * int(frames) // int(orig_freq))


class IngestTables:
    """The tap tables of every source rate seen so far, packed in two device buffers (first, taps) that
    rdx_ingest_resample reads. A rate's table is built once, on the host, and uploaded when it is first asked for."""

    def __init__(self, device, new_freq=16000):
        self.device, self.new_freq = torch.device(device), int(new_freq)
        self.rates = {}                 # rate -> (first_offset, taps_offset, ntap, width, orig_g, new_g)
        self._first, self._taps = [], []
        self.first = self.taps = None

    def entry(self, rate):
        rate = int(rate)
        if rate not in self.rates:
            if rate == self.new_freq:
                # no filter (as the oracle's resample returns its input): one tap of 1 at the frame itself, so a
                # multi-channel recording at the target rate is down-mixed only
                first, taps, width, og, ng = np.ones(1, np.int32), np.ones((1, 1), np.float32), 1, 1, 1
            else:
                first, taps, width, og, ng = ingest_taps(rate, self.new_freq)
            self.rates[rate] = (sum(a.size for a in self._first), sum(a.size for a in self._taps), taps.shape[0],
                                width, og, ng)
            self._first.append(first)
            self._taps.append(taps.reshape(-1))
            self.first = torch.from_numpy(np.concatenate(self._first)).to(self.device)
            self.taps = torch.from_numpy(np.concatenate(self._taps)).to(self.device)
        return self.rates[rate]

    def job(self, rate, channels, frames, in_offset, out_offset):
        fo, to, ntap, width, og, ng = self.entry(rate)
        return _lib.IngestJob(int(in_offset), int(frames), int(out_offset), fo, to, int(channels), og, ng, ntap, width,
                              0)


def ingest_resample(in_flat, out_flat, tables, jobs):
    """Down-mix and resample recordings on the device (rdx_ingest_resample): job j reads interleaved float32
    [frames, channels] at in_flat[in_offset:] and writes mono float32 [ingest_out_len] at out_flat[out_offset:].
    jobs: IngestJob records from tables.job(...); any number of them."""
    _require_gpu(in_flat, out_flat)
    for t in (in_flat, out_flat):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("ingest_resample: buffers must be contiguous float32 tensors")
    if not jobs:
        return out_flat
    arr = (_lib.IngestJob * len(jobs))(*jobs)
    check(lib().rdx_ingest_resample(_p(in_flat), in_flat.numel(), _p(out_flat), out_flat.numel(), _p(tables.first),
                                    tables.first.numel(), _p(tables.taps), tables.taps.numel(), arr, len(jobs),
                                    _stream(in_flat)), "ingest_resample")
    return out_flat


# ------------------------------------------------------------------------ silence trimming ----
TRIM_FRAME = 320                          # RDX_TRIM_FRAME
TRIM_MODES = {"ends": 0, "gaps": 1}       # RDX_TRIM_ENDS, RDX_TRIM_GAPS


def _trim_layout(sig_flat, offs, lens, what):
    """The checked host tables of packed recordings: (offs, lens, nframes, foffs) as int64 arrays."""
    _require_gpu(sig_flat)
    if sig_flat.dtype != torch.float32 or not sig_flat.is_contiguous():
        raise TypeError(f"{what}: sig must be a contiguous float32 tensor")
    offs, lens = _i64(offs)[0], _i64(lens)[0]
    if offs.size != lens.size or lens.size == 0:
        raise ValueError(f"{what}: offs and lens must pair up, one recording at least")
    if offs.min() < 0 or lens.min() <= 0 or (offs + lens).max() > sig_flat.numel():
        raise ValueError(f"{what}: a recording lies outside the {sig_flat.numel()}-sample buffer")
    nframes = -(-lens // TRIM_FRAME)
    foffs = np.zeros(lens.size, dtype=np.int64)
    np.cumsum(nframes[:-1], out=foffs[1:])
    return offs, lens, nframes, foffs


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def trim_energy(sig_flat, offs, lens):
    """float32 [sum of ceil(lens / 320)]: the mean square of every 320-sample frame of the packed recordings, the
    frames of recording r after those of r - 1 (rdx_trim_energy)."""
    offs, lens, nframes, foffs = _trim_layout(sig_flat, offs, lens, "trim_energy")
    e = torch.empty(int(nframes.sum()), device=sig_flat.device, dtype=torch.float32)
    check(lib().rdx_trim_energy(_p(sig_flat), _ip(offs), _ip(lens), _ip(foffs), lens.size, _p(e), _stream(sig_flat)),
          "trim_energy")
    return e


def trim_plan(e, lens, mode, db=40.0, pad=10):
    """int64 [frames + R] on the device, from the frame energies of trim_energy: dst, where each frame starts inside
    its trimmed recording (-1: dropped), followed by kept_len, the R trimmed lengths (rdx_trim_plan). One buffer, so
    one copy brings both to the host."""
    _require_gpu(e)
    if mode not in TRIM_MODES:
        raise ValueError(f"trim mode {mode!r} is not one of {sorted(TRIM_MODES)}")
    if not float(db) > 0 or int(pad) < 0 or int(pad) != pad:
        raise ValueError(f"trim: need db > 0 and a whole pad >= 0, got db {db}, pad {pad}")
    lens = _i64(lens)[0]
    nframes = -(-lens // TRIM_FRAME)
    foffs = np.zeros(lens.size, dtype=np.int64)
    np.cumsum(nframes[:-1], out=foffs[1:])
    total = int(nframes.sum())
    if e.dtype != torch.float32 or not e.is_contiguous() or e.numel() != total or lens.size == 0 or lens.min() <= 0:
        raise ValueError(f"trim_plan: e must hold the {total} float32 frame energies of the recordings")
    plan = torch.empty(total + lens.size, device=e.device, dtype=torch.int64)
    scratch = torch.empty(total, device=e.device, dtype=torch.int32)
    ratio = 10.0 ** (-float(db) / 10.0)
    if np.float32(ratio) <= 0:
        raise ValueError(f"trim: 10^(-{db} / 10) is zero in float32")
    check(lib().rdx_trim_plan(_p(e), _ip(foffs), _ip(nframes), _ip(lens), lens.size, ratio, int(pad),
                              TRIM_MODES[mode], _p(scratch), _p(plan), _p(plan[total:]), _stream(e)), "trim_plan")
    return plan


def trim_compact(sig_flat, offs, lens, dst, new_offs, out):
    """Copy the kept frames of every recording to out[new_offs[r] + dst ...] (rdx_trim_compact)."""
    offs, lens, nframes, foffs = _trim_layout(sig_flat, offs, lens, "trim_compact")
    new_offs = _i64(new_offs)[0]
    _require_gpu(dst, out)
    if dst.dtype != torch.int64 or not dst.is_contiguous() or dst.numel() != int(nframes.sum()):
        raise ValueError("trim_compact: dst must be the int64 plan of these recordings")
    if out.dtype != torch.float32 or not out.is_contiguous() or new_offs.size != lens.size or new_offs.min() < 0:
        raise ValueError("trim_compact: out must be a contiguous float32 tensor, new_offs one offset per recording")
    check(lib().rdx_trim_compact(_p(sig_flat), _ip(offs), _ip(lens), _ip(foffs), _p(dst), _ip(new_offs), lens.size,
                                 _p(out), _stream(sig_flat)), "trim_compact")
    return out


def trim_silence(sig_flat, offs, lens, mode, db=40.0, pad=10):
    """Drop the silent frames of packed recordings on the device (the rule: radhip.recordings; csrc/trim.hip).
    Returns (out, new_lens, kept_ids): the trimmed recordings packed in input order in a float32 device tensor,
    their lengths (int64 numpy) and, per recording, the source numbers of its kept frames (int64 numpy). The plan
    (one int64 per frame and one per recording) is the only thing brought to the host, in one copy. When no frame
    of any recording is dropped and the recordings are already packed, out is sig_flat itself."""
    offs, lens, nframes, foffs = _trim_layout(sig_flat, offs, lens, "trim_silence")
    plan = trim_plan(trim_energy(sig_flat, offs, lens), lens, mode, db, pad)
    host = plan.cpu().numpy()
    total = int(nframes.sum())
    new_lens = host[total:].copy()
    ends = foffs + nframes
    kept_ids = [np.nonzero(host[a:b] >= 0)[0] for a, b in zip(foffs, ends)]
    new_offs = np.zeros(lens.size, dtype=np.int64)
    np.cumsum(new_lens[:-1], out=new_offs[1:])
    if (new_lens == lens).all() and (new_offs == offs).all():
        return sig_flat, new_lens, kept_ids
    out = torch.empty(int(new_lens.sum()), device=sig_flat.device, dtype=torch.float32)
    trim_compact(sig_flat, offs, lens, plan[:total], new_offs, out)
    return out, new_lens, kept_ids


# ------------------------------------------------------- locating the spoofed parts ----
def score_track(scores, seg, lens, hop, win):
    """float32 [sum of ceil(lens / 320)] on the device: the per-frame score track of every recording, the frames of
    recording r after those of r - 1 (rdx_track_overlap; the rule: radhip.recordings, track_np). scores: the fp32
    window scores on the device; seg: host integer prefix offsets of the recordings' windows, as segment_reduce takes
    them; lens: the lengths of the scored signals. Every recording must own the windows the window rule gives its
    length."""
    _require_gpu(scores)
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        raise TypeError("score_track: scores must be a contiguous float32 tensor")
    seg, lens = _i64(seg)[0], _i64(lens)[0]
    hop, win = int(hop), int(win)
    if win < 1 or not 1 <= hop <= win:
        raise ValueError(f"score_track: need 1 <= hop <= win, got hop {hop}, win {win}")
    if lens.size == 0 or seg.size != lens.size + 1 or lens.min() <= 0:
        raise ValueError("score_track: one positive length per recording and one more prefix offset than recordings")
    if seg[0] < 0 or seg[-1] > scores.numel():
        raise ValueError(f"score_track: seg reaches outside the {scores.numel()} scores")
    nwin = np.ascontiguousarray(np.diff(seg))
    want = np.where(lens <= win, 1, 1 - (-(lens - win) // hop))
    bad = np.nonzero(nwin != want)[0]
    if bad.size:
        r = int(bad[0])
        raise ValueError(f"score_track: recording {r} of {int(lens[r])} samples owns {int(nwin[r])} windows, the "
                         f"window rule gives {int(want[r])} at hop {hop}")
    nframes = -(-lens // TRIM_FRAME)
    foffs = np.zeros(lens.size, dtype=np.int64)
    np.cumsum(nframes[:-1], out=foffs[1:])
    seg_dev = torch.from_numpy(seg).to(scores.device)
    t = torch.empty(int(nframes.sum()), device=scores.device, dtype=torch.float32)
    check(lib().rdx_track_overlap(_p(scores), _p(seg_dev), _ip(nwin), _ip(lens), _ip(foffs), lens.size, hop, win,
                                  _p(t), _stream(scores)), "track_overlap")
    return t


def track_segments(t, nframes, thr, merge=10, min_frames=25):
    """The flagged segments of packed per-frame tracks (rdx_track_segments, rdx_track_segment_stats; the rule:
    radhip.recordings, segments_np). t: any float32 device tensor that holds the nframes[r] frames of recording r
    after those of r - 1. Returns one (a, b, mean, min, argmin) per recording, host arrays with one entry per
    segment: first and last frame (int64), the fp32 mean and minimum of t[a .. b] and the first frame that attains
    the minimum (int64). Counts, bounds and statistics come back in one copy."""
    _require_gpu(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError("track_segments: t must be a contiguous float32 tensor")
    nframes = _i64(nframes)[0]
    total = int(nframes.sum())
    if nframes.size == 0 or nframes.min() <= 0 or total != t.numel():
        raise ValueError(f"track_segments: nframes must be positive and add up to the {t.numel()} frames of t")
    with np.errstate(over="ignore"):
        if not np.isfinite(np.float32(thr)):
            raise ValueError(f"track_segments: the threshold must be finite in float32, got {thr}")
    if int(merge) != merge or merge < 0 or int(min_frames) != min_frames or min_frames < 1:
        raise ValueError(f"track_segments: need whole merge >= 0 and min_frames >= 1, got {merge}, {min_frames}")
    merge, min_frames = (min(int(v), 2 ** 31 - 1) for v in (merge, min_frames))
    R = nframes.size
    foffs = np.zeros(R, dtype=np.int64)
    np.cumsum(nframes[:-1], out=foffs[1:])
    # one buffer of 32-bit words: count [R], then a, b, argmin (int32) and mean, min (fp32), one slot per frame each
    buf = torch.empty(R + 5 * total, device=t.device, dtype=torch.int32)
    count, a, b, arg = buf[:R], buf[R:R + total], buf[R + total:R + 2 * total], buf[R + 2 * total:R + 3 * total]
    mean, lo = (buf[R + k * total:R + (k + 1) * total].view(torch.float32) for k in (3, 4))
    check(lib().rdx_track_segments(_p(t), _ip(foffs), _ip(nframes), R, float(thr), merge, min_frames, _p(a), _p(b),
                                   _p(count), _stream(t)), "track_segments")
    check(lib().rdx_track_segment_stats(_p(t), _ip(foffs), _ip(nframes), R, _p(a), _p(b), _p(count), _p(mean), _p(lo),
                                        _p(arg), _stream(t)), "track_segment_stats")
    host = buf.cpu().numpy()
    ints = [host[R + k * total:R + (k + 1) * total] for k in range(3)]
    floats = [host[R + k * total:R + (k + 1) * total].view(np.float32) for k in (3, 4)]
    out = []
    for r in range(R):
        sl = slice(int(foffs[r]), int(foffs[r]) + int(host[r]))
        out.append((ints[0][sl].astype(np.int64), ints[1][sl].astype(np.int64), floats[0][sl].copy(),
                    floats[1][sl].copy(), ints[2][sl].astype(np.int64)))
    return out


# -------------------------------------------------------- SincNet residual stack (NHWC) -------
def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _empty_nhwc(shape, like, dtype=None):
    """An uninitialised channels_last [N, C, H, W] tensor on like's device, of like's dtype unless one is given."""
    return torch.empty(shape, device=like.device, dtype=dtype or like.dtype, memory_format=torch.channels_last)


def _f32_rows(*ts):
    return [t.detach().contiguous().float() for t in ts]


def _bnselu_fwd(c, f32):
    """selu(frozen_bn(c + conv_bias)), f32 = (conv_bias, mean, invstd, gamma, beta) fp32 rows."""
    N, C, H, W = c.shape
    y = torch.empty_like(c)
    check(_L(c).rdx_bnselu_fwd(_dtype_code(c), _p(c), *[_p(t) for t in f32], _p(y), N * H * W, C, _stream(c)),
          "bnselu_fwd")
    return y


def _bnselu_bwd(c, dy, f32):
    """_bnselu_fwd's backward: dc and the channel sums [3][C] (d conv_bias, d gamma, d beta; fp32 atomics)."""
    N, C, H, W = c.shape
    dc = torch.empty_like(c)
    sums = torch.zeros(3, C, device=c.device, dtype=torch.float32)
    check(_L(c).rdx_bnselu_bwd(_dtype_code(c), _p(c), _p(dy), *[_p(t) for t in f32], _p(dc), _p(sums), N * H * W, C,
                               _stream(c)), "bnselu_bwd")
    return dc, sums


def _res_tail_fwd(a, idn, bias):
    """y = MaxPool2d((1, 3))(a + idn + bias) and its window index bytes; a, idn NHWC of one dtype, bias fp32 [C]."""
    if idn.shape != a.shape:
        raise ValueError(f"radhip: residual shapes differ {tuple(a.shape)} vs {tuple(idn.shape)}")
    N, C, H, W = a.shape
    y = _empty_nhwc((N, C, H, W // 3), a)
    arg = _empty_nhwc((N, C, H, W // 3), a, torch.uint8)
    check(_L(a).rdx_res_tail_fwd(_dtype_code(a), _p(a), _p(idn), _p(bias), _p(y), _p(arg), N * H, W, C, _stream(a)),
          "res_tail_fwd")
    return y, arg


def _res_tail_bwd(dy, arg, shape):
    """The pool gradient scattered to the full-width `shape` (the gradient of a and of idn) and the bias gradient."""
    N, C, H, W = shape
    ds = _empty_nhwc(shape, dy)
    dbias = torch.zeros(C, device=dy.device, dtype=torch.float32)
    check(_L(dy).rdx_res_tail_bwd(_dtype_code(dy), _p(dy), _p(arg), _p(ds), _p(dbias), N * H, W, C, _stream(dy)),
          "res_tail_bwd")
    return ds, dbias


class BnSelu(torch.autograd.Function):
    """selu(frozen_bn(c + conv_bias)) on an NHWC [N, C, H, W] tensor (conv1 run without its bias)."""

    @staticmethod
    def forward(ctx, c, conv_bias, mean, invstd, weight, bias):
        _require_gpu(c)
        c = _nhwc(c)
        f32 = _f32_rows(conv_bias, mean, invstd, weight, bias)
        ctx.save_for_backward(c, *f32)
        return _bnselu_fwd(c, f32)

    @staticmethod
    def backward(ctx, dy):
        c, *f32 = ctx.saved_tensors
        dc, sums = _bnselu_bwd(c, _nhwc(dy.to(c.dtype)), f32)
        return dc, sums[0], None, None, sums[1], sums[2]


class ResTail(torch.autograd.Function):
    """MaxPool2d((1, 3))(a + identity + bias) on NHWC tensors; the gradient w.r.t. a and identity is
    the same scattered tensor, and bias gets sum(dy) per channel."""

    @staticmethod
    def forward(ctx, a, identity, bias):
        _require_gpu(a, identity)
        a, identity = _nhwc(a), _nhwc(identity.to(a.dtype))
        y, arg = _res_tail_fwd(a, identity, *_f32_rows(bias))
        ctx.save_for_backward(arg)
        ctx.shape, ctx.dtype = tuple(a.shape), a.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        dx, dbias = _res_tail_bwd(_nhwc(dy.to(ctx.dtype)), arg, ctx.shape)
        return dx, dx, dbias


def _b0_prep(x, w1, wd):
    """Block 0's operands as its kernels take them: x in the 16-bit autocast dtype (one channel: [N, H, W] in memory)
    and the 16-bit-rounded weights of conv1 [C][6] and conv_downsample [C][3] in fp32."""
    hd = half_dtype()
    C = w1.shape[0]
    return (x.to(hd).contiguous(), w1.detach().to(hd).float().reshape(C, 6).contiguous(),
            wd.detach().to(hd).float().reshape(C, 3).contiguous())


def _b0_fwd(xb, w1b, wdb, bn5):
    """c = conv1(x), out1 = selu(frozen_bn(c + conv1_bias)) and idn = conv_downsample(x) of block 0 in one pass."""
    N, _, H, W = xb.shape
    C = w1b.shape[0]
    c = _empty_nhwc((N, C, H + 1, W), xb)
    out1 = torch.empty_like(c)
    idn = _empty_nhwc((N, C, H, W), xb)
    with _timed("sincnet_b0_fwd", xb, 2.0 * (xb.numel() + 2 * c.numel() + idn.numel())):
        check(_L(xb).rdx_sincnet_b0_fwd(_p(xb), _p(w1b), _p(wdb), _p(bn5), _p(c), _p(out1), _p(idn), N, H, W, C,
                                       _stream(xb)), "sincnet_b0_fwd")
    return c, out1, idn


def _b0_bwd(xb, dc, di, w1b, wdb, shapes):
    """Both block-0 convolutions' backward in one pass: dx [N, 1, H, W] fp32 and the weight gradients in the
    shapes (conv1.weight's, conv_downsample.weight's)."""
    N, _, H, W = xb.shape
    C = shapes[0][0]
    dx = torch.empty(N, 1, H, W, device=xb.device, dtype=torch.float32)
    part = torch.empty(lib().rdx_sincnet_b0_nblk(N * H * W), C * 9, device=xb.device, dtype=torch.float32)
    with _timed("sincnet_b0_bwd", dc, 2 * (dc.numel() + di.numel()) + 4 * dx.numel() + 2 * xb.numel()):
        check(_L(xb).rdx_sincnet_b0_bwd(_p(xb), _p(dc), _p(di), _p(w1b), _p(wdb), _p(dx), _p(part), N, H, W, C,
                                       _stream(dc)), "sincnet_b0_bwd")
    dw = part.sum(0).view(C, 9)
    return dx, dw[:, :6].reshape(shapes[0]), dw[:, 6:].reshape(shapes[1])


class Block0Convs(torch.autograd.Function):
    """conv1 (2x3, padding (1, 1)) and conv_downsample (1x3, padding (0, 1)) of SincNet block 0, whose input
    has ONE channel (Residual_block.forward, src/models/DualStreamSEMamba.py:182-200): forward on MIOpen in
    bf16 (as autocast runs them), backward (dx, d conv1.weight, d conv_downsample.weight) in one HIP pass
    (rdx_sincnet_b0_bwd) instead of two single-output-channel backward-data and two weight-gradient
    convolutions."""

    @staticmethod
    def forward(ctx, x, w1, wd):
        _require_gpu(x)
        hd = half_dtype()
        xb = x.to(hd)
        w1b, wdb = w1.to(hd), wd.to(hd)
        c = torch.nn.functional.conv2d(xb, w1b, None, 1, (1, 1))
        idn = torch.nn.functional.conv2d(xb, wdb, None, 1, (0, 1))
        ctx.save_for_backward(xb, w1b, wdb)
        ctx.meta = (w1.shape, wd.shape, x.dtype)
        return c, idn

    @staticmethod
    def backward(ctx, dc, di):
        xb, w1b, wdb = ctx.saved_tensors
        w1_shape, wd_shape, x_dtype = ctx.meta
        dc = _nhwc(dc.to(xb.dtype))
        di = _nhwc(di.to(xb.dtype))
        xc = xb.contiguous(memory_format=torch.channels_last)      # one channel: [N, H, W] in memory
        # the 16-bit weights the forward used
        dx, dw1, dwd = _b0_bwd(xc, dc, di, w1b.float().contiguous(), wdb.float().contiguous(), (w1_shape, wd_shape))
        return dx.to(x_dtype), dw1, dwd


# ------------------------------------------------------------- SincNet residual convolutions ----
SCONV_CH = (32, 64)


def sconv_enabled():
    """RADHIP_SCONV=0: no convolution runs on csrc/sconv.hip."""
    return os.environ.get("RADHIP_SCONV", "1") != "0"


def sconv_weight_ok(weight):
    """The kernels csrc/sconv.hip has: C_in and C_out in {32, 64}, kernel (1|2) x 3 (RADHIP_SCONV=0: none)."""
    co, ci, kh, kw = weight.shape
    return ci in SCONV_CH and co in SCONV_CH and kh in (1, 2) and kw == 3 and sconv_enabled()


def sconv_ok(x, weight):
    """The shapes csrc/sconv.hip covers: bf16-autocast NHWC input on the GPU and a sconv_weight_ok kernel."""
    return x.is_cuda and x.dim() == 4 and x.shape[1] == weight.shape[1] and sconv_weight_ok(weight)


# Per-window cache of the SincNet convolution weight layouts (radhip/window.py sets it to a dict for the span
# of one accumulation window, in which the parameters do not change): the clean pass prepares them, the
# adversarial passes reuse them. Under HIP graphs the clean pass's graph rewrites the cached tensors on every
# replay and the adversarial graphs read them.
SCONV_WCACHE = None


def _sconv_w(weight, hd):
    if SCONV_WCACHE is not None:
        hit = SCONV_WCACHE.get((id(weight), hd))
        if hit is not None and hit[0] is weight:
            return hit[1], hit[2]
    wf, wd = _sconv_w_prep(weight, hd)
    if SCONV_WCACHE is not None:
        SCONV_WCACHE[(id(weight), hd)] = (weight, wf, wd)
    return wf, wd


def _sconv_w_prep(weight, hd):
    """[C_out, C_in, KH, 3] -> tap-major [KH*3][C_out][C_in] in the 16-bit dtype hd (forward) and the flipped,
    transposed [KH*3][C_in][C_out] (input gradient = the same convolution of dY)."""
    co, ci, kh, kw = weight.shape
    wb = weight.detach().to(hd)
    wf = wb.permute(2, 3, 0, 1).reshape(kh * kw, co, ci).contiguous()
    wd = wb.flip(2, 3).permute(2, 3, 1, 0).reshape(kh * kw, ci, co).contiguous()
    return wf, wd


def sconv_prep_many(weights, hd):
    """Fill SCONV_WCACHE with both 16-bit layouts of every weight (sconv_weight_ok, fp32 contiguous, on the GPU) in
    one launch per 32 weights (rdx_sconv_wprep_many): the window's SincNet stack prepared at once instead of four
    torch launches per weight on first use (_sconv_w_prep's layouts). `weights` are the parameters themselves (the
    cache is keyed by them); only their data is read."""
    cache = SCONV_WCACHE
    ws = [w for w in weights if w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and sconv_weight_ok(w)]
    if cache is None or not ws:
        return
    for i in range(0, len(ws), 32):
        g = ws[i:i + 32]
        wf, wd = [], []
        for w in g:
            co, ci, kh, kw = w.shape
            wf.append(torch.empty(kh * kw, co, ci, device=w.device, dtype=hd))
            wd.append(torch.empty(kh * kw, ci, co, device=w.device, dtype=hd))
        n = len(g)
        ints = lambda vals: (ctypes.c_int * n)(*vals)
        check(_L(hd).rdx_sconv_wprep_many(n, ptr_array([w.data_ptr() for w in g]), ptr_array([t.data_ptr() for t in wf]),
                                          ptr_array([t.data_ptr() for t in wd]), ints([w.shape[0] for w in g]),
                                          ints([w.shape[1] for w in g]), ints([w.shape[2] for w in g]),
                                          _stream(g[0])), "sconv_wprep_many")
        for w, a, b in zip(g, wf, wd):
            cache[(id(w), hd)] = (w, a, b)


def _sconv_run(x, w_tap, ci, co, kh, ph, y2=None, bn=None, res=None):
    """x: 16-bit NHWC (bf16 or fp16: the output's dtype and the library); res: an [N, co, Ho, W] channels_last
    tensor of x's dtype added in the epilogue (y = r(r(conv) + res), r = rounding to that dtype)."""
    N, _, H, W = x.shape
    Ho = H + 2 * ph - kh + 1
    y = _empty_nhwc((N, co, Ho, W), x)
    # algorithmic HBM bytes (the convolution is HBM-bound: ~100 FLOP per byte at these channel counts)
    nbytes = 2.0 * (N * H * W * ci + N * Ho * W * co * (2 if (y2 is not None or res is not None) else 1))
    with _timed("sconv_fwd", x, nbytes, shape=(N, H, W, ci, co, kh, ph)):
        if res is not None:
            if res.shape != y.shape or res.dtype != y.dtype or not res.is_contiguous(memory_format=torch.channels_last):
                raise ValueError("radhip sconv: residual must be NHWC of the output's shape and dtype")
            check(_L(x).rdx_sconv_fwd_res(_p(x), _p(w_tap), _p(y), _p(res), N, H, W, ci, co, kh, ph, _stream(x)),
                  "sconv_fwd_res")
        else:
            check(_L(x).rdx_sconv_fwd(_p(x), _p(w_tap), _p(y), _p(y2) if y2 is not None else None,
                                      _p(bn) if bn is not None else None, N, H, W, ci, co, kh, ph, _stream(x)),
                  "sconv_fwd")
    return y


SCONV_POOL_DEFAULT = "1"


def sconv_pool_ok(w2_shape, W, half):
    """conv2 shapes whose residual tail runs without the full-width tensors (half "fwd": rdx_sconv_fwd_pool; "bwd":
    the pooled-gradient backward kernels): 2 x 3, C_in = C_out in {32, 64}, at least one pool window.
    RADHIP_SCONV_POOL=1 both halves, fwd / bwd that half only, 0 none (the convolution, then rdx_res_tail_fwd /
    rdx_res_tail_bwd around the full-width tensors)."""
    co, ci, kh, kw = w2_shape
    return (ci == co and ci in SCONV_CH and kh == 2 and kw == 3 and W >= 3
            and os.environ.get("RADHIP_SCONV_POOL", SCONV_POOL_DEFAULT) in ("1", half))


def _sconv_run_pool(x, w_tap, idn, bias, c):
    """MaxPool2d((1, 3))(conv2(x) + idn + bias) and its window index bytes in one launch (kernel 2 x 3, no row padding,
    c -> c channels); x, idn: 16-bit NHWC, bias fp32 [c]."""
    N, _, H, W = x.shape
    Ho = H - 1
    if idn.shape != (N, c, Ho, W) or idn.dtype != x.dtype or not idn.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("radhip sconv: identity must be NHWC of the convolution output's shape and dtype")
    y = _empty_nhwc((N, c, Ho, W // 3), x)
    arg = _empty_nhwc((N, c, Ho, W // 3), x, torch.uint8)
    # x and the identity in, a third of a full-width output (+ one index byte per element) out
    nbytes = 2.0 * (N * H * W * c + N * Ho * W * c) + 3.0 * y.numel()
    with _timed("sconv_fwd", x, nbytes, shape=(N, H, W, c, c, 2, 0)):
        check(_L(x).rdx_sconv_fwd_pool(_p(x), _p(w_tap), _p(idn), _p(bias), _p(y), _p(arg), N, H, W, c, c, _stream(x)),
              "sconv_fwd_pool")
    return y, arg


def _sconv_run_res_pool(x, w_tap, dp, arg, dbias, ci, co, kh, ph):
    """_sconv_run with the residual given as the pooled gradient (dp, arg) of width W // 3; dbias [co] fp32 (zeroed)
    receives dp's per-channel sum."""
    N, _, H, W = x.shape
    Ho = H + 2 * ph - kh + 1
    y = _empty_nhwc((N, co, Ho, W), x)
    nbytes = 2.0 * (N * H * W * ci + N * Ho * W * co) + 3.0 * dp.numel()
    with _timed("sconv_fwd", x, nbytes, shape=(N, H, W, ci, co, kh, ph)):
        check(_L(x).rdx_sconv_fwd_res_pool(_p(x), _p(w_tap), _p(y), _p(dp), _p(arg), _p(dbias), N, H, W, ci, co, kh, ph,
                                           _stream(x)), "sconv_fwd_res_pool")
    return y


def _sconv_wgrad_pool(x, dp, arg, weight_shape):
    """The weight gradient of conv2 or of block 2's conv_downsample (no row padding) from the pooled gradient (dp, arg)
    of its output."""
    co, ci, kh, kw = weight_shape
    N, _, H, W = x.shape
    Ho = dp.shape[2]
    nblk = lib().rdx_sconv_wgrad_nblk(N, Ho, W)
    part = torch.empty(nblk, kh * 3 * co * ci, device=x.device, dtype=torch.float32)
    dw = torch.empty(kh * 3, co, ci, device=x.device, dtype=torch.float32)
    with _timed("sconv_wgrad", x, 2.0 * N * H * W * ci + 3.0 * dp.numel(), shape=(N, H, W, ci, co, kh, 0)):
        check(_L(x).rdx_sconv_wgrad_pool(_p(x), _p(dp), _p(arg), _p(dw), _p(part), N, H, W, ci, co, kh, 0, _stream(x)),
              "sconv_wgrad_pool")
    return dw.view(kh, 3, co, ci).permute(2, 3, 0, 1)


def _sconv_dgrad_pool(dp, arg, wd, weight_shape, W):
    """The input gradient [N, ci, H, W] of block 2's conv_downsample (weight_shape (64, 32, 1, 3), no row padding) from the
    pooled gradient (dp, arg) [N, 64, H, W // 3] of its output; wd: the flipped kernel [3][ci][co]."""
    co, ci, kh, kw = weight_shape
    N, _, H, _ = dp.shape
    dx = _empty_nhwc((N, ci, H, W), dp)
    with _timed("sconv_fwd", dp, 3.0 * dp.numel() + 2.0 * dx.numel(), shape=(N, H, W, co, ci, kh, 0)):
        check(_L(dp).rdx_sconv_dgrad_pool(_p(dp), _p(arg), _p(wd), _p(dx), N, H, W, co, ci, kh, 0, _stream(dp)),
              "sconv_dgrad_pool")
    return dx


def _pooled_grad_ok(dy, arg):
    """A pool gradient the pooled-gradient kernels take as it is: the argmax tensor's shape, 16-byte aligned."""
    return dy.shape == arg.shape and dy.data_ptr() % 16 == 0


def _sconv_backward(x, dy, wd, weight_shape, ph, need_dx):
    co, ci, kh, kw = weight_shape
    N, _, H, W = x.shape
    Ho = dy.shape[2]
    dx = _sconv_run(dy, wd, co, ci, kh, kh - 1 - ph) if need_dx else None
    nblk = lib().rdx_sconv_wgrad_nblk(N, Ho, W)
    part = torch.empty(nblk, kh * 3 * co * ci, device=x.device, dtype=torch.float32)
    dw = torch.empty(kh * 3, co, ci, device=x.device, dtype=torch.float32)
    with _timed("sconv_wgrad", x, 2.0 * (N * H * W * ci + N * Ho * W * co), shape=(N, H, W, ci, co, kh, ph)):
        check(_L(x).rdx_sconv_wgrad(_p(x), _p(dy), _p(dw), _p(part), N, H, W, ci, co, kh, ph, _stream(x)), "sconv_wgrad")
    return dx, dw.view(kh, 3, co, ci).permute(2, 3, 0, 1)


class SConv(torch.autograd.Function):
    """conv2d(x, weight, padding=(ph, 1)) of the SincNet residual stack, NHWC bf16, no bias (csrc/sconv.hip):
    the input gradient runs the same MFMA kernel on dY with the flipped kernel, the weight gradient the
    transposed-operand kernel (per-workgroup partials, fixed-order reduction)."""

    @staticmethod
    def forward(ctx, x, weight, ph):
        _require_gpu(x)
        x = _nhwc(x.to(half_dtype()))
        co, ci, kh, _ = weight.shape
        wf, wd = _sconv_w(weight, x.dtype)
        ctx.save_for_backward(x, wd)
        ctx.meta = (tuple(weight.shape), ph, weight.dtype)
        return _sconv_run(x, wf, ci, co, kh, ph)

    @staticmethod
    def backward(ctx, dy):
        x, wd = ctx.saved_tensors
        shape, ph, wdt = ctx.meta
        dy = _nhwc(dy.to(x.dtype))
        dx, dw = _sconv_backward(x, dy, wd, shape, ph, ctx.needs_input_grad[0])
        return dx, dw.to(wdt), None


class SConvBnSelu(torch.autograd.Function):
    """selu(frozen_bn(conv2d(x, weight, padding=(ph, 1)) + conv_bias)) in one forward launch (conv1 -> bn2 ->
    selu of Residual_block; BnSelu's arithmetic in the conv epilogue). Backward: rdx_bnselu_bwd on the saved
    conv output (d conv_bias, d gamma, d beta and dc), then the SConv gradients of dc."""

    @staticmethod
    def forward(ctx, x, weight, ph, conv_bias, mean, invstd, gamma, beta):
        _require_gpu(x)
        x = _nhwc(x.to(half_dtype()))
        co, ci, kh, _ = weight.shape
        wf, wd = _sconv_w(weight, x.dtype)
        f32 = _f32_rows(conv_bias, mean, invstd, gamma, beta)
        bn = torch.stack([f32[0], f32[1], f32[2] * f32[3], f32[4]]).contiguous()
        N, _, H, W = x.shape
        y = _empty_nhwc((N, co, H + 2 * ph - kh + 1, W), x)
        c = _sconv_run(x, wf, ci, co, kh, ph, y2=y, bn=bn)
        ctx.save_for_backward(x, wd, c, *f32)
        ctx.meta = (tuple(weight.shape), ph, weight.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wd, c, *f32 = ctx.saved_tensors
        shape, ph, wdt = ctx.meta
        dc, sums = _bnselu_bwd(c, _nhwc(dy.to(c.dtype)), f32)
        dx, dw = _sconv_backward(x, dc, wd, shape, ph, ctx.needs_input_grad[0])
        return dx, dw.to(wdt), None, sums[0], None, None, sums[1], sums[2]


def _fused_dgrad_bn_ok(w2_shape):
    co2, ci2, kh2, _ = w2_shape
    return ci2 == co2 and ci2 in (32, 64) and kh2 == 2 and os.environ.get("RADHIP_FUSED_DGRAD_BN", "1") != "0"


def _conv2_grad_to_c(da, out1, c, wd2, w2_shape, bn5, f32, arg=None):
    """From conv2's output gradient da back to conv1's pre-activation c: dc (bf16, c's shape), the frozen
    BN / conv1-bias sums [3][C] (d conv_bias, d gamma, d beta) and dw2. The 32- and 64-channel blocks run conv2's
    input gradient and the BN + SELU backward as ONE kernel (rdx_sconv_dgrad_bnselu: dO1 stays on chip);
    otherwise the input gradient and rdx_bnselu_bwd run one after the other. With arg, (da, arg) is the pooled
    gradient of the block's max-pool (width W // 3: sconv_pool_ok and _fused_dgrad_bn_ok shapes only) and both
    kernels expand it while they stage it."""
    co2, ci2, kh2, _ = w2_shape
    N, C, Ho, W = c.shape
    H = da.shape[2]
    if arg is None and not _fused_dgrad_bn_ok(w2_shape):
        dc, sums = _bnselu_bwd(c, _sconv_run(da, wd2, co2, ci2, kh2, kh2 - 1), f32)
        return dc, sums, _sconv_backward(out1, da, wd2, w2_shape, 0, False)[1]
    dc = torch.empty_like(c)
    sums = torch.zeros(3, C, device=c.device, dtype=torch.float32)
    if arg is not None:
        nbytes = 3.0 * da.numel() + 2.0 * (2 * N * Ho * W * C)
        with _timed("sconv_dgrad_bnselu", da, nbytes, shape=(N, H, W)):
            check(_L(da).rdx_sconv_dgrad_bnselu_pool(_p(da), _p(arg), _p(wd2), _p(c), _p(dc), _p(bn5), _p(sums), N, H, W,
                                                    co2, ci2, kh2, kh2 - 1, _stream(da)), "sconv_dgrad_bnselu_pool")
        return dc, sums, _sconv_wgrad_pool(out1, da, arg, w2_shape)
    nbytes = 2.0 * (N * H * W * co2 + 2 * N * Ho * W * C)
    with _timed("sconv_dgrad_bnselu", da, nbytes, shape=(N, H, W)):
        check(_L(da).rdx_sconv_dgrad_bnselu(_p(da), _p(wd2), _p(c), _p(dc), _p(bn5), _p(sums), N, H, W, co2, ci2,
                                           kh2, kh2 - 1, _stream(da)), "sconv_dgrad_bnselu")
    _, dw2 = _sconv_backward(out1, da, wd2, w2_shape, 0, False)
    return dc, sums, dw2


def _frozen_invstd(bn):
    """rsqrt(running_var + eps) of a frozen BatchNorm, once per accumulation window (SCONV_WCACHE)."""
    cache = SCONV_WCACHE
    if cache is None:
        return torch.rsqrt(bn.running_var + bn.eps)
    key = ("invstd", id(bn.running_var))
    hit = cache.get(key)
    if hit is not None and hit[0] is bn.running_var:
        return hit[1]
    v = torch.rsqrt(bn.running_var + bn.eps)
    cache[key] = (bn.running_var, v)
    return v


def _bn_rows(conv_bias, mean, invstd, gamma, beta):
    """The frozen-BN record rows [conv bias | mean | invstd * gamma | beta | invstd] of a block; within an
    accumulation window (ops.SCONV_WCACHE set) made once and shared by the window's passes (the parameters and
    running statistics do not change inside a window)."""
    src = (conv_bias, mean, invstd, gamma, beta)
    cache = SCONV_WCACHE
    key = ("bn5",) + tuple(id(t) for t in src)
    if cache is not None:
        hit = cache.get(key)
        if hit is not None and all(a is b for a, b in zip(hit[0], src)):
            return hit[1], hit[2]
    f32 = [t.detach().contiguous().float() for t in src]
    bn5 = torch.stack([f32[0], f32[1], f32[2] * f32[3], f32[4], f32[2]]).contiguous()
    if cache is not None:
        cache[key] = (src, f32, bn5)
    return f32, bn5


class SConvBnSeluSConv(torch.autograd.Function):
    """conv2(selu(frozen_bn(conv1(x) + conv1_bias))) of Residual_block (no conv2 bias: ResTail adds it):
    conv1 with the BN + SELU epilogue and conv2 on csrc/sconv.hip; the backward goes from conv2's output
    gradient to conv1's pre-activation in one pass where the channels allow (_conv2_grad_to_c)."""

    @staticmethod
    def forward(ctx, x, w1, ph1, conv_bias, mean, invstd, gamma, beta, w2):
        _require_gpu(x)
        x = _nhwc(x.to(half_dtype()))
        co, ci, kh, _ = w1.shape
        wf1, wd1 = _sconv_w(w1, x.dtype)
        wf2, wd2 = _sconv_w(w2, x.dtype)
        f32, bn5 = _bn_rows(conv_bias, mean, invstd, gamma, beta)
        N, _, H, W = x.shape
        out1 = _empty_nhwc((N, co, H + 2 * ph1 - kh + 1, W), x)
        c = _sconv_run(x, wf1, ci, co, kh, ph1, y2=out1, bn=bn5[:4])
        co2, ci2, kh2, _ = w2.shape
        a = _sconv_run(out1, wf2, ci2, co2, kh2, 0)
        ctx.save_for_backward(x, wd1, c, out1, wd2, bn5, *f32)
        ctx.meta = (tuple(w1.shape), ph1, w1.dtype, tuple(w2.shape), w2.dtype)
        return a

    @staticmethod
    def backward(ctx, da):
        x, wd1, c, out1, wd2, bn5, *f32 = ctx.saved_tensors
        s1, ph1, w1dt, s2, w2dt = ctx.meta
        da = _nhwc(da.to(x.dtype))
        dc, sums, dw2 = _conv2_grad_to_c(da, out1, c, wd2, s2, bn5, f32)
        dx, dw1 = _sconv_backward(x, dc, wd1, s1, ph1, ctx.needs_input_grad[0])
        return dx, dw1.to(w1dt), None, sums[0], None, None, sums[1], sums[2], dw2.to(w2dt)


class ResBlock(torch.autograd.Function):
    """A residual block past block 0 as one autograd op (Residual_block.forward,
    src/models/DualStreamSEMamba.py:182-200, frozen BN): MaxPool2d((1, 3))(conv2(selu(bn2(conv1(x) + cb))) + idn + bias).
    wdn None (SincNet blocks 1, 3-5): idn is the block input x and bias conv2's; with wdn (block 2, 32 -> 64 channels)
    idn = conv_downsample(x) on csrc/sconv.hip and bias the sum of both convolutions' biases.
    Forward: conv1 with the BN + SELU epilogue, conv_downsample, then conv2 with the residual sum and the pool in its
    epilogue (sconv_pool_ok "fwd": no full-width conv2 output, no tail launch; otherwise conv2 and rdx_res_tail_fwd).
    Backward: the pool gradient stays (dy, argmax byte) for the kernels that consume it (sconv_pool_ok "bwd";
    otherwise rdx_res_tail_bwd's full-width scatter feeds the plain kernels), conv2's input gradient runs with the
    BN + SELU backward, and the block input's gradient is ONE pass, conv1's input gradient with the identity branch's
    added in its epilogue (rdx_sconv_fwd_res; pooled and without wdn rdx_sconv_fwd_res_pool, which also sums the bias
    gradient): the bits autograd's separate add of the two full-size gradients produces, without that
    read-read-write pass. The same bits as SConvBnSeluSConv (+ SConv) + ResTail; with wdn the pooled bias gradient is
    a reduction over the pooled tensor."""

    @staticmethod
    def forward(ctx, x, w1, conv_bias, mean, invstd, gamma, beta, w2, bias, wdn):
        _require_gpu(x)
        x_dtype = x.dtype
        x = _nhwc(x.to(half_dtype()))
        co, ci, kh, _ = w1.shape
        wf1, wd1 = _sconv_w(w1, x.dtype)
        wf2, wd2 = _sconv_w(w2, x.dtype)
        wfd, wdd = _sconv_w(wdn, x.dtype) if wdn is not None else (None, None)
        f32, bn5 = _bn_rows(conv_bias, mean, invstd, gamma, beta)
        N, _, H, W = x.shape
        out1 = _empty_nhwc((N, co, H + 1, W), x)
        c = _sconv_run(x, wf1, ci, co, kh, 1, y2=out1, bn=bn5[:4])
        co2, ci2, kh2, _ = w2.shape
        idn = x if wdn is None else _sconv_run(x, wfd, ci, wdn.shape[0], wdn.shape[2], 0)
        bf = bias.detach().contiguous().float()
        if sconv_pool_ok(w2.shape, W, "fwd") and (N, co2, H + 2 - kh2, W) == tuple(idn.shape):
            # conv2 with the residual sum and the max-pool in its epilogue: its full-width output is never stored
            y, arg = _sconv_run_pool(out1, wf2, idn, bf, co2)
        else:
            y, arg = _res_tail_fwd(_sconv_run(out1, wf2, ci2, co2, kh2, 0), idn, bf)
        ctx.save_for_backward(x, wd1, c, out1, wd2, wdd, bn5, arg, *f32)
        ctx.meta = (tuple(w1.shape), w1.dtype, tuple(w2.shape), w2.dtype,
                    None if wdn is None else (tuple(wdn.shape), wdn.dtype), x_dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wd1, c, out1, wd2, wdd, bn5, arg, *f32 = ctx.saved_tensors
        s1, w1dt, s2, w2dt, down, x_dtype = ctx.meta
        N, _, H, W = x.shape
        C = s2[0]
        dy = _nhwc(dy.to(x.dtype))
        co, ci, kh, _ = s1
        need_dx = ctx.needs_input_grad[0]
        pooled = sconv_pool_ok(s2, W, "bwd") and _fused_dgrad_bn_ok(s2) and _pooled_grad_ok(dy, arg)
        dx = dwd = None
        if down is None and pooled and need_dx and co == ci and kh == 2:
            # the pool gradient stays pooled: its three consumers expand (dy, arg) while they stage it, and the
            # bias gradient (the sum of dy) comes out of the block input gradient's epilogue
            dbias = torch.zeros(C, device=dy.device, dtype=torch.float32)
            dc, sums, dw2 = _conv2_grad_to_c(dy, out1, c, wd2, s2, bn5, f32, arg=arg)
            dx = _sconv_run_res_pool(dc, wd1, dy, arg, dbias, co, ci, kh, kh - 1 - 1)
        elif down is not None and pooled and down[0] == (64, 32, 1, 3):
            dbias = dy.sum((0, 2, 3), dtype=torch.float32)
            dc, sums, dw2 = _conv2_grad_to_c(dy, out1, c, wd2, s2, bn5, f32, arg=arg)
            res = _sconv_dgrad_pool(dy, arg, wdd, down[0], W) if need_dx else None
            dwd = _sconv_wgrad_pool(x, dy, arg, down[0])
        else:
            ds, dbias = _res_tail_bwd(dy, arg, (N, C, H, W))
            dc, sums, dw2 = _conv2_grad_to_c(ds, out1, c, wd2, s2, bn5, f32)
            res, dwd = (ds, None) if down is None else _sconv_backward(x, ds, wdd, down[0], 0, need_dx)
        if dx is None and need_dx:
            # conv1's input gradient + the identity branch's
            dx = _sconv_run(dc, wd1, co, ci, kh, kh - 1 - 1, res=res)
        _, dw1 = _sconv_backward(x, dc, wd1, s1, 1, False)
        return (dx.to(x_dtype) if dx is not None else None, dw1.to(w1dt), sums[0], None, None, sums[1], sums[2],
                dw2.to(w2dt), dbias, dwd.to(down[1]) if down is not None else None)


class BnSeluSConv(torch.autograd.Function):
    """conv2(selu(frozen_bn(c + conv1_bias))) for block 0, whose conv1 runs in Block0Convs: BnSelu's forward,
    conv2 on csrc/sconv.hip, and the fused backward of _conv2_grad_to_c."""

    @staticmethod
    def forward(ctx, c, conv_bias, mean, invstd, gamma, beta, w2):
        _require_gpu(c)
        c = _nhwc(c.to(half_dtype()))
        f32, bn5 = _bn_rows(conv_bias, mean, invstd, gamma, beta)
        out1 = _bnselu_fwd(c, f32)
        wf2, wd2 = _sconv_w(w2, c.dtype)
        co2, ci2, kh2, _ = w2.shape
        a = _sconv_run(out1, wf2, ci2, co2, kh2, 0)
        ctx.save_for_backward(c, out1, wd2, bn5, *f32)
        ctx.meta = (tuple(w2.shape), w2.dtype)
        return a

    @staticmethod
    def backward(ctx, da):
        c, out1, wd2, bn5, *f32 = ctx.saved_tensors
        s2, w2dt = ctx.meta
        da = _nhwc(da.to(c.dtype))
        dc, sums, dw2 = _conv2_grad_to_c(da, out1, c, wd2, s2, bn5, f32)
        return dc, sums[0], None, None, sums[1], sums[2], dw2.to(w2dt)


class Block0Front(torch.autograd.Function):
    """SincNet block 0 up to conv2 (Residual_block.forward, src/models/DualStreamSEMamba.py:182-200, one input
    channel): c = conv1(x), idn = conv_downsample(x), out1 = selu(frozen_bn(c + conv1_bias)) in ONE HIP pass
    (rdx_sincnet_b0_fwd), then a = conv2(out1) on csrc/sconv.hip. Backward: conv2's input gradient with the
    BN + SELU backward (_conv2_grad_to_c), then both convolutions' backward in one pass (rdx_sincnet_b0_bwd).
    Returns (a, idn); the biases of conv2 / conv_downsample are added by ResTail."""

    @staticmethod
    def forward(ctx, x, w1, wd, conv_bias, mean, invstd, gamma, beta, w2):
        _require_gpu(x)
        xb, w1b, wdb = _b0_prep(x, w1, wd)
        f32, bn5 = _bn_rows(conv_bias, mean, invstd, gamma, beta)
        c, out1, idn = _b0_fwd(xb, w1b, wdb, bn5)
        wf2, wd2 = _sconv_w(w2, xb.dtype)
        co2, ci2, kh2, _ = w2.shape
        a = _sconv_run(out1, wf2, ci2, co2, kh2, 0)
        ctx.save_for_backward(xb, w1b, wdb, c, out1, wd2, bn5, *f32)
        ctx.meta = (tuple(w1.shape), tuple(wd.shape), x.dtype, tuple(w2.shape), w2.dtype)
        return a, idn

    @staticmethod
    def backward(ctx, da, di):
        xb, w1b, wdb, c, out1, wd2, bn5, *f32 = ctx.saved_tensors
        w1_shape, wd_shape, x_dtype, s2, w2dt = ctx.meta
        N, H, W = xb.shape[0], xb.shape[2], xb.shape[3]
        da = _nhwc(da.to(xb.dtype))
        dc, sums, dw2 = _conv2_grad_to_c(da, out1, c, wd2, s2, bn5, f32)
        di = (_nhwc(di.to(xb.dtype)) if di is not None
              else torch.zeros(N, w1_shape[0], H, W, device=xb.device, dtype=xb.dtype, memory_format=torch.channels_last))
        dx, dw1, dwd = _b0_bwd(xb, dc, di, w1b, wdb, (w1_shape, wd_shape))
        return dx.to(x_dtype), dw1, dwd, sums[0], None, None, sums[1], sums[2], dw2.to(w2dt)


class Block0Fused(torch.autograd.Function):
    """SincNet block 0 whole (Residual_block.forward, src/models/DualStreamSEMamba.py:182-200, one input channel,
    frozen BN): y = MaxPool2d((1, 3))(conv2(selu(bn2(conv1(x) + cb))) + conv_downsample(x) + b2 + bd) in ONE HIP
    pass (rdx_b0x_fwd: only x is read, only y and the window argmax are written; bit-identical to Block0Front +
    ResTail). Backward in one pass too (rdx_b0x_bwd: c and out1 recomputed from x, per-workgroup partial rows of
    every parameter gradient); RADHIP_B0X_BWD=0 runs the unfused backward kernels on recomputed intermediates
    instead (c / out1 by rdx_sincnet_b0_fwd, the pool gradient scattered by the argmax, Block0Front's kernels)."""

    @staticmethod
    def forward(ctx, x, w1, wd, conv_bias, mean, invstd, gamma, beta, w2, b2, bd):
        _require_gpu(x)
        xb, w1b, wdb = _b0_prep(x, w1, wd)
        hd = xb.dtype
        N, _, H, W = xb.shape
        C = w1.shape[0]
        f32, bn5 = _bn_rows(conv_bias, mean, invstd, gamma, beta)
        wf2, wd2 = _sconv_w(w2, hd)
        bias = (b2.detach().float() + bd.detach().float()).contiguous()
        y = _empty_nhwc((N, C, H, W // 3), xb)
        arg = _empty_nhwc((N, C, H, W // 3), xb, torch.uint8)
        # MFMA work: conv2 (32 -> 32, 2 x 3) over N x H x W positions; HBM: x in, y + argmax out
        with _timed("b0x_fwd", x, 2.0 * N * H * W * 32 * 192):
            check(_L(hd).rdx_b0x_fwd(_p(xb), _p(w1b), _p(wdb), _p(bn5), _p(wf2), _p(bias), _p(y), _p(arg), N, H, W,
                                    _stream(x)), "b0x_fwd")
        ctx.save_for_backward(xb, w1b, wdb, wd2, bn5, arg, *f32)
        ctx.meta = (tuple(w1.shape), tuple(wd.shape), x.dtype, tuple(w2.shape), w2.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, w1b, wdb, wd2, bn5, arg, *f32 = ctx.saved_tensors
        w1_shape, wd_shape, x_dtype, s2, w2dt = ctx.meta
        N, H, W = xb.shape[0], xb.shape[2], xb.shape[3]
        C = w1_shape[0]
        if os.environ.get("RADHIP_B0X_BWD", "1") != "0":
            dy = _nhwc(dy.to(xb.dtype))
            dx = torch.empty(N, 1, H, W, device=xb.device, dtype=torch.float32)
            part = torch.empty(lib().rdx_b0x_bwd_nblk(N, W), 6560, device=xb.device, dtype=torch.float32)
            # MFMA work: conv2's input gradient and weight gradient (2 x the forward's conv2)
            with _timed("b0x_bwd", dy, 4.0 * N * H * W * 32 * 192):
                check(_L(xb).rdx_b0x_bwd(_p(xb), _p(dy), _p(arg), _p(w1b), _p(wdb), _p(bn5), _p(wd2), _p(dx), _p(part),
                                        N, H, W, _stream(dy)), "b0x_bwd")
            tot = part.sum(0)
            dw2 = tot[:6144].view(2, 3, C, C).permute(2, 3, 0, 1)
            dw1 = tot[6144:6336].reshape(w1_shape)
            dwd = tot[6336:6432].reshape(wd_shape)
            dbias = tot[6432:6464]
            sums = tot[6464:6560].view(3, C)
            return (dx.to(x_dtype), dw1, dwd, sums[0], None, None, sums[1], sums[2], dw2.to(w2dt), dbias, dbias)
        c, out1, _ = _b0_fwd(xb, w1b, wdb, bn5)
        ds, dbias = _res_tail_bwd(_nhwc(dy.to(xb.dtype)), arg, (N, C, H, W))
        dc, sums, dw2 = _conv2_grad_to_c(ds, out1, c, wd2, s2, bn5, f32)
        dx, dw1, dwd = _b0_bwd(xb, dc, ds, w1b, wdb, (w1_shape, wd_shape))
        return dx.to(x_dtype), dw1, dwd, sums[0], None, None, sums[1], sums[2], dw2.to(w2dt), dbias, dbias


# ------------------------------------------------------------ WavLM positional convolution ----
def posconv_weights(weight, hd=torch.bfloat16):
    """Conv weight [1024, 64, 128] (weight_norm applied) -> the two 16-bit (hd) operand layouts of csrc/posconv.hip:
    wk [16][128][64 n][64 c] = W[g*64+n, c, k] (forward) and wkt [16][128][64 c][64 n] = W[g*64+n, c, 127-k]
    (input gradient)."""
    W = weight.detach().reshape(16, 64, 64, 128)                             # [g, n, c, k]
    wk = W.permute(0, 3, 1, 2).contiguous().to(hd)
    wkt = W.flip(-1).permute(0, 3, 2, 1).contiguous().to(hd)
    return wk, wkt


class PosConv(torch.autograd.Function):
    """gelu(conv1d(h, W, bias, padding=64, groups=16)[..., :T]) on bf16 [B, T, 1024] token-major rows: the
    WavLM positional embedding (HF WavLMPositionalConvEmbedding) with frozen W / bias, as one MFMA launch
    (rdx_posconv_fwd); the backward returns the input gradient only (rdx_posconv_bwd)."""

    @staticmethod
    def forward(ctx, h, wk, wkt, bias):
        _require_gpu(h)
        B, T, E = h.shape
        if E != 1024:
            raise ValueError("radhip posconv: 1024 channels (16 groups of 64) required")
        h = h.to(wk.dtype).contiguous()
        bias = bias.detach().float().contiguous()
        y = torch.empty_like(h)
        u = torch.empty_like(h)
        with _timed("posconv_fwd", h, 2.0 * B * T * E * 64 * 128):
            check(_L(h).rdx_posconv_fwd(_p(h), _p(wk), _p(bias), _p(y), _p(u), B, T, _stream(h)), "posconv_fwd")
        ctx.save_for_backward(u, wkt)
        return y

    @staticmethod
    def backward(ctx, dy):
        u, wkt = ctx.saved_tensors
        B, T, E = u.shape
        dy = dy.to(u.dtype).contiguous()
        dh = torch.empty_like(u)
        with _timed("posconv_bwd", dy, 2.0 * B * T * E * 64 * 128):
            check(_L(u).rdx_posconv_bwd(_p(dy), _p(u), _p(wkt), _p(dh), B, T, _stream(dy)), "posconv_bwd")
        return dh, None, None, None


# ---------------------------------------------------------------- WavLM gated attention -------
def _ld(t):
    """Row stride of a [B, T, E] view whose last dim is contiguous (e.g. a column slice of q|k|v)."""
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
        raise ValueError("radhip attention: expected a [B, T, E] row view with unit column stride")
    return t.stride(1)


def rel_bias_table(pb, check=True):
    """[H, T, T] position bias -> its relative-position table [H, 2T - 1] fp32, table[h, j - i + T - 1] =
    pb[h, i, j]. WavLM's bias (compute_bias: bucketed key - query offsets) depends on j - i only; `check`
    verifies that before the kernels rely on it. A [H, 2T - 1] input is taken as the table."""
    if pb.dim() == 2:
        return pb.detach().float().contiguous()
    H, T, T2 = pb.shape
    if T != T2:
        raise ValueError("radhip attention: square [H, T, T] position bias expected")
    pb = pb.detach().float()
    tab = torch.cat([pb[:, 1:, 0].flip(1), pb[:, 0, :]], dim=1).contiguous()            # d = -(T-1) .. T-1
    if check:
        i = torch.arange(T, device=pb.device)
        idx = (i[None, :] - i[:, None] + T - 1)                                          # [i, j] -> j - i + T - 1
        if not torch.equal(tab[:, idx], pb):
            raise ValueError("radhip attention: the position bias must depend on key - query only (Toeplitz)")
    return tab


FUSED_BWD_MAX_T = 224


def fused_bwd_enabled(T):
    return T <= FUSED_BWD_MAX_T and os.environ.get("RADHIP_ATTN_BWD", "fused") != "split"


def attn_keep_mask(B, T, H, p_drop, device):
    """uint32 buffer for the forward's dropout keep bits, read by the fused backward (None without
    dropout or when the fused backward does not apply)."""
    if p_drop <= 0 or not fused_bwd_enabled(T):
        return None
    return torch.empty(lib().rdx_attn_keep_mask_words(B, T, H), device=device, dtype=torch.int32)


_ATTN_WS = {}
_ATTN_NEED = {}   # device index -> (floats, counters): the largest split-backward workspace an eager launch asked for


def _attn_split_workspace(dev, n_floats, n_counters):
    """fp32 partial dQ / d gate and the per-(b, h) tickets of the split attention backward, one per (device,
    stream): launches on one stream run one after another, launches in flight on two streams must not share them;
    the tickets are zeroed here once and left at zero by each launch. Captured launches take the device's graph
    workspace (reserve_graph_workspace sizes it before capture; a capture that needs more grows it in the capture)."""
    need = _ATTN_NEED.get(dev.index, (0, 0))
    _ATTN_NEED[dev.index] = (max(need[0], n_floats), max(need[1], n_counters))
    capturing = torch.cuda.is_current_stream_capturing()
    key = (dev.index, "graph") if capturing else (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    cur = _ATTN_WS.get(key)
    if cur is None or cur[0].numel() < n_floats or cur[1].numel() < n_counters:
        cur = _grow_workspace(_ATTN_WS, key, cur, n_floats, n_counters, torch.float32, dev)
    return cur


def attn_bwd_launch(q, ldq, k, ldk, v, ldv, gate, rel, mask, seed, salt, p_drop, o, ldo, lse, do, lddo, D, dq, dk, dv,
                    ldg, dgate, B, T, H, stream, dtype=torch.bfloat16):
    """One gated-attention backward: the fused one-workgroup-per-(b, h) kernel when T <= 224 (dropout from
    the forward's keep mask), else the query-stationary dQ + key-stationary dK/dV kernel pair (dropout
    re-hashed from the seed). rel: the [H, 2T - 1] relative-position bias table; dtype: the 16-bit storage of
    q / k / v (the library)."""
    L = _L(dtype)
    if fused_bwd_enabled(T):
        if p_drop > 0 and mask is None:
            raise RuntimeError("fused attention backward with dropout needs the forward's keep mask")
        if B * H < 256 and (B * H) % 8 == 0 and os.environ.get("RADHIP_ATTN_SPLIT", "1") == "1":
            # B = 8: two workgroups per (b, h) over the key tiles, the second to finish combines dQ / d gate (fills
            # the chip; partials published write-through): 3.83 vs 4.01 ms of attention backward per step in-step
            # (profiles/r05_ab/asplit_*.json); RADHIP_ATTN_SPLIT=0 keeps one workgroup per (b, h)
            ws, cnt = _attn_split_workspace(gate.device, int(lib().rdx_attn_bwd_split_ws(B, H)), B * H)
            return check(L.rdx_attn_bwd_fused_split(q, ldq, k, ldk, v, ldv, _p(gate), _p(rel),
                                                        _p(mask) if mask is not None else None, p_drop, 0.125, o,
                                                        ldo, _p(lse), do, lddo, _p(D), dq, dk, dv, ldg, _p(dgate),
                                                        _p(ws), ws.numel(), _p(cnt), cnt.numel(), B, T, H, 64,
                                                        stream), "attn_bwd_fused_split")
        return check(L.rdx_attn_bwd_fused(q, ldq, k, ldk, v, ldv, _p(gate), _p(rel),
                                              _p(mask) if mask is not None else None, p_drop, 0.125, o, ldo, _p(lse),
                                              do, lddo, _p(D), dq, dk, dv, ldg, _p(dgate), B, T, H, 64, stream),
                     "attn_bwd_fused")
    return check(L.rdx_attn_bwd(q, ldq, k, ldk, v, ldv, _p(gate), _p(rel), seed, salt, p_drop, 0.125, o, ldo,
                                    _p(lse), do, lddo, _p(D), dq, dk, dv, ldg, _p(dgate), B, T, H, 64, stream),
                 "attn_bwd")


class GatedAttention(torch.autograd.Function):
    """softmax(Q K^T / sqrt(64) + gate[b,i,h] * pb[h,i,j]) with dropout, times V, per head (64-dim heads),
    on bf16 [B, T, H*64] row views; returns [B, T, H*64] bf16 (ready for out_proj). Gradients for q, k, v
    and gate (the position bias pb comes from the frozen rel_attn_embed table and takes none)."""

    @staticmethod
    def forward(ctx, q, k, v, gate, pos_bias, seed, p_drop, salt):
        _require_gpu(q, k, v, gate, pos_bias)
        B, T, E = q.shape
        H = gate.shape[2]
        if E != H * 64 or q.dtype not in HALF or k.dtype != q.dtype or v.dtype != q.dtype:
            raise ValueError("radhip attention: bf16 / fp16 q/k/v with 64-dim heads required")
        if pos_bias.requires_grad:
            raise ValueError("radhip attention: the position bias must be frozen")
        gate = gate.contiguous().float()
        rel = rel_bias_table(pos_bias)
        o = torch.empty(B, T, E, device=q.device, dtype=q.dtype)
        lse = torch.empty(B, H, T, device=q.device, dtype=torch.float32)
        sd = seed if seed is not None else torch.zeros(1, dtype=torch.int64, device=q.device)
        mask = attn_keep_mask(B, T, H, float(p_drop), q.device)
        with _timed("attn_fwd", q, 2.0 * 2 * B * H * T * T * 64):
            check(_L(q).rdx_attn_fwd(_p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(gate), _p(rel),
                                     _p(sd), int(salt), float(p_drop), 0.125, _p(o), E, _p(lse),
                                     _p(mask) if mask is not None else None, B, T, H, 64, _stream(q)), "attn_fwd")
        ctx.mask = mask
        ctx.save_for_backward(q, k, v, gate, rel, sd, o, lse)
        ctx.p, ctx.salt = float(p_drop), int(salt)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, gate, rel, sd, o, lse = ctx.saved_tensors
        B, T, E = q.shape
        H = gate.shape[2]
        do = do.to(q.dtype).contiguous()
        D = torch.empty(B, H, T, device=q.device, dtype=torch.float32)
        dq = torch.empty(B, T, E, device=q.device, dtype=q.dtype)
        dk, dv = torch.empty_like(dq), torch.empty_like(dq)
        dgate = torch.empty(B, T, H, device=q.device, dtype=torch.float32)
        with _timed("attn_bwd", q, 2.0 * 5 * B * H * T * T * 64):
            attn_bwd_launch(_p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), gate, rel, ctx.mask, _p(sd), ctx.salt,
                            ctx.p, _p(o), E, lse, _p(do), E, D, _p(dq), _p(dk), _p(dv), E, dgate, B, T, H, _stream(q),
                            q.dtype)
        return dq, dk, dv, dgate, None, None, None, None


def attention_dropout_mask(seed, salt, p_drop, shape):
    """The keep mask (uint8) GatedAttention uses for elements [B, H, T, T] (tests)."""
    n = 1
    for s in shape:
        n *= s
    keep = torch.empty(n, dtype=torch.uint8, device=seed.device)
    check(lib().rdx_attn_dropout_mask(_p(seed), int(salt), float(p_drop), _p(keep), n, int(shape[-1]), _stream(seed)),
          "attn_mask")
    return keep.view(*shape)


def dropout_mask(seed, salt, p_drop, shape):
    """The keep mask (uint8) of the element-wise counter-hash dropout of csrc/wavlm_layer.hip (hidden and
    LoRA dropouts of the fused WavLM layer) over elements [*shape] in row-major order (tests)."""
    n = 1
    for s in shape:
        n *= s
    keep = torch.empty(n, dtype=torch.uint8, device=seed.device)
    check(lib().rdx_dropout_mask(_p(seed), int(salt), float(p_drop), _p(keep), n, _stream(seed)), "dropout_mask")
    return keep.view(*shape)


# ------------------------------------------------------------------------ 16-bit GEMM --------
def gemm_flops(M, N, K):
    return 2.0 * M * N * K


def gemm(a, b, bias=None, epilogue=_lib.EPI_BIAS, aux=None, out=None, aux_out=None, seed=None, salt=0, p_drop=0.0,
         name="gemm"):
    """C[M, N] = a[M, K] @ b[N, K]^T (+ fused epilogue) on the hand-written MFMA kernel (csrc/gemm.hip):
    16-bit (bf16 or fp16) row views a, b (unit inner stride); returns C (a's dtype, or fp32 for EPI_RESID_DROP)."""
    _require_gpu(a, b)
    if a.dtype not in HALF or b.dtype != a.dtype or a.stride(-1) != 1 or b.stride(-1) != 1:
        raise ValueError("radhip gemm: bf16 / fp16 operands of one dtype with unit inner stride required")
    M, K = a.shape
    N, K2 = b.shape
    if K != K2:
        raise ValueError(f"radhip gemm: K mismatch {K} vs {K2}")
    if out is None:
        dt = torch.float32 if epilogue == _lib.EPI_RESID_DROP else a.dtype
        out = torch.empty(M, N, device=a.device, dtype=dt)
    if epilogue == _lib.EPI_BIAS_GELU and aux_out is None:
        aux_out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    with _timed(name, a, gemm_flops(M, N, K), shape=(M, N, K)):
        check(_L(a).rdx_gemm_bf16(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K,
                                  _p(bias) if bias is not None else None, int(epilogue),
                                  _p(aux) if aux is not None else None, aux.stride(0) if aux is not None else 0,
                                  _p(aux_out) if aux_out is not None else None,
                                  aux_out.stride(0) if aux_out is not None else 0,
                                  _p(seed) if seed is not None else None, int(salt), float(p_drop), _stream(a)),
              "gemm_bf16")
    return (out, aux_out) if epilogue == _lib.EPI_BIAS_GELU else out


# (tile, splits) of csrc/wgemm.hip per WavLM layer GEMM and token-count class; a missing entry runs on hipBLASLt.
# Chosen in the step (rocprofv3 traces of bench.py, profiles/r03_wgemm_in_step.txt), not from standalone timings:
# standalone (tools/bench_wgemm.py, profiles/r03_wgemm_sweep.jsonl) the B = 8 q/k/v GEMM took 17.3 us on the
# 128 x 192 tile vs hipBLASLt's 22.7, in the step 21.3 vs 22.1 (cold weights from HBM); FFN2's input gradient
# with the GELU backward fused took 30.9 us in the step vs 18.0 + 9.3 for hipBLASLt's 128 x 192 kernel + the
# GELU backward, so it stays unfused. out_proj / its input gradient (64 x 64 tiles, 10.3 us vs 20-27) and FFN1 +
# GELU (28.3 vs 32.7) run here; every B = 32 shape and the N = 1024, K = 3072 / 4096 ones stay on hipBLASLt.
#
# Round 5: csrc/hgemm.hip ("hg", tile, splits, group_m), the 8-wave ping-pong kernel with the slab ring and the
# A&S-erf GELU epilogues, standalone against hipBLASLt on one box (tools/bench_hgemm.py,
# profiles/r05_hgemm_sweep.jsonl, us): B = 8 q/k/v 15.8 vs 22.8 (pgemm 18.9), FFN1 + GELU 22.4 vs 30.2 (with torch's
# GELU), FFN2's input gradient + GELU backward 22.4, out_proj / its input gradient 11.3 vs 21.8; B = 32 out_proj /
# d_out 18.5 vs 23, FFN1 + GELU 71 vs 80, FFN2 56.5 vs 60, d_ffn1 56 vs 60, d_qkv 44.9 vs 46.5, q/k/v 46.7 vs 46.0,
# d_ffn2 81.7 vs 81 (+ the separate GELU backward). The B = 8 N = 1024 long-K shapes (FFN2, d_ffn1, d_qkv: 104
# tiles of 128 x 128 on 256 CUs) take split-K 2 with write-through partials: 25.2 vs 25.6, 20.9 vs 21.2
# (profiles/r05_hgemm_splitk.jsonl; stream-K over all 256 CUs measured slower, 29.3: two prologues and two partials
# per run).
WGEMM_POLICY_R4 = {
    "b8": {"qkv": ("pg", 4, 4), "out": (5, 1), "d_out": (5, 1), "ffn1": (6, 1)},
    "b32": {},
}
# tile orders (group_m) chosen by L2 fill traffic: rocprofv3 FETCH_SIZE per launch under column-panel order (0),
# 4-row-tile groups (4) and the XCD grid (-R), profiles/r05_pmc_hgemm_order.jsonl (e.g. B = 32 FFN1 9.2x the A + B
# bytes in column order, 4.7x at 4; B = 8 FFN2 5.9x -> 4.2x at 4) and by time (standalone sweep of the orders,
# profiles/r05_hgemm_orders.jsonl: 4 fastest for every shape but the B = 8 FFN1 pair, 0); in-step A/B of the first
# such table 469.7 vs 461.0 utt/s (profiles/r05_ab/fo_*.json)
WGEMM_POLICY_R5A = {
    "b8": {"qkv": ("hg", 3, 1, 0), "out": ("hg", 4, 1, 0), "d_out": ("hg", 4, 1, 0), "ffn1": ("hg", 202, 1, 0),
           "d_ffn2": ("hg", 202, 1, 0), "ffn2": ("hg", 4, 2, 0), "d_ffn1": ("hg", 4, 2, 0), "d_qkv": ("hg", 4, 2, 0)},
    "b32": {"qkv": ("hg", 1, 1, 0), "out": ("hg", 2, 1, 0), "d_out": ("hg", 2, 1, 0), "ffn1": ("hg", 0, 1, 0),
            "d_ffn2": ("hg", 0, 1, 0), "ffn2": ("hg", 2, 1, 0), "d_ffn1": ("hg", 2, 1, 0), "d_qkv": ("hg", 2, 1, 0)},
}
WGEMM_POLICY_R5G = {
    "b8": {"qkv": ("hg", 3, 1, 4), "out": ("hg", 4, 1, 4), "d_out": ("hg", 4, 1, 4), "ffn1": ("hg", 202, 1, 0),
           "d_ffn2": ("hg", 202, 1, 0), "ffn2": ("hg", 4, 2, 4), "d_ffn1": ("hg", 4, 2, 4), "d_qkv": ("hg", 4, 2, 4)},
    "b32": {"qkv": ("hg", 1, 1, 4), "out": ("hg", 2, 1, 4), "d_out": ("hg", 2, 1, 4), "ffn1": ("hg", 0, 1, 4),
            "d_ffn2": ("hg", 0, 1, 4), "ffn2": ("hg", 2, 1, 4), "d_ffn1": ("hg", 2, 1, 4), "d_qkv": ("hg", 2, 1, 4)},
}
# 64 x 128 tiles (code 6) for the B = 8 N = 1024 shapes: 208 tiles on 256 CUs instead of 104, no split-K.
# Standalone (tools/bench_hgemm.py, profiles/r05_hgemm_tile64.jsonl, us) every such shape gained: out / d_out
# 11.1 -> 9.2, FFN2 24.0 -> 22.7, FFN1's input gradient 24.1 -> 22.4, q/k/v's 20.8 -> 18.4; in the step
# (profiles/r05_ab/t6_*, per-shape graph timings) only the K = 1024 pair did (13.05 -> 11.2), the K = 4096 pair lost
# (26.1 -> 27.5) and K = 3072 was even: the long-K shapes keep 128 x 128 with split-K 2
WGEMM_POLICY_T6 = {
    "b8": {"qkv": ("hg", 3, 1, 4), "out": ("hg", 6, 1, 4), "d_out": ("hg", 6, 1, 4), "ffn1": ("hg", 202, 1, 0),
           "d_ffn2": ("hg", 202, 1, 0), "ffn2": ("hg", 6, 1, 4), "d_ffn1": ("hg", 6, 1, 4), "d_qkv": ("hg", 6, 1, 4)},
    "b32": {"qkv": ("hg", 1, 1, 4), "out": ("hg", 2, 1, 4), "d_out": ("hg", 2, 1, 4), "ffn1": ("hg", 0, 1, 4),
            "d_ffn2": ("hg", 0, 1, 4), "ffn2": ("hg", 2, 1, 4), "d_ffn1": ("hg", 2, 1, 4), "d_qkv": ("hg", 2, 1, 4)},
}
# B = 32 long-K shapes (ffn2, d_ffn1, d_qkv: N = 1024 at K = 4096 / 3072) on 256 x 128 tiles (code 5) instead of
# 128 x 128: in-step A/B 6 of 6 interleaved rounds faster, 485.3 / 486.9 / 485.1 / 484.9 / 484.5 / 485.5 vs
# 484.9 / 485.2 / 484.5 / 484.9 / 484.1 / 483.1 utt/s (tools/gpu_policy_ab.sh, profiles/r06_policy_ab.jsonl); the
# other variants tried there (B = 8 ffn1 on code 7, long-K on 64 x 128, qkv on code 7) were 1.5-4 % slower
WGEMM_POLICY = {
    "b8": {"qkv": ("hg", 3, 1, 4), "out": ("hg", 6, 1, 4), "d_out": ("hg", 6, 1, 4), "ffn1": ("hg", 202, 1, 0),
           "d_ffn2": ("hg", 202, 1, 0), "ffn2": ("hg", 4, 2, 4), "d_ffn1": ("hg", 4, 2, 4), "d_qkv": ("hg", 4, 2, 4)},
    "b32": {"qkv": ("hg", 1, 1, 4), "out": ("hg", 2, 1, 4), "d_out": ("hg", 2, 1, 4), "ffn1": ("hg", 0, 1, 4),
            "d_ffn2": ("hg", 0, 1, 4), "ffn2": ("hg", 5, 1, 4), "d_ffn1": ("hg", 5, 1, 4), "d_qkv": ("hg", 5, 1, 4)},
}
WGEMM_POLICY_R6A = {"b8": WGEMM_POLICY["b8"], "b32": WGEMM_POLICY_R5G["b32"]}   # the default before that A/B


def wgemm_policy(name, M, N, K):
    """The kernel for the fused WavLM layer's GEMM `name` (qkv, out, ffn1, ffn2 and the input gradients d_qkv,
    d_out, d_ffn1 (FFN1's), d_ffn2 (FFN2's, with the GELU backward fused)) at M token rows: (tile, splits) of
    csrc/wgemm.hip, ("pg", tile, group_m) of csrc/pgemm.hip, or None for hipBLASLt. RADHIP_WGEMM=0 routes
    everything to hipBLASLt; RADHIP_WGEMM_POLICY (JSON, same layout as WGEMM_POLICY) overrides the table for A/B
    runs."""
    if os.environ.get("RADHIP_WGEMM", "1") == "0" or K % 64 or N % 8:
        return None
    table = WGEMM_POLICY
    env = os.environ.get("RADHIP_WGEMM_POLICY")
    if env:     # a JSON table, or the name of one of this module's tables (R4, R5A, R5G, T6, R6A)
        import json
        table = json.loads(env) if env.lstrip().startswith("{") else globals()["WGEMM_POLICY_" + env.upper()]
    ent = table.get("b8" if M <= 2048 else "b32", {}).get(name)
    if ent is None:
        return None
    if ent[0] == "pg":
        return ("pg", int(ent[1]), int(ent[2]))
    if ent[0] == "hg":
        return ("hg", int(ent[1]), int(ent[2]), int(ent[3]))
    return (int(ent[0]), int(ent[1]))


def layer_gemm(pol, a, b, bias=None, epilogue=_lib.EPI_BIAS, aux=None):
    """Run a WavLM layer GEMM C = a @ b^T (+ epilogue) on the kernel `pol` names (wgemm_policy, not None)."""
    if pol[0] == "pg":
        return pgemm(a, b, bias, epilogue=epilogue, aux=aux, tile=pol[1], group_m=pol[2])
    if pol[0] == "hg":
        return hgemm(a, b, bias, epilogue=epilogue, aux=aux, tile=pol[1], splits=pol[2], group_m=pol[3])
    return wgemm(a, b, bias, epilogue=epilogue, aux=aux, tile=pol[0], splits=pol[1])


def wgrad_acc(dy, x, dw, db=None):
    """dw += dy^T x and db += dy.sum(0) in fp32 on csrc/wgrad.hip: dy [M, N], x [M, K] bf16 row views (unit inner
    stride; bf16 or fp16, one dtype), dw fp32 [N, K] (row stride >= K, unit inner stride), db fp32 [N] or None."""
    _require_gpu(dy, x)
    if dy.dtype not in HALF or x.dtype != dy.dtype or dy.stride(-1) != 1 or x.stride(-1) != 1:
        raise ValueError("radhip wgrad_acc: bf16 / fp16 operands of one dtype with unit inner stride required")
    M, N = dy.shape
    M2, K = x.shape
    if M != M2 or dw.shape != (N, K) or dw.dtype != torch.float32 or dw.stride(-1) != 1:
        raise ValueError(f"radhip wgrad_acc: shapes dy {tuple(dy.shape)} x {tuple(x.shape)} dw {tuple(dw.shape)}")
    if db is not None and (db.shape != (N,) or db.dtype != torch.float32 or not db.is_contiguous()):
        raise ValueError("radhip wgrad_acc: db must be fp32 [N]")
    if _WGRAD_BATCH is not None and torch.cuda.current_stream(dy.device) == _WGRAD_BATCH[0]:
        _WGRAD_BATCH[1].append((dy, x, dw, db))       # run with the pass's other weight gradients (wgrad_batch)
        return
    ws = torch.empty(int(lib().rdx_wgrad_ws_floats(M, N, K)), device=dy.device, dtype=torch.float32)
    with _timed("wgrad_acc", dy, gemm_flops(N, K, M), shape=(M, N, K)):
        check(_L(dy).rdx_wgrad_acc(_p(dy), dy.stride(0), _p(x), x.stride(0), M, N, K, _p(dw), dw.stride(0),
                                  _p(db) if db is not None else None, _p(ws), ws.numel(), _stream(dy)), "wgrad_acc")



# (stream, [(dy, x, dw, db), ...]) while a backward pass batches its weight gradients (wgrad_batch)
_WGRAD_BATCH = None
WGRAD_MANY_MAX = 32     # problems per batched launch (csrc/wgrad.hip WGM_MAXP)


class wgrad_batch:
    """Within the block, wgrad_acc calls on the current stream (SideLinear's backward: the detector head's 31
    linears per pass) are collected instead of launched, and on exit run as batched launches (csrc/wgrad.hip
    rdx_wgrad_acc_many, two kernels per up to 32 gradients instead of two per gradient). Launched one by one in a
    captured graph they cost ~12 us each, almost all launch boundary. The accumulation into each .grad is the
    same add; only its place in the stream moves to the end of the backward, before anything reads .grad.
    RADHIP_WGRAD_BATCH=0 (or a nested block) leaves the launches where they were."""

    def __init__(self, device=None):
        self.device = device

    def __enter__(self):
        global _WGRAD_BATCH
        self.on = (_WGRAD_BATCH is None and torch.cuda.is_available()
                   and os.environ.get("RADHIP_WGRAD_BATCH", "1") != "0")
        if self.on:
            _WGRAD_BATCH = (torch.cuda.current_stream(self.device), [])
        return self

    def __exit__(self, et, ev, tb):
        global _WGRAD_BATCH
        if not self.on:
            return False
        pend = _WGRAD_BATCH[1]
        _WGRAD_BATCH = None
        if et is None:
            wgrad_acc_many(pend)
        return False


def wgrad_groups(items):
    """Split (dy, x, dw, db) items into launches of at most WGRAD_MANY_MAX problems of one dtype in which every dw /
    db is targeted once, keeping item order."""
    groups, cur, seen = [], [], set()
    for it in items:
        keys = {it[2].data_ptr()} | ({it[3].data_ptr()} if it[3] is not None else set())
        if cur and (len(cur) == WGRAD_MANY_MAX or keys & seen or it[0].dtype != cur[0][0].dtype):
            groups.append(cur)
            cur, seen = [], set()
        cur.append(it)
        seen |= keys
    if cur:
        groups.append(cur)
    return groups


def wgrad_acc_many(items):
    """dw += dy^T x (and db += dy.sum(0)) for every (dy, x, dw, db) of `items`, each as wgrad_acc takes them, in
    batched launches of up to WGRAD_MANY_MAX problems of one dtype. A launch holds each output once: a gradient
    whose dw / db an earlier item of the launch already targets starts the next launch (same stream: the adds stay
    in item order)."""
    for g in wgrad_groups(items):
        n = len(g)
        ints = lambda vals: (ctypes.c_int * n)(*vals)
        i64s = lambda vals: (ctypes.c_int64 * n)(*vals)
        M = ints([it[0].shape[0] for it in g])
        N = ints([it[0].shape[1] for it in g])
        K = ints([it[1].shape[1] for it in g])
        L = _L(g[0][0])
        nws = int(lib().rdx_wgrad_many_ws_floats(n, M, N, K, ints([int(it[3] is not None) for it in g])))
        dy0 = g[0][0]
        ws = torch.empty(nws, device=dy0.device, dtype=torch.float32)
        flops = sum(gemm_flops(it[0].shape[1], it[1].shape[1], it[0].shape[0]) for it in g)
        with _timed("wgrad_many", dy0, flops, shape=(n, sum(it[0].shape[0] for it in g))):
            check(L.rdx_wgrad_acc_many(n, ptr_array([it[0].data_ptr() for it in g]),
                                       i64s([it[0].stride(0) for it in g]), ptr_array([it[1].data_ptr() for it in g]),
                                       i64s([it[1].stride(0) for it in g]), M, N, K,
                                       ptr_array([it[2].data_ptr() for it in g]), i64s([it[2].stride(0) for it in g]),
                                       ptr_array([it[3].data_ptr() if it[3] is not None else None for it in g]),
                                       _p(ws), ws.numel(), _stream(dy0)), "wgrad_acc_many")

_WG_WS = {}
_WG_NEED = {}   # device index -> (bytes, counters): the largest split-K workspace an eager launch has asked for


def _wgemm_workspace(dev, ws_bytes, n_counters):
    """Split-K workspace of csrc/wgemm.hip / csrc/hgemm.hip: fp32 partial slabs and per-tile arrival tickets (zeroed
    once here; the last arriver re-zeroes its ticket). Eager launches take one per (device, stream): launches on one
    stream run one after another, while two launches in flight at once on different streams (the SincNet side
    stream, SideLinear's) must not share slabs or tickets. Launches captured into HIP graphs take the device's graph
    workspace, reserved before capture (reserve_graph_workspace) at the largest size the eager warm-up asked for, and
    grown inside a capture that needs more: the graphs' split-K GEMMs (the WavLM layers') are captured on one stream
    and replayed one graph after another."""
    need = _WG_NEED.get(dev.index, (0, 0))
    _WG_NEED[dev.index] = (max(need[0], ws_bytes), max(need[1], n_counters))
    capturing = torch.cuda.is_current_stream_capturing()
    key = (dev.index, "graph") if capturing else (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    cur = _WG_WS.get(key)
    if cur is None or cur[0].numel() < ws_bytes or cur[1].numel() < n_counters:
        cur = _grow_workspace(_WG_WS, key, cur, ws_bytes, n_counters, torch.uint8, dev)
    return cur


_WS_KEEP = []         # every graph workspace pair ever handed out: captured graphs hold raw pointers into them
_CAPTURE_TICKETS = []  # tickets allocated inside a capture: zeroed eagerly by finalize_graph_workspace


def _grow_workspace(table, key, cur, n, n_counters, dtype, dev):
    """A larger (slab, zeroed tickets) workspace for `key`. During a capture the allocation comes from the graph's
    memory pool and its zero fill is only a node of the capturing graph: another graph captured later on the same
    (device, "graph") key could replay first and find the tickets uninitialised. So the tickets grown in a capture are
    also zeroed eagerly once the capture has ended (finalize_graph_workspace, called by every capture site before
    any replay). A graph workspace it replaces stays referenced (_WS_KEEP): graphs captured earlier keep its
    addresses. An eager per-stream workspace it replaces is freed (no graph points into it)."""
    n = max(n, cur[0].numel() if cur else 0)
    nc = max(n_counters, cur[1].numel() if cur else 0)
    new = (torch.empty(n, dtype=dtype, device=dev), torch.zeros(nc, dtype=torch.int32, device=dev))
    if key[1] == "graph":
        _WS_KEEP.append(new)
        if torch.cuda.is_current_stream_capturing():
            _CAPTURE_TICKETS.append(new[1])
    table[key] = new
    return new


def finalize_graph_workspace(dev=None):
    """After a capture (before any replay): zero, eagerly, every split-K / split-attention ticket array a capture
    allocated, then synchronise."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("finalize_graph_workspace inside a capture")
    while _CAPTURE_TICKETS:
        _CAPTURE_TICKETS.pop().zero_()
    torch.cuda.synchronize(dev)


def reserve_graph_workspace(dev):
    """Allocate (outside capture) the graph workspaces (split-K GEMM, split attention backward) at the largest size
    an eager launch on `dev` needed."""
    dev = torch.device(dev)
    key = (dev.index, "graph")
    for table, need, dt in ((_WG_WS, _WG_NEED, torch.uint8), (_ATTN_WS, _ATTN_NEED, torch.float32)):
        nb, nc = need.get(dev.index, (0, 0))
        if nb == 0:
            continue
        cur = table.get(key)
        if cur is None or cur[0].numel() < nb or cur[1].numel() < nc:
            _grow_workspace(table, key, cur, nb, nc, dt, dev)


def wgemm(a, b, bias=None, epilogue=_lib.EPI_BIAS, aux=None, out=None, aux_out=None, tile=-1, name="wgemm",
          splits=1):
    """C[M, N] = a[M, K] @ b[N, K]^T (+ fused epilogue) on csrc/wgemm.hip (LDS-DMA pipelined MFMA GEMM):
    16-bit (bf16 / fp16) row views a, b (unit inner stride, 16-byte aligned, K % 64 == 0); returns C, or
    (C, gelu(C)) for EPI_BIAS_GELU. splits > 1: split-K over that many workgroups per output tile (last-arriver
    reduction)."""
    _require_gpu(a, b)
    if a.dtype not in HALF or b.dtype != a.dtype or a.stride(-1) != 1 or b.stride(-1) != 1:
        raise ValueError("radhip wgemm: bf16 / fp16 operands of one dtype with unit inner stride required")
    M, K = a.shape
    N, K2 = b.shape
    if K != K2 or K % 64:
        raise ValueError(f"radhip wgemm: K {K} vs {K2} (K % 64 == 0 required)")
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    if epilogue == _lib.EPI_BIAS_GELU and aux_out is None:
        aux_out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    st = _stream(a)
    ws = cnt = None
    ws_bytes = n_cnt = 0
    if splits > 1:
        if tile < 0:
            raise ValueError("radhip wgemm: split-K needs an explicit tile")
        ws_bytes = int(lib().rdx_wgemm_ws_bytes(M, N, int(tile), int(splits)))
        n_cnt = int(lib().rdx_wgemm_counters(M, N, int(tile)))
        if ws_bytes <= 0 or n_cnt <= 0:
            raise ValueError(f"radhip wgemm: no split-K geometry for tile {tile}")
        ws, cnt = _wgemm_workspace(a.device, ws_bytes, n_cnt)
        ws_bytes, n_cnt = ws.numel(), cnt.numel()
    with _timed(name, a, gemm_flops(M, N, K), shape=(M, N, K)):
        check(_L(a).rdx_wgemm_bf16_ex(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K,
                                      _p(bias) if bias is not None else None, int(epilogue),
                                      _p(aux) if aux is not None else None, aux.stride(0) if aux is not None else 0,
                                      _p(aux_out) if aux_out is not None else None,
                                      aux_out.stride(0) if aux_out is not None else 0, int(tile), int(splits),
                                      _p(ws) if ws is not None else None, ws_bytes,
                                      _p(cnt) if cnt is not None else None, n_cnt, st),
              "wgemm_bf16")
    return (out, aux_out) if epilogue == _lib.EPI_BIAS_GELU else out


def pgemm(a, b, bias=None, epilogue=_lib.EPI_BIAS, aux=None, out=None, aux_out=None, tile=4, group_m=4,
          name="pgemm"):
    """C[M, N] = a[M, K] @ b[N, K]^T (+ fused epilogue) on csrc/pgemm.hip (8-wave deep-pipelined MFMA GEMM, one
    workgroup per output tile): 16-bit (bf16 / fp16) row views a, b (unit inner stride, 16-byte aligned,
    K % 64 == 0); returns C, or (C, gelu(C)) for EPI_BIAS_GELU."""
    _require_gpu(a, b)
    if a.dtype not in HALF or b.dtype != a.dtype or a.stride(-1) != 1 or b.stride(-1) != 1:
        raise ValueError("radhip pgemm: bf16 / fp16 operands of one dtype with unit inner stride required")
    M, K = a.shape
    N, K2 = b.shape
    if K != K2 or K % 64:
        raise ValueError(f"radhip pgemm: K {K} vs {K2} (K % 64 == 0 required)")
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    if epilogue == _lib.EPI_BIAS_GELU and aux_out is None:
        aux_out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    with _timed(name, a, gemm_flops(M, N, K), shape=(M, N, K)):
        check(_L(a).rdx_pgemm_bf16(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K,
                                   _p(bias) if bias is not None else None, int(epilogue),
                                   _p(aux) if aux is not None else None, aux.stride(0) if aux is not None else 0,
                                   _p(aux_out) if aux_out is not None else None,
                                   aux_out.stride(0) if aux_out is not None else 0, int(tile), int(group_m),
                                   _stream(a)), "pgemm_bf16")
    return (out, aux_out) if epilogue == _lib.EPI_BIAS_GELU else out


def hgemm(a, b, bias=None, epilogue=_lib.EPI_BIAS, aux=None, out=None, aux_out=None, tile=0, splits=1, group_m=0,
          name="hgemm"):
    """C[M, N] = a[M, K] @ b[N, K]^T (+ fused epilogue) on csrc/hgemm.hip (8-wave ping-pong MFMA GEMM with a slab
    ring, one workgroup per output tile or split): 16-bit (bf16 / fp16) row views a, b (unit inner stride, 16-byte
    aligned, K % 64 == 0); returns C, or (C, gelu(C)) for EPI_BIAS_GELU. splits > 1: split-K with the in-launch
    last-arriver sum (the per-stream workspace of wgemm); splits == 0: stream-K (one workgroup per CU over equal runs
    of the (tile, K step) units, shared tiles summed by their last arriver; tiles 2-4)."""
    _require_gpu(a, b)
    if a.dtype not in HALF or b.dtype != a.dtype or a.stride(-1) != 1 or b.stride(-1) != 1:
        raise ValueError("radhip hgemm: bf16 / fp16 operands of one dtype with unit inner stride required")
    M, K = a.shape
    N, K2 = b.shape
    if K != K2 or K % 64:
        raise ValueError(f"radhip hgemm: K {K} vs {K2} (K % 64 == 0 required)")
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    if epilogue == _lib.EPI_BIAS_GELU and aux_out is None:
        aux_out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    ws = cnt = None
    ws_bytes = n_cnt = 0
    if splits != 1:
        ws_bytes = int(lib().rdx_hgemm_ws_bytes(M, N, int(tile), int(splits)) if splits > 1
                       else lib().rdx_hgemm_sk_ws_bytes(M, N, K, int(tile)))
        n_cnt = int(lib().rdx_hgemm_counters(M, N, int(tile)))
        if ws_bytes <= 0 or n_cnt <= 0:
            raise ValueError(f"radhip hgemm: no split-K geometry for tile {tile}")
        ws, cnt = _wgemm_workspace(a.device, ws_bytes, n_cnt)
        ws_bytes, n_cnt = ws.numel(), cnt.numel()
    with _timed(name, a, gemm_flops(M, N, K), shape=(M, N, K)):
        check(_L(a).rdx_hgemm(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K,
                              _p(bias) if bias is not None else None, int(epilogue),
                              _p(aux) if aux is not None else None, aux.stride(0) if aux is not None else 0,
                              _p(aux_out) if aux_out is not None else None,
                              aux_out.stride(0) if aux_out is not None else 0, int(tile), int(splits), int(group_m),
                              _p(ws) if ws is not None else None, ws_bytes, _p(cnt) if cnt is not None else None,
                              n_cnt, _stream(a)), "hgemm")
    return (out, aux_out) if epilogue == _lib.EPI_BIAS_GELU else out


# ------------------------------------------------------------------- WavLM CNN feature encoder ----
def fe_conv_weights(layers, hd=torch.bfloat16):
    """Per-layer device operands of the fused frozen CNN (csrc/featconv.hip) from the ConvLayer modules, for the
    16-bit storage dtype hd (the autocast dtype): layer 0 (w fp32 [512, 10] and bias fp32, both rounded to hd as
    autocast feeds them), layers >= 1 the weight permuted to [C_out][k][C_in] = [512, K*512] and the bias, in hd;
    LayerNorm gamma/beta fp32."""
    out = []
    with torch.no_grad():
        for i, ly in enumerate(layers):
            c = ly.conv
            w = c.weight.detach()
            b = c.bias.detach().to(hd) if c.bias is not None else None   # wavlm-large: conv_bias False
            if i == 0:
                wk = w.reshape(w.shape[0], -1).to(hd).float().contiguous()
                bk = b.float().contiguous() if b is not None else torch.zeros(w.shape[0], device=w.device)
            else:
                wk = w.permute(0, 2, 1).reshape(w.shape[0], -1).to(hd).contiguous()
                bk = b.contiguous() if b is not None else None
            out.append((wk, bk, ly.layer_norm.weight.detach().float().contiguous(),
                        ly.layer_norm.bias.detach().float().contiguous(), float(ly.layer_norm.eps),
                        c.kernel_size[0], c.stride[0]))
    return out


# hgemm tile of the frozen CNN's strided convolutions (rdx_hgemm_batched); -1: csrc/gemm.hip's strided GEMM (round 2-5).
# Whole CNN at the window's 32 x 64600 clean batch (tools/bench_fe.py, profiles/r06_bench_fe.jsonl, fp16 / bf16 ms):
# gemm.hip 1.69 / 1.53, hgemm 256 x 256 1.25 / 1.20, 128 x 256 1.29 / 1.24, 128 x 128 1.47 / 1.42
FE_HGEMM_TILE = int(os.environ.get("RADHIP_FE_TILE", "0"))


def feature_encoder_fused(x, ops_):
    """Frozen WavLM CNN, x [B, L] fp32 -> [B, T, 512] fp32 token-major (HF WavLMFeatureEncoder, "layer" norm):
    conv0+LN+GELU in one kernel, then per layer the implicit GEMM (rdx_gemm_bf16_strided, rows of the
    token-major input overlapping at stride*512) and the LN+GELU pass; the last LN+GELU writes fp32."""
    _require_gpu(x)
    if len(ops_) < 2:
        raise ValueError("fused feature encoder: needs at least two conv layers")
    x = x.contiguous().float()
    B, L = x.shape
    w0, b0, g0, be0, eps0, k0, s0 = ops_[0]
    hd = ops_[1][0].dtype                                   # the 16-bit storage dtype the weights were made for
    Lb = _L(hd)
    T = (L - k0) // s0 + 1
    h = torch.empty(B, T, 512, device=x.device, dtype=hd)
    with _timed("fe_conv0", x, 4.0 * B * L + 2.0 * B * T * 512):            # bytes: waveform in, bf16 out
        check(Lb.rdx_fe_conv0(_p(x), B, L, _p(w0), _p(b0), _p(g0), _p(be0), eps0, k0, s0, _p(h), _stream(x)),
              "fe_conv0")
    for i, (w, b, g, be, eps, k, s) in enumerate(ops_[1:], start=1):
        To = (T - k) // s + 1
        y = torch.empty(B, To, 512, device=x.device, dtype=hd)
        with _timed("fe_conv_gemm", x, gemm_flops(B * To, 512, k * 512), shape=(B, T, k)):
            if FE_HGEMM_TILE >= 0 and (k * 512) % 64 == 0:
                # csrc/hgemm.hip batched over the utterances (blockIdx.y), the token-major input read as the
                # im2col matrix (rows overlapping at stride * 512)
                check(Lb.rdx_hgemm_batched(_p(h), s * 512, T * 512, _p(w), w.stride(0), _p(y), 512, To * 512, To,
                                           512, k * 512, B, _p(b) if b is not None else None, FE_HGEMM_TILE, 0,
                                           _stream(x)), "hgemm_batched")
            else:
                check(Lb.rdx_gemm_bf16_strided(_p(h), s * 512, T * 512, _p(w), w.stride(0), _p(y), 512, To, B, To,
                                               512, k * 512, _p(b) if b is not None else None, _stream(x)),
                      "gemm_bf16_strided")
        last = i == len(ops_) - 1
        out32 = torch.empty(B, To, 512, device=x.device, dtype=torch.float32) if last else None
        with _timed("fe_ln_gelu", x, (2.0 + (4.0 if last else 2.0)) * B * To * 512, shape=(B, To)):
            check(Lb.rdx_fe_ln_gelu(_p(y), B * To, _p(g), _p(be), eps, _p(out32) if last else None, _stream(x)),
                  "fe_ln_gelu")
        h, T = (out32 if last else y), To
    return h


# ------------------------------------------------------------------- detector-head small GEMMs ----
def lgemm(a, w, bias=None, epilogue=_lib.EPI_BIAS, aux=None, out_dtype=None, residual=None, out=None, aux_out=None,
          name="lgemm"):
    """C[M, N] = a[M, K] @ w[N, K]^T (+ fused epilogue) on csrc/lgemm.hip, the head's small-GEMM kernel: a 16-bit
    or fp32 (rounded to w's 16-bit dtype on load) 2-D view with unit inner stride and any row stride, w 16-bit.
    out_dtype: w.dtype (default) or torch.float32 (the 16-bit result widened). residual [M, N] in the output dtype:
    C = residual + C (rounded in 16 bits; `out` may be `residual` itself: in-place accumulation). EPI_BIAS_GELU
    returns (u, gelu(u)); EPI_GELU_BWD multiplies by gelu'(aux)."""
    _require_gpu(a, w)
    if w.dtype not in HALF or a.dtype not in (w.dtype, torch.float32) or a.dim() != 2 or w.dim() != 2:
        raise ValueError("radhip lgemm: 2-D a (16-bit or fp32) and 16-bit w required")
    if not ((a.stride(-1) == 1 or a.shape[1] == 1) and (w.stride(-1) == 1 or w.shape[1] == 1)):
        raise ValueError("radhip lgemm: unit inner stride required")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise ValueError(f"radhip lgemm: K {K} vs {K2}")
    od = w.dtype if out_dtype is None else out_dtype
    if od not in (w.dtype, torch.float32):
        raise ValueError("radhip lgemm: output in w's dtype or fp32")
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=od)
    if epilogue == _lib.EPI_BIAS_GELU and aux_out is None:
        aux_out = torch.empty(M, N, device=a.device, dtype=w.dtype)
    def unit(t):
        return t.stride(-1) == 1 or t.shape[-1] == 1
    for t in (bias, aux, aux_out):
        if t is not None and (t.dtype != w.dtype or not unit(t)):
            raise ValueError("radhip lgemm: bias / aux in w's dtype with unit inner stride")
    if residual is not None and (residual.dtype != od or not unit(residual) or residual.shape != (M, N)):
        raise ValueError("radhip lgemm: residual [M, N] in the output dtype with unit inner stride")
    if out.shape != (M, N) or out.dtype != od or not unit(out):
        raise ValueError("radhip lgemm: out [M, N] in the output dtype with unit inner stride")
    def ld(t, cols):   # row stride as the kernel reads it (any value for a single row)
        return t.stride(0) if t.shape[0] > 1 else cols
    if ld(a, K) < K or ld(w, K) < K or ld(out, N) < N:
        raise ValueError("radhip lgemm: overlapping rows")
    with _timed(name, a, gemm_flops(M, N, K), shape=(M, N, K)):
        check(_L(w).rdx_lgemm(_p(a), ld(a, K), int(a.dtype == torch.float32), _p(w), ld(w, K), _p(out),
                              ld(out, N), int(od == torch.float32), M, N, K,
                              _p(bias) if bias is not None else None, int(epilogue),
                              _p(aux) if aux is not None else None, ld(aux, N) if aux is not None else 0,
                              _p(aux_out) if aux_out is not None else None,
                              ld(aux_out, N) if aux_out is not None else 0,
                              _p(residual) if residual is not None else None,
                              ld(residual, N) if residual is not None else 0, _stream(w)), "lgemm")
    return (out, aux_out) if epilogue == _lib.EPI_BIAS_GELU else out


def colsum_many(pairs):
    """out[c] = sum over rows of part[r, c] for each (part [rows, cols] fp32, unit inner stride, out fp32 [cols]) in
    `pairs` (up to 4): one csrc/layersum.hip launch, rows in order (deterministic)."""
    n = len(pairs)
    if not 0 < n <= 4:
        raise ValueError("radhip colsum_many: 1-4 problems")
    for part, out in pairs:
        _require_gpu(part, out)
        if (part.dtype != torch.float32 or out.dtype != torch.float32 or part.dim() != 2 or part.stride(1) != 1
                or out.shape != (part.shape[1],) or not out.is_contiguous()):
            raise ValueError("radhip colsum_many: fp32 [rows, cols] parts and [cols] outputs")
    ints = lambda v: (ctypes.c_int * n)(*v)
    check(lib().rdx_colsum_many(n, ptr_array([p.data_ptr() for p, _ in pairs]), ints([p.shape[0] for p, _ in pairs]),
                                ints([p.shape[1] for p, _ in pairs]),
                                (ctypes.c_int64 * n)(*[p.stride(0) for p, _ in pairs]),
                                ptr_array([o.data_ptr() for _, o in pairs]), _stream(pairs[0][0])), "colsum_many")

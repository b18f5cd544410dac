"""The SincNet stream of the fp32 scoring pass on the x3 kernels (radhip/sinc_x3.py, csrc/sconv_x3.hip).

Every reference is fp64 torch on the CPU and shares no code with the kernels.
  1, 2  the two kernels against fp64 F.conv2d restatements. Bound: max |err| < 5e-5 max |ref|, the bound the project
        holds rdx_hgemm_x3 and the strided-conv GEMM to. Power: on the reference alone, a single bf16 product
        (bf16(x) . bf16(w) summed in fp64) misses that bound at least tenfold, so a kernel that drops the lo planes
        fails. The output buffer carries a sentinel row past its end.
  3     sinc_x3.forward against the same encoder deep-copied to fp64 (SincConv included, the reference's forward
        restated over the copy's modules), BN statistics randomised. Bound: the project's N2, 1e-3 max |ref| (eleven x3
        convolutions at 5e-5 sum to well under it). The measured maxima and the fp32 module path's error on the same
        inputs (recorded, not asserted) go to profiles/sinc_x3_errors.json.
  4     dispatch: which calls take the new path, and that every other call gives the bits RADHIP_X3_SINC=0 gives.
  5     the cached planes follow the weights.
  6     the full DualStreamSEMamba (2-layer WavLM-Large geometry) through radhip.infer._scores(amp="x3"), both streams
        on their x3 kernels: logits within the project's 1e-3 of the fp64 oracle at |logit| about 10, and bit-equal from
        pass to pass.
Block 0's kernel walks strips of 42 pool windows = 126 positions (csrc/sconv_x3.hip BX_J); rdx_x3_sconv_fwd tiles a row
by 128 positions.
"""
import copy
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
KERNEL_BOUND = 5e-5
STACK_BOUND = 1e-3
POWER = 1e-2          # what a weight change has to move the fp64 output by, relative to max |ref|
STRIP = 126           # positions per strip of rdx_x3_b0x_fwd
SENTINEL = -12345.0
_CACHE = {}


def _bf16(t):
    return t.float().to(torch.bfloat16).double()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bn_params(C, g):
    """(conv bias, running mean, running var, gamma, beta), fp64, BN far from the identity."""
    return (0.3 * torch.randn(C, generator=g, dtype=torch.float64), 0.3 * torch.randn(C, generator=g, dtype=torch.float64),
            0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64),
            0.5 + torch.rand(C, generator=g, dtype=torch.float64), 0.3 * torch.randn(C, generator=g, dtype=torch.float64))


def _bn_selu(c, bn, eps=1e-5):
    cb, mean, var, gamma, beta = (t.view(1, -1, 1, 1) for t in bn)
    return F.selu((c + cb - mean) * (gamma / torch.sqrt(var + eps)) + beta)


def _bn_table(bn, eps=1e-5):
    cb, mean, var, gamma, beta = bn
    return torch.stack([cb, mean, gamma / torch.sqrt(var + eps), beta]).float().contiguous()


def _planes_tap_major(w):
    from radhip import sinc_x3, wavlm_x3
    return wavlm_x3.planes(sinc_x3.tap_major(w.float()).to(DEV))


# ------------------------------------------------------------------------------- 1. rdx_x3_sconv_fwd ----------
def sconv_case(ci, co, kh, ph, W, with_bn, seed):
    """Inputs and fp64 references of one convolution: x NCHW N(0, 1), w N(0, 1 / K)."""
    g = _gen(seed)
    N, H = 2, 3
    x = torch.randn(N, ci, H, W, generator=g, dtype=torch.float64).float().double()
    K = kh * 3 * ci
    w = (torch.randn(co, ci, kh, 3, generator=g, dtype=torch.float64) / K ** 0.5).float().double()
    bn = _bn_params(co, g) if with_bn else None
    bn = tuple(t.float().double() for t in bn) if bn else None
    post = (lambda c: _bn_selu(c, bn)) if with_bn else (lambda c: c)
    ref = post(F.conv2d(x, w, padding=(ph, 1)))
    single = post(F.conv2d(_bf16(x), _bf16(w), padding=(ph, 1)))
    return x, w, bn, ref, single


SCONV_CFGS = [(32, 32, 2, 1), (32, 32, 2, 0), (32, 64, 2, 1), (64, 64, 2, 0), (64, 64, 2, 1), (32, 64, 1, 0),
              (64, 64, 1, 0)]


@pytest.mark.parametrize("ci,co,kh,ph", SCONV_CFGS)
def test_sconv_x3_vs_fp64_conv2d(ci, co, kh, ph):
    from radhip._lib import lib
    for W in (3, 130, 257):
        for with_bn in (False, True):
            x, w, bn, ref, single = sconv_case(ci, co, kh, ph, W, with_bn, seed=1000 + W + ci + 7 * co + kh + ph)
            top = float(ref.abs().max())
            miss = float((single - ref).abs().max())
            assert miss >= 10 * KERNEL_BOUND * top, ("a single bf16 product would pass", miss / top)
            N, _, H, _ = x.shape
            Ho = ref.shape[2]
            xd = x.float().permute(0, 2, 3, 1).contiguous().to(DEV)
            wh, wl = _planes_tap_major(w)
            tbl = _bn_table(bn).to(DEV) if with_bn else None
            buf = torch.full((N * Ho + 1, W, co), SENTINEL, device=DEV, dtype=torch.float32)
            rc = lib().rdx_x3_sconv_fwd(xd.data_ptr(), wh.data_ptr(), wl.data_ptr(),
                                        tbl.data_ptr() if tbl is not None else None, buf.data_ptr(), N, H, W, ci, co,
                                        kh, ph, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
            torch.cuda.synchronize()
            got = buf[:N * Ho].view(N, Ho, W, co).permute(0, 3, 1, 2).double().cpu()
            err = float((got - ref).abs().max())
            print(f"[sconv_x3 {ci}->{co} kh {kh} ph {ph} W {W} bn {with_bn}] max|ref| {top:.3f} err {err / top:.3e} "
                  f"single product {miss / top:.3e}")
            assert bool((buf[N * Ho] == SENTINEL).all()), "wrote past the end"
            assert err < KERNEL_BOUND * top, (W, with_bn, err / top)


# --------------------------------------------------------------------------------- 2. rdx_x3_b0x_fwd ----------
def b0_case(H, W, with_fbn, seed):
    g = _gen(seed)
    N = 2
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x = r(N, 1, H, W).float().double()
    fbn = None
    if with_fbn:
        fbn = torch.stack([0.5 + torch.rand((), generator=g, dtype=torch.float64), 0.3 * r(())]).float().double()
    w1 = (r(32, 1, 2, 3) / 6 ** 0.5).float().double()
    wd = (r(32, 1, 1, 3) / 3 ** 0.5).float().double()
    w2 = (r(32, 32, 2, 3) / 192 ** 0.5).float().double()
    bn = tuple(t.float().double() for t in _bn_params(32, g))
    bias = (0.3 * r(32)).float().double()
    xa = F.selu(x * fbn[0] + fbn[1]) if with_fbn else x
    out1 = _bn_selu(F.conv2d(xa, w1, padding=(1, 1)), bn)
    idn = F.conv2d(xa, wd, padding=(0, 1)) + bias.view(1, -1, 1, 1)
    ref = F.max_pool2d(F.conv2d(out1, w2, padding=(0, 1)) + idn, (1, 3))
    single = F.max_pool2d(F.conv2d(_bf16(out1), _bf16(w2), padding=(0, 1)) + idn, (1, 3))
    return dict(x=x, fbn=fbn, w1=w1, wd=wd, w2=w2, bn=bn, bias=bias, ref=ref, single=single)


B0_WIDTHS = (3, 5, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 48)


@pytest.mark.parametrize("H", [1, 23])
def test_b0x_x3_vs_fp64_block0(H):
    from radhip._lib import lib
    for W in B0_WIDTHS:
        for with_fbn in (True, False):
            c = b0_case(H, W, with_fbn, seed=2000 + 31 * H + W + int(with_fbn))
            ref, top = c["ref"], float(c["ref"].abs().max())
            miss = float((c["single"] - ref).abs().max())
            assert miss >= 10 * KERNEL_BOUND * top, ("a single bf16 product would pass", miss / top)
            N, Wo = 2, W // 3
            f = lambda t: t.float().contiguous().to(DEV)   # noqa: E731
            x, w1, wd, bias = f(c["x"].view(N, H, W)), f(c["w1"].view(32, 6)), f(c["wd"].view(32, 3)), f(c["bias"])
            tbl = _bn_table(c["bn"]).to(DEV)
            wh, wl = _planes_tap_major(c["w2"])
            fbn = f(c["fbn"]) if with_fbn else None
            buf = torch.full((N * H + 1, Wo, 32), SENTINEL, device=DEV, dtype=torch.float32)
            rc = lib().rdx_x3_b0x_fwd(x.data_ptr(), fbn.data_ptr() if fbn is not None else None, w1.data_ptr(),
                                      wd.data_ptr(), tbl.data_ptr(), wh.data_ptr(), wl.data_ptr(), bias.data_ptr(),
                                      buf.data_ptr(), N, H, W, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
            torch.cuda.synchronize()
            got = buf[:N * H].view(N, H, Wo, 32).permute(0, 3, 1, 2).double().cpu()
            err = float((got - ref).abs().max())
            print(f"[b0x_x3 H {H} W {W} fbn {with_fbn}] max|ref| {top:.3f} err {err / top:.3e} "
                  f"single product {miss / top:.3e}")
            assert bool((buf[N * H] == SENTINEL).all()), "wrote past the end"
            assert err < KERNEL_BOUND * top, (W, with_fbn, err / top)


# ------------------------------------------------------------------------------------ 3. whole stack ----------
def _encoder(seed=7):
    """A SincNetEncoder in eval mode whose BatchNorms are far from the identity."""
    from radhip.sinc import SincNetEncoder
    torch.manual_seed(seed)
    enc = SincNetEncoder()
    g = _gen(seed + 1)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                _, mean, var, gamma, beta = _bn_params(C, g)
                m.running_mean.copy_(mean)
                m.running_var.copy_(var)
                m.weight.copy_(gamma)
                m.bias.copy_(beta)
    return enc.to(DEV).eval()


def _wave(B, L, seed=21):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.clip(0.1 * rng.standard_normal((B, L)), -1, 1).astype(np.float32))


def _ref64(enc, x):
    """The reference's SincNetEncoder.forward (src/models/DualStreamSEMamba.py:238-270) over a fp64 CPU copy of
    enc's present state: conv1d -> |.| -> 3x3 max pool -> first_bn -> SELU -> the residual blocks -> max |.| over
    the filter rows -> [B, T', 64]."""
    e = copy.deepcopy(enc)
    e.__dict__.pop("_x3w", None)
    e = e.cpu().double().eval()
    with torch.no_grad():
        c = e.conv_time(x.double().cpu().unsqueeze(1))
        h = F.max_pool2d(torch.abs(c.unsqueeze(1)), (3, 3))
        h = e.encoder(e.selu(e.first_bn(h)))
        return torch.max(torch.abs(h), dim=2)[0].transpose(1, 2).contiguous()


def _x3(enc, x):
    from radhip import sinc_x3, wavlm_x3
    assert os.environ.get("RADHIP_X3_SINC", "1") != "0"
    with torch.no_grad(), wavlm_x3.scoring():
        assert sinc_x3.eligible(enc, x, False)
        return enc(x).double().cpu()


def _stack_inputs(tag):
    if tag not in _CACHE:
        B, L = {"short": (2, 2400), "full": (1, 64600)}[tag]
        enc = _CACHE.setdefault("enc", _encoder())
        x = _wave(B, L).to(DEV)
        _CACHE[tag] = (enc, x, _ref64(enc, x))
    return _CACHE[tag]


@pytest.mark.parametrize("tag", ["short", "full"])
def test_stack_vs_fp64_encoder(tag):
    enc, x, ref = _stack_inputs(tag)
    got = _x3(enc, x)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top = float(ref.abs().max())
    err = float((got - ref).abs().max())
    with torch.no_grad():
        e32 = float((enc(x).double().cpu() - ref).abs().max())
    print(f"[sinc_x3 stack {tag}] max|ref| {top:.4f}: x3 err {err / top:.3e}, fp32 module path {e32 / top:.3e}")
    path = os.path.join(PROFILES, "sinc_x3_errors.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[tag] = {"shape": list(x.shape), "ref_absmax": top, "x3_max_abs_err": err, "x3_rel": err / top,
                "fp32_module_max_abs_err": e32, "fp32_module_rel": e32 / top, "bound_rel": STACK_BOUND}
    os.makedirs(PROFILES, exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    assert err <= STACK_BOUND * top, err / top


# --------------------------------------------------------------------------------------- 4. dispatch ----------
def test_dispatch(monkeypatch):
    from radhip import sinc_x3, wavlm_x3
    enc, x, _ = _stack_inputs("short")
    calls = []
    real = sinc_x3.forward
    monkeypatch.setattr(sinc_x3, "forward", lambda e, t: (calls.append(1), real(e, t))[1])

    def run(e, t, env=None, grad=False, autocast=False, freq_aug=False):
        for k in ("RADHIP_X3_SINC", "RADHIP_X3"):
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        np.random.seed(5)
        random.seed(5)
        with torch.set_grad_enabled(grad), wavlm_x3.scoring(), \
                torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return e(t, freq_aug=freq_aug).detach().clone()

    monkeypatch.delenv("RADHIP_X3_SINC", raising=False)
    enc.__dict__.pop("_x3w", None)
    y = run(enc, x)
    assert len(calls) == 1 and "_x3w" in enc.__dict__, "the x3 SincNet stream did not run"
    off = run(enc, x, env={"RADHIP_X3_SINC": "0"})
    assert len(calls) == 1
    assert torch.equal(run(enc, x, env={"RADHIP_X3_SINC": "1"}), y) and len(calls) == 2
    del calls[1:]
    assert not torch.equal(y, off), "the new path returned the module path's bits: did it run?"
    trn = copy.deepcopy(enc).train()
    cases = {
        "RADHIP_X3=0": (enc, x, dict(env={"RADHIP_X3": "0"})),
        "training mode": (trn, x, {}),
        "grad enabled": (enc, x, dict(grad=True)),
        "bf16 autocast": (enc, x, dict(autocast=True)),
        "freq_aug": (enc, x, dict(freq_aug=True)),
        "L = 2300": (enc, _wave(2, 2300).to(DEV), {}),
    }
    def outcome(e, t, may_raise=False, **kw):
        try:
            return run(copy.deepcopy(e) if e is trn else e, t, **kw)
        except RuntimeError as err:
            if not may_raise:
                raise
            return str(err)

    for name, (e, t, kw) in cases.items():
        a = outcome(e, t, may_raise=name == "L = 2300", **kw)
        kw0 = dict(kw)
        kw0["env"] = dict(kw.get("env") or {}, RADHIP_X3_SINC="0")
        b = outcome(e, t, may_raise=name == "L = 2300", **kw0)
        assert len(calls) == 1, f"{name}: took the x3 path"
        if name == "L = 2300":
            # the last block is 2 positions wide: MaxPool2d((1, 3)) has no output there, and the module path
            # refuses it (rdx_res_tail_fwd, W >= 3) whatever RADHIP_X3_SINC says; the stream must not take it over
            assert isinstance(a, str) and a == b, (a, b)
            continue
        assert torch.is_tensor(a) and torch.is_tensor(b), (name, a, b)
        assert torch.equal(a, b), f"{name}: differs from the RADHIP_X3_SINC=0 output"
    # outside scoring() nothing changes either
    with torch.no_grad():
        assert torch.equal(enc(x), off) and len(calls) == 1


# --------------------------------------------------------------------------- 5. cache follows weights ----------
def _tracks(enc, x, before, what):
    ref = _ref64(enc, x)
    got = _x3(enc, x)
    top = float(ref.abs().max())
    moved, err = float((ref - before).abs().max()), float((got - ref).abs().max())
    print(f"[sinc_x3 {what}] reference moved {moved / top:.3e}, x3 err {err / top:.3e}")
    assert moved >= POWER * top, (what, moved / top)
    assert err <= STACK_BOUND * top, (what, err / top)
    return ref


def test_cache_follows_the_weights():
    from radhip import wavlm_x3
    from radhip.optim import AdamW
    base, x, ref = _stack_inputs("short")
    enc = copy.deepcopy(base)
    enc.__dict__.pop("_x3w", None)
    _x3(enc, x)
    first = enc.__dict__["_x3w"][1]
    _x3(enc, x)
    assert enc.__dict__["_x3w"][1] is first, "unchanged weights rebuilt the planes"
    g = _gen(77)
    with torch.no_grad():   # a version bump, no invalidate()
        bn = enc.encoder[3][0].bn2
        bn.running_mean.copy_(bn.running_mean + 1.0)
    ref = _tracks(enc, x, ref, "running_mean copy_")
    w = enc.encoder[4][0].conv2.weight   # behind the version counter, then invalidate()
    w.data.add_(0.05 * torch.randn(w.shape, generator=g).to(DEV))
    wavlm_x3.invalidate()
    ref = _tracks(enc, x, ref, "conv2.weight p.data + invalidate")
    ps = [p for p in enc.parameters()]
    opt = AdamW(ps, lr=2e-2, weight_decay=0.0)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    _tracks(enc, x, ref, "radhip.optim.AdamW step")


def test_drop_removes_the_encoder_planes(golden):
    """wavlm_x3.drop(model) on a full DualStreamSEMamba (reduced-width WavLM) pops the SincNet planes too."""
    import models.DualStreamSEMamba as DS
    from radhip import wavlm_x3

    class Args:
        emb_size, num_encoders, d_state, sinc_channels, wavlm_freeze_layers = 144, 2, 16, 70, -1
        wavlm_config = json.loads(str(golden("model_tiny.npz")["wavlm_config"]))
    torch.manual_seed(0)
    m = DS.Model(Args(), device=torch.device(DEV)).to(DEV).eval()
    _x3(m.sinc_stream, _wave(1, 2400).to(DEV))
    assert "_x3w" in m.sinc_stream.__dict__
    wavlm_x3.drop(m)
    assert "_x3w" not in m.sinc_stream.__dict__


# ------------------------------------------------------------------------------------- 6. full model ----------
def test_full_model_scores_through_both_x3_streams(monkeypatch):
    """The place the stream is for: the whole model under `_scores(..., "x3")`. With the SincNet kernels beside the
    WavLM stream's batched CNN GEMM the logits moved from pass to pass by up to 4e-3; the model runs the two x3
    streams in order, and this test holds repeated passes to the same bits and to the oracle."""
    from radhip.infer import _scores
    from test_x3_gpu import _model_and_oracle
    monkeypatch.delenv("RADHIP_X3_SINC", raising=False)
    monkeypatch.delenv("RADHIP_X3", raising=False)
    m, o = _model_and_oracle("reference", depth=2, targets=[])
    x = _wave(3, 64600, seed=23).to(DEV)
    with torch.no_grad():
        ref = o(x.double())[1][:, 1]
        s = 10.0 / float(ref.abs().max())
        for mod in (m, o):
            mod.classifier.weight.mul_(s)
            mod.classifier.bias.mul_(s)
        ref = o(x.double())[1][:, 1]
        passes = [_scores(m, x, None, "x3").double() for _ in range(4)]
        assert "_x3w" in m.sinc_stream.__dict__ and "_x3w" in m.wavlm_stream._core().__dict__, "an x3 stream did not run"
        monkeypatch.setenv("RADHIP_X3_SINC", "0")
        off = _scores(m, x, None, "x3").double()
    err, err_off = float((passes[0] - ref).abs().max()), float((off - ref).abs().max())
    print(f"[sinc_x3 full model] |logit| max {float(ref.abs().max()):.3f}: x3 + x3 SincNet err {err:.3e}, "
          f"x3 + module SincNet {err_off:.3e}")
    for p in passes[1:]:
        assert torch.equal(p, passes[0]), (passes[0], p)
    assert err < 1e-3, err

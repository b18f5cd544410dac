"""The four row kernels of the fused WavLM layer (csrc/wavlm_layer.hip: LN1 forward, add + LN forward, LN backward,
LN1 backward) at every launch geometry their policy can select, against a float64 restatement written here.

A geometry is (waves per row, rows per workgroup). (1, 4) is the one-wave-per-row form: a lane sums its 16 values in
order and the wave adds the lanes, the reduction order these kernels had before rows were shared between waves. It is
not their earlier arithmetic bit for bit: a lane now holds 4 values of each of 4 chunks, not 16 contiguous ones, so its
partial sums are over other elements, and no mapping with coalesced lanes can give the old partial sums. It is built
from the same new helpers as the other forms, so every form, (1, 4) included, is first held to float64 on its own (A).
The geometries under test are whatever rdx_wl_rows_policy answers, per kernel, for the training shapes (M = 1608,
6432) and the shapes below, with and without LoRA (LoRA active: (1, 4) alone).

Shapes: M = 1 (one live row, dead rows beside it), 5 (dead rows in the last workgroup: they must reach the barriers of
the live rows), 204 = 201 + 3 and 205 (many workgroups, the last one full / one row in). Dropout p = 0 and 0.1 with a
fixed device seed; dres / ddrop / sg present and null; row strides above E; LoRA on and off; bf16 and fp16 storage.

Assertions:
 (A) every geometry, each output: max |kernel - float64| <= an absolute bound worked out from the number formats and the
     operation counts, never from a kernel's result (u = 2^-24, eps32 = 2 u, ulp16 / ulp32 = one ulp of the type at the
     reference's largest magnitude):
       fp32 elementwise sums (h2, hout)    2 ulp32 (a product and a sum, or one fma)
       mean                                16 eps32 max_rows(sum |v| / E): at most 22 fp32 additions deep (16 in a lane,
                                           6 across the wave, 1-3 across waves), error <= depth u sum |v|
       rstd                                16 eps32 max rstd: the same depth on sum d^2 (no cancellation), halved by the
                                           square root, plus the rounding of d, d^2, the rsqrt and the mean's error
       16-bit LayerNorm outputs (x, x1)    ulp16: half an ulp of rounding, the fp32 error before it is far below the rest
       gate                                6 u max(Sa + Sb) + 32 u, S = sum |w| |x1| + |b| of the 4 gate rows: z is <= 24
                                           additions deep, |d gate / d z| <= 1/4, sigmoid and the last 3 operations 32 u
       a (LoRA down-projection)            16 u max sum |A| |x| + ulp16: 8 packed dots in a lane, 6 levels across
       dh (LN backward)                    32 u max_rows rstd (S1 + max|xh| S2) + 8 ulp32, S1 = sum |g| / E,
                                           S2 = sum |g xh| / E: the two row sums at that depth, the elementwise rest
       dh (LN1 backward)                   that, plus P (16 u max D + W8 (0.2 max|dg| 24 u max S + 16 u max |dz|)):
                                           D the absolute terms of dx1 + gate + LoRA gradients, W8 = max_d sum_j |wg|,
                                           0.2 bounds |d dz / d z|, P = max rstd max gamma (2 + max |xh|) carries an
                                           elementwise error of dx through the LayerNorm backward; plus, only where an
                                           element of the recomputed x1 lies within fp32 error of a 16-bit rounding tie
                                           (counted per row from float64), the effect of that many one-ulp16 changes
                                           of x1 on that row
       ddrop, xd                           the fp32 bound times 1 / (1 - p), plus ulp16
     and the dropout keep pattern of every output that shows one (forward residual with delta = 1; the zeros of ddrop
     and xd) equals the pattern of the stand-alone mask kernel (ops.dropout_mask); the LoRA dropouts of `a` show in no
     pattern, they are in its float64 restatement through the same mask;
 (a) keep patterns and every purely elementwise output are bit-identical between each geometry and (1, 4);
 (b) for each output but the row mean, max |kernel - float64| <= 2 x the (1, 4) form's on the same inputs + one ulp of
     the output dtype at the output's largest magnitude. The row mean is held to (A) alone: its terms cancel, so
     ulp(|mean|) is far below the rounding error of any fp32 summation order (relative to sum |v|), and a single row's
     (1, 4) result can be near exact by chance, which makes 2 e1 + ulp(|mean|) a bound no other order can keep;
 (c) two runs are bit-identical.
The 16-bit rounding of x1 sits between the LayerNorm and the gate / LoRA parts, so the float64 restatement of those
parts starts from the x1 the kernel under test stored (forward, x1 itself being held to (A)) or from x1 recomputed from
the mean / rstd inputs (backward, elementwise and therefore the same in every geometry).
Every measured error and bound goes to profiles/wl_rows_errors.json.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from radhip import ops
from radhip._lib import check
from radhip.ops import _p

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, H, R = 1024, 16, 8
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
RECORD = os.path.join(PROFILES, "wl_rows_errors.json")
REF_GEO = (1, 4)
MS = (1, 5, 204, 205)
EPS = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
K_LN1_FWD, K_ADD_LN, K_LN_BWD, K_LN1_BWD = 0, 1, 2, 3


def record(key, obj):
    os.makedirs(PROFILES, exist_ok=True)
    cur = {}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            cur = json.load(f)
    cur[key] = obj
    cur["_format"] = ("per case and output: {geometry 'WxR': [max error against float64, the absolute bound (A), the "
                      "relative bound (b) = 2 x the 1x4 form's error + one ulp of the output dtype (null: 1x4, mean)]}")
    with open(RECORD, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(cur[k], sort_keys=True)}" for k in sorted(cur))
                + "\n}\n")


def geometries(L, kernel, lora):
    """Every geometry the policy can select for this kernel, besides the one-wave reference form."""
    out = set()
    w, r = ctypes.c_int(), ctypes.c_int()
    for M in MS + (1608, 6432):
        check(L.rdx_wl_rows_policy(kernel, M, int(lora), ctypes.byref(w), ctypes.byref(r)), "rows_policy")
        out.add((w.value, r.value))
    out.discard(REF_GEO)
    return sorted(out)


class forced:
    def __init__(self, L, geo):
        self.L, self.geo = L, geo

    def __enter__(self):
        check(self.L.rdx_wl_rows_override(*self.geo), "rows_override")

    def __exit__(self, *exc):
        check(self.L.rdx_wl_rows_override(0, 0), "rows_override")


def ulp(dtype, ref):
    mag = float(ref.abs().max())
    return EPS[dtype] * 2.0 ** math.floor(math.log2(mag)) if mag > 0 else 0.0


def err(out, ref):
    return float((out.double() - ref).abs().max())


def rnd(gen, *shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=gen, device=DEV) * scale).to(dtype)


def inv_keep(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def scale_of(seed, salt, p, M):
    """The dropout factor of every element of an [M, E] tensor, float64 (mask from the stand-alone mask kernel)."""
    if p == 0:
        return torch.ones(M, E, device=DEV, dtype=torch.float64)
    return ops.dropout_mask(seed, salt, p, (M, E)).double() * inv_keep(p)


def ln_stats64(h):
    mean = h.mean(1, keepdim=True)
    var = ((h - mean) ** 2).mean(1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + 1e-5)


def gate64(x1, wg, bg, gc):
    """ga, gb [M, H] from x1 [M, E] float64."""
    z = x1.view(-1, H, 64) @ wg.double().t() + bg.double()
    return torch.sigmoid(z[..., :4].sum(-1)), torch.sigmoid(z[..., 4:].sum(-1))


def ln_bwd64(dx, h, mean, rstd, gm):
    xh = (h - mean) * rstd
    g = dx * gm
    return rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))


U = 2.0 ** -24
EPS32 = 2.0 ** -23


def near_tie(y, hd, tol):
    """Elements of y (float64) within tol of a rounding tie of the 16-bit type hd."""
    r = y.float().to(hd).double()
    e = torch.floor(torch.log2(y.abs().clamp_min(1e-300)))
    e = e.clamp_min(-14.0) if hd == torch.float16 else e
    half = torch.exp2(e - (10 if hd == torch.float16 else 7)) / 2
    return ((y - r).abs() - half).abs() < tol


def compare(key, runs, refs, dtypes, absb, exact=(), patterns=None, norel=()):
    """runs: {geo: {name: tensor}}; refs: {geo: {name: float64}} (the restatement may start from the run's own x1);
    absb: {geo: {name: bound}} for (A); patterns: {name: (expected nonzero pattern, elements exempt from it)}.
    Asserts (A), (a), (b) and records the errors."""
    base = runs[REF_GEO]
    rec = {}
    failures = []
    for name in base:
        e1 = err(base[name], refs[REF_GEO][name])
        row = {}
        for geo, outs in runs.items():
            e = e1 if geo == REF_GEO else err(outs[name], refs[geo][name])
            ab = absb[geo][name]
            if torch.is_tensor(ab):     # a bound per row: every element within its row's, the tightest recorded
                inside = bool(((outs[name].double() - refs[geo][name]).abs() <= ab).all())
                ab = float(ab.min())
            else:
                inside = e <= ab
            rel = None
            if not inside:
                failures.append((name, geo, e, "absolute bound", ab))
            if patterns and name in patterns:
                want, exempt = patterns[name]
                if not torch.equal((outs[name] != 0) | exempt, want | exempt):
                    failures.append((name, geo, "keep pattern differs from the mask kernel's"))
            if geo != REF_GEO:
                if name not in norel:
                    rel = 2.0 * e1 + ulp(dtypes[name], refs[geo][name])
                    if not e <= rel:
                        failures.append((name, geo, e, "relative bound", rel))
                if name in exact and not torch.equal(outs[name], base[name]):
                    failures.append((name, geo, "not bit-identical to the one-wave form"))
                if patterns and name in patterns and not torch.equal(outs[name] != 0, base[name] != 0):
                    failures.append((name, geo, "keep pattern differs from the one-wave form"))
            row[f"{geo[0]}x{geo[1]}"] = [e, ab, rel]
        rec[name] = row
    print(key, json.dumps(rec, sort_keys=True))
    record(key, rec)
    assert not failures, failures


def fwd_bounds(hd, hr, ref):
    """(A) for the outputs both forward kernels share; hr: the float64 LayerNorm input, ref: its restatement."""
    return {"keep": 0.0, "mean": 16 * EPS32 * float(hr.abs().mean(1).max()), "rstd": 16 * EPS32 * float(ref["rstd"].max()),
            "res": 2 * ulp(torch.float32, hr), "ln": ulp(hd, ref["ln"])}


def ln_bwd_bound(dx, h, mean, rstd, gm, extra):
    """(A) for dh = rstd (g - mean g - xh mean(g xh)) + extra terms (float64 inputs)."""
    xh = (h - mean) * rstd
    g = dx * gm
    s = rstd[:, 0] * (g.abs().mean(1) + xh.abs().max(1).values * (g * xh).abs().mean(1))
    return 32 * U * float(s.max()) + 8 * ulp(torch.float32, extra)


def run_geos(L, kernel, lora, fn):
    """fn() -> {name: tensor} under every geometry; (c): a second run of each is bit-identical."""
    runs = {}
    for geo in [REF_GEO] + geometries(L, kernel, lora):
        with forced(L, geo):
            a, b = fn(), fn()
        torch.cuda.synchronize()
        for name in a:
            assert torch.equal(a[name], b[name]), (geo, name, "two runs differ")
        runs[geo] = a
    return runs


def params(M, hd, seed):
    g = torch.Generator(device=DEV).manual_seed(1000 * seed + M)
    d = dict(gm=torch.rand(E, generator=g, device=DEV) + 0.5, bt=rnd(g, E, scale=0.1), wg=rnd(g, 8, 64, scale=0.1),
             bg=rnd(g, 8, scale=0.1), gc=torch.rand(H, generator=g, device=DEV),
             aq=rnd(g, R, E, scale=0.05, dtype=hd), av=rnd(g, R, E, scale=0.05, dtype=hd),
             seed=torch.tensor([1234 + M], dtype=torch.int64, device=DEV))
    return g, d


@pytest.mark.parametrize("hd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M", MS)
def test_add_ln_fwd(M, p, hd):
    L = ops._L(hd)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g, c = params(M, hd, 1)
    h = rnd(g, M, E)
    for tag, delta in (("rand", rnd(g, M, E, dtype=hd)), ("ones", torch.ones(M, E, device=DEV, dtype=hd))):
        def fn():
            h2, x = torch.empty(M, E, device=DEV), torch.empty(M, E, device=DEV, dtype=hd)
            mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
            check(L.rdx_wl_add_ln_fwd(_p(h), _p(delta), _p(c["seed"]) if p else None, 3, p, _p(h2), _p(c["gm"]),
                                      _p(c["bt"]), 1e-5, _p(x), _p(mean), _p(rstd), M, E, st), "add_ln")
            return {"h2": h2, "x": x, "mean": mean, "rstd": rstd, "keep": (h2 != h).float()}
        runs = run_geos(L, K_ADD_LN, False, fn)
        s = scale_of(c["seed"], 3, p, M)
        h2r = h.double() + delta.double() * s
        mean, rstd = ln_stats64(h2r)
        ref = {"h2": h2r, "x": (h2r - mean) * rstd * c["gm"].double() + c["bt"].double(), "mean": mean[:, 0],
               "rstd": rstd[:, 0], "keep": (s != 0).double()}
        if tag == "ones":
            for o in runs.values():
                assert torch.equal(o["keep"].double(), ref["keep"])   # the pattern the mask kernel gives
        fb = fwd_bounds(hd, h2r, {"rstd": rstd, "ln": ref["x"]})
        ab = {"h2": fb["res"], "x": fb["ln"], "mean": fb["mean"], "rstd": fb["rstd"], "keep": 0.0}
        compare(f"add_ln_fwd[M={M},p={p},{hd},{tag}]", runs, {k: ref for k in runs},
                {"h2": torch.float32, "x": hd, "mean": torch.float32, "rstd": torch.float32, "keep": torch.float32},
                {k: ab for k in runs}, exact=("h2", "keep"), norel=("mean",))


@pytest.mark.parametrize("hd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("lora", [False, True], ids=["nolora", "lora"])
def test_ln1_fwd(lora, M, p, hd):
    L = ops._L(hd)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g, c = params(M, hd, 2)
    h = rnd(g, M, E)
    ldx = E + 16 + 8
    sd = _p(c["seed"]) if p else None
    aq, av = (_p(c["aq"]), _p(c["av"])) if lora else (None, None)
    for tag, delta in (("plain", None), ("res", rnd(g, M, E, dtype=hd)),
                       ("res_ones", torch.ones(M, E, device=DEV, dtype=hd))):
        def fn():
            x1 = torch.zeros(M, ldx, device=DEV, dtype=hd)
            gate, hout = torch.empty(M, H, device=DEV), torch.empty(M, E, device=DEV)
            mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
            if delta is None:
                check(L.rdx_wl_ln1_fwd(_p(h), _p(c["gm"]), _p(c["bt"]), 1e-5, _p(c["wg"]), _p(c["bg"]), _p(c["gc"]),
                                       aq, av, R, sd, 11, 12, p, _p(x1), ldx, _p(gate), _p(mean), _p(rstd), M, E, st),
                      "ln1_fwd")
                hout.copy_(h)
            else:
                check(L.rdx_wl_res_ln1_fwd(_p(h), _p(delta), 5, p, _p(hout), _p(c["gm"]), _p(c["bt"]), 1e-5,
                                           _p(c["wg"]), _p(c["bg"]), _p(c["gc"]), aq, av, R, sd, 11, 12, p, _p(x1),
                                           ldx, _p(gate), _p(mean), _p(rstd), M, E, st), "res_ln1_fwd")
            o = {"hout": hout, "x1": x1[:, :E].contiguous(), "gate": gate, "mean": mean, "rstd": rstd,
                 "keep": (hout != h).float()}
            if lora:
                o["a"] = x1[:, E:E + 16].contiguous()
            assert not x1[:, E + (16 if lora else 0):].any()     # nothing written past the row's columns
            return o
        runs = run_geos(L, K_LN1_FWD, lora, fn)
        s = scale_of(c["seed"], 5, p, M)
        hr = h.double() if delta is None else h.double() + delta.double() * s
        mean, rstd = ln_stats64(hr)
        refs, abs_ = {}, {}
        x1r = (hr - mean) * rstd * c["gm"].double() + c["bt"].double()
        fb = fwd_bounds(hd, hr, {"rstd": rstd, "ln": x1r})
        wabs, babs = c["wg"].double().abs(), c["bg"].double().abs()
        for geo, o in runs.items():
            x1k = o["x1"].double()
            ga, gb = gate64(x1k, c["wg"], c["bg"], c["gc"])
            ref = {"hout": hr, "x1": x1r, "mean": mean[:, 0],
                   "rstd": rstd[:, 0], "gate": ga * (gb * c["gc"].double() - 1.0) + 2.0,
                   "keep": (hr != h.double()).double()}
            sz = (x1k.abs().view(-1, H, 64) @ wabs.t() + babs).sum(-1)       # Sa + Sb per head
            ab = {"hout": fb["res"], "x1": fb["ln"], "mean": fb["mean"], "rstd": fb["rstd"], "keep": 0.0,
                  "gate": 6 * U * float(sz.max()) + 32 * U}
            if lora:
                xs = [(o["x1"].float() * scale_of(c["seed"], salt, p, M).float()).to(hd).double() for salt in (11, 12)]
                ref["a"] = torch.cat([xs[0] @ c["aq"].double().t(), xs[1] @ c["av"].double().t()], 1)
                sa = torch.cat([xs[0].abs() @ c["aq"].double().abs().t(), xs[1].abs() @ c["av"].double().abs().t()], 1)
                ab["a"] = 16 * U * float(sa.max()) + ulp(hd, ref["a"])
            refs[geo], abs_[geo] = ref, ab
            if tag == "res_ones":
                assert torch.equal(o["keep"].double(), (s != 0).double())   # the pattern the mask kernel gives
        dt = {"hout": torch.float32, "x1": hd, "gate": torch.float32, "mean": torch.float32, "rstd": torch.float32,
              "keep": torch.float32, "a": hd}
        compare(f"ln1_fwd[{'lora' if lora else 'nolora'},M={M},p={p},{hd},{tag}]", runs, refs, dt, abs_,
                exact=("hout", "keep"), norel=("mean",))


@pytest.mark.parametrize("hd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M", MS)
def test_ln_bwd(M, p, hd):
    L = ops._L(hd)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g, c = params(M, hd, 3)
    h, dres = rnd(g, M, E), rnd(g, M, E)
    m64, r64 = ln_stats64(h.double())
    mean, rstd = m64[:, 0].float().contiguous(), r64[:, 0].float().contiguous()
    for ldd in (E, E + 24):
        dx = rnd(g, M, ldd, dtype=hd)
        for with_res in (True, False):
            for with_drop in (True, False):
                def fn():
                    dh = torch.empty(M, E, device=DEV)
                    dd = torch.zeros(M, E, device=DEV, dtype=hd)
                    check(L.rdx_wl_ln_bwd(_p(dx), ldd, _p(h), _p(mean), _p(rstd), _p(c["gm"]),
                                          _p(dres) if with_res else None, _p(dh), _p(c["seed"]) if p else None, 3, p,
                                          _p(dd) if with_drop else None, M, E, st), "ln_bwd")
                    return {"dh": dh, "ddrop": dd} if with_drop else {"dh": dh}
                runs = run_geos(L, K_LN_BWD, False, fn)
                dhr = ln_bwd64(dx[:, :E].double(), h.double(), mean.double()[:, None], rstd.double()[:, None],
                               c["gm"].double())
                if with_res:
                    dhr = dhr + dres.double()
                sc = scale_of(c["seed"], 3, p, M)
                ref = {"dh": dhr, "ddrop": dhr * sc}
                bdh = ln_bwd_bound(dx[:, :E].double(), h.double(), mean.double()[:, None], rstd.double()[:, None],
                                   c["gm"].double(), torch.cat([dhr, dres.double()]))
                ab = {"dh": bdh, "ddrop": bdh * inv_keep(p) + ulp(hd, ref["ddrop"])}
                compare(f"ln_bwd[M={M},p={p},{hd},ldd={ldd},dres={with_res},ddrop={with_drop}]", runs,
                        {k: ref for k in runs}, {"dh": torch.float32, "ddrop": hd}, {k: ab for k in runs},
                        patterns={"ddrop": (sc != 0, ref["ddrop"].abs() < 1e-6)})


@pytest.mark.parametrize("hd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("lora", [False, True], ids=["nolora", "lora"])
def test_ln1_bwd(lora, M, p, hd):
    L = ops._L(hd)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g, c = params(M, hd, 4)
    h, dres, sg, dgate = rnd(g, M, E), rnd(g, M, E), rnd(g, M, E), rnd(g, M, H)
    sw = torch.tensor([0.37], device=DEV)
    m64, r64 = ln_stats64(h.double())
    mean, rstd = m64[:, 0].float().contiguous(), r64[:, 0].float().contiguous()
    ldx = E + 16 + 8
    dx1 = rnd(g, M, ldx, dtype=hd)
    sd = _p(c["seed"]) if p else None
    aq, av = (_p(c["aq"]), _p(c["av"])) if lora else (None, None)
    # the float64 restatement (x1 from the mean / rstd inputs, rounded to the storage type as the kernel does)
    xh = (h.double() - mean.double()[:, None]) * rstd.double()[:, None]
    y1 = xh * c["gm"].double() + c["bt"].double()
    x1 = y1.float().to(hd).double()
    amb = near_tie(y1, hd, 8 * EPS32 * ((xh * c["gm"].double()).abs() + c["bt"].double().abs()))   # 4 fp32 roundings
    ga, gb = gate64(x1, c["wg"], c["bg"], c["gc"])
    gc, dg = c["gc"].double(), dgate.double()
    dza, dzb = dg * (gb * gc - 1.0) * ga * (1.0 - ga), dg * ga * gc * gb * (1.0 - gb)
    wg = c["wg"].double()
    dxr = dx1[:, :E].double() + (dza[..., None] * wg[:4].sum(0) + dzb[..., None] * wg[4:].sum(0)).reshape(M, E)
    dabs = dx1[:, :E].double().abs() + (dza.abs()[..., None] * wg[:4].abs().sum(0)
                                        + dzb.abs()[..., None] * wg[4:].abs().sum(0)).reshape(M, E)
    xdr = xpat = None
    if lora:
        da = dx1[:, E:E + 16].double()
        sq, sv = scale_of(c["seed"], 11, p, M), scale_of(c["seed"], 12, p, M)
        dxr = dxr + sq * (da[:, :R] @ c["aq"].double()) + sv * (da[:, R:] @ c["av"].double())
        dabs = dabs + sq * (da[:, :R].abs() @ c["aq"].double().abs()) + sv * (da[:, R:].abs() @ c["av"].double().abs())
        xdr = torch.stack([x1 * sq, x1 * sv])
        xpat = (torch.stack([sq != 0, sv != 0]) & (x1 != 0), (xdr.abs() < 1e-6) | amb)
    # (A): see the module docstring
    w8, wmax = float(wg.abs().sum(0).max()), float(wg.abs().max())
    sz = float(((x1.abs().view(-1, H, 64) @ wg.abs().t()) + c["bg"].double().abs()).sum(-1).max())
    dgmax, dzmax = float(dg.abs().max()), float(torch.maximum(dza.abs(), dzb.abs()).max())
    p_row = rstd.double() * float(c["gm"].max()) * (2.0 + xh.abs().max(1).values)      # [M]
    P = float(p_row.max())
    b_dx = 16 * U * float(dabs.max()) + w8 * (0.2 * dgmax * 24 * U * sz + 16 * U * dzmax)
    # a row's ambiguous x1 elements: each may differ by one ulp16 from the kernel's, moving za and zb by |w| ulp16, dz
    # by 0.2 |dg| of that each, the head's dx by W8 times that, the row's dh by P times that
    b_flip = (p_row * w8 * 2 * 0.2 * dg.abs().max(1).values * wmax * EPS[hd] * x1.abs().max(1).values
              * amb.sum(1))[:, None]
    base = ln_bwd64(dxr, h.double(), mean.double()[:, None], rstd.double()[:, None], c["gm"].double()) + dres.double()
    for with_sg in (True, False):
        for with_drop in (True, False):
            def fn():
                dh = torch.empty(M, E, device=DEV)
                dd = torch.zeros(M, E, device=DEV, dtype=hd)
                xd = torch.zeros(2, M, E, device=DEV, dtype=hd)
                check(L.rdx_wl_ln1_bwd_ex(_p(dx1), ldx, _p(dgate), _p(h), _p(mean), _p(rstd), _p(c["gm"]), _p(c["bt"]),
                                          _p(c["wg"]), _p(c["bg"]), _p(c["gc"]), aq, av, R, sd, 11, 12, p, _p(dres),
                                          _p(dh), _p(xd) if lora else None, _p(sg) if with_sg else None,
                                          _p(sw) if with_sg else None, 7, p, _p(dd) if with_drop else None, M, E, st),
                      "ln1_bwd")
                o = {"dh": dh}
                if with_drop:
                    o["ddrop"] = dd
                if lora:
                    o["xd"] = xd
                return o
            runs = run_geos(L, K_LN1_BWD, lora, fn)
            dhr = base + (0.37 * sg.double() if with_sg else 0.0)
            sc = scale_of(c["seed"], 7, p, M)
            ref = {"dh": dhr, "ddrop": dhr * sc, "xd": xdr}
            bdh = ln_bwd_bound(dxr, h.double(), mean.double()[:, None], rstd.double()[:, None], c["gm"].double(),
                               torch.cat([dhr, dres.double(), sg.double()])) + P * b_dx + b_flip
            ab = {"dh": bdh, "ddrop": bdh * inv_keep(p) + ulp(hd, ref["ddrop"])}
            pats = {"ddrop": (sc != 0, ref["ddrop"].abs() < (4 * bdh).clamp_min(1e-6))}
            if lora:
                ab["xd"] = ulp(hd, xdr) + 1.12 * ulp(hd, x1) * (amb.sum(1) > 0)[None, :, None]
                pats["xd"] = xpat
            compare(f"ln1_bwd[{'lora' if lora else 'nolora'},M={M},p={p},{hd},sg={with_sg},ddrop={with_drop}]", runs,
                    {k: ref for k in runs}, {"dh": torch.float32, "ddrop": hd, "xd": hd}, {k: ab for k in runs},
                    exact=("xd",), patterns=pats)

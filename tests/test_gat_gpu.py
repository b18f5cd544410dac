"""csrc/gat.hip (radhip.ops.GatAtt: rdx_gat_att_fwd / rdx_gat_att_bwd) against the layer's formula in float64.

Reference: the same formula (pair product -> att_proj -> tanh -> @ att_weight -> / temp -> softmax over j -> @ x) in
float64 torch on the CPU, forward and, for the loss sum(agg * G), backward. Metric, per tensor (att, agg, dx, dW, db,
dw): max |got - ref64| / max |ref64|.

Bounds: measured once on an MI355X for the kernel and for the torch fp32 module path (the same formula in fp32 on the
GPU) on the same inputs, every case below; both are in profiles/gat_errors.json (written by running this file as a
script). Each tensor's bound is 4 x the module path's largest measured value over the cases, rounded up to one digit
and not below 2e-6: the kernel does the same fp32 arithmetic in another order, so it has no reason to be much worse,
and a missing term of the backward is an O(1) error.

Cases (B, N, Din, Dout): the model's own shapes, the lower limits (N = 1, N = 2), the upper limits (32, 64, 64), one
with nothing a multiple of 16, and the conf's batch of 24; each at temp 1 and 100; one with x scaled until tanh
saturates (|p| > 20) and the scores of a row spread by more than 50 (the softmax's max subtraction matters); one with
x a transpose(1, 2) view; one with W / b / w not requiring a gradient (dx only)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":      # run as a script to measure: the paths tests/conftest.py sets up for pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "robust-audio-deepfake-evolution_amd"), os.path.join(_root, "tests", "golden")):
        sys.path.insert(0, _p)

from seeded import seeded_array  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")

SHAPES = [(2, 23, 64, 32), (2, 29, 64, 32), (3, 12, 32, 16),      # GAT_layer_T, _S, _ST
          (1, 1, 8, 4), (1, 2, 64, 32),                           # lower limits
          (2, 32, 64, 64),                                        # upper limits
          (2, 13, 20, 5),                                         # nothing a multiple of 16
          (24, 29, 64, 32)]                                       # the conf's batch
TEMPS = [1.0, 100.0]
TENSORS = ("att", "agg", "dx", "dW", "db", "dw")
# 4 x the fp32 module path's largest error over the cases (profiles/gat_errors.json "module_max"), one digit, >= 2e-6
# module_max: att 2.95e-6, agg 3.44e-6, dx 3.61e-6, dW 4.57e-6, db 4.87e-6, dw 4.03e-6 (kernel: 3.09e-6, 3.49e-6, 8.02e-6,
# 6.00e-6, 6.69e-6, 6.56e-6)
BOUNDS = {"att": 2e-5, "agg": 2e-5, "dx": 2e-5, "dW": 2e-5, "db": 2e-5, "dw": 2e-5}


def _inputs(B, N, Din, Dout, xscale=1.0, wscale=0.5):
    tag = f"gat{B}_{N}_{Din}_{Dout}"
    f = lambda name, shape, s: torch.from_numpy(seeded_array(f"{tag}.{name}", shape, scale=s)).float()
    return dict(x=f("x", (B, N, Din), xscale), W=f("W", (Dout, Din), 0.2), b=f("b", (Dout,), 0.1),
                w=f("w", (Dout,), wscale), G=f("G", (B, N, Din), 1.0))


def _formula(x, W, b, w, temp, G):
    """The layer's attention map and aggregation as batched tensor ops in the dtype and on the device of x, and the
    gradients of sum(agg * G): the float64 reference on the CPU, the fp32 module path on the GPU."""
    x, W, b, w = (t.detach().clone().requires_grad_(True) for t in (x, W, b, w))
    p = torch.nn.functional.linear(x.unsqueeze(2) * x.unsqueeze(1), W, b)          # [B, N, N, Dout]
    s = (torch.tanh(p) @ w.unsqueeze(1)).squeeze(-1) / temp
    att = torch.softmax(s, dim=-1)
    agg = att @ x
    (agg * G).sum().backward()
    out = dict(att=att, agg=agg, dx=x.grad, dW=W.grad, db=b.grad, dw=w.grad)
    return {k: v.detach().double().cpu() for k, v in out.items()}, p.detach(), s.detach()


def _kernel(x, W, b, w, temp, G, weights_need_grad=True):
    from radhip import ops
    x = x.detach().requires_grad_(True)
    W, b, w = (t.detach().clone().requires_grad_(weights_need_grad) for t in (W, b, w))
    agg, att = ops.GatAtt.apply(x.contiguous(), W, b, w, temp)
    assert agg.dtype == att.dtype == torch.float32 and not att.requires_grad
    (agg * G).sum().backward()
    return dict(att=att.detach(), agg=agg.detach(), dx=x.grad, dW=W.grad, db=b.grad, dw=w.grad)


def _errors(got, ref):
    """max |got - ref| / max |ref| per tensor; a reference that is zero everywhere (N = 1: the softmax of one score
    is constant, so dW, db and dw vanish) admits only an exact zero (error 0, else inf)."""
    out = {}
    for k in TENSORS:
        if got.get(k) is None:
            continue
        d, r = float((got[k].double().cpu() - ref[k]).abs().max()), float(ref[k].abs().max())
        out[k] = d / r if r > 0 else (0.0 if d == 0 else float("inf"))
    return out


def _case(B, N, Din, Dout, temp, xscale=1.0, wscale=0.5):
    """(kernel errors, module-path errors, p64, s64) of one case."""
    t = _inputs(B, N, Din, Dout, xscale, wscale)
    ref, p, s = _formula(*(t[k].double() for k in ("x", "W", "b", "w")), temp, t["G"].double())
    g = {k: v.to(DEV) for k, v in t.items()}
    mod, _, _ = _formula(g["x"], g["W"], g["b"], g["w"], temp, g["G"])
    ker = _kernel(g["x"], g["W"], g["b"], g["w"], temp, g["G"])
    return _errors(ker, ref), _errors(mod, ref), p, s


def _check(ek, em, what):
    for k in TENSORS:
        print(f"[gat {what}] {k}: kernel {ek[k]:.3e} module {em[k]:.3e} bound {BOUNDS[k]:.0e}")
    bad = {k: (ek[k], BOUNDS[k]) for k in TENSORS if not ek[k] <= BOUNDS[k]}
    assert not bad, (what, bad)


SATURATED = dict(B=2, N=23, Din=64, Dout=32, temp=1.0, xscale=6.0, wscale=4.0)


@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("B,N,Din,Dout", SHAPES)
def test_kernel_matches_fp64_formula(B, N, Din, Dout, temp):
    ek, em, _, _ = _case(B, N, Din, Dout, temp)
    _check(ek, em, f"{B}x{N}x{Din}x{Dout} temp {temp}")


def test_saturated_tanh_and_wide_score_spread():
    ek, em, p, s = _case(**SATURATED)
    assert float(p.abs().median()) > 20.0                     # most of tanh is saturated
    assert float((s.max(-1)[0] - s.min(-1)[0]).max()) > 50.0   # exp() of a raw score difference would underflow
    _check(ek, em, "saturated")


def test_transposed_view_through_gat_att():
    """The encoders hand over transpose(1, 2) views: ops.gat_att makes them contiguous, and the gradient comes back
    in the view's layout."""
    from radhip import ops
    B, N, Din, Dout = 2, 23, 64, 32
    t = _inputs(B, N, Din, Dout)
    ref, _, _ = _formula(*(t[k].double() for k in ("x", "W", "b", "w")), 1.0, t["G"].double())
    lin = torch.nn.Linear(Din, Dout).to(DEV)
    aw = torch.nn.Parameter(t["w"].to(DEV).view(Dout, 1))
    with torch.no_grad():
        lin.weight.copy_(t["W"])
        lin.bias.copy_(t["b"])
    base = t["x"].transpose(1, 2).contiguous().to(DEV).requires_grad_(True)       # [B, Din, N], as an encoder's output
    xv = base.transpose(1, 2)
    assert not xv.is_contiguous() and ops.gat_eligible(xv, lin, aw)
    agg, att = ops.gat_att(xv, lin, aw)
    (agg * t["G"].to(DEV)).sum().backward()
    got = dict(att=att.detach(), agg=agg.detach(), dx=base.grad.transpose(1, 2), dW=lin.weight.grad, db=lin.bias.grad,
               dw=aw.grad.view(-1))
    ek = _errors(got, ref)
    _check(ek, ek, "transposed view")


def test_weights_without_grad_give_dx_only():
    B, N, Din, Dout = 2, 13, 20, 5
    t = _inputs(B, N, Din, Dout)
    ref, _, _ = _formula(*(t[k].double() for k in ("x", "W", "b", "w")), 1.0, t["G"].double())
    g = {k: v.to(DEV) for k, v in t.items()}
    got = _kernel(g["x"], g["W"], g["b"], g["w"], 1.0, g["G"], weights_need_grad=False)
    assert got["dW"] is None and got["db"] is None and got["dw"] is None
    full = _kernel(g["x"], g["W"], g["b"], g["w"], 1.0, g["G"])
    assert torch.equal(got["dx"], full["dx"])
    e = _errors(got, ref)
    assert e["dx"] <= BOUNDS["dx"] and e["agg"] <= BOUNDS["agg"], e


def test_two_runs_are_bit_identical():
    g = {k: v.to(DEV) for k, v in _inputs(24, 29, 64, 32).items()}
    a = _kernel(g["x"], g["W"], g["b"], g["w"], 1.0, g["G"])
    b = _kernel(g["x"], g["W"], g["b"], g["w"], 1.0, g["G"])
    for k in TENSORS:
        assert torch.equal(a[k], b[k]), k


def _raw(L, x, W, b, w, temp, B, N, Din, Dout):
    """The C entries called directly on the default stream: (rc_fwd, rc_bwd, att, agg, dx, dW, db, dw)."""
    o = dict(att=torch.zeros(B, N, N, device=DEV), agg=torch.zeros(B, N, Din, device=DEV),
             dx=torch.zeros(B, N, Din, device=DEV), dW=torch.zeros(B, Dout, Din, device=DEV),
             db=torch.zeros(B, Dout, device=DEV), dw=torch.zeros(B, Dout, device=DEV))
    G = torch.ones(B, N, Din, device=DEV)
    torch.cuda.synchronize()
    rf = L.rdx_gat_att_fwd(x.data_ptr(), W.data_ptr(), b.data_ptr(), w.data_ptr(), temp, B, N, Din, Dout,
                           o["att"].data_ptr(), o["agg"].data_ptr(), None)
    rb = L.rdx_gat_att_bwd(G.data_ptr(), x.data_ptr(), W.data_ptr(), b.data_ptr(), w.data_ptr(), temp,
                           o["att"].data_ptr(), B, N, Din, Dout, o["dx"].data_ptr(), o["dW"].data_ptr(),
                           o["db"].data_ptr(), o["dw"].data_ptr(), None)
    torch.cuda.synchronize()
    return rf, rb, o


@pytest.mark.parametrize("N,Din,Dout", [(33, 64, 32), (29, 65, 32), (29, 64, 65)])
def test_beyond_the_limits_is_unsupported(N, Din, Dout):
    from radhip import _lib, ops
    B = 2
    x = torch.ones(B, N, Din, device=DEV)
    lin = torch.nn.Linear(Din, Dout).to(DEV)
    aw = torch.nn.Parameter(torch.ones(Dout, 1, device=DEV))
    assert not ops.gat_eligible(x, lin, aw)
    assert not _lib.lib().rdx_gat_eligible(x.data_ptr(), N, Din, Dout, 1.0)
    rf, rb, o = _raw(_lib.lib(), x, lin.weight.detach(), lin.bias.detach(), aw.detach().view(-1), 1.0, B, N, Din, Dout)
    assert rf == -2 and rb == -2
    assert not any(bool(v.any()) for v in o.values())          # nothing was launched
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.gat_att(x, lin, aw)


def test_bad_arguments():
    from radhip import _lib, ops
    L = _lib.lib()
    B, N, Din, Dout = 1, 4, 8, 4
    g = {k: v.to(DEV) for k, v in _inputs(B, N, Din, Dout).items()}
    att, agg = torch.zeros(B, N, N, device=DEV), torch.zeros(B, N, Din, device=DEV)
    assert L.rdx_gat_att_fwd(None, g["W"].data_ptr(), g["b"].data_ptr(), g["w"].data_ptr(), 1.0, B, N, Din, Dout,
                             att.data_ptr(), agg.data_ptr(), None) == -1
    assert L.rdx_gat_att_fwd(g["x"].data_ptr(), g["W"].data_ptr(), g["b"].data_ptr(), g["w"].data_ptr(), 1.0, B, N,
                             Din, Dout, att.data_ptr(), None, None) == -1
    assert L.rdx_gat_att_bwd(g["G"].data_ptr(), g["x"].data_ptr(), g["W"].data_ptr(), g["b"].data_ptr(),
                             g["w"].data_ptr(), 1.0, att.data_ptr(), B, N, Din, Dout, None, None, None, None,
                             None) == -1
    assert L.rdx_gat_att_fwd(g["x"].data_ptr(), g["W"].data_ptr(), g["b"].data_ptr(), g["w"].data_ptr(), 0.0, B, N,
                             Din, Dout, att.data_ptr(), agg.data_ptr(), None) == -2        # temp must be positive
    lin = torch.nn.Linear(Din, Dout).to(DEV)
    aw = torch.nn.Parameter(torch.ones(Dout, 1, device=DEV))
    assert not ops.gat_eligible(g["x"].cpu(), lin, aw) and not ops.gat_eligible(g["x"].double(), lin, aw)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.GatAtt.apply(g["x"].double(), g["W"], g["b"], g["w"], 1.0)
    with pytest.raises(ValueError, match="required"):
        ops.GatAtt.apply(g["x"], g["W"][:, :4].contiguous(), g["b"], g["w"], 1.0)
    with pytest.raises(ValueError, match="positive"):
        ops.GatAtt.apply(g["x"], g["W"], g["b"], g["w"], 0.0)
    torch.cuda.synchronize()


def test_f16_library_gives_the_same_bits():
    """Both libraries export the entries; the arithmetic is fp32 in both."""
    from radhip import _lib
    B, N, Din, Dout = 2, 29, 64, 32
    g = {k: v.to(DEV) for k, v in _inputs(B, N, Din, Dout).items()}
    a = _raw(_lib.lib(), g["x"], g["W"], g["b"], g["w"], 1.0, B, N, Din, Dout)
    b = _raw(_lib.lib16(), g["x"], g["W"], g["b"], g["w"], 1.0, B, N, Din, Dout)
    assert a[0] == a[1] == b[0] == b[1] == 0
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]) and bool(a[2][k].any()), k


def measure():
    """Kernel and fp32-module-path errors of every case -> profiles/gat_errors.json."""
    rows, mod_max, ker_max = {}, dict.fromkeys(TENSORS, 0.0), dict.fromkeys(TENSORS, 0.0)
    cases = [(f"B{B},N{N},Din{Di},Dout{Do},temp{t:g}", dict(B=B, N=N, Din=Di, Dout=Do, temp=t))
             for (B, N, Di, Do) in SHAPES for t in TEMPS] + [("saturated", SATURATED)]
    for name, kw in cases:
        ek, em, _, _ = _case(**kw)
        rows[name] = {k: [float(f"{ek[k]:.3g}"), float(f"{em[k]:.3g}")] for k in TENSORS}
        for k in TENSORS:
            mod_max[k], ker_max[k] = max(mod_max[k], em[k]), max(ker_max[k], ek[k])
    out = {"_format": "per case and tensor: [kernel, fp32 module path], max |got - ref64| / max |ref64|",
           "cases": rows, "module_max": {k: float(f"{v:.3g}") for k, v in mod_max.items()},
           "kernel_max": {k: float(f"{v:.3g}") for k, v in ker_max.items()}, "bounds": BOUNDS}
    os.makedirs(PROFILES, exist_ok=True)
    with open(os.path.join(PROFILES, "gat_errors.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("module_max", "kernel_max")}))


if __name__ == "__main__":
    measure()

"""oracle/attn16.py and the power of tests/test_attn_edges_gpu.py's criterion, on the CPU.

  - the plain reference equals torch float64 autograd of the formula, to 1e-12 relative;
  - the inputs of every case (tests/attn_cases.py) have the properties the GPU test relies on;
  - the rounding-faithful reference lies within the derived plain-tier bound of the plain one (the derivation covers
    the roundings it names);
  - every mutation of attn16.MUTATIONS, applied to the faithful reference, exceeds the GPU test's criterion, with the
    committed constants, by a factor of at least 4 in at least one element, on every case it applies to.
"""
import pytest
import torch

import attn_cases as AC
from oracle import attn16
from oracle.head16 import EPS, ulp

IDS = [AC.case_id(c) for c in AC.CASES]


@pytest.mark.parametrize("T", [1, 2, 33, 65])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_plain_reference_equals_autograd(T, p):
    B, H = 2, 3
    g = torch.Generator().manual_seed(T)
    q, k, v = (torch.randn(B, H, T, 64, generator=g, dtype=torch.float64).requires_grad_() for _ in range(3))
    do = torch.randn(B, H, T, 64, generator=g, dtype=torch.float64)
    gate = (3 * torch.rand(B, H, T, generator=g, dtype=torch.float64)).requires_grad_()
    rel = torch.randn(H, 2 * T - 1, generator=g, dtype=torch.float64)
    keep = AC.keep_array(B, T, H, p) if p > 0 else None
    if keep is not None:
        keep[..., 0] = 1                        # no row without a key (T = 1)
    ref = attn16.reference(q.detach(), k.detach(), v.detach(), gate.detach(), rel, keep, p, do, torch.bfloat16,
                           faithful=False)
    s = 0.125 * (q @ k.transpose(-1, -2)) + gate[..., None] * attn16.rel_matrix(rel, T)[None]
    P = torch.softmax(s, -1)
    if keep is not None:
        P = P * keep * attn16.inv_keep(p)
    o = P @ v
    o.backward(do)
    want = {"o": o.detach(), "lse": torch.logsumexp(s, -1).detach(), "D": (do * o.detach()).sum(-1),
            "dq": q.grad, "dk": k.grad, "dv": v.grad, "dgate": gate.grad}
    for n, w in want.items():
        # relative to the result, or where it cancels to zero (dq, dk, dgate at T = 1) to its uncancelled terms
        scale = max(float(w.abs().max()), float(ref["F_" + n].max()) if "F_" + n in ref else 0.0)
        assert float((ref[n] - w).abs().max()) <= 1e-12 * scale, n


def test_keep_array_statistics():
    keep = AC.keep_array(2, 201, 4, 0.1)
    assert abs(float(keep.mean()) - (1 - 6554 / 65536)) < 2e-3
    assert not torch.equal(keep[0], keep[1])


@pytest.mark.parametrize("c", AC.CASES, ids=IDS)
def test_input_properties(c):
    B, T, H, dt, p, st, lay, route = c
    x = AC.inputs(c)
    ref = AC.reference(c, True)
    for n, t in list(ref.items()) + list(AC.tolerances(c).items()):
        if torch.is_tensor(t):
            assert bool(torch.isfinite(t).all()), n
    for n in ("q", "k", "v", "do"):
        assert torch.equal(x[n].to(dt).double(), x[n])
    assert float(x["gate"].min()) > 0 and float(x["gate"].max()) < 3
    nt = (T + 31) // 32
    if st in ("ramp_up", "ramp_down") and nt > 1:
        s = 0.125 * (x["q"] @ x["k"].transpose(-1, -2)) + x["gate"][..., None] * attn16.rel_matrix(x["rel"], T)[None]
        tile = s.argmax(-1) // 32
        frac = float((tile == (nt - 1 if st == "ramp_up" else 0)).double().mean())
        assert frac >= 0.9, frac
    if p > 0:
        tail = x["keep"][..., 32 * (nt - 1):]
        assert bool((tail == 1).any()) and bool((tail == 0).any())
        assert bool((x["keep"].sum(-1) > 0).all())
    assert AC.expected_entry(c) == AC.ENTRY_OF_ROUTE[route.split(":")[0]]
    assert attn16.fwd_is_split(B, T, H) == ((B, T, H) not in ((33, 33, 16), (17, 161, 16)))


def _ratio(c, got):
    """The largest |got - ref| / tolerance over every element of every result, the larger of the two tiers."""
    dt = c[3]
    plain, faith, tol = AC.reference(c, False), AC.reference(c, True), AC.tolerances(c)
    worst = 0.0
    for n in attn16.RES16 + attn16.RES32:
        worst = max(worst, float(((got[n] - plain[n]).abs() / tol[n].clamp_min(1e-300)).max()))
    for n in attn16.RES16:
        t = AC.K_FAITH[dt][n] * EPS[dt] * faith["A_" + n] + ulp(faith[n], dt) + attn16.slack_faithful(faith, n)
        worst = max(worst, float(((got[n] - faith[n]).abs() / t).max()))
    return worst


@pytest.mark.parametrize("c", AC.CASES, ids=IDS)
def test_faithful_within_plain_bound_and_mutations_exceed_it(c):
    B, T, H, dt, p, st, lay, route = c
    plain, faith, tol = AC.reference(c, False), AC.reference(c, True), AC.tolerances(c)
    for n in attn16.RES16 + attn16.RES32:
        r = float(((faith[n] - plain[n]).abs() / tol[n].clamp_min(1e-300)).max())
        assert r <= 1.0, (n, r)
    for mut in attn16.MUTATIONS:
        if attn16.mutation_applies(mut, B, T, H, p, st):
            r = _ratio(c, AC.reference(c, True, mutate=mut))
            assert r >= 4.0, (mut, r)

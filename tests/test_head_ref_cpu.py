"""oracle/head16.py, the fp64 reference of the fused head ops, checked on its own (no GPU).

Its backward is hand-written so that 16-bit roundings can be placed inside it, which autograd cannot see. With
rnd = identity it must therefore equal autograd through the unrounded formulas (mean -> relu(W1 .) -> sigmoid(W2 .)
-> product; softmax(f w + b, dim=1)^T f; F.interpolate(nearest) then cat): outputs and every gradient to 1e-10
relative, at every shape of tests/head_cases.py. The input properties the GPU tests rely on (an open gate, dead and
live squeeze units, flat and peaked attention, fp16-finite values) are asserted here on the rounded reference.
"""
import pytest
import torch
import torch.nn.functional as F

import head_cases as HC
from oracle import head16

REL = 1e-10


def _close(got, want, what):
    err = float((got - want).abs().max())
    assert err <= REL * max(float(want.abs().max()), 1e-300), (what, err, float(want.abs().max()))


def _leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize("shape", HC.SE_SHAPES, ids=str)
def test_se_identity_rounding_is_autograd(shape):
    c = HC.se_case(shape, torch.bfloat16)
    ref = head16.se(c["x"], c["w1"], c["w2"], c["dy"])
    x, w1, w2 = _leaf(c["x"]), _leaf(c["w1"]), _leaf(c["w2"])
    y = head16.se_plain(x, w1, w2)
    y.backward(c["dy"])
    _close(ref["y"], y.detach(), "y")
    _close(ref["dx"], x.grad, "dx")
    _close(ref["dw1"], w1.grad, "dw1")
    _close(ref["dw2"], w2.grad, "dw2")
    assert bool((ref["A1"] >= ref["dw1"].abs() * (1 - 1e-12)).all()) and bool((ref["A2"] >= ref["dw2"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("variant", HC.POOL_VARIANTS)
@pytest.mark.parametrize("shape", HC.POOL_SHAPES, ids=str)
def test_pool_identity_rounding_is_autograd(shape, variant):
    c = HC.pool_case(shape, variant, torch.float16)
    ref = head16.pool(c["f"], c["w"], c["b"], c["dfeat"])
    f, w = _leaf(c["f"]), _leaf(c["w"])
    b = _leaf(c["b"]) if c["b"] is not None else None
    feat = head16.pool_plain(f, w, b)
    feat.backward(c["dfeat"])
    _close(ref["feat"], feat.detach(), "feat")
    _close(ref["df"], f.grad, "df")
    if shape[1] > 1:
        _close(ref["dw"], w.grad, "dw")
    else:       # one frame: a = 1 and every dz, so dw and db, is zero up to the rounding of da - a da
        assert float(ref["dw"].abs().max()) <= 1e-12 * float(ref["Aw"].max() + 1.0)
    if b is not None:
        # db = sum_t dz is zero in exact arithmetic: held to the scale of its terms
        assert abs(float(ref["db"] - b.grad)) <= REL * float(ref["Ab"] + 1e-300), (float(ref["db"]), float(b.grad))
    assert bool((ref["Aw"] >= ref["dw"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("shape", HC.UPCAT_SHAPES, ids=str)
def test_upcat_identity_rounding_is_autograd(shape):
    c = HC.upcat_case(shape, torch.bfloat16)
    ref = head16.upcat(c["fw"], c["fs"], c["dout"])
    fw, fs = _leaf(c["fw"]), _leaf(c["fs"])
    out = head16.upcat_plain(fw, fs)
    out.backward(c["dout"])
    assert torch.equal(ref["out"], out.detach())
    assert torch.equal(ref["dfw"], fw.grad)
    _close(ref["dfs"], fs.grad, "dfs")
    # the index is torch's own: the same gather in the 16-bit storage types, where interpolate runs in fp32
    B, T1, T2, C = shape
    idx = head16.nearest_index(T1, T2)
    t2 = torch.arange(T2, dtype=torch.float32).view(1, 1, T2)
    assert torch.equal(F.interpolate(t2, size=T1, mode="nearest").view(-1).long(), idx)
    assert int(idx.min()) == 0 and int(idx.max()) == T2 - 1 and bool((idx[1:] >= idx[:-1]).all())


@pytest.mark.parametrize("dt", HC.DTYPES, ids=str)
@pytest.mark.parametrize("shape", HC.SE_SHAPES, ids=str)
def test_se_inputs_open_the_gate(shape, dt):
    HC.check_se_props(shape, HC.se_case(shape, dt), dt)


@pytest.mark.parametrize("dt", HC.DTYPES, ids=str)
@pytest.mark.parametrize("variant", HC.POOL_VARIANTS)
@pytest.mark.parametrize("shape", HC.POOL_SHAPES, ids=str)
def test_pool_inputs_are_flat_and_peaked(shape, variant, dt):
    HC.check_pool_props(shape, variant, HC.pool_case(shape, variant, dt))


def test_roundings_change_the_reference():
    """The rounding points are live: the reference with a storage type's rounding differs from the exact one, and
    its 16-bit results are values of that type."""
    for dt in HC.DTYPES:
        rnd = head16.rounder(dt)
        c = HC.se_case(HC.SE_LAYOUT_SHAPE, dt)
        exact = head16.se(c["x"], c["w1"], c["w2"], c["dy"])
        for k in ("y", "dx", "m", "h", "s"):
            assert torch.equal(rnd(c["ref"][k]), c["ref"][k]) and not torch.equal(exact[k], c["ref"][k]), k
        p = HC.pool_case(HC.POOL_SHAPES[2], "peaked", dt)
        exact = head16.pool(p["f"], p["w"], p["b"], p["dfeat"])
        for k in ("feat", "df"):
            assert torch.equal(rnd(p["ref"][k]), p["ref"][k]) and not torch.equal(exact[k], p["ref"][k]), k


def test_ulp_metric():
    one = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0, 2.0 ** -20, -3.0], dtype=torch.float64)
    assert head16.ulp(one, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133,
                                                        2.0 ** -27, 2.0 ** -6]
    assert head16.ulp(one, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24,
                                                       2.0 ** -24, 2.0 ** -9]
    for dt in HC.DTYPES:      # the spacing is the distance to the type's next value
        v = torch.tensor([1.0, 0.3, 100.0, 2.0 ** -13], dtype=torch.float64).to(dt)
        step = (v.view(torch.int16) + 1).view(dt).double() - v.double()
        assert torch.equal(head16.ulp(v.double(), dt), step), dt
    ref = torch.tensor([4.0, 0.0], dtype=torch.float64)
    assert head16.ulp_floored(ref, torch.float16).tolist() == [2.0 ** -8, 2.0 ** -22]
    assert head16.dist16(torch.tensor([4.0, 2.0 ** -21]).double(), ref, torch.float16) == 2.0
    A = torch.tensor([1.0, 0.0], dtype=torch.float64)
    assert head16.dist32(torch.tensor([1.0 + 2.0 ** -10, 0.0]).double(), torch.tensor([1.0, 0.0]).double(), A,
                         torch.float16) == 2.0
    assert head16.dist32(torch.tensor([1.0, 1e-30]).double(), torch.tensor([1.0, 0.0]).double(), A,
                         torch.float16) == float("inf")


def test_sum_metric_and_bounds_bite():
    """A one-ulp flip of one branch of dx reads as many ulps of a cancelled sum but as about 1 against the branches'
    spacing; a 10 % error in one channel of y is far outside the bound y is held to."""
    from test_head_edges_gpu import K_RES
    for dt in HC.DTYPES:
        rnd = head16.rounder(dt)
        r = HC.se_case(HC.SE_LAYOUT_SHAPE, dt)["ref"]
        got = rnd(r["dx1"] + r["dx2"] + head16.ulp(r["dx2"], dt))
        assert head16.dist16(got, r["dx"], dt) >= 16.0
        assert head16.dist16_sum(got, r["dx"], (r["dx1"], r["dx2"]), dt) <= 2.0
        y = r["y"].clone()
        y[:, :, 5] = rnd(y[:, :, 5] * 1.1)
        assert head16.dist16(y, r["y"], dt) > 10.0 * K_RES["se"][dt]["y"]

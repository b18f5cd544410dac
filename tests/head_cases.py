"""Inputs of the head edge tests (tests/test_head_ref_cpu.py, tests/test_head_edges_gpu.py): the shapes at which
csrc/head.hip changes geometry, and for each a seeded fp64 input set that the 16-bit storage type represents exactly,
built so that the gates are open. The properties are asserted on the fp64 reference (oracle/head16.py) alone.
"""
import zlib

import torch

from oracle import head16

DTYPES = [torch.bfloat16, torch.float16]

# (B, T, C, R): nq = C / 8 chunks, G = 256 / nq row groups, fc1 on 16 lanes per output (R <= 16), one [T, C] LDS image
# of at most 64 KiB
SE_SHAPES = [
    (1, 1, 8, 1),          # one frame, nq = 1, G = 256, T < G, R = 1
    (2, 5, 136, 8),        # nq = 17, G = 15: 255 active threads and one idle; T < G
    (3, 37, 144, 9),       # the model's channels, ragged T
    (5, 33, 16, 16),       # R = 16, the fc1 lane-group maximum, with R = C
    (2, 128, 256, 16),     # image exactly 64 KiB, nq = 32, G = 8, every thread busy
    (1, 227, 144, 9),      # the largest T that fits at C = 144
]
SE_LAYOUT_SHAPE = (3, 37, 144, 9)      # run once as a channel slice and once 8 bytes off alignment

# (B, T, C, bias): a thread per row (T > 256: two), channel loops of C / 256 passes, image of at most 128 KiB
POOL_SHAPES = [
    (1, 1, 8, True),       # a = 1, dz = 0, df = dfeat
    (2, 3, 1024, True),    # nq = 128, G = 2, four channel passes per thread
    (2, 257, 144, True),   # one thread owns two rows
    (1, 1024, 64, True),   # T at AP_TMAX, image exactly 128 KiB
    (2, 455, 144, True),   # the largest T that fits at C = 144
    (3, 201, 144, False),  # SideLinear(144, 1, bias=False): the bias = None / db = None path
]
POOL_VARIANTS = ["flat", "peaked"]
FLAT_MIN_T = 100           # max_t a < 0.05 needs at least 21 frames; asked of the shapes with T >= 100

# (B, T1, T2, C)
UPCAT_SHAPES = [
    (1, 5, 1, 8),          # T2 = 1
    (2, 201, 50, 8),       # ratio just above the 4.0 gate
    (1, 203, 29, 8),       # exact ratio of 7
    (1, 41, 10, 16),       # small ragged case
    (2, 1000, 7, 8),       # long runs in the backward's search
]

_CACHE = {}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def se_case(shape, dt):
    """x = randn + a per-channel offset in [-2, 2], dy = randn; W1's rows along +- the mean direction (so that every
    squeeze unit is clearly live or clearly dead, unit 0 live and, when R >= 2, unit 1 dead) plus per-element noise; W2
    random, its rows signed and scaled so that the gate s opens both ways. Returns the inputs, the reference `ref` for
    dt, and `pre` / `Apre`: fc1's sums before rounding and the sums of their terms' magnitudes."""
    key = ("se", shape, dt)
    if key in _CACHE:
        return _CACHE[key]
    B, T, C, R = shape
    rnd = head16.rounder(dt)
    g = _gen("se", shape)
    off = torch.rand(C, generator=g, dtype=torch.float64) * 4.0 - 2.0
    x = rnd(_randn(g, B, T, C) + off)
    dy = rnd(_randn(g, B, T, C))
    m = rnd(x.sum(1) / T)
    u = m.mean(0)
    u = u / (u @ u)                                            # m u is about 1 for every utterance
    sign = torch.where(torch.rand(R, generator=g) < 0.5, -1.0, 1.0).double()
    sign[0] = 1.0                                              # live: a sum that skipped unit 0 must show
    if R >= 2:
        sign[1] = -1.0
    beta = 0.6 + 0.8 * torch.rand(R, generator=g, dtype=torch.float64)
    w1 = rnd((sign * beta)[:, None] * (u[None, :] + 0.2 * u.norm() * _randn(g, R, C)))
    pre, Apre = m @ w1.t(), m.abs() @ w1.abs().t()
    h = torch.relu(rnd(pre))
    w2 = _randn(g, C, R)
    z0 = (h @ w2.t())[0]
    alt = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    w2 = w2 * (alt * torch.sign(z0))[:, None]                  # utterance 0: even channels pushed up, odd ones down
    z0 = z0.abs() * alt
    w2 = rnd(w2 * (1.2 / min(float(z0.max()), float(-z0.min()))))
    case = {"x": x, "dy": dy, "w1": w1, "w2": w2, "pre": pre, "Apre": Apre,
            "ref": head16.se(x, w1, w2, dy, rnd)}
    _CACHE[key] = case
    return case


def check_se_props(shape, case, dt):
    R = shape[3]
    ref = case["ref"]
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    assert float(ref["s"].min()) < 0.3 and float(ref["s"].max()) > 0.7, (float(ref["s"].min()), float(ref["s"].max()))
    if R >= 2:
        assert bool((ref["h"] == 0).any()) and bool((ref["h"] > 0).any())
    else:
        assert bool((ref["h"] > 0).all())
    # no unit sits on the relu's edge: a 16-bit rounding of every m (relative 2 eps of each term at the most) cannot
    # change a unit's sign, so kernel and reference agree on which units are dead
    assert bool((case["pre"].abs() >= 4.0 * head16.EPS[dt] * case["Apre"]).all())


def pool_case(shape, variant, dt):
    """f, dfeat = randn; w = gamma randn / sqrt(C). flat: gamma = 0.5 (scores of about +-1, near-uniform weights).
    peaked: the smallest gamma of 8, 16, 32, ... at which every utterance has one frame with a > 0.5 and the largest
    score magnitude is >= 20. bias 0.37 where the shape has one."""
    key = ("pool", shape, variant, dt)
    if key in _CACHE:
        return _CACHE[key]
    B, T, C, has_b = shape
    rnd = head16.rounder(dt)
    g = _gen("pool", shape)
    f = rnd(_randn(g, B, T, C))
    dfeat = rnd(_randn(g, B, C))
    w0 = _randn(g, C) / C ** 0.5
    b = rnd(torch.tensor(0.37, dtype=torch.float64)) if has_b else None
    gamma = 0.5 if variant == "flat" else 8.0
    while True:
        w = rnd(gamma * w0)
        ref = head16.pool(f, w, b, dfeat, rnd)
        if variant == "flat" or (float(ref["a"].max(1)[0].min()) > 0.5 and float(ref["z"].abs().max()) >= 20.0):
            break
        gamma *= 2.0
        assert gamma <= 1024.0
    case = {"f": f, "dfeat": dfeat, "w": w, "b": b, "ref": ref}
    _CACHE[key] = case
    return case


def check_pool_props(shape, variant, case):
    T = shape[1]
    ref = case["ref"]
    f16 = head16.rounder(torch.float16)
    for k, v in ref.items():       # finite, and still finite once stored in fp16
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(f16(v)).all()), k
    if variant == "flat":
        if T >= FLAT_MIN_T:
            assert float(ref["a"].max()) < 0.05, float(ref["a"].max())
    else:
        assert float(ref["a"].max(1)[0].min()) > 0.5
        assert float(ref["z"].abs().max()) >= 20.0


def upcat_case(shape, dt):
    key = ("upcat", shape, dt)
    if key in _CACHE:
        return _CACHE[key]
    B, T1, T2, C = shape
    rnd = head16.rounder(dt)
    g = _gen("upcat", shape)
    fw, fs, dout = rnd(_randn(g, B, T1, C)), rnd(_randn(g, B, T2, C)), rnd(_randn(g, B, T1, 2 * C))
    case = {"fw": fw, "fs": fs, "dout": dout, "ref": head16.upcat(fw, fs, dout, rnd)}
    _CACHE[key] = case
    return case

"""Cases of the gated-attention edge tests (tests/test_attn_ref_cpu.py, tests/test_attn_edges_gpu.py): the smallest
shapes that reach every launch path of csrc/attention.hip, and for each a seeded input set whose properties are
asserted on the fp64 reference (oracle/attn16.py) alone.

A case is (B, T, H, dtype, p_drop, input set, layout, backward route).

Forward (rdx_attn_fwd): the key-split kernel while B H ceil(nt / 4) <= 512, nt = ceil(T / 32); else the unsplit one,
reached by (33, 33, 16) (one workgroup per (b, h), nt = 2: two idle waves) and (17, 161, 16) (two workgroups per (b, h),
nt = 6: the second has two active waves and a one-row tail), each with and without dropout. The forward with 64-bit
dropout pair ids (kIdx32 = false) needs B H T ceil(T / 2) > 2^32, over 4 GB per operand: out of scope.

Backward routes (ops.attn_bwd_launch):
  fused1   rdx_attn_bwd_fused, one workgroup per (b, h): B H % 8 != 0 or B H >= 256, or RADHIP_ATTN_SPLIT=0
  fsplit   rdx_attn_bwd_fused_split, two workgroups per (b, h): B H < 256 and B H % 8 == 0. (8, T, 1) takes the plain
           block map (H % 8 != 0), (1, T, 8) and (2, T, 16) the XCD map with hpx = 1 and 2, (1, T, 24) hpx = 3
  pair     rdx_attn_bwd, the dQ + dK/dV kernels: T > 224, or RADHIP_ATTN_BWD=split

Layouts: `packed` (every row stride E = 64 H), `model` (q | k | v column slices of one [B T, 3E] buffer, dq | dk | dv of
another, o and dO packed: radhip/wavlm_fused.py's call), `padded` (q | k | v and dq | dk | dv in buffers of row stride
3E + 8, o and dO of E + 8, NaN in the inputs' pad columns, a canary in the outputs' and in 32 guard rows).

Input sets: q, k, v = 0.5 randn, dO = randn, gates uniform in (0, 3) throughout; the table is
  plain      unit normal (the existing tests' distribution)
  ramp_up    RAMP d / 32 + unit normal (d = key - query): the row maximum moves into every later key tile, so alpha
             rescales the accumulators at every tile and the merge of the key halves takes its state from the second.
             Used where the last tile is (nearly) full, T in {64, 223, 224, 255, 256}: a tail of one key seldom holds
             the maximum at a slope the scores can carry
  ramp_down  - RAMP d / 32 + unit normal: the maximum sits in the first tile swept and every later tile is small
  bucketed   piecewise constant like WavLM's compute_bias: one value per offset for |d| < 8, 8 log-spaced buckets per
             sign up to |d| = 64, constant beyond

The dropout keep array is computed here on the CPU by the kernels' paired counter hash (csrc/common.h: pair_hash,
half_keep, attn_seed); the GPU test checks rdx_attn_dropout_mask and the forward's mask words against it.
"""
import collections
import zlib

import numpy as np
import torch

from oracle import attn16

BF, HF = torch.bfloat16, torch.float16
RAMP = 8.0            # table slope per 32-key tile of the ramp sets (see test_attn_ref_cpu.py: >= 90 % of rows)
SEED, SALT = 1234567, 3

# (B, T, H, dtype, p_drop, set, layout, route)
CASES = [
    # ---- forward unsplit (more than 512 workgroups); backward fused1 by B H >= 256 (XCD map)
    (33, 33, 16, BF, 0.0, "plain", "packed", "fused1"),
    (33, 33, 16, HF, 0.1, "ramp_down", "model", "fused1"),
    (17, 161, 16, HF, 0.0, "ramp_down", "padded", "fused1"),
    (17, 161, 16, BF, 0.1, "plain", "packed", "fused1"),
    # ---- fused, one workgroup per (b, h)
    (1, 1, 3, BF, 0.0, "plain", "packed", "fused1"),
    (1, 31, 3, BF, 0.0, "ramp_up", "padded", "fused1"),
    (1, 32, 3, BF, 0.0, "plain", "model", "fused1"),
    (1, 65, 3, BF, 0.1, "plain", "padded", "fused1"),
    (1, 129, 3, HF, 0.0, "ramp_down", "packed", "fused1"),
    (1, 223, 3, BF, 0.0, "ramp_up", "packed", "fused1"),
    (1, 224, 3, BF, 0.1, "ramp_down", "model", "fused1"),
    (16, 65, 16, BF, 0.0, "bucketed", "model", "fused1"),          # 256 blocks, XCD map
    (1, 33, 24, BF, 0.1, "plain", "packed", "fused1:nosplit"),     # RADHIP_ATTN_SPLIT=0, hpx = 3
    # ---- fused, key-split
    (1, 2, 8, BF, 0.0, "plain", "packed", "fsplit"),               # the second workgroup has no key tile
    (1, 33, 8, BF, 0.1, "ramp_down", "padded", "fsplit"),
    (1, 64, 8, BF, 0.0, "ramp_up", "model", "fsplit"),
    (1, 97, 8, BF, 0.0, "ramp_down", "packed", "fsplit"),            # nt = 4, key halves 2 / 2
    (1, 224, 8, BF, 0.0, "ramp_up", "packed", "fsplit"),
    (8, 65, 1, BF, 0.0, "ramp_down", "padded", "fsplit"),          # plain block map
    (8, 161, 1, HF, 0.1, "plain", "model", "fsplit"),
    (1, 129, 24, BF, 0.0, "bucketed", "model", "fsplit"),          # hpx = 3
    (2, 201, 16, BF, 0.1, "ramp_down", "model", "fsplit"),
    (2, 201, 16, BF, 0.5, "plain", "packed", "fsplit"),
    # ---- dQ + dK/dV pair
    (1, 225, 2, BF, 0.1, "plain", "padded", "pair"),
    (1, 225, 2, BF, 0.0, "ramp_down", "packed", "pair"),
    (1, 255, 2, HF, 0.1, "ramp_up", "model", "pair"),
    (1, 256, 2, BF, 0.1, "ramp_up", "packed", "pair"),
    (1, 256, 2, BF, 0.0, "bucketed", "model", "pair"),
    (2, 201, 4, BF, 0.1, "plain", "model", "pair:forced"),         # RADHIP_ATTN_BWD=split
]
REUSE = ((2, 201, 16, BF, 0.1, "ramp_down", "model", "fsplit"), (1, 33, 8, BF, 0.1, "ramp_down", "padded", "fsplit"))

# Faithful-tier constants, per storage type and result: 2 x the worst value of the 16-bit torch restatement (the
# `torch` columns of profiles/attn_edges_errors.json, measured by `python tests/test_attn_edges_gpu.py`) in
# attn16.dist_faithful; 0 leaves the spacing term ulp(ref) alone.
K_FAITH = {BF: {"o": 0.995, "dq": 0, "dk": 0, "dv": 2.23},
           HF: {"o": 1.81, "dq": 0, "dk": 0, "dv": 1.14}}


def case_id(c):
    B, T, H, dt, p, st, lay, route = c
    return f"{B}x{T}x{H}-{'bf16' if dt == BF else 'fp16'}-p{p}-{st}-{lay}-{route}"


def route_env(route):
    """The environment a case's backward route is reached under."""
    return {"RADHIP_ATTN_BWD": "split" if route == "pair:forced" else "fused",
            "RADHIP_ATTN_SPLIT": "0" if route == "fused1:nosplit" else "1"}


def expected_entry(c):
    """The library entry point ops.attn_bwd_launch must take for the case, from its own conditions."""
    B, T, H, dt, p, st, lay, route = c
    env = route_env(route)
    if T > 224 or env["RADHIP_ATTN_BWD"] == "split":
        return "rdx_attn_bwd"
    if B * H < 256 and (B * H) % 8 == 0 and env["RADHIP_ATTN_SPLIT"] == "1":
        return "rdx_attn_bwd_fused_split"
    return "rdx_attn_bwd_fused"


ENTRY_OF_ROUTE = {"fused1": "rdx_attn_bwd_fused", "fsplit": "rdx_attn_bwd_fused_split", "pair": "rdx_attn_bwd"}


# ---- the kernels' dropout hash, on the CPU
def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85ebca6b)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xc2b2ae35)
    return h ^ (h >> np.uint32(16))


def keep_array(B, T, H, p, seed=SEED, salt=SALT):
    """{0, 1} keep [B, H, T, T] of the attention dropout: one hash per pair of keys of a score row, pair id =
    row ceil(T / 2) + key / 2, the low 16 bits deciding the even key and the high 16 the odd one against
    thr = round(p 2^16)."""
    M = (1 << 64) - 1
    s = ((seed & M) * 0x9E3779B97F4A7C15 + (salt & 0xffffffff) * 0xD1B54A32D192ED03) & M
    thr = int(min(max(p * 65536.0 + 0.5, 1.0), 65535.0))
    hp = (T + 1) // 2
    with np.errstate(over="ignore"):
        pid = np.arange(B * H * T * hp, dtype=np.uint64)
        x = ((pid & np.uint64(0xffffffff)).astype(np.uint32) ^ np.uint32(s & 0xffffffff)) * np.uint32(0x9E3779B1)
        x = x ^ (pid >> np.uint64(32)).astype(np.uint32) ^ np.uint32(((s >> 32) * 0x85ebca6b) & 0xffffffff)
        h = _fmix32(x).reshape(B, H, T, hp)
    both = np.stack([(h & np.uint32(0xffff)) >= thr, (h >> np.uint32(16)) >= thr], -1).reshape(B, H, T, 2 * hp)
    return torch.from_numpy(both[..., :T].astype(np.float64))


def bucket_table(g, H, T):
    d = torch.arange(-(T - 1), T)
    a = d.abs().clamp_max(64).double()
    b = torch.where(a < 8, a, 8 + torch.floor(torch.log(a.clamp_min(8) / 8) / np.log(8.0) * 8).clamp_max(8))
    b = (b + 17 * (d > 0)).long()                                        # 34 buckets: 17 per sign
    vals = torch.randn(H, 34, generator=g, dtype=torch.float64)
    return vals[:, b]


_CACHE = collections.OrderedDict()
KEEP_CASES = 2        # cases whose inputs, references and tolerances stay cached (the reuse test needs two at once)


def _slot(c):
    """The cache of one case; the least recently used case is dropped, so a session never holds more than
    KEEP_CASES cases' float64 arrays (the (17, 161, 16) cases are about 1 GB each)."""
    if c in _CACHE:
        _CACHE.move_to_end(c)
    else:
        _CACHE[c] = {}
        while len(_CACHE) > KEEP_CASES:
            _CACHE.popitem(last=False)
    return _CACHE[c]


def inputs(c):
    """Seeded inputs of a case: q, k, v, do [B, H, T, 64] and gate [B, H, T], rel [H, 2T - 1] in fp64 holding values of
    the storage types; keep [B, H, T, T] or None."""
    slot, key = _slot(c), "in"
    if key not in slot:
        B, T, H, dt, p, st = c[:6]
        g = torch.Generator().manual_seed(zlib.crc32(repr((B, T, H, str(dt), p, st)).encode()))
        q, k, v = ((0.5 * torch.randn(B, H, T, 64, generator=g)).to(dt).double() for _ in range(3))
        do = torch.randn(B, H, T, 64, generator=g).to(dt).double()
        gate = (3.0 * torch.rand(B, H, T, generator=g)).clamp_min(2.0 ** -20).double()
        d = torch.arange(-(T - 1), T).double()
        if st == "bucketed":
            rel = bucket_table(g, H, T)
        else:
            rel = torch.randn(H, 2 * T - 1, generator=g, dtype=torch.float64)
            if st == "ramp_up":
                rel = rel + RAMP * d / 32
            elif st == "ramp_down":
                rel = rel - RAMP * d / 32
            else:
                assert st == "plain"
        rel = rel.float().double()
        slot[key] = {"q": q, "k": k, "v": v, "do": do, "gate": gate, "rel": rel,
                     "keep": keep_array(B, T, H, p) if p > 0 else None}
    return slot[key]


def reference(c, faithful, mutate=None):
    """oracle/attn16.py on the case's inputs with the roundings of the path the case takes; computed once per case
    (a mutated reference is not kept). The faithful reference drops its [B, H, T, T] array P at once, the plain one
    once the tolerances are formed from it."""
    B, T, H, dt, p, st, lay, route = c
    slot, key = _slot(c), ("ref", faithful)
    if mutate is not None or key not in slot:
        x = inputs(c)
        r = attn16.reference(x["q"], x["k"], x["v"], x["gate"], x["rel"], x["keep"], p, x["do"], dt,
                             faithful=faithful, fwd_split=attn16.fwd_is_split(B, T, H),
                             dgate16=not route.startswith("pair"), mutate=mutate)
        if faithful:
            r.pop("P")
        if mutate is not None:
            return r
        slot[key] = r
    return slot[key]


def tolerances(c):
    slot = _slot(c)
    if "tol" not in slot:
        plain = reference(c, False)
        slot["tol"] = attn16.tolerances_plain(plain, inputs(c)["do"], c[3])
        plain.pop("P")
    return slot["tol"]

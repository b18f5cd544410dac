"""rdx_ingest_resample (csrc/ingest.hip) against the fp64 oracle, elementwise, on the GPU.

Reference: oracle.resample.resample(x.mean(axis=1), rate, 16000) in float64 (mean and resampling are linear). For
output o with taps k_i the kernel must satisfy

    |out_o - ref_o| <= (ntap + C + 2) 2^-24 sum_i |k_i| mean_c |x_{c,i}|

the first-order bound of an ntap-term fp32 fma chain (ntap u), the fp32 rounding of the stored taps (u) and a C-term
mean (C u). The bound's sum is evaluated with the oracle's own dense kernel. The largest err / bound of every case
goes to profiles/ingest_errors.json.

Shapes: (rate, C) in {(8000, 1), (11025, 2), (44100, 2), (48000, 2), (96000, 1), (32000, 6), (16001, 1)} (the last
reads its taps from global memory, 11025 has the largest table that is staged in LDS), each with recordings of 1,
orig_g - 1, width - 1 frames and of three output blocks plus 7 outputs, at odd input offsets and output offsets that
are not multiples of 4, in a buffer pre-filled with a sentinel. The oracle's dense kernel for 16001 Hz is 2 GB and
takes about 15 s to build: it is built once for the module and shared.

Measured on one MI355X (largest err / bound): 8000 x1 0.261, 11025 x2 0.203, 44100 x2 0.098, 48000 x2 0.119,
96000 x1 0.068, 32000 x6 0.074, 16001 x1 0.254, the 70 mixed jobs 0.341.
"""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import oracle.resample as oracle_resample

pytestmark = pytest.mark.gpu
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
RECORD = os.path.join(PROFILES, "ingest_errors.json")
CASES = [(8000, 1), (11025, 2), (44100, 2), (48000, 2), (96000, 1), (32000, 6), (16001, 1)]
SENTINEL = -777.25
U = 2.0 ** -24


def _record(key, obj):
    os.makedirs(PROFILES, exist_ok=True)
    cur = {}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            cur = json.load(f)
    cur[key] = obj
    cur["_format"] = ("per case: the largest |out - ref| / ((ntap + C + 2) 2^-24 sum_i |k_i| mean_c |x_ci|) over every "
                      "output of every job, ref = the fp64 oracle; must be <= 1")
    with open(RECORD, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(cur[k], sort_keys=True)}" for k in sorted(cur))
                + "\n}\n")


@pytest.fixture(scope="module", autouse=True)
def shared_oracle_kernels():
    """oracle.resample.resample builds its dense kernel on every call; here each rate's kernel is built once."""
    mp = pytest.MonkeyPatch()
    cached = functools.lru_cache(maxsize=None)(oracle_resample.sinc_kernel)
    mp.setattr(oracle_resample, "sinc_kernel", cached)
    yield
    mp.undo()
    cached.cache_clear()


def _abs_term(a, rate):
    """sum_i |k_i| a_i for every output, evaluated as oracle.resample.resample evaluates sum_i k_i x_i."""
    kern, width, orig, new = oracle_resample.sinc_kernel(rate, 16000, 6, 0.99)
    xp = np.concatenate([np.zeros(width), a, np.zeros(width + orig)])
    kw = kern.shape[1]
    nblk = (len(xp) - kw) // orig + 1
    win = np.lib.stride_tricks.sliding_window_view(xp, kw)[::orig][:nblk]
    return (win @ np.abs(kern).T).reshape(-1)[:int(math.ceil(new * len(a) / orig))]


def _reference(x, rate):
    """(ref fp64 [out_len], bound term fp64 [out_len]) of one recording x float32 [frames, C]."""
    x64 = x.astype(np.float64)
    ref = oracle_resample.resample(x64.mean(axis=1), rate, 16000)
    return ref, _abs_term(np.abs(x64).mean(axis=1), rate)


def _frames_for(out_len, og, ng):
    """The fewest frames that give at least out_len outputs (an up-sampled length comes in steps of new_g / orig_g)."""
    f = -(-out_len * og // ng)
    assert out_len <= -(-ng * f // og) < out_len + max(ng // og, 1) + 1
    return f


def _signal(rng, frames, ch):
    return (0.3 * rng.standard_normal((frames, ch))).astype(np.float32)


def _launch(tables, specs, in_pad=1, out_pad=3):
    """specs: [(rate, x [frames, C])]. Packs the inputs at odd offsets and the outputs at offsets that are no
    multiple of 4, launches once, returns (out host array, [(out_offset, out_len)], packed device input, jobs)."""
    from radhip import ops
    ins, outs, jobs = [], [], []
    ci, co = in_pad, out_pad
    for rate, x in specs:
        n = ops.ingest_out_len(x.shape[0], rate)
        ins.append((ci, x))
        outs.append((co, n))
        jobs.append(tables.job(rate, x.shape[1], x.shape[0], ci, co))
        ci += x.size + 2
        ci += 1 - ci % 2                       # odd element offsets
        co += n + 5
        co += (co % 4 == 0)
    host = np.full(ci, 5.5, dtype=np.float32)
    for o, x in ins:
        host[o:o + x.size] = x.reshape(-1)
    src = torch.from_numpy(host).cuda()
    dst = torch.full((co,), SENTINEL, device="cuda", dtype=torch.float32)
    ops.ingest_resample(src, dst, tables, jobs)
    assert all(o % 2 == 1 for o, _ in ins) and all(o % 4 for o, _ in outs)
    return dst.cpu().numpy(), outs, src, jobs


def _check(specs, got, outs, ntaps):
    """Every output of every job within its bound; every float between the jobs still the sentinel. Returns the
    largest err / bound."""
    worst = 0.0
    written = np.zeros(got.size, dtype=bool)
    for (rate, x), (o, n), ntap in zip(specs, outs, ntaps):
        ref, term = _reference(x, rate)
        assert ref.shape == (n,) == term.shape
        bound = (ntap + x.shape[1] + 2) * U * term
        err = np.abs(got[o:o + n].astype(np.float64) - ref)
        bad = np.nonzero(err > bound)[0]
        assert bad.size == 0, (rate, x.shape, int(bad[0]), float(err[bad[0]]), float(bound[bad[0]]))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[nz]).max()))
        written[o:o + n] = True
    assert (got[~written] == np.float32(SENTINEL)).all(), "a float outside every job was written"
    return worst


@pytest.mark.parametrize("rate,ch", CASES)
def test_kernel_matches_fp64_oracle(rate, ch):
    from radhip import ops
    tables = ops.IngestTables("cuda")
    _, _, ntap, width, og, ng = tables.entry(rate)
    ob, lds, in_lds = ops.ingest_plan(og, ng, ntap, ch)
    assert in_lds == (rate != 16001) and lds <= 65536
    rng = np.random.default_rng(rate + ch)
    blocks3 = _frames_for(3 * ob + 7, og, ng)
    lengths = sorted({1, max(og - 1, 1), max(width - 1, 1), blocks3})
    specs = [(rate, _signal(rng, f, ch)) for f in lengths]
    got, outs, src, jobs = _launch(tables, specs)
    # three whole blocks and a ragged fourth
    assert 3 * ob + 7 <= outs[lengths.index(blocks3)][1] < 3 * ob + 7 + 3
    worst = _check(specs, got, outs, [ntap] * len(specs))
    print(f"rate {rate} x{ch}: ntap {ntap}, block {ob}, taps in LDS {in_lds}: largest err / bound {worst:.3f}")
    _record(f"{rate}x{ch}", {"ntap": ntap, "block": ob, "taps_in_lds": in_lds, "frames": lengths,
                            "max_err_over_bound": worst})
    # a second launch on the same input writes the same bits
    again = torch.full((got.size,), SENTINEL, device="cuda", dtype=torch.float32)
    ops.ingest_resample(src, again, tables, jobs)
    assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_seventy_mixed_jobs_in_one_call():
    """Past the 64 jobs rdx_resample_batch takes, mixed rates, channel counts and lengths (1 .. a few thousand
    frames), one call: every job against the oracle, the gaps untouched."""
    from radhip import ops
    tables = ops.IngestTables("cuda")
    rng = np.random.default_rng(70)
    rates = [r for r, _ in CASES] + [22050, 16000]
    specs = []
    for i in range(70):
        rate = rates[i % len(rates)]
        frames = 1 if i < 3 else int(rng.integers(2, 5000))
        specs.append((rate, _signal(rng, frames, 1 + i % 3)))
    got, outs, _, _ = _launch(tables, specs)
    worst = _check(specs, got, outs, [tables.entry(r)[2] for r, _ in specs])
    print(f"70 mixed jobs: largest err / bound {worst:.3f}")
    _record("70_mixed_jobs", {"jobs": len(specs), "rates": sorted(set(rates)), "max_err_over_bound": worst})
    # the 16 kHz jobs are a pure down-mix
    for (rate, x), (o, n) in zip(specs, outs):
        if rate == 16000:
            assert n == x.shape[0]


def test_bad_arguments_launch_nothing():
    from radhip import _lib, ops
    L = _lib.lib()
    tables = ops.IngestTables("cuda")
    fo, to, ntap, width, og, ng = tables.entry(48000)
    src = torch.zeros(4096, device="cuda")
    dst = torch.full((4096,), SENTINEL, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(job, inp=src.data_ptr(), n_in=src.numel(), n_out=dst.numel()):
        arr = (_lib.IngestJob * 2)(_lib.IngestJob(0, 30, 0, fo, to, 1, og, ng, ntap, width, 0), job)
        return L.rdx_ingest_resample(inp, n_in, dst.data_ptr(), n_out, tables.first.data_ptr(), tables.first.numel(),
                                     tables.taps.data_ptr(), tables.taps.numel(), arr, 2, stream)

    def job(**kw):
        f = dict(in_offset=0, frames=300, out_offset=100, first_offset=fo, taps_offset=to, channels=2, orig_g=og,
                 new_g=ng, ntap=ntap, width=width, reserved=0)
        f.update(kw)
        return _lib.IngestJob(**f)
    assert call(job(), inp=None) == -1                              # null pointer
    assert call(job(frames=0)) == -1 and call(job(frames=-5)) == -1
    assert call(job(in_offset=4096 - 599)) == -1                    # 600 floats from there end past the input
    assert call(job(in_offset=-1)) == -1
    assert call(job(out_offset=4096 - 99)) == -1                    # 100 outputs from there end past the output
    assert call(job(taps_offset=tables.taps.numel())) == -1 and call(job(first_offset=tables.first.numel())) == -1
    assert call(job(channels=0)) == -1
    assert call(job(channels=1025, frames=3)) == -2                 # inside the buffers: unsupported, not invalid
    torch.cuda.synchronize()
    # the valid first job of each call was not launched either
    assert (dst == SENTINEL).all()
    assert call(job()) == 0
    torch.cuda.synchronize()
    assert (dst[:10] != SENTINEL).all() and (dst[100:200] != SENTINEL).all() and (dst[10:100] == SENTINEL).all()

"""Host side of the ingest stage (csrc/ingest.hip rdx_ingest_taps / rdx_ingest_plan, csrc/flac.cpp
rdx_flac_read_batch_interleaved, radhip.audio.read_batch_interleaved / probe_any, the chunk plan of
radhip/recordings.py): the entries of the built libraries, no GPU.

The compact taps are compared with oracle.resample.sinc_kernel, the dense fp64 kernel. At 16001 Hz that kernel is
16000 x 16015 (2 GB as fp64, several times that while numpy builds it, about 15 s): it is built once, checked and
dropped.
"""
import math

import numpy as np
import pytest

from flac_writer import encode
from oracle.resample import sinc_kernel

RATES = [8000, 11025, 22050, 44100, 48000, 96000, 16001, 32000]
NTAP = {8000: 13, 11025: 13, 16001: 13, 22050: 17, 44100: 34, 48000: 37, 96000: 73}


@pytest.mark.parametrize("rate", RATES)
def test_compact_taps_match_dense_oracle(rate):
    from radhip import ops
    first, taps, width, og, ng = ops.ingest_taps(rate, 16000)
    ntap = taps.shape[0]
    dense, w, o, n = sinc_kernel(rate, 16000)
    assert (w, o, n) == (width, og, ng) and dense.shape == (ng, 2 * width + og)
    assert first.shape == (ng,) and first.dtype == np.int32 and taps.dtype == np.float32
    assert ntap <= 2 * width + 2
    if rate in NTAP:
        assert ntap == NTAP[rate]
    kw = dense.shape[1]
    assert first.min() >= 0 and first.max() < kw
    # compact[p, j] against the dense value at first[p] + j (positions past the dense row are padding)
    pos = first[:, None].astype(np.int64) + np.arange(ntap)[None, :]
    inside = pos < kw
    want = np.where(inside, np.take_along_axis(dense, np.minimum(pos, kw - 1), axis=1), 0.0)
    got = taps.T                                                   # [ng, ntap]
    same = got == want.astype(np.float32)
    # a slot past the phase's own count is zero where the dense row holds the clipped window's < 1e-30
    padded = (got == 0) & (np.abs(want) < 1e-30)
    assert (same | padded).all(), (rate, np.argwhere(~(same | padded))[:4])
    # ... and only there: every dense value the table drops is below 1e-30
    outside = np.ones(dense.shape, dtype=bool)
    rows = np.broadcast_to(np.arange(ng)[:, None], pos.shape)
    outside[rows[inside], pos[inside]] = False
    assert float(np.abs(dense[outside]).max(initial=0.0)) < 1e-30
    assert float(np.abs(want[padded & ~same]).max(initial=0.0)) < 1e-30
    # the size query answers the same numbers and a short buffer is refused
    import ctypes
    from radhip import _lib
    q = [ctypes.c_int() for _ in range(4)]
    assert _lib.lib().rdx_ingest_taps(rate, 16000, 6, 0.99, None, None, 0, *[ctypes.byref(v) for v in q]) == 0
    assert [v.value for v in q] == [ntap, width, og, ng]
    small = np.empty(ntap * ng - 1, dtype=np.float32)
    assert _lib.lib().rdx_ingest_taps(rate, 16000, 6, 0.99, first.ctypes.data, small.ctypes.data, small.size,
                                      *[ctypes.byref(v) for v in q]) == -1


@pytest.mark.parametrize("rate", RATES + [192000])
def test_block_span_fits_the_planned_tile(rate):
    """The kernel stages frames m_first(o0) .. m_first(o0 + ob - 1) + ntap - 1 of a block: for every phase a block can
    start at, that span lies inside the x tile the plan reserves (ceil((ob - 1) orig / new) + ntap + 2 frames), first
    never decreases, and the plan's LDS stays within 64 KiB."""
    from radhip import ops
    first, taps, width, og, ng = ops.ingest_taps(rate, 16000)
    ntap = taps.shape[0]
    first = first.astype(np.int64)
    assert (np.diff(first) >= 0).all() and first[0] + og >= first[-1]
    for ch in (1, 2, 6):
        ob, lds, in_lds = ops.ingest_plan(og, ng, ntap, ch)
        assert ob % 256 == 0 and 256 <= ob <= 1024 and lds <= 65536
        xcap = -(-og * (ob - 1) // ng) + ntap + 2
        raw = 2048 if ch > 1 else 0
        assert lds == 4 * (xcap + raw + (ng * (ntap + 1) if in_lds else 0))
        assert in_lds == (rate != 16001)           # 0.8 MiB of taps stay in global memory
        p0 = np.arange(ng)
        ql = p0 + ob - 1
        span = (ql // ng) * og + first[ql % ng] + ntap - first[p0]
        assert 0 < span.min() and span.max() <= xcap


def test_plan_refuses_what_does_not_fit():
    import ctypes
    from radhip import _lib
    L = _lib.lib()
    out = [ctypes.byref(ctypes.c_int()) for _ in range(3)]
    assert L.rdx_ingest_plan(3, 1, 37, 2, *out) == 0
    assert L.rdx_ingest_plan(3, 1, 37, 1025, *out) == -2       # more channels than a staging pass holds
    assert L.rdx_ingest_plan(100, 1, 1201, 1, *out) == -2      # 256 outputs' input span beyond 64 KiB
    assert L.rdx_ingest_plan(0, 1, 37, 1, *out) == -1 and L.rdx_ingest_plan(3, 1, 37, 0, *out) == -1


# ------------------------------------------------------------------------- interleaved reader ----
def _pcm(n, ch, bits, seed):
    rng = np.random.default_rng(seed)
    amp = 2 ** (bits - 1)
    x = np.clip(np.round(0.1 * amp * rng.standard_normal((n, ch))), -amp, amp - 1).astype(np.int64)
    x[0, 0], x[-1, -1] = -amp, amp - 1            # both ends of the range
    return x[:, 0] if ch == 1 else x


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from scipy.io import wavfile
    root = tmp_path_factory.mktemp("ingest_files")
    out = []
    for ch in (1, 2, 6):
        for bits in (16, 24):
            p = root / f"c{ch}_b{bits}.flac"
            kinds = ["verbatim", "fixed2"]
            p.write_bytes(encode(_pcm(5000 + 37 * ch + bits, ch, bits, seed=ch * 100 + bits), sample_rate=44100,
                                 bps=bits, plan=lambda f, c, b: {"kind": kinds[(f + c) % 2]}))
            out.append(p)
    rng = np.random.default_rng(3)
    p = root / "pcm16.wav"
    wavfile.write(p, 48000, _pcm(3001, 2, 16, seed=7).astype(np.int16))
    out.append(p)
    p = root / "f32.wav"
    wavfile.write(p, 22050, (0.3 * rng.standard_normal((2000, 3))).astype(np.float32))
    out.append(p)
    p = root / "mono_f32.wav"
    wavfile.write(p, 8000, (0.3 * rng.standard_normal(777)).astype(np.float32))
    out.append(p)
    return out


def test_library_exports_the_interleaved_header():
    from radhip import audio
    syms = audio.header_symbols("radio_interleaved.h")
    assert syms == ["rdx_flac_read_batch_interleaved"] and hasattr(audio.lib(), syms[0])
    assert syms[0] in audio.SIGNATURES


def test_interleaved_reader_equals_read(files):
    from radhip import audio
    buf, offsets, frames, chans, rates = audio.read_batch_interleaved(files, threads=3)
    assert buf.dtype == np.float32 and buf.size == int((frames * chans).sum())
    o = 0
    for p, off, f, c, r in zip(files, offsets, frames, chans, rates):
        x, sr = audio.read(p)
        assert (f, c, r) == (x.shape[0], 1 if x.ndim == 1 else x.shape[1], sr) == audio.probe_any(p)
        assert off == o
        np.testing.assert_array_equal(buf[off:off + f * c], x.astype(np.float32).reshape(-1))
        o += f * c
    # a caller's buffer (as the scorer's pinned one), larger than needed: the rest is untouched
    import torch
    mine = torch.full((buf.size + 5,), 9.0)
    audio.read_batch_interleaved(files, out=mine, threads=1)
    np.testing.assert_array_equal(mine[:buf.size].numpy(), buf)
    assert (mine[buf.size:] == 9.0).all()
    with pytest.raises(ValueError, match="too small"):
        audio.read_batch_interleaved(files, out=np.empty(buf.size - 1, dtype=np.float32))


def test_interleaved_reader_names_the_missing_file(files, tmp_path):
    from radhip import audio
    for name in ("gone.flac", "gone.wav"):
        with pytest.raises(audio.AudioReadError, match=name):
            audio.read_batch_interleaved([files[0], tmp_path / name, files[1]])


def test_native_entry_refuses_another_channel_count(files):
    """The buffer is sized from channels[i]: a file with more channels must not be decoded into it."""
    import ctypes
    import os
    from radhip import audio
    L = audio.lib()
    stereo = [p for p in files if p.name == "c2_b16.flac"][0]
    frames = audio.probe(stereo)[0]
    out = np.full(frames + 8, 7.0, dtype=np.float32)
    i64 = ctypes.POINTER(ctypes.c_int64)
    offs, caps, got = (np.array([v], dtype=np.int64) for v in (0, frames, 0))
    ch, status = np.array([1], dtype=np.int32), np.zeros(1, dtype=np.int32)
    code = L.rdx_flac_read_batch_interleaved((ctypes.c_char_p * 1)(os.fsencode(str(stereo))), 1, out.ctypes.data,
                                             offs.ctypes.data_as(i64), caps.ctypes.data_as(i64),
                                             ch.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                             got.ctypes.data_as(i64),
                                             status.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 2)
    assert code == status[0] == -107 and (out == 7.0).all()
    assert b"channel count" in L.rdx_io_strerror(-107)


# --------------------------------------------------------------------------------- chunk plan ----
def test_converted_lengths_and_chunk_cuts(monkeypatch):
    from radhip import recordings
    frames = np.array([1, 3, 441, 193803, 82687, 50000, 64600, 16001, 16000])
    rates = np.array([48000, 48000, 44100, 48000, 44100, 8000, 16000, 16001, 16001])
    lens = recordings.converted_lengths(frames, rates)
    assert lens.tolist() == [math.ceil(16000 * f / r) for f, r in zip(frames, rates)]
    assert lens.tolist() == [1, 1, 160, 64601, 30000, 100000, 64600, 16000, 16000]

    monkeypatch.setattr(recordings, "CHUNK_SAMPLES", 1000)
    cap = recordings.CHUNK_SAMPLES
    #        raw floats (frames x channels)     16 kHz samples
    raw = [600, 600, 100, 100, 5000, 10, 300, 300, 300]
    out = [200, 200, 600, 600, 1700, 20, 100, 100, 100]
    cuts = list(recordings._chunks_convert(raw, out, cap))
    # 600 + 600 raw is over the cap; 100 + 100 raw fits but 600 + 600 converted does not; the 5000-float recording is
    # alone in its chunk; the tail fits both ways
    assert cuts == [(0, 1), (1, 3), (3, 4), (4, 5), (5, 9)]
    assert [i for a, b in cuts for i in range(a, b)] == list(range(len(raw)))
    for a, b in cuts:
        assert b - a == 1 or (sum(raw[a:b]) <= cap and sum(out[a:b]) <= cap)
    # with equal sizes the two-cap rule is the existing one
    same = [400, 700, 100, 1200, 300]
    assert list(recordings._chunks_convert(same, same, cap)) == list(recordings._chunks(same, cap))
    assert list(recordings._chunks_convert([], [], cap)) == []

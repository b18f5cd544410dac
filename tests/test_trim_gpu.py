"""The silence-trimming kernels (csrc/trim.hip: rdx_trim_energy, rdx_trim_plan, rdx_trim_compact) against the numpy
statement of the rule (radhip.recordings.trim_plan_np / trim_apply_np, pinned by tests/test_trim_cpu.py), through
ops.trim_silence and through the entry points themselves.

One launch holds eleven recordings packed at an odd offset: the hand-built cases of the CPU file (zeros around a
burst, an inner gap of 2 pad and of 2 pad + 1 frames at pad = 2, all zeros, n = 1, 319, 320, 321, a one-sample last
frame that is the peak), a mix of seeded noise at 0 dB, -20 dB and -60 dB with exact zeros cut at odd samples, and
one recording of 699 917 samples = 2 188 frames, more than two scan tiles of 1 024, in which speech and silence
change exactly at the tile boundaries (frames 1 024 and 2 048) and all along. It is planned with trim_db 40 and 10
and pads 0, 2, 10 and one larger than any recording, in both modes.

Exact: keep, dst, kept_len, kept_ids and the compacted samples (a copy). Energy: |e - e64| <= 4e-5 e64, twice the
worst-case relative error 321 * 2^-24 = 1.9e-5 of an fp32 sum of 320 non-negative products. The decisions can be
compared exactly because no frame of the float64 reference lies within 1e-3 of a threshold, relatively
(test_reference_keeps_clear_of_the_thresholds, on the host): the fp32 error cannot flip one.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F = 320
LEAD = 3                                    # samples in front of the first recording
PARAMS = [(40.0, 10), (40.0, 2), (40.0, 0), (10.0, 2), (10.0, 0), (10.0, 5000)]
MODES = ["ends", "gaps"]
LEVEL = {"0": 0.1, "-20": 0.01, "-60": 0.0001, "z": 0.0}


def _noise(rng, parts):
    """parts: (samples, level name) runs of seeded gaussian noise."""
    return np.concatenate([(LEVEL[lv] * rng.standard_normal(n)).astype(np.float32) for n, lv in parts])


def _long(rng):
    """2 188 frames: a cycle of runs cut at half frames, then speech up to frame 1 023 / silence from 1 024, and
    silence up to 2 047 / speech from 2 048."""
    cycle = [(13 * F, "0"), (30 * F, "z"), (7 * F, "-20"), (25 * F, "-60"), (5 * F + 160, "0"), (20 * F + 160, "z")]
    n = 2187 * F + 77
    parts, total = [], 0
    while total < n:
        parts.append(cycle[len(parts) % len(cycle)])
        total += parts[-1][0]
    x = _noise(rng, parts)[:n]
    for a, b, lv in [(1000, 1024, "0"), (1024, 1060, "z"), (2010, 2048, "z"), (2048, 2060, "0")]:
        x[a * F:b * F] = _noise(rng, [((b - a) * F, lv)])
    return x


@pytest.fixture(scope="module")
def recs():
    rng = np.random.default_rng(20240)
    const = lambda *parts: np.concatenate([np.full(n, a, dtype=np.float32) for n, a in parts])   # noqa: E731
    xs = [const((3 * F, 0.0), (2 * F, 0.5), (4 * F, 0.0)),
          const((1, 0.25)),
          _long(rng),
          np.zeros(5 * F + 7, dtype=np.float32),
          const((319, 0.25)), const((320, 0.25)), const((321, 0.25)),
          const((2 * F, 0.1), (1, 1.0)),
          _noise(rng, [(F, "0"), (4 * F, "z"), (F, "0")]),
          _noise(rng, [(F, "0"), (5 * F, "z"), (F, "0")]),
          _noise(rng, [(8000, "z"), (7040, "-60"), (20000, "0"), (5000, "-20"), (4000, "z"), (3001, "0")])]
    lens = np.array([x.size for x in xs], dtype=np.int64)
    offs = LEAD + np.concatenate([[0], np.cumsum(lens[:-1])])
    packed = np.concatenate([np.full(LEAD, 7.0, dtype=np.float32)] + xs)
    nf = -(-lens // F)
    return {"xs": xs, "lens": lens, "offs": offs, "nf": nf, "foffs": np.concatenate([[0], np.cumsum(nf[:-1])]),
            "packed": packed, "sig": torch.from_numpy(packed).cuda(), "ref": {}}


def _ref(recs, mode, db, pad):
    """Per recording (keep, kept_ids, m, dst, y) by the numpy rule, computed once per setting."""
    from radhip.recordings import trim_apply_np, trim_plan_np
    key = (mode, db, pad)
    if key not in recs["ref"]:
        out = []
        for x in recs["xs"]:
            keep, ids, m = trim_plan_np(x, mode, db, pad)
            flen = np.minimum(F, x.size - F * np.arange(keep.size))
            dst = np.where(keep, np.cumsum(np.where(keep, flen, 0)) - np.where(keep, flen, 0), -1)
            out.append((keep, ids, m, dst.astype(np.int64), trim_apply_np(x, ids)))
        recs["ref"][key] = out
    return recs["ref"][key]


def _assert_clear(xs, db):
    """No frame of the float64 reference has e / (peak ratio) inside [1 - 1e-3, 1 + 1e-3]."""
    from radhip.recordings import frame_energy_np
    for r, x in enumerate(xs):
        e = frame_energy_np(x)
        if e.max() == 0:
            continue
        q = e / (e.max() * 10.0 ** (-db / 10.0))
        near = np.nonzero((q >= 1 - 1e-3) & (q <= 1 + 1e-3))[0]
        assert near.size == 0, (db, r, near[:5], q[near[:5]])


def test_reference_keeps_clear_of_the_thresholds(recs):
    """The condition under which exact comparison is fair, on the float64 energies alone."""
    assert recs["nf"][2] == 2188 > 2 * 1024 and recs["lens"][7] % F == 1 and recs["lens"][1] == 1
    for db in sorted({db for db, _ in PARAMS}):
        _assert_clear(recs["xs"], db)
    # the long recording changes state at both tile boundaries and is cut there
    keep = _ref(recs, "gaps", 40.0, 2)[2][0]
    assert keep[1023 + 2] and not keep[1024 + 2] and not keep[2047 - 2] and keep[2048 - 2]
    assert 0 < keep[:1024].sum() < 1024 and 0 < keep[1024:2048].sum() < 1024 and 0 < keep[2048:].sum() < 140


def test_energy_is_within_the_fp32_sum_bound(recs):
    from radhip import ops
    from radhip.recordings import frame_energy_np
    e = ops.trim_energy(recs["sig"], recs["offs"], recs["lens"])
    again = ops.trim_energy(recs["sig"], recs["offs"], recs["lens"])
    assert e.dtype == torch.float32 and e.numel() == int(recs["nf"].sum())
    assert torch.equal(e.view(torch.int32), again.view(torch.int32))
    got = e.cpu().numpy().astype(np.float64)
    e64 = np.concatenate([frame_energy_np(x) for x in recs["xs"]])
    rel = np.abs(got - e64) / np.where(e64 > 0, e64, 1.0)
    print(f"largest |e - e64| / e64 = {rel.max():.3e} over {e64.size} frames (bound 4e-5)")
    assert (got[e64 == 0] == 0).all()
    assert (np.abs(got - e64) <= 4e-5 * e64).all(), rel.max()


@pytest.mark.parametrize("db,pad", PARAMS)
@pytest.mark.parametrize("mode", MODES)
def test_plan_and_compaction_equal_the_numpy_rule(recs, mode, db, pad):
    from radhip import ops
    ref = _ref(recs, mode, db, pad)
    sig, offs, lens, foffs, nf = (recs[k] for k in ("sig", "offs", "lens", "foffs", "nf"))
    total = int(nf.sum())
    # the entry points one by one
    e = ops.trim_energy(sig, offs, lens)
    plan = ops.trim_plan(e, lens, mode, db, pad)
    assert torch.equal(plan, ops.trim_plan(e, lens, mode, db, pad))
    host = plan.cpu().numpy()
    dst, kept_len = host[:total], host[total:]
    assert kept_len.tolist() == [m for _, _, m, _, _ in ref]
    for r, (keep, ids, m, want, y) in enumerate(ref):
        got = dst[foffs[r]:foffs[r] + nf[r]]
        np.testing.assert_array_equal(got >= 0, keep, err_msg=f"keep of recording {r}")
        np.testing.assert_array_equal(got, want, err_msg=f"dst of recording {r}")
    new_offs = 5 + np.concatenate([[0], np.cumsum(kept_len[:-1])])
    out = torch.full((5 + int(kept_len.sum()) + 5,), -9.0, device="cuda")
    ops.trim_compact(sig, offs, lens, plan[:total], new_offs, out)
    want = np.concatenate([np.full(5, -9.0, np.float32)] + [y for *_, y in ref] + [np.full(5, -9.0, np.float32)])
    np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    # the composed call
    y, new_lens, kept_ids = ops.trim_silence(sig, offs, lens, mode, db, pad)
    y2 = ops.trim_silence(sig, offs, lens, mode, db, pad)[0]
    assert new_lens.tolist() == kept_len.tolist() and len(kept_ids) == len(ref)
    for got, (_, ids, *_) in zip(kept_ids, ref):
        assert got.dtype == np.int64 and got.tolist() == ids.tolist()
    np.testing.assert_array_equal(y.cpu().numpy().view(np.int32), want[5:-5].view(np.int32))
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32))


def test_nothing_to_trim_returns_the_packed_input(recs):
    from radhip import ops
    x = torch.from_numpy(np.concatenate([recs["xs"][5], recs["xs"][3]])).cuda()
    y, new_lens, kept_ids = ops.trim_silence(x, [0, 320], [320, 5 * F + 7], "gaps", 40.0, 0)
    assert y.data_ptr() == x.data_ptr() and new_lens.tolist() == [320, 5 * F + 7]
    assert [k.tolist() for k in kept_ids] == [[0], list(range(6))]


def test_more_recordings_than_one_launch_holds(recs):
    """150 short recordings: the entry points cut them into launches of 64, and kept_len lands in order."""
    from radhip import ops
    from radhip.recordings import trim_apply_np, trim_plan_np
    rng = np.random.default_rng(7)
    xs = [_noise(rng, [(int(rng.integers(1, 4)) * F + int(rng.integers(0, F)), "z"), (int(rng.integers(200, 900)), "0"),
                       (int(rng.integers(0, 700)), "z")]) for _ in range(150)]
    _assert_clear(xs, 10.0)
    lens = np.array([x.size for x in xs])
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    y, new_lens, kept_ids = ops.trim_silence(torch.from_numpy(np.concatenate(xs)).cuda(), offs, lens, "gaps", 10.0, 1)
    plans = [trim_plan_np(x, "gaps", 10.0, 1) for x in xs]
    assert new_lens.tolist() == [m for *_, m in plans]
    assert all(a.tolist() == b.tolist() for a, (_, b, _) in zip(kept_ids, plans))
    np.testing.assert_array_equal(y.cpu().numpy(), np.concatenate([trim_apply_np(x, p[1]) for x, p in zip(xs, plans)]))


def test_entry_points_refuse_bad_arguments_and_write_nothing(recs):
    from radhip import _lib
    L = _lib.lib()
    sig, total, R = recs["sig"], int(recs["nf"].sum()), recs["lens"].size
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))  # noqa: E731
    offs, lens, foffs, nf = (np.ascontiguousarray(recs[k], dtype=np.int64) for k in ("offs", "lens", "foffs", "nf"))
    e = torch.full((total,), -1.0, device="cuda")
    dst = torch.full((total + R,), -77, device="cuda", dtype=torch.int64)
    scratch = torch.zeros(total, device="cuda", dtype=torch.int32)
    out = torch.full((int(lens.sum()),), -9.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    kl = ctypes.c_void_p(dst.data_ptr() + 8 * total)
    bad_lens = lens.copy()
    bad_lens[4] = 0
    assert L.rdx_trim_energy(None, ip(offs), ip(lens), ip(foffs), R, p(e), None) == -1
    assert L.rdx_trim_energy(p(sig), ip(offs), ip(lens), ip(foffs), R, None, None) == -1
    assert L.rdx_trim_energy(p(sig), None, ip(lens), ip(foffs), R, p(e), None) == -1
    assert L.rdx_trim_energy(p(sig), ip(offs), ip(lens), ip(foffs), 0, p(e), None) == -1
    assert L.rdx_trim_energy(p(sig), ip(offs), ip(bad_lens), ip(foffs), R, p(e), None) == -1
    good = (p(e), ip(foffs), ip(nf), ip(lens), R)
    for ratio, pad, mode in [(0.0, 10, 1), (1.5, 10, 1), (float("nan"), 10, 1), (-0.1, 10, 0), (1e-4, -1, 1),
                             (1e-4, 10, 2), (1e-4, 10, -1)]:
        assert L.rdx_trim_plan(*good, ratio, pad, mode, p(scratch), p(dst), kl, None) == -1, (ratio, pad, mode)
    assert L.rdx_trim_plan(None, ip(foffs), ip(nf), ip(lens), R, 1e-4, 10, 1, p(scratch), p(dst), kl, None) == -1
    assert L.rdx_trim_plan(*good, 1e-4, 10, 1, None, p(dst), kl, None) == -1
    assert L.rdx_trim_plan(*good, 1e-4, 10, 1, p(scratch), None, kl, None) == -1
    assert L.rdx_trim_plan(*good, 1e-4, 10, 1, p(scratch), p(dst), None, None) == -1
    assert L.rdx_trim_plan(p(e), ip(foffs), ip(nf + 1), ip(lens), R, 1e-4, 10, 1, p(scratch), p(dst), kl, None) == -1
    assert L.rdx_trim_plan(p(e), ip(foffs), ip(nf), ip(lens), -3, 1e-4, 10, 1, p(scratch), p(dst), kl, None) == -1
    new_offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    assert L.rdx_trim_compact(p(sig), ip(offs), ip(lens), ip(foffs), None, ip(new_offs), R, p(out), None) == -1
    assert L.rdx_trim_compact(p(sig), ip(offs), ip(lens), ip(foffs), p(dst), None, R, p(out), None) == -1
    assert L.rdx_trim_compact(p(sig), ip(offs), ip(lens), ip(foffs), p(dst), ip(new_offs), R, None, None) == -1
    assert L.rdx_trim_compact(p(sig), ip(offs), ip(lens), ip(foffs), p(dst), ip(-new_offs - 1), R, p(out), None) == -1
    torch.cuda.synchronize()
    assert (e == -1.0).all() and (dst == -77).all() and (scratch == 0).all() and (out == -9.0).all()
    # the host wrapper names its own refusals
    from radhip import ops
    with pytest.raises(ValueError, match="mode"):
        ops.trim_silence(sig, offs, lens, "middle")
    with pytest.raises(ValueError, match="db"):
        ops.trim_silence(sig, offs, lens, "gaps", 0.0)
    with pytest.raises(ValueError, match="pad"):
        ops.trim_silence(sig, offs, lens, "gaps", 40.0, -1)
    with pytest.raises(ValueError, match="outside"):
        ops.trim_silence(sig, offs + 1, lens, "gaps")

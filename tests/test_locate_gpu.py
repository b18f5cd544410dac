"""The locating kernels (csrc/locate.hip: rdx_track_overlap, rdx_track_segments, rdx_track_segment_stats) against the
numpy statement of the rule (radhip.recordings.track_np / segments_np, pinned by tests/test_locate_cpu.py), through
ops.score_track / ops.track_segments and through the entry points themselves, on seeded synthetic scores.

Track. One call holds recordings of 30 000, 64 600, 64 601, 64 920, 100 000 and 700 160 samples (the last has 2 188
frames), a second one 70 short recordings, past the 64 recordings a launch carries; hops 64 600, 32 300, 3 200, 1 000
and 333. Bound, per frame j with c_j covering windows:
    |t[j] - track_np[j]| <= (c_j + 3) 2^-24 max_k |s_k|
c_j roundings of the fmaf chain (each at most 2^-24 of a partial sum that the final division scales to at most
max|s|), one conversion of the weight sum, one division, and one unit of slack for second order. The largest
err / bound of every case goes to profiles/locate_errors.json. Two launches give the same bits, and canary floats
around the output stay untouched.

Segments. Compared against segments_np applied to the very fp32 track the device read: bounds, counts, min and argmin
exactly (no threshold-proximity precondition is needed), mean within (frames - 1) 2^-24 max|t| of float64 (the
two-sum bound of rdx_segment_reduce). Hand-built tracks of 2 188 frames, more than two tiles of 1 024: flags that
change at frames 1 023 / 1 024 / 1 025 and 2 047 / 2 048; a gap of `merge` frames across frame 1 024 with a run of
`min_frames` frames across frame 2 048, and the same with merge + 1 and min_frames - 1; seeded flags; all of it next
to tracks of 1, 2, 1 023, 1 024 and 1 025 frames. Grid (merge, min_frames) in {(0, 1), (2, 1), (0, 3), (10, 25),
(5000, 1), (0, 5000)}, thresholds below every value, above every value and in between.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
RECORD = os.path.join(PROFILES, "locate_errors.json")
F, WIN, U = 320, 64600, 2.0 ** -24
HOPS = [64600, 32300, 3200, 1000, 333]
LENS = [30000, 64600, 64601, 64920, 100000, 700160]
GRID = [(0, 1), (2, 1), (0, 3), (10, 25), (5000, 1), (0, 5000)]
SENTINEL, LEAD = -777.25, 5
EINVAL, EUNSUPPORTED = -1, -2


def _record(key, obj):
    os.makedirs(PROFILES, exist_ok=True)
    cur = {}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            cur = json.load(f)
    cur[key] = obj
    cur["_format"] = ("track_*: the largest |t - track_np| / ((c + 3) 2^-24 max|s|) over every frame of the call, c = "
                      "the frame's covering windows; segments_*: the largest |mean - fp64 mean| / ((frames - 1) 2^-24 "
                      "max|t|) over every segment of more than one frame; both must be <= 1")
    with open(RECORD, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(cur[k], sort_keys=True)}" for k in sorted(cur))
                + "\n}\n")


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _covering(m, hop):
    """c_j: the windows that overlap frame j."""
    from radhip.recordings import window_table
    _, start, _ = window_table([m], hop)
    c = np.zeros(-(-m // F) + 1, dtype=np.int64)
    if m <= WIN:
        return c[:-1] + 1
    np.add.at(c, start // F, 1)
    np.add.at(c, (start + WIN - 1) // F + 1, -1)
    return np.cumsum(c)[:-1]


def _track_case(lens, hop, rng):
    """The fp32 scores of the recordings' windows, LEAD unused scores in front, and the float64 reference."""
    from radhip.recordings import track_np, window_table
    lens = np.asarray(lens, dtype=np.int64)
    _, _, seg = window_table(lens, hop)
    seg = seg + LEAD
    s = (3.0 * rng.standard_normal(int(seg[-1]))).astype(np.float32)
    s[:LEAD] = np.nan       # a read in front of the first recording's scores would show
    ref = [track_np(int(m), s[a:b], hop) for m, a, b in zip(lens, seg[:-1], seg[1:])]
    bound = [(_covering(int(m), hop) + 3) * U * float(np.abs(s[a:b]).max()) for m, a, b in zip(lens, seg[:-1], seg[1:])]
    return lens, seg, s, np.concatenate(ref), np.concatenate(bound)


def _track_direct(s_dev, seg, lens, hop):
    """rdx_track_overlap itself, into a buffer with LEAD canaries on each side."""
    from radhip import _lib
    nfr = -(-lens // F)
    foffs = np.concatenate([[0], np.cumsum(nfr[:-1])]).astype(np.int64)
    total = int(nfr.sum())
    buf = torch.full((total + 2 * LEAD,), SENTINEL, device="cuda", dtype=torch.float32)
    seg_dev = torch.from_numpy(seg).cuda()
    nwin = np.ascontiguousarray(np.diff(seg))
    _lib.check(_lib.lib().rdx_track_overlap(_p(s_dev), _p(seg_dev), _ip(nwin), _ip(lens), _ip(foffs), lens.size, hop,
                                            WIN, _p(buf, LEAD), None), "track_overlap")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:LEAD] == SENTINEL).all() and (host[LEAD + total:] == SENTINEL).all()
    return host[LEAD:LEAD + total]


@pytest.mark.parametrize("hop", HOPS)
def test_track_is_within_the_fp32_bound_of_the_rule(hop):
    from radhip import ops
    rng = np.random.default_rng(7000 + hop)
    short = rng.integers(1, 130000, 70)
    short[:4] = [1, 320, 321, 64600]
    worst = {}
    for name, lens in (("six", LENS), ("seventy", short)):
        lens, seg, s, ref, bound = _track_case(lens, hop, rng)
        assert name != "six" or -(-lens[-1] // F) == 2188
        s_dev = torch.from_numpy(s).cuda()
        got = _track_direct(s_dev, seg, lens, hop)
        assert got.dtype == np.float32 and got.size == ref.size and np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - ref)
        worst[name] = float((err / bound).max())
        print(f"hop {hop}, {name}: {lens.size} recordings, {got.size} frames, largest err / bound {worst[name]:.3f}")
        j = int(np.argmax(err / bound))
        assert (err <= bound).all(), (name, j, got[j], ref[j], bound[j])
        # a second launch, through the op, writes the same bits
        again = ops.score_track(s_dev, seg, lens, hop, WIN)
        assert again.dtype == torch.float32 and again.is_cuda
        assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32))
    _record(f"track_hop{hop}", {"max_err_over_bound": worst, "lens_six": LENS, "recordings_seventy": 70})


def test_track_pins_the_worked_values_and_the_tiled_recording():
    from radhip import ops
    s = torch.tensor([0.75, -2.5, 9.0], device="cuda")
    t = ops.score_track(s, [0, 2, 3], [64601, 30000], 32300, WIN).cpu().numpy().astype(np.float64)
    assert t.size == 202 + 94
    assert abs(t[0] - (320 * 0.75 + 319 * -2.5) / 639) <= 5 * U * 2.5
    assert abs(t[201] - (280 * 0.75 + 281 * -2.5) / 561) <= 5 * U * 2.5
    assert (t[202:] == 9.0).all()


def test_track_refusals():
    from radhip import _lib, ops
    L = _lib.lib()
    s = torch.zeros(8, device="cuda")
    lens = np.array([64601, 100], dtype=np.int64)
    seg = np.array([0, 2, 3], dtype=np.int64)
    nwin, foffs = np.array([2, 1], dtype=np.int64), np.array([0, 202], dtype=np.int64)
    seg_dev, t = torch.from_numpy(seg).cuda(), torch.full((203,), SENTINEL, device="cuda")
    good = [_p(s), _p(seg_dev), _ip(nwin), _ip(lens), _ip(foffs), 2, 32300, WIN, _p(t), None]
    assert L.rdx_track_overlap(*good) == 0
    for k in (0, 1, 2, 3, 4, 8):
        bad = list(good)
        bad[k] = None
        assert L.rdx_track_overlap(*bad) == EINVAL, k
    for k, v in ((5, 0), (5, -2), (6, 0), (6, WIN + 1), (7, 0)):
        bad = list(good)
        bad[k] = v
        assert L.rdx_track_overlap(*bad) == EINVAL, (k, v)
    for arr in (np.array([1, 1]), np.array([2, 2]), np.array([3, 1])):     # not the rule's window count
        bad = list(good)
        bad[2] = _ip(arr.astype(np.int64))
        assert L.rdx_track_overlap(*bad) == EINVAL
    for k, arr in ((3, np.array([64601, 0])), (4, np.array([0, -1]))):
        bad = list(good)
        bad[k] = _ip(arr.astype(np.int64))
        assert L.rdx_track_overlap(*bad) == EINVAL
    # refused calls wrote nothing new; the one good call wrote every frame
    torch.cuda.synchronize()
    assert (t.cpu().numpy() != SENTINEL).all()
    with pytest.raises(ValueError, match="window rule"):
        ops.score_track(s, [0, 1, 2], lens, 32300, WIN)
    with pytest.raises(ValueError, match="hop"):
        ops.score_track(s, seg, lens, 0, WIN)
    with pytest.raises(ValueError, match="outside"):
        ops.score_track(s, seg + 6, lens, 32300, WIN)
    with pytest.raises(ValueError):
        ops.score_track(s, seg, [64601, 0], 32300, WIN)
    with pytest.raises(TypeError):
        ops.score_track(s.double(), seg, lens, 32300, WIN)


# ---------------------------------------------------------------------------------- segments ----
NF = 2188


def _values(rng, flag):
    """fp32 track values for a flag pattern: flagged frames in [-2, -1], the others in [1, 2]."""
    lo, hi = rng.uniform(-2, -1, flag.size), rng.uniform(1, 2, flag.size)
    return np.where(flag, lo, hi).astype(np.float32)


def _tracks(merge, min_frames, rng):
    """The hand-built tracks for one grid point (the structure is built with merge and min_frames capped at 40)."""
    M, K = min(merge, 40), min(min_frames, 40)
    flags = []
    a = np.zeros(NF, dtype=bool)                    # A: changes at 1023 / 1024 / 1025 and 2047 / 2048
    a[1000:1024] = True
    a[1025:1100] = True
    a[2048:2100] = True
    a[0] = a[NF - 1] = True
    flags.append(a)
    for gap, run in ((M, K), (M + 1, max(K - 1, 1))):
        b = np.zeros(NF, dtype=bool)
        g0 = 1024 - gap // 2                        # the gap [g0, g0 + gap) lies across frame 1024
        b[g0 - 30:g0] = True
        b[g0 + gap:g0 + gap + 30] = True
        r0 = 2048 - (run + 1) // 2                  # the run [r0, r0 + run) lies across frame 2048
        b[r0:r0 + run] = True
        flags.append(b)
    flags.append(rng.random(NF) < 0.5)
    flags.append(rng.random(NF) < 0.05)
    flags.append(rng.random(NF) < 0.95)
    for n in (1, 1, 2, 2, 1023, 1024, 1024, 1025):
        flags.append(rng.random(n) < 0.5)
    flags[6][:] = True                              # one frame, flagged
    flags[7][:] = False                             # one frame, not flagged
    flags[12][:] = True                             # 1024 frames, all flagged: the run ends at the virtual position
    ts = [_values(rng, f) for f in flags]
    ts[3][5:9] = np.float32(-1.5)                   # equal minima: the first wins
    return ts


def _check_segments(ts, thr, merge, min_frames, got):
    from radhip.recordings import segments_np
    assert len(got) == len(ts)
    worst, count = 0.0, 0
    for r, (t, g) in enumerate(zip(ts, got)):
        a, b, mean, lo, arg = segments_np(t, thr, merge, min_frames)
        what = (r, thr, merge, min_frames)
        assert all(x.dtype == np.int64 for x in (g[0], g[1], g[4])) and g[2].dtype == g[3].dtype == np.float32, what
        assert g[0].tolist() == a.tolist() and g[1].tolist() == b.tolist(), what
        assert np.array_equal(g[3].view(np.uint32), lo.view(np.uint32)) and g[4].tolist() == arg.tolist(), what
        for x, y, mu, gm in zip(a, b, mean, g[2]):
            bound = (y - x) * U * float(np.abs(t[x:y + 1]).max())
            err = abs(float(gm) - mu)
            assert err <= bound, (what, x, y, gm, mu, bound)
            if y > x:
                worst = max(worst, err / bound)
        count += a.size
    return worst, count


@pytest.mark.parametrize("merge,min_frames", GRID)
def test_segments_equal_the_rule_on_the_device_track(merge, min_frames):
    from radhip import ops
    rng = np.random.default_rng(100 * merge + min_frames)
    ts = _tracks(merge, min_frames, rng)
    assert ts[0].size == NF > 2 * 1024
    nfr = np.array([t.size for t in ts], dtype=np.int64)
    dev = torch.from_numpy(np.concatenate(ts)).cuda()
    worst, total = 0.0, 0
    for thr in (-3.0, 3.0, 0.0, -1.5):      # below every value, above every value, between the groups, inside one
        got = ops.track_segments(dev, nfr, thr, merge, min_frames)
        w, n = _check_segments(ts, thr, merge, min_frames, got)
        worst, total = max(worst, w), total + n
        if thr == -3.0:
            assert n == 0
        if thr == 3.0:      # every frame is flagged: one segment per recording that is long enough
            assert n == int((nfr >= min_frames).sum())
        # a second launch gives the same bits
        again = ops.track_segments(dev, nfr, thr, merge, min_frames)
        for g, h in zip(got, again):
            assert all(np.array_equal(x, y) for x, y in zip(g, h))
    if merge <= 40 and min_frames <= 40:    # the built gap and run behave as the rule says, across the tile boundaries
        got = ops.track_segments(dev, nfr, 0.0, merge, min_frames)
        g0, r0 = 1024 - merge // 2, 2048 - (min_frames + 1) // 2
        assert (g0 - 30, g0 + merge + 29) in list(zip(got[1][0].tolist(), got[1][1].tolist()))
        assert (r0, r0 + min_frames - 1) in list(zip(got[1][0].tolist(), got[1][1].tolist()))
        g1 = 1024 - (merge + 1) // 2
        assert list(zip(got[2][0].tolist(), got[2][1].tolist()))[:2] == [(g1 - 30, g1 - 1),
                                                                        (g1 + merge + 1, g1 + merge + 30)]
        assert got[2][0].size == (2 if min_frames > 1 else 3)
    print(f"merge {merge}, min_frames {min_frames}: {total} segments, largest mean err / bound {worst:.3f}")
    _record(f"segments_merge{merge}_min{min_frames}", {"segments": total, "max_mean_err_over_bound": worst})


def test_segments_of_seventy_recordings_and_untouched_slots():
    """Past the 64 recordings of one launch, through the entry points, with canaries in every slot array."""
    from radhip import _lib
    from radhip.recordings import segments_np
    L = _lib.lib()
    rng = np.random.default_rng(31)
    nfr = rng.integers(1, 300, 70).astype(np.int64)
    nfr[:3] = [1, 2, 3]
    ts = [_values(rng, rng.random(int(n)) < 0.6) for n in nfr]
    foffs = np.concatenate([[0], np.cumsum(nfr[:-1])]).astype(np.int64)
    total, R = int(nfr.sum()), nfr.size
    dev = torch.from_numpy(np.concatenate(ts)).cuda()
    ints = torch.full((4, total + 2 * LEAD), -7, device="cuda", dtype=torch.int32)
    flts = torch.full((2, total + 2 * LEAD), SENTINEL, device="cuda", dtype=torch.float32)
    count = ints[3]
    a, b, arg = (_p(ints[k], LEAD) for k in range(3))
    mean, lo = (_p(flts[k], LEAD) for k in range(2))
    seg_args = [_p(dev), _ip(foffs), _ip(nfr), R, 0.0, 1, 2, a, b, _p(count, LEAD), None]
    stat_args = [_p(dev), _ip(foffs), _ip(nfr), R, a, b, _p(count, LEAD), mean, lo, arg, None]
    _lib.check(L.rdx_track_segments(*seg_args), "track_segments")
    _lib.check(L.rdx_track_segment_stats(*stat_args), "track_segment_stats")
    torch.cuda.synchronize()
    hi, hf = ints.cpu().numpy(), flts.cpu().numpy()
    assert (hi[:, :LEAD] == -7).all() and (hi[:3, LEAD + total:] == -7).all() and (hi[3, LEAD + R:] == -7).all()
    assert (hf[:, :LEAD] == SENTINEL).all() and (hf[:, LEAD + total:] == SENTINEL).all()
    for r in range(R):
        ra, rb, rmean, rlo, rarg = segments_np(ts[r], 0.0, 1, 2)
        n, o = int(hi[3, LEAD + r]), LEAD + int(foffs[r])
        assert n == ra.size <= (nfr[r] + 1) // 2, r
        assert hi[0, o:o + n].tolist() == ra.tolist() and hi[1, o:o + n].tolist() == rb.tolist(), r
        assert hi[2, o:o + n].tolist() == rarg.tolist() and np.array_equal(hf[1, o:o + n], rlo), r
        assert (np.abs(hf[0, o:o + n] - rmean) <= (rb - ra) * U * 2.0).all(), r
        # slots at or past count are not written
        end = LEAD + int(foffs[r]) + int(nfr[r])
        assert (hi[:3, o + n:end] == -7).all() and (hf[:, o + n:end] == SENTINEL).all(), r
    # refusals
    for k in (0, 1, 2, 7, 8, 9):
        bad = list(seg_args)
        bad[k] = None
        assert L.rdx_track_segments(*bad) == EINVAL, k
    for k, v in ((3, 0), (4, float("nan")), (5, -1), (6, 0)):
        bad = list(seg_args)
        bad[k] = v
        assert L.rdx_track_segments(*bad) == EINVAL, (k, v)
    zero = nfr.copy()
    zero[5] = 0
    huge = nfr.copy()
    huge[5] = 2 ** 31 - 1
    for entry, args in ((L.rdx_track_segments, seg_args), (L.rdx_track_segment_stats, stat_args)):
        bad = list(args)
        bad[2] = _ip(zero)
        assert entry(*bad) == EINVAL
        bad[2] = _ip(huge)
        assert entry(*bad) == EUNSUPPORTED
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9):
        bad = list(stat_args)
        bad[k] = None
        assert L.rdx_track_segment_stats(*bad) == EINVAL, k


def test_track_segments_checks_its_arguments():
    from radhip import ops
    t = torch.zeros(10, device="cuda")
    for nfr, kw in (([4, 5], {}), ([10, 0], {}), ([], {}), ([10], {"thr": float("nan")}), ([10], {"thr": 1e39}),
                    ([10], {"merge": -1}), ([10], {"merge": 0.5}), ([10], {"min_frames": 0})):
        args = dict(thr=0.5, merge=1, min_frames=1)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.track_segments(t, nfr, **args)
    with pytest.raises(TypeError):
        ops.track_segments(t.double(), [10], 0.5, 1, 1)
    with pytest.raises(Exception):
        ops.track_segments(torch.zeros(10), [10], 0.5, 1, 1)       # a host tensor: there is no CPU path
    assert [x.size for x in ops.track_segments(t, [10], 0.5, 1, 1)[0]] == [1] * 5

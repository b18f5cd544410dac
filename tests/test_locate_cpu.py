"""The locating rule of whole-recording scoring (radhip.recordings.track_np / segments_np / segment_span, the numpy
statements the HIP kernels of csrc/locate.hip are compared against) on cases whose answer is written out here, a
brute-force per-sample restatement of the track, and the refusals of the scorer's constructor, of the numpy functions
and of the CLI parser. Host only."""
import numpy as np
import pytest

import main as cli
from radhip.recordings import (RecordingScorer, segment_span, segments_np, track_np, track_src_frames, trim_src,
                               window_table)

F, WIN = 320, 64600


def _brute(m, s, hop, win):
    """Per sample the windows that contain it; per frame sum_k ov s_k / sum_k ov with ov counted sample by sample."""
    _, start, _ = window_table([m], hop, win)
    nfy = -(-m // F)
    if m <= win:
        return np.full(nfy, float(s[0]))
    num, den = np.zeros(m), np.zeros(m)
    for a, sk in zip(start, s):
        num[a:a + win] += sk
        den[a:a + win] += 1
    assert den.min() >= 1
    out = np.empty(nfy)
    for j in range(nfy):
        out[j] = num[j * F:(j + 1) * F].sum() / den[j * F:(j + 1) * F].sum()
    return out


# ------------------------------------------------------------------------------------- track ----
@pytest.mark.parametrize("hop", [1, 333, 32300, 64600])
def test_the_two_worked_values(hop):
    s0, s1 = 0.75, -2.5
    t = track_np(64601, [s0, s1], hop)
    assert t.shape == (202,) and t.dtype == np.float64
    assert t[0] == pytest.approx((320 * s0 + 319 * s1) / 639, rel=1e-15)
    assert t[201] == pytest.approx((280 * s0 + 281 * s1) / 561, rel=1e-15)
    # every frame in between lies in both windows whole
    np.testing.assert_allclose(t[1:201], (s0 + s1) / 2, rtol=1e-15)


def test_constant_scores_give_a_constant_track():
    for m, hop in [(64601, 1), (100000, 3200), (700160, 333), (64920, 64600)]:
        n = window_table([m], hop)[2][1]
        t = track_np(m, np.full(n, 1.25), hop)
        assert t.shape == (-(-m // F),)
        np.testing.assert_allclose(t, 1.25, rtol=1e-15)


@pytest.mark.parametrize("m", [1, 319, 320, 321, 30000, 64600])
def test_a_recording_no_longer_than_a_window_has_its_one_score_everywhere(m):
    t = track_np(m, [-3.5], 32300)
    assert t.shape == (-(-m // F),) and (t == -3.5).all()


def test_one_frame_more_than_a_window():
    m, (s0, s1) = WIN + F, (2.0, -1.0)
    # windows at 0 and 320: frame 0 lies in the first alone, frame 202 in the second alone. 64 600 = 201 F + 280, so
    # frame 201 has 280 samples in the first window and all 320 in the second
    t = track_np(m, [s0, s1], 32300)
    assert t.shape == (203,)
    assert t[0] == s0 and t[202] == s1
    np.testing.assert_allclose(t[1:201], 0.5, rtol=1e-15)
    assert t[201] == pytest.approx((280 * s0 + 320 * s1) / 600, rel=1e-15)


def test_a_hop_that_is_no_multiple_of_the_frame():
    m, hop = WIN + 1000, 333
    _, start, _ = window_table([m], hop)
    assert start.tolist() == [0, 333, 666, 999, 1000]
    s = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    t = track_np(m, s, hop)
    # frame 1 = [320, 640): window 0 whole, window 1 from 333 (307 samples)
    assert t[1] == pytest.approx((320 * 1.0 + 307 * 2.0) / 627, rel=1e-15)
    # frame 3 = [960, 1280): windows 0 .. 2 whole, 999 -> 281 samples, 1000 -> 280 samples
    assert t[3] == pytest.approx((320 * (1 + 2 + 4) + 281 * 8.0 + 280 * 16.0) / (3 * 320 + 281 + 280), rel=1e-15)
    np.testing.assert_allclose(t, _brute(m, s, hop, WIN), rtol=1e-13)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_track_equals_the_per_sample_restatement(seed):
    rng = np.random.default_rng(seed)
    win = int(rng.choice([700, 1000, 6460]))
    for _ in range(6):
        m = int(rng.integers(1, 6 * win))
        hop = int(rng.integers(1, win + 1))
        n = int(window_table([m], hop, win)[2][1])
        s = rng.standard_normal(n)
        np.testing.assert_allclose(track_np(m, s, hop, win), _brute(m, s, hop, win), rtol=1e-12, atol=1e-14,
                                   err_msg=f"m {m} hop {hop} win {win}")


def test_track_refuses_a_wrong_number_of_scores():
    with pytest.raises(ValueError, match="windows"):
        track_np(64601, [1.0], 32300)
    with pytest.raises(ValueError, match="windows"):
        track_np(100, [1.0, 2.0], 32300)
    with pytest.raises(ValueError, match="hop"):
        track_np(100, [1.0], 0)
    with pytest.raises(ValueError, match="no samples"):
        track_np(0, [1.0], 32300)


# ---------------------------------------------------------------------------------- segments ----
def _segs(t, thr, merge, min_frames):
    a, b, mean, lo, arg = segments_np(np.asarray(t, dtype=np.float32), thr, merge, min_frames)
    assert a.dtype == b.dtype == arg.dtype == np.int64 and mean.dtype == np.float64 and lo.dtype == np.float32
    return list(zip(a.tolist(), b.tolist()))


def _track(*runs):
    """runs: (frames, value)."""
    return np.concatenate([np.full(n, v, dtype=np.float32) for n, v in runs])


def test_none_and_all_flagged():
    t = _track((10, 1.0))
    assert _segs(t, 1.0, 0, 1) == []            # strict: a value equal to the threshold is not flagged
    assert _segs(t, 0.0, 5, 1) == []
    assert _segs(t, 1.5, 0, 1) == [(0, 9)]
    assert _segs(t, 1.5, 0, 10) == [(0, 9)]
    assert _segs(t, 1.5, 0, 11) == []


def test_a_gap_of_merge_frames_is_bridged_and_one_more_is_not():
    merge = 3
    t = _track((2, 0.0), (merge, 1.0), (2, 0.0), (merge + 1, 1.0), (2, 0.0))
    assert _segs(t, 0.5, merge, 1) == [(0, 6), (11, 12)]
    assert _segs(t, 0.5, merge + 1, 1) == [(0, 12)]
    assert _segs(t, 0.5, 0, 1) == [(0, 1), (5, 6), (11, 12)]
    a, b, mean, lo, arg = segments_np(t, 0.5, merge, 1)
    # the bridged frames count in the mean; the minimum is first attained at the segment's first frame
    assert mean[0] == pytest.approx(3.0 / 7) and lo.tolist() == [0.0, 0.0] and arg.tolist() == [0, 11]


def test_a_run_of_min_frames_stays_and_one_frame_less_goes():
    n = 4
    t = _track((3, 1.0), (n, 0.0), (3, 1.0), (n - 1, 0.0), (3, 1.0))
    assert _segs(t, 0.5, 0, n) == [(3, 6)]
    assert _segs(t, 0.5, 0, n - 1) == [(3, 6), (10, 12)]
    # bridged first, measured after: the two runs and the gap make one segment of 10 frames
    assert _segs(t, 0.5, 3, 10) == [(3, 12)]
    assert _segs(t, 0.5, 3, 11) == []


def test_runs_at_the_ends_and_gaps_at_the_ends():
    t = _track((2, 0.0), (5, 1.0), (3, 0.0))
    assert _segs(t, 0.5, 0, 1) == [(0, 1), (7, 9)]
    # an unflagged run that touches frame 0 or the last frame is never closed, however large merge is
    t = _track((2, 1.0), (3, 0.0), (2, 1.0))
    assert _segs(t, 0.5, 100, 1) == [(2, 4)]
    t = _track((1, 1.0), (1, 0.0), (1, 1.0), (1, 0.0), (1, 1.0))
    assert _segs(t, 0.5, 100, 1) == [(1, 3)]
    assert _segs(t, 0.5, 0, 1) == [(1, 1), (3, 3)]


def test_merge_and_min_frames_larger_than_the_recording():
    t = _track((1, 0.0), (6, 1.0), (1, 0.0), (2, 1.0))
    assert _segs(t, 0.5, 5000, 1) == [(0, 7)]
    assert _segs(t, 0.5, 5000, 8) == [(0, 7)]
    assert _segs(t, 0.5, 5000, 9) == []
    assert _segs(t, 0.5, 0, 5000) == []


def test_stats_of_a_segment():
    t = np.array([5, 1, 3, 0.5, 4, 0.5, 9, 2, 9], dtype=np.float32)
    a, b, mean, lo, arg = segments_np(t, 4.5, 1, 2)
    assert (a.tolist(), b.tolist()) == ([1], [7])
    assert mean[0] == pytest.approx((1 + 3 + 0.5 + 4 + 0.5 + 9 + 2) / 7) and lo[0] == 0.5 and arg[0] == 3
    # a NaN is not flagged
    t[3] = np.nan
    a, b, *_ = segments_np(t, 4.5, 0, 1)
    assert (a.tolist(), b.tolist()) == ([1, 4, 7], [2, 5, 7])


# --------------------------------------------------------------------------------- positions ----
def test_source_positions_without_trimming():
    start, end = segment_span([0, 3, 200], [1, 3, 201], 64601)
    assert start.tolist() == [0, 960, 64000] and end.tolist() == [640, 1280, 64601]


def test_source_positions_with_hand_made_kept_ids():
    n = 20 * F + 7                                  # 21 source frames, the last of 7 samples
    ids = np.array([2, 3, 4, 9, 10, 20])            # frames 5 - 8 and 11 - 19 were dropped
    m = 5 * F + 7
    assert track_src_frames(ids, n, m) is not None
    start, end = segment_span([0, 2, 4, 5], [1, 3, 5, 5], n, ids)
    assert start.tolist() == [2 * F, 4 * F, 10 * F, 20 * F]
    # the second spans the dropped frames 5 - 8; the last two end with the recording, inside its partial last frame
    assert end.tolist() == [4 * F, 10 * F, n, n]
    # the same positions through trim_src, sample by sample
    assert start.tolist() == trim_src(ids, np.array([0, 2, 4, 5]) * F).tolist()
    last = np.minimum((np.array([1, 3, 5, 5]) + 1) * F, m) - 1
    assert end.tolist() == (trim_src(ids, last) + 1).tolist()


def test_a_partial_frame_before_the_last_kept_one_is_refused():
    n = 20 * F + 7
    with pytest.raises(AssertionError):
        track_src_frames([2, 20, 25], n, 2 * F + 7)         # frame 20 has 7 samples and is not the last kept
    with pytest.raises(AssertionError):
        track_src_frames([2, 3], n, 2 * F + 1)              # the length does not match the frames
    with pytest.raises(AssertionError):
        track_src_frames([3, 2], n, 2 * F)


# ----------------------------------------------------------------------------- argument errors ----
def test_segments_np_refuses_bad_arguments():
    t = np.zeros(4, dtype=np.float32)
    for bad in [dict(thr=np.nan), dict(thr=np.inf), dict(thr=1e39), dict(merge=-1), dict(merge=1.5),
                dict(min_frames=0), dict(min_frames=2.5)]:
        kw = dict(thr=0.5, merge=1, min_frames=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            segments_np(t, **kw)
    with pytest.raises(ValueError):
        segments_np(np.zeros(0, dtype=np.float32), 0.5, 1, 1)


def test_the_scorer_checks_the_new_arguments_before_anything_else():
    with pytest.raises(RuntimeError, match="no CPU path"):
        RecordingScorer(None, "cpu", track=True, segments=0.0)
    for bad in [dict(segments=float("nan")), dict(segments=float("inf")), dict(segments=1e39), dict(seg_merge=-1),
                dict(seg_merge=2.5), dict(seg_min=0), dict(seg_min=1.5)]:
        with pytest.raises(ValueError, match="seg"):
            RecordingScorer(None, "cuda", **bad)
    s = RecordingScorer(None, "cuda")
    assert (s.track, s.segments, s.seg_merge, s.seg_min) == (False, None, 10, 25)
    s = RecordingScorer(None, "cuda", track=True, segments=-1.5, seg_merge=0, seg_min=1)
    assert (s.track, s.segments, s.seg_merge, s.seg_min) == (True, -1.5, 0, 1)


@pytest.mark.parametrize("flags", [["--score_segments", "0.5"], ["--score_seg_merge", "3"], ["--score_seg_min", "3"],
                                   ["--score_track"]])
def test_cli_refuses_the_new_flags_without_score_files(flags, capsys):
    with pytest.raises(SystemExit):
        cli.parse_args(["--config", "x.conf"] + flags)
    assert "goes with --score_files" in capsys.readouterr().err


@pytest.mark.parametrize("flags", [["--score_segments", "nan"], ["--score_segments", "inf"],
                                   ["--score_seg_merge", "-1"], ["--score_seg_min", "0"]])
def test_cli_refuses_bad_values(flags, capsys):
    with pytest.raises(SystemExit):
        cli.parse_args(["--config", "x.conf", "--score_files", "l.txt", "--eval_model_weights", "w.pth"] + flags)
    assert "--score_seg" in capsys.readouterr().err


def test_cli_defaults_leave_the_options_off():
    a = cli.parse_args(["--config", "x.conf", "--score_files", "l.txt", "--eval_model_weights", "w.pth"])
    assert a.score_segments is None and a.score_track is False and a.score_seg_merge is None and a.score_seg_min is None
    a = cli.parse_args(["--config", "x.conf", "--score_files", "l.txt", "--eval_model_weights", "w.pth",
                        "--score_segments", "-0.25", "--score_seg_merge", "0", "--score_seg_min", "1", "--score_track"])
    assert (a.score_segments, a.score_seg_merge, a.score_seg_min, a.score_track) == (-0.25, 0, 1, True)

"""The silence-trimming rule of whole-recording scoring (radhip.recordings.trim_plan_np, the numpy statement the HIP
kernels are compared against) on hand-built signals whose answer is written out here, and the refusals of the
scorer's constructor and of the CLI parser. Host only."""
import numpy as np
import pytest

import main as cli
from radhip.recordings import (RecordingScorer, frame_energy_np, trim_apply_np, trim_plan_np, trim_src, window_table)

F = 320


def _sig(*parts):
    """parts: (frames, amplitude) runs, or (samples, amplitude, "samples")."""
    return np.concatenate([np.full(p[0] if len(p) == 3 else p[0] * F, p[1], dtype=np.float32) for p in parts])


def _plan(x, mode, db=40.0, pad=10):
    keep, ids, m = trim_plan_np(x, mode, db, pad)
    assert keep.dtype == bool and ids.dtype == np.int64 and keep.size == -(-x.size // F)
    assert ids.tolist() == np.nonzero(keep)[0].tolist() and m >= 1
    y = trim_apply_np(x, ids)
    assert y.size == m and y.dtype == x.dtype
    return ids.tolist(), m, y


@pytest.mark.parametrize("mode", ["ends", "gaps"])
def test_zeros_around_a_burst(mode):
    x = _sig((3, 0.0), (2, 0.5), (4, 0.0))
    ids, m, y = _plan(x, mode, pad=1)
    assert ids == [2, 3, 4, 5] and m == 4 * F
    np.testing.assert_array_equal(y, x[2 * F:6 * F])
    # pad = 0: the burst alone; a pad larger than the recording: everything
    assert _plan(x, mode, pad=0)[:2] == ([3, 4], 2 * F)
    ids, m, y = _plan(x, mode, pad=100)
    assert ids == list(range(9)) and m == x.size
    np.testing.assert_array_equal(y, x)


def test_gap_of_twice_the_pad_stays_and_one_more_frame_loses_its_middle():
    pad = 2
    whole = _sig((1, 0.5), (2 * pad, 0.0), (1, 0.5))
    assert _plan(whole, "gaps", pad=pad)[:2] == (list(range(6)), 6 * F)
    longer = _sig((1, 0.5), (2 * pad + 1, 0.0), (1, 0.5))
    ids, m, y = _plan(longer, "gaps", pad=pad)
    assert ids == [0, 1, 2, 4, 5, 6] and m == 6 * F
    np.testing.assert_array_equal(y, np.concatenate([longer[:3 * F], longer[4 * F:]]))
    # "ends" never cuts an inner pause
    assert _plan(longer, "ends", pad=pad)[:2] == (list(range(7)), 7 * F)
    assert _plan(_sig((1, 0.5), (50, 0.0), (1, 0.5)), "ends", pad=0)[:2] == (list(range(52)), 52 * F)
    assert _plan(_sig((1, 0.5), (50, 0.0), (1, 0.5)), "gaps", pad=0)[:2] == ([0, 51], 2 * F)


@pytest.mark.parametrize("mode", ["ends", "gaps"])
def test_all_zeros_is_not_trimmed(mode):
    x = np.zeros(5 * F + 7, dtype=np.float32)
    ids, m, y = _plan(x, mode, pad=0)
    assert ids == list(range(6)) and m == x.size and not y.any()


@pytest.mark.parametrize("n,nf", [(1, 1), (319, 1), (320, 1), (321, 2)])
@pytest.mark.parametrize("mode", ["ends", "gaps"])
def test_lengths_around_one_frame(n, nf, mode):
    x = np.full(n, 0.25, dtype=np.float32)
    e = frame_energy_np(x)
    assert e.tolist() == [0.0625] * nf          # a partial frame is divided by its own count
    ids, m, y = _plan(x, mode, pad=0)
    assert ids == list(range(nf)) and m == n
    np.testing.assert_array_equal(y, x)


def test_partial_last_frame_as_the_peak():
    x = _sig((2, 0.1), (1, 1.0, "samples"))
    assert x.size == 2 * F + 1
    np.testing.assert_allclose(frame_energy_np(x), [0.01, 0.01, 1.0], rtol=1e-6)
    # 10 dB below the one-sample frame's energy of 1 is 0.1: the two full frames (0.01) are silent
    for mode in ("ends", "gaps"):
        ids, m, y = _plan(x, mode, db=10.0, pad=0)
        assert ids == [2] and m == 1 and y.tolist() == [1.0]
        assert _plan(x, mode, db=10.0, pad=1)[:2] == ([1, 2], F + 1)
        assert _plan(x, mode, db=30.0, pad=0)[:2] == ([0, 1, 2], 2 * F + 1)     # 0.01 >= 0.001


def test_threshold_is_relative_to_the_loudest_frame():
    x = _sig((2, 10 ** -2.5), (1, 1.0), (2, 10 ** -2.5))          # a floor 50 dB under the burst
    assert _plan(x, "gaps", db=40.0, pad=0)[0] == [2]
    assert _plan(x, "gaps", db=60.0, pad=0)[0] == [0, 1, 2, 3, 4]
    assert _plan(0.01 * x, "gaps", db=40.0, pad=0)[0] == [2]      # the absolute level does not matter


def test_source_positions():
    x = np.arange(7 * F + 5, dtype=np.float32)                   # a sample's value is its position
    x[3 * F:4 * F] = 0.0
    x[:F] = 0.0
    ids = np.array([1, 2, 4, 5, 6, 7])
    y = trim_apply_np(x, ids)
    m = y.size
    assert m == 5 * F + 5
    assert trim_src(ids, 0) == F and trim_src(ids, m - 1) == 7 * F + 4             # first and last sample
    assert trim_src(ids, [2 * F - 1, 2 * F]).tolist() == [3 * F - 1, 4 * F]        # around the cut
    p = np.arange(m)
    np.testing.assert_array_equal(x[trim_src(ids, p)], y)
    # the windows of the trimmed signal, as the scorer reports them: starts and one-past-the-end in the source
    rec, start, seg = window_table([m], 600, win=1000)
    stop = np.minimum(start + 1000, m) - 1
    assert start.tolist() == [0, 600, 605]
    assert trim_src(ids, start).tolist() == [F, 2 * F + 280, 2 * F + 285]
    assert (trim_src(ids, stop) + 1).tolist() == [5 * F + 40, 7 * F, 7 * F + 5]    # the first spans the cut


def test_rule_refuses_bad_arguments():
    x = np.ones(10, dtype=np.float32)
    for kw in ({"mode": "middle"}, {"mode": "gaps", "db": 0.0}, {"mode": "ends", "pad": -1}):
        with pytest.raises(ValueError):
            trim_plan_np(x, **kw)
    with pytest.raises(ValueError):
        frame_energy_np(np.zeros(0, dtype=np.float32))


@pytest.mark.parametrize("kw", [{"trim": "middle"}, {"trim": "gaps", "trim_db": 0.0}, {"trim": "ends", "trim_db": -3},
                                {"trim": "gaps", "trim_pad": -1}, {"trim": "gaps", "trim_pad": 1.5},
                                {"trim_db": float("nan")}])
def test_constructor_refuses_bad_trim_values(kw):
    with pytest.raises(ValueError, match="trim"):
        RecordingScorer(None, "cuda", **kw)


def test_constructor_defaults():
    s = RecordingScorer(None, "cuda")
    assert (s.trim, s.trim_db, s.trim_pad) == (None, 40.0, 10)
    s = RecordingScorer(None, "cuda", trim="gaps", trim_db=30, trim_pad=0)
    assert (s.trim, s.trim_db, s.trim_pad) == ("gaps", 30.0, 0)


def test_cli_trim_flags_parse():
    base = ["--config", "c.conf"]
    score = base + ["--score_files", "list.txt", "--eval_model_weights", "w.pth"]
    a = cli.parse_args(score)
    assert (a.score_trim, a.score_trim_db, a.score_trim_pad) == (None, None, None)
    a = cli.parse_args(score + ["--score_trim", "gaps", "--score_trim_db", "30", "--score_trim_pad", "0"])
    assert (a.score_trim, a.score_trim_db, a.score_trim_pad) == ("gaps", 30.0, 0)
    assert cli.parse_args(score + ["--score_trim", "ends"]).score_trim == "ends"
    for bad in (base + ["--score_trim", "gaps"], base + ["--score_trim_db", "30"], base + ["--score_trim_pad", "3"],
                score + ["--score_trim", "middle"], score + ["--score_trim", "gaps", "--score_trim_db", "0"],
                score + ["--score_trim", "gaps", "--score_trim_db", "-1"],
                score + ["--score_trim", "gaps", "--score_trim_pad", "-1"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)

"""The window rule of whole-recording scoring (radhip.recordings.window_table) and the CLI flags, on the host."""
import numpy as np
import pytest

import main as cli
from oracle.data import pad
from radhip.recordings import _chunks, window_samples, window_table

WIN = 64600


def _cases():
    for hop in (64600, 32300, 16150):
        for n in (1, 2, 64599, 64600, 64601, 64600 + hop - 1, 64600 + hop, 64600 + hop + 1, 3 * 64600 + 7):
            yield n, hop
    yield 64601, 7
    yield 64700, 7


@pytest.mark.parametrize("n,hop", sorted(set(_cases())))
def test_window_rule(n, hop):
    rec, start, seg = window_table([n], hop)
    assert rec.dtype == start.dtype == seg.dtype == np.int64
    count = 1 if n <= WIN else 1 + -(-(n - WIN) // hop)
    assert seg.tolist() == [0, count] and rec.tolist() == [0] * count and start.size == count
    if n <= WIN:
        assert start.tolist() == [0]
        return
    assert (np.diff(start) > 0).all()
    assert start[:-1].tolist() == [k * hop for k in range(count - 1)]
    assert start[-1] == n - WIN
    covered = np.zeros(n, dtype=bool)
    for s in start:
        assert 0 <= s and s + WIN <= n
        covered[s:s + WIN] = True
    assert covered.all()


@pytest.mark.parametrize("n", [1, 2, 3, 64599, 64600])
def test_short_recording_is_the_eval_pad(n):
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    np.testing.assert_array_equal(window_samples(x, 0), pad(x))


def test_long_recording_windows_are_plain_slices():
    x = np.arange(100000, dtype=np.float32)
    _, start, _ = window_table([x.size], 32300)
    assert start.tolist() == [0, 32300, 35400]
    for s in start:
        np.testing.assert_array_equal(window_samples(x, s), x[s:s + WIN])


def test_table_of_several_recordings():
    lens = [30000, 64600, 64601, 100000, 200000]
    rec, start, seg = window_table(lens, 32300)
    assert seg.tolist() == [0, 1, 2, 4, 7, 13]
    assert rec.tolist() == [0, 1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 4]
    assert start.tolist() == [0, 0, 0, 1, 0, 32300, 35400, 0, 32300, 64600, 96900, 129200, 135400]
    # a small window, as the kernel test uses it
    rec, start, seg = window_table([1, 3, 39, 40, 41, 56, 57, 121], 16, win=40)
    assert np.diff(seg).tolist() == [1, 1, 1, 1, 2, 2, 3, 7]
    assert start[seg[6]:seg[7]].tolist() == [0, 16, 17] and start[-1] == 81


@pytest.mark.parametrize("hop", [0, -1, 64601])
def test_bad_hop_is_rejected(hop):
    with pytest.raises(ValueError, match="hop"):
        window_table([70000], hop)


def test_empty_recording_is_named():
    with pytest.raises(ValueError, match="b.flac"):
        window_table([5, 0, 7], 32300, names=["a.flac", "b.flac", "c.flac"])
    with pytest.raises(ValueError, match="recording 1"):
        window_table([5, 0, 7], 32300)


def test_chunks_respect_the_cap_and_keep_order():
    assert list(_chunks([4, 4, 4, 9, 1, 1], 8)) == [(0, 2), (2, 3), (3, 4), (4, 6)]
    assert list(_chunks([], 8)) == []
    assert list(_chunks([3], 8)) == [(0, 1)]


def test_cli_flags_parse():
    a = cli.parse_args(["--config", "c.conf"])
    assert (a.score_files, a.score_hop, a.score_reduce, a.score_timeline) == (None, 32300, "mean", False)
    a = cli.parse_args(["--config", "c.conf", "--score_files", "list.txt", "--eval_model_weights", "w.pth",
                        "--score_hop", "16150", "--score_reduce", "min", "--score_timeline"])
    assert (a.score_files, a.score_hop, a.score_reduce, a.score_timeline) == ("list.txt", 16150, "min", True)
    with pytest.raises(SystemExit):
        cli.parse_args(["--config", "c.conf", "--score_files", "list.txt"])                 # no weights
    with pytest.raises(SystemExit):
        cli.parse_args(["--config", "c.conf", "--score_files", "l", "--eval_model_weights", "w", "--score_hop", "0"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--config", "c.conf", "--score_files", "l", "--eval_model_weights", "w", "--score_reduce",
                        "median"])

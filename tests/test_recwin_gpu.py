"""csrc/recwin.hip on the GPU: rdx_window_gather against its numpy restatement (a copy: equality is the bound) and
rdx_segment_reduce against fp64 on the host."""
import numpy as np
import pytest
import torch

from radhip.recordings import window_samples, window_table

pytestmark = pytest.mark.gpu


def _packed(lens, seed):
    """Recordings packed back to back, so most of them start at an odd, unaligned element offset."""
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return xs, offs, torch.from_numpy(np.concatenate(xs)).cuda()


def _expected(xs, rec, start, win):
    return np.stack([window_samples(xs[r], s, win) for r, s in zip(rec, start)])


@pytest.mark.parametrize("win,hop,lens", [(40, 16, [1, 3, 39, 40, 41, 56, 57, 121]),
                                          (64600, 32300, [30000, 64600, 64601, 100000])])
def test_gather_is_bit_exact(win, hop, lens):
    from radhip.ops import window_gather
    xs, offs, flat = _packed(lens, seed=win)
    assert (offs % 4 != 0).any()
    rec, start, _ = window_table(lens, hop, win)
    out = window_gather(flat, offs, lens, rec, start, win)
    np.testing.assert_array_equal(out.cpu().numpy(), _expected(xs, rec, start, win))
    # the table in another recording order, and a single window, into a caller's buffer
    order = np.random.default_rng(1).permutation(rec.size)
    assert (np.diff(rec[order]) < 0).any()
    out = window_gather(flat, offs, lens, rec[order], start[order], win)
    np.testing.assert_array_equal(out.cpu().numpy(), _expected(xs, rec[order], start[order], win))
    buf = torch.full((3, win), -7.0, device="cuda")
    window_gather(flat, offs, lens, rec[-1:], start[-1:], win, out=buf[1:2])
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[1], _expected(xs, rec[-1:], start[-1:], win)[0])
    assert (got[0] == -7.0).all() and (got[2] == -7.0).all()        # nothing written outside the row


def test_gather_more_windows_than_one_launch_holds():
    """130 windows: the entry cuts the table into launches of 64."""
    from radhip.ops import window_gather
    lens = [40 + 16 * 128, 7]
    xs, offs, flat = _packed(lens, seed=3)
    rec, start, seg = window_table(lens, 16, 40)
    assert rec.size == 130
    out = window_gather(flat, offs, lens, rec, start, 40)
    np.testing.assert_array_equal(out.cpu().numpy(), _expected(xs, rec, start, 40))


SEGS = [1, 2, 63, 64, 65, 257]


def test_segment_reduce_against_fp64():
    from radhip.ops import segment_reduce
    rng = np.random.default_rng(11)
    seg = np.concatenate([[0], np.cumsum(SEGS)]).astype(np.int64)
    s = (3.0 * rng.standard_normal(seg[-1])).astype(np.float32)
    # a constructed tie: the minimum of the 65-window segment sits at 9 and again at 40 and at 64 (another lane, and the
    # lane of index 0 one round later); of the 257-window segment at 70 and 200
    a, b = seg[4], seg[5]
    s[a + 9] = s[a + 40] = s[a + 64] = s[a:a + 65].min() - 1.0
    s[b + 70] = s[b + 200] = s[b:b + 257].min() - 1.0
    dev = torch.from_numpy(s).cuda()
    mean, lo, hi, arg = (t.cpu().numpy() for t in segment_reduce(dev, seg))
    again = [t.cpu().numpy() for t in segment_reduce(dev, seg)]
    for r, n in enumerate(SEGS):
        x = s[seg[r]:seg[r + 1]]
        bound = (n - 1) * 2.0 ** -24 * float(np.abs(x).max())
        err = abs(float(mean[r]) - float(x.astype(np.float64).mean()))
        print(f"n={n}: |mean - mean64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (n, err, bound)
        assert lo[r] == x.min() and hi[r] == x.max()
        assert arg[r] == int(np.argmin(x))                          # numpy: the first occurrence
    assert arg[4] == 9 and arg[5] == 70
    for got, rep in zip((mean, lo, hi, arg), again):
        assert got.tobytes() == rep.tobytes()
    # one segment alone gives the bits it gave inside the larger launch
    m1, l1, h1, a1 = segment_reduce(dev[seg[5]:seg[6]].contiguous(), [0, 257])
    assert m1.cpu().numpy().tobytes() == mean[5:6].tobytes() and int(a1) == 70


def test_bad_arguments_are_errors_not_faults():
    from radhip import _lib
    from radhip.ops import segment_reduce, window_gather
    L, I64 = _lib.lib(), _lib.c_i64 * 1
    flat = torch.zeros(256, device="cuda")
    out = torch.zeros(1, 40, device="cuda")
    one, zero = I64(0), I64(0)
    ln = I64(100)
    ok = (flat.data_ptr(), one, ln, zero, zero, 1, 40, out.data_ptr(), None)
    _lib.check(L.rdx_window_gather(*ok), "window_gather")
    for i in (0, 1, 2, 3, 4, 7):                                    # each pointer null in turn
        bad = list(ok)
        bad[i] = None
        with pytest.raises(RuntimeError, match="invalid argument"):
            _lib.check(L.rdx_window_gather(*bad), "window_gather")
    with pytest.raises(RuntimeError, match="invalid argument"):     # nwin = 0
        _lib.check(L.rdx_window_gather(*ok[:5], 0, 40, out.data_ptr(), None), "window_gather")
    with pytest.raises(RuntimeError, match="invalid argument"):     # out off the 16-byte grid
        window_gather(flat, [0], [100], [0], [0], 40, out=torch.zeros(44, device="cuda")[1:41].view(1, 40))
    with pytest.raises(RuntimeError, match="invalid argument"):     # a window past its recording's end
        _lib.check(L.rdx_window_gather(*ok[:4], I64(61), 1, 40, out.data_ptr(), None), "window_gather")
    with pytest.raises(RuntimeError, match="unsupported shape"):    # rows that a dwordx4 store would straddle
        _lib.check(L.rdx_window_gather(*ok[:6], 42, out.data_ptr(), None), "window_gather")
    with pytest.raises(ValueError):                                 # a recording outside the packed buffer
        window_gather(flat, [200], [100], [0], [0], 40)
    sc = torch.zeros(8, device="cuda")
    sg = torch.tensor([0, 8], device="cuda")
    f = torch.zeros(3, device="cuda")
    am = torch.zeros(1, dtype=torch.int64, device="cuda")
    ok = (sc.data_ptr(), sg.data_ptr(), 1, f[0:].data_ptr(), f[1:].data_ptr(), f[2:].data_ptr(), am.data_ptr(), None)
    _lib.check(L.rdx_segment_reduce(*ok), "segment_reduce")
    for i in (0, 1, 3, 4, 5, 6):
        bad = list(ok)
        bad[i] = None
        with pytest.raises(RuntimeError, match="invalid argument"):
            _lib.check(L.rdx_segment_reduce(*bad), "segment_reduce")
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.check(L.rdx_segment_reduce(*ok[:2], 0, *ok[3:]), "segment_reduce")
    with pytest.raises(ValueError):                                 # an empty segment, a segment past the scores
        segment_reduce(sc, [0, 4, 4, 8])
    with pytest.raises(ValueError):
        segment_reduce(sc, [0, 9])
    torch.cuda.synchronize()

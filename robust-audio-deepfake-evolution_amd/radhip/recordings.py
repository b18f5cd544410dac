"""Scoring whole recordings of any length: "which of these files are spoofed, and where?".

The trial-list scorer (radhip/infer.py, radhip/data.py) feeds the model the reference's `pad` of every file: its first
64 600 samples, or the file tiled to that length. Here a recording is covered by windows of 64 600 samples instead,
every window is scored by the unchanged model forward, and the window scores are reduced to one record per recording.

The window rule (`window_table`, the only statement of it):
  * len <= win: one window at start 0, filled as `pad` fills it (head crop at len == win, else x[i % len]), so a file
    of ASVspoof length gets exactly the samples the eval path feeds the model;
  * len >  win: n = 1 + ceil((len - win) / hop) windows, starts k * hop for k < n - 1 and len - win for the last,
    which therefore ends flush with the recording. Every sample lies in a window; nothing is tiled or zero-padded;
  * len == 0: an error that names the recording.

Data path: recordings are decoded by the native batch reader into one packed pinned buffer (radhip.audio.read_batch),
uploaded in one copy, cut into model inputs on the device by rdx_window_gather, scored through radhip.infer._scores
and reduced on the device by rdx_segment_reduce (csrc/recwin.hip). There is no CPU path.

With convert=True a recording may have any integer sample rate and channel count (.flac or .wav): the chunk is
uploaded as it was decoded, interleaved, and rdx_ingest_resample (csrc/ingest.hip) writes its channel mean, resampled
to 16 kHz by the filter the training augmentation uses, into the packed buffer the window gather reads. The window
rule then applies to the converted signal: every length and window start in a record is in 16 kHz samples.

The trimming rule (trim="ends" or "gaps", off by default; `trim_plan_np` restates it in numpy, csrc/trim.hip runs
it on the packed chunk between the conversion and the window gather). It applies to one 16 kHz mono signal x of
length n, the converted one under convert=True, with trim_db > 0 and trim_pad >= 0 frames:
  * frames: F = 320 samples (20 ms), not overlapping, nf = ceil(n / F); frame f covers [f F, min((f + 1) F, n)), so
    only the last can be partial; e[f] is the mean of x^2 over the samples the frame really has;
  * active: peak = max_f e[f]; active[f] = e[f] > 0 and e[f] >= peak 10^(-trim_db / 10). If no frame is active (an
    all-zero signal) nothing is trimmed;
  * kept, "gaps": keep[f] iff some active frame lies in [f - trim_pad, f + trim_pad]: an inactive run of at most
    2 trim_pad frames between active frames stays whole, a longer one loses its middle;
  * kept, "ends": keep[f] iff first_active - trim_pad <= f <= last_active + trim_pad: inner pauses are never cut;
  * output: y = the kept frames in order, no cross-fade, m = len(y) >= 1; kept_ids = their source frame numbers;
  * positions: only the last kept frame can be partial, so sample p of y is source sample
    src(p) = kept_ids[p // F] F + p % F (`trim_src`);
  * windows: the window rule then applies to y unchanged, the tiling of a y no longer than a window included.

The locating rule (track=True, segments=thr; off by default; `track_np` and `segments_np` restate it in float64 numpy,
csrc/locate.hip runs it on the window scores of the whole list). y is the scored signal of one recording, of length
m: the trimmed signal when trimming is on, otherwise the 16 kHz signal. Its windows are those of the window rule,
starts a_k and fp32 scores s_k for k < n. F = 320 as above; the frames of y are nfy = ceil(m / F), frame j spans
[j F, min((j + 1) F, m)), so only the last can be partial.
  * track: m <= win (one tiled window): t[j] = s_0 for every j. m > win: ov(k, j) = the samples of frame j's span
    inside [a_k, a_k + win), an integer in 0 .. 320, and t[j] = sum_k ov(k, j) s_k / sum_k ov(k, j), summed over k
    ascending. Every sample lies in a window, so the denominator is at least the frame's own length. The weights are
    the plain overlap counts, there is no taper. (m = 64 601, two windows at 0 and 1, 202 frames:
    t[0] = (320 s_0 + 319 s_1) / 639 and t[201] = (280 s_0 + 281 s_1) / 561, frame 201 spanning [64 320, 64 601).)
  * segments, on the fp32 track with an fp32 thr, merge >= 0 and min_frames >= 1: flag[j] = t[j] < thr, strictly
    (scores are bona-fide logits or cosines: lower is more spoof-like); closed[j] = flag[j], or j lies in an unflagged
    run of at most `merge` frames that has a flagged frame immediately on both sides (a run that touches either end
    of the recording is never closed); a segment is a maximal run [a, b] of closed frames with
    b - a + 1 >= min_frames. Per segment: frames = b - a + 1, the mean of t[a .. b] (bridged frames included), the
    min, and argmin = the first frame that attains it;
  * positions are reported in the untrimmed 16 kHz signal of length N: track frame j is source frame j without
    trimming and source frame kept_ids[j] with it (exact, because only the last kept frame can be partial:
    `track_src_frames`). A segment has start = srcframe(a) F and end = min((srcframe(b) + 1) F, N). In "gaps" mode a
    segment may span dropped silence, as window_ends may: it is not split, and `frames` says how many were scored.
The model is trained on whole utterances, so the track is nothing finer than the 4 s window scores spread over the
frames they cover: its resolution is set by hop and win, not by the 20 ms frame.
"""
import numpy as np
import torch

from . import audio
from .data import CUT, _PinnedBuf
from .infer import _scores
from .ops import (TRIM_FRAME, TRIM_MODES, IngestTables, ingest_out_len, ingest_resample, score_track, segment_reduce,
                  track_segments, trim_silence, window_gather)

SAMPLE_RATE = 16000
# Packed samples resident per chunk of recordings: 2^24 fp32 samples = 64 MiB on the host (pinned) and on the device,
# about 17 minutes of audio. A chunk always holds at least one recording, so a single longer recording is the only
# way past the cap.
CHUNK_SAMPLES = 1 << 24
AMP = {None: None, "fp32": None, "x3": "x3", "bf16": torch.bfloat16, "fp16": torch.float16}
REDUCE = ("mean", "min", "max")


def window_table(lens, hop, win=CUT, names=None):
    """(rec[int64 W], start[int64 W], seg[int64 n + 1]): window w covers recording rec[w] from sample start[w], and
    recording r owns windows seg[r] .. seg[r + 1]. 1 <= hop <= win. `names` only words the zero-length error."""
    hop, win = int(hop), int(win)
    if win < 1 or not 1 <= hop <= win:
        raise ValueError(f"window_table: need 1 <= hop <= win, got hop {hop}, win {win}")
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    bad = np.nonzero(lens <= 0)[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"{names[i] if names is not None else f'recording {i}'}: no samples to score "
                         f"(length {int(lens[i])})")
    count = np.where(lens <= win, 1, 1 - (-(lens - win) // hop))
    seg = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(count, out=seg[1:])
    rec = np.repeat(np.arange(lens.size, dtype=np.int64), count)
    k = np.arange(rec.size, dtype=np.int64) - seg[rec]
    start = np.where(lens[rec] <= win, 0, np.minimum(k * hop, lens[rec] - win)).astype(np.int64)
    return rec, start, seg


def window_samples(x, start, win=CUT):
    """The numpy restatement of one window of recording x (what rdx_window_gather writes for it)."""
    x = np.asarray(x)
    n = x.shape[0]
    if n <= win:
        return x[np.arange(win) % n]
    return x[start:start + win]


def frame_energy_np(x):
    """float64 [ceil(n / 320)]: the mean of x^2 over the samples each frame really has (what rdx_trim_energy
    computes in fp32)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    if n == 0:
        raise ValueError("frame_energy_np: no samples")
    nf = -(-n // TRIM_FRAME)
    sq = np.zeros(nf * TRIM_FRAME, dtype=np.float64)
    sq[:n] = x * x
    count = np.minimum(TRIM_FRAME, n - TRIM_FRAME * np.arange(nf, dtype=np.int64))
    return sq.reshape(nf, TRIM_FRAME).sum(axis=1) / count


def trim_plan_np(x, mode, db=40.0, pad=10):
    """The numpy restatement of the trimming rule, in float64: (keep bool [nf], kept_ids int64, m), m = the length
    of the trimmed signal (what rdx_trim_plan decides for one recording)."""
    if mode not in TRIM_MODES:
        raise ValueError(f"trim mode {mode!r} is not one of {sorted(TRIM_MODES)}")
    if not db > 0 or pad < 0:
        raise ValueError(f"trim_plan_np: need db > 0 and pad >= 0, got db {db}, pad {pad}")
    e = frame_energy_np(x)
    n, nf, pad = np.asarray(x).size, e.size, int(pad)
    active = (e > 0) & (e >= e.max() * 10.0 ** (-float(db) / 10.0))
    f = np.arange(nf, dtype=np.int64)
    if not active.any():
        keep = np.ones(nf, dtype=bool)
    elif mode == "gaps":
        before = np.concatenate([[0], np.cumsum(active)])       # before[k]: active frames among the first k
        keep = before[np.minimum(f + pad + 1, nf)] - before[np.maximum(f - pad, 0)] > 0
    else:
        on = np.nonzero(active)[0]
        keep = (f >= on[0] - pad) & (f <= on[-1] + pad)
    kept_ids = np.nonzero(keep)[0].astype(np.int64)
    m = int(np.minimum(TRIM_FRAME, n - TRIM_FRAME * kept_ids).sum())
    return keep, kept_ids, m


def trim_apply_np(x, kept_ids):
    """y: the kept frames of x in order (what rdx_trim_compact writes for one recording)."""
    x = np.asarray(x).reshape(-1)
    idx = (TRIM_FRAME * np.asarray(kept_ids, dtype=np.int64)[:, None] + np.arange(TRIM_FRAME)).reshape(-1)
    return x[idx[idx < x.size]]


def trim_src(kept_ids, p):
    """src(p): the source sample of sample(s) p of the trimmed signal."""
    p = np.asarray(p, dtype=np.int64)
    return np.asarray(kept_ids, dtype=np.int64)[p // TRIM_FRAME] * TRIM_FRAME + p % TRIM_FRAME


def track_src_frames(kept_ids, n, m):
    """kept_ids, as the source frame of every frame of the trimmed signal of length m cut from a signal of length n.
    Frame j of the trimmed signal is exactly source frame kept_ids[j], because a kept frame other than the last is
    whole: only the source's last frame can be partial, and it can only be kept last. Asserted here."""
    ids = np.asarray(kept_ids, dtype=np.int64)
    assert ids.size >= 1 and (np.diff(ids) > 0).all() and ((ids[:-1] + 1) * TRIM_FRAME <= n).all(), \
        "a kept frame before the last is partial"
    assert m == (ids.size - 1) * TRIM_FRAME + min(TRIM_FRAME, n - int(ids[-1]) * TRIM_FRAME), (m, n, ids.size)
    return ids


def track_np(m, scores, hop, win=CUT):
    """The numpy restatement of the track rule, in float64: t [ceil(m / 320)] of one scored signal of length m whose
    windows (window_table([m], hop, win)) have `scores` (what rdx_track_overlap computes in fp32)."""
    m = int(m)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    _, start, _ = window_table([m], hop, win)
    if s.size != start.size:
        raise ValueError(f"track_np: {s.size} scores for the {start.size} windows of {m} samples at hop {hop}")
    nfy = -(-m // TRIM_FRAME)
    if m <= win:
        return np.full(nfy, s[0])
    num, den = np.zeros(nfy, dtype=np.float64), np.zeros(nfy, dtype=np.int64)
    for a, sk in zip(start.tolist(), s.tolist()):       # k ascending
        j = np.arange(a // TRIM_FRAME, (a + win - 1) // TRIM_FRAME + 1, dtype=np.int64)
        ov = np.minimum(np.minimum((j + 1) * TRIM_FRAME, m), a + win) - np.maximum(j * TRIM_FRAME, a)
        num[j] += ov * sk
        den[j] += ov
    return num / den


def segments_np(t, thr, merge=10, min_frames=25):
    """The numpy restatement of the segment rule on one fp32 track: (a, b, mean, min, argmin), one entry per segment:
    first and last frame (int64), the float64 mean and the fp32 minimum of t[a .. b] and the first frame that attains
    it (what rdx_track_segments and rdx_track_segment_stats compute for one recording)."""
    t = np.asarray(t, dtype=np.float32).reshape(-1)
    with np.errstate(over="ignore"):
        thr32 = np.float32(thr)
    if t.size == 0 or not np.isfinite(thr32):
        raise ValueError(f"segments_np: need a track of one frame at least and a finite threshold, got {thr}")
    if int(merge) != merge or merge < 0 or int(min_frames) != min_frames or min_frames < 1:
        raise ValueError(f"segments_np: need whole merge >= 0 and min_frames >= 1, got {merge}, {min_frames}")
    nf = t.size

    def runs(mask):     # [first, last + 1) of every maximal run of True
        d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
        return np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    flag = t < thr32
    u0, u1 = runs(~flag)
    ok = (u0 > 0) & (u1 < nf) & (u1 - u0 <= merge)
    delta = np.zeros(nf + 1, dtype=np.int64)
    delta[u0[ok]] += 1
    delta[u1[ok]] -= 1
    closed = flag | (np.cumsum(delta[:-1]) > 0)
    a, e = runs(closed)
    keep = e - a >= min_frames
    a, b = a[keep].astype(np.int64), e[keep].astype(np.int64) - 1
    mean = np.array([t[x:y + 1].astype(np.float64).mean() for x, y in zip(a, b)], dtype=np.float64)
    lo = np.array([t[x:y + 1].min() for x, y in zip(a, b)], dtype=np.float32)
    arg = np.array([x + int(np.argmin(t[x:y + 1])) for x, y in zip(a, b)], dtype=np.int64)
    return a, b, mean, lo, arg


def segment_span(a, b, n_source, kept_ids=None):
    """(start, end) of segments [a, b] (track frames) as sample positions in the untrimmed signal of n_source
    samples: start = srcframe(a) F, end = min((srcframe(b) + 1) F, n_source), srcframe(j) = j, or kept_ids[j] under
    trimming."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if kept_ids is not None:
        ids = np.asarray(kept_ids, dtype=np.int64)
        a, b = ids[a], ids[b]
    return a * TRIM_FRAME, np.minimum((b + 1) * TRIM_FRAME, int(n_source))


def _chunks(lens, cap):
    """[i0, i1) runs of recordings whose packed samples stay within cap (one recording at least)."""
    i0, total = 0, 0
    for i, n in enumerate(lens):
        if i > i0 and total + n > cap:
            yield i0, i
            i0, total = i, 0
        total += int(n)
    if len(lens) > i0:
        yield i0, len(lens)


def _chunks_convert(raw, lens, cap):
    """_chunks under two caps: [i0, i1) runs whose raw interleaved floats and whose converted samples both stay
    within cap (one recording at least)."""
    i0, a, b = 0, 0, 0
    for i, (r, n) in enumerate(zip(raw, lens)):
        if i > i0 and (a + r > cap or b + n > cap):
            yield i0, i
            i0, a, b = i, 0, 0
        a, b = a + int(r), b + int(n)
    if len(lens) > i0:
        yield i0, len(lens)


def converted_lengths(frames, rates):
    """The 16 kHz length of every recording: ceil(16000 * frames / rate), what rdx_ingest_resample writes."""
    return np.array([ingest_out_len(f, r, SAMPLE_RATE) for f, r in zip(frames, rates)], dtype=np.int64)


class RecordingScorer:
    """One record per recording: {name, n_samples, n_windows, score, min, max, argmin_start} and, with
    timeline=True, window_starts / window_scores. The score of a window is the bona-fide logit (or the OC-Softmax
    cosine when `criterion` carries a centre), so `min` is the most spoof-like window and `argmin_start` the sample
    at which it starts; `score` is the mean, min or max of the windows according to `reduce`.

    The windows of all recordings, in input order, are cut into batches of `batch_size`: short and long recordings
    share batches and only the last batch is partial. Recordings are read, uploaded and cut in chunks of at most
    CHUNK_SAMPLES (2^24) packed samples, 64 MiB of pinned host memory and as much device memory, however long the
    list is; a batch may straddle two chunks. What grows with the list is one fp32 score per window and the records.

    amp: "x3" (default, the scorer of main.py --eval), "fp32", "bf16" or "fp16", as radhip.infer._scores takes them.

    convert=True: recordings of any integer sample rate and channel count, .flac or .wav, are down-mixed (channel
    mean) and resampled to 16 kHz on the device first (rdx_ingest_resample). n_samples, window_starts and
    argmin_start are then in 16 kHz samples, and every record also carries source_rate, source_channels and
    source_frames. A chunk holds at most CHUNK_SAMPLES floats both as decoded and as converted. A recording that is
    already mono 16 kHz is copied, not filtered. The tap tables are built once per source rate and stay on the device.

    trim="ends" or "gaps" (None: off): the silent frames of every recording are dropped on the device first, by the
    trimming rule in this module's docstring with trim_db (> 0) and trim_pad (frames, >= 0), after the conversion
    when convert=True. The windows then cover the trimmed signal: n_samples is its length, and every record also
    carries untrimmed_samples (the 16 kHz length before trimming) and kept_frames. argmin_start and window_starts
    stay positions in the untrimmed 16 kHz signal, src(start), and with timeline=True window_ends gives
    src(last sample the window covers) + 1: in "gaps" mode a window can span more than `win` source samples. The
    window table is built chunk by chunk, from the trimmed lengths that come back from the device (one copy of the
    plan per chunk).

    track=True and segments=thr (a float; None: off) locate the spoofed parts by the locating rule in this module's
    docstring, on the device, once the window scores of the whole list exist. track=True adds track_scores, one fp32
    value per 20 ms frame of the scored signal, and under trimming track_frames, the source frame number of each.
    segments=thr adds segments, a list of {start, end, frames, mean, min, argmin_start} with positions in samples
    of the untrimmed 16 kHz signal, for the runs of frames whose track lies below thr after gaps of at most
    seg_merge frames are bridged and runs shorter than seg_min frames are dropped (defaults: 0.2 s and 0.5 s), and
    flagged_samples, the samples of the scored signal inside segments (flagged_samples / n_samples is the flagged
    share). The track is the window scores spread over the frames they cover: its resolution is that of hop and
    win, so localising wants a small hop (3 200, say, where about 20 windows cover an instant against 2 at the
    default 32 300, and the forward runs about 10 times as many windows). The track costs 4 bytes per 20 ms on the
    device for the whole list; with either option on, trimming keeps every recording's kept_ids on the host past its
    chunk, 8 bytes per kept frame. The segment slots (counts, bounds and statistics) come back in one copy.
    """

    def __init__(self, model, device, criterion=None, amp="x3", batch_size=32, hop=32300, reduce="mean", win=CUT,
                 threads=8, convert=False, trim=None, trim_db=40.0, trim_pad=10, track=False, segments=None,
                 seg_merge=10, seg_min=25):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RecordingScorer runs the HIP path and needs a ROCm GPU (there is no CPU path)")
        if amp not in AMP:
            raise ValueError(f"amp {amp!r} is not one of {[a for a in AMP if a]}")
        if reduce not in REDUCE:
            raise ValueError(f"reduce {reduce!r} is not one of {list(REDUCE)}")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        window_table([1], hop, win)     # the rule's own check of hop and win
        if trim is not None and trim not in TRIM_MODES:
            raise ValueError(f"trim {trim!r} is not one of {sorted(TRIM_MODES)} (or None)")
        if not float(trim_db) > 0:
            raise ValueError(f"trim_db must be positive, got {trim_db}")
        if int(trim_pad) != trim_pad or trim_pad < 0:
            raise ValueError(f"trim_pad must be a whole number of frames >= 0, got {trim_pad}")
        self.trim, self.trim_db, self.trim_pad = trim, float(trim_db), int(trim_pad)
        if segments is not None:
            with np.errstate(over="ignore"):
                if not np.isfinite(np.float32(segments)):
                    raise ValueError(f"segments (the threshold) must be finite in float32, got {segments}")
        if int(seg_merge) != seg_merge or seg_merge < 0:
            raise ValueError(f"seg_merge must be a whole number of frames >= 0, got {seg_merge}")
        if int(seg_min) != seg_min or seg_min < 1:
            raise ValueError(f"seg_min must be a whole number of frames >= 1, got {seg_min}")
        self.track, self.segments = bool(track), None if segments is None else float(segments)
        self.seg_merge, self.seg_min = int(seg_merge), int(seg_min)
        self.model, self.criterion, self.amp = model, criterion, AMP[amp]
        self.B, self.hop, self.win, self.reduce, self.threads = int(batch_size), int(hop), int(win), reduce, threads
        self.pin = _PinnedBuf()
        self.convert = bool(convert)
        self.tables = IngestTables(self.device, SAMPLE_RATE) if self.convert else None

    # ------------------------------------------------------------------ inputs -----------------
    def score(self, paths, timeline=False):
        """paths: mono 16 kHz .flac files. A file that is not raises AudioReadError naming it before anything is
        scored (resampling and down-mixing are not done here). With convert=True: .flac or .wav files of any integer
        sample rate and channel count; only a file without samples or with a non-positive rate is refused."""
        paths = [str(p) for p in paths]
        if self.convert:
            return self._score_converted(paths, timeline)
        lens = np.empty(len(paths), dtype=np.int64)
        for i, p in enumerate(paths):
            frames, ch, sr, _ = audio.probe(p)
            if ch != 1:
                raise audio.AudioReadError(f"{p}: expected a mono recording, got {ch} channels")
            if sr != SAMPLE_RATE:
                raise audio.AudioReadError(f"{p}: expected {SAMPLE_RATE} Hz, got {sr} Hz (resampling is not done here)")
            if frames == 0:
                raise audio.AudioReadError(f"{p}: STREAMINFO has no sample count")
            lens[i] = frames

        def load(i0, i1, host):
            audio.read_batch(paths[i0:i1], out=host, threads=self.threads)
        return self._run(paths, lens, load, timeline)

    def _score_converted(self, paths, timeline):
        n = len(paths)
        frames, chans, rates = (np.empty(n, dtype=np.int64) for _ in range(3))
        for i, p in enumerate(paths):
            frames[i], chans[i], rates[i] = audio.probe_any(p)
            if frames[i] <= 0:
                raise audio.AudioReadError(f"{p}: no samples to score (the header gives {frames[i]} frames)")
            if rates[i] <= 0:
                raise audio.AudioReadError(f"{p}: sample rate {rates[i]} Hz")

        def load(i0, i1, host):
            audio.read_batch_interleaved(paths[i0:i1], out=host, threads=self.threads)
        return self._run(paths, converted_lengths(frames, rates), load, timeline, (frames, chans, rates))

    def score_arrays(self, arrays, names=None, timeline=False, rates=None):
        """arrays: float32 waveforms, 1-D at 16 kHz. With convert=True an array may also be [n, C] (interleaved
        channels) and `rates` gives its sample rate: one int for all arrays or one per array (None: 16 kHz); the
        arrays then take the device path of `score` on files."""
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        names = [f"array {i}" for i in range(len(arrays))] if names is None else [str(n) for n in names]
        if len(names) != len(arrays):
            raise ValueError(f"{len(names)} names for {len(arrays)} arrays")
        if not self.convert:
            if rates is not None:
                raise ValueError("score_arrays: rates needs a scorer built with convert=True")
            for n, a in zip(names, arrays):
                if a.ndim != 1:
                    raise ValueError(f"{n}: expected a 1-D waveform, got shape {a.shape}")
        else:
            for n, a in zip(names, arrays):
                if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] < 1):
                    raise ValueError(f"{n}: expected a [n] or [n, channels] waveform, got shape {a.shape}")
        lens = np.array([a.shape[0] for a in arrays], dtype=np.int64)

        def load(i0, i1, host):
            o = 0
            for a in arrays[i0:i1]:
                host[o:o + a.size] = torch.from_numpy(a.reshape(-1))
                o += a.size
        if not self.convert:
            return self._run(names, lens, load, timeline)
        rates = np.asarray(SAMPLE_RATE if rates is None else rates, dtype=np.int64)
        if rates.ndim == 0:
            rates = np.full(len(arrays), int(rates), dtype=np.int64)
        if rates.shape != (len(arrays),):
            raise ValueError(f"{rates.size} rates for {len(arrays)} arrays")
        for n, f, r in zip(names, lens, rates):
            if f <= 0:
                raise ValueError(f"{n}: no samples to score (length {int(f)})")
            if r <= 0:
                raise ValueError(f"{n}: sample rate {int(r)} Hz")
        chans = np.array([1 if a.ndim == 1 else a.shape[1] for a in arrays], dtype=np.int64)
        return self._run(names, converted_lengths(lens, rates), load, timeline, (lens, chans, rates))

    # ----------------------------------------------------------------- scoring -----------------
    def _batch_scores(self, xb):
        return _scores(self.model, xb, self.criterion, self.amp).float()

    def _converted(self, i0, i1, lens, load, source):
        """The packed 16 kHz signal of recordings i0 .. i1 - 1: the chunk is loaded and uploaded as decoded, then
        down-mixed and resampled on the device. A chunk of mono 16 kHz recordings is its own upload."""
        frames, chans, rates = (a[i0:i1] for a in source)
        raw = frames * chans
        rtotal = int(raw.sum())
        load(i0, i1, self.pin.get(rtotal))
        src = self.pin.upload(rtotal, self.device)
        same = (chans == 1) & (rates == SAMPLE_RATE)
        if same.all():
            return src
        roffs, offs = (np.zeros(i1 - i0, dtype=np.int64) for _ in range(2))
        np.cumsum(raw[:-1], out=roffs[1:])
        np.cumsum(lens[i0:i1][:-1], out=offs[1:])
        sig = torch.empty(int(lens[i0:i1].sum()), device=self.device, dtype=torch.float32)
        ingest_resample(src, sig, self.tables, [self.tables.job(rates[k], chans[k], frames[k], roffs[k], offs[k])
                                                for k in np.nonzero(~same)[0]])
        for k in np.nonzero(same)[0]:
            sig[offs[k]:offs[k] + frames[k]].copy_(src[roffs[k]:roffs[k] + frames[k]])
        return sig

    @torch.no_grad()
    def _run(self, names, lens, load, timeline, source=None):
        """source: None, or the (frames, channels, rates) arrays of recordings that `load` delivers interleaved at
        their own rate; lens are then their 16 kHz lengths."""
        if len(names) == 0:
            return []
        if self.trim is not None:
            return self._run_trimmed(names, lens, load, timeline, source)
        rec, start, seg = window_table(lens, self.hop, self.win, names)
        self.model.eval()
        xb = torch.empty(self.B, self.win, device=self.device, dtype=torch.float32)
        fill, parts = 0, []
        if self.amp == "x3":
            # as produce_evaluation_file_sharded: a pass neither starts from cached weight planes nor keeps them
            from . import wavlm_x3
            wavlm_x3.drop(self.model)
        try:
            with torch.cuda.device(self.device):
                cuts = (_chunks(lens, CHUNK_SAMPLES) if source is None
                        else _chunks_convert(source[0] * source[1], lens, CHUNK_SAMPLES))
                for i0, i1 in cuts:
                    if source is None:
                        total = int(lens[i0:i1].sum())
                        load(i0, i1, self.pin.get(total))
                        sig = self.pin.upload(total, self.device)
                    else:
                        sig = self._converted(i0, i1, lens, load, source)
                    clens = lens[i0:i1]
                    offs = np.zeros(i1 - i0, dtype=np.int64)
                    np.cumsum(clens[:-1], out=offs[1:])
                    w, w1 = int(seg[i0]), int(seg[i1])
                    while w < w1:
                        m = min(self.B - fill, w1 - w)
                        window_gather(sig, offs, clens, rec[w:w + m] - i0, start[w:w + m], self.win,
                                      out=xb[fill:fill + m])
                        w, fill = w + m, fill + m
                        if fill == self.B:
                            parts.append(self._batch_scores(xb))
                            fill = 0
                if fill:
                    parts.append(self._batch_scores(xb[:fill]))
        finally:
            if self.amp == "x3":
                wavlm_x3.drop(self.model)
        scores = torch.cat(parts)
        mean, lo, hi, arg = segment_reduce(scores, seg)
        mean, lo, hi = (t.cpu().numpy().astype(np.float32).tolist() for t in (mean, lo, hi))
        first = start[seg[:-1] + arg.cpu().numpy()].tolist()
        pick = {"mean": mean, "min": lo, "max": hi}[self.reduce]
        out = [{"name": names[r], "n_samples": int(lens[r]), "n_windows": int(seg[r + 1] - seg[r]), "score": pick[r],
                "min": lo[r], "max": hi[r], "argmin_start": int(first[r])} for r in range(len(names))]
        if source is not None:
            for r, d in enumerate(out):
                d["source_frames"], d["source_channels"], d["source_rate"] = (int(a[r]) for a in source)
        if timeline:
            flat = scores.cpu().numpy().astype(np.float32).tolist()
            for r, d in enumerate(out):
                d["window_starts"] = start[seg[r]:seg[r + 1]].tolist()
                d["window_scores"] = flat[int(seg[r]):int(seg[r + 1])]
        if self.track or self.segments is not None:
            self._locate(out, scores, seg, lens, lens, None)
        return out

    def _locate(self, out, scores, seg, mlens, nsrc, ids):
        """Adds the track and segment keys to the records `out` of the whole list (the locating rule): scores and seg
        are the window scores on the device and their per-recording prefix, mlens the lengths of the scored signals,
        nsrc those of the untrimmed ones, ids the kept_ids of every recording under trimming (else None)."""
        mlens = np.asarray(mlens, dtype=np.int64)
        nfr = -(-mlens // TRIM_FRAME)
        fo = np.zeros(nfr.size + 1, dtype=np.int64)
        np.cumsum(nfr, out=fo[1:])
        t = score_track(scores, seg, mlens, self.hop, self.win)
        if ids is not None:
            ids = [track_src_frames(k, nsrc[r], mlens[r]) for r, k in enumerate(ids)]
        if self.track:
            flat = t.cpu().numpy().tolist()
            for r, d in enumerate(out):
                d["track_scores"] = flat[int(fo[r]):int(fo[r + 1])]
                if ids is not None:
                    d["track_frames"] = ids[r].tolist()
        if self.segments is not None:
            found = track_segments(t, nfr, self.segments, self.seg_merge, self.seg_min)
            for r, (d, (a, b, mean, lo, arg)) in enumerate(zip(out, found)):
                kept = None if ids is None else ids[r]
                first, last = segment_span(a, b, nsrc[r], kept)
                worst, _ = segment_span(arg, arg, nsrc[r], kept)
                d["segments"] = [{"start": s, "end": e, "frames": n, "mean": mu, "min": v, "argmin_start": w}
                                 for s, e, n, mu, v, w in zip(first.tolist(), last.tolist(), (b - a + 1).tolist(),
                                                              mean.tolist(), lo.tolist(), worst.tolist())]
                d["flagged_samples"] = int((np.minimum((b + 1) * TRIM_FRAME, mlens[r]) - a * TRIM_FRAME).sum())

    def _run_trimmed(self, names, lens, load, timeline, source):
        """_run with trimming: a chunk's window table exists only once its trimmed lengths are back from the device,
        so the table is built chunk by chunk and appended; batches still straddle chunks and only the last is
        partial. Window positions are turned into source positions while the chunk's kept_ids are at hand."""
        window_table(lens, self.hop, self.win, names)       # names a recording without samples before any work
        self.model.eval()
        xb = torch.empty(self.B, self.win, device=self.device, dtype=torch.float32)
        fill, parts = 0, []
        tlens, kept, counts, first, last = [], [], [], [], []   # per recording (2) and per window (3), by chunk
        locate = self.track or self.segments is not None
        all_ids = []            # with locate: every recording's kept_ids, kept past its chunk
        if self.amp == "x3":
            from . import wavlm_x3
            wavlm_x3.drop(self.model)
        try:
            with torch.cuda.device(self.device):
                cuts = (_chunks(lens, CHUNK_SAMPLES) if source is None
                        else _chunks_convert(source[0] * source[1], lens, CHUNK_SAMPLES))
                for i0, i1 in cuts:
                    if source is None:
                        total = int(lens[i0:i1].sum())
                        load(i0, i1, self.pin.get(total))
                        sig = self.pin.upload(total, self.device)
                    else:
                        sig = self._converted(i0, i1, lens, load, source)
                    offs = np.zeros(i1 - i0, dtype=np.int64)
                    np.cumsum(lens[i0:i1][:-1], out=offs[1:])
                    sig, clens, ids = trim_silence(sig, offs, lens[i0:i1], self.trim, self.trim_db, self.trim_pad)
                    offs = np.zeros(i1 - i0, dtype=np.int64)
                    np.cumsum(clens[:-1], out=offs[1:])
                    rec, start, seg = window_table(clens, self.hop, self.win, names[i0:i1])
                    stop = np.minimum(start + self.win, clens[rec]) - 1     # the last sample of the window's span
                    tlens.append(clens)
                    kept.append(np.array([k.size for k in ids], dtype=np.int64))
                    counts.append(np.diff(seg))
                    if locate:
                        all_ids.extend(ids)
                    first.append(np.concatenate([trim_src(ids[r], start[seg[r]:seg[r + 1]])
                                                 for r in range(i1 - i0)]))
                    last.append(np.concatenate([trim_src(ids[r], stop[seg[r]:seg[r + 1]]) + 1
                                                for r in range(i1 - i0)]))
                    w, w1 = 0, int(seg[-1])
                    while w < w1:
                        m = min(self.B - fill, w1 - w)
                        window_gather(sig, offs, clens, rec[w:w + m], start[w:w + m], self.win,
                                      out=xb[fill:fill + m])
                        w, fill = w + m, fill + m
                        if fill == self.B:
                            parts.append(self._batch_scores(xb))
                            fill = 0
                if fill:
                    parts.append(self._batch_scores(xb[:fill]))
        finally:
            if self.amp == "x3":
                wavlm_x3.drop(self.model)
        tlens, kept, first, last = (np.concatenate(a) for a in (tlens, kept, first, last))
        seg = np.zeros(len(names) + 1, dtype=np.int64)
        np.cumsum(np.concatenate(counts), out=seg[1:])
        scores = torch.cat(parts)
        mean, lo, hi, arg = segment_reduce(scores, seg)
        mean, lo, hi = (t.cpu().numpy().astype(np.float32).tolist() for t in (mean, lo, hi))
        worst = first[seg[:-1] + arg.cpu().numpy()].tolist()
        pick = {"mean": mean, "min": lo, "max": hi}[self.reduce]
        out = [{"name": names[r], "n_samples": int(tlens[r]), "n_windows": int(seg[r + 1] - seg[r]), "score": pick[r],
                "min": lo[r], "max": hi[r], "argmin_start": int(worst[r]), "untrimmed_samples": int(lens[r]),
                "kept_frames": int(kept[r])} for r in range(len(names))]
        if source is not None:
            for r, d in enumerate(out):
                d["source_frames"], d["source_channels"], d["source_rate"] = (int(a[r]) for a in source)
        if timeline:
            flat = scores.cpu().numpy().astype(np.float32).tolist()
            for r, d in enumerate(out):
                d["window_starts"] = first[seg[r]:seg[r + 1]].tolist()
                d["window_ends"] = last[seg[r]:seg[r + 1]].tolist()
                d["window_scores"] = flat[int(seg[r]):int(seg[r + 1])]
        if locate:
            self._locate(out, scores, seg, tlens, lens, all_ids)
        return out


def write_scores(path, records):
    """One line per recording, in input order: "name n_samples n_windows score min max argmin_start". The floats are
    written as radhip.infer._write writes a score: str() of the float32 value widened to a double."""
    with open(path, "w") as fh:
        for d in records:
            fh.write("{} {} {} {} {} {} {}\n".format(d["name"], d["n_samples"], d["n_windows"], d["score"], d["min"],
                                                     d["max"], d["argmin_start"]))


def write_timeline(path, records):
    """One line per window: "name start score"."""
    with open(path, "w") as fh:
        for d in records:
            for st, sco in zip(d["window_starts"], d["window_scores"]):
                fh.write("{} {} {}\n".format(d["name"], st, sco))


def write_segments(path, records):
    """One line per flagged segment (segments=thr): "name start end frames mean min", positions in samples of the
    untrimmed 16 kHz signal, floats as write_scores writes them."""
    with open(path, "w") as fh:
        for d in records:
            for s in d["segments"]:
                fh.write("{} {} {} {} {} {}\n".format(d["name"], s["start"], s["end"], s["frames"], s["mean"],
                                                      s["min"]))


def write_track(path, records):
    """One line per scored frame (track=True): "name frame_start score", frame_start the frame's first sample in the
    untrimmed 16 kHz signal."""
    with open(path, "w") as fh:
        for d in records:
            frames = d.get("track_frames", range(len(d["track_scores"])))
            for f, sco in zip(frames, d["track_scores"]):
                fh.write("{} {} {}\n".format(d["name"], f * TRIM_FRAME, sco))

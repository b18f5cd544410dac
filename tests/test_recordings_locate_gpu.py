"""Locating the spoofed parts through the scorer (RecordingScorer(track=..., segments=...), main.py --score_track /
--score_segments) on the GPU, on the tiny Dual-Stream model of tests/test_recordings_trim_gpu.py (its recipe restated
here), x3, batches of 4, hop 3 200.

Files, mono 16 kHz .flac of seeded noise: 30 000 samples (one tiled window), 64 601 (two windows one sample apart),
100 000, and 200 000 with 2 s of inner zeros. And, for convert=True, a 48 kHz stereo .flac.

The kernels are pinned by tests/test_locate_gpu.py. Here the plumbing is pinned, each run against ITSELF so that the
scorer's run-to-run spread plays no part: track_scores lie within (c_j + 3) 2^-24 max|s| of track_np of the same
run's window_scores; segments equal segments_np of the same run's track_scores (positions, frames, min exactly; mean
within (frames - 1) 2^-24 max|t|); positions under trimming equal the source mapping of the numpy trimming rule.
Where two runs are compared (options off against a scorer built without them, small chunks, the CLI), numbers are
equal bitwise when the scorer's own spread on one batch is zero, else within 4 x that spread, the rule of
tests/test_recordings_trim_gpu.py, and the segment structure is compared at a threshold above every score, where no
spread can move a flag.
"""
import json
import os

import numpy as np
import pytest
import torch

from flac_writer import encode
from seeded import seeded_fill_

pytestmark = pytest.mark.gpu
HOP, BATCH, WIN, F, U = 3200, 4, 64600, 320, 2.0 ** -24
DB, PAD = 40.0, 10
FILES = [("short.flac", [(30000, 3000)]),
         ("two.flac", [(64601, 3000)]),
         ("mid.flac", [(100000, 3000)]),
         ("pause.flac", [(90000, 3000), (32000, 0), (78000, 3000)])]
WIDE = ("wide_48k_st.flac", 48000, 2, [(300000, 3000)], 100000)
HIGH = 1.0e30           # a threshold above every score


def _pcm(runs, ch, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.clip(np.round(a * rng.standard_normal((n, ch))), -32768, 32767) for n, a in runs])
    x = x.astype(np.int64)
    return x[:, 0] if ch == 1 else x


@pytest.fixture(scope="module")
def setup(tmp_path_factory, golden):
    import main as cli  # noqa: F401  (puts the package on sys.path)
    from radhip import audio
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    root = tmp_path_factory.mktemp("recordings_locate")
    cfg = load_config("Phase6_Proposed.conf")
    cfg["database_path"] = str(root / "unused")
    cfg["num_epochs"], cfg["batch_size"] = 1, 2
    cfg["test_config"] = {"batch_size": BATCH, "num_workers": 0}
    cfg["model_config"]["num_encoders"] = 2
    cfg["model_config"]["wavlm_config"] = json.loads(str(golden("model_tiny.npz")["wavlm_config"]))
    conf = root / "Tiny.conf"
    conf.write_text(json.dumps(cfg, indent=2))
    torch.manual_seed(0)
    model = apply_lora_to_wavlm(get_model(cfg["model_config"], "cuda"), cfg["training_config"])
    seeded_fill_(model, seed=41)
    model = model.cuda().eval()
    weights = root / "tiny.pth"
    torch.save(model.state_dict(), weights)
    plain = lambda f, c, b: {"kind": "verbatim"}    # noqa: E731
    paths = []
    for k, (name, runs) in enumerate(FILES):
        (root / name).write_bytes(encode(_pcm(runs, 1, seed=60 + k), sample_rate=16000, plan=plain))
        paths.append(root / name)
    signals = [audio.read(p)[0].astype(np.float32) for p in paths]
    name, rate, ch, runs, _ = WIDE
    wide = root / name
    wide.write_bytes(encode(_pcm(runs, ch, seed=70), sample_rate=rate, plan=plain))
    from radhip.infer import _scores
    from radhip.recordings import AMP
    first = torch.from_numpy(np.stack([signals[2][:WIN]] * BATCH)).cuda()
    with torch.no_grad():
        a, b = (_scores(model, first, None, AMP["x3"]).float().cpu().numpy() for _ in range(2))
    return {"root": root, "conf": conf, "model": model, "weights": weights, "paths": paths, "signals": signals,
            "wide": wide, "spread": float(np.abs(a - b).max()), "cache": {}}


def _scorer(setup, **kw):
    from radhip.recordings import RecordingScorer
    return RecordingScorer(setup["model"], "cuda", amp="x3", batch_size=BATCH, hop=HOP, **kw)


def _same(a, b, spread, what):
    if spread == 0.0:
        assert a == b, (what, a, b)
    else:
        assert abs(a - b) <= 4 * spread, (what, a, b, spread)


def _same_records(got, want, spread):
    """Two runs of the same list: the same keys, the same integers, floats by the spread rule."""
    def same(x, y, what):
        assert type(x) is type(y), (what, x, y)
        if isinstance(x, dict):
            assert list(x) == list(y), what
            for k in x:
                same(x[k], y[k], (what, k))
        elif isinstance(x, list):
            assert len(x) == len(y), what
            for a, b in zip(x, y):
                same(a, b, what)
        else:
            _same(x, y, spread if isinstance(x, float) else 0.0, what)
    same(got, want, "records")


def _covering(m):
    from radhip.recordings import window_table
    _, start, _ = window_table([m], HOP)
    if m <= WIN:
        return np.ones(-(-m // F), dtype=np.int64)
    c = np.zeros(-(-m // F) + 1, dtype=np.int64)
    np.add.at(c, start // F, 1)
    np.add.at(c, (start + WIN - 1) // F + 1, -1)
    return np.cumsum(c)[:-1]


def _check_track(d):
    """track_scores of one record against track_np of the same record's window_scores."""
    from radhip.recordings import track_np
    m, s = d["n_samples"], np.array(d["window_scores"], dtype=np.float32)
    t = np.array(d["track_scores"], dtype=np.float64)
    assert all(isinstance(v, float) for v in d["track_scores"]) and t.size == -(-m // F)
    assert np.array_equal(t.astype(np.float32).astype(np.float64), t)      # fp32 values
    ref = track_np(m, s, HOP)
    bound = (_covering(m) + 3) * U * float(np.abs(s).max())
    err = np.abs(t - ref)
    assert (err <= bound).all(), (d["name"], int(np.argmax(err / bound)), float((err / bound).max()))


def _check_segments(d, thr, merge, min_frames, n_source, ids=None):
    """segments / flagged_samples of one record against segments_np of the same record's track_scores."""
    from radhip.recordings import segment_span, segments_np
    t = np.array(d["track_scores"], dtype=np.float32)
    a, b, mean, lo, arg = segments_np(t, thr, merge, min_frames)
    start, end = segment_span(a, b, n_source, ids)
    worst, _ = segment_span(arg, arg, n_source, ids)
    assert len(d["segments"]) == a.size, (d["name"], len(d["segments"]), a.size)
    for s, *want in zip(d["segments"], start, end, b - a + 1, lo, worst, mean, a, b):
        assert list(s) == ["start", "end", "frames", "mean", "min", "argmin_start"]
        assert [s["start"], s["end"], s["frames"], s["min"], s["argmin_start"]] == [int(want[0]), int(want[1]),
                                                                                   int(want[2]), float(want[3]),
                                                                                   int(want[4])], (d["name"], s)
        x, y = int(want[6]), int(want[7])
        assert abs(s["mean"] - want[5]) <= (y - x) * U * float(np.abs(t[x:y + 1]).max()), (d["name"], s)
    assert d["flagged_samples"] == int((np.minimum((b + 1) * F, d["n_samples"]) - a * F).sum())
    return t < np.float32(thr)


def _median_threshold(records):
    """The midpoint of two adjacent distinct sorted track values near the median of the whole list's track."""
    v = np.unique(np.concatenate([np.array(d["track_scores"], dtype=np.float32) for d in records]))
    assert v.size >= 2
    k = min(max(v.size // 2, 1), v.size - 1)
    return (float(v[k - 1]) + float(v[k])) / 2


def _first_pass(setup):
    if "first" not in setup["cache"]:
        setup["cache"]["first"] = _scorer(setup, track=True).score(setup["paths"], timeline=True)
    return setup["cache"]["first"]


def test_options_off_change_nothing(setup):
    base = _scorer(setup).score(setup["paths"], timeline=True)
    off = _scorer(setup, track=False, segments=None, seg_merge=3, seg_min=7).score(setup["paths"], timeline=True)
    assert list(base[0]) == ["name", "n_samples", "n_windows", "score", "min", "max", "argmin_start", "window_starts",
                             "window_scores"]
    _same_records(off, base, setup["spread"])
    assert [d["n_windows"] for d in base] == [1, 2, 13, 44]


def test_track_scores_follow_the_rule_on_the_runs_own_window_scores(setup):
    recs = _first_pass(setup)
    for d, x in zip(recs, setup["signals"]):
        assert d["n_samples"] == x.size and "track_frames" not in d and "segments" not in d
        _check_track(d)
    assert [len(d["track_scores"]) for d in recs] == [94, 202, 313, 625]
    assert len(set(recs[0]["track_scores"])) == 1 and recs[0]["track_scores"][0] == recs[0]["window_scores"][0]


def test_segments_equal_the_rule_on_the_returned_track(setup):
    thr = _median_threshold(_first_pass(setup))
    recs = _scorer(setup, track=True, segments=thr, seg_merge=2, seg_min=3).score(setup["paths"], timeline=True)
    flags = np.concatenate([_check_segments(d, thr, 2, 3, d["n_samples"]) for d in recs])
    assert flags.any() and not flags.all(), (thr, int(flags.sum()), flags.size)
    for d in recs:
        _check_track(d)
    # segments alone: no track keys; the defaults bridge 10 frames and want 25
    only = _scorer(setup, segments=HIGH).score(setup["paths"])
    for d, x in zip(only, setup["signals"]):
        assert "track_scores" not in d and "window_scores" not in d
        assert [(s["start"], s["end"], s["frames"]) for s in d["segments"]] == [(0, x.size, -(-x.size // F))]
        assert d["flagged_samples"] == d["n_samples"] == x.size
        assert d["segments"][0]["min"] <= d["segments"][0]["mean"] and d["segments"][0]["argmin_start"] % F == 0
    none = _scorer(setup, segments=-HIGH).score(setup["paths"])
    assert all(d["segments"] == [] and d["flagged_samples"] == 0 for d in none)


def _trim_clear(x):
    from radhip.recordings import frame_energy_np
    e = frame_energy_np(x)
    q = e / (e.max() * 10.0 ** (-DB / 10.0))
    assert not ((q >= 1 - 1e-3) & (q <= 1 + 1e-3)).any()


def _trimmed(setup):
    """(records at the median threshold, records at HIGH, thr, kept_ids) under trim="gaps", track and segments on."""
    from radhip.recordings import trim_plan_np
    if "trimmed" not in setup["cache"]:
        for x in setup["signals"]:
            _trim_clear(x)
        kw = dict(trim="gaps", trim_db=DB, trim_pad=PAD, track=True, seg_merge=2, seg_min=3)
        thr = _median_threshold(_scorer(setup, **kw).score(setup["paths"]))
        mid = _scorer(setup, segments=thr, **kw).score(setup["paths"], timeline=True)
        high = _scorer(setup, segments=HIGH, **kw).score(setup["paths"], timeline=True)
        ids = [trim_plan_np(x, "gaps", DB, PAD)[1] for x in setup["signals"]]
        setup["cache"]["trimmed"] = (mid, high, thr, ids)
    return setup["cache"]["trimmed"]


def test_positions_under_trimming_are_source_positions(setup):
    mid, high, thr, ids = _trimmed(setup)
    assert ids[3].size == 625 - 99 + 2 * PAD        # the pause lost its middle
    for recs, t in ((mid, thr), (high, HIGH)):
        for d, x, k in zip(recs, setup["signals"], ids):
            assert d["track_frames"] == k.tolist() and d["kept_frames"] == k.size and d["untrimmed_samples"] == x.size
            _check_track(d)
            _check_segments(d, t, 2, 3, x.size, k)
    # every frame flagged: one segment per recording, from the first kept frame to the end of the last, and the one
    # of the file with the pause spans more source samples than it scored
    for d, x, k in zip(high, setup["signals"], ids):
        (s,) = d["segments"]
        assert (s["start"], s["end"], s["frames"]) == (int(k[0]) * F, min((int(k[-1]) + 1) * F, x.size), k.size)
        assert d["flagged_samples"] == d["n_samples"]
    s = high[3]["segments"][0]
    assert s["end"] - s["start"] == 200000 > s["frames"] * F
    spans = [s for s in mid[3]["segments"] if s["end"] - s["start"] > s["frames"] * F]
    print(f"median threshold {thr}: {len(mid[3]['segments'])} segments in the file with the pause, {len(spans)} "
          f"across it")


def test_small_chunks_give_the_same_records(setup, monkeypatch):
    from radhip import recordings
    kw = dict(track=True, segments=HIGH, seg_merge=2, seg_min=3)
    trimming, plain = _scorer(setup, trim="gaps", trim_db=DB, trim_pad=PAD, **kw), _scorer(setup, **kw)
    one = [s.score(setup["paths"], timeline=True) for s in (trimming, plain)]
    monkeypatch.setattr(recordings, "CHUNK_SAMPLES", 100000)
    many = [s.score(setup["paths"], timeline=True) for s in (trimming, plain)]
    for a, b in zip(many, one):
        _same_records(a, b, setup["spread"])
    assert "track_frames" in many[0][0] and "track_frames" not in many[1][0]


def test_locating_follows_the_conversion(setup):
    name, rate, ch, runs, n16 = WIDE
    first = _scorer(setup, convert=True, track=True).score([setup["wide"], setup["paths"][1]], timeline=True)
    thr = _median_threshold(first)
    recs = _scorer(setup, convert=True, track=True, segments=thr, seg_merge=2, seg_min=3).score(
        [setup["wide"], setup["paths"][1]], timeline=True)
    assert (recs[0]["source_rate"], recs[0]["source_channels"], recs[0]["n_samples"]) == (rate, ch, n16)
    flags = []
    for d in recs:
        _check_track(d)
        flags.append(_check_segments(d, thr, 2, 3, d["n_samples"]))
    flags = np.concatenate(flags)
    assert flags.any() and not flags.all()


def test_cli_writes_the_same_numbers(setup):
    import main as cli
    root, paths, spread = setup["root"], setup["paths"], setup["spread"]
    lst = root / "files.txt"
    lst.write_text("\n".join(str(p) for p in paths) + "\n")
    base = ["--config", str(setup["conf"]), "--output_dir", str(root / "exp"), "--eval_model_weights",
            str(setup["weights"]), "--score_files", str(lst), "--score_hop", str(HOP), "--score_trim", "gaps"]
    cli.main(cli.parse_args(base + ["--comment", "plain"]))
    os.environ.pop("WORLD_SIZE", None)
    cli.main(cli.parse_args(base + ["--comment", "loc", "--score_track", "--score_segments", str(HIGH),
                                    "--score_seg_merge", "2", "--score_seg_min", "3"]))
    os.environ.pop("WORLD_SIZE", None)
    plain, loc = root / "exp" / "LA_Tiny_ep1_bs2_plain", root / "exp" / "LA_Tiny_ep1_bs2_loc"
    assert not (plain / "recording_segments.txt").exists() and not (plain / "recording_track.txt").exists()
    # recording_scores.txt is what a run without the flags writes
    a, b = ((d / "recording_scores.txt").read_text() for d in (plain, loc))
    if spread == 0.0:
        assert a == b
    rows_a, rows_b = ([ln.split(" ") for ln in t.splitlines()] for t in (a, b))
    assert len(rows_a) == len(rows_b) == len(paths) and all(len(r) == 7 for r in rows_b)
    for ra, rb in zip(rows_a, rows_b):
        assert ra[:3] == rb[:3]
        for x, y in zip(ra[3:6], rb[3:6]):
            _same(float(x), float(y), spread, "score")
    # the records to compare with come from a scorer that runs after the CLI, as in tests/test_recordings_trim_gpu.py
    high = _scorer(setup, trim="gaps", track=True, segments=HIGH, seg_merge=2, seg_min=3).score(paths)
    seg = [ln.split(" ") for ln in (loc / "recording_segments.txt").read_text().splitlines()]
    want = [(d["name"], s) for d in high for s in d["segments"]]
    assert len(seg) == len(want) == len(paths) and all(len(r) == 6 for r in seg)
    for r, (name, s) in zip(seg, want):
        assert (r[0], int(r[1]), int(r[2]), int(r[3])) == (name, s["start"], s["end"], s["frames"])
        _same(float(r[4]), s["mean"], spread, "mean")
        _same(float(r[5]), s["min"], spread, "min")
    tr = [ln.split(" ") for ln in (loc / "recording_track.txt").read_text().splitlines()]
    want = [(d["name"], f * F, v) for d in high for f, v in zip(d["track_frames"], d["track_scores"])]
    assert len(tr) == len(want) and all(len(r) == 3 for r in tr)
    for r, (name, pos, v) in zip(tr, want):
        assert (r[0], int(r[1])) == (name, pos)
        _same(float(r[2]), v, spread, "track score")

"""Whole-recording scoring with silence trimming (RecordingScorer(trim=...), main.py --score_trim) on the GPU, on the
tiny Dual-Stream model of tests/test_recordings_gpu.py (its recipe restated here), hop 32300, batches of 4.

Files, mono 16 kHz .flac: 8 000 zeros + 70 000 samples of noise + 16 000 zeros; 200 000 samples with a 3 s inner gap;
70 000 samples of constant-level noise (nothing to trim); 20 000 samples with leading zeros (a tiled window). And,
for convert=True, a 48 kHz stereo .flac with silent ends whose noise starts and stops inside a 16 kHz frame, so
that the resampler's ringing into the zeros stays in frames that are loud anyway.

The kernels are pinned by tests/test_trim_gpu.py. Here the plumbing is pinned: the records of the trimming scorer
equal those of a plain scorer's score_arrays fed the numpy-trimmed signals (radhip.recordings.trim_plan_np /
trim_apply_np): n_samples and n_windows exactly, scores by the rule of tests/test_recordings_gpu.py (bitwise when the
scorer's own run-to-run spread on one batch is zero, else within 4 x that spread); and every position equals
src(...) of the numpy rule. Exact comparison is fair because no frame of the float64 energies lies within 1e-3 of
the threshold, relatively, which is asserted first (for the converted file on the signal the device wrote).
"""
import json
import os

import numpy as np
import pytest
import torch

from flac_writer import encode
from seeded import seeded_fill_

pytestmark = pytest.mark.gpu
HOP, BATCH, WIN, F = 32300, 4, 64600, 320
DB, PAD = 40.0, 10
#        name          runs of (samples, amplitude in PCM units)
FILES = [("ends.flac", [(8000, 0), (70000, 3000), (16000, 0)]),
         ("gap.flac", [(80000, 3000), (48000, 0), (72000, 3000)]),
         ("level.flac", [(70000, 3000)]),
         ("short.flac", [(6000, 0), (14000, 3000)])]
WIDE = ("wide_48k_st.flac", 48000, 2, [(24480, 0), (210000, 3000), (30000, 0)], 88160)


def _pcm(runs, ch, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.clip(np.round(a * rng.standard_normal((n, ch))), -32768, 32767) for n, a in runs])
    x = x.astype(np.int64)
    return x[:, 0] if ch == 1 else x


@pytest.fixture(scope="module")
def setup(tmp_path_factory, golden):
    import main as cli  # noqa: F401  (puts the package on sys.path)
    from radhip import audio, ops
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    root = tmp_path_factory.mktemp("recordings_trim")
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
        (root / name).write_bytes(encode(_pcm(runs, 1, seed=30 + k), sample_rate=16000, plan=plain))
        paths.append(root / name)
    signals = [audio.read(p)[0].astype(np.float32) for p in paths]
    name, rate, ch, runs, n16 = WIDE
    wide = root / name
    wide.write_bytes(encode(_pcm(runs, ch, seed=40), sample_rate=rate, plan=plain))
    raw = audio.read(wide)[0].astype(np.float32).reshape(-1, ch)
    tables = ops.IngestTables("cuda")
    dst = torch.empty(n16, device="cuda")
    ops.ingest_resample(torch.from_numpy(raw.reshape(-1)).cuda(), dst, tables, [tables.job(rate, ch, raw.shape[0], 0, 0)])
    from radhip.infer import _scores
    from radhip.recordings import AMP
    first = torch.from_numpy(np.stack([signals[1][:WIN]] * BATCH)).cuda()
    with torch.no_grad():
        a, b = (_scores(model, first, None, AMP["x3"]).float().cpu().numpy() for _ in range(2))
    return {"root": root, "conf": conf, "model": model, "weights": weights, "paths": paths, "signals": signals,
            "wide": wide, "wide_signal": dst.cpu().numpy(), "spread": float(np.abs(a - b).max())}


def _assert_clear(x, db=DB):
    from radhip.recordings import frame_energy_np
    e = frame_energy_np(x)
    q = e / (e.max() * 10.0 ** (-db / 10.0))
    near = np.nonzero((q >= 1 - 1e-3) & (q <= 1 + 1e-3))[0]
    assert near.size == 0, (near[:5], q[near[:5]])


def _same(a, b, spread, what):
    if spread == 0.0:
        assert a == b, (what, a, b)
    else:
        assert abs(a - b) <= 4 * spread, (what, a, b, spread)


def _scorer(setup, **kw):
    from radhip.recordings import RecordingScorer
    return RecordingScorer(setup["model"], "cuda", amp="x3", batch_size=BATCH, hop=HOP, **kw)


def _check(setup, got, signals, mode):
    """got: records of a trimming scorer (timeline=True) for `signals`; the reference: a plain scorer on the
    numpy-trimmed signals, and src(...) of the numpy rule for every position."""
    from radhip.recordings import trim_apply_np, trim_plan_np, trim_src, window_table
    plans = [trim_plan_np(x, mode, DB, PAD) for x in signals]
    want = _scorer(setup).score_arrays([trim_apply_np(x, ids) for x, (_, ids, _) in zip(signals, plans)],
                                       timeline=True)
    spread = setup["spread"]
    assert len(got) == len(want) == len(signals)
    for g, w, x, (_, ids, m) in zip(got, want, signals, plans):
        assert (g["n_samples"], g["n_windows"]) == (w["n_samples"], w["n_windows"]) and g["n_samples"] == m
        assert (g["untrimmed_samples"], g["kept_frames"]) == (x.size, ids.size)
        for k in ("score", "min", "max"):
            _same(g[k], w[k], spread, k)
        for a, b in zip(g["window_scores"], w["window_scores"]):
            _same(a, b, spread, "window score")
        _, start, _ = window_table([m], HOP)
        assert w["window_starts"] == start.tolist()
        assert g["window_starts"] == trim_src(ids, start).tolist()
        assert g["window_ends"] == (trim_src(ids, np.minimum(start + WIN, m) - 1) + 1).tolist()
        if spread == 0.0:
            assert g["argmin_start"] == int(trim_src(ids, w["argmin_start"]))
        assert g["argmin_start"] in g["window_starts"]
    return plans


@pytest.mark.parametrize("mode", ["ends", "gaps"])
def test_trimmed_records_equal_a_plain_scorer_on_numpy_trimmed_signals(setup, mode):
    for x in setup["signals"]:
        _assert_clear(x)
    got = _scorer(setup, trim=mode, trim_db=DB, trim_pad=PAD).score(setup["paths"], timeline=True)
    assert [d["name"] for d in got] == [str(p) for p in setup["paths"]]
    plans = _check(setup, got, setup["signals"], mode)
    # what the rule leaves of these files: the ends go in both modes, the 3 s gap only in "gaps"
    kept = [ids.size for _, ids, _ in plans]
    assert kept[0] == 219 + 2 * PAD and kept[2] == 219 and kept[3] == 45 + PAD and got[3]["n_windows"] == 1
    assert kept[1] == (625 if mode == "ends" else 625 - 150 + 2 * PAD)
    if mode == "gaps":       # a window across the cut covers more source samples than it has
        d = got[1]
        spans = [e - s for s, e in zip(d["window_starts"], d["window_ends"])]
        assert max(spans) == WIN + (150 - 2 * PAD) * F and min(spans) == WIN
    # arrays in place of files, without the timeline
    again = _scorer(setup, trim=mode, trim_db=DB, trim_pad=PAD).score_arrays(setup["signals"])
    for a, b in zip(again, got):
        assert "window_ends" not in a and (a["n_samples"], a["kept_frames"]) == (b["n_samples"], b["kept_frames"])
        _same(a["score"], b["score"], setup["spread"], "score")


def test_nothing_to_trim_equals_the_untrimmed_scorer(setup):
    p = [setup["paths"][2]]
    plain = _scorer(setup).score(p, timeline=True)
    for mode in ("ends", "gaps"):
        got = _scorer(setup, trim=mode).score(p, timeline=True)
        for k in ("name", "n_samples", "n_windows", "window_starts"):
            assert got[0][k] == plain[0][k], k
        assert got[0]["untrimmed_samples"] == 70000 and got[0]["kept_frames"] == 219
        assert got[0]["window_ends"] == [s + WIN for s in plain[0]["window_starts"]]
        for k in ("score", "min", "max"):
            _same(got[0][k], plain[0][k], setup["spread"], k)
        for a, b in zip(got[0]["window_scores"], plain[0]["window_scores"]):
            _same(a, b, setup["spread"], "window score")
        if setup["spread"] == 0.0:
            assert got[0]["argmin_start"] == plain[0]["argmin_start"]


def test_small_chunks_give_the_same_records(setup, monkeypatch):
    """The window table is appended chunk by chunk; batches straddle the chunks."""
    from radhip import recordings
    scorer = _scorer(setup, trim="gaps", trim_db=DB, trim_pad=PAD)
    one = scorer.score(setup["paths"], timeline=True)
    monkeypatch.setattr(recordings, "CHUNK_SAMPLES", 100000)
    many = scorer.score(setup["paths"], timeline=True)
    for a, b in zip(many, one):
        for k in ("n_samples", "n_windows", "kept_frames", "untrimmed_samples", "window_starts", "window_ends"):
            assert a[k] == b[k], k
        for x, y in zip(a["window_scores"], b["window_scores"]):
            _same(x, y, setup["spread"], "window score")


def test_trimming_follows_the_conversion(setup):
    name, rate, ch, runs, n16 = WIDE
    x16 = setup["wide_signal"]
    assert x16.size == n16
    _assert_clear(x16)
    got = _scorer(setup, convert=True, trim="ends", trim_db=DB, trim_pad=PAD).score(
        [setup["wide"], setup["paths"][0]], timeline=True)
    plans = _check(setup, got, [x16, setup["signals"][0]], "ends")
    assert (got[0]["source_rate"], got[0]["source_channels"], got[0]["source_frames"]) == (rate, ch, 264480)
    ids = plans[0][1]
    assert ids[0] == 25 - PAD and ids[-1] == 244 + PAD and got[0]["untrimmed_samples"] == n16


def test_cli_writes_the_same_numbers(setup):
    import main as cli
    root, paths = setup["root"], setup["paths"]
    lst = root / "files.txt"
    lst.write_text("\n".join(str(p) for p in paths) + "\n")
    out = root / "exp"
    cli.main(cli.parse_args(["--config", str(setup["conf"]), "--output_dir", str(out), "--eval_model_weights",
                             str(setup["weights"]), "--score_files", str(lst), "--score_trim", "gaps",
                             "--score_timeline", "--comment", "trim"]))
    os.environ.pop("WORLD_SIZE", None)
    recs = _scorer(setup, trim="gaps").score(paths, timeline=True)
    tag = out / "LA_Tiny_ep1_bs2_trim"
    rows = [ln.split(" ") for ln in (tag / "recording_scores.txt").read_text().splitlines()]
    assert [r[0] for r in rows] == [str(p) for p in paths] and all(len(r) == 7 for r in rows)
    for r, d in zip(rows, recs):
        assert [int(r[1]), int(r[2]), int(r[6])] == [d["n_samples"], d["n_windows"], d["argmin_start"]]
        for txt, key in zip(r[3:6], ("score", "min", "max")):
            _same(float(txt), d[key], setup["spread"], key)
    tl = [ln.split(" ") for ln in (tag / "recording_timeline.txt").read_text().splitlines()]
    want = [(d["name"], st, sc) for d in recs for st, sc in zip(d["window_starts"], d["window_scores"])]
    assert len(tl) == len(want) and all(len(r) == 3 for r in tl)
    for (name, st, sc), (n2, st2, sc2) in zip(tl, want):
        assert (name, int(st)) == (n2, st2)
        _same(float(sc), sc2, setup["spread"], "timeline score")

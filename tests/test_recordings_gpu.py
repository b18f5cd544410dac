"""Whole-recording scoring end to end on the GPU (radhip/recordings.py, main.py --score_files): five synthetic mono
16 kHz FLAC files of 30000, 64600, 64601, 100000 and 200000 samples, hop 32300, batches of 4, on the tiny Dual-Stream
model the CLI test builds. By the window rule these are 1 + 1 + 2 + 3 + 6 = 13 windows: three full batches and a last
batch of one, with the long recordings straddling batches.

Reference: the windows built in numpy (radhip.recordings.window_samples, pinned to the reference's `pad` in
tests/test_recordings_cpu.py), fed to radhip.infer._scores in the same batch partition, reduced in fp64.

Bound on a window score: the existing scorer scores one batch twice first. If the two runs agree bitwise, the new
path's window scores must equal the reference's exactly (the gather is a copy and the batches are the same); otherwise
4 x the measured spread is allowed. Both figures go to profiles/recordings_errors.json. A recording's mean lies
within (n - 1) 2^-24 max|s| of the fp64 mean of its own n window scores (the summation bound of rdx_segment_reduce).

Measured on one MI355X: x3 spread 0, deviation 0 (exact); fp32 (torch SDPA + hipBLASLt, itself not repeatable) spread
2.4e-7, deviation 6.0e-7 against the 9.5e-7 allowed; largest |mean - mean64| 0.15 of its bound.
"""
import json
import os

import numpy as np
import pytest
import torch

from flac_writer import encode
from seeded import seeded_fill_

pytestmark = pytest.mark.gpu
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
RECORD = os.path.join(PROFILES, "recordings_errors.json")
LENS = [30000, 64600, 64601, 100000, 200000]
HOP, BATCH, WIN = 32300, 4, 64600


def _record(key, obj):
    os.makedirs(PROFILES, exist_ok=True)
    cur = {}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            cur = json.load(f)
    cur[key] = obj
    cur["_format"] = ("per scoring precision: the existing scorer's run-to-run spread on one batch, the new path's "
                      "largest window-score deviation from the numpy-window reference, and the largest |mean - mean64| "
                      "over its summation bound")
    with open(RECORD, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(cur[k], sort_keys=True)}" for k in sorted(cur))
                + "\n}\n")


def _flac(path, n, seed, sample_rate=16000, channels=1):
    rng = np.random.default_rng(seed)
    shape = n if channels == 1 else (n, channels)
    x = np.clip(np.round(3000 * rng.standard_normal(shape)), -32768, 32767).astype(np.int64)
    path.write_bytes(encode(x, sample_rate=sample_rate, plan=lambda f, c, b: {"kind": "verbatim"}))
    return path


@pytest.fixture(scope="module")
def setup(tmp_path_factory, golden):
    import main as cli  # noqa: F401  (puts the package on sys.path)
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    root = tmp_path_factory.mktemp("recordings")
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
    paths = [_flac(root / f"rec_{n}.flac", n, seed=n) for n in LENS]
    return {"root": root, "conf": conf, "model": model, "weights": weights, "paths": paths}


def _reference(model, paths, amp):
    """(window scores fp32 [W], seg, start) of the numpy windows in batches of BATCH, and the scorer's own spread."""
    from radhip import audio
    from radhip.infer import _scores
    from radhip.recordings import AMP, window_samples, window_table
    xs = [audio.read(p)[0].astype(np.float32) for p in paths]
    rec, start, seg = window_table([x.size for x in xs], HOP)
    wins = np.stack([window_samples(xs[r], s) for r, s in zip(rec, start)]).astype(np.float32)
    with torch.no_grad():
        first = torch.from_numpy(wins[:BATCH]).cuda()
        a, b = (_scores(model, first, None, AMP[amp]).float().cpu().numpy() for _ in range(2))
        spread = float(np.abs(a - b).max())
        ref = np.concatenate([_scores(model, torch.from_numpy(wins[i:i + BATCH]).cuda(), None, AMP[amp]).float()
                              .cpu().numpy() for i in range(0, len(wins), BATCH)])
    return ref.astype(np.float32), seg, start, spread


@pytest.mark.parametrize("amp", ["fp32", "x3"])
def test_scorer_matches_numpy_windows(setup, amp):
    from radhip.recordings import RecordingScorer
    model, paths = setup["model"], setup["paths"]
    ref, seg, start, spread = _reference(model, paths, amp)
    assert ref.size == 13 and np.diff(seg).tolist() == [1, 1, 2, 3, 6]
    scorer = RecordingScorer(model, "cuda", amp=amp, batch_size=BATCH, hop=HOP)
    recs = scorer.score(paths, timeline=True)
    assert [d["name"] for d in recs] == [str(p) for p in paths]
    assert [d["n_samples"] for d in recs] == LENS and [d["n_windows"] for d in recs] == [1, 1, 2, 3, 6]
    got = np.array([s for d in recs for s in d["window_scores"]], dtype=np.float32)
    assert [s for d in recs for s in d["window_starts"]] == start.tolist()
    dev = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    worst = 0.0
    for r, d in enumerate(recs):
        s = got[seg[r]:seg[r + 1]]
        n = s.size
        mean64 = float(s.astype(np.float64).mean())
        err, bound = abs(d["score"] - mean64), (n - 1) * 2.0 ** -24 * float(np.abs(s).max())
        print(f"{amp} rec {r}: n={n} |mean - mean64| = {err:.3e}, bound {bound:.3e}")
        worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
        assert err <= bound, (r, err, bound)
        assert d["min"] == float(s.min()) and d["max"] == float(s.max())
        assert d["argmin_start"] == int(start[seg[r] + int(np.argmin(s))])
        if n == 1:
            assert d["min"] == d["max"] == d["score"] == float(s[0])
    print(f"{amp}: scorer spread {spread:.3e}, window-score deviation {dev:.3e}")
    _record(amp, {"scorer_spread": spread, "window_score_deviation": dev, "mean_error_over_bound": worst,
                  "windows": int(ref.size), "bound": "exact" if spread == 0.0 else 4 * spread})
    if spread == 0.0:
        np.testing.assert_array_equal(got, ref)
    else:
        assert dev <= 4 * spread, (dev, spread)
    # min / max as the recording's score, and arrays in place of files
    from radhip import audio
    xs = [audio.read(p)[0].astype(np.float32) for p in paths]
    lo = RecordingScorer(model, "cuda", amp=amp, batch_size=BATCH, hop=HOP, reduce="min").score_arrays(xs)
    assert [d["name"] for d in lo] == [f"array {i}" for i in range(len(xs))]
    assert all(d["score"] == d["min"] and "window_scores" not in d for d in lo)
    assert all(abs(a["min"] - b["min"]) <= 4 * spread for a, b in zip(lo, recs))


def test_cli_writes_scores_and_timeline(setup, monkeypatch):
    import main as cli
    from radhip import recordings
    root, paths = setup["root"], setup["paths"]
    lst = root / "files.txt"
    lst.write_text("\n".join(str(p) for p in paths) + "\n")
    seen = []
    real = recordings.RecordingScorer.score

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        seen.append((self, out))
        return out
    monkeypatch.setattr(recordings.RecordingScorer, "score", spy)
    out = root / "exp"
    cli.main(cli.parse_args(["--config", str(setup["conf"]), "--output_dir", str(out), "--eval_model_weights",
                             str(setup["weights"]), "--score_files", str(lst), "--score_timeline", "--comment", "rec"]))
    (scorer, recs), = seen
    assert (scorer.B, scorer.hop, scorer.reduce, scorer.amp) == (BATCH, HOP, "mean", "x3")
    tag = out / "LA_Tiny_ep1_bs2_rec"
    rows = [ln.split(" ") for ln in (tag / "recording_scores.txt").read_text().splitlines()]
    assert [r[0] for r in rows] == [str(p) for p in paths] and all(len(r) == 7 for r in rows)
    for r, d in zip(rows, recs):
        assert [int(r[1]), int(r[2]), int(r[6])] == [d["n_samples"], d["n_windows"], d["argmin_start"]]
        for txt, key in zip(r[3:6], ("score", "min", "max")):
            assert txt == str(float(np.float32(d[key]))) and float(txt) == d[key]
    tl = [ln.split(" ") for ln in (tag / "recording_timeline.txt").read_text().splitlines()]
    want = [(d["name"], st, sc) for d in recs for st, sc in zip(d["window_starts"], d["window_scores"])]
    assert len(tl) == 13 == len(want)
    for (name, st, sc), (n2, st2, sc2) in zip(tl, want):
        assert (name, int(st)) == (n2, st2) and sc == str(float(np.float32(sc2)))
    # the CLI's numbers are the API's on the same files (x3 on this model: bitwise unless the scorer itself is not)
    monkeypatch.undo()
    again = recordings.RecordingScorer(setup["model"], "cuda", amp="x3", batch_size=BATCH, hop=HOP).score(paths)
    spread = _reference(setup["model"], paths, "x3")[3]
    for a, b in zip(again, recs):
        assert abs(a["score"] - b["score"]) <= 4 * spread and a["n_windows"] == b["n_windows"]
    os.environ.pop("WORLD_SIZE", None)


@pytest.mark.parametrize("kind", ["8khz", "stereo"])
def test_cli_refuses_other_formats(setup, kind):
    import main as cli
    from radhip.audio import AudioReadError
    root, paths = setup["root"], setup["paths"]
    bad = (_flac(root / "bad_8khz.flac", 20000, 5, sample_rate=8000) if kind == "8khz"
           else _flac(root / "bad_stereo.flac", 20000, 6, channels=2))
    lst = root / f"files_{kind}.txt"
    lst.write_text("\n".join(str(p) for p in [paths[0], bad, paths[1]]) + "\n")
    out = root / "exp"
    with pytest.raises(AudioReadError, match=bad.name):
        cli.main(cli.parse_args(["--config", str(setup["conf"]), "--output_dir", str(out), "--eval_model_weights",
                                 str(setup["weights"]), "--score_files", str(lst), "--score_timeline",
                                 "--comment", kind]))
    tag = out / f"LA_Tiny_ep1_bs2_{kind}"
    assert not (tag / "recording_scores.txt").exists() and not (tag / "recording_timeline.txt").exists()
    os.environ.pop("WORLD_SIZE", None)

"""Whole-recording scoring with conversion (RecordingScorer(convert=True), main.py --score_convert) on the GPU: a
48 kHz stereo .flac whose 16 kHz length is 64 601, a 44.1 kHz mono .wav whose 16 kHz length is 30 000, an 8 kHz mono
.flac of 100 000 output samples and a plain mono 16 kHz .flac, hop 32300, batches of 4, on the tiny Dual-Stream model
of tests/test_recordings_gpu.py (its recipe restated here).

The conversion's numerics are pinned elementwise by tests/test_ingest_gpu.py. Here the plumbing is pinned: the window
scores must equal those of score_arrays fed with the converted signals that ops.ingest_resample itself wrote, under
the equality rule of tests/test_recordings_gpu.py: bitwise when the scorer's own run-to-run spread on one batch is
zero, else within 4 x that spread.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from flac_writer import encode
from seeded import seeded_fill_

pytestmark = pytest.mark.gpu
HOP, BATCH, WIN = 32300, 4, 64600
#        name             rate  channels frames   16 kHz length
FILES = [("a_48k_st.flac", 48000, 2, 193802, 64601),
         ("b_44k_mono.wav", 44100, 1, 82687, 30000),
         ("c_8k_mono.flac", 8000, 1, 50000, 100000),
         ("d_16k_mono.flac", 16000, 1, 70000, 70000)]


def _pcm(n, ch, seed):
    rng = np.random.default_rng(seed)
    x = np.clip(np.round(3000 * rng.standard_normal((n, ch))), -32768, 32767).astype(np.int64)
    return x[:, 0] if ch == 1 else x


@pytest.fixture(scope="module")
def setup(tmp_path_factory, golden):
    import main as cli  # noqa: F401  (puts the package on sys.path)
    from scipy.io import wavfile
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    root = tmp_path_factory.mktemp("recordings_convert")
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
    paths = []
    for k, (name, rate, ch, frames, n16) in enumerate(FILES):
        assert math.ceil(16000 * frames / rate) == n16
        p = root / name
        x = _pcm(frames, ch, seed=10 + k)
        if name.endswith(".wav"):
            wavfile.write(p, rate, x.astype(np.int16))
        else:
            p.write_bytes(encode(x, sample_rate=rate, plan=lambda f, c, b: {"kind": "verbatim"}))
        paths.append(p)
    return {"root": root, "conf": conf, "model": model, "weights": weights, "paths": paths}


def _spread(model, x16):
    """The scorer's own run-to-run spread on one batch (the rule of tests/test_recordings_gpu.py)."""
    from radhip.infer import _scores
    from radhip.recordings import AMP
    first = torch.from_numpy(np.stack([x16[:WIN]] * BATCH)).cuda()
    with torch.no_grad():
        a, b = (_scores(model, first, None, AMP["x3"]).float().cpu().numpy() for _ in range(2))
    return float(np.abs(a - b).max())


def _same(a, b, spread, what):
    if spread == 0.0:
        assert a == b, (what, a, b)
    else:
        assert abs(a - b) <= 4 * spread, (what, a, b, spread)


def _same_records(got, want, spread, keys=("score", "min", "max")):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["n_samples"], g["n_windows"]) == (w["n_samples"], w["n_windows"])
        if spread == 0.0:
            assert g["argmin_start"] == w["argmin_start"]
        for k in keys:
            _same(g[k], w[k], spread, k)
        if "window_scores" in g and "window_scores" in w:
            assert g["window_starts"] == w["window_starts"]
            for a, b in zip(g["window_scores"], w["window_scores"]):
                _same(a, b, spread, "window score")


@pytest.fixture(scope="module")
def converted(setup):
    """The files' records with convert=True, and the converted signals written by ops.ingest_resample itself."""
    from radhip import audio, ops
    from radhip.recordings import RecordingScorer
    scorer = RecordingScorer(setup["model"], "cuda", amp="x3", batch_size=BATCH, hop=HOP, convert=True)
    recs = scorer.score(setup["paths"], timeline=True)
    tables = ops.IngestTables("cuda")
    signals = []
    for p, (name, rate, ch, frames, n16) in zip(setup["paths"], FILES):
        x = audio.read(p)[0].astype(np.float32).reshape(frames, ch)
        if (rate, ch) == (16000, 1):
            signals.append(x[:, 0].copy())
            continue
        dst = torch.empty(n16, device="cuda")
        ops.ingest_resample(torch.from_numpy(x.reshape(-1)).cuda(), dst, tables, [tables.job(rate, ch, frames, 0, 0)])
        signals.append(dst.cpu().numpy())
    return {"scorer": scorer, "records": recs, "signals": signals, "spread": _spread(setup["model"], signals[2])}


def test_lengths_windows_and_source_fields(setup, converted):
    from radhip.recordings import window_table
    recs = converted["records"]
    lens = [math.ceil(16000 * frames / rate) for _, rate, _, frames, _ in FILES]
    assert lens == [n16 for *_, n16 in FILES]
    assert [d["name"] for d in recs] == [str(p) for p in setup["paths"]]
    assert [d["n_samples"] for d in recs] == lens
    rec, start, seg = window_table(lens, HOP)
    assert [d["n_windows"] for d in recs] == np.diff(seg).tolist() == [2, 1, 3, 2]
    assert [s for d in recs for s in d["window_starts"]] == start.tolist()
    for d, (_, rate, ch, frames, _) in zip(recs, FILES):
        assert (d["source_rate"], d["source_channels"], d["source_frames"]) == (rate, ch, frames)
        assert d["argmin_start"] in d["window_starts"] and len(d["window_scores"]) == d["n_windows"]


def test_scores_are_those_of_the_converted_signals(setup, converted):
    from radhip.recordings import RecordingScorer
    plain = RecordingScorer(setup["model"], "cuda", amp="x3", batch_size=BATCH, hop=HOP)
    want = plain.score_arrays(converted["signals"], timeline=True)
    assert all("source_rate" not in d for d in want)
    _same_records(converted["records"], want, converted["spread"])


def test_identity_file_equals_the_unconverted_record(setup, converted):
    from radhip.recordings import RecordingScorer
    p = setup["paths"][3]
    plain = RecordingScorer(setup["model"], "cuda", amp="x3", batch_size=BATCH, hop=HOP).score([p], timeline=True)
    conv = converted["scorer"].score([p], timeline=True)
    _same_records(conv, plain, converted["spread"])
    assert (conv[0]["source_rate"], conv[0]["source_channels"], conv[0]["source_frames"]) == (16000, 1, 70000)


def test_small_chunks_give_the_same_records(setup, converted, monkeypatch):
    """Chunks cut by the raw and the converted cap (every recording alone here) score as one chunk does."""
    from radhip import recordings
    monkeypatch.setattr(recordings, "CHUNK_SAMPLES", 90000)
    again = converted["scorer"].score(setup["paths"], timeline=True)
    _same_records(again, converted["records"], converted["spread"])


def test_score_arrays_with_rates_agrees_with_files(setup, converted):
    from radhip import audio
    arrays = [audio.read(p)[0].astype(np.float32) for p in setup["paths"]]
    assert arrays[0].shape == (193802, 2) and arrays[1].ndim == 1
    got = converted["scorer"].score_arrays(arrays, rates=[r for _, r, *_ in FILES], timeline=True)
    _same_records(got, converted["records"], converted["spread"])
    assert [d["source_channels"] for d in got] == [2, 1, 1, 1]
    # one rate for all arrays (against the file alone: the same two windows in the same batch)
    one = converted["scorer"].score_arrays([arrays[0]], rates=48000)
    _same_records(one, converted["scorer"].score(setup["paths"][:1]), converted["spread"])


def test_cli_converts_with_the_flag_and_refuses_without(setup):
    import main as cli
    from radhip.audio import AudioReadError
    root, paths = setup["root"], setup["paths"]
    order = [paths[3], paths[0], paths[1], paths[2]]     # a conforming file first: the refusal names the second
    lst = root / "files.txt"
    lst.write_text("\n".join(str(p) for p in order) + "\n")
    out = root / "exp"
    common = ["--config", str(setup["conf"]), "--output_dir", str(out), "--eval_model_weights", str(setup["weights"]),
              "--score_files", str(lst)]
    with pytest.raises(AudioReadError, match=paths[0].name):
        cli.main(cli.parse_args(common + ["--comment", "plain"]))
    tag = out / "LA_Tiny_ep1_bs2_plain"
    assert not (tag / "recording_scores.txt").exists() and not (tag / "recording_timeline.txt").exists()
    os.environ.pop("WORLD_SIZE", None)
    cli.main(cli.parse_args(common + ["--score_convert", "--comment", "conv"]))
    os.environ.pop("WORLD_SIZE", None)
    rows = [ln.split(" ") for ln in (out / "LA_Tiny_ep1_bs2_conv" / "recording_scores.txt").read_text().splitlines()]
    assert [r[0] for r in rows] == [str(p) for p in order] and all(len(r) == 7 for r in rows)
    assert [int(r[1]) for r in rows] == [70000, 64601, 30000, 100000]
    assert [int(r[2]) for r in rows] == [2, 2, 1, 3]

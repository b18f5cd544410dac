"""The ingest stage of whole-recording scoring (csrc/ingest.hip, RecordingScorer(convert=True)) on one device.

Kernel arms, per input kind (48 kHz stereo, 44.1 kHz stereo, 8 kHz mono; `--recordings` seeded recordings of uneven
length whose 16 kHz lengths add up to about one CHUNK_SAMPLES = 2^24):
  ingest  rdx_ingest_resample: one call, interleaved input, down-mix and compact taps in the kernel;
  batch   the existing rdx_resample_batch on the same recordings, down-mixed to mono beforehand (not timed), dense taps,
          in calls of at most 64 jobs. This is the yardstick.
The two are alternated `--reps` times after `--warmup` untimed rounds, each timed by a pair of device events; reported
are the median, min, max and spread = (max - min) / median of each, ingest's algorithmic bytes (input + output floats,
the tap table not counted) over its median time as a share of the 8 TB/s HBM peak, and the largest |ingest - batch|.

End to end (`--e2e-recordings`, 0 to skip), with tools/bench_recordings.py's method (Phase-6 model, random-init
weights, x3, batch 32, hop 32300, a warm-up pass, then `--rounds` alternated timed passes ending in a synchronise):
  convert  RecordingScorer(convert=True).score_arrays on 48 kHz stereo recordings of 2 to 20 s;
  mono16   RecordingScorer().score_arrays on mono 16 kHz recordings of the same durations, the same session;
and the share of the convert pass spent in the conversion (device events around every rdx_ingest_resample call of a
pass, summed).
Prints one JSON line and writes it to profiles/ingest_bench.json.

    python tools/bench_ingest.py [--recordings 96] [--reps 20] [--e2e-recordings 64] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "robust-audio-deepfake-evolution_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
KINDS = [("48k_stereo", 48000, 2), ("44k1_stereo", 44100, 2), ("8k_mono", 8000, 1)]


def _stats(ms):
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / med, 4), "reps": len(ms)}


def kernel_arms(rate, ch, nrec, total_out, warmup, reps, dev):
    from radhip import _lib, ops
    rng = np.random.default_rng(rate + ch)
    w = rng.uniform(0.2, 1.8, nrec)
    out_lens = np.maximum((w / w.sum() * total_out).astype(np.int64), 1)
    frames = np.array([(n - 1) * rate // 16000 + 1 for n in out_lens], dtype=np.int64)
    out_lens = np.array([ops.ingest_out_len(f, rate) for f in frames], dtype=np.int64)
    roffs = np.concatenate([[0], np.cumsum(frames * ch)[:-1]])
    moffs = np.concatenate([[0], np.cumsum(frames)[:-1]])
    ooffs = np.concatenate([[0], np.cumsum(out_lens)[:-1]])
    gen = torch.Generator(device=dev).manual_seed(rate)
    src = (0.1 * torch.randn(int((frames * ch).sum()), device=dev, generator=gen)).clamp_(-1, 1)
    mono = torch.empty(int(frames.sum()), device=dev)
    for f, ro, mo in zip(frames, roffs, moffs):
        mono[mo:mo + f] = src[ro:ro + f * ch].view(f, ch).mean(dim=1)
    out_a = torch.zeros(int(out_lens.sum()), device=dev)
    out_b = torch.zeros_like(out_a)
    tables = ops.IngestTables(dev)
    jobs_a = [tables.job(rate, ch, f, ro, oo) for f, ro, oo in zip(frames, roffs, ooffs)]
    kern, width, og, ng = ops.resample_kernel(rate, 16000)
    kern = kern.to(dev).contiguous()
    jobs_b = [_lib.ResampleJob(int(mo), int(f), int(oo), int(n), og, ng, width, 0)
              for f, mo, oo, n in zip(frames, moffs, ooffs, out_lens)]

    def a():
        ops.ingest_resample(src, out_a, tables, jobs_a)

    def b():
        for i in range(0, len(jobs_b), 64):
            ops.resample_batch(mono, out_b, kern, jobs_b[i:i + 64])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a))
        tb.append(timed(b))
    nbytes = 4 * (int((frames * ch).sum()) + int(out_lens.sum()))
    sa, sb = _stats(ta), _stats(tb)
    ntap = tables.entry(rate)[2]
    ob, lds, in_lds = ops.ingest_plan(og, ng, ntap, ch)
    return {"rate": rate, "channels": ch, "recordings": nrec, "input_floats": int((frames * ch).sum()),
            "output_samples": int(out_lens.sum()), "ntap": ntap, "dense_taps": 2 * width + og, "block": ob,
            "lds_bytes": lds, "taps_in_lds": in_lds, "ingest": sa, "batch": sb,
            "batch_calls": -(-len(jobs_b) // 64),
            "batch_over_ingest": round(sb["median_ms"] / sa["median_ms"], 3),
            "ingest_bytes": nbytes, "ingest_bytes_per_s": round(nbytes / (sa["median_ms"] * 1e-3), 1),
            "ingest_share_of_hbm_peak": round(nbytes / (sa["median_ms"] * 1e-3) / HBM_PEAK, 4),
            "max_abs_diff_ingest_vs_batch": float((out_a - out_b).abs().max())}


def end_to_end(nrec, rounds, batch, hop, dev):
    from radhip import ops, recordings
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    cfg = load_config("Phase6_Proposed.conf")
    torch.manual_seed(1234)
    model = apply_lora_to_wavlm(get_model(cfg["model_config"], dev), cfg["training_config"]).eval()
    rng = np.random.default_rng(7)
    secs = rng.uniform(2.0, 20.0, nrec)
    x48 = [np.clip(0.1 * rng.standard_normal((int(s * 48000), 2)), -1, 1).astype(np.float32) for s in secs]
    x16 = [np.clip(0.1 * rng.standard_normal(ops.ingest_out_len(x.shape[0], 48000)), -1, 1).astype(np.float32)
           for x in x48]
    conv = recordings.RecordingScorer(model, dev, amp="x3", batch_size=batch, hop=hop, convert=True)
    plain = recordings.RecordingScorer(model, dev, amp="x3", batch_size=batch, hop=hop)
    spans = []
    real = recordings.ingest_resample

    def stamped(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real(*a, **k)
        e1.record()
        spans.append((e0, e1))
        return out
    recordings.ingest_resample = stamped
    arms = {"convert": lambda: conv.score_arrays(x48, rates=48000), "mono16": lambda: plain.score_arrays(x16)}
    nwin = {}
    for name, fn in arms.items():       # warm-up: weight planes, solver choices, the allocator's blocks, tap tables
        nwin[name] = sum(d["n_windows"] for d in fn())
    torch.cuda.synchronize()
    res = {name: [] for name in arms}
    share = []
    for _ in range(rounds):
        for name, fn in arms.items():
            spans.clear()
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            res[name].append({"seconds": round(dt, 4), "recordings_s": round(nrec / dt, 2),
                              "windows_s": round(nwin[name] / dt, 2)})
            if name == "convert":
                ms = sum(e0.elapsed_time(e1) for e0, e1 in spans)
                share.append({"ingest_ms": round(ms, 3), "calls": len(spans), "share_of_pass": round(ms * 1e-3 / dt, 5)})
    recordings.ingest_resample = real
    out = {"workload": f"{nrec} synthetic recordings of 2-20 s, Phase6_Proposed.conf, random-init weights, x3, batch "
                       f"{batch}, hop {hop}; convert: 48 kHz stereo through score_arrays(rates=48000); mono16: the "
                       "same durations as mono 16 kHz through the unconverted path, same session",
           "windows": nwin, "rounds": res, "conversion": share}
    for name in arms:
        r = [x["recordings_s"] for x in res[name]]
        med = float(np.median(r))
        out[name] = {"recordings_s_median": med, "spread": round((max(r) - min(r)) / med, 4)}
    out["convert_over_mono16"] = round(out["convert"]["recordings_s_median"] / out["mono16"]["recordings_s_median"], 4)
    out["conversion_share_median"] = float(np.median([s["share_of_pass"] for s in share]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=96)
    ap.add_argument("--total-out", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-recordings", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hop", type=int, default=32300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py measures on a ROCm GPU; none is visible")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "kernel": {}}
    for name, rate, ch in KINDS:
        res["kernel"][name] = kernel_arms(rate, ch, a.recordings, a.total_out, a.warmup, a.reps, dev)
    if a.e2e_recordings > 0:
        res["end_to_end"] = end_to_end(a.e2e_recordings, a.rounds, a.batch, a.hop, dev)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""The silence-trimming stage of whole-recording scoring (csrc/trim.hip, RecordingScorer(trim=...)) on one device.

Kernels (`--recordings` seeded recordings of uneven length adding up to one CHUNK_SAMPLES = 2^24, 30 % of every
recording exact zeros at the ends and in one inner gap, "gaps" mode, 40 dB, pad 10): rdx_trim_energy, rdx_trim_plan
and rdx_trim_compact, each timed by its own pair of device events, `--reps` times after `--warmup` untimed rounds.
Reported per kernel: median, min, max, spread = (max - min) / median, its algorithmic bytes (energy: the samples
read and the energies written; plan: energies read, prefix written and read twice, dst written; compaction: dst read
and the kept samples read and written) and those bytes over the median time as a share of the 8 TB/s HBM peak.

End to end (`--e2e-recordings`, 0 to skip), with tools/bench_recordings.py's method (Phase-6 model, random-init
weights, x3, batch 32, hop 32300, a warm-up pass per arm, then `--rounds` alternated timed passes that end in a
synchronise), on recordings of 2 to 20 s through score_arrays:
  loud list    no silence:  trim=None against trim="gaps" (the difference is what the stage costs);
  silent list  the same durations, 30 % zeros: trim=None against trim="gaps" (windows scored, recordings per second).
Prints one JSON line and writes it to profiles/trim_bench.json.

    python tools/bench_trim.py [--recordings 50] [--reps 20] [--e2e-recordings 48] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
F = 320


def _stats(ms):
    import numpy as np
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / med, 4), "reps": len(ms)}


def _silenced(x, rng):
    """x with 30 % of it zeroed: 10 % at each end and 10 % in one inner gap."""
    n = x.shape[0]
    a, g = n // 10, int(rng.integers(3 * n // 10, 6 * n // 10))
    x = x.copy()
    x[:a] = 0
    x[n - a:] = 0
    x[g:g + a] = 0
    return x


def kernels(nrec, total, warmup, reps, dev):
    import numpy as np
    import torch
    from radhip import ops
    rng = np.random.default_rng(11)
    w = rng.uniform(0.2, 1.8, nrec)
    lens = np.maximum((w / w.sum() * total).astype(np.int64), 1)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    host = (0.1 * rng.standard_normal(int(lens.sum()))).astype(np.float32)
    for o, n in zip(offs, lens):
        host[o:o + n] = _silenced(host[o:o + n], rng)
    sig = torch.from_numpy(host).to(dev)
    nf = -(-lens // F)
    frames = int(nf.sum())
    box = {}

    def energy():
        box["e"] = ops.trim_energy(sig, offs, lens)

    def plan():
        box["plan"] = ops.trim_plan(box["e"], lens, "gaps", 40.0, 10)

    energy()
    plan()
    kept_len = box["plan"][frames:].cpu().numpy()
    new_offs = np.concatenate([[0], np.cumsum(kept_len[:-1])])
    out = torch.empty(int(kept_len.sum()), device=dev)

    def compact():
        ops.trim_compact(sig, offs, lens, box["plan"][:frames], new_offs, out)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    arms = {"energy": energy, "plan": plan, "compact": compact}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    kept = int(kept_len.sum())
    nbytes = {"energy": 4 * int(lens.sum()) + 4 * frames, "plan": frames * (4 + 4 + 8 + 8) + 8 * nrec,
              "compact": 8 * frames + 8 * kept}
    res = {"recordings": nrec, "samples": int(lens.sum()), "frames": frames, "kept_samples": kept,
           "longest_recording_frames": int(nf.max()), "mode": "gaps", "db": 40.0, "pad": 10,
           "note": "each arm includes its host wrapper: table building, and for energy / plan the allocation of "
                   "their outputs from the caching allocator"}
    for k in arms:
        s = _stats(ms[k])
        s["bytes"] = nbytes[k]
        s["bytes_per_s"] = round(nbytes[k] / (s["median_ms"] * 1e-3), 1)
        s["share_of_hbm_peak"] = round(s["bytes_per_s"] / HBM_PEAK, 5)
        res[k] = s
    tot = sum(res[k]["median_ms"] for k in arms)
    res["sum_median_ms"] = round(tot, 4)
    res["dominant"] = max(arms, key=lambda k: res[k]["median_ms"])
    return res


ARMS = {"loud_none": ("loud", None), "loud_gaps": ("loud", "gaps"), "silent_none": ("silent", None),
        "silent_gaps": ("silent", "gaps")}


def end_to_end(nrec, rounds, batch, hop, dev):
    import numpy as np
    import torch
    from radhip import recordings
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    cfg = load_config("Phase6_Proposed.conf")
    torch.manual_seed(1234)
    model = apply_lora_to_wavlm(get_model(cfg["model_config"], dev), cfg["training_config"]).eval()
    rng = np.random.default_rng(7)
    secs = rng.uniform(2.0, 20.0, nrec)
    lists = {"loud": [np.clip(0.1 * rng.standard_normal(int(s * 16000)), -1, 1).astype(np.float32) for s in secs]}
    lists["silent"] = [_silenced(x, rng) for x in lists["loud"]]
    run = {}
    for name, (which, trim) in ARMS.items():
        scorer = recordings.RecordingScorer(model, dev, amp="x3", batch_size=batch, hop=hop, trim=trim)
        run[name] = lambda s=scorer, xs=lists[which]: s.score_arrays(xs)
    nwin = {name: sum(d["n_windows"] for d in fn()) for name, fn in run.items()}     # warm-up
    torch.cuda.synchronize()
    res = {name: [] for name in run}
    for _ in range(rounds):
        for name, fn in run.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            res[name].append({"seconds": round(dt, 4), "recordings_s": round(nrec / dt, 2),
                              "windows_s": round(nwin[name] / dt, 2)})
    out = {"workload": f"{nrec} synthetic mono 16 kHz recordings of 2-20 s through score_arrays, Phase6_Proposed.conf, "
                       f"random-init weights, x3, batch {batch}, hop {hop}; silent: 30 % of every recording zeroed",
           "windows": nwin, "rounds": res}
    for name in run:
        r = [x["recordings_s"] for x in res[name]]
        med = float(np.median(r))
        out[name] = {"recordings_s_median": med, "recordings_s": r, "spread": round((max(r) - min(r)) / med, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=50)
    ap.add_argument("--total", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-recordings", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hop", type=int, default=32300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trim_bench.json"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "robust-audio-deepfake-evolution_amd"), ROOT]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_trim.py measures on a ROCm GPU; none is visible")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    res["kernels"] = kernels(a.recordings, a.total, a.warmup, a.reps, dev)
    if a.e2e_recordings > 0:
        res["end_to_end"] = end_to_end(a.e2e_recordings, a.rounds, a.batch, a.hop, dev)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""The locating stage of whole-recording scoring (csrc/locate.hip, RecordingScorer(track=..., segments=...)) on one
device, by the method of tools/bench_trim.py.

Per call (`--recordings` recordings of uneven length adding up to one CHUNK_SAMPLES = 2^24 samples, about 52 000
frames, and ONE recording of that length, the long-scan case; seeded window scores; hops 32 300 and 3 200; the
threshold at the median of the track, merge 10, min_frames 25): rdx_track_overlap through ops.score_track (with its
host wrapper: tables, the upload of seg and the allocation of the track), rdx_track_segments and
rdx_track_segment_stats through their entry points on buffers allocated once, and ops.track_segments whole (both
kernels, the one copy back and the unpacking on the host). Each is timed by its own pair of device events, `--reps`
times after `--warmup` untimed rounds. Reported per arm: median, min, max, spread = (max - min) / median, and for the
three kernels their algorithmic bytes (track: scores and seg read, the track written; segments: the track read, bounds
and counts written; stats: the frames inside segments and their bounds read, three words per segment written) and
those bytes over the median time as a share of the 8 TB/s HBM peak.

End to end (`--e2e-recordings`, 0 to skip): Phase-6 model, random-init weights, x3, batch 32, hop 3 200, recordings of
2 to 20 s through score_arrays, a warm-up pass per arm, then `--rounds` alternated timed passes that end in a
synchronise:
  off      no new option;
  device   track=True, segments=thr (the device path);
  host     timeline=True, then track_np and segments_np per recording on the host (the alternative).
Prints one JSON line and writes it to profiles/locate_bench.json.

    python tools/bench_locate.py [--recordings 50] [--reps 20] [--e2e-recordings 24] [--rounds 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
F, WIN = 320, 64600


def _stats(ms):
    import numpy as np
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / med, 4), "reps": len(ms)}


def kernels(lens, hop, warmup, reps, dev):
    import numpy as np
    import torch
    from radhip import _lib, ops
    from radhip.recordings import window_table
    L = _lib.lib()
    rng = np.random.default_rng(13)
    lens = np.asarray(lens, dtype=np.int64)
    _, _, seg = window_table(lens, hop)
    scores = torch.from_numpy(rng.standard_normal(int(seg[-1])).astype(np.float32)).to(dev)
    nfr = -(-lens // F)
    foffs = np.concatenate([[0], np.cumsum(nfr[:-1])]).astype(np.int64)
    total, R = int(nfr.sum()), lens.size
    box = {"t": ops.score_track(scores, seg, lens, hop, WIN)}
    thr = float(np.median(box["t"].cpu().numpy()))
    ints = torch.empty(3, total, device=dev, dtype=torch.int32)
    flts = torch.empty(2, total, device=dev, dtype=torch.float32)
    count = torch.empty(R, device=dev, dtype=torch.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))     # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())                         # noqa: E731

    def track():
        box["t"] = ops.score_track(scores, seg, lens, hop, WIN)

    def segments():
        _lib.check(L.rdx_track_segments(p(box["t"]), ip(foffs), ip(nfr), R, thr, 10, 25, p(ints[0]), p(ints[1]),
                                        p(count), None), "track_segments")

    def stats():
        _lib.check(L.rdx_track_segment_stats(p(box["t"]), ip(foffs), ip(nfr), R, p(ints[0]), p(ints[1]), p(count),
                                             p(flts[0]), p(flts[1]), p(ints[2]), None), "track_segment_stats")

    def segments_op():
        box["found"] = ops.track_segments(box["t"], nfr, thr, 10, 25)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    arms = {"track": track, "segments": segments, "stats": stats, "segments_op": segments_op}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    nseg = sum(f[0].size for f in box["found"])
    inside = sum(int((f[1] - f[0] + 1).sum()) for f in box["found"])
    nbytes = {"track": 4 * int(seg[-1]) + 8 * (R + 1) + 4 * total, "segments": 4 * total + 8 * nseg + 4 * R,
              "stats": 4 * inside + 8 * nseg + 4 * R + 12 * nseg}
    res = {"recordings": R, "hop": hop, "windows": int(seg[-1]), "frames": total, "longest_recording_frames":
           int(nfr.max()), "threshold": thr, "merge": 10, "min_frames": 25, "segments_found": nseg,
           "frames_in_segments": inside, "windows_per_frame": round(min(WIN / hop + 1, float(seg[-1]) / R), 2)}
    for k in arms:
        s = _stats(ms[k])
        if k in nbytes:
            s["bytes"] = nbytes[k]
            s["bytes_per_s"] = round(nbytes[k] / (s["median_ms"] * 1e-3), 1)
            s["share_of_hbm_peak"] = round(s["bytes_per_s"] / HBM_PEAK, 6)
        res[k] = s
    return res


def host_locate(records, hop, thr, merge=10, min_frames=25):
    """The host alternative: the locating rule in numpy on the window scores a timeline=True pass brought back."""
    import numpy as np
    from radhip.recordings import segment_span, segments_np, track_np
    for d in records:
        t = track_np(d["n_samples"], d["window_scores"], hop).astype(np.float32)
        a, b, mean, lo, arg = segments_np(t, thr, merge, min_frames)
        start, end = segment_span(a, b, d["n_samples"])
        d["track_scores"] = t.tolist()
        d["segments"] = [{"start": s, "end": e, "frames": n, "mean": float(np.float32(mu)), "min": v,
                          "argmin_start": w * F}
                         for s, e, n, mu, v, w in zip(start.tolist(), end.tolist(), (b - a + 1).tolist(),
                                                      mean.tolist(), lo.tolist(), arg.tolist())]
    return records


def end_to_end(nrec, rounds, batch, hop, dev):
    import numpy as np
    import torch
    from radhip import recordings
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    cfg = load_config("Phase6_Proposed.conf")
    torch.manual_seed(1234)
    model = apply_lora_to_wavlm(get_model(cfg["model_config"], dev), cfg["training_config"]).eval()
    rng = np.random.default_rng(7)
    xs = [np.clip(0.1 * rng.standard_normal(int(s * 16000)), -1, 1).astype(np.float32)
          for s in rng.uniform(2.0, 20.0, nrec)]
    mk = lambda **kw: recordings.RecordingScorer(model, dev, amp="x3", batch_size=batch, hop=hop, **kw)   # noqa: E731
    first = mk(track=True).score_arrays(xs)
    thr = float(np.median(np.concatenate([d["track_scores"] for d in first])))
    off, on = mk(), mk(track=True, segments=thr)
    run = {"off": lambda: off.score_arrays(xs), "device": lambda: on.score_arrays(xs),
           "host": lambda: host_locate(off.score_arrays(xs, timeline=True), hop, thr)}
    warm = {name: fn() for name, fn in run.items()}     # warm-up
    torch.cuda.synchronize()
    nwin = sum(d["n_windows"] for d in warm["off"])
    agree = all([(s["start"], s["end"]) for s in a["segments"]] == [(s["start"], s["end"]) for s in b["segments"]]
                for a, b in zip(warm["device"], warm["host"]))
    secs = {name: [] for name in run}
    for _ in range(rounds):
        for name, fn in run.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[name].append(round(time.perf_counter() - t, 4))
    out = {"workload": f"{nrec} synthetic mono 16 kHz recordings of 2-20 s through score_arrays, Phase6_Proposed.conf, "
                       f"random-init weights, x3, batch {batch}, hop {hop}, threshold at the median of the track",
           "windows": nwin, "frames": sum(len(d["track_scores"]) for d in warm["device"]),
           "segments": sum(len(d["segments"]) for d in warm["device"]),
           "device_and_host_segment_bounds_agree_in_the_warm_up": agree, "seconds": secs}
    for name in run:
        med = float(np.median(secs[name]))
        out[name] = {"seconds_median": med, "spread": round((max(secs[name]) - min(secs[name])) / med, 4)}
    out["device_minus_off_s"] = round(out["device"]["seconds_median"] - out["off"]["seconds_median"], 4)
    out["host_minus_off_s"] = round(out["host"]["seconds_median"] - out["off"]["seconds_median"], 4)
    out["off_spread_s"] = round(max(secs["off"]) - min(secs["off"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=50)
    ap.add_argument("--total", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-recordings", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hop", type=int, default=3200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_bench.json"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "robust-audio-deepfake-evolution_amd"), ROOT]
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_locate.py measures on a ROCm GPU; none is visible")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "note": "track and segments_op include their host wrappers (tables, allocation from the caching allocator; "
                   "segments_op also the copy back and the unpacking); segments and stats are the entry points alone",
           "kernels": {}}
    w = np.random.default_rng(11).uniform(0.2, 1.8, a.recordings)
    uneven = np.maximum((w / w.sum() * a.total).astype(np.int64), 1)
    for hop in (32300, 3200):
        res["kernels"][f"uneven_hop{hop}"] = kernels(uneven, hop, a.warmup, a.reps, dev)
        res["kernels"][f"single_hop{hop}"] = kernels([a.total], hop, a.warmup, a.reps, dev)
    if a.e2e_recordings > 0:
        res["end_to_end"] = end_to_end(a.e2e_recordings, a.rounds, a.batch, a.hop, dev)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Whole-recording scoring throughput (radhip/recordings.py) on the full Phase-6 model, random-init weights as
tools/bench_eval.py builds it: a seeded synthetic set of 64 recordings of 2 to 20 s at 16 kHz, hop 32300, batch 32, x3.

Three arms, alternated `--rounds` times on one device:
  new    RecordingScorer.score_arrays: packed upload, rdx_window_gather into full batches shared between recordings,
         rdx_segment_reduce;
  host   the obvious host-side alternative: per recording, numpy windows, one upload and one _scores call over that
         recording's windows (batches of 1 to 13 windows), numpy reduction;
  fixed  tools/bench_eval.py's fixed-length pass: 6 resident batches of 32 x 64600 samples through _scores.
Prints one JSON line (recordings/s and windows/s per arm and round, medians, spread = (max - min) / median) and
writes it to profiles/recordings_bench.json.

    python tools/bench_recordings.py [--recordings 64] [--rounds 3] [--batch 32]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hop", type=int, default=32300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recordings_bench.json"))
    a = ap.parse_args()
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    from radhip.infer import _scores
    from radhip.recordings import RecordingScorer, window_samples, window_table
    dev = torch.device("cuda", 0)
    cfg = load_config("Phase6_Proposed.conf")
    torch.manual_seed(1234)
    model = apply_lora_to_wavlm(get_model(cfg["model_config"], dev), cfg["training_config"]).eval()
    rng = np.random.default_rng(7)
    lens = rng.integers(2 * 16000, 20 * 16000 + 1, a.recordings)
    xs = [np.clip(0.1 * rng.standard_normal(n), -1, 1).astype(np.float32) for n in lens]
    rec, start, seg = window_table(lens, a.hop)
    nwin = int(rec.size)
    fixed = [torch.from_numpy(np.clip(0.1 * rng.standard_normal((a.batch, 64600)), -1, 1).astype(np.float32)).to(dev)
             for _ in range(6)]
    scorer = RecordingScorer(model, dev, amp="x3", batch_size=a.batch, hop=a.hop)

    def new():
        return [d["score"] for d in scorer.score_arrays(xs)]

    @torch.no_grad()
    def host():
        out = []
        for r, x in enumerate(xs):
            w = np.stack([window_samples(x, s) for s in start[seg[r]:seg[r + 1]]])
            s = _scores(model, torch.from_numpy(w).to(dev), None, "x3").float().cpu().numpy()
            out.append(float(s.astype(np.float64).mean()))
        return out

    @torch.no_grad()
    def fixed_pass():
        out = [_scores(model, x, None, "x3") for x in fixed]
        torch.cuda.synchronize()
        return out

    arms = {"new": (new, a.recordings, nwin), "host": (host, a.recordings, nwin),
            "fixed": (fixed_pass, a.batch * 6, a.batch * 6)}
    for fn, _, _ in arms.values():      # warm-up: weight planes, solver choices, the allocator's blocks
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in arms}
    means = {}
    for _ in range(a.rounds):
        for name, (fn, nrec, nw) in arms.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            means[name] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            rounds[name].append({"seconds": round(dt, 4), "recordings_s": round(nrec / dt, 2),
                                 "windows_s": round(nw / dt, 2)})
    res = {"workload": f"{a.recordings} synthetic recordings of 2-20 s ({int(lens.sum())} samples, {nwin} windows at hop "
                       f"{a.hop}), Phase6_Proposed.conf, random-init weights, x3, batch {a.batch}; fixed: 6 x {a.batch} "
                       "utterances of 64600 samples resident on the device (tools/bench_eval.py's pass)",
           "rounds": rounds}
    for name in arms:
        w = [r["windows_s"] for r in rounds[name]]
        med = float(np.median(w))
        res[name] = {"windows_s_median": med, "recordings_s_median": float(np.median([r["recordings_s"]
                                                                                      for r in rounds[name]])),
                     "spread": round((max(w) - min(w)) / med, 4)}
    res["new_over_host"] = round(res["new"]["windows_s_median"] / res["host"]["windows_s_median"], 3)
    res["new_over_fixed"] = round(res["new"]["windows_s_median"] / res["fixed"]["windows_s_median"], 3)
    res["max_abs_mean_diff_new_vs_host"] = float(np.abs(np.array(means["new"]) - np.array(means["host"])).max())
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

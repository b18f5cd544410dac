"""The x3 scoring pass with and without the x3 SincNet stream (radhip/sinc_x3.py), and the stream's kernels alone.

Part 1: the workload of tools/bench_eval.py in x3 mode (Phase6_Proposed.conf, batch 32 x 64 600 samples, random-init
weights, radhip.infer._scores), RADHIP_X3_SINC=0 (the module path: MIOpen fp32 convolutions) and =1 alternating in
one process, `--repeats` timed windows of `--batches` batches each after a warm-up of both. The spread of the
RADHIP_X3_SINC=0 windows is the run-to-run noise a gain has to exceed.
Part 2: every launch shape of rdx_x3_b0x_fwd / rdx_x3_sconv_fwd at that batch, timed alone with device events:
microseconds, the three-product FLOP rate against the 2.5 PF bf16 MFMA peak, and the fp32 bytes in + out against
8 TB/s of HBM.

    python tools/bench_sinc_x3.py [--batch 32] [--batches 6] [--repeats 5] [--out profiles/sinc_x3_eval.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "robust-audio-deepfake-evolution_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

MFMA_PEAK, HBM_PEAK = 2.5e15, 8.0e12


def eval_ab(a, dev):
    from radhip.build import apply_lora_to_wavlm, get_model, load_config
    from radhip.infer import _scores
    cfg = load_config("Phase6_Proposed.conf")
    torch.manual_seed(1234)
    model = apply_lora_to_wavlm(get_model(cfg["model_config"], dev), cfg["training_config"]).eval()
    rng = np.random.default_rng(7)
    xs = [torch.from_numpy(np.clip(0.1 * rng.standard_normal((a.batch, 64600)), -1, 1).astype(np.float32)).to(dev)
          for _ in range(a.batches)]
    ms = {"0": [], "1": []}
    scores = {}
    with torch.no_grad():
        for flag in ("0", "1"):
            os.environ["RADHIP_X3_SINC"] = flag
            for i in range(a.warmup):
                _scores(model, xs[i % len(xs)], None, "x3")
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for flag in ("0", "1"):
                os.environ["RADHIP_X3_SINC"] = flag
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = [_scores(model, x, None, "x3") for x in xs]
                torch.cuda.synchronize()
                ms[flag].append((time.perf_counter() - t) / a.batches * 1e3)
                scores[flag] = torch.cat(out).double()
    os.environ.pop("RADHIP_X3_SINC", None)

    def row(v):
        med = statistics.median(v)
        return {"ms_per_batch": [round(t, 3) for t in v], "median_ms_per_batch": round(med, 3),
                "spread_ms": round(max(v) - min(v), 3), "utt_s": round(a.batch / med * 1e3, 1)}
    off, on = row(ms["0"]), row(ms["1"])
    gain = off["median_ms_per_batch"] - on["median_ms_per_batch"]
    return {"workload": f"Phase6_Proposed.conf x3 scoring pass, batch {a.batch} x 64600 samples, random-init weights",
            "batches_per_window": a.batches, "windows": a.repeats, "RADHIP_X3_SINC=0": off, "RADHIP_X3_SINC=1": on,
            "gain_ms_per_batch": round(gain, 3), "gain_exceeds_baseline_spread": bool(gain > off["spread_ms"]),
            "max_abs_score_diff": float((scores["0"] - scores["1"]).abs().max()),
            "wavlm_only_target": "20.3 ms per batch, about 1580 utt/s (round-6 record)"}


def kernels(a, dev):
    from radhip import sinc_x3, wavlm_x3
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)   # noqa: E731
    N, H = a.batch, 23
    w = (64600 - 129 + 1) // 3
    rows = []

    def timed(name, fn, flops, nbytes, shape):
        for _ in range(2):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.kreps)]
        for s, e in ev:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        us = statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3
        rows.append({"kernel": name, "shape": shape, "us": round(us, 1), "x3_tflops": round(flops / us * 1e-6, 1),
                     "of_bf16_mfma_peak": round(flops / (us * 1e-6) / MFMA_PEAK, 4),
                     "gb_s": round(nbytes / us * 1e-3, 1), "of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)})

    def planes(co, ci, kh):
        return wavlm_x3.planes(rnd(kh * 3, co, ci) / (kh * 3 * ci) ** 0.5)

    x = rnd(N, H, w)
    args = (x, torch.tensor([1.0, 0.1], device=dev), rnd(32, 6) * 0.4, rnd(32, 3) * 0.5,
            torch.stack([rnd(32) * 0.1, rnd(32) * 0.1, 1 + 0.1 * rnd(32), rnd(32) * 0.1]).contiguous(),
            planes(32, 32, 2), rnd(32) * 0.1)
    timed("x3_b0x_fwd", lambda: sinc_x3.b0x(*args), 3 * 2.0 * N * H * w * 6 * 32 * 32,
          4.0 * N * H * w + 4.0 * N * H * (w // 3) * 32, [N, H, w])
    del x, args
    w //= 3
    for ci, co, down in sinc_x3._LAYOUT:
        cases = [("conv1", ci, co, 2, 1, H, True), ("conv2", co, co, 2, 0, H + 1, False)]
        if down:
            cases.append(("conv_downsample", ci, co, 1, 0, H, False))
        for what, c_in, c_out, kh, ph, h, bn in cases:
            x = rnd(N, h, w, c_in)
            wp = planes(c_out, c_in, kh)
            tbl = torch.stack([rnd(c_out) * 0.1, rnd(c_out) * 0.1, 1 + 0.1 * rnd(c_out), rnd(c_out) * 0.1]).contiguous()
            ho = h + 2 * ph - kh + 1
            timed("x3_sconv", lambda: sinc_x3.sconv(x, wp, kh, ph, bn=tbl if bn else None),
                  3 * 2.0 * N * ho * w * kh * 3 * c_in * c_out, 4.0 * N * w * (h * c_in + ho * c_out),
                  [what, N, h, w, c_in, c_out, kh, ph])
            del x
        w //= 3
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinc_x3_eval.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinc_x3 needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    res = {"eval": eval_ab(a, dev)}
    torch.cuda.empty_cache()
    res["kernels"] = kernels(a, dev)
    res["kernels_total_us_per_batch"] = round(sum(r["us"] for r in res["kernels"]), 1)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Phase-6 training throughput on MI355X (BASELINE.json metric: train utts/sec).

One step = one optimizer step of the Phase-6 recipe on every rank: `accum` (4) micro-batches of
`micro_batch` (8) synthetic utterances, each micro-batch = GPU RawBoost (algo 5, p 0.8) + codec
resampling (p 0.3 x 0.5) + pad_random/tile to 64 600 + mixup, fp16-autocast forward (the reference's dtype,
src/main.py:28,1049; the kernels of libradhip_f16.so; --amp bf16 runs libradhip.so) of the full DualStreamSEMamba (random-init WavLM-Large + LoRA r8 q/v, SincNet, 4 Bi-Mamba layers), focal loss,
backward (GradScaler-scaled, as src/main.py:1077-1108), FGM attack (eps 0.5 on feature_projection) + adversarial
forward/backward + restore; then all-reduce (RCCL, N > 1), unscale + clip 3.0, AdamW, EMA, LR schedule. An utterance counts once per step.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line. A plain run does only what the headline figure needs: set-up, graph capture, W warm-up
steps, the K timed steps, and the line (throughput, `ms_per_step`, configuration, loss). `--dump-outputs DIR` also
writes what the last timed step left behind (see dump_outputs). `--full` adds everything else: `roofline` for the
dominant hand-written HIP kernel of the step (largest total time) with the per-kernel and per-shape tables, timed
with device clock stamps over a kernel-timing region of K more steps (HIP events on the launch stream with --eager),
and `cpu_baseline`, which times the oracle (CPU restatement, fp32) on a bounded sample on the host cores.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "robust-audio-deepfake-evolution_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")  # see radhip/__init__.py (graph memset replay)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAKS = {"hbm": 8000.0, "fp32": 157.3, "bf16": 2500.0}  # GB/s ; TFLOP/s (MI355X_MICROARCH.md, dense; "bf16" = the
# 16-bit MFMA peak, which fp16 shares: --amp fp16 runs the same kernels from libradhip_f16.so at the same rate)
KERNEL_BOUND = {"sincconv_absmaxpool": ("mfma", "fp32"), "sincconv_mfma": ("mfma", "bf16"), "selective_scan_fwd": ("hbm", None),
                "selective_scan_bwd": ("hbm", None), "layer_wsum_fwd": ("hbm", None),
                "layer_wsum_bwd": ("hbm", None), "rawboost_batch": ("hbm", None),
                "attn_fwd": ("mfma", "bf16"), "attn_bwd": ("mfma", "bf16"),
                "posconv_fwd": ("mfma", "bf16"), "posconv_bwd": ("mfma", "bf16"),
                "sincnet_b0_bwd": ("hbm", None), "sincnet_b0_fwd": ("hbm", None),
                "b0x_fwd": ("mfma", "bf16"), "b0x_bwd": ("mfma", "bf16"), "wgrad_acc": ("mfma", "bf16"), "wgrad_many": ("mfma", "bf16"),
                "sconv_fwd": ("hbm", None), "sconv_wgrad": ("hbm", None),
                "sconv_dgrad_bnselu": ("hbm", None),
                "fe_conv0": ("hbm", None), "fe_ln_gelu": ("hbm", None), "fe_conv_gemm": ("mfma", "bf16"),
                "gemm": ("mfma", "bf16"), "wgemm": ("mfma", "bf16"), "pgemm": ("mfma", "bf16"), "hgemm": ("mfma", "bf16"), "lgemm": ("mfma", "bf16"), "sincconv_abspool1d": ("mfma", "fp32")}
TRAIN_FLOP_PER_UTT = 0.72e12                # SURVEY.md §8d (algorithmic, FGM step)


class Heartbeat:
    """A line on stderr every `every` seconds naming the current phase: a first run on a fresh box spends
    minutes in MIOpen find / graph capture without other output."""

    def __init__(self, every=30.0):
        import threading
        self.phase, self.t0 = "start", time.time()
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, args=(every,), daemon=True)
        self._th.start()

    def _run(self, every):
        while not self._stop.wait(every):
            print(f"[bench] {self.phase} ({time.time() - self.t0:.0f} s)", file=sys.stderr, flush=True)

    def set(self, phase):
        self.phase = phase
        print(f"[bench] {phase} ({time.time() - self.t0:.0f} s)", file=sys.stderr, flush=True)

    def stop(self):
        self._stop.set()


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)   # ~1.5 s of GPU work; 5 steps read +-1 %
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro-batch", type=int, default=8)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--amp", default="fp16", choices=["bf16", "fp16", "fp32"],
                    help="autocast dtype: fp16 + GradScaler = the reference's (default); bf16 the same kernels "
                         "with bf16 storage")
    ap.add_argument("--layerdrop", type=float, default=0.0,
                    help="WavLM LayerDrop during the bench (0 = every layer runs; never less work)")
    ap.add_argument("--pool", type=int, default=64, help="synthetic utterances resident in HBM per rank")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: per-kernel timings and the roofline "
                         "(a second graph capture and a kernel-timing region of --steps more steps) and the CPU "
                         "baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one left (trained parameters, EMA, mean loss) "
                         "as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--cpu-protocol", default="bounded", choices=["bounded", "full"],
                    help="bounded: B=2 (1 warm-up + 2 timed steps) and B=8 (1 + 1), ~1 min; full: BASELINE.md §3, B=2 and B=8, "
                         "3 warm-up + 10 timed steps each (~8 min on 16 threads)")
    ap.add_argument("--cpu-only", action="store_true", help="run only the CPU baseline leg (no GPU)")
    ap.add_argument("--config", default="Phase6_Proposed.conf")
    ap.add_argument("--lora-mode", default="reference", choices=["reference", "active"],
                    help="reference: the LoRA adapters are bypassed, as the reference's HF WavLM bypasses them "
                         "(DESIGN.md §2); active: the adapters are applied and trained")
    ap.add_argument("--eager", action="store_true",
                    help="launch the micro-step kernel by kernel instead of replaying it as HIP graphs")
    ap.add_argument("--no-window", action="store_true",
                    help="run the accumulation window micro-batch by micro-batch (reference order) instead of "
                         "batching its clean passes (radhip/window.py)")
    return ap.parse_args()


def dist_setup():
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if ws > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        torch.cuda.set_device(0)
    return ws, rank, local


def synthetic_pool(n, length, seed, device):
    """16 kHz utterances x = clip(0.1 N(0,1), -1, 1), labels Bernoulli(0.102)."""
    rng = np.random.default_rng(seed)
    x = np.clip(0.1 * rng.standard_normal((n, length)), -1, 1).astype(np.float32)
    y = (rng.random(n) < 0.102).astype(np.int64)
    return torch.from_numpy(x.reshape(-1)).to(device), torch.from_numpy(y)


def build(config, device, layerdrop):
    from radhip.build import apply_lora_to_wavlm, get_model
    torch.manual_seed(1234)
    model = get_model(config["model_config"], device)
    model = apply_lora_to_wavlm(model, config["training_config"])
    core = model.wavlm_stream._core()
    core.config.layerdrop = layerdrop
    return model


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, trainer):
    """What a caller of the timed path holds after its last step, as <out_dir>/<name>.npy (float32 / float64, at
    most DUMP_MAX_BYTES in all): `params`, every trained parameter (Trainer.params order, flattened and
    concatenated); `ema`, the EMA copy of the trainable parameters (EMA.names order); `loss`, the mean training
    loss per utterance over the warm-up and timed steps. An array over its share of the budget is written as a
    fixed sample (elements at sorted indices drawn from default_rng(0)), the same from run to run."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"params": [p.detach() for p in trainer.params]}
    if trainer.ema is not None and trainer.ema.shadow is not None:
        arrays["ema"] = list(trainer.ema.shadow)
    budget = (DUMP_MAX_BYTES - 4096) // (4 * len(arrays))      # float32 elements per array; .npy headers aside
    written = {}
    for name, tensors in arrays.items():
        flat = torch.cat([t.reshape(-1).float() for t in tensors]).cpu().numpy()
        if flat.size > budget:
            flat = flat[np.sort(np.random.default_rng(0).choice(flat.size, budget, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), flat)
        written[name] = int(flat.size)
    loss = np.array([float(trainer.loss_sum.item()) / max(trainer.n_seen, 1)], dtype=np.float64)
    np.save(os.path.join(out_dir, "loss.npy"), loss)
    written["loss"] = 1
    return written


def roofline_from_rows(rows, steps, graphed=False, split=False):
    """The dominant hand-written kernel = largest total time over the timed region (every launch site
    counted: GraphTimer scales its sampled sites), with its achieved rate over its average launch."""
    if not rows:
        return None, rows
    for r in rows.values():
        r["launches_per_step"] = round(r["launches"] / steps, 2)
        r["ms_per_step"] = r["total_ms"] / steps
    dom = max(rows, key=lambda k: rows[k]["total_ms"])
    r = rows[dom]
    bound, kind = KERNEL_BOUND.get(dom, ("hbm", None))
    if bound == "mfma":
        achieved = r["avg_work"] / (r["avg_ms"] * 1e-3) / 1e12
        peak, unit = PEAKS[kind], "TFLOP/s"
    else:
        achieved = r["avg_work"] / (r["avg_ms"] * 1e-3) / 1e9
        peak, unit = PEAKS["hbm"], "GB/s"
    traffic = None
    pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc):
        try:
            traffic = json.load(open(pmc)).get(dom, {}).get("hbm_bytes_per_launch")
        except Exception:
            traffic = None
    roof = {"bound": bound, "achieved": round(achieved, 3), "peak": peak, "unit": unit,
            "frac": round(achieved / peak, 4), "traffic": traffic, "kernel": dom,
            "avg_launch_ms": round(r["avg_ms"], 5), "work_per_launch": r["avg_work"],
            "work_unit": "FLOP" if bound == "mfma" else "bytes",
            "launches_per_step": r["launches_per_step"], "ms_per_step": round(r["ms_per_step"], 4),
            "timing": ("device wall-clock stamps (rdx_timestamp_acc) captured around the first 2 launch sites of each "
                       "kernel and shape in each replayed HIP graph (each standing for the graph's same-shape sites "
                       "of that kernel), accumulated over every replay"
                       + (" of a kernel-timing region of the same steps right after the timed region, replaying a "
                          "second capture of the window with these stamps and the SincNet branch serialized on the "
                          "main stream (the timed region replays unstamped graphs with the branch concurrent)"
                          if split else " of the timed region")
                       + "; each stamped launch minus the average of one empty stamp pair per graph (the stamps' own "
                         "cost, `stamp_overhead_us`); HIP events on the launch stream for eager launches") if graphed else
                      "HIP events on the launch stream around every launch of the timed region"}
    return roof, rows


def shape_table(shape_rows, kernel, steps):
    """Per-shape rows of `kernel` (keys "name[M, N, K]" for the GEMMs): launches and ms per step, µs per launch,
    work per launch and the achieved rate against its peak."""
    if not kernel:
        return None
    bound, kind = KERNEL_BOUND.get(kernel, ("hbm", None))
    out = {}
    for k, r in shape_rows.items():
        if not k.startswith(kernel + "[") or r["avg_ms"] <= 0:   # a shape with no timed launch (short runs)
            continue
        rate = r["avg_work"] / (r["avg_ms"] * 1e-3) / (1e12 if bound == "mfma" else 1e9)
        peak = PEAKS[kind] if bound == "mfma" else PEAKS["hbm"]
        out[k[len(kernel):]] = {"launches_per_step": round(r["launches"] / steps, 2),
                                "ms_per_step": round(r["total_ms"] / steps, 4), "us_per_launch": round(1e3 * r["avg_ms"], 2),
                                "work_per_launch": r["avg_work"], "achieved": round(rate, 1),
                                "frac": round(rate / peak, 4)}
    return out or None


def host_cpu():
    """(CPU model, physical cores of the machine, logical CPUs this process may run on)."""
    model, cores = None, set()
    try:
        phys = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "model name" and model is None:
                    model = v
                elif k == "physical id":
                    phys = v
                elif k == "core id":
                    cores.add((phys, v))
    except OSError:
        pass
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return model, (len(cores) or None), avail


def cpu_baseline(config, threads, protocol):
    """The oracle (CPU restatement, fp32; pinned to the reference by tests/golden) running the Phase-6
    train step of BASELINE.md §3 on the host cores: per micro-batch RawBoost algo 5 (p 0.8) + codec
    (p 0.3 x 0.5) in numpy, pad_random to 64 600, mixup, full WavLM-Large (random init) + SincNet +
    sequential Bi-Mamba, focal loss (alpha 0.9, gamma 2.5), backward, FGM attack (eps 0.5) + adversarial
    forward/backward + restore; clip 3.0 + AdamW every 4th micro-batch (accumulation 4).

    protocol "full" = BASELINE.md §3: 3 warm-up + 10 timed steps at micro-batch 2 and at 8, a step being
    one FGM micro-batch step (an optimizer step is 4 of them: the per-utterance rate is the same, and the
    optimizer-step reading at B = 8 would take ~25 min, past one GPU-box call).
    protocol "bounded" (bench default): 1 warm-up + 2 timed steps at micro-batch 2 and 1 + 3 at micro-batch 8
    (~1.5 min on the box's 16-CPU share; the reported value is the B = 8 rate, the reference's batch). The full
    protocol's result is committed under profiles/ (bench.py --cpu-only --cpu-protocol full)."""
    from oracle import rawboost as orb
    from oracle.data import pad_random
    from oracle.model import OracleModel
    from oracle.resample import codec_roundtrip
    import random as pyrandom
    from radhip.wavlm import WAVLM_LARGE
    torch.set_num_threads(threads)
    cfg = {k: v for k, v in WAVLM_LARGE.items()}
    cfg["layerdrop"] = 0.0
    cfg["conv_dim"] = tuple(cfg["conv_dim"])
    torch.manual_seed(0)
    m = OracleModel(cfg)
    for n, p in m.named_parameters():
        p.requires_grad_(not n.startswith("wavlm_stream.model.") or "feature_projection" in n)
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    train_params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(train_params, lr=1e-5)
    rng = np.random.default_rng(1234)
    pool = np.clip(0.1 * rng.standard_normal((16, 64000)), -1, 1)
    labels = (rng.random(16) < 0.102).astype(np.int64)

    def focal(logits, y, a=0.9, g=2.5):
        lp = torch.log_softmax(logits, 1).gather(1, y[:, None]).squeeze(1)
        return (-torch.where(y == 0, 1 - a, a) * (1 - lp.exp()) ** g * lp).sum() / (2 * y.shape[0])

    state = {"micro": 0}

    def step(B):
        idx = rng.integers(0, len(pool), B)
        batch = []
        for i in idx:
            x = pool[i]
            if pyrandom.random() < 0.8:
                x = orb.process(x, [1, 2, 3, 4])
            if pyrandom.random() < 0.3 and pyrandom.random() < 0.5:
                x = codec_roundtrip(x, pyrandom.choice([8000, 6000, 4000]))
            batch.append(pad_random(x))
        xb = torch.tensor(np.stack(batch), dtype=torch.float32)
        ys = torch.from_numpy(labels[idx])
        lam = float(np.random.beta(1, 1))
        perm = torch.randperm(B)
        xb = lam * xb + (1 - lam) * xb[perm]
        _, out = m(xb)
        loss = (lam * focal(out, ys) + (1 - lam) * focal(out, ys[perm])) / 4
        loss.backward()
        fp = [p for n, p in m.named_parameters() if "feature_projection" in n]
        bk = [p.data.clone() for p in fp]
        with torch.no_grad():
            for p in fp:
                nrm = p.grad.norm()
                if nrm != 0 and not torch.isnan(nrm):
                    p.add_(0.5 * p.grad / nrm)
        _, out = m(xb)
        ((lam * focal(out, ys) + (1 - lam) * focal(out, ys[perm])) / 4).backward()
        with torch.no_grad():
            for p, b in zip(fp, bk):
                p.copy_(b)
        state["micro"] += 1
        if state["micro"] % 4 == 0:
            torch.nn.utils.clip_grad_norm_(train_params, 3.0)
            opt.step()
            opt.zero_grad()

    plan = [(2, 3, 10), (8, 3, 10)] if protocol == "full" else [(2, 1, 2), (8, 1, 3)]
    runs = []
    for B, warm, timed in plan:
        for i in range(warm):
            step(B)
            print(f"[cpu_baseline] B={B} warm-up step {i + 1}/{warm}", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        for i in range(timed):
            step(B)
            print(f"[cpu_baseline] B={B} timed step {i + 1}/{timed} {time.perf_counter() - t0:.1f} s",
                  file=sys.stderr, flush=True)
        dt = time.perf_counter() - t0
        runs.append({"micro_batch": B, "warmup_steps": warm, "timed_steps": timed, "seconds": round(dt, 2),
                     "utt_s": round(B * timed / dt, 4)})
    model_name, phys, avail = host_cpu()
    best = runs[-1]
    return {"value": best["utt_s"], "unit": "utt/s", "cores": threads, "kind": "port",
            "sample": (f"{protocol} protocol: " + "; ".join(
                f"B={r['micro_batch']}: {r['warmup_steps']} warm-up + {r['timed_steps']} timed FGM micro-batch "
                f"steps, {r['seconds']} s" for r in runs)
                + " (fp32 CPU oracle: numpy RawBoost/codec, WavLM-Large + SincNet + Bi-Mamba fwd+bwd x2, "
                  "AdamW every 4th step)"),
            "runs": runs, "threads": threads, "cpu_model": model_name, "physical_cores_machine": phys,
            "logical_cpus_available": avail, "granted_cpus": granted_cpus(),
            "granted_evidence": ("OMP_NUM_THREADS=%s in the GPU box's environment: the harness grants one GPU's "
                                 "process a 16-CPU share and sets its thread pools to it; the affinity mask lists the "
                                 "whole machine's logical CPUs, which are not ours to use"
                                 % os.environ.get("OMP_NUM_THREADS", "unset"))}


CPU_FULL_PROTOCOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r04_cpu_baseline_full.json")


def protocol_baseline(live):
    """The line's cpu_baseline: BASELINE.md §3's full protocol (3 warm-up + 10 timed FGM micro-batch steps at B = 8,
    ~4 min of CPU, too long for every bench run) as measured by `bench.py --cpu-only --cpu-protocol full` on a GPU
    box's 16-CPU share and committed under profiles/; the live run of this bench (the bounded sample unless
    --cpu-protocol full) rides along as `live_sample`. A live full-protocol run is reported as is."""
    if live.get("sample", "").startswith("full"):
        return live
    try:
        with open(CPU_FULL_PROTOCOL) as f:
            full = json.load(f)["cpu_baseline"]
    except (OSError, ValueError, KeyError):
        return live
    out = dict(full)
    out["sample"] = (full["sample"] + "; committed result of the same oracle on a GPU box's 16-CPU share ("
                     + os.path.relpath(CPU_FULL_PROTOCOL, os.path.dirname(os.path.abspath(__file__)))
                     + "); this run's live bounded sample: live_sample")
    out["live_sample"] = live
    return out


def granted_cpus():
    """The CPU share granted to this process: OMP_NUM_THREADS as the GPU box sets it (16 per GPU), else the
    affinity mask."""
    try:
        return int(os.environ["OMP_NUM_THREADS"])
    except (KeyError, ValueError):
        return host_cpu()[2]


def cpu_threads(args):
    """Threads for the CPU leg: --cpu-threads, else every CPU of the granted share (16 on the GPU box)."""
    return args.cpu_threads or min(granted_cpus(), host_cpu()[2])


def main():
    args = parse()
    if args.cpu_only:
        from radhip.build import load_config
        res = cpu_baseline(load_config(args.config), cpu_threads(args), args.cpu_protocol)
        print(json.dumps({"cpu_baseline": res}), flush=True)
        return
    hb = Heartbeat()
    ws, rank, local = dist_setup()
    dev = torch.device("cuda", local)
    from radhip import ops
    from radhip.build import load_config
    from radhip.train import Augmenter, GraphedMicroStep, Trainer, total_optimizer_steps
    config = load_config(args.config)
    tc = config["training_config"]
    tc["accumulation_steps"] = args.accum
    tc["lora_mode"] = args.lora_mode
    config["batch_size"] = args.micro_batch
    amp = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.amp]
    model = build(config, dev, args.layerdrop)
    total_steps = args.steps + args.warmup
    trainer = Trainer(model, config, dev, total_optimizer_steps(1, total_steps * args.accum, args.accum), amp)
    dc = config["data_config"]
    aug = Augmenter(dev, algo=dc.get("rawboost_algo", 0), rawboost_p=dc.get("rawboost_p", 1.0),
                    use_codec=dc.get("use_codec_aug", False), codec_p=dc.get("codec_p", 0.5))
    L_RAW = 64000
    pool_x, pool_y = synthetic_pool(args.pool, L_RAW, 1234 + rank, dev)
    np.random.seed(1234 + rank)
    import random as pyrandom
    pyrandom.seed(1234 + rank)
    B = args.micro_batch
    graph, graph_timer, window, window_t = None, None, None, None
    if not args.no_window:
        from radhip.window import WindowStep
        window = WindowStep(trainer, B, graphs=not args.eager)
    elif not args.eager:
        graph = GraphedMicroStep(trainer, B)
    if not args.eager:
        hb.set("capturing HIP graphs")
        if args.full:
            graph_timer = ops.GraphTimer(dev)
        if window is not None:
            # the timed region replays unstamped graphs (SincNet stream as a concurrent branch); the kernel
            # timings come from a second capture of the same window with captured clock stamps around the
            # radhip launches and the branch serialized (as rocprofv3's kernel trace runs it), replayed over
            # a kernel-timing region of the same number of steps after the timed one
            def capture(w):
                for k in range(args.accum):     # capture needs one staged window of draws
                    w.add(k, np.zeros(B, dtype=np.int64))
                w.capture()
                w.reset_host()
            capture(window)
            if args.full:
                prev = os.environ.get("RADHIP_SINC_BRANCH")
                os.environ["RADHIP_SINC_BRANCH"] = "0"
                ops.CAPTURE_TIMING = graph_timer
                try:
                    # built under the switch: the window picks its batched adversarial SincNet stream at
                    # construction
                    window_t = WindowStep(trainer, B, graphs=True)
                    capture(window_t)
                finally:
                    ops.CAPTURE_TIMING = None
                    if prev is None:
                        os.environ.pop("RADHIP_SINC_BRANCH")
                    else:
                        os.environ["RADHIP_SINC_BRANCH"] = prev
        else:
            ops.CAPTURE_TIMING = graph_timer    # --full: clock stamps captured around every radhip launch
            graph.capture()
            ops.CAPTURE_TIMING = None

    cur = {"window": window}

    def micro(i, last):
        idx = np.random.randint(0, args.pool, size=B)
        offs = [int(j) * L_RAW for j in idx]
        lens = [L_RAW] * B
        plan = aug.draw(lens)
        lam, perm = trainer.mixup_draw(B)
        w = cur["window"]
        if w is not None:
            aug.run(pool_x, offs, lens, plan, perm, lam, out=w.xslot(i))
            w.add(i, pool_y[idx].numpy(), lam, perm)
            if last:
                w.run()
        elif graph is not None:
            aug.run(pool_x, offs, lens, plan, perm, lam, out=graph.x)
            graph.run(pool_y[idx].numpy(), lam, perm, last_in_epoch=last)
        else:
            x = aug.run(pool_x, offs, lens, plan, perm, lam)
            trainer.micro_step(x, pool_y[idx], lam, perm, last_in_epoch=last)

    def step():
        for i in range(args.accum):
            micro(i, i == args.accum - 1)

    hb.set("warm-up")
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if ws > 1:
        dist.barrier()
    torch.cuda.synchronize()
    hb.set("timed steps")
    split = window_t is not None            # kernel timings from their own region (see the capture above)
    ops.TIMING = {} if args.full and not split else None
    if graph_timer is not None:
        graph_timer.reset()
    stream = torch.cuda.current_stream(dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    prof = None
    if os.environ.get("RADHIP_TORCH_PROFILE"):     # tools: which framework ops launch the small kernels
        from torch.profiler import ProfilerActivity, profile
        prof = profile(activities=[ProfilerActivity.CPU], record_shapes=True)
        prof.__enter__()
    cprof = None
    if os.environ.get("RADHIP_CPROFILE"):          # tools: where the host spends a step (python-level)
        import cProfile
        cprof = cProfile.Profile()
        cprof.enable()
    for _ in range(args.steps):
        step()
    if cprof is not None:
        cprof.disable()
        import pstats
        with open(os.environ["RADHIP_CPROFILE"], "w") as f:
            pstats.Stats(cprof, stream=f).sort_stats("tottime").print_stats(60)
            pstats.Stats(cprof, stream=f).sort_stats("cumulative").print_stats(60)
    if prof is not None:
        prof.__exit__(None, None, None)
        with open(os.environ["RADHIP_TORCH_PROFILE"], "w") as f:
            f.write(prof.key_averages(group_by_input_shape=True).table(sort_by="count", row_limit=int(
                os.environ.get("RADHIP_TORCH_PROFILE_ROWS", "250")),
                                                                         max_name_column_width=40,
                                                                         max_shapes_column_width=120))
    ev1.record(stream)
    host_submit = time.perf_counter() - t0      # the host has issued every step (diagnostic: host- vs GPU-bound)
    torch.cuda.synchronize()
    if ws > 1:
        dist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dumped = None
    if args.dump_outputs and rank == 0:
        hb.set("writing outputs")
        dumped = dump_outputs(args.dump_outputs, trainer)
    if split:
        hb.set("kernel-timing steps")
        cur["window"] = window_t
        ops.TIMING = {}
        graph_timer.reset()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        cur["window"] = window
    timing, ops.TIMING = ops.TIMING, None
    rows = ops.event_rows(timing) if args.full else {}      # eager launches (augmentation, FGM)
    shape_rows = graph_timer.rows(by_shape=True) if graph_timer is not None else {}
    if graph_timer is not None:              # launches inside the replayed graphs
        for k, r in graph_timer.rows().items():
            if k in rows:
                a = rows[k]
                n = a["launches"] + r["launches"]
                a["avg_work"] = (a["avg_work"] * a["launches"] + r["avg_work"] * r["launches"]) / n
                a["launches"], a["total_ms"] = n, a["total_ms"] + r["total_ms"]
                a["avg_ms"] = a["total_ms"] / n
            else:
                rows[k] = r
    t = torch.tensor([wall], device=dev, dtype=torch.float64)
    if ws > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    wall_max = float(t.item())
    loss = trainer.epoch_loss()
    roof, rows = roofline_from_rows(rows, args.steps, graphed=not args.eager, split=split)
    if graph_timer is not None and roof is not None:
        khz = ops.lib().rdx_wallclock_khz(dev.index or 0)
        roof["stamp_overhead_us"] = round(graph_timer.overhead_ticks() / khz * 1e3, 3) if khz > 0 else None
    utts = ws * args.steps * args.accum * B
    value = utts / wall_max
    if rank == 0:
        line = {
            "metric": "Phase-6 train throughput (utterances/sec), DualStreamSEMamba + LoRA + RawBoost/codec + FGM",
            "value": round(value, 3), "unit": "utt/s", "n_gpus": ws, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1000 * wall_max / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.amp, "data": "synthetic (16 kHz, 64000 samples, clip(0.1 N(0,1)))",
            "config": {"workload": "Phase6_Proposed.conf train step on ASVspoof19-LA-shaped utterances",
                       "model": "DualStreamSEMamba (WavLM-Large random init + LoRA r8 q/v, SincNet, 4x PN-BiMamba)",
                       "micro_batch": B, "accumulation": args.accum, "global_batch": ws * B * args.accum,
                       "seq_len": 64600, "parallelism": f"dp{ws}", "fgm": True, "mixup": True,
                       "rawboost_algo": dc.get("rawboost_algo"), "codec_p": dc.get("codec_p"),
                       "wavlm_layerdrop": args.layerdrop, "lora_mode": args.lora_mode, "hip_graphs": not args.eager,
                       "window_batched_clean_passes": window is not None},
            "step_mfma_frac": round(value / ws * TRAIN_FLOP_PER_UTT / 2.5e15, 4),
            "final_loss": round(loss, 6),
            # host time to issue the K steps (no sync inside): close to ms_per_step means the GPU waited on the host
            "host_submit_ms_per_step": round(1000 * host_submit / args.steps, 3),
            "full": args.full,
        }
        if dumped is not None:
            line["dumped_outputs"] = dumped
        if args.full:
            line["roofline"] = roof
            line["kernels"] = {k: {kk: round(vv, 5) if isinstance(vv, float) else vv for kk, vv in v.items()}
                               for k, v in rows.items()}
            # the dominant kernel per (kernel, shape): every shape sampled in every graph (GraphTimer keys)
            line["kernel_shapes"] = shape_table(shape_rows, roof["kernel"] if roof else None, args.steps)
            if ws == 1 and not args.no_cpu_baseline:
                hb.set("cpu baseline")
                line["cpu_baseline"] = protocol_baseline(cpu_baseline(config, cpu_threads(args), args.cpu_protocol))
            else:
                line["cpu_baseline"] = None
        print(json.dumps(line), flush=True)
    hb.stop()
    if ws > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""dnet_amd flagship benchmark: Qwen-2.5 32B int8 pipelined-ring decode.

Measures the BASELINE.json headline metric — output tokens/sec (whole node)
plus p50 TTFT — on synthetic data with random-init weights (no network).

Single GPU:   python bench.py --steps 32 --warmup 8
Multi GPU:    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                  --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

One rank per GPU; ring hops are RCCL send/recv over xGMI. A "step" = every
sequence in every microbatch advances one token (one full ring round).
Rank 0 prints ONE JSON line.

A plain run does only what the headline figure needs: one prefill (to fill
the KV cache), warmup, the timed steps. ``--full`` adds the p50 TTFT over
several prefills and the individually timed step samples. ``--dump-outputs
DIR`` writes what the last timed step computed as DIR/<name>.npy; weights
and prompt tokens are seeded, so the inputs are identical from run to run.
On the GPU the benchmark switches the decode GEMMs to their reproducible
split-k mode (dnet_amd.ops.set_reproducible), so the dense-model outputs
are identical from run to run as well.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import time

import sys as _sys

import dnet_amd

# TunableOp algo cache covers the HEADLINE model's prefill shapes only;
# enabling it globally taxes eager-decode models (see enable_tunableop_cache)
def _bench_model_arg() -> str:
    av = _sys.argv
    for i, a in enumerate(av):
        if a == "--model" and i + 1 < len(av):
            return av[i + 1]
        if a.startswith("--model="):
            return a.split("=", 1)[1]
    return "qwen-2.5-32b"


if _bench_model_arg().startswith("qwen-2.5-32b"):
    dnet_amd.enable_tunableop_cache()
import torch

logging.basicConfig(level=logging.INFO)

from dnet_amd.models import ModelConfig, PRESETS, QuantConfig
from dnet_amd.parallel.comm import init_from_env
from dnet_amd.parallel.ring import RingExecutor


DUMP_BUDGET_BYTES = 60 << 20   # all dumped arrays together stay under 64 MB


def _dump_outputs(out_dir: str, ex: RingExecutor) -> None:
    """Write what the last decode step produced as <out_dir>/<name>.npy:

    tokens  float64 [mb_count, mb_size]         sampled token ids (first stage)
    logits  float32 [mb_count, mb_size, cols]   lm_head output (last stage)
    logits_columns  float64 [cols]              vocab ids of the logit columns

    All vocab columns are kept when they fit the budget; otherwise a fixed,
    seeded sample of columns (the same ones in every run)."""
    import numpy as np
    # one writer per file: tp_rank is the rank inside the stage group for
    # tensor AND context parallelism (tp and cp are mutually exclusive), so
    # only the group's rank 0 of the first / last stage writes
    if ex.tp_rank != 0:
        return
    os.makedirs(out_dir, exist_ok=True)
    if ex.is_first:
        toks = torch.stack([t.cpu() for t in ex.tokbuf]).to(torch.float64)
        np.save(os.path.join(out_dir, "tokens.npy"), toks.numpy())
    if ex.is_last:
        V = ex.cfg.vocab_size
        rows = ex.mb_count * ex.mb_size
        keep = min(V, max(1, DUMP_BUDGET_BYTES // (4 * rows) - 2))
        if keep < V:
            g = torch.Generator().manual_seed(2024)
            cols = torch.randperm(V, generator=g)[:keep].sort().values
        else:
            cols = torch.arange(V)
        logits = torch.stack([l.float().cpu()[:, cols] for l in ex.logits_buf])
        np.save(os.path.join(out_dir, "logits.npy"), logits.numpy())
        np.save(os.path.join(out_dir, "logits_columns.npy"),
                cols.to(torch.float64).numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--model", default="qwen-2.5-32b")
    ap.add_argument("--quant", default="int8",
                    choices=["int8", "int4", "bf16", "mxfp4"])
    ap.add_argument("--mb-size", type=int, default=64,
                    help="sequences per microbatch")
    ap.add_argument("--mb-per-rank", type=int, default=0,
                    help="microbatches = mb_per_rank * world (pipeline fill); "
                         "0 = auto (1 on a single GPU, 2 per rank otherwise)")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--smax", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=0,
                    help="override layer count (debug only; invalid for scoring)")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--kv-bits", type=int, default=16, choices=[8, 16])
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel degree inside each pipeline stage")
    ap.add_argument("--cp", type=int, default=1,
                    help="context-parallel degree (KV sequence sharding)")
    ap.add_argument("--prefill-chunk", type=int, default=0,
                    help="prefill position-chunk size (bounds activation "
                         "memory for long prompts; 0 = one shot)")
    ap.add_argument("--residency", type=int, default=0,
                    help="GPU-resident layers per rank (0=all; <local layers "
                         "enables host-DRAM weight streaming)")
    ap.add_argument("--full", action="store_true",
                    help="also measure p50 TTFT over several prefills and "
                         "individually timed step samples (extra GPU time)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's "
                         "outputs (tokens, logits) as DIR/<name>.npy")
    args = ap.parse_args()

    rank, world, device = init_from_env()
    on_gpu = device.type == "cuda"
    if on_gpu:
        # order-independent split-k sums: without it the last bit of every
        # decode GEMM varies per run and greedy sampling turns that into
        # different tokens, so two runs (or two builds) could not be
        # compared output for output. Same kernels, same speed.
        import dnet_amd.ops as ops
        ops.set_reproducible(True)

    quant = None
    if args.quant == "int8":
        quant = QuantConfig(8, 128)
    elif args.quant == "int4":
        quant = QuantConfig(4, 128)
    elif args.quant == "mxfp4":
        quant = QuantConfig(4, 32, fmt="mxfp4")   # expert banks only
    hf = dict(PRESETS[args.model])
    if args.layers:
        hf["num_hidden_layers"] = args.layers
    cfg = ModelConfig.from_hf(hf, quant=quant)

    mb_per_rank = args.mb_per_rank or (1 if world == 1 else 2)
    mb_count = max(mb_per_rank * world, 1)
    ex = RingExecutor(cfg, rank, world, device, mb_count=mb_count,
                      mb_size=args.mb_size, smax=args.smax, seed=1234,
                      use_graphs=on_gpu and not args.no_graphs and args.tp == 1,
                      residency=args.residency, tp=args.tp,
                      cp=args.cp,
                      kv_bits=args.kv_bits)

    g = torch.Generator().manual_seed(7)
    tokens = torch.randint(0, cfg.vocab_size,
                           (mb_count, args.mb_size, args.prompt_len),
                           generator=g).to(device)

    def barrier_sync():
        if world > 1:
            torch.distributed.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    # TTFT (--full): p50 over >= 5 prefills (a single
    # measurement is not a p50); each prefill resets the ring KV first.
    # A plain run prefills once, untimed, only to fill the KV cache.
    ttft_samples = []
    n_prefills = (max(1, int(os.environ.get("DNET_BENCH_PREFILLS", "5")))
                  if args.full else 1)
    for i in range(n_prefills):
        ex.reset()
        barrier_sync()
        t0 = time.perf_counter()
        ex.prefill(tokens, chunk=args.prefill_chunk)
        barrier_sync()
        ttft_samples.append((time.perf_counter() - t0) * 1e3)
    ttft_samples.sort()
    ttft_ms = ttft_samples[len(ttft_samples) // 2]

    # warmup decode
    ex.decode_rounds(args.warmup, collect=False)
    barrier_sync()

    t0 = time.perf_counter()
    ex.decode_rounds(args.steps, collect=False)
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # what the last timed step computed, copied out before anything else
    # advances the ring
    if args.dump_outputs:
        _dump_outputs(args.dump_outputs, ex)

    # self-corroboration (--full): a few individually timed steps AFTER the
    # timed region (sync per step), so the record shows per-step times
    # without cross-referencing profiles/
    step_samples = []
    for _ in range(3 if args.full else 0):
        barrier_sync()
        t1 = time.perf_counter()
        ex.decode_rounds(1, collect=False)
        barrier_sync()
        step_samples.append(round((time.perf_counter() - t1) * 1e3, 2))

    # max over ranks
    if world > 1:
        t = torch.tensor([elapsed], device=device if on_gpu else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t[0])

    total_seqs = mb_count * args.mb_size
    tokens_generated = total_seqs * args.steps
    toks_per_s = tokens_generated / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    if rank == 0:
        result = {
            "metric": f"output tokens/sec (whole node), {args.model} "
                      f"{args.quant} pipelined ring",
            "value": round(toks_per_s, 2),
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("bf16" if quant is None else
                      ("mxfp4 experts (bf16 attention/compute)"
                       if quant.fmt == "mxfp4" else
                       f"int{quant.bits}-g{quant.group} weights (bf16 compute)")),
            "data": "synthetic (random tokens, random-init weights)",
            "config": {
                "model": args.model,
                "global_batch": total_seqs,
                "seq_len": args.prompt_len,
                "gen_len": args.steps,
                "parallelism": (f"ring-pp{world // (args.tp * args.cp)}"
                                + (f"xtp{args.tp}" if args.tp > 1 else "")
                                + (f"xcp{args.cp}" if args.cp > 1 else ""))
                               + (f"+offload(res={args.residency})"
                                  if args.residency else ""),
                "microbatches": mb_count,
                "mb_size": args.mb_size,
                "layers": cfg.num_layers,
            },
        }
        if args.full:
            result["ttft_ms"] = round(ttft_ms, 1)
            result["ttft_samples_ms"] = [round(t, 1) for t in ttft_samples]
            result["step_samples_ms"] = step_samples
        print(json.dumps(result))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

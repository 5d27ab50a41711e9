"""Continuation-prefill attention over the latent MLA cache, both ways, on
one MI355X: ops.mla_prefill (absorbed, reads the cache in place) against
_expand_kv + ops.attn_prefill (kv_b over all p0 + T cached rows).

--what layer   one DeepSeek-V2-Lite attention block (16 heads, bf16 kv_b,
               B = 1), rmsnorm output in, lw.o input out, at p0 in {2048,
               8192} and T in {16 .. 512}: device events, the two paths
               alternating, median of --reps calls after 3 warm-ups; peak
               transient bytes (max_memory_allocated over the resident
               set) and the largest difference between the two outputs.
--what hit     first token of a prompt whose first 2048 tokens are in the
               prefix store plus 64 new ones, deepseek-v2-lite bf16 through
               the in-process ShardRuntime of prefix_cache_bench.py, with
               DNET_MLA_PREFILL=0 and =1 alternating.

    python scripts/mla_prefill_bench.py --what layer --out x.jsonl
    python scripts/mla_prefill_bench.py --what layer --rehearse  # CPU, tiny
                                    # shapes: checks the script, not a time
"""
import argparse
import json
import os
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

from dnet_amd.models import ModelConfig, PRESETS, get_ring_model  # noqa: E402


def bench_layer(out, reps, rehearse):
    dev = "cpu" if rehearse else "cuda:0"
    hf = dict(PRESETS["deepseek-v2-lite"])
    hf["num_hidden_layers"] = 1          # layer 0 is dense: no experts built
    cfg = ModelConfig.from_hf(hf)
    p0s, Ts = ((8,), (4,)) if rehearse else ((2048, 8192),
                                            (16, 32, 64, 128, 256, 512))
    smax = max(p0s) + max(Ts)
    m = get_ring_model("deepseek_v2")(cfg, range(1), dev, True, True,
                                      smax=smax)
    m.init_random(0)
    lw = m._layer(0)
    os.environ["DNET_MLA_PERHEAD"] = "0"
    kv = m.make_kv_cache(1, smax)
    gen = torch.Generator().manual_seed(1)
    kv.ckv.copy_(torch.randn(kv.ckv.shape, generator=gen))
    kv.kpe.copy_(torch.randn(kv.kpe.shape, generator=gen))
    m._absorbed(lw)                      # resident, as after the first decode
    paths = {"expanded": m._expanded_prefill, "absorbed": m._latent_prefill}
    cuda = not rehearse

    def sync():
        if cuda:
            torch.cuda.synchronize()

    for p0 in p0s:
        for T in Ts:
            y = torch.randn(T, cfg.hidden_size, generator=gen).to(
                torch.bfloat16).to(dev)
            pos = torch.arange(p0, p0 + T, device=dev)
            call = {k: (lambda f=f: f(y, lw, kv, 0, pos, 1, T, p0))
                    for k, f in paths.items()}
            res, peak = {}, {}
            for k, f in call.items():
                for _ in range(3):
                    res[k] = f()
                sync()
                if cuda:
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    r = f()
                    sync()
                    peak[k] = torch.cuda.max_memory_allocated() - base
                    del r
            ms = {k: [] for k in call}
            for _ in range(reps):
                for k, f in call.items():
                    if cuda:
                        a = torch.cuda.Event(enable_timing=True)
                        b = torch.cuda.Event(enable_timing=True)
                        a.record()
                        f()
                        b.record()
                        b.synchronize()
                        ms[k].append(a.elapsed_time(b))
                    else:
                        t0 = time.perf_counter()
                        f()
                        ms[k].append((time.perf_counter() - t0) * 1e3)
            diff = float((res["absorbed"].float()
                          - res["expanded"].float()).abs().max())
            out({"what": "layer_attention_ms", "p0": p0, "T": T, "reps": reps,
                 **{f"{k}_ms_median": statistics.median(v)
                    for k, v in ms.items()},
                 **{f"{k}_ms_min": min(v) for k, v in ms.items()},
                 **{f"{k}_peak_bytes": v for k, v in peak.items()},
                 "max_abs_diff": diff,
                 "out_abs_max": float(res["expanded"].float().abs().max())})


def bench_hit(out, reps):
    from prefix_cache_bench import Driver, bench_ttft
    d = Driver("deepseek-v2-lite", 27, "", 16, 4096, entries=2)
    for rnd in range(2):
        for flag in ("0", "1"):
            os.environ["DNET_MLA_PREFILL"] = flag
            bench_ttft(d, 2048, reps, out,
                       {"model": "deepseek-v2-lite", "round": rnd,
                        "DNET_MLA_PREFILL": flag})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("layer", "hit"), default="layer")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        sys.exit("needs a GPU (or --rehearse)")
    fh = open(a.out, "a") if a.out else None

    def out(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    if a.what == "layer":
        bench_layer(out, a.reps or (2 if a.rehearse else 30), a.rehearse)
    else:
        bench_hit(out, a.reps or 3)


if __name__ == "__main__":
    main()

"""Prefix-cache measurements on one MI355X, in process (no servers): an
in-process ShardRuntime on the synthetic Qwen-2.5-32B int8 entry, kv_bits 8
and 16, slot-scheduled (max_batch 4, max_seq 4096), prefix store on.

1. Admit -> first token (host clock from queueing the request to its first
   token frame, which the runtime emits after a device sync) for prompts
   whose first 512 / 2048 / 3584 tokens are in the store, against the SAME
   prompt sent with cache_prompt=false — what every request pays without
   the cache. Hit and cold alternate; each prompt has a fresh 64-token
   suffix.
2. ops.kv_copy_rows (slot -> store entry, all layers and planes, one
   launch) at those row counts, device events, next to the torch
   slice-assignment path on the same GPU tensors: one assignment per plane
   (the reference path) and one per layer per plane.
3. The int8-KV cost a hit still pays in prefill_window: dequantizing the
   slot's whole max_seq cache per layer, timed on its own.

    python scripts/prefix_cache_bench.py            # one JSON line per point
    python scripts/prefix_cache_bench.py --rehearse # tiny model on the CPU:
                                                    # checks the script, its
                                                    # times mean nothing
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from dnet_amd import ops  # noqa: E402
from dnet_amd.core.types import ShardLoadModelRequest  # noqa: E402
from dnet_amd.ops import reference as ref  # noqa: E402
from dnet_amd.shard.runtime import ShardRuntime  # noqa: E402

SUFFIX = 64


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def dev_ms(fn, n, warm=3):
    """Median / min ms of fn over n calls: device events on the GPU."""
    for _ in range(warm):
        fn()
    sync()
    out = []
    for _ in range(n):
        if torch.cuda.is_available():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        else:
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


class Driver:
    def __init__(self, model, layers, quant, kv_bits, max_seq, entries):
        self.frames = {}
        frames = self.frames

        class Cap:
            def send(self, fr):
                frames.setdefault(fr["nonce"], []).append(
                    (time.perf_counter(), fr))

            def close(self):
                pass

        self.rt = ShardRuntime("prefix-bench")
        self.rt._load(ShardLoadModelRequest(
            model_path=model, model_name=model, total_layers=layers,
            layers=list(range(layers)), rank=0, world_size=1, max_batch=4,
            max_seq=max_seq, kv_bits=kv_bits, quant=quant,
            prefix_entries=entries))
        self.rt._callback = Cap()
        self.vocab = int(self.rt.executor.cfg.vocab_size)
        self.n = 0

    def first_token_ms(self, tokens, **params):
        """Queue one single-token request; ms until its first frame."""
        self.n += 1
        nonce = f"r{self.n}"
        sync()
        t0 = time.perf_counter()
        self.rt.infer_q.put({
            "nonce": nonce, "prompt_len": len(tokens),
            "tokens": np.asarray(tokens, dtype=np.int32).tobytes(),
            "max_tokens": 1, "stop_ids": [], "params": params})
        for _ in range(64):
            self.rt._slots_tick()
            if nonce in self.frames:
                break
        t1, fr = self.frames[nonce][0]
        while not (all(s is None for s in self.rt.slots)
                   and self.rt._pending is None):
            self.rt._slots_tick()
        sync()
        return (t1 - t0) * 1e3, fr.get("cached_tokens")


def bench_ttft(d, cached, reps, out, tag):
    g = torch.Generator().manual_seed(cached)
    prefix = torch.randint(0, d.vocab, (cached,), generator=g).tolist()
    d.first_token_ms(prefix)                     # fills the store (and warms)
    hit, cold = [], []
    for i in range(reps + 1):
        sfx = torch.randint(0, d.vocab, (SUFFIX,), generator=g).tolist()
        h, n = d.first_token_ms(prefix + sfx)
        assert n == cached, (n, cached)
        c, n0 = d.first_token_ms(prefix + sfx, cache_prompt=False)
        assert n0 == 0
        if i:                                    # round 0 warms both shapes
            hit.append(h)
            cold.append(c)
    out({"what": "first_token_ms", **tag, "cached": cached,
         "prompt": cached + SUFFIX, "reps": reps,
         "hit_ms_median": statistics.median(hit), "hit_ms_min": min(hit),
         "cold_ms_median": statistics.median(cold), "cold_ms_min": min(cold),
         "speedup": statistics.median(cold) / statistics.median(hit)})


def bench_floor(d, reps, out, tag):
    """First token of a SUFFIX-token prompt on its own (no cache): what a
    hit would cost if the cached rows were free."""
    g = torch.Generator().manual_seed(7)
    ms = []
    for i in range(reps + 1):
        p = torch.randint(0, d.vocab, (SUFFIX,), generator=g).tolist()
        t, _ = d.first_token_ms(p, cache_prompt=False)
        if i:
            ms.append(t)
    out({"what": "suffix_only_first_token_ms", **tag, "prompt": SUFFIX,
         "ms_median": statistics.median(ms), "ms_min": min(ms)})


def bench_copy(d, rows, out, tag, n=30):
    slot = d.rt.executor.kvs[0].planes()
    store = d.rt.prefix_kv.planes()
    L = slot[0].shape[0]
    nbytes = sum(p.shape[0] * int(np.prod(p.shape[2:-2])) * rows
                 * p.shape[-1] * p.element_size() for p in slot)

    def per_layer():
        for dp, sp in zip(store, slot):
            for l in range(L):
                dp[l, 1, ..., :rows, :] = sp[l, 0, ..., :rows, :]

    res = {}
    for name, fn in (
            ("hip_one_launch", lambda: ops.kv_copy_rows(store, 1, slot, 0, 0,
                                                        rows)),
            ("torch_per_plane", lambda: ref.kv_copy_rows(store, 1, slot, 0,
                                                         0, rows)),
            ("torch_per_layer_plane", per_layer)):
        med, mn = dev_ms(fn, n)
        res[name + "_ms"] = med
        res[name + "_ms_min"] = mn
        res[name + "_payload_GBps"] = nbytes / (med * 1e-3) / 1e9
    out({"what": "kv_copy_rows", **tag, "rows": rows, "planes": len(slot),
         "layers": L, "payload_bytes": nbytes, **res})


def bench_dequant(d, out, tag, n=10):
    """What prefill_window pays per hit with int8 KV, besides its GEMMs:
    k_deq / v_deq of the slot's whole max_seq cache, every layer."""
    kv = d.rt.executor.kvs[0].slot(0)
    if not kv.quantized:
        return
    L = kv.k.shape[0]

    def deq():
        for li in range(L):
            kv.k_deq(li)
            kv.v_deq(li)

    med, mn = dev_ms(deq, n, warm=2)
    out({"what": "int8_kv_dequant_all_layers_ms", **tag, "layers": L,
         "ms_median": med, "ms_min": mn})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-bits", default="8,16")
    ap.add_argument("--cached", default="512,2048,3584")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        sys.exit("no GPU: nothing here can be measured on a CPU "
                 "(--rehearse only checks the script)")
    model, layers, quant, max_seq = "qwen-2.5-32b", 64, "int8-g128", 4096
    cached = [int(c) for c in a.cached.split(",")]
    if a.rehearse:
        model, layers, quant, max_seq = "tiny", 4, "", 256
        cached = [32, 128]
    sink = open(a.out, "w") if a.out else None

    def out(rec):
        if a.rehearse:
            rec["rehearsal_not_a_measurement"] = True
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for kv_bits in (int(b) for b in a.kv_bits.split(",")):
        tag = {"model": model, "quant": quant, "kv_bits": kv_bits,
               "max_seq": max_seq}
        t0 = time.perf_counter()
        d = Driver(model, layers, quant, kv_bits, max_seq, entries=2)
        out({"what": "load_s", **tag, "s": time.perf_counter() - t0,
             "store_bytes": d.rt.prefix_kv.nbytes(),
             "graphs": bool(d.rt.executor.use_graphs)})
        for c in cached:
            bench_ttft(d, c, a.reps, out, tag)
        bench_floor(d, a.reps, out, tag)
        for c in cached:
            bench_copy(d, c, out, tag)
        bench_dequant(d, out, tag)
        out({"what": "prefix_stats", **tag, **d.rt.prefix_stats()})
        d.rt._unload()
        del d
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

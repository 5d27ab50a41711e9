"""Time RowSampler.sample on bf16 logits at V = 152064 on one MI355X: the
fused HIP sampler against the torch sort path (fused = False, what
DNET_FUSED_SAMPLER=0 selects and what ran before the fused sampler
existed). Versions alternate; device events around each call.

The logprob mixes (every row asks for `top_logprobs=20`) also time the
logprob step on its own: the HIP logprob kernel on the bf16 logits against
the torch step it replaces (`.float()`, logsumexp, gather, topk over the
whole batch), with sampling excluded from both.

    python scripts/sampler_bench.py            # prints one JSON line per point
    python scripts/sampler_bench.py --mixes all_sampled,one_sampled
"""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from dnet_amd.core.sampler import DecodingConfig, RowSampler  # noqa: E402

V = 152064
STEP_MS = 16.4        # Qwen-2.5-32B int8 batch-64 decode step (README)
MIXES = ("all_sampled", "one_sampled", "all_sampled_pen", "one_biased",
         "all_greedy_logprobs20", "all_sampled_logprobs20")


def make(B, mix, fused):
    rs = RowSampler(B, device="cuda", vocab=V)
    rs.fused = fused
    sampled = dict(temperature=0.8, top_p=0.9, top_k=50)
    g = torch.Generator().manual_seed(1)
    for i in range(B):
        cfg = dict(sampled) if (mix != "one_sampled" or i == 0) else {}
        if mix == "all_sampled_pen":
            cfg.update(repetition_penalty=1.1, presence_penalty=0.5,
                       frequency_penalty=0.3)
        if mix.startswith("all_greedy"):
            cfg = {}
        if mix.endswith("logprobs20"):
            cfg.update(logprobs=True, top_logprobs=20)
        if mix == "one_biased" and i == 0:
            # one row with 24 entries among sampled rows
            cfg.update(logit_bias=dict(zip(
                torch.randint(0, V, (24,), generator=g).tolist(),
                (torch.rand(24, generator=g) * 8 - 4).tolist())))
        rs.set_row(i, DecodingConfig(**cfg))
        rs.note_prompt(i, torch.randint(0, V, (512,)).tolist())
    return rs


def timeit(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(fns, counts, rounds=3):
    acc = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            acc[k] += timeit(fn, counts[k])
    return {k: statistics.median(v) for k, v in acc.items()}, \
        {k: statistics.quantiles(v, n=10)[-1] for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixes", default=",".join(MIXES))
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    for B in (8, 64):
        logits = (torch.randn(B, V, device="cuda") * 3).to(torch.bfloat16)
        for mix in args.mixes.split(","):
            fus, tor = make(B, mix, True), make(B, mix, False)
            med, p90 = alternate(
                {"torch": lambda: tor.sample(logits),
                 "fused": lambda: fus.sample(logits)},
                {"torch": 10, "fused": 100})
            f, t = med["fused"], med["torch"]
            row = {"B": B, "mix": mix, "torch_ms": round(t, 4),
                   "fused_ms": round(f, 4), "speedup": round(t / f, 1),
                   "fused_p90_ms": round(p90["fused"], 4),
                   "fused_frac_of_step": round(f / STEP_MS, 4)}
            if mix.endswith("logprobs20"):
                # the logprob step alone, on the tokens just drawn
                tok = fus.sample(logits)
                med, p90 = alternate(
                    {"torch": lambda: tor._logprobs_for(logits.float(), tok),
                     "fused": lambda: fus._logprobs_for(logits, tok)},
                    {"torch": 10, "fused": 100})
                lf, lt = med["fused"], med["torch"]
                # the whole step as it ran before the logprob kernel: the
                # same sampling, then the torch logprob step
                nolp = make(B, mix[:-len("_logprobs20")], True)

                def before():
                    tor._logprobs_for(logits.float(), nolp.sample(logits))

                med, _ = alternate(
                    {"before": before, "fused": lambda: fus.sample(logits)},
                    {"before": 10, "fused": 100})
                row.update(step_before_ms=round(med["before"], 4),
                           step_speedup=round(med["before"] / med["fused"],
                                              1))
                row.update(lp_torch_ms=round(lt, 4), lp_fused_ms=round(lf, 4),
                           lp_fused_p90_ms=round(p90["fused"], 4),
                           lp_speedup=round(lt / lf, 1),
                           lp_fused_frac_of_step=round(lf / STEP_MS, 4))
            if args.tag:
                row["tag"] = args.tag
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

"""Time RowSampler.sample on bf16 logits at V = 152064 on one MI355X: the
fused HIP sampler against the torch sort path (fused = False, what
DNET_FUSED_SAMPLER=0 selects and what ran before the fused sampler
existed). Versions alternate; device events around each call.

    python scripts/sampler_bench.py            # prints one JSON line per point
"""
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from dnet_amd.core.sampler import DecodingConfig, RowSampler  # noqa: E402

V = 152064
STEP_MS = 16.4        # Qwen-2.5-32B int8 batch-64 decode step (README)


def make(B, mix, fused):
    rs = RowSampler(B, device="cuda", vocab=V)
    rs.fused = fused
    sampled = dict(temperature=0.8, top_p=0.9, top_k=50)
    for i in range(B):
        cfg = dict(sampled) if (mix != "one_sampled" or i == 0) else {}
        if mix == "all_sampled_pen":
            cfg.update(repetition_penalty=1.1, presence_penalty=0.5,
                       frequency_penalty=0.3)
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


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    for B in (8, 64):
        logits = (torch.randn(B, V, device="cuda") * 3).to(torch.bfloat16)
        for mix in ("all_sampled", "one_sampled", "all_sampled_pen"):
            fus, tor = make(B, mix, True), make(B, mix, False)
            acc = {"fused": [], "torch": []}
            for _ in range(3):
                acc["torch"] += timeit(lambda: tor.sample(logits), 10)
                acc["fused"] += timeit(lambda: fus.sample(logits), 100)
            f = statistics.median(acc["fused"])
            t = statistics.median(acc["torch"])
            print(json.dumps({
                "B": B, "mix": mix, "torch_ms": round(t, 4),
                "fused_ms": round(f, 4), "speedup": round(t / f, 1),
                "fused_frac_of_step": round(f / STEP_MS, 4)}), flush=True)


if __name__ == "__main__":
    main()

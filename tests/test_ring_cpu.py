"""Pipelined-ring executor tests on CPU: single-rank and 2-rank (gloo,
world_size=2 multi-process on localhost) must generate identical tokens to
each other for the same seed — the layer-seeded random init guarantees
identical global weights under any sharding."""
import multiprocessing as mp
import os
import socket

import pytest
import torch


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p

from conftest import retry_flaky
from dnet_amd.models import ModelConfig, PRESETS
from dnet_amd.parallel.ring import RingExecutor, RingPlan, split_layers

CFG = dict(PRESETS["tiny"])
MB_COUNT, MB_SIZE, T, NGEN = 2, 2, 7, 6


def _tokens(cfg):
    g = torch.Generator().manual_seed(123)
    return torch.randint(0, cfg.vocab_size, (MB_COUNT, MB_SIZE, T), generator=g)


def _run_single() -> torch.Tensor:
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, 0, 1, "cpu", mb_count=MB_COUNT, mb_size=MB_SIZE,
                      smax=64, seed=7, use_graphs=False)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    return torch.cat([first.unsqueeze(-1), gen], dim=-1)


def test_split_layers():
    assert split_layers(10, 3) == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]]
    assert split_layers(4, 1) == [[0, 1, 2, 3]]


def test_single_rank_ring():
    out = _run_single()
    assert out.shape == (MB_COUNT, MB_SIZE, NGEN + 1)
    # tokens should not be all identical (sanity)
    assert out.unique().numel() > 1


def _rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(360)
@retry_flaky()
def test_two_rank_ring_matches_single():
    single = _run_single()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out, single), f"ring-2 != single:\n{out}\n{single}"


@pytest.mark.timeout(360)
@retry_flaky()
def test_two_rank_ring_compressed_hops():
    """Ring with column-sparsified activation hops still generates sane
    tokens (lossy, so no exact-match; shapes/flow must hold)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main_compressed, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert out.shape == (MB_COUNT, MB_SIZE, NGEN + 1)


def _rank_main_compressed(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False,
                      compress_ratio=0.9)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(360)
@retry_flaky()
def test_tp2_matches_single():
    """One stage with TP=2 (sharded heads/MLP + gloo all-reduce) must
    generate exactly the single-rank tokens (same deterministic weights)."""
    single = _run_single()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main_tp, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out, single), f"tp2 != single:\n{out}\n{single}"


def _rank_main_tp(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False,
                      tp=2)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_pp2_tp2_matches_single():
    """4 ranks = 2 pipeline stages x TP 2 must equal the single-rank run."""
    single = _run_single()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main_pp_tp, args=(r, 4, port, q))
             for r in range(4)]
    for p in procs:
        p.start()
    out = q.get(timeout=200)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out, single)


def _rank_main_pp_tp(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False,
                      tp=2)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(360)
@retry_flaky()
def test_two_rank_two_rounds_matches_single():
    """k=2 ring rounds (interleaved layer windows, two laps per token) must
    equal the single-rank run (prima.cpp-style k-round pipelining)."""
    single = _run_single()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main_rounds, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out, single), f"k2 != single:\n{out}\n{single}"


def _rank_main_rounds(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor, RingPlan
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    # tiny has 4 layers: rank0 rounds [0],[2]; rank1 rounds [1],[3]
    plan = RingPlan([[[0], [2]], [[1], [3]]])
    ex = RingExecutor(cfg, rank, world, "cpu", plan=plan, mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


def test_bench_contract_multiproc_cpu(tmp_path):
    """The driver's SCALE invocation end-to-end: torch.distributed.run with
    2 ranks over gloo runs bench.py and rank 0 prints ONE valid JSON line
    with the contract fields."""
    import json
    import subprocess
    import sys

    port = _free_port()
    env = dict(os.environ)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1", "--model", "tiny",
         "--quant", "bf16", "--mb-size", "2", "--prompt-len", "8",
         "--smax", "32"],
        capture_output=True, text=True, timeout=300, env=env,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 2 and j["warmup"] == 1
    assert j["value"] > 0 and j["ms_per_step"] > 0
    assert j["scaling"] == "weak" and "config" in j
    assert j["config"]["global_batch"] == 2 * 2 * 2  # mb_count(2*2) * mb_size


def _bench_cpu(extra):
    """One single-process bench.py run of the tiny model on the CPU path
    (devices hidden from the child so it behaves the same on a GPU box)."""
    import json
    import subprocess
    import sys

    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
         "--warmup", "1", "--model", "tiny", "--quant", "bf16",
         "--mb-size", "2", "--prompt-len", "8", "--smax", "32"] + extra,
        capture_output=True, text=True, timeout=300, env=env,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_plain_full_and_dump_outputs_cpu(tmp_path):
    """A plain run carries the headline fields only; --full adds the TTFT
    and per-step samples; --dump-outputs writes the last timed step's
    tokens and logits, identical from run to run for the same arguments."""
    import numpy as np

    a, b = tmp_path / "a", tmp_path / "b"
    plain = _bench_cpu(["--dump-outputs", str(a)])
    full = _bench_cpu(["--full", "--dump-outputs", str(b)])
    for j in (plain, full):
        assert j["steps"] == 3 and j["warmup"] == 1
        assert j["value"] > 0 and j["ms_per_step"] > 0
        assert j["unit"] == "tokens/s" and j["higher_is_better"] is True
        assert j["dtype"] == "bf16" and "metric" in j
        # value is derived from the timed steps: batch 2, ms_per_step
        assert j["value"] == pytest.approx(2 * 1e3 / j["ms_per_step"],
                                           rel=1e-2)
    assert "ttft_ms" not in plain and "step_samples_ms" not in plain
    assert full["ttft_ms"] > 0 and len(full["ttft_samples_ms"]) == 5
    assert len(full["step_samples_ms"]) == 3

    vocab = CFG["vocab_size"]
    for d in (a, b):
        assert sorted(p.name for p in d.iterdir()) == [
            "logits.npy", "logits_columns.npy", "tokens.npy"]
    ta, la = np.load(a / "tokens.npy"), np.load(a / "logits.npy")
    assert ta.dtype == np.float64 and ta.shape == (1, 2)
    assert la.dtype == np.float32 and la.shape == (1, 2, vocab)
    assert np.isfinite(la).all()
    # the dumped tokens are the greedy sample of the dumped logits
    picked = np.take_along_axis(la, ta.astype(np.int64)[..., None], -1)
    assert (picked[..., 0] == la.max(-1)).all()
    assert (np.load(a / "logits_columns.npy") == np.arange(vocab)).all()
    assert (ta == np.load(b / "tokens.npy")).all()
    assert (la == np.load(b / "logits.npy")).all()


DS_CFG = dict(model_type="deepseek_v2", hidden_size=64, num_hidden_layers=3,
              num_attention_heads=4, num_key_value_heads=4, vocab_size=128,
              intermediate_size=128, kv_lora_rank=32, qk_nope_head_dim=16,
              qk_rope_head_dim=8, v_head_dim=16, n_routed_experts=4,
              num_experts_per_tok=2, n_shared_experts=1,
              moe_intermediate_size=32, first_k_dense_replace=1,
              routed_scaling_factor=1.0, rope_theta=10000.0)


def _ds_run_single():
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    cfg = ModelConfig.from_hf(DS_CFG)
    ex = RingExecutor(cfg, 0, 1, "cpu", mb_count=MB_COUNT, mb_size=MB_SIZE,
                      smax=64, seed=7, use_graphs=False)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    return torch.cat([first.unsqueeze(-1), gen], dim=-1)


def _ds_rank_main_tp(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(DS_CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False,
                      tp=2)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_deepseek_tp2_matches_single():
    """DeepSeek MLA with TP=2 (per-head q/kv_b/o sharding + EP experts +
    sliced shared experts) == single-rank, token-exact."""
    single = _ds_run_single()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ds_rank_main_tp, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out, single), f"ds tp2 != single:\n{out}\n{single}"


def _cp_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from dnet_amd.parallel.context import cp_attn_decode, shard_bounds
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(42)
    B, Hq, Hkv, S, D = 2, 8, 2, 96, 64
    qt = torch.randn(B, Hq, D, generator=g).to(torch.bfloat16)
    kc = torch.randn(B, Hkv, S, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, S, D, generator=g).to(torch.bfloat16)
    pos = torch.tensor([90, 33], dtype=torch.int32)
    s0, s1 = shard_bounds(S, world, rank)
    ln = (pos - s0).clamp(0, s1 - s0).to(torch.int32)
    out = cp_attn_decode(qt, kc[:, :, s0:s1].contiguous(),
                         vc[:, :, s0:s1].contiguous(), ln, D ** -0.5)
    if rank == 0:
        q.put(out)
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_context_parallel_attn_matches_full():
    """KV sequence sharded across 2 gloo ranks: gathered flash-decode
    partials combine to the full-attention result."""
    from dnet_amd.ops import reference as ref
    g = torch.Generator().manual_seed(42)
    B, Hq, Hkv, S, D = 2, 8, 2, 96, 64
    qt = torch.randn(B, Hq, D, generator=g).to(torch.bfloat16)
    kc = torch.randn(B, Hkv, S, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, S, D, generator=g).to(torch.bfloat16)
    pos = torch.tensor([90, 33], dtype=torch.int32)
    full = ref.attn_decode(qt, kc, vc, pos, D ** -0.5)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cp_rank_main, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.allclose(out.float(), full.float(), atol=3e-2, rtol=3e-2)


def _cp2_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False,
                      cp=2)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_cp2_matches_single():
    """One stage with context parallelism (KV sequence sharded across 2
    ranks, partials-combined attention) must generate the single-rank
    tokens (same deterministic weights)."""
    single = _run_single()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cp2_rank_main, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out, single), f"cp2 != single:\n{out}\n{single}"


def _ppcp_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False,
                      cp=2)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_pp2_cp2_matches_single():
    """4 ranks = 2 pipeline stages x CP 2 == the single-rank run."""
    single = _run_single()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ppcp_rank_main, args=(r, 4, port, q))
             for r in range(4)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out, single), f"pp2xcp2 != single:\n{out}\n{single}"


def _cp2_kv8_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False,
                      cp=2, kv_bits=8)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_cp2_kv8_matches_single_kv8():
    """CP + int8 KV cache: quantized shard writes and dequant-on-read
    combine must equal the single-rank int8-KV run token-exactly."""
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, 0, 1, "cpu", mb_count=MB_COUNT, mb_size=MB_SIZE,
                      smax=64, seed=7, use_graphs=False, kv_bits=8)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    single = torch.cat([first.unsqueeze(-1), gen], dim=-1)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cp2_kv8_rank_main, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out, single), f"cp2-kv8 != single-kv8:\n{out}\n{single}"


def _tiny_llama_sd(seed=99):
    """HF-llama-style state dict matching the tiny preset shapes."""
    g = torch.Generator().manual_seed(seed)
    cfg = ModelConfig.from_hf(CFG)
    H, I, nq, nkv, d = (cfg.hidden_size, cfg.intermediate_size,
                        cfg.num_q_heads, cfg.num_kv_heads, cfg.head_dim)

    def r(*shape):
        return (torch.randn(*shape, generator=g) / 10).to(torch.bfloat16)

    sd = {"model.embed_tokens.weight": r(cfg.vocab_size, H),
          "model.norm.weight": 1 + r(H) * 0.01,
          "lm_head.weight": r(cfg.vocab_size, H)}
    for lid in range(cfg.num_layers):
        p = f"model.layers.{lid}."
        sd[p + "input_layernorm.weight"] = 1 + r(H) * 0.01
        sd[p + "post_attention_layernorm.weight"] = 1 + r(H) * 0.01
        sd[p + "self_attn.q_proj.weight"] = r(nq * d, H)
        sd[p + "self_attn.k_proj.weight"] = r(nkv * d, H)
        sd[p + "self_attn.v_proj.weight"] = r(nkv * d, H)
        sd[p + "self_attn.o_proj.weight"] = r(H, nq * d)
        sd[p + "mlp.gate_proj.weight"] = r(I, H)
        sd[p + "mlp.up_proj.weight"] = r(I, H)
        sd[p + "mlp.down_proj.weight"] = r(H, I)
    return sd


def _ckpt_tp_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False,
                      tp=2, init_weights=False)
    ex.model.load_state_dict(_tiny_llama_sd())
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_tp2_checkpoint_load_matches_single():
    """Loading the SAME HF-style checkpoint under TP=2 (loader slices
    heads/MLP per rank) must reproduce the single-rank tokens."""
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, 0, 1, "cpu", mb_count=MB_COUNT, mb_size=MB_SIZE,
                      smax=64, seed=7, use_graphs=False, init_weights=False)
    ex.model.load_state_dict(_tiny_llama_sd())
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    single = torch.cat([first.unsqueeze(-1), ex.decode_rounds(NGEN)], dim=-1)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ckpt_tp_rank_main, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # all-reduce summation order can flip near-tie argmaxes a few tokens
    # in; a slicing bug would diverge at the very first token
    assert torch.equal(out[..., :4], single[..., :4]), \
        f"tp2 ckpt != single:\n{out}\n{single}"


GPTOSS_CFG = dict(model_type="gpt_oss", hidden_size=64, num_hidden_layers=3,
                  num_attention_heads=4, num_key_value_heads=2, head_dim=16,
                  vocab_size=128, intermediate_size=64, num_local_experts=4,
                  num_experts_per_tok=2, sliding_window=16,
                  rope_theta=10000.0, attention_bias=True, rms_norm_eps=1e-5)


def _gptoss_run(rank, world, port, q, tp):
    if world > 1:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                          MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          LOCAL_RANK=str(rank))
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    cfg = ModelConfig.from_hf(GPTOSS_CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=5, use_graphs=False,
                      tp=tp)
    toks = _tokens(cfg)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(NGEN)
    out = torch.cat([first.unsqueeze(-1), gen], dim=-1)
    if rank == 0:
        q.put(out) if q is not None else None
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return out


@pytest.mark.timeout(480)
@retry_flaky()
def test_gpt_oss_tp2_matches_single():
    """gpt-oss under TP=2: sliced qkv bias + per-head sinks + rank-0-only
    o bias + EP experts must reproduce the single-rank tokens."""
    single = _gptoss_run(0, 1, 0, None, 1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gptoss_run, args=(r, 2, port, q, 2))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # EP reorders expert partial sums across ranks (bf16), which can flip
    # near-tie argmaxes after a few steps on a random-init tiny model; a
    # sharding bug (bias double-count, wrong sink slice) diverges at the
    # FIRST token
    assert torch.equal(out[..., :3], single[..., :3]), \
        f"gpt-oss tp2 != single:\n{out}\n{single}"


def _slots_pp2_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    from dnet_amd.core.types import ShardLoadModelRequest
    from dnet_amd.shard.runtime import ShardRuntime
    layer_rounds = [[0, 1]] if rank == 0 else [[2, 3]]
    rt = ShardRuntime(f"s{rank}")
    rt._load(ShardLoadModelRequest(
        model_path="tiny", model_name="tiny", total_layers=4,
        layers=layer_rounds[0], layer_rounds=layer_rounds, rank=rank,
        world_size=2, master_addr="127.0.0.1", master_port=port + 1,
        max_batch=2, max_seq=64))
    emitted: dict = {}
    finished = [0]

    class Cap:
        def send(self, frame):
            emitted.setdefault(frame["nonce"], []).append(frame["token_id"])
            if frame.get("finished"):
                finished[0] += 1

        def close(self):
            pass

    if rank == 1:
        rt._callback = Cap()
    prompt = torch.arange(1, 9, dtype=torch.int32).numpy().tobytes()
    if rank == 0:
        rt.infer_q.put({"nonce": "a", "tokens": prompt, "prompt_len": 8,
                        "max_tokens": 6, "stop_ids": [], "params": {}})
        rt.infer_q.put({"nonce": "b", "tokens": prompt, "prompt_len": 8,
                        "max_tokens": 4, "stop_ids": [], "params": {}})
        while (any(s is not None for s in rt.slots)
               or not rt.infer_q.empty()):
            rt._slots_tick()
        q.put(("rank0", None))
    else:
        while finished[0] < 2:
            cmd = rt._recv_cmd()
            from dnet_amd.shard import runtime as R
            if cmd[0] == R.CMD_SLOT_ADMIT:
                rt._slot_admit_follower(cmd)
            elif cmd[0] == R.CMD_SLOT_STEP:
                rt._slot_step_exec()
        q.put(("rank1", emitted))
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_slots_pp2_matches_single():
    """Multi-rank continuous batching: 2 concurrent requests over a
    2-stage ring produce exactly the single-rank slot scheduler's tokens
    (same deterministic weights; the last stage samples and emits)."""
    # single-rank slots reference
    from dnet_amd.core.types import ShardLoadModelRequest
    from dnet_amd.shard.runtime import ShardRuntime
    emitted: dict = {}

    class Cap:
        def send(self, frame):
            emitted.setdefault(frame["nonce"], []).append(frame["token_id"])

        def close(self):
            pass

    rt = ShardRuntime("single")
    rt._load(ShardLoadModelRequest(
        model_path="tiny", model_name="tiny", total_layers=4,
        layers=[0, 1, 2, 3], rank=0, world_size=1, max_batch=2, max_seq=64))
    rt._callback = Cap()
    prompt = torch.arange(1, 9, dtype=torch.int32).numpy().tobytes()
    rt.infer_q.put({"nonce": "a", "tokens": prompt, "prompt_len": 8,
                    "max_tokens": 6, "stop_ids": [], "params": {}})
    rt.infer_q.put({"nonce": "b", "tokens": prompt, "prompt_len": 8,
                    "max_tokens": 4, "stop_ids": [], "params": {}})
    for _ in range(30):
        rt._slots_tick()
        if (all(s is None for s in rt.slots) and rt._pending is None
                and rt.infer_q.empty()):
            break
    rt._unload()
    assert len(emitted["a"]) == 6 and len(emitted["b"]) == 4

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_slots_pp2_rank_main, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        name, data = q.get(timeout=200)
        results[name] = data
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    pp2 = results["rank1"]
    assert pp2["a"] == emitted["a"], f"{pp2}\n{emitted}"
    assert pp2["b"] == emitted["b"]


def _chunk_rank_main(rank, world, port, q, chunk):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=7, use_graphs=False)
    toks = _tokens(cfg)
    first = ex.prefill(toks, chunk=chunk)
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_chunked_prefill_matches_full():
    """Prefill in 3-token position chunks (bounded activation memory for
    long prompts) == one-shot prefill, token-exact — single rank and over
    a 2-stage ring."""
    single = _run_single()
    cfg = ModelConfig.from_hf(CFG)
    ex = RingExecutor(cfg, 0, 1, "cpu", mb_count=MB_COUNT, mb_size=MB_SIZE,
                      smax=64, seed=7, use_graphs=False)
    toks = _tokens(cfg)
    first = ex.prefill(toks, chunk=3)
    out = torch.cat([first.unsqueeze(-1), ex.decode_rounds(NGEN)], dim=-1)
    assert torch.equal(out, single)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_chunk_rank_main, args=(r, 2, port, q, 3))
             for r in range(2)]
    for p in procs:
        p.start()
    out2 = q.get(timeout=150)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(out2, single)


MOE_CFG = dict(model_type="mixtral", hidden_size=64, num_hidden_layers=4,
               num_attention_heads=4, num_key_value_heads=2, head_dim=16,
               vocab_size=128, intermediate_size=64, num_local_experts=4,
               num_experts_per_tok=2, rope_theta=10000.0, rms_norm_eps=1e-5)


def _moe_tp_run(rank, world, port, q, tp, residency):
    if world > 1:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                          MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          LOCAL_RANK=str(rank))
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from dnet_amd.models import ModelConfig
    from dnet_amd.parallel.ring import RingExecutor
    cfg = ModelConfig.from_hf(MOE_CFG)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=1, mb_size=2,
                      smax=32, seed=11, use_graphs=False, tp=tp,
                      residency=residency)
    g = torch.Generator().manual_seed(42)
    toks = torch.randint(0, cfg.vocab_size, (1, 2, 6), generator=g)
    first = ex.prefill(toks)
    gen = ex.decode_rounds(4)
    out = torch.cat([first.unsqueeze(-1), gen], dim=-1)
    if rank == 0 and q is not None:
        q.put(out)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return out


@pytest.mark.timeout(480)
@retry_flaky()
def test_moe_tp2_offload_matches_fit():
    """Regression (advisor r1, medium): TP + offload on a MoE model. The
    offload path restores the FULL expert bank per weight-cache slot, so
    each TP rank's grouped-kernel route weights must zero non-owned
    experts — the cached full-bank stack must not make every rank compute
    ALL experts (the stage all-reduce would double the routed output)."""
    single = _moe_tp_run(0, 1, 0, None, 1, 0)
    ctx = mp.get_context("spawn")
    port = _free_port()
    outs = {}
    for residency in (0, 2):     # tp2 fit AND tp2+offload
        q = ctx.Queue()
        procs = [ctx.Process(target=_moe_tp_run,
                             args=(r, 2, port + residency, q, 2, residency))
                 for r in range(2)]
        for p in procs:
            p.start()
        outs[residency] = q.get(timeout=150)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        # vs single rank: EP reorders partial sums (bf16) and can flip
        # near-tie argmaxes after a few steps on a tiny random model; a
        # real sharding bug diverges at the first token
        assert torch.equal(outs[residency][..., :3], single[..., :3]), \
            f"moe tp2 residency={residency} != single:\n{outs}\n{single}"
    # offload MUST be token-exact vs fit at the same tp: the old
    # unconditional stack cache made every rank compute ALL experts from
    # the restored full bank (all-reduce doubled the routed output)
    assert torch.equal(outs[0], outs[2]), \
        f"moe tp2 offload != fit:\n{outs[2]}\n{outs[0]}"


def _cp2_win_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from dnet_amd.models import ModelConfig
    from dnet_amd.models.base import RingModel
    from dnet_amd.parallel.ring import RingExecutor
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # the whole point: CP prefill must never gather the full KV
    def _no_gather(self, t):
        raise AssertionError("CP prefill gathered the full KV")
    RingModel._cp_gather = _no_gather
    cfg = ModelConfig.from_hf(GPTOSS_CFG)   # windowed model (gpt-oss)
    ex = RingExecutor(cfg, rank, world, "cpu", mb_count=MB_COUNT,
                      mb_size=MB_SIZE, smax=64, seed=5, use_graphs=False,
                      cp=2)
    toks = _tokens(cfg)
    first = ex.prefill(toks, chunk=3)       # chunked continuation prefill
    gen = ex.decode_rounds(NGEN)
    if rank == 0:
        q.put(torch.cat([first.unsqueeze(-1), gen], dim=-1))
    dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_cp2_sliding_window_matches_single():
    """CP with a sliding-window model (gpt-oss) —
    windowed decode partials + gather-free chunked CP prefill must
    reproduce the single-rank tokens; the full KV is asserted to never
    be gathered."""
    single = _gptoss_run(0, 1, 0, None, 1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cp2_win_rank_main, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=200)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # the partials merge reorders fp sums (shard-then-combine), which can
    # flip near-tie argmaxes after a few steps on a tiny random model —
    # same tolerance rationale as the gpt-oss EP test above; a real
    # masking/offset bug diverges at the FIRST token
    assert torch.equal(out[..., :3], single[..., :3]), \
        f"cp2+window != single:\n{out}\n{single}"


def test_cp_windowed_partials_math():
    """Direct math check (no dist): windowed decode partials computed per
    shard and merged == full windowed attention, with the window binding
    ACROSS the shard boundary (and one shard fully outside the window)."""
    from dnet_amd.ops import reference as ref
    from dnet_amd.parallel.context import (_partials_windowed,
                                           local_lengths)
    import dnet_amd.ops as ops
    g = torch.Generator().manual_seed(3)
    B, Hq, Hkv, D, cap, world = 2, 4, 2, 32, 24, 3
    S = cap * world
    kc = torch.randn(B, Hkv, S, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, S, D, generator=g).to(torch.bfloat16)
    qt = torch.randn(B, Hq, D, generator=g).to(torch.bfloat16)
    pos = torch.tensor([61, 30], dtype=torch.int32)   # query INDEX per seq
    window = 20                                        # binds mid-shard
    # ref takes LENGTHS (pos+1); the runtime helpers take the index
    full = ref.attn_decode(qt, kc, vc, pos + 1, D ** -0.5, window=window)
    parts = []
    for r in range(world):
        ln = local_lengths(pos + 1, cap, r)
        parts.append(_partials_windowed(
            qt, kc[:, :, r * cap:(r + 1) * cap],
            vc[:, :, r * cap:(r + 1) * cap], ln, D ** -0.5, r * cap,
            pos.long(), window))
    merged = ops.attn_combine(torch.cat(parts, dim=2))
    assert torch.allclose(merged.float(), full.float(), atol=2e-2,
                          rtol=2e-2), (merged - full).abs().max()

    # prefill partials: chunk of queries, window + causal, merged shards
    from dnet_amd.parallel.context import cp_prefill_attention
    T, q0 = 9, 40
    qp = torch.randn(B, Hq, T, D, generator=g).to(torch.bfloat16)
    from dnet_amd.models.base import _chunked_causal_attention
    want = _chunked_causal_attention(qp, kc[:, :, :q0 + T],
                                     vc[:, :, :q0 + T], D ** -0.5, q0,
                                     window)
    outs = []
    for r in range(world):
        outs.append(cp_prefill_attention(
            qp, kc[:, :, r * cap:(r + 1) * cap].contiguous(),
            vc[:, :, r * cap:(r + 1) * cap].contiguous(), q0 + T, q0,
            D ** -0.5, cap, r, window=window))
    # world=1 per call (no dist): merge manually via the partial identity
    # is already exercised above; here each rank's call degenerates to
    # its shard only, so instead run the single-rank full-cache case
    got = cp_prefill_attention(qp, kc[:, :, :q0 + T].contiguous(),
                               vc[:, :, :q0 + T].contiguous(), q0 + T, q0,
                               D ** -0.5, q0 + T, 0, window=window)
    assert torch.allclose(got.float(), want.float(), atol=2e-2, rtol=2e-2)


def _linkmx_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from dnet_amd.parallel.profiler import measure_link_matrix
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = measure_link_matrix(rank, world, torch.device("cpu"),
                            size=4096, reps=3)
    q.put((rank, m))
    dist.destroy_process_group()


@pytest.mark.timeout(360)
@retry_flaky()
def test_link_matrix_all_pairs():
    """All-pairs fabric probe: every ordered pair measured, full matrix
    identical on every rank (this is what /health surfaces for xGMI-aware
    ring ordering)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    world = 3
    procs = [ctx.Process(target=_linkmx_rank_main, args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, m = q.get(timeout=150)
        res[r] = m
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    keys = {f"{i}-{j}" for i in range(world) for j in range(world) if i != j}
    assert set(res[0]) == keys
    assert set(res[1]) == keys == set(res[2])
    for k in keys:
        assert res[0][k]["latency_ms"] > 0
        assert res[0][k] == res[1][k] == res[2][k]

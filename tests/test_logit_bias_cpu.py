"""logit_bias without a GPU: the CPU reference of the sampler contract, the
torch path of RowSampler, the request model, and the shard runtime (slot
scheduler, serial path, two-rank gloo ring) on the tiny random model.
"""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import sample_reference as sr
import dnet_amd.ops as ops
from conftest import retry_flaky
from dnet_amd.core.sampler import DecodingConfig, RowSampler, Sampler


# ---------------------------------------------------------------- reference

def _bias_table(logits, V, B, seed):
    g = torch.Generator().manual_seed(seed)
    order = logits.float().argsort(dim=-1, descending=True)
    table = torch.zeros(B, V)
    for b in range(B):
        ids = order[b, :4].tolist() + order[b, -2:].tolist() \
            + torch.randint(0, V, (18,), generator=g).tolist()
        vals = [-100.0, -3.5, 2.25, -0.75, 100.0 if b % 4 == 0 else 6.0,
                1.5] + (torch.rand(18, generator=g) * 8 - 4).tolist()
        for i, v in zip(ids, vals):
            table[b, i] = v
    return table


@pytest.mark.parametrize("V", [1000, 4099])
def test_reference_with_bias_matches_fp64(V):
    """reference.sample_rows with a bias table against the fp64 reference
    on l' = fl32(l + bias), rows with the flag off against the raw logits."""
    logits, params, _ = sr.case(V)
    table = _bias_table(logits, V, sr.B, 4321 + V)
    on = torch.ones(sr.B, dtype=torch.bool)
    on[5::6] = False
    eff = torch.where(on[:, None], table, torch.zeros_like(table))
    table[~on] = float("nan")              # never read
    lb = (logits.float().numpy() + eff.numpy()).astype(np.float32)
    refs = [sr.row_reference(lb[b], *params[b]) for b in range(sr.B)]
    eps = sr.derive_eps(V)
    temp, top_k, top_p, min_p = sr.param_tensors(params)
    for u in sr.uniforms(V)[:4]:
        toks = ops.sample_rows(logits, temp, top_k, top_p, min_p,
                               torch.as_tensor(u), bias=table, bias_on=on)
        sr.check_tokens(toks.numpy(), refs, u, eps, cap=1)
    # without flags every row is biased
    refs = [sr.row_reference(
        (logits[b].float().numpy() + eff[b].numpy()).astype(np.float32),
        *params[b]) for b in range(sr.B)]
    u = sr.uniforms(V)[5]
    toks = ops.sample_rows(logits, temp, top_k, top_p, min_p,
                           torch.as_tensor(u), bias=eff)
    sr.check_tokens(toks.numpy(), refs, u, eps, cap=1)


def test_reference_bias_acts_before_penalties():
    """Token 1 is in the prompt: 32 / 1.3 = 24.6 with the bias first,
    2 / 1.3 + 30 = 31.5 the other way round; token 2 is 28 either way."""
    V = 16
    logits = torch.zeros(1, V)
    logits[0, 1], logits[0, 2] = 2.0, 1.5
    bias = torch.zeros(1, V)
    bias[0, 1], bias[0, 2] = 30.0, 26.5
    seen = torch.zeros(1, V, dtype=torch.int32)
    seen[0, 1] = sr.PROMPT_BIT
    z = torch.zeros(1)
    tok = ops.sample_rows(logits, z, torch.zeros(1, dtype=torch.int64),
                          torch.ones(1), z, z, rep=torch.full((1,), 1.3),
                          seen=seen, bias=bias)
    assert tok.tolist() == [2] and int(seen[0, 2]) == 1
    lf = ops.apply_penalties(ops.apply_logit_bias(logits, bias), seen,
                             1.3, 0.0, 0.0)
    assert int(lf.argmax()) == 1            # counted token 2 once: 28 - 0


# --------------------------------------------------------------- RowSampler

V_RS = 257


def _rs_logits():
    return torch.randn(3, V_RS, generator=torch.Generator().manual_seed(3))


def test_row_sampler_ban_force_and_neighbour():
    logits = _rs_logits()
    top = int(logits[0].argmax())
    rs = RowSampler(3, vocab=V_RS)
    plain = RowSampler(3, vocab=V_RS)
    rs.set_row(0, DecodingConfig(temperature=1.0,
                                 logit_bias={top: -100.0, V_RS + 3: 100.0}),
               seed=1)
    rs.set_row(1, DecodingConfig(temperature=1.0, logit_bias={41: 100.0}),
               seed=2)
    rs.set_row(2, DecodingConfig(temperature=1.0), seed=3)
    plain.set_row(2, DecodingConfig(temperature=1.0), seed=3)
    assert plain.bias is None
    assert rs.bias.shape == (3, V_RS) and rs.bias_on.tolist() == [True, True,
                                                                  False]
    # ids >= V are dropped, never written
    assert int((rs.bias[0] != 0).sum()) == 1
    drawn = set()
    for _ in range(200):
        a, p = rs.sample(logits), plain.sample(logits)
        assert int(a[0]) != top                 # banned: never drawn
        assert int(a[1]) == 41                  # forced: always drawn
        assert int(a[2]) == int(p[2])           # the neighbour is untouched
        drawn.add(int(a[0]))
    assert len(drawn) > 20
    # a freed and reused row keeps no residue
    rs.clear_row(0)
    assert not bool(rs.bias_on[0])
    rs.set_row(0, DecodingConfig())
    assert int(rs.sample(logits)[0]) == top
    rs.set_row(0, DecodingConfig(logit_bias={7: 100.0}))
    assert int((rs.bias[0] != 0).sum()) == 1    # the old entry is gone
    assert int(rs.sample(logits)[0]) == 7       # greedy and biased
    rs.set_row(0, DecodingConfig())             # set_row alone clears too
    assert int(rs.sample(logits)[0]) == top


def test_sampler_takes_a_bias_row():
    logits = _rs_logits()[:1]
    top = int(logits[0].argmax())
    bias = torch.zeros(1, V_RS)
    bias[0, top] = -100.0
    tok, lp, tops = Sampler(DecodingConfig(logprobs=True, top_logprobs=2)
                            ).sample(logits, None, bias)
    assert int(tok[0]) != top
    # logprobs stay on the raw logits: the banned token still leads them
    assert list(tops[0])[0] == top
    want = torch.log_softmax(logits.double(), -1)[0, int(tok[0])]
    assert abs(float(lp[0]) - float(want)) < 1e-5
    assert DecodingConfig(logit_bias={1: 2.0}).has_bias
    assert not DecodingConfig(logit_bias={}).has_bias
    assert not DecodingConfig().has_bias


# ---------------------------------------------------------------------- API

def test_chat_request_logit_bias():
    from pydantic import ValidationError
    from dnet_amd.api.inference import decoding_params
    from dnet_amd.api.models import ChatRequestModel

    base = dict(model="m", messages=[{"role": "user", "content": "x"}])
    assert "logit_bias" not in decoding_params(ChatRequestModel(**base))
    assert "logit_bias" not in decoding_params(
        ChatRequestModel(**base, logit_bias={}))
    r = ChatRequestModel(**base, logit_bias={"17": -100, "4": 2.5,
                                             "0": 100.0})
    assert decoding_params(r)["logit_bias"] == [[17, -100.0], [4, 2.5],
                                                [0, 100.0]]
    for bad in ({"abc": 1.0}, {"-1": 1.0}, {"5": 100.5}, {"5": -100.5},
                {"1.5": 1.0}, {str(i): 0.5 for i in range(301)},
                {str(2 ** 31): 1.0}, {str(2 ** 63): 1.0}, {str(2 ** 64): 1.0},
                {"9" * 400: 1.0}):
        with pytest.raises(ValidationError):
            ChatRequestModel(**base, logit_bias=bad)
    ChatRequestModel(**base, logit_bias={str(2 ** 31 - 1): 1.0})
    ChatRequestModel(**base, logit_bias={str(i): 0.5 for i in range(300)})


def test_api_rejects_bad_logit_bias_with_422():
    from fastapi.testclient import TestClient
    from dnet_amd.api.cluster import ClusterManager
    from dnet_amd.api.server import ApiState, build_api_app
    from dnet_amd.config import get_settings

    class NoDevices:
        async def async_get_properties(self):
            return {}

        async def async_start(self):
            pass

    client = TestClient(build_api_app(
        ApiState(ClusterManager(NoDevices()), get_settings())))
    # a well-formed request gets past validation (no model loaded: 400)
    assert client.post("/v1/chat/completions", json=dict(
        model="tiny-random", messages=[{"role": "user", "content": "x"}],
        logit_bias={"5": -100})).status_code == 400
    body = dict(model="tiny-random",
                messages=[{"role": "user", "content": "x"}])
    for bad in ({"abc": 1.0}, {"-1": 1.0}, {"5": 100.5},
                {str(i): 0.5 for i in range(301)}, {str(2 ** 63): 1.0},
                {str(2 ** 64): 1.0}):
        r = client.post("/v1/chat/completions",
                        json=dict(body, logit_bias=bad))
        assert r.status_code == 422, (bad, r.status_code)


def test_wire_frame_carries_pairs():
    import msgpack
    from dnet_amd.api.inference import decoding_params
    from dnet_amd.api.models import ChatRequestModel
    r = ChatRequestModel(model="m", messages=[{"role": "user",
                                               "content": "x"}],
                         logit_bias={"9": 1.25})
    frame = {"t": "infer", "params": decoding_params(r)}
    back = msgpack.unpackb(msgpack.packb(frame))
    assert back["params"]["logit_bias"] == [[9, 1.25]]


# ------------------------------------------------------------------ runtime

class _Cap:
    def __init__(self):
        self.emitted: dict = {}
        self.finished = 0

    def send(self, frame):
        self.emitted.setdefault(frame["nonce"], []).append(frame["token_id"])
        self.finished += bool(frame.get("finished"))

    def close(self):
        pass


def _load(max_batch):
    from dnet_amd.core.types import ShardLoadModelRequest
    from dnet_amd.shard.runtime import ShardRuntime
    rt = ShardRuntime("probe")
    rt._load(ShardLoadModelRequest(
        model_path="tiny", model_name="tiny", total_layers=4,
        layers=[0, 1, 2, 3], rank=0, world_size=1, max_batch=max_batch,
        max_seq=64))
    rt._callback = _Cap()
    return rt


PROMPT = torch.arange(1, 9, dtype=torch.int32)
X = 201
N_TOK = 6


def _slots(requests, max_batch=3):
    rt = _load(max_batch)
    for name, params in requests:
        rt.infer_q.put({"nonce": name, "tokens": PROMPT.numpy().tobytes(),
                        "prompt_len": 8, "max_tokens": N_TOK, "stop_ids": [],
                        "params": params})
    for _ in range(40):
        rt._slots_tick()
        if (all(s is None for s in rt.slots) and rt._pending is None
                and rt.infer_q.empty()):
            break
    out = rt._callback.emitted
    rt._unload()
    return out


def test_slot_scheduler_honours_logit_bias():
    alone = _slots([("plain", {})])["plain"]
    assert len(alone) == N_TOK and X not in alone
    got = _slots([("force", {"logit_bias": [[X, 100.0]]}),
                  ("plain", {}),
                  ("ban", {"logit_bias": [[alone[0], -100.0],
                                          [10 ** 6, 100.0]]})])
    assert got["force"] == [X] * N_TOK          # at every step
    assert got["ban"][0] != alone[0]
    assert alone[0] not in got["ban"]
    assert got["plain"] == alone                # the neighbour is untouched

    # the serial path gives the same tokens
    rt = _load(1)
    for name in ("force", "ban"):
        params = {"force": {"logit_bias": [[X, 100.0]]},
                  "ban": {"logit_bias": [[alone[0], -100.0]]}}[name]
        rt._execute_infer(name, PROMPT.long().view(1, 1, -1), N_TOK, [],
                          params)
    assert rt.executor.bias_row is not None
    rt._execute_infer("plain", PROMPT.long().view(1, 1, -1), N_TOK, [], {})
    assert rt.executor.bias_row is None
    ser = rt._callback.emitted
    rt._unload()
    assert ser["force"] == got["force"] and ser["ban"] == got["ban"]
    assert ser["plain"] == alone


# ids past the vocabulary, one of them past int64: dropped on rank 0 before
# anything is broadcast, so the ring stays in step
PP2_REQS = [("a", {"logit_bias": [[X, 3.5], [17, -100.0], [5, 0.1 + 0.2],
                                  [2 ** 63, 100.0], [10 ** 6, 100.0]]}),
            ("b", {})]


def _pp2_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    from dnet_amd.core.types import ShardLoadModelRequest
    from dnet_amd.shard import runtime as R
    layer_rounds = [[0, 1]] if rank == 0 else [[2, 3]]
    rt = R.ShardRuntime(f"s{rank}")
    rt._load(ShardLoadModelRequest(
        model_path="tiny", model_name="tiny", total_layers=4,
        layers=layer_rounds[0], layer_rounds=layer_rounds, rank=rank,
        world_size=2, master_addr="127.0.0.1", master_port=port + 1,
        max_batch=2, max_seq=64))
    cap = _Cap()
    if rank == 1:
        rt._callback = cap
    if rank == 0:
        for name, params in PP2_REQS:
            rt.infer_q.put({"nonce": name,
                            "tokens": PROMPT.numpy().tobytes(),
                            "prompt_len": 8, "max_tokens": N_TOK,
                            "stop_ids": [], "params": params})
        while (any(s is not None for s in rt.slots)
               or not rt.infer_q.empty()):
            rt._slots_tick()
        q.put(("rank0", None))
    else:
        while cap.finished < 2:
            cmd = rt._recv_cmd()
            if cmd[0] == R.CMD_SLOT_ADMIT:
                rt._slot_admit_follower(cmd)
            elif cmd[0] == R.CMD_SLOT_STEP:
                rt._slot_step_exec()
        # the last stage received exactly the bias rank 0 got
        bias = rt._row_sampler.bias
        q.put(("rank1", (cap.emitted,
                         None if bias is None else bias[0].tolist())))
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


@pytest.mark.timeout(480)
@retry_flaky()
def test_slots_pp2_with_bias_matches_single():
    """Two-rank gloo ring, slot scheduler: a biased request and a plain one
    are token-exact against a single rank; the entries reach the sampling
    rank bit for bit."""
    single = _slots(PP2_REQS, max_batch=2)
    plain = _slots([("a", {}), ("b", {})], max_batch=2)
    assert single["a"] != plain["a"] and single["b"] == plain["b"]

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_pp2_rank_main, args=(r, 2, port, q))
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
    emitted, row = results["rank1"]
    assert emitted["a"] == single["a"] and emitted["b"] == single["b"]
    want = torch.zeros(256)
    for i, v in PP2_REQS[0][1]["logit_bias"]:
        if i < 256:
            want[i] = v
    assert row == want.tolist()

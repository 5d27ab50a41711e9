"""Sampler semantics on the CPU: the torch reference of ops.sample_rows
against the fp64 reference, penalties through RowSampler / Sampler, the
request fields, and penalties end to end through real API + shard
processes (single rank and a two-rank gloo ring).
"""
import contextlib
import os
import signal
import socket
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

import sample_reference as sr
import dnet_amd.ops as ops
from dnet_amd.core.sampler import DecodingConfig, RowSampler, Sampler

REPO = Path(__file__).resolve().parent.parent


def _run(logits, params, u, **pen):
    temp, top_k, top_p, min_p = sr.param_tensors(params)
    return ops.sample_rows(logits, temp, top_k, top_p, min_p,
                           torch.as_tensor(u, dtype=torch.float32),
                           **pen).numpy()


# ------------------------------------------------- reference vs fp64

@pytest.mark.parametrize("V", [1000, 4099])
def test_reference_interval_and_keep_set(V):
    logits, params, refs = sr.case(V)
    eps = sr.derive_eps(V)
    for u in sr.uniforms(V):
        toks = _run(logits, params, u)
        assert ((toks >= 0) & (toks < V)).all()
        sr.check_tokens(toks, refs, u, eps, cap=1)


@pytest.mark.parametrize("V", sr.SHAPES)
def test_fp64_reference_stays_inside_skip_cap(V):
    """The seeds of the shared cases leave at most one ambiguous row in 16
    at the derived eps, for every shape the GPU test uses."""
    _, _, refs = sr.case(V)
    eps = sr.derive_eps(V)
    assert eps <= 2.0 ** -16
    assert sum("margin" in r and r["margin"] <= eps for r in refs) <= 1


REP, PRES, FREQ = 1.3, 0.7, 0.4


def _penalty_case(V, B=8):
    g = torch.Generator().manual_seed(77 + V)
    logits = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16)
    seen = torch.zeros(B, V, dtype=torch.int32)
    order = logits.float().argsort(dim=-1, descending=True)
    for b in range(B):
        hot = torch.cat([order[b, :6], order[b, -3:],
                         torch.randint(0, V, (40,), generator=g)])
        for n, t in enumerate(hot.tolist()):
            kind = n % 3
            if kind == 0:
                seen[b, t] = sr.PROMPT_BIT
            elif kind == 1:
                seen[b, t] = 1 + (n // 3) % 3
            else:
                seen[b, t] = sr.PROMPT_BIT | (1 + (n // 3) % 2)
    return logits, seen


def _pen(B):
    f = lambda v: torch.full((B,), v, dtype=torch.float32)
    return dict(rep=f(REP), pres=f(PRES), freq=f(FREQ))


@pytest.mark.parametrize("V", [1000, 4099])
def test_reference_penalties(V):
    B = 8
    logits, seen = _penalty_case(V, B)
    # greedy rows against the fp64 argmax
    work = seen.clone()
    toks = _run(logits, [(0.0, 0, 1.0, 0.0)] * B, np.zeros(B, np.float32),
                seen=work, **_pen(B))
    checked = moved = 0
    for b in range(B):
        l64 = sr.penalise(logits[b].float().numpy(), seen[b].numpy(), REP,
                          PRES, FREQ, dtype=np.float64)
        top2 = np.sort(l64)[-2:]
        if top2[1] - top2[0] > 3 * 2.0 ** -24 * 32:
            assert toks[b] == int(np.argmax(l64)), b
            checked += 1
        moved += int(np.argmax(l64)) != int(logits[b].float().argmax())
    assert checked >= B - 1 and moved >= 1
    expect = seen.clone()
    expect[torch.arange(B), torch.as_tensor(toks)] += 1
    assert torch.equal(work, expect)
    # the torch penalties are the contract's f32 arithmetic, bit for bit
    got = ops.apply_penalties(logits.float(), seen, REP, PRES, FREQ)
    for b in range(B):
        want = sr.penalise(logits[b].float().numpy(), seen[b].numpy(), REP,
                           PRES, FREQ)
        assert np.array_equal(got[b].numpy(), want)
    # sampled rows with penalties through the interval check
    params = [(0.7, 50, 0.9, 0.0)] * B
    refs = [sr.row_reference(
        sr.penalise(logits[b].float().numpy(), seen[b].numpy(), REP, PRES,
                    FREQ), *params[b]) for b in range(B)]
    for u in sr.uniforms(V, B)[:4]:
        toks = _run(logits, params, u, seen=seen.clone(), **_pen(B))
        sr.check_tokens(toks, refs, u, sr.derive_eps(V), cap=0)


def test_reference_degenerate_rows():
    V = 1000
    inf, nan = float("inf"), float("nan")
    rows = torch.randn(5, V, generator=torch.Generator().manual_seed(5))
    rows[0] = nan
    rows[1, 345] = inf
    rows[1, 700] = inf
    rows[2] = -inf
    rows[2, 999] = -3.0
    rows[3] = -inf
    rows[3, 77] = nan
    rows[4, ::2] = nan
    for temp in (0.0, 0.8):
        toks = _run(rows, [(temp, 50, 0.9, 0.05)] * 5, [0.3] * 5)
        assert toks[:4].tolist() == [0, 345, 999, 77] and toks[4] % 2 == 1


def test_reference_tiny_vocab():
    for V in (1, 5, 63, 129):
        logits = (torch.randn(4, V, generator=torch.Generator()
                              .manual_seed(V)) * 3).to(torch.bfloat16)
        params = [(1.0, 0, 1.0, 0.0), (0.0, 0, 1.0, 0.0),
                  (0.7, 3, 0.9, 0.0), (1.3, 0, 0.5, 0.05)]
        refs = [sr.row_reference(logits[b].float().numpy(), *params[b])
                for b in range(4)]
        for uu in (0.0, 0.37, sr.U_MAX):
            u = np.full(4, uu, np.float32)
            sr.check_tokens(_run(logits, params, u), refs, u,
                            sr.derive_eps(V), cap=0)


# ------------------------------------------------- RowSampler / Sampler

def test_row_sampler_repetition_penalty_never_repeats():
    V, B, T = 64, 2, 20
    logits = torch.randn(B, V, generator=torch.Generator().manual_seed(3)) + 4
    prompt = logits[0].argsort(descending=True)[:5].tolist()
    rs = RowSampler(B, vocab=V)
    rs.set_row(0, DecodingConfig(repetition_penalty=1e4))
    rs.set_row(1, DecodingConfig())              # neutral neighbour
    rs.note_prompt(0, prompt)
    out = [rs.sample(logits).tolist() for _ in range(T)]
    row0 = [o[0] for o in out]
    assert len(set(row0)) == T and not set(row0) & set(prompt)
    assert len({o[1] for o in out}) == 1          # greedy, unpenalised
    # the first token of a slot comes from Sampler: note_token counts it
    rs.set_row(0, DecodingConfig(repetition_penalty=1e4))
    first = int(logits[0].argmax())
    rs.note_token(0, first)
    assert int(rs.sample(logits)[0]) != first
    rs.clear_row(0)
    assert int(rs.sample(logits)[0]) == first


def test_sampler_with_table_never_repeats():
    V, T = 64, 20
    logits = torch.randn(1, V, generator=torch.Generator().manual_seed(4)) + 4
    seen = torch.zeros(1, V, dtype=torch.int32)
    prompt = logits[0].argsort(descending=True)[:5]
    seen[0, prompt] = sr.PROMPT_BIT
    s = Sampler(DecodingConfig(repetition_penalty=1e4))
    toks = [int(s.sample(logits, seen)[0][0]) for _ in range(T)]
    assert len(set(toks)) == T and not set(toks) & set(prompt.tolist())
    # without a table the config's penalty cannot act
    assert int(s.sample(logits)[0][0]) == int(logits.argmax())


def test_neutral_config_allocates_no_table():
    rs = RowSampler(4, vocab=1000)
    rs.set_row(0, DecodingConfig(temperature=0.7, top_p=0.9, top_k=50))
    rs.note_prompt(0, [1, 2, 3])
    rs.note_token(0, 5)
    rs.sample(torch.randn(4, 1000))
    assert rs.seen is None
    assert not DecodingConfig().has_penalty
    rs.set_row(1, DecodingConfig(frequency_penalty=0.5))
    assert rs.seen is not None and rs.seen.shape == (4, 1000)

    from dnet_amd.models import ModelConfig, PRESETS
    from dnet_amd.parallel.ring import RingExecutor
    ex = RingExecutor(ModelConfig.from_hf(dict(PRESETS["tiny"])), 0, 1, "cpu",
                      mb_count=1, mb_size=1, smax=32, seed=0)
    assert ex.seen is None
    ex.set_decoding(DecodingConfig(temperature=0.5))
    assert ex.seen is None
    ex.set_decoding(DecodingConfig(presence_penalty=1.0))
    assert ex.seen is not None and len(ex.seen) == 1
    ex.set_decoding(DecodingConfig())
    assert ex.seen is None


# ------------------------------------------------- request plumbing

def test_chat_request_fields_and_bounds():
    from pydantic import ValidationError
    from dnet_amd.api.inference import decoding_params
    from dnet_amd.api.models import ChatRequestModel
    from dnet_amd.core.types import DecodingParams

    base = dict(model="m", messages=[{"role": "user", "content": "x"}])
    r = ChatRequestModel(**base)
    assert (r.repetition_penalty, r.presence_penalty,
            r.frequency_penalty) == (1.0, 0.0, 0.0)
    r = ChatRequestModel(**base, repetition_penalty=1.2,
                         presence_penalty=-2.0, frequency_penalty=2.0)
    p = decoding_params(r)
    assert (p["repetition_penalty"], p["presence_penalty"],
            p["frequency_penalty"]) == (1.2, -2.0, 2.0)
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                dict(presence_penalty=2.1), dict(presence_penalty=-2.1),
                dict(frequency_penalty=2.5), dict(frequency_penalty=-3.0)):
        with pytest.raises(ValidationError):
            ChatRequestModel(**base, **bad)
    d = DecodingParams(presence_penalty=0.5, frequency_penalty=0.25)
    assert d.presence_penalty == 0.5 and d.frequency_penalty == 0.25


def test_runtime_paths_apply_frequency_penalty():
    """In process, single rank: the serial path (max_batch 1) and the slot
    path give the same penalised tokens, which differ from the plain ones
    and never use a token more often than the penalty allows."""
    from dnet_amd.core.types import ShardLoadModelRequest
    from dnet_amd.shard.runtime import ShardRuntime

    emitted: dict[str, list] = {}

    class Cap:
        def send(self, frame):
            emitted.setdefault(frame["nonce"], []).append(frame["token_id"])

        def close(self):
            pass

    def load(max_batch):
        rt = ShardRuntime("probe")
        rt._load(ShardLoadModelRequest(
            model_path="tiny", model_name="tiny", total_layers=4,
            layers=[0, 1, 2, 3], rank=0, world_size=1,
            max_batch=max_batch, max_seq=64))
        rt._callback = Cap()
        return rt

    prompt_t = torch.arange(1, 9, dtype=torch.int32)
    prompt = prompt_t.numpy().tobytes()
    pen = {"frequency_penalty": 2.0, "repetition_penalty": 1.5}
    rt1 = load(1)
    for name, p in (("s-plain", {}), ("s-pen", pen)):
        rt1._execute_infer(name, prompt_t.long().view(1, 1, -1), 12, [], p)
    assert rt1.executor.seen is not None
    rt1._execute_infer("s-plain2", prompt_t.long().view(1, 1, -1), 12, [], {})
    assert rt1.executor.seen is None
    rt1._unload()
    assert emitted["s-plain"] == emitted["s-plain2"]
    assert emitted["s-pen"] != emitted["s-plain"]

    rt = load(2)
    rt.infer_q.put({"nonce": "b-plain", "tokens": prompt, "prompt_len": 8,
                    "max_tokens": 12, "stop_ids": [], "params": {}})
    rt.infer_q.put({"nonce": "b-pen", "tokens": prompt, "prompt_len": 8,
                    "max_tokens": 12, "stop_ids": [], "params": pen})
    for _ in range(40):
        rt._slots_tick()
        if all(s is None for s in rt.slots) and all(
                len(emitted.get(k, ())) == 12 for k in ("b-plain", "b-pen")):
            break
    rt._unload()
    assert emitted["b-plain"] == emitted["s-plain"]
    assert emitted["b-pen"] == emitted["s-pen"]


def test_chunked_prefill_keeps_penalised_history_clean(monkeypatch):
    """A penalised long prompt admitted in chunks while another slot
    decodes: the decode steps in between sample the parked row's dummy
    logits, and none of that may count as generated. Its tokens equal
    those of the same request run alone."""
    from dnet_amd.core.types import ShardLoadModelRequest
    from dnet_amd.shard.runtime import ShardRuntime

    def load(cap_dict):
        rt = ShardRuntime("probe")
        rt._load(ShardLoadModelRequest(
            model_path="tiny", model_name="tiny", total_layers=4,
            layers=[0, 1, 2, 3], rank=0, world_size=1, max_batch=2,
            max_seq=64))

        class Cap:
            def send(self, frame):
                cap_dict.setdefault(frame["nonce"], []).append(
                    frame["token_id"])

            def close(self):
                pass

        rt._callback = Cap()
        return rt

    def run_all(rt):
        for _ in range(60):
            rt._slots_tick()
            if (all(s is None for s in rt.slots) and rt._pending is None
                    and rt.infer_q.empty()):
                break

    short = torch.arange(1, 9, dtype=torch.int32).numpy().tobytes()
    longp = torch.arange(1, 13, dtype=torch.int32).numpy().tobytes()
    # strong enough that one wrongly counted token changes the argmax
    pen = {"frequency_penalty": 2.0, "presence_penalty": 2.0,
           "repetition_penalty": 2.0}
    req_a = {"nonce": "A", "tokens": longp, "prompt_len": 12,
             "max_tokens": 12, "stop_ids": [], "params": pen}
    req_b = {"nonce": "B", "tokens": short, "prompt_len": 8,
             "max_tokens": 16, "stop_ids": [], "params": {}}

    monkeypatch.setenv("DNET_PREFILL_CHUNK", "4")
    solo: dict = {}
    rt = load(solo)
    rt.infer_q.put(dict(req_a))
    run_all(rt)
    rt._unload()

    mixed: dict = {}
    rt = load(mixed)
    rt.infer_q.put(dict(req_b))
    rt._slots_tick()            # B admitted and decoding
    rt._slots_tick()
    rt.infer_q.put(dict(req_a))
    seen_counts, active_checks = [], 0
    for _ in range(60):
        rt._slots_tick()
        st = next((s for s in rt.slots if s and s["nonce"] == "A"), None)
        if st is not None:
            si = rt.slots.index(st)
            counted = int((rt._row_sampler.seen[si] & sr.COUNT_MASK).sum())
            if st.get("state") == "prefill":
                seen_counts.append(counted)
            else:
                # only real tokens: what was emitted, plus the step in flight
                assert counted <= st["produced"] + 1, (counted, st["produced"])
                active_checks += 1
        if (all(s is None for s in rt.slots) and rt._pending is None
                and rt.infer_q.empty()):
            break
    rt._unload()
    # the hazard is real: the parked row was counted during its prefill
    assert seen_counts and max(seen_counts) >= 2 and active_checks >= 5
    assert len(solo["A"]) == 12 and mixed["A"] == solo["A"]


# ------------------------------------------------- end to end

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _wait_http(url, timeout=90):
    import httpx
    t0 = time.time()
    while time.time() - t0 < timeout:
        try:
            if httpx.get(url, timeout=2).status_code == 200:
                return True
        except httpx.HTTPError:
            pass
        time.sleep(0.5)
    return False


@contextlib.contextmanager
def _cluster(tmp, n_shards):
    http = [_free_port() for _ in range(n_shards)]
    wire = [_free_port() for _ in range(n_shards)]
    api_port, api_wire = _free_port(), _free_port()
    hostfile = tmp / f"hosts{n_shards}"
    hostfile.write_text("".join(
        f"shard{i} 127.0.0.1 {http[i]} {wire[i]} 0\n"
        for i in range(n_shards)))
    env = dict(os.environ)
    env["DNET_LOG_DIR"] = str(tmp / f"logs{n_shards}")
    env["DNET_TRANSPORT_MASTER_PORT"] = str(_free_port())
    # CPU shards on every machine: this is the gloo ring, and two shards
    # on one GPU cannot form an RCCL group
    env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = "-1"
    procs = []
    try:
        for i in range(n_shards):
            procs.append(subprocess.Popen(
                [sys.executable, "-m", "dnet_amd.cli.shard", "--name",
                 f"shard{i}", "--host", "127.0.0.1", "--http-port",
                 str(http[i]), "--wire-port", str(wire[i])],
                cwd=REPO, env=env))
        procs.append(subprocess.Popen(
            [sys.executable, "-m", "dnet_amd.cli.api", "--hostfile",
             str(hostfile), "--host", "127.0.0.1", "--port", str(api_port),
             "--wire-port", str(api_wire), "--callback-addr",
             f"127.0.0.1:{api_wire}"],
            cwd=REPO, env=env))
        for i in range(n_shards):
            assert _wait_http(f"http://127.0.0.1:{http[i]}/health")
        assert _wait_http(f"http://127.0.0.1:{api_port}/health")
        yield f"http://127.0.0.1:{api_port}"
    finally:
        for p in procs:
            p.send_signal(signal.SIGTERM)
        for p in procs:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                p.kill()


def _chat_pair(api, assignments):
    """Load tiny-random on the given split and return the greedy text
    without and with a frequency penalty."""
    import httpx
    with httpx.Client(timeout=180) as c:
        r = c.post(f"{api}/v1/prepare_topology_manual", json={
            "model": "tiny-random", "assignments": assignments})
        assert r.status_code == 200, r.text
        r = c.post(f"{api}/v1/load_model", json={"model": "tiny-random"})
        assert r.status_code == 200, r.text
        out = []
        for extra in ({}, {"frequency_penalty": 2.0}):
            r = c.post(f"{api}/v1/chat/completions", json={
                "model": "tiny-random", "stream": False, "max_tokens": 16,
                "messages": [{"role": "user", "content": "hi there"}],
                **extra})
            assert r.status_code == 200, r.text
            out.append(r.json()["choices"][0]["message"]["content"])
        r = c.post(f"{api}/v1/chat/completions", json={
            "model": "tiny-random", "max_tokens": 4, "presence_penalty": 3.0,
            "messages": [{"role": "user", "content": "hi"}]})
        assert r.status_code == 422
        assert c.post(f"{api}/v1/unload_model").status_code == 200
    return out


@pytest.mark.timeout(400)
def test_frequency_penalty_end_to_end(tmp_path):
    """Slot-scheduled serving (the default load) through real processes:
    the penalty changes a greedy completion, and the two-rank gloo ring,
    which carries the fields in its slot-admit broadcast, produces what a
    single rank produces."""
    with _cluster(tmp_path, 1) as api:
        one = _chat_pair(api, [{"instance": "shard0",
                                "layers": [0, 1, 2, 3]}])
    assert one[0] != one[1]
    with _cluster(tmp_path, 2) as api:
        two = _chat_pair(api, [{"instance": "shard0", "layers": [0, 1]},
                               {"instance": "shard1", "layers": [2, 3]}])
    assert two == one

"""Prompt-prefix KV cache, everything that runs without a GPU: the host
index, ops.kv_copy_rows on CPU tensors (same case list as the GPU kernel
test), the serving scenarios on the in-process tiny runtime, and the API
plumbing."""
from __future__ import annotations

import asyncio

import numpy as np
import pytest
import torch

from dnet_amd import ops

import prefix_cache_cases as pcc
from prefix_cache_cases import D8, P48, Rt, cold_tokens, env, suffix_avoiding


# ------------------------------------------------------------ 1. host index

def test_prefix_cache_index():
    from dnet_amd.core.prefix_cache import PrefixCache

    pc = PrefixCache(2, min_prefix=4)
    a = list(range(10, 20))                       # 10 tokens
    assert pc.lookup(a) == (-1, 0) and pc.misses == 1
    assert pc.plan_insert(a) == (0, 0)
    # LCP capped at T - 1: one token must still be prefilled
    assert pc.lookup(a) == (0, 9)
    assert pc.lookup(a + [1, 2]) == (0, 10)
    assert pc.lookup(a[:6] + [99, 98]) == (0, 6)
    # below min_prefix: a miss
    assert pc.lookup(a[:3] + [99, 98, 97]) == (-1, 0)
    assert pc.lookup(a[:4]) == (-1, 0)            # capped to 3 < 4
    # a prefix of (or equal to) an existing entry inserts nothing
    assert pc.plan_insert(a[:7]) == (-1, 0)
    assert pc.plan_insert(a) == (-1, 0)
    assert pc.inserts == 1
    # an entry that is a prefix of the new tokens is extended in place
    assert pc.plan_insert(a + [1, 2, 3]) == (0, 10)
    assert pc.length(0) == 13 and pc.inserts == 2
    # unrelated tokens take the empty entry, then the LRU victim
    b = list(range(100, 110))
    assert pc.plan_insert(b) == (1, 0) and pc.evictions == 0
    assert pc.lookup(a + [5]) == (0, 10)          # entry 0 is now the MRU
    c = list(range(200, 212))
    assert pc.plan_insert(c) == (1, 0)            # b was least recent
    assert pc.evictions == 1
    assert pc.lookup(b + [1]) == (-1, 0)          # evicted prefix misses
    # a hit refreshes recency: c is hit, so a's entry is the next victim
    assert pc.lookup(c + [1]) == (1, 12)
    d = list(range(300, 310))
    assert pc.plan_insert(d) == (0, 0) and pc.evictions == 2
    assert pc.lookup(a + [5]) == (-1, 0)
    # ties go to the most recently used entry
    pc2 = PrefixCache(2, min_prefix=2)
    pc2.plan_insert([1, 2, 3, 4, 50])
    pc2.plan_insert([1, 2, 3, 4, 60])
    assert pc2.lookup([1, 2, 3, 4, 70, 71]) == (1, 4)
    pc2.lookup([1, 2, 3, 4, 50, 9])               # touches entry 0 (n = 5)
    assert pc2.lookup([1, 2, 3, 4, 70, 71]) == (0, 4)
    st = pc.stats()
    assert st["hits"] == 5 and st["misses"] == 5
    assert st["tokens_reused"] == 9 + 10 + 6 + 10 + 12
    assert st["inserts"] == 5 and st["evictions"] == 2
    assert st["entries"] == 2 and st["used"] == 2
    # a dropped entry is empty again and is the next one filled
    pc.drop(0)
    assert pc.length(0) == 0 and pc.lookup(d + [1]) == (-1, 0)
    assert pc.plan_insert(b) == (0, 0) and pc.evictions == 2


# ------------------------------------------------------------ 2. the op, CPU

_CASES = pcc.kernel_cases()


def test_kernel_case_list_is_pairwise_not_product():
    assert 24 <= len(_CASES) <= 60
    for ps in pcc.PLANE_SETS:
        for rr in pcc.ROW_RANGES:
            assert any(c["planes"] == ps and c["r0"] == rr[0]
                       and c["r1"] == (c["S"] if rr[1] == "S" else rr[1])
                       for c in _CASES), (ps, rr)
    assert sum(c["alias"] for c in _CASES) == len(pcc.PLANE_SETS)


@pytest.mark.parametrize("c", _CASES, ids=pcc.case_id)
def test_kv_copy_rows_cpu(c):
    if c["alias"]:
        src = dst = pcc.make_planes(c["planes"], c["L"], c["Bs"], c["H"],
                                    c["S"], seed=1)
    else:
        src = pcc.make_planes(c["planes"], c["L"], c["Bs"], c["H"], c["S"],
                              seed=1)
        dst = pcc.make_planes(c["planes"], c["L"], c["Bd"], c["H"], c["S"],
                              seed=2)
    want = [pcc.expected_bytes(d, c["dst_b"], s, c["src_b"], c["r0"],
                               c["r1"]) for d, s in zip(dst, src)]
    ops.kv_copy_rows(dst, c["dst_b"], src, c["src_b"], c["r0"], c["r1"])
    for d, w in zip(dst, want):
        assert np.array_equal(pcc.raw_bytes(d), w)


def test_kv_copy_rows_cpu_argument_checks():
    src = pcc.make_planes("int8_d64", 2, 3, 2, 50, seed=1)
    dst = pcc.make_planes("int8_d64", 2, 2, 2, 50, seed=2)
    before = [pcc.raw_bytes(d).copy() for d in dst]
    other = pcc.make_planes("int8_d64", 2, 2, 2, 64, seed=3)      # other S
    heads = pcc.make_planes("int8_d64", 2, 2, 1, 50, seed=3)      # other H
    bad = [
        (dst, 0, src, 0, 0, 51),          # r1 > S
        (dst, 0, src, 0, 9, 8),           # r0 > r1
        (dst, 0, src, 0, -1, 8),
        (dst, 2, src, 0, 0, 8),           # dst_b out of range
        (dst, 0, src, 3, 0, 8),           # src_b out of range
        (dst, -1, src, 0, 0, 8),
        (dst, 0, other, 0, 0, 8),         # geometry
        (dst, 0, heads, 0, 0, 8),
        (dst, 0, src[:2], 0, 0, 8),       # plane count
        (dst, 1, dst, 1, 0, 8),           # aliased, same batch index
    ]
    for a in bad:
        with pytest.raises((RuntimeError, ValueError)):
            ops.kv_copy_rows(*a)
    for d, b in zip(dst, before):
        assert np.array_equal(pcc.raw_bytes(d), b)


def test_cache_planes():
    from dnet_amd.models import ModelConfig, PRESETS
    from dnet_amd.models.base import KVCache
    cfg = ModelConfig.from_hf(dict(PRESETS["tiny"]))
    kv = KVCache(cfg, [0, 1], 2, 16, "cpu", kv_bits=8)
    assert [p.shape[-1] * p.element_size() for p in kv.planes()] == \
        [64, 64, 2, 2]
    kv = KVCache(cfg, [0, 1], 2, 16, "cpu")
    assert len(kv.planes()) == 2 and kv.planes()[0] is kv.k


# ------------------------------------------------------------ 3. prompt reuse

@pytest.mark.parametrize("variant", ["plain", "chunk8", "busy"])
@pytest.mark.parametrize("kv_bits", [16, 8])
def test_prompt_region_reuse_is_token_exact(kv_bits, variant):
    """B = P + S after A = P: B's first frame reports 48 cached tokens and
    B's tokens equal those of a runtime without the cache. chunk8: the
    suffix goes through the chunked admission state; busy: another stream
    decodes throughout and keeps its solo tokens."""
    chunk = 8 if variant == "chunk8" else None
    with env(DNET_KV_PREFIX_MIN=16, DNET_PREFILL_CHUNK=chunk):
        w = Rt(kv_bits=kv_bits, prefix_entries=2)
        try:
            assert w.rt.prefix is not None and w.rt.prefix.min_prefix == 16
            if variant == "busy":
                w.put("D", D8, 60)
                w.tick(2)
            w.put("A", P48, 4)
            w.run_until(lambda: w.finished("A"))
            a = w.toks("A")
            assert len(a) == 4
            assert w.frames["A"][0]["cached_tokens"] == 0
            assert "cached_tokens" not in w.frames["A"][1]
            S = suffix_avoiding(a[0])
            w.put("B", P48 + S, 8)
            w.run_until(lambda: w.finished("B"))
            assert w.frames["B"][0]["cached_tokens"] == 48
            if variant == "busy":
                assert not w.finished("D")       # it really ran throughout
            w.run_all()
            warm_b, warm_d = w.toks("B"), w.toks("D")
            st = w.rt.prefix_stats()
            assert st["hits"] == 1 and st["tokens_reused"] == 48
        finally:
            w.close()
    cold = cold_tokens(kv_bits, [("A", P48, 4), ("B", P48 + S, 8)])
    assert cold["A"] == a
    assert warm_b == cold["B"] and len(warm_b) == 8
    if variant == "busy":
        assert warm_d == cold_tokens(kv_bits, [("D", D8, 60)])["D"]
        assert len(warm_d) == 60


# ------------------------------------------------------------ 4. retirement

@pytest.mark.parametrize("kv_bits", [16, 8])
def test_retirement_bookkeeping_and_generated_reuse(kv_bits):
    pcc.retirement_scenario(kv_bits)


# ------------------------------------------------------------ 5. policy

def test_policy_opt_out_min_prefix_and_equal_prompt():
    with env(DNET_KV_PREFIX_MIN=16, DNET_PREFILL_CHUNK=None):
        w = Rt(prefix_entries=2)
        try:
            w.put("A", P48, 4)
            w.run_all()
            a = w.toks("A")
            ins = w.rt.prefix.inserts
            S = suffix_avoiding(a[0])
            # opt-out: neither lookup nor insert
            w.put("B", P48 + S, 4, cache_prompt=False)
            w.run_all()
            assert w.frames["B"][0]["cached_tokens"] == 0
            assert w.rt.prefix.inserts == ins
            assert w.rt.prefix.hits == 0 and w.rt.prefix.misses == 1
            # shares 10 < prefix_min tokens with the entry
            w.put("M", P48[:10] + [250] * 30, 2)
            w.run_all()
            assert w.frames["M"][0]["cached_tokens"] == 0
            # a prompt EQUAL to an entry's tokens: T - 1 rows, cold tokens
            w.put("E", P48, 4)
            w.run_all()
            assert w.frames["E"][0]["cached_tokens"] == 47
            assert w.toks("E") == a
        finally:
            w.close()
    assert cold_tokens(16, [("A", P48, 4)])["A"] == a


def test_policy_eviction_and_cancel():
    p1 = P48
    p2 = [(5 * i + 1) % 241 for i in range(40)]
    p3 = [(3 * i + 2) % 233 for i in range(40)]
    with env(DNET_KV_PREFIX_MIN=16, DNET_PREFILL_CHUNK=None):
        w = Rt(prefix_entries=2)
        try:
            for n, p in (("1", p1), ("2", p2)):
                w.put(n, p, 2)
                w.run_all()
            assert w.rt.prefix.evictions == 0
            # p1's entry is the LRU one; asking for exactly what p2's entry
            # holds (prompt + first generated token) hits without inserting
            w.put("2b", p2 + w.toks("2")[:1], 1)
            w.run_all()
            assert w.frames["2b"][0]["cached_tokens"] == 40
            assert w.rt.prefix.evictions == 0 and w.rt.prefix.inserts == 4
            w.put("3", p3, 2)                     # evicts p1's entry (LRU)
            w.run_all()
            assert w.rt.prefix.evictions == 1
            w.put("1b", p1 + [9, 9], 2)
            w.run_until(lambda: "1b" in w.frames)
            assert w.frames["1b"][0]["cached_tokens"] == 0
            w.run_all()
            # a cancelled request still stores T + m - 1 rows
            p4 = [(13 * i + 7) % 229 for i in range(20)]
            w.put("X", p4, 60)
            w.run_until(lambda: len(w.frames.get("X", [])) >= 3)
            m = len(w.frames["X"])
            w.rt.submit_cancel("X")
            w.tick()
            assert all(s is None for s in w.rt.slots)
            e = w.entry_with(p4 + w.toks("X")[:m - 1])
            assert e >= 0 and w.rt.prefix.length(e) == 20 + m - 1
            w.run_all()
        finally:
            w.close()


def test_policy_unsupported_configurations_stay_off():
    from dnet_amd.core.types import ShardLoadModelRequest
    from dnet_amd.shard.runtime import ShardRuntime
    with env(DNET_KV_PREFIX_MIN=16):
        w = Rt(prefix_entries=2, max_batch=1)     # serial path
        try:
            assert w.rt.prefix is None and w.rt.prefix_kv is None
            assert w.rt.prefix_stats() == {}
        finally:
            w.close()
    # multi-rank: decided from the request alone (no process group here)
    req = ShardLoadModelRequest(model_path="tiny", world_size=2,
                                max_batch=4, prefix_entries=2)
    assert ShardRuntime._prefix_supported(req, cp=1) is False
    assert ShardRuntime._prefix_supported(
        req.model_copy(update={"world_size": 1}), cp=1) is True
    assert ShardRuntime._prefix_supported(
        req.model_copy(update={"world_size": 1}), cp=2) is False
    # default: off, and a token frame without the key
    w = Rt(prefix_entries=0)
    try:
        assert w.rt.prefix is None
        w.put("A", P48, 2)
        w.run_all()
        assert all("cached_tokens" not in f for f in w.frames["A"])
    finally:
        w.close()


def test_settings_and_request_fields():
    from dnet_amd.api.models import APILoadModelRequest
    from dnet_amd.config import get_settings
    from dnet_amd.core.types import ShardLoadModelRequest
    assert ShardLoadModelRequest(model_path="x").prefix_entries == 0
    assert APILoadModelRequest(model="x").prefix_cache == 0
    with env(DNET_KV_PREFIX_ENTRIES=None, DNET_KV_PREFIX_MIN=None):
        s = get_settings().kv_cache
        assert (s.prefix_entries, s.prefix_min) == (0, 32)
    with env(DNET_KV_PREFIX_ENTRIES=3, DNET_KV_PREFIX_MIN=8):
        s = get_settings().kv_cache
        assert (s.prefix_entries, s.prefix_min) == (3, 8)


# ------------------------------------------------------------ 6. API

def _chat(first_frame_extra: dict, **req_kw):
    from dnet_amd.api.inference import InferenceManager
    from dnet_amd.api.models import ChatRequestModel
    from dnet_amd.api.tokenizer import ByteTokenizer

    class MM:
        tokenizer = ByteTokenizer(512)
        stop_ids = [ByteTokenizer(512).EOS]

    sent = []

    class FakeHead:
        def __init__(self, im):
            self.im = im

        async def request(self, frame):
            sent.append(frame)

            async def feed():
                nonce = frame["nonce"]
                for i, ch in enumerate(b"ok"):
                    fr = {"t": "token", "nonce": nonce, "token_id": int(ch),
                          "finished": False}
                    if i == 0:
                        fr.update(first_frame_extra)
                    self.im.resolve_token(fr)
                self.im.resolve_token({"t": "token", "nonce": nonce,
                                       "token_id": MM.stop_ids[0],
                                       "finished": True})
            asyncio.get_event_loop().create_task(feed())
            return {"t": "ack"}

    im = InferenceManager(MM(), token_timeout_s=10)
    im.head_client = FakeHead(im)
    im.callback_addr = "127.0.0.1:1"

    async def run():
        req = ChatRequestModel(model="tiny-random", profile=True,
                               messages=[{"role": "user", "content": "hi"}],
                               **req_kw)
        return await im.chat_completions(req)

    return asyncio.run(run()), sent


def test_api_reports_cached_tokens():
    resp, sent = _chat({"cached_tokens": 48})
    assert resp.choices[0].message.content == "ok"
    assert resp.usage.prompt_tokens_details == {"cached_tokens": 48}
    assert resp.metrics["cached_tokens"] == 48
    assert resp.model_dump()["usage"]["prompt_tokens_details"] == \
        {"cached_tokens": 48}
    assert sent[0]["params"]["cache_prompt"] is True
    # a miss is reported as 0, not dropped
    resp, _ = _chat({"cached_tokens": 0})
    assert resp.usage.prompt_tokens_details == {"cached_tokens": 0}
    assert resp.metrics["cached_tokens"] == 0


def test_api_without_cache_has_no_new_keys():
    resp, sent = _chat({}, cache_prompt=False)
    assert resp.usage.prompt_tokens_details is None
    assert "cached_tokens" not in resp.metrics
    for dumped in (resp.model_dump(), resp.model_dump(exclude_none=True)):
        assert "prompt_tokens_details" not in dumped["usage"]
        assert set(dumped["usage"]) == {"prompt_tokens", "completion_tokens",
                                        "total_tokens"}
    assert "prompt_tokens_details" not in resp.model_dump_json()
    assert sent[0]["params"]["cache_prompt"] is False

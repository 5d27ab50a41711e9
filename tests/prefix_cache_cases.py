"""Shared cases and drivers for the prefix-cache tests (CPU and GPU files):
the kv_copy_rows case list with an independent expected result, and an
in-process ShardRuntime driver for the serving scenarios."""
from __future__ import annotations

import contextlib
import itertools
import os

import numpy as np
import torch

# ------------------------------------------------------------ kernel cases

PLANE_SETS = ("int8_d128", "int8_d64", "bf16_d128", "mla")
ROW_RANGES = ((0, 1), (1, 2), (7, 8), (3, 50), (0, "S"), (5, 5))
_PARAMS = {
    "planes": PLANE_SETS,
    "L": (1, 3),
    "H": (1, 2),
    "S": (50, 64),    # 50: segments no 16-B multiples, src/dst misaligned
    "Bs": (1, 3),
    "Bd": (1, 2),
    "rows": ROW_RANGES,
}


def _all_pairs(params: dict) -> list:
    """Greedy pairwise cover of the parameter table (deterministic): every
    value pair of every two parameters occurs in at least one case. Not the
    full product (768 cases)."""
    names = list(params)
    todo = set()
    for a, b in itertools.combinations(range(len(names)), 2):
        for va in params[names[a]]:
            for vb in params[names[b]]:
                todo.add((a, va, b, vb))
    full = list(itertools.product(*(params[n] for n in names)))
    cases = []
    while todo:
        def gain(c):
            return sum(1 for a, b in itertools.combinations(
                range(len(names)), 2) if (a, c[a], b, c[b]) in todo)
        best = max(full, key=gain)       # first maximum: deterministic
        for a, b in itertools.combinations(range(len(names)), 2):
            todo.discard((a, best[a], b, best[b]))
        cases.append(dict(zip(names, best)))
    return cases


def kernel_cases() -> list:
    """Dicts with planes, L, H, S, Bs, Bd, src_b, dst_b, r0, r1, alias."""
    out = []
    for c in _all_pairs(_PARAMS):
        c = dict(c)
        r0, r1 = c.pop("rows")
        c["r0"], c["r1"] = r0, (c["S"] if r1 == "S" else r1)
        c["src_b"], c["dst_b"] = c["Bs"] - 1, c["Bd"] - 1
        c["alias"] = False
        out.append(c)
    # src and dst the SAME tensors, different batch indices
    for i, ps in enumerate(PLANE_SETS):
        r0, r1 = ((3, 50), (0, 50), (1, 2), (7, 8))[i]
        out.append(dict(planes=ps, L=2, H=2, S=50, Bs=3, Bd=3, src_b=2,
                        dst_b=0, r0=r0, r1=r1, alias=True))
    # sizes at which the kernel takes another path (see make_planes):
    # big: 1.1 MB segments, past one pass of the capped chunk grid (the
    #      4-deep main loop, its remainder, the grid stride), plus a 2-byte
    #      plane whose src/dst are 8 bytes out of phase;
    # many: more segments than the capped segment grid, 2 bytes out of phase;
    # bytes: odd row bytes, src/dst an odd number of bytes out of phase.
    out.append(dict(planes="big", L=1, H=1, S=1100, Bs=2, Bd=1, src_b=1,
                    dst_b=0, r0=1, r1=1100, alias=False))
    out.append(dict(planes="many", L=64, H=131, S=5, Bs=2, Bd=1, src_b=1,
                    dst_b=0, r0=0, r1=5, alias=False))
    out.append(dict(planes="bytes", L=2, H=3, S=5, Bs=2, Bd=1, src_b=1,
                    dst_b=0, r0=1, r1=4, alias=False))
    return out


def case_id(c: dict) -> str:
    return (f"{c['planes']}-L{c['L']}H{c['H']}S{c['S']}-B{c['Bs']}to{c['Bd']}"
            f"-r{c['r0']}_{c['r1']}" + ("-alias" if c["alias"] else ""))


def _rand_like(shape, dtype, gen) -> torch.Tensor:
    """Every bit pattern, none of them zero-biased: raw random bytes."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(1, 256, (n,), dtype=torch.int16, generator=gen)
    return raw.to(torch.uint8).view(dtype).view(*shape)


def make_planes(kind: str, L: int, B: int, H: int, S: int, seed: int) -> list:
    """CPU cache planes of one plane set, filled with a non-zero pattern."""
    g = torch.Generator().manual_seed(seed)
    if kind == "mla":          # latent: [L, B, S, row], H = 1
        return [_rand_like((L, B, S, 512), torch.bfloat16, g),   # 1024 B
                _rand_like((L, B, S, 64), torch.bfloat16, g)]    # 128 B
    if kind == "big":          # 1024-B rows + 2-B rows, long S
        return [_rand_like((L, B, H, S, 512), torch.bfloat16, g),
                _rand_like((L, B, H, S, 1), torch.bfloat16, g)]
    if kind == "many":         # 2-B rows, L*H segments
        return [_rand_like((L, B, H, S, 1), torch.bfloat16, g)]
    if kind == "bytes":        # 3-B rows
        return [_rand_like((L, B, H, S, 3), torch.int8, g)]
    if kind == "bf16_d128":
        return [_rand_like((L, B, H, S, 128), torch.bfloat16, g)
                for _ in range(2)]
    d = 128 if kind == "int8_d128" else 64
    return ([_rand_like((L, B, H, S, d), torch.int8, g) for _ in range(2)]
            + [_rand_like((L, B, H, S, d // 64), torch.bfloat16, g)
               for _ in range(2)])                # 4-B / 2-B scale rows


def as_int(t: torch.Tensor) -> torch.Tensor:
    """Integer view for bit-for-bit comparison (bf16 NaN patterns too)."""
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def expected_bytes(dst: torch.Tensor, dst_b: int, src: torch.Tensor,
                   src_b: int, r0: int, r1: int) -> np.ndarray:
    """Expected dst after the copy as raw bytes, built segment by segment
    with explicit byte offsets (no slice assignment on the cache layout):
    per (l, h) the bytes [r0*rb, r1*rb) of the S*rb-byte head block."""
    L, Bd = dst.shape[0], dst.shape[1]
    Bs = src.shape[1]
    S, rb = dst.shape[-2], dst.shape[-1] * dst.element_size()
    H = int(np.prod(dst.shape[2:-2])) if dst.dim() > 4 else 1
    d = dst.cpu().contiguous().view(torch.uint8).numpy().reshape(
        L, Bd, H * S * rb).copy()
    s = src.cpu().contiguous().view(torch.uint8).numpy().reshape(
        L, Bs, H * S * rb)
    for l in range(L):
        for h in range(H):
            a, b = h * S * rb + r0 * rb, h * S * rb + r1 * rb
            d[l, dst_b, a:b] = s[l, src_b, a:b]
    return d.reshape(-1)


def raw_bytes(t: torch.Tensor) -> np.ndarray:
    return t.cpu().contiguous().view(torch.uint8).numpy().reshape(-1)


# ------------------------------------------------------------ runtime driver

P48 = [(7 * i + 3) % 251 for i in range(48)]
S16 = [(11 * i + 5) % 239 for i in range(16)]
D8 = [200 + i for i in range(8)]          # the "other stream" prompt


@contextlib.contextmanager
def env(**kv):
    """Set environment variables (None = unset) and re-read the settings;
    restore both on the way out."""
    from dnet_amd.config import reset_settings
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        reset_settings()
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        reset_settings()


class Rt:
    """In-process ShardRuntime("tiny") with a frame-capturing callback."""

    def __init__(self, kv_bits: int = 16, prefix_entries: int = 0,
                 max_batch: int = 2, max_seq: int = 128, world_size: int = 1):
        from dnet_amd.core.types import ShardLoadModelRequest
        from dnet_amd.shard.runtime import ShardRuntime
        self.frames: dict = {}
        frames = self.frames

        class Cap:
            def send(self, fr):
                frames.setdefault(fr["nonce"], []).append(dict(fr))

            def close(self):
                pass

        self.rt = ShardRuntime("prefix")
        self.rt._load(ShardLoadModelRequest(
            model_path="tiny", model_name="tiny", total_layers=4,
            layers=[0, 1, 2, 3], rank=0, world_size=world_size,
            max_batch=max_batch, max_seq=max_seq, kv_bits=kv_bits,
            prefix_entries=prefix_entries))
        self.rt._callback = Cap()

    def put(self, nonce: str, tokens: list, max_tokens: int, **params):
        self.rt.infer_q.put({
            "nonce": nonce, "prompt_len": len(tokens),
            "tokens": np.asarray(tokens, dtype=np.int32).tobytes(),
            "max_tokens": max_tokens, "stop_ids": [], "params": params})

    def tick(self, n: int = 1):
        for _ in range(n):
            self.rt._slots_tick()

    def toks(self, nonce: str) -> list:
        return [f["token_id"] for f in self.frames.get(nonce, [])]

    def finished(self, nonce: str) -> bool:
        fr = self.frames.get(nonce, [])
        return bool(fr) and bool(fr[-1]["finished"])

    def idle(self) -> bool:
        rt = self.rt
        return (all(s is None for s in rt.slots) and rt._pending is None
                and rt.infer_q.empty())

    def run_until(self, cond, limit: int = 200):
        for _ in range(limit):
            if cond():
                return
            self.rt._slots_tick()
        assert cond(), "scenario did not reach its end state"

    def run_all(self):
        self.run_until(self.idle)

    def slot_of(self, nonce: str) -> int:
        return next(i for i, s in enumerate(self.rt.slots)
                    if s is not None and s.get("nonce") == nonce)

    def slot_rows(self, si: int, r1: int) -> list:
        """Clone rows [0, r1) of slot si, every plane, integer view."""
        return [as_int(p)[:, si, ..., :r1, :].clone()
                for p in self.rt.executor.kvs[0].planes()]

    def entry_rows(self, e: int, r1: int) -> list:
        return [as_int(p)[:, e, ..., :r1, :].clone()
                for p in self.rt.prefix_kv.planes()]

    def entry_with(self, tokens: list) -> int:
        """Index of the store entry whose token list is exactly `tokens`."""
        for e in range(self.rt.prefix.entries):
            if self.rt.prefix.tokens[e].tolist() == list(tokens):
                return e
        return -1

    def close(self):
        self.rt._unload()


def suffix_avoiding(first_generated: int) -> list:
    """S16 with S[0] != A's first generated token (so B shares exactly the
    48 prompt rows with the entry A leaves behind)."""
    s = list(S16)
    if s[0] == first_generated:
        s[0] = (s[0] + 1) % 251
    return s


def cold_tokens(kv_bits: int, jobs: list, chunk=None) -> dict:
    """Tokens of `jobs` [(nonce, prompt, max_tokens)], run one after the
    other on a fresh runtime with the cache off."""
    with env(DNET_PREFILL_CHUNK=chunk):
        c = Rt(kv_bits=kv_bits, prefix_entries=0)
        try:
            for nonce, prompt, mt in jobs:
                c.put(nonce, prompt, mt)
                c.run_all()
            assert c.rt.prefix is None
            return {n: c.toks(n) for n, _, _ in jobs}
        finally:
            c.close()


def retirement_scenario(kv_bits: int):
    """A = P48 (4 tokens) retires while D keeps
    decoding: the entry is rows [0, 51) of A's slot, bit for bit; it stays
    so over later ticks; C = P + g1..g3 + S then takes all 51 rows."""
    with env(DNET_KV_PREFIX_MIN=16, DNET_PREFILL_CHUNK=None):
        w = Rt(kv_bits=kv_bits, prefix_entries=2)
        try:
            w.put("D", D8, 100)
            w.tick(2)
            w.put("A", P48, 4)
            w.run_until(lambda: "A" in w.frames)
            sa = w.slot_of("A")
            # tick by tick up to the one that emits A's finished frame; the
            # slot rows are cloned right after that same tick
            w.run_until(lambda: w.finished("A"))
            slot = w.slot_rows(sa, 51)
            a = w.toks("A")
            assert len(a) == 4
            T, m = 48, 4
            R = T + m - 1
            e = w.entry_with(P48 + a[:3])
            assert e >= 0 and w.rt.prefix.length(e) == R == 51
            entry = w.entry_rows(e, 51)
            assert len(entry) == (4 if kv_bits == 8 else 2)
            for x, y in zip(entry, slot):
                assert torch.equal(x, y)
            # the freed slot's row 0 is overwritten by dummy appends and one
            # more step was in flight: none of it may reach the entry
            w.tick(7)
            assert not w.finished("D")
            for x, y in zip(w.entry_rows(e, 51), entry):
                assert torch.equal(x, y)
            assert any(not torch.equal(x[..., :1, :], y[..., :1, :])
                       for x, y in zip(w.slot_rows(sa, 51), slot)), \
                "row 0 of the freed slot was expected to be overwritten"
            S = suffix_avoiding(-1)
            w.put("C", P48 + a[:3] + S, 8)
            w.run_until(lambda: "C" in w.frames)
            assert w.frames["C"][0]["cached_tokens"] == 51
            sc = w.slot_of("C")
            for x, y in zip(w.slot_rows(sc, 51), entry):
                assert torch.equal(x, y)
            w.run_until(lambda: w.finished("C"))
            c = w.toks("C")
            assert len(c) == 8 and all(0 <= t < 256 for t in c)
        finally:
            w.close()

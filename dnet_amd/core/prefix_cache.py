"""Host-side index of the prompt-prefix KV store.

The store itself is a second KV cache object with ``entries`` batch rows
(shard/runtime.py); this class only decides WHICH entry a prompt can reuse
and which entry a finished prompt goes to. Pure Python/numpy, no GPU calls.

Invariant kept by the runtime: row j of an entry holds the KV of
``tokens[j]`` — so a prompt sharing its first n tokens with an entry can
take rows [0, n) verbatim and prefill only [n, T).
"""
from __future__ import annotations

import numpy as np


def _lcp(a: np.ndarray, b: np.ndarray) -> int:
    """Length of the longest common prefix of two int arrays."""
    n = min(a.shape[0], b.shape[0])
    if n == 0:
        return 0
    ne = np.flatnonzero(a[:n] != b[:n])
    return int(ne[0]) if ne.size else n


class PrefixCache:
    def __init__(self, entries: int, min_prefix: int = 32):
        self.entries = int(entries)
        self.min_prefix = max(1, int(min_prefix))
        self.tokens = [np.zeros(0, dtype=np.int32)
                       for _ in range(self.entries)]
        self.last_use = [0] * self.entries     # 0 = never used / empty
        self._tick = 0
        self.hits = self.misses = self.tokens_reused = 0
        self.inserts = self.evictions = 0

    def length(self, e: int) -> int:
        return int(self.tokens[e].shape[0])

    def _touch(self, e: int) -> None:
        self._tick += 1
        self.last_use[e] = self._tick

    def lookup(self, prompt) -> tuple:
        """(entry, n): the entry sharing the longest prefix with `prompt`
        and that prefix's length, capped at len(prompt) - 1 (one token must
        still be prefilled to get logits). (-1, 0) on a miss, i.e. when
        n < min_prefix. Ties go to the most recently used entry; a hit
        makes its entry the most recently used."""
        p = np.asarray(prompt, dtype=np.int32).reshape(-1)
        cap = p.shape[0] - 1
        best, best_n = -1, 0
        for e in range(self.entries):
            if self.length(e) == 0:
                continue
            n = min(_lcp(self.tokens[e], p), cap)
            if n > best_n or (n == best_n and best >= 0
                              and self.last_use[e] > self.last_use[best]):
                best, best_n = e, n
        if best < 0 or best_n < self.min_prefix:
            self.misses += 1
            return -1, 0
        self.hits += 1
        self.tokens_reused += best_n
        self._touch(best)
        return best, best_n

    def plan_insert(self, tokens) -> tuple:
        """(entry, have) for storing the KV rows of `tokens`: the caller
        copies rows [have, len(tokens)) into `entry`. (-1, 0) when an entry
        already covers `tokens` (they are a prefix of it, or equal). An
        entry whose tokens are a prefix of `tokens` is extended in place
        (`have` = its old length); otherwise an empty entry, else the
        least recently used one, is overwritten from row 0. The index is
        updated here, so the copy must follow."""
        t = np.asarray(tokens, dtype=np.int32).reshape(-1).copy()
        if self.entries == 0 or t.shape[0] == 0:
            return -1, 0
        extend = -1
        for e in range(self.entries):
            le = self.length(e)
            if le == 0:
                continue
            n = _lcp(self.tokens[e], t)
            if n == t.shape[0]:
                self._touch(e)           # covered already: nothing to copy
                return -1, 0
            if n == le and (extend < 0 or le > self.length(extend)):
                extend = e
        if extend >= 0:
            have = self.length(extend)
            self.tokens[extend] = t
            self._touch(extend)
            self.inserts += 1
            return extend, have
        empty = [e for e in range(self.entries) if self.length(e) == 0]
        if empty:
            e = empty[0]
        else:
            e = min(range(self.entries), key=lambda i: self.last_use[i])
            self.evictions += 1
        self.tokens[e] = t
        self._touch(e)
        self.inserts += 1
        return e, 0

    def drop(self, e: int) -> None:
        """Forget entry `e` (its rows are no longer trustworthy)."""
        self.tokens[e] = np.zeros(0, dtype=np.int32)
        self.last_use[e] = 0

    def stats(self) -> dict:
        return {"entries": self.entries,
                "used": sum(1 for e in range(self.entries)
                            if self.length(e)),
                "hits": self.hits, "misses": self.misses,
                "tokens_reused": self.tokens_reused,
                "inserts": self.inserts, "evictions": self.evictions}

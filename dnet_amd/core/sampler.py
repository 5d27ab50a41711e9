"""Token sampling: repetition / presence / frequency penalties,
temperature / top-k / top-p / min-p + logprobs.

Reference counterpart: src/dnet/core/decoding/sampler.py (mlx_lm
make_sampler); here implemented on torch logits [B, V].
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class DecodingConfig:
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    logprobs: bool = False
    top_logprobs: int = 0
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    # OpenAI `logit_bias`: token id -> additive bias on the raw logit
    logit_bias: Optional[dict] = None

    @property
    def has_penalty(self) -> bool:
        return (self.repetition_penalty != 1.0 or self.presence_penalty != 0.0
                or self.frequency_penalty != 0.0)

    @property
    def has_bias(self) -> bool:
        return bool(self.logit_bias)


def new_seen_table(rows: int, vocab: int, device=None) -> torch.Tensor:
    """Per-row token history for the penalties: bits 0..29 count how often
    the request generated the token, bit 30 marks prompt tokens."""
    return torch.zeros(rows, vocab, dtype=torch.int32, device=device)


def mark_prompt(seen_row: torch.Tensor, tokens) -> None:
    idx = torch.as_tensor(tokens, dtype=torch.long,
                          device=seen_row.device).reshape(-1)
    seen_row[idx] |= _ops().ref.SEEN_PROMPT_BIT


def fill_bias_row(row: torch.Tensor, logit_bias) -> None:
    """Zero one [V] f32 row of a bias table and scatter a request's
    `logit_bias` (id -> value) into it. Ids outside [0, V) are dropped and
    never written; of two entries for one id the last wins."""
    V = row.shape[0]
    row.zero_()
    ent = {int(k): float(v) for k, v in dict(logit_bias or {}).items()
           if 0 <= int(k) < V}
    if ent:
        row[torch.tensor(list(ent), dtype=torch.long, device=row.device)] = \
            torch.tensor(list(ent.values()), dtype=torch.float32,
                         device=row.device)


def _ops():
    from .. import ops
    return ops


def _fused_on() -> bool:
    from ..config import get_settings
    return bool(get_settings().sampling.fused_sampler)


class Sampler:
    def __init__(self, cfg: DecodingConfig | None = None,
                 generator: Optional[torch.Generator] = None):
        self.cfg = cfg or DecodingConfig()
        self.generator = generator

    def sample(self, logits: torch.Tensor, seen: torch.Tensor | None = None,
               bias: torch.Tensor | None = None):
        """logits [B, V] -> (tokens [B] int64, logprob [B] or None,
        top_logprobs list or None). A `bias` row [1, V] or table [B, V]
        (f32, the request's logit_bias) is added to the raw logits first;
        with a `seen` table [B, V] the config's penalties then shape the
        choice and the returned tokens are counted in it. Logprobs stay on
        the raw logits."""
        c = self.cfg
        lf = logits.float()
        raw = logits if logits.dtype == torch.bfloat16 else lf
        if bias is not None:
            lf = _ops().apply_logit_bias(lf, bias.expand(lf.shape[0], -1))
        if seen is not None and c.has_penalty:
            lf = _ops().apply_penalties(lf, seen, c.repetition_penalty,
                                        c.presence_penalty,
                                        c.frequency_penalty)
        tok = self._choose(lf)
        if seen is not None:
            _ops().count_tokens(seen, tok)
        return self._logprobs(raw, tok)

    def _choose(self, lf: torch.Tensor) -> torch.Tensor:
        c = self.cfg
        if c.temperature <= 0.0:
            tok = lf.argmax(dim=-1)
        else:
            x = lf / c.temperature
            if c.top_k and c.top_k > 0:
                kth = torch.topk(x, min(c.top_k, x.shape[-1]), dim=-1).values[..., -1:]
                x = x.masked_fill(x < kth, float("-inf"))
            if c.top_p < 1.0:
                sx, si = torch.sort(x, descending=True, dim=-1)
                probs = torch.softmax(sx, dim=-1)
                cum = probs.cumsum(dim=-1)
                keep = cum - probs < c.top_p  # keep at least the top token
                sx = sx.masked_fill(~keep, float("-inf"))
                x = torch.full_like(x, float("-inf")).scatter_(-1, si, sx)
            if c.min_p > 0.0:
                p = torch.softmax(x, dim=-1)
                x = x.masked_fill(p < c.min_p * p.amax(-1, keepdim=True),
                                  float("-inf"))
            probs = torch.softmax(x, dim=-1)
            # degenerate rows (NaN logits, or everything masked) would trip
            # multinomial's device-side assert and abort the whole process
            # (HSA exception) — fall back to greedy for those rows, without
            # a host sync (stays usable inside the serving loop)
            probs = torch.nan_to_num(probs, nan=0.0, posinf=0.0)
            ok = probs.sum(dim=-1, keepdim=True) > 0
            fallback = torch.nn.functional.one_hot(
                lf.nan_to_num(nan=0.0).argmax(dim=-1), lf.shape[-1]).float()
            probs = torch.where(ok, probs, fallback)
            tok = torch.multinomial(probs, 1, generator=self.generator).squeeze(-1)
        return tok

    def _logprobs(self, raw, tok):
        """Logprobs of the raw (unbiased, unpenalised) logits: one launch
        of the HIP logprob kernel on GPU logits, torch on f32 otherwise."""
        c = self.cfg
        if not c.logprobs:
            return tok, None, None
        if raw.is_cuda and _fused_on():
            B = raw.shape[0]
            K = min(int(c.top_logprobs or 0), 20)
            chosen, tv, ti = _ops().logprobs_rows(
                raw, tok, torch.full((B,), K, dtype=torch.int32,
                                     device=raw.device), K)
            tops = None
            if K:
                tv, ti = tv.tolist(), ti.tolist()
                tops = [{i: v for v, i in zip(tv[b], ti[b]) if i >= 0}
                        for b in range(B)]
            return tok, chosen, tops
        raw = raw.float()
        logp = raw - torch.logsumexp(raw, dim=-1, keepdim=True)
        chosen = logp.gather(-1, tok.unsqueeze(-1)).squeeze(-1)
        tops = None
        if c.top_logprobs:
            tv, ti = torch.topk(logp, c.top_logprobs, dim=-1)
            tops = [{int(i): float(v) for v, i in zip(tv[b], ti[b])}
                    for b in range(raw.shape[0])]
        return tok, chosen, tops


class RowSampler:
    """Per-row sampling for slot-batched serving: each row of the logits
    batch carries its own request's decoding params (temperature / top_k /
    top_p / min_p / penalties), vectorized in one pass. Greedy rows
    (temperature 0) take the argmax. On GPU logits every other batch is one
    launch of the fused HIP sampler (``ops.sample_rows``) on the bf16
    logits; CPU logits, and GPU ones when ``DNET_FUSED_SAMPLER=0``, go
    through per-row filtered multinomial with the same degenerate-row
    guard as ``Sampler``."""

    def __init__(self, batch: int, device=None, vocab: int | None = None):
        from ..config import get_settings
        self.batch = batch
        self.vocab = vocab         # sizes the token-history table
        self.device = device
        self.fused = bool(get_settings().sampling.fused_sampler)
        # penalties: neutral rows cost nothing; the [batch, V] token
        # history is allocated when the first penalised row is set
        self.rep = torch.ones(batch, device=device)
        self.pres = torch.zeros(batch, device=device)
        self.freq = torch.zeros(batch, device=device)
        self._pen_py = [False] * batch
        self.seen: Optional[torch.Tensor] = None
        # logit_bias: a dense [batch, V] f32 table, allocated when the
        # first biased row is set, and a per-row on/off flag
        self.bias: Optional[torch.Tensor] = None
        self.bias_on = torch.zeros(batch, dtype=torch.bool, device=device)
        self._bias_py = [False] * batch
        self._u0 = None            # zeros: uniforms of an all-greedy batch
        self.temp = torch.zeros(batch, device=device)
        self.top_p = torch.ones(batch, device=device)
        self.top_k = torch.zeros(batch, dtype=torch.long, device=device)
        self.min_p = torch.zeros(batch, device=device)
        self._has_min_p = False    # python-side (no device sync per step)
        # per-row RNG for seeded requests (OpenAI `seed`); None = shared
        # default stream. Seeded rows sample via inverse-CDF with a u drawn
        # from their own generator, so one request's stream is reproducible
        # regardless of which other slots are active.
        self.gens: list = [None] * batch
        # per-row logprob config (OpenAI `logprobs`/`top_logprobs`); the
        # sampler computes them for the WHOLE batch when any row wants
        # them, and the emitter picks per row
        self.want_lp: list = [False] * batch
        self.n_top: list = [0] * batch
        # the same per row for the HIP logprob kernel: -1 = row skipped
        self._ntop_dev = torch.full((batch,), -1, dtype=torch.int32,
                                    device=device)
        self.last_logp = None    # [B] device, chosen-token logprob
        self.last_topv = None    # [B, K] device
        self.last_topi = None
        # python-side mirrors: the hot sample() picks its fast path
        # (greedy-only / filterless) without device syncs
        self._temp_py = [0.0] * batch
        self._filt_py = [False] * batch

    def set_row(self, i: int, cfg: DecodingConfig, seed=None):
        self.rep[i] = cfg.repetition_penalty
        self.pres[i] = cfg.presence_penalty
        self.freq[i] = cfg.frequency_penalty
        self._pen_py[i] = cfg.has_penalty
        if cfg.has_penalty and self.seen is None:
            if self.vocab is None:
                raise ValueError("penalties need RowSampler(vocab=...)")
            self.seen = new_seen_table(self.batch, int(self.vocab),
                                       self.device)
        if self.seen is not None:
            self.seen[i].zero_()
        if cfg.has_bias:
            if self.bias is None:
                if self.vocab is None:
                    raise ValueError("logit_bias needs RowSampler(vocab=...)")
                self.bias = torch.zeros(self.batch, int(self.vocab),
                                        dtype=torch.float32,
                                        device=self.device)
            fill_bias_row(self.bias[i], cfg.logit_bias)
        self.bias_on[i] = cfg.has_bias
        self._bias_py[i] = cfg.has_bias
        self.temp[i] = cfg.temperature
        self.top_p[i] = cfg.top_p
        self.top_k[i] = cfg.top_k
        self.min_p[i] = cfg.min_p
        if cfg.min_p > 0:
            self._has_min_p = True
        self.want_lp[i] = bool(cfg.logprobs)
        self.n_top[i] = int(cfg.top_logprobs or 0)
        self._ntop_dev[i] = min(self.n_top[i], 20) if cfg.logprobs else -1
        self._temp_py[i] = float(cfg.temperature)
        self._filt_py[i] = bool(cfg.top_k or cfg.top_p < 1.0 or cfg.min_p)
        g = None
        if seed is not None:
            g = torch.Generator(device=self.device)
            g.manual_seed(int(seed))
        self.gens[i] = g
        return g

    def clear_row(self, i: int):
        """Reset a freed slot so stale sampling params don't keep the
        batch off the greedy fast path."""
        self.temp[i] = 0.0
        self.top_p[i] = 1.0
        self.top_k[i] = 0
        self.min_p[i] = 0.0
        self.rep[i] = 1.0
        self.pres[i] = 0.0
        self.freq[i] = 0.0
        self._pen_py[i] = False
        self.bias_on[i] = False
        self._bias_py[i] = False
        self._temp_py[i] = 0.0
        self._filt_py[i] = False
        self.want_lp[i] = False
        self.n_top[i] = 0
        self._ntop_dev[i] = -1
        self.gens[i] = None

    def note_prompt(self, i: int, tokens) -> None:
        """Mark row i's prompt tokens (after ``set_row``)."""
        if self.seen is not None and self._pen_py[i]:
            mark_prompt(self.seen[i], tokens)

    def seen_rows(self, i: int):
        """Row i of the token history as a [1, V] table for ``Sampler``,
        or None when the row carries no penalty."""
        if self.seen is not None and self._pen_py[i]:
            return self.seen[i:i + 1]
        return None

    def bias_rows(self, i: int):
        """Row i of the bias table as a [1, V] row for ``Sampler``, or None
        when the row carries no logit_bias."""
        if self.bias is not None and self._bias_py[i]:
            return self.bias[i:i + 1]
        return None

    def reset_counts(self, i: int) -> None:
        """Forget what row i was counted as generating, keep its prompt
        marks. Every row of the batch is sampled and counted each step,
        also a slot that is parked while its prompt prefills chunk by
        chunk; call this before the slot's first real token."""
        if self.seen is not None and self._pen_py[i]:
            self.seen[i] &= _ops().ref.SEEN_PROMPT_BIT

    def note_token(self, i: int, tok: int) -> None:
        """Count a token of row i that was sampled elsewhere (the first
        token of a slot comes from ``Sampler``)."""
        if self.seen is not None and self._pen_py[i]:
            _ops().count_tokens(self.seen[i:i + 1],
                                torch.tensor([int(tok)], device=self.device))

    def _uniforms(self, B, device):
        # seeded rows draw from their own generator, so a request's stream
        # depends on nothing but its seed
        u = torch.rand(B, 1, device=device)
        for i, g in enumerate(self.gens[:B]):
            if g is not None:
                u[i] = torch.rand(1, 1, device=device, generator=g)
        return u

    def _logprobs_for(self, lf, tok):
        """Logprobs of the raw logits for the rows that want them: GPU
        logits (bf16 or f32 as they come) take one launch of the HIP
        logprob kernel, which skips the other rows; the torch path works
        on f32 over the whole batch."""
        B = lf.shape[0]
        if lf.is_cuda and self.fused:
            if any(self.want_lp[:B]):
                kmax = min(max(self.n_top[:B]), 20)
                self.last_logp, tv, ti = _ops().logprobs_rows(
                    lf, tok, self._ntop_dev, kmax)
                self.last_topv, self.last_topi = (tv, ti) if kmax else \
                    (None, None)
            else:
                self.last_logp = self.last_topv = self.last_topi = None
            return
        lf = lf.float()
        if any(self.want_lp[:B]):
            logp = lf - torch.logsumexp(lf, dim=-1, keepdim=True)
            self.last_logp = logp.gather(-1, tok.unsqueeze(-1)).squeeze(-1)
            kmax = max(self.n_top[:B])
            if kmax > 0:
                self.last_topv, self.last_topi = torch.topk(logp, kmax,
                                                            dim=-1)
            else:
                self.last_topv = self.last_topi = None
        else:
            self.last_logp = self.last_topv = self.last_topi = None

    def sample(self, logits: torch.Tensor) -> torch.Tensor:
        B, V = logits.shape
        pen = any(self._pen_py[:B])
        biased = any(self._bias_py[:B])
        sampled = any(t > 0 for t in self._temp_py[:B])
        if logits.is_cuda and self.fused:
            if pen or sampled or biased:
                # one launch over the bf16 logits: bias, penalties,
                # temperature, filters and the draw, sort-free
                tok = _ops().sample_rows(
                    logits, self.temp, self.top_k, self.top_p, self.min_p,
                    self._uniforms(B, logits.device) if sampled
                    else self._zeros(),
                    self.rep if pen else None, self.pres if pen else None,
                    self.freq if pen else None, self.seen if pen else None,
                    bias=self.bias if biased else None,
                    bias_on=self.bias_on if biased else None)
            else:
                tok = logits.float().argmax(dim=-1)   # all-greedy fast path
            self._logprobs_for(logits, tok)
            return tok
        raw = lf = logits.float()
        if biased:
            lf = _ops().apply_logit_bias(lf, self.bias, self.bias_on)
        if pen:
            lf = _ops().apply_penalties(lf, self.seen, self.rep, self.pres,
                                        self.freq)
        tok = self._sample_torch(lf, raw, B, V)
        if pen:
            _ops().count_tokens(self.seen[:B], tok)
        return tok

    def _zeros(self):
        # all-greedy penalised batch: the kernel reads no uniform
        if self._u0 is None:
            self._u0 = torch.zeros(self.batch, device=self.device)
        return self._u0

    def _sample_torch(self, lf, raw, B, V):
        """Torch path over (penalised) f32 logits `lf`; logprobs are taken
        from the raw logits."""
        greedy_tok = lf.argmax(dim=-1)
        # fast path: every row greedy (the common serving batch) — the
        # full sort/softmax/multinomial over [B, V] cost ~25 ms/step on
        # a 152k vocab and collapsed serving throughput 4x (today's stack
        # measures 1.0-1.8 ms for it: profiles/r04_fused_sampler.md)
        if not any(t > 0 for t in self._temp_py[:B]):
            self._logprobs_for(raw, greedy_tok)
            return greedy_tok
        t = self.temp.clamp_min(1e-6).unsqueeze(-1)
        x = lf / t
        if not any(self._filt_py[:B]):
            # sampled but filterless: plain softmax + draw (no sort)
            probs = torch.softmax(x, dim=-1)
            probs = torch.nan_to_num(probs, nan=0.0, posinf=0.0)
            ok = probs.sum(dim=-1, keepdim=True) > 0
            fallback = torch.nn.functional.one_hot(
                lf.nan_to_num(nan=0.0).argmax(dim=-1), V).float()
            probs = torch.where(ok, probs, fallback)
            tok = self._draw(probs, B, V, lf.device)
            tok = torch.where(self.temp[:B] <= 0.0, greedy_tok, tok)
            self._logprobs_for(raw, tok)
            return tok
        sx, si = torch.sort(x, descending=True, dim=-1)
        ranks = torch.arange(V, device=lf.device).expand(B, V)
        keep = torch.ones_like(sx, dtype=torch.bool)
        # per-row top-k (0 = off)
        k = torch.where(self.top_k > 0, self.top_k,
                        torch.full_like(self.top_k, V))
        keep &= ranks < k.unsqueeze(-1)
        # per-row top-p (keep at least the top token)
        probs_s = torch.softmax(sx, dim=-1)
        cum = probs_s.cumsum(dim=-1)
        keep &= (cum - probs_s) < self.top_p.unsqueeze(-1)
        sx = sx.masked_fill(~keep, float("-inf"))
        x = torch.full_like(x, float("-inf")).scatter_(-1, si, sx)
        if self._has_min_p:
            p = torch.softmax(x, dim=-1)
            thresh = self.min_p.unsqueeze(-1) * p.amax(-1, keepdim=True)
            x = x.masked_fill(p < thresh, float("-inf"))
        probs = torch.softmax(x, dim=-1)
        probs = torch.nan_to_num(probs, nan=0.0, posinf=0.0)
        ok = probs.sum(dim=-1, keepdim=True) > 0
        fallback = torch.nn.functional.one_hot(
            lf.nan_to_num(nan=0.0).argmax(dim=-1), V).float()
        probs = torch.where(ok, probs, fallback)
        tok = self._draw(probs, B, V, lf.device)
        tok = torch.where(self.temp[:B] <= 0.0, greedy_tok, tok)
        self._logprobs_for(raw, tok)
        return tok

    def _draw(self, probs, B, V, device):
        if any(g is not None for g in self.gens[:B]):
            # inverse-CDF with per-row uniforms: seeded rows draw from
            # their own generator, unseeded rows from the default stream
            u = torch.rand(B, 1, device=device)
            for i, g in enumerate(self.gens[:B]):
                if g is not None:
                    u[i] = torch.rand(1, 1, device=device, generator=g)
            cdf = probs.cumsum(-1)
            return torch.searchsorted(
                cdf, u * cdf[..., -1:]).squeeze(-1).clamp_(0, V - 1)
        return torch.multinomial(probs, 1).squeeze(-1)

"""dnet_amd.ops — gfx950 HIP kernels with CPU reference fallback.

GPU tensors dispatch to the in-tree ``_C.so`` extension (hand-written
CDNA4/HIP kernels); if the extension is missing on a GPU machine the ops
FAIL LOUDLY — there is no silent eager fallback on the GPU path. CPU
tensors use the fp32 reference implementations (tests / no-GPU machines).
"""
from __future__ import annotations

import importlib.util
from pathlib import Path

import torch

from . import reference as ref

_SO = Path(__file__).resolve().parent / "_C.so"
_C = None
_load_error: Exception | None = None


def _try_load():
    global _C, _load_error
    if _C is not None or _load_error is not None:
        return _C
    try:
        spec = importlib.util.spec_from_file_location("dnet_amd.ops._C", _SO)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _C = mod
    except Exception as e:  # pragma: no cover
        _load_error = e
    return _C


def has_native() -> bool:
    return _try_load() is not None


def _native():
    c = _try_load()
    if c is None:
        raise RuntimeError(
            f"dnet_amd native extension not available ({_SO}): {_load_error}. "
            "Run `python -m dnet_amd.ops.build` — GPU tensors never fall back "
            "to eager.")
    return c


def set_reproducible(on: bool) -> None:
    """Opt-in bit-reproducible decode GEMMs (OFF by default).

    The split-k decode GEMM stores one f32 partial per split and its
    consumer sums them in a fixed order, so two launches already agree
    bit for bit; what still changes the last bit is the number of splits
    (a heuristic that may move between builds). When on, partials are
    rounded to a 2^-16 grid first, which makes the additions exact
    (independent of order and grouping) while sums stay below 2^8 — at
    the price of an absolute precision floor of 2^-17 per partial. Meant
    for synthetic benchmark runs with O(1) activations whose outputs are
    compared across runs or builds; leave it off for real checkpoints.
    Process-wide; set it before decode graphs are captured. The MoE expert
    kernels are not covered. CPU tensors use the reference path, which is
    reproducible already."""
    _native().set_splitk_exact(bool(on))


def rmsnorm(x: torch.Tensor, residual: torch.Tensor | None, w: torch.Tensor,
            eps: float = 1e-6) -> torch.Tensor:
    if x.is_cuda:
        y = torch.empty_like(x)
        _native().rmsnorm(x, residual, w, y, eps)
        return y
    return ref.rmsnorm(x, residual, w, eps)


# Per-device f32 buffers of 64 x 152064 elements each (the largest M=64
# pass, lm_head-class N).
_scratch: dict = {}
_partials: dict = {}
_SPLITK_ELEMS = 64 * 152064


def _get_scratch(device) -> torch.Tensor:
    """The zero-at-rest f32 buffer of the legacy (splits = 1) consumer
    mode. No GEMM writes it any more: callers that fill it themselves and
    run a *_f32 consumer with splits = 1 get it back zeroed."""
    key = str(device)
    if key not in _scratch:
        _scratch[key] = torch.zeros(_SPLITK_ELEMS, dtype=torch.float32,
                                    device=device)
    return _scratch[key]


def _get_partials(device) -> torch.Tensor:
    """Split-k partials of the decode GEMM, [sk][M][N] f32: split s stores
    its whole [M,N] tile into slice s and the consumer sums the slices, so
    the contents at rest mean nothing and are never cleaned. Too small a
    buffer silently lowers sk (measured on gateup N=55296 without split-k:
    864 blocks quantize badly onto 256 CUs at 3 blocks/CU); pick_splitk
    never asks for more than 8.4 M elements at M <= 64."""
    key = str(device)
    if key not in _partials:
        _partials[key] = torch.empty(_SPLITK_ELEMS, dtype=torch.float32,
                                     device=device)
    return _partials[key]


def gemv_bf16(x: torch.Tensor, w: torch.Tensor,
              bias: torch.Tensor | None = None) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        if x.shape[1] % 64 == 0:
            _native().gemm_m16(x, w, None, bias, out, _get_partials(x.device),
                               0, False, 16)
        else:
            _native().gemv_bf16(x, w, out, bias)
        return out
    return ref.gemv_bf16(x, w, bias)


def gemv_int8(x: torch.Tensor, w: torch.Tensor, scales: torch.Tensor,
              group: int, bias: torch.Tensor | None = None,
              packed: bool = False) -> torch.Tensor:
    """Two weight contracts: the MFMA path (packed, M > 2) and the CPU
    reference multiply by bf16(q*s); the scalar kernel (M <= 2, or unpacked
    weights at any M) multiplies by the unrounded q*s."""
    if x.is_cuda:
        out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        if packed and x.shape[0] > 2:
            _native().gemm_m16(x, w, scales, bias, out, _get_partials(x.device),
                               group, True, 8)
        else:
            # M<=2: the scalar GEMV reads 16B/lane and hits 4-5.6 TB/s
            _native().gemv_int8(x, w, scales, out, group, bias, packed)
        return out
    if packed:
        w = ref.unpack_int8_mfma(w)
    return ref.gemv_int8(x, w, scales, group, bias)


def gemv_int4(x: torch.Tensor, w: torch.Tensor, scales: torch.Tensor,
              group: int, bias: torch.Tensor | None = None,
              packed: bool = False) -> torch.Tensor:
    if x.is_cuda:
        assert packed, "GPU int4 path needs the packed layout"
        out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        _native().gemm_m16(x, w, scales, bias, out, _get_partials(x.device),
                           group, True, 4)
        return out
    return ref.gemv_int4(x, w, scales, group, bias)


def dequant_int4(w: torch.Tensor, scales: torch.Tensor, group: int,
                 packed: bool = True) -> torch.Tensor:
    if w.is_cuda:
        assert packed
        out = torch.empty(w.shape[0], w.shape[1] * 2, dtype=torch.bfloat16,
                          device=w.device)
        _native().dequant_int4(w, scales, out, group)
        return out
    return ref.dequant_int4(w, scales, group)


def dequant_int8(w: torch.Tensor, scales: torch.Tensor, group: int,
                 packed: bool = False) -> torch.Tensor:
    if w.is_cuda:
        out = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
        _native().dequant_int8(w, scales, out, group, packed)
        return out
    if packed:
        w = ref.unpack_int8_mfma(w)
    return ref.dequant_int8(w, scales, group)


def _attn_splits(b: int, hkv: int, smax: int) -> int:
    # fill ~1024 blocks (4/CU); cap so each split owns >= ~512 positions of
    # capacity (short actual sequences leave idle splits + combine overhead)
    import os
    force = os.environ.get("DNET_ATTN_SPLITS")
    if force:
        return max(1, int(force))
    splits = 1
    cap = max(1, smax // 512)
    # target ~2048 blocks (8/CU): measured at 2k ctx batch 32 (qwen-32b,
    # 512 base blocks) splits=4 runs 21.5 ms/step vs 27.2 at splits=2 —
    # serial chunks per block hurt more than combine overhead until the
    # per-split span drops under ~512 positions (the cap)
    while (b * hkv * splits * 2 <= 2048 and splits * 2 <= cap):
        splits *= 2
    return splits


def attn_decode(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                pos: torch.Tensor, scale: float, window: int = 0,
                sinks: torch.Tensor | None = None,
                kscale: torch.Tensor | None = None,
                vscale: torch.Tensor | None = None) -> torch.Tensor:
    if q.is_cuda:
        # q may be a strided slice of the fused QKV buffer; out is contiguous.
        B, Hq, D = q.shape
        dv = vcache.shape[-1]           # MLA: v head dim < qk head dim
        out = torch.empty(B, Hq, dv, dtype=q.dtype, device=q.device)
        splits = _attn_splits(B, kcache.shape[1], kcache.shape[2])
        partials = None
        if splits > 1:
            partials = torch.empty(B * Hq * splits * (dv + 2),
                                   dtype=torch.float32, device=q.device)
        _native().attn_decode(q, kcache, vcache, pos, out, scale, window,
                              sinks, kscale, vscale, partials, splits)
        return out
    return ref.attn_decode(q, kcache, vcache, pos, scale, window, sinks,
                           kscale, vscale)


_PREFILL_DIMS = {(128, 128), (64, 64), (192, 128), (96, 96)}


def attn_prefill_supported(d: int, dv: int) -> bool:
    return (d, dv) in _PREFILL_DIMS


def attn_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 scale: float, q_off: int, window: int = 0,
                 sinks: torch.Tensor | None = None) -> torch.Tensor:
    """Fused MFMA flash prefill attention (causal + window + sinks).

    q [B,Hq,T,D], k/v [B,Hkv,S,D(v)] -> [B,Hq,T,Dv]. GPU-only; callers
    gate on attn_prefill_supported and fall back to the chunked-einsum
    path otherwise (models/base.py)."""
    B, Hq, T, D = q.shape
    Dv = v.shape[-1]
    out = torch.empty(B, Hq, T, Dv, dtype=q.dtype, device=q.device)
    _native().attn_prefill(q.contiguous(), k.contiguous(), v.contiguous(),
                           sinks, out, q_off, window, scale)
    return out


def rope_append(q, k, v, kcache, vcache, pos, cos, sin,
                kscale=None, vscale=None, wpos=None) -> None:
    if q.is_cuda:
        _native().rope_append(q, k, v, kcache, vcache, pos, cos, sin,
                              kscale, vscale, wpos)
        return
    ref.rope_append(q, k, v, kcache, vcache, pos, cos, sin, kscale, vscale,
                    wpos)


_defer_cache: dict = {}


def _will_defer(M: int, N: int, K: int, group: int, bits: int,
                scratch_elems: int) -> bool:
    """scratch_elems: capacity of the partials buffer (the legacy scratch
    has the same size)."""
    key = (M, N, K, group, bits)
    v = _defer_cache.get(key)
    if v is None:
        v = _native().gemm_m16_will_defer(M, N, K, group, bits, scratch_elems)
        _defer_cache[key] = v
    return v


def gemv_qkv_rope(y: torch.Tensor, w: torch.Tensor, scales: torch.Tensor,
                  group: int, bits: int, bias, nq: int, nkv: int, d: int,
                  kcache, vcache, pos, cos, sin, kscale=None, vscale=None,
                  wpos=None):
    """Fused qkv GEMM + RoPE + KV append for the decode path: when the
    GEMM runs split-k, RoPE sums the f32 partial slices itself,
    applies the qkv bias, writes the rotated q to a
    dedicated buffer and k/v straight to the cache — the combine kernel
    and the bf16 k/v round trip disappear from the dependency chain.
    Returns the rotated q [B, nq, d]."""
    B = y.shape[0]
    part = _get_partials(y.device)
    if _will_defer(B, w.shape[0], y.shape[1], group, bits, part.numel()):
        out = torch.empty(B, w.shape[0], dtype=y.dtype, device=y.device)
        sk = _native().gemm_m16(y, w, scales, None, out, part, group, True,
                                bits, True)
        assert sk > 1, "will_defer disagreed with gemm_m16"
        q = torch.empty(B, nq, d, dtype=y.dtype, device=y.device)
        _native().rope_append_f32(part, bias, q, nkv, kcache, vcache,
                                  pos, cos, sin, kscale, vscale, wpos, sk)
        return q
    gemv = gemv_int8 if bits == 8 else gemv_int4
    qkv = gemv(y, w, scales, group, bias, True)
    q = qkv[:, :nq * d].view(B, nq, d)
    k = qkv[:, nq * d:(nq + nkv) * d].view(B, nkv, d)
    v = qkv[:, (nq + nkv) * d:].view(B, nkv, d)
    rope_append(q, k, v, kcache, vcache, pos, cos, sin, kscale, vscale,
                wpos=wpos)
    return q


class _Deferred:
    """Sentinel: the projection's result lives (un-combined, f32) in the
    split-k partials buffer; the consumer must sum its slices."""


DEFERRED = _Deferred()

# slices of the last gemv_defer per device: what a consumer called
# without an explicit count sums. Read when the consumer is launched (or
# captured), and handed to the kernel as an argument.
_deferred_splits: dict = {}


def gemv_defer(x: torch.Tensor, w: torch.Tensor, scales: torch.Tensor,
               group: int, bits: int) -> int:
    """Launch the GEMM leaving its f32 split-k partials un-combined
    (caller checked _will_defer). Returns the number of slices (> 1),
    which rmsnorm_f32_scratch / resid_add_scratch take as ``splits``."""
    out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
    sk = _native().gemm_m16(x, w, scales, None, out, _get_partials(x.device),
                            group, True, bits, True)
    assert sk > 1, "will_defer disagreed with gemm_m16"
    _deferred_splits[str(x.device)] = sk
    return sk


def rmsnorm_f32_scratch(residual: torch.Tensor, wn: torch.Tensor,
                        eps: float, splits: int | None = None) -> torch.Tensor:
    """RMSNorm(+residual) whose x input is the deferred f32 partials
    (``splits`` slices; default: those of the last gemv_defer)."""
    if splits is None:
        splits = _deferred_splits[str(residual.device)]
    y = torch.empty_like(residual)
    _native().rmsnorm_f32(_get_partials(residual.device), residual, wn, y,
                          eps, splits)
    return y


def resid_add_scratch(h: torch.Tensor, splits: int | None = None) -> None:
    """h += the deferred f32 partials (see rmsnorm_f32_scratch)."""
    if splits is None:
        splits = _deferred_splits[str(h.device)]
    _native().resid_add_f32(h, _get_partials(h.device), splits)


def linear_will_defer(x: torch.Tensor, w: torch.Tensor, group: int,
                      bits: int) -> bool:
    return _will_defer(x.shape[0], w.shape[0], x.shape[1], group, bits,
                       _get_partials(x.device).numel())


def gemv_rmsnorm(x: torch.Tensor, w: torch.Tensor, scales: torch.Tensor,
                 group: int, bits: int, residual: torch.Tensor,
                 wn: torch.Tensor, eps: float) -> torch.Tensor:
    """Fused projection GEMM + RMSNorm(+residual) for the decode path:
    when the GEMM runs split-k, the norm sums the f32 partial slices
    itself — the combine kernel disappears from the chain.
    Updates `residual` in place (residual += proj) like ops.rmsnorm."""
    part = _get_partials(x.device)
    if _will_defer(x.shape[0], w.shape[0], x.shape[1], group, bits,
                   part.numel()):
        out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype,
                          device=x.device)
        sk = _native().gemm_m16(x, w, scales, None, out, part, group, True,
                                bits, True)
        assert sk > 1, "will_defer disagreed with gemm_m16"
        y = torch.empty_like(residual)
        _native().rmsnorm_f32(part, residual, wn, y, eps, sk)
        return y
    gemv = gemv_int8 if bits == 8 else gemv_int4
    o = gemv(x, w, scales, group, None, True)
    return rmsnorm(o, residual, wn, eps)


def gemv_swiglu(x: torch.Tensor, w: torch.Tensor, scales: torch.Tensor,
                group: int, bits: int = 8,
                packed: bool = True) -> torch.Tensor:
    """Fused gate/up GEMM + SwiGLU for the decode path: when the GEMM
    runs split-k, SwiGLU sums the f32 partial slices itself
    instead of going through the f32->bf16 combine kernel — one fewer
    dependent ~5 us kernel per layer per step."""
    if not (x.is_cuda and packed and 2 < x.shape[0] <= 64):
        gemv = gemv_int8 if bits == 8 else gemv_int4
        return swiglu(gemv(x, w, scales, group, None, packed))
    M, N = x.shape[0], w.shape[0]
    out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    part = _get_partials(x.device)
    sk = _native().gemm_m16(x, w, scales, None, out, part, group, True,
                            bits, True)
    y = torch.empty(M, N // 2, dtype=x.dtype, device=x.device)
    if sk:
        _native().swiglu_f32(part, y, N, sk)
    else:
        _native().swiglu(out, y)
    return y


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    if gu.is_cuda:
        i = gu.shape[-1] // 2
        y = torch.empty(*gu.shape[:-1], i, dtype=gu.dtype, device=gu.device)
        _native().swiglu(gu, y)
        return y
    return ref.swiglu(gu)


def moe_gateup(x: torch.Tensor, w: torch.Tensor, scales, bias,
               we: torch.Tensor, group: int = 0, packed: bool = False,
               glu: int = 0, alpha: float = 1.702,
               limit: float = 7.0) -> torch.Tensor:
    """Grouped expert gate+up with fused GLU: x [M,K], stacked w [E,2I,K]
    (bf16 or grouped-int8), we [M,E] f32 routing weights -> act [E,M,I].
    Experts with all-zero we are skipped on GPU (their act rows hold
    garbage; moe_down never reads them)."""
    if x.is_cuda:
        e, i2, _ = w.shape
        act = torch.empty(e, x.shape[0], i2 // 2, dtype=torch.bfloat16,
                          device=x.device)
        _native().moe_gateup(x, w, scales, bias, we, act, group, packed,
                             glu, alpha, limit)
        return act
    return ref.moe_gateup(x, w, scales, bias, we, group, packed, glu,
                          alpha, limit)


def moe_down(act: torch.Tensor, w: torch.Tensor, scales, bias,
             we: torch.Tensor, group: int = 0,
             packed: bool = False) -> torch.Tensor:
    """Grouped expert down projection, weighted f32 accumulation:
    act [E,M,I], stacked w [E,H,I], we [M,E] -> out [M,H] f32."""
    if act.is_cuda:
        out = torch.zeros(act.shape[1], w.shape[1], dtype=torch.float32,
                          device=act.device)
        _native().moe_down(act, w, scales, bias, we, out, group, packed)
        return out
    return ref.moe_down(act, w, scales, bias, we, group, packed)


quantize_int8 = ref.quantize_int8
quantize_int4 = ref.quantize_int4
pack_int8_mfma = ref.pack_int8_mfma
pack_int4_mfma = ref.pack_int4_mfma
unpack_int8_mfma = ref.unpack_int8_mfma
rope_tables = ref.rope_tables
rope_apply = ref.rope_apply
mxfp4_dequant = ref.mxfp4_dequant
quantize_mxfp4 = ref.quantize_mxfp4
apply_penalties = ref.apply_penalties
count_tokens = ref.count_tokens
apply_logit_bias = ref.apply_logit_bias


def sample_rows(logits: torch.Tensor, temp: torch.Tensor,
                top_k: torch.Tensor, top_p: torch.Tensor,
                min_p: torch.Tensor, u: torch.Tensor, rep=None, pres=None,
                freq=None, seen: torch.Tensor | None = None,
                out: torch.Tensor | None = None,
                bias: torch.Tensor | None = None,
                bias_on: torch.Tensor | None = None) -> torch.Tensor:
    """Fused per-row sampler: logits [B, V] (bf16 or f32, row stride >= V)
    -> tokens [B] int64. Per-row temp / top_k / top_p / min_p and a uniform
    u in [0, 1); optional rep / pres / freq penalties over the int32 `seen`
    table [>= B, V], whose count for the returned token is incremented;
    optional f32 `bias` table [>= B, V] (dense rows, any stride >= V),
    added to the raw logit before the penalties on the rows whose
    `bias_on` flag (bool [>= B]) is set, on every row without flags. The
    parameter tensors may be longer than B. One launch on the current
    stream, no host sync; semantics in ``reference.sample_rows``."""
    if logits.is_cuda:
        B = logits.shape[0]
        if out is None:
            out = torch.empty(B, dtype=torch.int64, device=logits.device)
        if top_k.dtype != torch.int64:
            top_k = top_k.to(torch.int64)
        _native().sample_rows(logits, temp, top_k, top_p, min_p, rep, pres,
                              freq, seen, u.reshape(-1), out, bias,
                              bias_on if bias is not None else None)
        return out[:B]
    return ref.sample_rows(logits, temp, top_k, top_p, min_p, u, rep, pres,
                           freq, seen, bias, bias_on)


def logprobs_rows(logits: torch.Tensor, tok: torch.Tensor,
                  n_top: torch.Tensor, K: int, logp=None, topv=None,
                  topi=None):
    """Chosen-token and ordered top-K logprobs of raw logits [B, V] (bf16
    or f32, row stride >= V) -> (logp [B] f32, topv [B, K] f32, topi [B, K]
    int64), 0 <= K <= 20. `tok` [B] int64; `n_top` [B] int32 on the logits'
    device: -1 skips the row (its entries of the given outputs stay
    untouched), 0..20 is the number of top entries wanted; the rest up to K
    is (-1, NaN). One launch on the current stream, no sort, no host sync,
    bit-reproducible; semantics in ``reference.logprobs_rows``."""
    if logits.is_cuda:
        B = logits.shape[0]
        dev = logits.device
        if logp is None:
            logp = torch.empty(B, dtype=torch.float32, device=dev)
        if topv is None:
            topv = torch.empty(B, K, dtype=torch.float32, device=dev)
        if topi is None:
            topi = torch.empty(B, K, dtype=torch.int64, device=dev)
        _native().logprobs_rows(logits, tok, n_top, logp, topv, topi)
        return logp, topv, topi
    return ref.logprobs_rows(logits, tok, n_top, K, logp, topv, topi)


def kv_copy_rows(dst_planes, dst_b: int, src_planes, src_b: int, r0: int,
                 r1: int) -> None:
    """Copy KV rows [r0, r1) of batch index `src_b` to the same rows of
    batch index `dst_b`, for every plane (``KVCache.planes()``), local
    layer and head. A plane is a contiguous cache tensor
    [L, B, (H,) S, row]; L, H, S and row bytes must agree between a src
    plane and its dst plane, B may differ, and src may be dst itself with
    two different batch indices. One launch on the current stream for all
    planes (none when r0 == r1); eager only, never inside graph capture.
    A violated precondition raises before anything is launched."""
    dst_planes, src_planes = list(dst_planes), list(src_planes)
    if dst_planes and dst_planes[0].is_cuda:
        _native().kv_copy_rows(dst_planes, int(dst_b), src_planes,
                               int(src_b), int(r0), int(r1))
        return
    ref.kv_copy_rows(dst_planes, int(dst_b), src_planes, int(src_b),
                     int(r0), int(r1))


def dequant_mxfp4(w: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """MXFP4 row-major (nibbles [N, K/2] + e8m0 [N, K/32]) -> bf16."""
    if w.is_cuda and has_native():
        out = torch.empty(w.shape[0], w.shape[1] * 2, dtype=torch.bfloat16,
                          device=w.device)
        _native().dequant_mxfp4(w, scales, out)
        return out
    return ref.dequant_mxfp4(w, scales)


def attn_decode_partials(q, kcache, vcache, pos, scale,
                         kscale=None, vscale=None) -> torch.Tensor:
    """Local flash-decode partials [B, Hq, splits, Dv+2] f32 over THIS
    cache shard — the combinable form for context-parallel attention
    (combine with ``attn_combine`` after gathering shards)."""
    if q.is_cuda:
        B, Hq, _ = q.shape
        dv = vcache.shape[-1]
        splits = _attn_splits(B, kcache.shape[1], kcache.shape[2])
        partials = torch.zeros(B, Hq, splits, dv + 2, dtype=torch.float32,
                               device=q.device)
        partials[..., dv] = -1e30   # empty shards stay neutral in combine
        out = torch.empty(B, Hq, dv, dtype=q.dtype, device=q.device)
        _native().attn_decode(q, kcache, vcache, pos, out, scale, 0, None,
                              kscale, vscale, partials.view(-1), splits,
                              False)
        return partials
    return ref.attn_decode_partials(q, kcache, vcache, pos, scale,
                                    kscale, vscale)


def attn_combine(partials: torch.Tensor,
                 sinks: torch.Tensor | None = None) -> torch.Tensor:
    """partials [B, Hq, S, Dv+2] -> out [B, Hq, Dv]."""
    if partials.is_cuda:
        B, Hq, S, W = partials.shape
        out = torch.empty(B, Hq, W - 2, dtype=torch.bfloat16,
                          device=partials.device)
        _native().attn_combine(partials.contiguous().view(-1), sinks, out, S)
        return out
    return ref.attn_combine(partials, sinks)

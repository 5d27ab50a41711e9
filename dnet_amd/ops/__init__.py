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


def gemm_rows_supported(M: int, N: int, K: int, group: int, bits: int,
                        packed: bool) -> bool:
    """Can gemm_rows (the fused-dequant MFMA prefill GEMM, M > 64) take
    this call? Needs the native library, the packed MFMA weight layout,
    int8 with K % 64 == 0 and group % 64 == 0 or int4 with K % 128 == 0
    and group % 128 == 0 (group dividing K), and more than 64 rows: up to
    64 the decode GEMM is the kernel."""
    if not (packed and bits in (8, 4) and has_native()):
        return False
    align = 64 if bits == 8 else 128
    return (M > 64 and N > 0 and K > 0 and group > 0 and K % align == 0
            and group % align == 0 and K % group == 0)


def gemm_rows(x: torch.Tensor, w: torch.Tensor, scales: torch.Tensor,
              group: int, bias: torch.Tensor | None = None,
              bits: int = 8) -> torch.Tensor:
    """out[M, N] = x[M, K] @ W[N, K]^T (+ bias) for bf16 CUDA x with more
    than 64 rows, W int8 (pack_int8_mfma) or int4 (pack_int4_mfma) with
    bf16 group scales [N, K/group]. Multiplies from the packed bytes
    (weights enter as bf16(q*s), f32 accumulation, one bf16 rounding, K
    never split): a row's bits depend on that row alone."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2):
        raise ValueError("gemm_rows: x must be a 2-D bf16 CUDA tensor")
    if bits not in (8, 4):
        raise ValueError(f"gemm_rows: bits must be 8 or 4, got {bits}")
    M, K = x.shape
    if not (w.dim() == 2 and scales.dim() == 2 and w.device == x.device
            and scales.device == x.device):
        raise ValueError("gemm_rows: w and scales are 2-D, on x's device")
    N = w.shape[0]
    if w.dtype != (torch.int8 if bits == 8 else torch.uint8) \
            or w.shape[1] != (K if bits == 8 else K // 2):
        raise ValueError("gemm_rows: w must be packed int8 [N, K] "
                         "(bits=8) or packed uint8 [N, K/2] (bits=4)")
    if not gemm_rows_supported(M, N, K, group, bits, True):
        _native()     # a missing library is reported as such
        raise ValueError(
            f"gemm_rows: unsupported call M={M} N={N} K={K} group={group} "
            f"bits={bits} (M > 64; int8 K, group % 64; int4 K, group % 128)")
    if scales.dtype != torch.bfloat16 or tuple(scales.shape) != (N, K // group):
        raise ValueError("gemm_rows: scales must be bf16 [N, K/group]")
    if bias is not None and not (bias.dtype == torch.bfloat16
                                 and bias.numel() == N
                                 and bias.device == x.device):
        raise ValueError("gemm_rows: bias must be bf16 [N] on x's device")
    out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _native().gemm_rows(x.contiguous(), w.contiguous(), scales.contiguous(),
                        None if bias is None else bias.contiguous(), out,
                        group, bits)
    return out


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


def mla_decode_supported(lora: int, rope: int) -> bool:
    """Latent dims the HIP mla_decode kernel serves (every released
    DeepSeek-V2/V3 checkpoint: kv_lora_rank 512, qk_rope_head_dim 64)."""
    return (lora, rope) == (512, 64)


def _mla_splits(b: int, nh: int, smax: int) -> int:
    # B x head-tile groups is a handful of blocks (16 for V2-Lite at batch
    # 16), so split until ~512 blocks (2 per CU: a block holds 73 KB of
    # LDS) while a split still owns two 64-position chunks of capacity
    groups = -(-nh // 64)
    splits = 1
    while b * groups * splits * 2 <= 512 and splits * 2 <= smax // 128:
        splits *= 2
    return splits


def mla_decode(q_lat: torch.Tensor, q_pe: torch.Tensor, ckv: torch.Tensor,
               kpe: torch.Tensor, lens: torch.Tensor, scale: float,
               splits: int | None = None) -> torch.Tensor:
    """Absorbed-MLA decode attention over the latent cache.

    q_lat [B,nh,512] (query folded through W_k), q_pe [B,nh,64] (roped),
    ckv [B,S,512], kpe [B,S,64] bf16 (rows contiguous, any batch stride:
    ``MLAKVCache`` planes and their ``slot()`` views), lens [B] int32 ->
    o_lat [B,nh,512] = softmax(scale * (q_lat.ckv^T + q_pe.kpe^T))[:len]
    @ ckv[:len]. Rows >= len are never read; len 0 gives zeros. ``splits``
    (split-S factor) defaults to a heuristic over (B, nh, S)."""
    if q_lat.is_cuda:
        B, nh, lora = q_lat.shape
        if splits is None:
            splits = _mla_splits(B, nh, ckv.shape[1])
        out = torch.empty(B, nh, lora, dtype=q_lat.dtype, device=q_lat.device)
        partials = None
        if splits > 1:
            partials = torch.empty(B * nh * splits * (lora + 2),
                                   dtype=torch.float32, device=q_lat.device)
        _native().mla_decode(q_lat.contiguous(), q_pe.contiguous(), ckv, kpe,
                             lens, out, float(scale), partials, int(splits))
        return out
    return ref.mla_decode(q_lat, q_pe, ckv, kpe, lens, scale)


def mla_prefill_supported(lora: int, rope: int) -> bool:
    """Latent dims the HIP mla_prefill kernel serves (those of
    mla_decode)."""
    return (lora, rope) == (512, 64)


def _mla_prefill_splits(b: int, t: int, nh: int, n: int) -> int:
    # a block holds 4 (token, 16-head tile) items and 73 KB of LDS: split
    # until ~512 blocks (2 per CU, as _mla_splits) while a split still owns
    # two 64-position chunks of the n = q_off + T attended rows
    groups = -(-(t * -(-nh // 16)) // 4)
    chunks = -(-n // 64)
    splits = 1
    while b * groups * splits * 2 <= 512 and splits * 2 <= chunks // 2:
        splits *= 2
    return splits


def mla_prefill(q_lat: torch.Tensor, q_pe: torch.Tensor, ckv: torch.Tensor,
                kpe: torch.Tensor, q_off: int, scale: float,
                splits: int | None = None) -> torch.Tensor:
    """Absorbed-MLA continuation-prefill attention over the latent cache,
    read in place.

    q_lat [B,T,nh,512] (queries folded through W_k), q_pe [B,T,nh,64]
    (roped), ckv [B,S,512], kpe [B,S,64] bf16 (rows contiguous, any
    16-byte-aligned batch stride: ``MLAKVCache`` planes and their
    ``slot()`` views) -> o_lat [B,T,nh,512]; token t sits at position
    q_off + t and attends rows [0, q_off + t + 1), which must already hold
    the chunk's own latents. Rows >= q_off + T are never read. ``splits``
    (split-S factor) defaults to a heuristic over (B, T, nh, q_off + T).
    Eager only (q_off is a host int)."""
    if q_lat.is_cuda:
        B, T, nh, lora = q_lat.shape
        if splits is None:
            splits = _mla_prefill_splits(B, T, nh, int(q_off) + T)
        out = torch.empty(B, T, nh, lora, dtype=q_lat.dtype,
                          device=q_lat.device)
        partials = None
        if splits > 1:
            partials = torch.empty(B * T * nh * splits * (lora + 2),
                                   dtype=torch.float32, device=q_lat.device)
        _native().mla_prefill(q_lat.contiguous(), q_pe.contiguous(), ckv, kpe,
                              out, int(q_off), float(scale), partials,
                              int(splits))
        return out
    return ref.mla_prefill(q_lat, q_pe, ckv, kpe, int(q_off), scale)


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


_PREFILL_KV_DIMS = {(128, 128), (64, 64), (96, 96)}


def attn_prefill_kv_supported(d: int, dv: int, int8: bool) -> bool:
    """Head dims the in-place prefill pair (rope_append_rows +
    attn_prefill_kv) serves; an int8 cache needs whole 64-dim groups."""
    return (d, dv) in _PREFILL_KV_DIMS and not (int8 and d % 64)


def rope_append_rows(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     kcache: torch.Tensor, vcache: torch.Tensor, p0: int,
                     cos: torch.Tensor, sin: torch.Tensor,
                     kscale: torch.Tensor | None = None,
                     vscale: torch.Tensor | None = None) -> torch.Tensor:
    """Fused prefill RoPE + KV append. q [B,T,Hq,D], k/v [B,T,Hkv,D] bf16
    (column slices of the fused qkv buffer are fine: head stride D, any
    token/batch stride); token t sits at position p0+t. Rotated k and raw
    v go to rows [p0, p0+T) of kcache/vcache [B,Hkv,Smax,D] (bf16, or int8
    with bf16 scales [B,Hkv,Smax,D/64]; any batch stride); no other row is
    written. Returns the rotated q as [B,Hq,T,D], the layout
    ``attn_prefill_kv`` reads. Eager only (p0 is a host int)."""
    if q.is_cuda:
        B, T, Hq, D = q.shape
        q_rot = torch.empty(B, Hq, T, D, dtype=q.dtype, device=q.device)
        _native().rope_append_rows(q, k, v, q_rot, kcache, vcache, int(p0),
                                   cos, sin, kscale, vscale)
        return q_rot
    return ref.rope_append_rows(q, k, v, kcache, vcache, int(p0), cos, sin,
                                kscale, vscale)


def attn_prefill_kv(q: torch.Tensor, kcache: torch.Tensor,
                    vcache: torch.Tensor, kv_len: int, scale: float,
                    q_off: int, window: int = 0,
                    sinks: torch.Tensor | None = None,
                    kscale: torch.Tensor | None = None,
                    vscale: torch.Tensor | None = None) -> torch.Tensor:
    """Flash prefill attention that reads the KV cache in place (bf16 or
    int8 + scales, strides as ``KVCache.slot()`` hands them out): the
    semantics of ``attn_prefill`` on ``cache[:, :, :kv_len]`` (rows
    >= kv_len are never read). q [B,Hq,T,D] contiguous -> [B, T, Hq*Dv],
    token-major for the o-projection. A query row's output bits do not
    depend on how the prompt was chunked."""
    if q.is_cuda:
        B, Hq, T, _ = q.shape
        out = torch.empty(B, T, Hq * vcache.shape[-1], dtype=q.dtype,
                          device=q.device)
        _native().attn_prefill_kv(q, kcache, vcache, sinks, out, int(kv_len),
                                  int(q_off), int(window or 0), float(scale),
                                  kscale, vscale)
        return out
    return ref.attn_prefill_kv(q, kcache, vcache, int(kv_len), scale,
                               int(q_off), window or 0, sinks, kscale, vscale)


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
    (bf16 or grouped-int8; uint8 nibbles [E,2I,K/2] with e8m0 uint8 scales
    = mxfp4, with bf16 group scales = int4, which on the GPU takes the
    MFMA kernels of moe_int4.hip.cpp and needs ``packed``, the
    pack_int4_mfma layout, and M <= 64), we [M,E] f32 routing weights ->
    act [E,M,I]. Experts with all-zero we are skipped on GPU (their act
    rows hold garbage; moe_down never reads them)."""
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
        # the int4 kernels store every element; the others accumulate
        int4 = w.dtype == torch.uint8 and scales.dtype == torch.bfloat16
        out = (torch.empty if int4 else torch.zeros)(
            act.shape[1], w.shape[1], dtype=torch.float32, device=act.device)
        _native().moe_down(act, w, scales, bias, we, out, group, packed)
        return out
    return ref.moe_down(act, w, scales, bias, we, group, packed)


def moe_int4_supported(K: int, I: int, H: int, group: int,
                       packed: bool) -> bool:
    """Should the models send an int4 expert bank (gate/up [E,2I,K/2],
    down [E,H,I/2], bf16 scales) with T <= 64 rows through moe_gateup /
    moe_down on the GPU? The MFMA kernels take the pack_int4_mfma layout
    with K, I and the group multiples of 128 and H a multiple of 16."""
    if not packed or group <= 0 or group % 128:
        return False
    return not (K % 128 or I % 128 or K % group or I % group or H % 16)


def moe_int4_force_ks(ks: int) -> None:
    """Waves per column strip in the int4 MoE kernels: 0 picks by shape,
    1 or 4 forces it (M > 32 always runs 1). Process-wide; for benchmarks
    and tests."""
    _native().moe_int4_force_ks(ks)


def moe_rows_supported(w: torch.Tensor, K: int, I: int, H: int, group: int,
                       packed: bool) -> bool:
    """Should the models send a stacked expert bank ``w`` through the
    token-routed MFMA path (moe_route / moe_gateup_rows / moe_down_rows)?
    True for mxfp4 banks (uint8 nibble rows, e8m0 scales, block 32) with
    every dim a multiple of 64.

    The kernels also run bf16 banks and int8 banks in the pack_int8_mfma
    layout (group % 64 == 0), and the ops accept them, but at 8192 rows
    they measured 2-3x slower than the per-expert loop (docs/KERNELS.md,
    "MoE rows"), so those formats stay on the loop, as does unpacked int8,
    which the kernels do not serve at all. Grouped int4 (also uint8, bf16
    scales, group % 128 == 0) is not this predicate's business: it has
    kernels of its own behind the same ops, see moe_rows_int4_supported."""
    if K % 64 or I % 64 or H % 64:
        return False
    return bool(w.dtype == torch.uint8 and group == 32 and not packed)


def moe_rows_int4_supported(K: int, I: int, H: int, group: int,
                            packed: bool) -> bool:
    """Do moe_gateup_rows / moe_down_rows serve an int4 expert bank (gate/up
    [E,2I,K/2], down [E,H,I/2], bf16 group scales) on the GPU? The kernels
    of moe_rows_int4.hip.cpp take the pack_int4_mfma layout with K, I and
    the group multiples of 128, the group dividing K and I, and H a
    multiple of 64. Whether the models use them by default is their
    decision (models/moe.py, int4_rows)."""
    if not packed or group <= 0 or group % 128:
        return False
    return not (K % 128 or I % 128 or K % group or I % group or H % 64)


def _is_int4_bank(w: torch.Tensor, scales) -> bool:
    return (w.dtype == torch.uint8 and scales is not None
            and scales.dtype == torch.bfloat16)


def moe_route(we: torch.Tensor, topk: int) -> dict:
    """Sort the routed (token, expert) pairs of dense routing weights
    we [T, E] f32 by expert. (t, e) is routed iff we[t, e] != 0; ``topk``
    (host int) bounds the non-zeros per row, rows may hold fewer or none.
    Routed pairs get consecutive slots, experts ascending and tokens
    ascending inside an expert. Returns a plan of int32 device tensors and
    host-known capacities:

    counts [E], offsets [E+1]   expert e owns slots offsets[e]:offsets[e+1]
    slot_token [slots_cap]      slot -> token, -1 past the live slots
    token_slots [T, topk]       token -> its slots, e ascending, then -1
    tiles [tiles_cap, 3]        (expert, first slot, rows <= 64) per GEMM
                                tile, live ones first; zeros after
    ntiles [1]                  number of live tiles
    T, E, topk, slots_cap, tiles_cap   host ints

    Two launches, no host sync, no atomics; the plan is a function of
    ``we != 0`` alone."""
    if not we.is_cuda:
        return ref.moe_route(we, int(topk))
    T, E = we.shape
    topk = int(topk)
    slots_cap, tiles_cap = ref.moe_plan_caps(T, E, topk)
    i32 = dict(dtype=torch.int32, device=we.device)
    plan = {"counts": torch.empty(E, **i32),
            "offsets": torch.empty(E + 1, **i32),
            "slot_token": torch.empty(slots_cap, **i32),
            "token_slots": torch.empty(T, topk, **i32),
            "tiles": torch.empty(tiles_cap, 3, **i32),
            "ntiles": torch.empty(1, **i32), "T": T, "E": E, "topk": topk,
            "slots_cap": slots_cap, "tiles_cap": tiles_cap}
    blockcnt = torch.empty(-(-T // 256) * E, **i32)
    _native().moe_route(we.contiguous(), blockcnt, plan["counts"],
                        plan["offsets"], plan["slot_token"],
                        plan["token_slots"], plan["tiles"], plan["ntiles"],
                        topk)
    return plan


def moe_gateup_rows(x: torch.Tensor, gw: torch.Tensor, gs, gb, plan: dict,
                    group: int = 0, packed: bool = False, glu: int = 0,
                    alpha: float = 1.702, limit: float = 7.0) -> torch.Tensor:
    """Routed gate+up with fused GLU: x [T,K] bf16, stacked gw [E,2I,K]
    -> act [slots_cap, I] bf16, compact in the plan's slot order:
    act[slot] = glu(x[t] . Wg[e]^T + bg, x[t] . Wu[e]^T + bu). Rows past
    the live slots are never written (nor read by moe_down_rows). A slot's
    bits depend on its own token only. A uint8 bank with bf16 scales is
    int4 (uint8 scales: mxfp4) and runs the 128-row kernels of
    moe_rows_int4.hip.cpp, which need ``packed`` and the dims of
    moe_rows_int4_supported."""
    if x.is_cuda:
        act = torch.empty(plan["slots_cap"], gw.shape[1] // 2,
                          dtype=torch.bfloat16, device=x.device)
        if _is_int4_bank(gw, gs):
            _native().moe_rows_int4_gateup(
                x, gw, gs, gb, plan["slot_token"], plan["offsets"],
                plan["tiles"], plan["ntiles"], act, group, packed, glu,
                alpha, limit)
            return act
        _native().moe_rows_gateup(x, gw, gs, gb, plan["slot_token"],
                                  plan["tiles"], plan["ntiles"], act, group,
                                  packed, glu, alpha, limit)
        return act
    return ref.moe_gateup_rows(x, gw, gs, gb, plan, group, packed, glu,
                               alpha, limit)


def moe_down_rows(act: torch.Tensor, dw: torch.Tensor, ds, db,
                  we: torch.Tensor, plan: dict, group: int = 0,
                  packed: bool = False) -> torch.Tensor:
    """Routed down projection and combine: act [slots_cap, I], stacked dw
    [E,H,I], we [T,E] (the weights the plan was made from) -> out [T,H]
    f32, out[t] = sum_e we[t,e] * (act[slot(t,e)] . Wd[e]^T + bd[e]) over
    the token's slots in ascending-e order; exact zeros for a token with
    no routed expert. Fixed summation order, no atomics. int4 banks
    (uint8 with bf16 scales) take the kernels of moe_rows_int4.hip.cpp,
    as in moe_gateup_rows."""
    if act.is_cuda:
        H = dw.shape[1]
        y = torch.empty(plan["slots_cap"], H, dtype=torch.float32,
                        device=act.device)
        out = torch.empty(plan["T"], H, dtype=torch.float32,
                          device=act.device)
        if _is_int4_bank(dw, ds):
            _native().moe_rows_int4_down(
                act, dw, ds, db, we.contiguous(), plan["slot_token"],
                plan["token_slots"], plan["offsets"], plan["tiles"],
                plan["ntiles"], y, out, group, packed)
            return out
        _native().moe_rows_down(act, dw, ds, db, we.contiguous(),
                                plan["slot_token"], plan["token_slots"],
                                plan["tiles"], plan["ntiles"], y, out, group,
                                packed)
        return out
    return ref.moe_down_rows(act, dw, ds, db, we, plan, group, packed)


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

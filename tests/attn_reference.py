"""fp64 references and derived error bounds for the attention, RoPE and
KV-append kernels (helper for tests/test_attention_gpu.py; not a test
module).

Everything here is plain torch: inputs (bf16 / int8 / f32, on any device)
are moved to the CPU and evaluated in float64, so the reference's own
error is negligible next to one bf16 rounding.

Run as a script it replays the decode case matrix in a fresh process
(``python tests/attn_reference.py --decode-cases``): the decode kernel
variant is chosen by ``DNET_ATTN_MFMA`` once per process, so the MFMA
variant can only be exercised from a child.
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import sys

import torch

F64 = torch.float64


# ---------------------------------------------------------------- attention

def _dequant_kv64(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """int8 g64 KV -> fp64, rounding through bf16 exactly where the kernel
    does (it stages bf16(code * scale) into LDS). code * scale is exact in
    f32 (8 x 8 significant bits)."""
    *lead, d = codes.shape
    x = codes.float().view(*lead, d // 64, 64) * scales.float().unsqueeze(-1)
    return x.view(*lead, d).to(torch.bfloat16).to(F64)


def attn_ref(q, k, v, lens, scale, window, sinks, q_off=None, kscale=None,
             vscale=None):
    """Masked softmax attention in fp64 with the kernels' semantics.

    Decode (``q_off is None``): q [B,Hq,D], k/v [B,Hkv,S,D(v)], lens [B];
    row b attends positions [max(0, len-window), len) (window 0 = all).
    Prefill: q [B,Hq,T,D]; query t attends s <= q_off+t and
    s > q_off+t-window (lens ignored; all S rows are valid).
    ``sinks`` [Hq]: one extra logit per head whose mass is dropped.
    Rows outside the attended range are never read, so they may hold NaN.
    Returns (out, out_abs) in fp64; out_abs is the same attention applied
    to |V|. A query with nothing to attend gives zeros.
    """
    decode = q_off is None
    q = q.detach().cpu()
    k = k.detach().cpu()
    v = v.detach().cpu()
    if decode:
        q = q.unsqueeze(2)
    B, Hq, T, D = q.shape
    Hkv, S, DV = k.shape[1], k.shape[2], v.shape[-1]
    G = Hq // Hkv
    sk = None if sinks is None else sinks.detach().cpu().to(F64).view(Hkv, G, 1)
    out = torch.zeros(B, Hq, T, DV, dtype=F64)
    out_abs = torch.zeros_like(out)
    for b in range(B):
        if decode:
            ln = int(lens[b])
            qpos = torch.tensor([ln - 1])
            hi = ln
        else:
            qpos = q_off + torch.arange(T)
            hi = min(S, q_off + T)
        lo = max(0, int(qpos[0]) - window + 1) if window > 0 else 0
        if hi <= lo:
            continue
        if kscale is not None:
            kb = _dequant_kv64(k[b, :, lo:hi], kscale.detach().cpu()[b, :, lo:hi])
            vb = _dequant_kv64(v[b, :, lo:hi], vscale.detach().cpu()[b, :, lo:hi])
        else:
            kb = k[b, :, lo:hi].to(F64)
            vb = v[b, :, lo:hi].to(F64)
        spos = torch.arange(lo, hi).view(1, -1)
        live = spos <= qpos.view(-1, 1)
        if window > 0:
            live &= spos > qpos.view(-1, 1) - window
        qb = q[b].to(F64).view(Hkv, G, T, D)
        s = torch.einsum("hgtd,hsd->hgts", qb, kb) * float(scale)
        s = s.masked_fill(~live.view(1, 1, T, -1), float("-inf"))
        m = s.amax(dim=-1)
        if sk is not None:
            m = torch.maximum(m, sk)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        p = torch.exp(s - m.unsqueeze(-1))
        denom = p.sum(-1)
        if sk is not None:
            denom = denom + torch.exp(sk - m)
        w = torch.where(denom > 0, 1.0 / denom, torch.zeros_like(denom))
        p = p * w.unsqueeze(-1)
        out[b] = torch.einsum("hgts,hsd->hgtd", p, vb).reshape(Hq, T, DV)
        out_abs[b] = torch.einsum("hgts,hsd->hgtd", p,
                                  vb.abs()).reshape(Hq, T, DV)
    if decode:
        return out[:, :, 0], out_abs[:, :, 0]
    return out, out_abs


def attn_tol(out: torch.Tensor, out_abs: torch.Tensor) -> torch.Tensor:
    """Elementwise bound on |kernel - fp64| for a bf16-output attention
    kernel: 2^-8 * (|out| + out_abs).

    bf16 keeps 8 significant bits, so one round-to-nearest costs at most
    2^-8 relative (half an ulp at the bottom of a binade, 2^-9 at the
    top). The output is rounded to bf16: <= 2^-8 |out|, which is at most
    half the bound because out_abs >= |out|. The MFMA kernels round P to
    bf16 before PV: each weight moves by <= 2^-8 p, so the sum moves by
    <= 2^-8 * sum p|v| = 2^-8 out_abs, and only if every rounding error
    lines up with the sign of its v. f32 accumulation over <= 2048
    positions and __expf are orders of magnitude below either term. A CPU
    simulation of the tiled bf16-P, f32-accumulate algorithm (L = 1..2048,
    D = 64..192, with and without sinks) peaked at 0.59 of the bound."""
    return 2.0 ** -8 * (out.abs() + out_abs)


def worst_ratio(got: torch.Tensor, out: torch.Tensor,
                out_abs: torch.Tensor) -> float:
    """max |got - out| / attn_tol over all elements (nan/inf -> inf; an
    element with zero tolerance must match exactly)."""
    got = got.detach().cpu().to(F64)
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - out).abs()
    tol = attn_tol(out, out_abs)
    ratio = torch.where(tol > 0, err / tol,
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


# --------------------------------------------------------------------- rope

def rope_ref(x, cos, sin, pos):
    """fp64 neox rotation of x [B,H,D] at table rows pos [B].
    Returns (rotated, mag): mag = |x1 c| + |x2 s| (first half) and
    |x2 c| + |x1 s| (second half), the magnitude the two products had
    before they cancelled."""
    x = x.detach().cpu().to(F64)
    half = x.shape[-1] // 2
    idx = pos.detach().cpu().long()
    c = cos.detach().cpu().to(F64)[idx].unsqueeze(1)
    s = sin.detach().cpu().to(F64)[idx].unsqueeze(1)
    x1, x2 = x[..., :half], x[..., half:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                     (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return rot, mag


def rope_tol(rot: torch.Tensor, mag: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp (2^-7 relative at worst: round-to-nearest plus an
    fma-contraction flip next to a rounding boundary) plus the f32
    cancellation floor."""
    return 2.0 ** -7 * rot.abs() + 2.0 ** -16 * mag


def check_kv8(codes, scales, x_true) -> None:
    """Contract of the int8 group-64 KV cache, independent of
    ref.quantize_kv_rows. For every 64-wide group:
      |scale - amax/127| <= 2^-8 * amax/127   (one bf16 round-to-nearest)
      |code * scale - x| <= 0.51 * scale      (round-to-nearest gives 0.5;
                                               the clamp costs at most 0.25
                                               when the scale rounded down)
      |code| <= 127
    """
    codes = codes.detach().cpu()
    *lead, d = codes.shape
    ng = d // 64
    x = x_true.detach().cpu().to(F64).reshape(*lead, ng, 64)
    c = codes.to(F64).view(*lead, ng, 64)
    sc = scales.detach().cpu().to(F64).reshape(*lead, ng)
    ideal = x.abs().amax(dim=-1).clamp_min(1e-8) / 127.0
    assert torch.isfinite(sc).all(), "non-finite scale"
    bad = (sc - ideal).abs() > 2.0 ** -8 * ideal
    assert not bad.any(), (
        f"scale off: got {sc[bad][:4].tolist()} want {ideal[bad][:4].tolist()}")
    assert int(c.abs().max()) <= 127, "code out of [-127, 127]"
    err = (c * sc.unsqueeze(-1) - x).abs()
    lim = 0.51 * sc.unsqueeze(-1)
    assert (err <= lim).all(), (
        f"dequant error {float((err / lim).max()):.3f} x the 0.51*scale bound")


# ------------------------------------------------------- decode case matrix

DECODE_DIMS = [(64, 64, 16, 1), (128, 128, 10, 2), (128, 128, 2, 2),
               (192, 128, 3, 1)]          # (D, DV, Hq, Hkv): G = 16, 5, 1, 3
DECODE_SPLITS = [1, 2, 4, 8]              # 8 > nchunks at Smax=320
DECODE_POS = [(0, 1, 63), (64, 65, 320), (129, 7, 200)]
DECODE_WINDOWS = [0, 1, 48, 64, 200]
SINK_KINDS = ["none", "randn", "big", "small"]
DECODE_SMAX = 320


def pairwise(axes, seed_rows=()):
    """Greedy all-pairs cover of the cartesian product of ``axes`` (lists
    of values): every pair of values of two different axes appears in at
    least one row. Deterministic. ``seed_rows`` count as already chosen."""
    n = len(axes)
    need = set()
    for i, j in itertools.combinations(range(n), 2):
        for a in range(len(axes[i])):
            for b in range(len(axes[j])):
                need.add((i, a, j, b))

    def pairs(row):
        return {(i, row[i], j, row[j])
                for i, j in itertools.combinations(range(n), 2)}

    for r in seed_rows:
        need -= pairs(r)
    rows = []
    cand = list(itertools.product(*[range(len(a)) for a in axes]))
    while need:
        best = max(cand, key=lambda r: len(pairs(r) & need))
        rows.append(best)
        need -= pairs(best)
    return rows


def decode_cases():
    """The attn_decode matrix: ~65 cases covering all pairs of (dims,
    int8, splits, pos, window, sinks), with every sinks x window
    combination present on an int8 cache at splits > 1."""
    axes = [DECODE_DIMS, [False, True], DECODE_SPLITS, DECODE_POS,
            DECODE_WINDOWS, SINK_KINDS]
    rows = []
    # splits x lengths x window is the triple the chunk loop depends on:
    # keep it whole (60 rows) and rotate the other axes over it so that,
    # per window, the nine splits > 1 rows hold all four sink kinds on an
    # int8 cache
    for wi, si, pi in itertools.product(range(len(DECODE_WINDOWS)),
                                        range(len(DECODE_SPLITS)),
                                        range(len(DECODE_POS))):
        if si == 0:
            kind, q8, dims = (pi + wi) % 4, pi % 2, (pi + wi) % 4
        else:
            idx = (si - 1) * 3 + pi                     # 0..8
            kind = (idx + wi) % 4
            q8 = 1 if (idx // 4) % 2 == 0 else 0        # idx 0-3 and 8
            dims = (idx + wi + idx // 4) % 4
        rows.append((dims, q8, si, pi, wi, kind))
    rows += pairwise(axes, rows)
    cases = [dict(dims=DECODE_DIMS[d], int8=bool(q), splits=DECODE_SPLITS[s],
                  pos=DECODE_POS[p], window=DECODE_WINDOWS[w],
                  sinks=SINK_KINDS[k], smax=DECODE_SMAX)
             for d, q, s, p, w, k in rows]
    # window start exactly on a chunk boundary (129 - 65 = 64), and windows
    # that skip whole chunks so split 0's first chunk is not chunk 0
    for splits, q8 in ((2, False), (4, True)):
        cases.append(dict(dims=DECODE_DIMS[1], int8=q8, splits=splits,
                          pos=(129, 7, 200), window=65, sinks="randn",
                          smax=DECODE_SMAX))
    cases.append(dict(dims=DECODE_DIMS[0], int8=False, splits=2,
                      pos=(320, 193, 130), window=64, sinks="none",
                      smax=DECODE_SMAX))
    for i, c in enumerate(cases):
        c["seed"] = 1000 + i
    return cases


# B=1, Hkv=1, Smax=1024: _attn_splits picks 2 with DNET_ATTN_SPLITS unset
NATURAL_CASE = dict(dims=(128, 128, 8, 1), int8=False, splits=None,
                    pos=(1000,), window=0, sinks="none", smax=1024, seed=999)


def case_id(c) -> str:
    d, dv, hq, hkv = c["dims"]
    return (f"d{d}v{dv}h{hq}k{hkv}-{'i8' if c['int8'] else 'bf16'}"
            f"-s{c['splits']}-p{'_'.join(map(str, c['pos']))}"
            f"-w{c['window']}-{c['sinks']}")


def make_sinks(kind: str, hq: int, gen) -> torch.Tensor | None:
    if kind == "none":
        return None
    if kind == "randn":
        return torch.randn(hq, generator=gen).to(torch.bfloat16)
    return torch.full((hq,), 30.0 if kind == "big" else -30.0,
                      dtype=torch.bfloat16)


def build_decode_inputs(c, device):
    """Inputs of one decode case, generated on the CPU from the case's own
    seed (identical in every process), then moved to ``device``.

    Rows >= len are poisoned: NaN in a bf16 cache; in an int8 cache the
    codes stay random and the scales are NaN. Rows below the window start
    hold finite garbage of magnitude 1e4. (They cannot hold NaN: the
    scalar kernel walks every staged row s < valid of the window's first
    chunk and multiplies V by an exact-zero weight for rows below the
    start, so NaN there would reach the output. That is a known limit of
    the kernel, not tested here.)
    q is the leading column slice of a wider fused-QKV buffer, as in
    production (row stride (Hq + 2 Hkv) * D)."""
    D, DV, Hq, Hkv = c["dims"]
    B, S, window = len(c["pos"]), c["smax"], c["window"]
    gen = torch.Generator().manual_seed(c["seed"])
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=gen).to(torch.bfloat16)
    k = torch.randn(B, Hkv, S, D, generator=gen)
    v = torch.randn(B, Hkv, S, DV, generator=gen)
    sinks = make_sinks(c["sinks"], Hq, gen)
    for b, ln in enumerate(c["pos"]):
        start = max(0, ln - window) if window > 0 else 0
        k[b, :, :start] *= 1e4
        v[b, :, :start] *= 1e4
    k, v = k.to(torch.bfloat16), v.to(torch.bfloat16)
    ks = vs = None
    if c["int8"]:
        from dnet_amd.ops import reference as ref
        k, ks = ref.quantize_kv_rows(k)
        v, vs = ref.quantize_kv_rows(v)
        for b, ln in enumerate(c["pos"]):
            ks[b, :, ln:] = float("nan")
            vs[b, :, ln:] = float("nan")
        ks, vs = ks.to(device), vs.to(device)
    else:
        for b, ln in enumerate(c["pos"]):
            k[b, :, ln:] = float("nan")
            v[b, :, ln:] = float("nan")
    qkv = qkv.to(device)
    q = qkv[:, :Hq * D].view(B, Hq, D)
    assert B == 1 or q.stride(0) == (Hq + 2 * Hkv) * D
    pos = torch.tensor(c["pos"], dtype=torch.int32, device=device)
    if sinks is not None:
        sinks = sinks.to(device)
    return dict(q=q, k=k.to(device), v=v.to(device), pos=pos, sinks=sinks,
                kscale=ks, vscale=vs, scale=D ** -0.5, window=window)


def run_decode_case(c, device):
    """ops.attn_decode on one case -> (worst err/tol, out, ref). The
    caller sets DNET_ATTN_SPLITS (c["splits"]; unset for None)."""
    import dnet_amd.ops as ops
    x = build_decode_inputs(c, device)
    got = ops.attn_decode(x["q"], x["k"], x["v"], x["pos"], x["scale"],
                          x["window"], x["sinks"], x["kscale"], x["vscale"])
    out, out_abs = attn_ref(x["q"], x["k"], x["v"], x["pos"], x["scale"],
                            x["window"], x["sinks"], kscale=x["kscale"],
                            vscale=x["vscale"])
    return worst_ratio(got, out, out_abs), got, out


def checksum(t: torch.Tensor) -> str:
    """sha256 of the raw bf16 bits."""
    raw = t.detach().cpu().contiguous().view(torch.int16).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def _set_splits(splits) -> None:
    if splits is None:
        os.environ.pop("DNET_ATTN_SPLITS", None)
    else:
        os.environ["DNET_ATTN_SPLITS"] = str(splits)


def main_decode_cases() -> int:
    """Replay the decode matrix on cuda in this process; one JSON line per
    case, then the output checksum of the natural-splits case."""
    for c in decode_cases() + [NATURAL_CASE]:
        _set_splits(c["splits"])
        ratio, got, _ = run_decode_case(c, "cuda")
        torch.cuda.synchronize()
        line = {"case": case_id(c), "ratio": ratio}
        if c is NATURAL_CASE:
            line["checksum"] = checksum(got)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    if "--decode-cases" in sys.argv[1:]:
        sys.exit(main_decode_cases())
    sys.exit("usage: attn_reference.py --decode-cases")

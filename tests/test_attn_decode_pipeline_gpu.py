"""The pipelined schedule of the scalar decode-attention kernel (next chunk
prefetched into registers, one walk over V per wave, P.V dealt over the
waves in (head, 64 dims) units) against the fp64 reference and bound of
tests/attn_reference.py.

Every launch mixes the lengths that move the chunk loop in one batch:
none, one chunk, a chunk boundary minus / plus one, a prefetch that lands
exactly on the last chunk, and len == Smax on the last batch row, where
the last KV head's last cache row is the end of the allocation. Rows >= len
are poisoned (NaN in a bf16 cache, NaN scales in an int8 cache), so a
prefetched or zero-filled row that leaks shows as a non-finite output.
Rows below a window's start hold finite garbage of magnitude 1e4 (the
kernel walks those with an exact-zero weight; see attn_reference).
"""
import pytest
import torch

import attn_reference as ar
import dnet_amd.ops as ops
from dnet_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HKV = 2


def _lens(smax):
    return [0, 1, 63, 64, 65, 127, 128, 129, 192, smax]


def _inputs(d, dv, g, smax, lens, int8, window, sinks, seed):
    """CPU-generated inputs of one launch (q is the leading slice of a
    fused-QKV buffer, as in production)."""
    hq, B = g * HKV, len(lens)
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, (hq + 2 * HKV) * d, generator=gen).to(BF16)
    k = torch.randn(B, HKV, smax, d, generator=gen)
    v = torch.randn(B, HKV, smax, dv, generator=gen)
    sk = ar.make_sinks("randn" if sinks else "none", hq, gen)
    for b, ln in enumerate(lens):
        start = max(0, ln - window) if window > 0 else 0
        k[b, :, :start] *= 1e4
        v[b, :, :start] *= 1e4
    k, v = k.to(BF16), v.to(BF16)
    ks = vs = None
    if int8:
        k, ks = ref.quantize_kv_rows(k)
        v, vs = ref.quantize_kv_rows(v)
        for b, ln in enumerate(lens):
            ks[b, :, ln:] = float("nan")
            vs[b, :, ln:] = float("nan")
    else:
        for b, ln in enumerate(lens):
            k[b, :, ln:] = float("nan")
            v[b, :, ln:] = float("nan")
    return dict(qkv=qkv, k=k, v=v, ks=ks, vs=vs, sinks=sk, hq=hq, d=d,
                lens=list(lens), window=window)


def _run(x):
    """ops.attn_decode on the GPU -> (out, tensors as the kernel saw them)."""
    dev = "cuda"
    qkv = x["qkv"].to(dev)
    q = qkv[:, :x["hq"] * x["d"]].view(len(x["lens"]), x["hq"], x["d"])
    k, v = x["k"].to(dev), x["v"].to(dev)
    ks = None if x["ks"] is None else x["ks"].to(dev)
    vs = None if x["vs"] is None else x["vs"].to(dev)
    sk = None if x["sinks"] is None else x["sinks"].to(dev)
    pos = torch.tensor(x["lens"], dtype=torch.int32, device=dev)
    out = ops.attn_decode(q, k, v, pos, x["d"] ** -0.5, x["window"], sk, ks,
                          vs)
    torch.cuda.synchronize()
    return out, (q, k, v, pos, sk, ks, vs)


def _ratio(x, out, t):
    q, k, v, pos, sk, ks, vs = t
    want, want_abs = ar.attn_ref(q, k, v, pos, x["d"] ** -0.5, x["window"],
                                 sk, kscale=ks, vscale=vs)
    return ar.worst_ratio(out, want, want_abs)


# (D, DV, G, int8, window, sinks, splits, Smax): every value of every axis,
# G = 5 and 16 on each head shape (G = 5 gives the waves 3 and 2 P.V heads
# at DV = 128 and 2, 1, 1, 1 at DV = 64; G = 16 the longest head lists),
# splits = 4 so that len = 65 leaves splits without a chunk, and the
# unpipelined 192-wide body next to the pipelined ones.
CASES = [
    (128, 128, 5, False, 0, False, 2, 192),
    (128, 128, 5, True, 70, True, 1, 256),
    (128, 128, 5, False, 70, True, 4, 256),
    (128, 128, 16, False, 0, True, 1, 192),
    (128, 128, 16, True, 0, False, 4, 256),
    (128, 128, 1, True, 0, False, 2, 192),
    (128, 128, 4, False, 70, False, 1, 256),
    (128, 128, 8, True, 70, True, 2, 192),
    (64, 64, 5, False, 0, True, 4, 192),
    (64, 64, 16, True, 70, False, 2, 256),
    (64, 64, 1, False, 70, True, 1, 192),
    (64, 64, 8, False, 0, False, 1, 256),
    (64, 64, 4, True, 0, True, 2, 256),
    (192, 128, 5, False, 70, False, 2, 256),
    (192, 128, 16, True, 0, True, 1, 192),
    (192, 128, 4, False, 0, True, 4, 192),
    (192, 128, 1, True, 70, False, 4, 256),
    (192, 128, 8, False, 0, False, 2, 192),
]


def _id(c):
    d, dv, g, int8, window, sinks, splits, smax = c
    return (f"d{d}v{dv}g{g}-{'i8' if int8 else 'bf16'}-w{window}"
            f"-{'sinks' if sinks else 'nosinks'}-s{splits}-S{smax}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mixed_lengths_poisoned(case, monkeypatch):
    """Within the fp64 bound, finite despite the poison, exactly zero where
    there is nothing to attend, and the same bits on a second launch."""
    d, dv, g, int8, window, sinks, splits, smax = case
    monkeypatch.setenv("DNET_ATTN_SPLITS", str(splits))
    x = _inputs(d, dv, g, smax, _lens(smax), int8, window, sinks,
                seed=4000 + CASES.index(case))
    out, t = _run(x)
    ratio = _ratio(x, out, t)
    print(f"[err/tol] {_id(case)}: {ratio:.3f}")
    assert torch.isfinite(out.float()).all()
    assert ratio <= 1.0, f"err/tol = {ratio:.3f} > 1"
    assert out[0].float().abs().max().item() == 0.0      # len = 0
    again, _ = _run(x)
    assert torch.equal(out, again)


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("splits", [1, 2])
def test_batch_rows_are_independent(int8, splits, monkeypatch):
    """Another row's length and cache contents do not move a row's bits:
    row 4 goes from 65 positions (prefetch of a one-row chunk) to 192 with
    a fresh cache."""
    monkeypatch.setenv("DNET_ATTN_SPLITS", str(splits))
    smax, lens = 192, _lens(192)
    x = _inputs(128, 128, 5, smax, lens, int8, 0, False, seed=4100)
    base, _ = _run(x)
    lens2 = list(lens)
    lens2[4] = 192
    y = _inputs(128, 128, 5, smax, lens2, int8, 0, False, seed=4101)
    for key in ("k", "v", "ks", "vs"):
        if x[key] is not None:
            x[key][4] = y[key][4]
    x["lens"] = lens2
    moved, t = _run(x)
    keep = [b for b in range(len(lens)) if b != 4]
    assert torch.equal(base[keep], moved[keep])
    assert not torch.equal(base[4], moved[4])
    assert _ratio(x, moved, t) <= 1.0

"""In-place prefill: ops.rope_append_rows and ops.attn_prefill_kv against
the fp64 references and bounds of tests/attn_reference.py, chunk
independence of the attention output, and prefill_window end to end."""
import pytest
import torch

import attn_reference as ar
import dnet_amd.ops as ops
from dnet_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
DIMS = [(64, False), (64, True), (128, False), (128, True), (96, False)]
DIM_IDS = [f"d{d}-{'i8' if q8 else 'bf16'}" for d, q8 in DIMS]


# ------------------------------------------------------- rope_append_rows

@pytest.mark.parametrize("T,p0", [(1, 0), (17, 5), (65, 63)])
@pytest.mark.parametrize("D,int8", DIMS, ids=DIM_IDS)
def test_rope_append_rows_vs_fp64(D, int8, T, p0):
    B, Hq, Hkv, Smax = 2, 4, 2, 160
    gen = torch.Generator().manual_seed(D + 3 * T + p0)
    N = (Hq + 2 * Hkv) * D
    qkv = torch.randn(B, T, N, generator=gen).to(BF16).to(DEV)
    q = qkv[..., :Hq * D].view(B, T, Hq, D)
    k = qkv[..., Hq * D:(Hq + Hkv) * D].view(B, T, Hkv, D)
    v = qkv[..., (Hq + Hkv) * D:].view(B, T, Hkv, D)
    cos, sin = (t.to(DEV) for t in ops.rope_tables(Smax, D, 10000.0))
    # slots 1-2 of a 3-slot cache, everything pre-filled with a sentinel
    if int8:
        planes = [torch.full((3, Hkv, Smax, D), 77, dtype=torch.int8,
                             device=DEV) for _ in range(2)]
        planes += [torch.full((3, Hkv, Smax, D // 64), 7.0, dtype=BF16,
                              device=DEV) for _ in range(2)]
    else:
        planes = [torch.full((3, Hkv, Smax, D), 7.0, dtype=BF16, device=DEV)
                  for _ in range(2)]
    before = [p.clone() for p in planes]
    views = [p[1:3] for p in planes]
    q_rot = ops.rope_append_rows(q, k, v, views[0], views[1], p0, cos, sin,
                                 *views[2:])

    pos = (p0 + torch.arange(T)).repeat(B)

    def rot(x):           # [B,T,H,D] -> fp64 rotation and bound, [B,H,T,D]
        r, mag = ar.rope_ref(x.reshape(B * T, -1, D), cos, sin, pos)
        return (r.view(B, T, -1, D).transpose(1, 2),
                ar.rope_tol(r, mag).view(B, T, -1, D).transpose(1, 2))

    q_true, q_tol = rot(q)
    k_true, k_tol = rot(k)
    assert q_rot.shape == (B, Hq, T, D) and q_rot.is_contiguous()
    assert ((q_rot.cpu().double() - q_true).abs() <= q_tol).all()
    rows = [p[:, :, p0:p0 + T].cpu() for p in views]
    v_true = v.transpose(1, 2).cpu()
    if int8:
        ar.check_kv8(rows[0], rows[2], k_true)
        ar.check_kv8(rows[1], rows[3], v_true)
    else:
        assert ((rows[0].double() - k_true).abs() <= k_tol).all()
        assert torch.equal(rows[1], v_true)
    # nothing else was written: slot 0, and every row outside [p0, p0+T)
    for p, b4 in zip(planes, before):
        b4[1:3, :, p0:p0 + T] = p[1:3, :, p0:p0 + T]
        assert torch.equal(p, b4)


# -------------------------------------------------------- attn_prefill_kv

def _attn_inputs(D, int8, T, q_off, window, sink_kind, seed):
    """q, sinks and a [B+1]-slot cache whose slots 1.. are the case (slot 0
    and rows >= kv_len are poisoned, rows below the window are finite and
    scaled by 1e4)."""
    B, Hq, Hkv = 2, 10, 2
    kv_len = q_off + T
    Smax = kv_len + 40
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, T, D, generator=gen).to(BF16).to(DEV)
    k = torch.randn(B + 1, Hkv, Smax, D, generator=gen)
    v = torch.randn(B + 1, Hkv, Smax, D, generator=gen)
    sinks = ar.make_sinks(sink_kind, Hq, gen)
    if window > 0:
        lo = max(0, q_off - window + 1)
        k[:, :, :lo] *= 1e4
        v[:, :, :lo] *= 1e4
    k, v = k.to(BF16), v.to(BF16)
    ks = vs = None
    if int8:
        k, ks = ref.quantize_kv_rows(k)
        v, vs = ref.quantize_kv_rows(v)
        poison = [ks, vs]
    else:
        poison = [k, v]
    for t in poison:
        t[0] = float("nan")
        t[:, :, kv_len:] = float("nan")

    def dev(t):   # slots 1.. of plane 0 of a [B+1, 2, ...] buffer: a view
        if t is None:      # with its own batch stride, as slot() hands out
            return None
        big = torch.zeros(B + 1, 2, *t.shape[1:], dtype=t.dtype, device=DEV)
        big[:, 0] = t.to(DEV)
        return big[1:, 0]

    return dict(q=q, k=dev(k), v=dev(v), ks=dev(ks), vs=dev(vs),
                sinks=None if sinks is None else sinks.to(DEV),
                kv_len=kv_len, scale=D ** -0.5)


def _run(x, q, kv_len, q_off, window):
    return ops.attn_prefill_kv(q, x["k"], x["v"], kv_len, x["scale"], q_off,
                               window, x["sinks"], x["ks"], x["vs"])


@pytest.mark.parametrize("sink_kind", ["none", "randn"])
@pytest.mark.parametrize("window", [0, 33])
@pytest.mark.parametrize("T,q_off", [(1, 0), (17, 5), (64, 0), (33, 95),
                                     (65, 70)])
@pytest.mark.parametrize("D,int8", DIMS, ids=DIM_IDS)
def test_attn_prefill_kv_vs_fp64(D, int8, T, q_off, window, sink_kind):
    x = _attn_inputs(D, int8, T, q_off, window, sink_kind,
                     D + 7 * T + q_off + window)
    assert not x["k"].is_contiguous()          # a batch view, as slot() gives
    got = _run(x, x["q"], x["kv_len"], q_off, window)
    B, Hq = x["q"].shape[:2]
    assert got.shape == (B, T, Hq * D)
    out, out_abs = ar.attn_ref(x["q"], x["k"], x["v"], None, x["scale"],
                               window, x["sinks"], q_off=q_off,
                               kscale=x["ks"], vscale=x["vs"])
    ratio = ar.worst_ratio(got.view(B, T, Hq, D).transpose(1, 2), out,
                           out_abs)
    print(f"[err/tol] d{D} i8={int8} T{T} o{q_off} w{window} {sink_kind}: "
          f"{ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("window", [0, 33])
@pytest.mark.parametrize("int8", [False, True], ids=["bf16", "i8"])
def test_attn_prefill_kv_chunk_independent(int8, window):
    """One call over 80 tokens == calls over [0,48) and [48,80), bit for
    bit (what token-exact chunked / prefix-cached prefill rests on)."""
    x = _attn_inputs(128, int8, 80, 0, 0, "none", 5)
    q = x["q"]
    whole = _run(x, q, 80, 0, window)
    a = _run(x, q[:, :, :48].contiguous(), 48, 0, window)
    b = _run(x, q[:, :, 48:].contiguous(), 80, 48, window)
    assert torch.equal(torch.cat([a, b], dim=1), whole)


@pytest.mark.parametrize("window", [0, 33])
def test_bf16_path_keeps_the_unfused_path_bits(window):
    """On a bf16 cache the pair computes what rope_apply + attn_prefill
    compute, bit for bit (same f32 roundings, same 32-position softmax
    steps), so switching prefill_window over changed no model output."""
    B, T, Hq, Hkv, D, p0, Smax = 2, 70, 4, 2, 128, 37, 160
    gen = torch.Generator().manual_seed(window)
    q, k, v = (torch.randn(B, T, h, D, generator=gen).to(BF16).to(DEV)
               for h in (Hq, Hkv, Hkv))
    cos, sin = (t.to(DEV) for t in ops.rope_tables(Smax, D, 10000.0))
    kc = torch.randn(B, Hkv, Smax, D, generator=gen).to(BF16).to(DEV)
    vc = torch.randn(B, Hkv, Smax, D, generator=gen).to(BF16).to(DEV)
    pos = torch.arange(p0, p0 + T, device=DEV)
    q_rot = ops.rope_append_rows(q, k, v, kc, vc, p0, cos, sin)
    assert torch.equal(q_rot, ops.rope_apply(q, cos, sin, pos).transpose(1, 2))
    assert torch.equal(kc[:, :, p0:p0 + T],
                       ops.rope_apply(k, cos, sin, pos).transpose(1, 2))
    got = ops.attn_prefill_kv(q_rot, kc, vc, p0 + T, D ** -0.5, p0, window)
    old = ops.attn_prefill(q_rot, kc[:, :, :p0 + T], vc[:, :, :p0 + T],
                           D ** -0.5, p0, window)
    assert torch.equal(got, old.transpose(1, 2).reshape(B, T, Hq * D))


# ------------------------------------------------------------ model level

@pytest.mark.parametrize("inplace", ["1", "0"])
@pytest.mark.parametrize("kv_bits", [16, 8])
def test_prefill_window_chunked_gpu_vs_cpu(kv_bits, inplace, monkeypatch):
    """Tiny llama (2 layers, head_dim 64, GQA): 24 tokens prefilled as
    chunks of 16 and 8 on the GPU agree with the CPU model, with the
    in-place path and with DNET_PREFILL_INPLACE=0."""
    from dnet_amd.models import ModelConfig, get_ring_model
    from test_ops_gpu import _clone_model
    monkeypatch.setenv("DNET_PREFILL_INPLACE", inplace)
    cfg = ModelConfig.from_hf(dict(
        model_type="llama", hidden_size=128, num_hidden_layers=2,
        num_attention_heads=4, num_key_value_heads=2, head_dim=64,
        intermediate_size=256, vocab_size=256, rope_theta=10000.0))

    def build(dev):
        m = get_ring_model("llama")(cfg, range(2), dev, True, True, smax=64)
        m.kv_bits = kv_bits
        m.init_random(3)
        return m

    mg, mc = build("cuda:0"), build("cpu")
    _clone_model(mg, mc)
    toks = torch.randint(0, 256, (2, 24), generator=torch.Generator()
                         .manual_seed(1))
    outs = []
    for m in (mg, mc):
        kv = m.make_kv_cache(2, 64)
        hs = []
        for t0, t1 in ((0, 16), (16, 24)):
            h = m.embed_tokens(toks[:, t0:t1].to(m.device)).clone()
            hs.append(m.prefill_window(h, m.layer_ids, kv, t0).float().cpu())
        outs.append(torch.cat(hs, dim=1))
    cos = torch.nn.functional.cosine_similarity(outs[0], outs[1], dim=-1)
    assert (cos > 0.99).all(), f"gpu vs cpu prefill, min cosine {cos.min()}"

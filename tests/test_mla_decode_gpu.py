"""ops.mla_decode (HIP flash-decode over the latent MLA cache) against the
fp64 reference and bound of tests/attn_reference.py, and the DeepSeek
latent decode step end to end."""
import os

import pytest
import torch

import attn_reference as ar
import dnet_amd.ops as ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
SCALE = 192 ** -0.5
LENS = [(1, 63, 64), (65, 129, 320), (0, 7, 200)]


def _inputs(nh, lens, smax, seed):
    """q_lat, q_pe and the layer-1 planes of an [L=2, B, S, .] latent cache
    whose rows >= len hold NaN."""
    B = len(lens)
    gen = torch.Generator().manual_seed(seed)
    q_lat = torch.randn(B, nh, 512, generator=gen).to(BF16).to(DEV)
    q_pe = torch.randn(B, nh, 64, generator=gen).to(BF16).to(DEV)
    ckv = torch.randn(2, B, smax, 512, generator=gen).to(BF16)
    kpe = torch.randn(2, B, smax, 64, generator=gen).to(BF16)
    for b, ln in enumerate(lens):
        ckv[:, b, ln:] = float("nan")
        kpe[:, b, ln:] = float("nan")
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    return q_lat, q_pe, ckv.to(DEV), kpe.to(DEV), lens_t


def _ratio(got, q_lat, q_pe, ckv, kpe, lens_t):
    out, out_abs = ar.attn_ref(torch.cat([q_lat, q_pe], -1),
                               torch.cat([ckv, kpe], -1)[:, None],
                               ckv[:, None], lens_t.cpu(), SCALE, 0, None)
    return ar.worst_ratio(got, out, out_abs)


@pytest.mark.parametrize("nh,splits,li", [
    (16, 1, 0), (16, 2, 1), (16, 4, 2), (16, 8, 0),
    (8, 1, 1), (8, 2, 2), (8, 4, 0), (8, 8, 1),
    (40, 1, 2), (40, 2, 0), (40, 4, 1), (40, 8, 2),
    (128, 1, 0), (128, 2, 1), (128, 4, 2), (128, 8, 0),
])
def test_mla_decode_vs_fp64(nh, splits, li):
    lens = LENS[li]
    q_lat, q_pe, ckv, kpe, lens_t = _inputs(nh, lens, 320,
                                            nh + 10 * splits + li)
    ckv, kpe = ckv[1], kpe[1]
    got = ops.mla_decode(q_lat, q_pe, ckv, kpe, lens_t, SCALE, splits=splits)
    assert got.shape == (3, nh, 512) and got.dtype == BF16
    ratio = _ratio(got, q_lat, q_pe, ckv, kpe, lens_t)
    print(f"[err/tol] nh{nh} splits{splits} lens{lens}: {ratio:.3f}")
    assert ratio <= 1.0
    for b, ln in enumerate(lens):
        if ln == 0:
            assert (got[b] == 0).all()
    again = ops.mla_decode(q_lat, q_pe, ckv, kpe, lens_t, SCALE,
                           splits=splits)
    assert torch.equal(got, again)


@pytest.mark.parametrize("splits", [1, 4])
def test_mla_decode_slot_view(splits):
    """The [:, 1:2] view MLAKVCache.slot(1) hands out: batch 1, the batch
    stride of the 3-row allocation."""
    q_lat, q_pe, ckv, kpe, lens_t = _inputs(16, LENS[1], 320, 5)
    ckv, kpe = ckv[:, 1:2][1], kpe[:, 1:2][1]
    assert ckv.stride(0) == 320 * 512 and ckv.shape[0] == 1
    args = (q_lat[1:2].contiguous(), q_pe[1:2].contiguous(), ckv, kpe,
            lens_t[1:2])
    got = ops.mla_decode(*args, SCALE, splits=splits)
    assert _ratio(got, *args) <= 1.0


def test_mla_decode_natural_splits():
    q_lat, q_pe, ckv, kpe, lens_t = _inputs(16, (2000,), 2048, 11)
    assert ops._mla_splits(1, 16, 2048) > 1
    got = ops.mla_decode(q_lat, q_pe, ckv[1], kpe[1], lens_t, SCALE)
    ratio = _ratio(got, q_lat, q_pe, ckv[1], kpe[1], lens_t)
    print(f"[err/tol] natural splits: {ratio:.3f}")
    assert ratio <= 1.0


def test_deepseek_latent_kernel_matches_perhead():
    """One decode step after a 70-token prefill, real MLA dims: (a) per-head
    cache, (b) latent einsum path, (c) latent HIP kernel. (b) - (a) is the
    spread of two bf16 orderings of the same math; the kernel, a third
    rounding of the same size, stays within twice that."""
    from dnet_amd.models import ModelConfig, get_ring_model
    cfg = ModelConfig.from_hf(dict(
        model_type="deepseek_v2", hidden_size=256, num_hidden_layers=2,
        num_attention_heads=16, num_key_value_heads=16, vocab_size=256,
        intermediate_size=512, kv_lora_rank=512, qk_nope_head_dim=128,
        qk_rope_head_dim=64, v_head_dim=128, rope_theta=10000.0))
    gen = torch.Generator().manual_seed(4)
    toks = torch.randint(0, 256, (2, 70), generator=gen).to(DEV)
    nxt = torch.randint(0, 256, (2,), generator=gen).to(DEV)

    def run(env):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            m = get_ring_model("deepseek_v2")(cfg, range(2), "cuda:0", True,
                                              True, smax=256)
            m.init_random(3)
            kv = m.make_kv_cache(2, 256)
            m.prefill_window(m.embed_tokens(toks).clone(), m.layer_ids, kv, 0)
            kv.pos.fill_(70)
            h = m.decode_window(m.embed_tokens(nxt).clone(), m.layer_ids, kv)
            return h.float().cpu()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    a = run({"DNET_MLA_PERHEAD": "1"})
    b = run({"DNET_MLA_PERHEAD": "0", "DNET_MLA_KERNEL": "0"})
    c = run({"DNET_MLA_PERHEAD": "0", "DNET_MLA_KERNEL": "1"})
    d_ref = float((b - a).abs().max())
    d_ker = float((c - a).abs().max())
    print(f"[mla model] d_ref {d_ref:.5f} kernel {d_ker:.5f} "
          f"ratio {d_ker / d_ref if d_ref else float('inf'):.3f}")
    assert d_ref > 0
    assert d_ker <= 2 * d_ref

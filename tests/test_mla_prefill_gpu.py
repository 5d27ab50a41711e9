"""ops.mla_prefill (HIP flash-prefill over the latent MLA cache) against the
fp64 reference and bound of tests/attn_reference.py, and the DeepSeek
continuation prefill end to end."""
import functools
import os

import pytest
import torch

import attn_reference as ar
import dnet_amd.ops as ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
SCALE = 192 ** -0.5

# (T, q_off): one token; a block's tokens straddle 64 (n = 61..65); straddle
# 128 with blocks of 4 + 3; pure causal (early items see fewer chunks than
# their block); the last chunk
SHAPES16 = [(1, 0), (5, 60), (7, 122), (33, 0), (6, 250)]
CASES = ([(16, T, o, s) for T, o in SHAPES16 for s in (1, 2, 4)]
         + [(16, 5, 60, 8)]                 # a split owns no chunk
         # ragged tile; 3 tiles (a block spans two tokens); 8 tiles
         + [(nh, T, o, s) for nh in (8, 40, 128)
            for T, o in ((5, 60), (7, 122)) for s in (1, 4)])


@functools.lru_cache(maxsize=None)
def _case(nh, T, q_off, smax=320, B=2):
    """Inputs (layer-1 planes of an [L=2, B, S, .] latent cache whose rows
    >= q_off + T hold NaN) and the fp64 reference, shared by every split
    count of a shape."""
    gen = torch.Generator().manual_seed(1000 * nh + 10 * T + q_off)
    q_lat = torch.randn(B, T, nh, 512, generator=gen).to(BF16).to(DEV)
    q_pe = torch.randn(B, T, nh, 64, generator=gen).to(BF16).to(DEV)
    ckv = torch.randn(2, B, smax, 512, generator=gen).to(BF16)
    kpe = torch.randn(2, B, smax, 64, generator=gen).to(BF16)
    ckv[:, :, q_off + T:] = float("nan")
    kpe[:, :, q_off + T:] = float("nan")
    ckv, kpe = ckv.to(DEV), kpe.to(DEV)
    q = torch.cat([q_lat, q_pe], -1).permute(0, 2, 1, 3)
    out, out_abs = ar.attn_ref(q, torch.cat([ckv[1], kpe[1]], -1)[:, None],
                               ckv[1][:, None], None, SCALE, 0, None,
                               q_off=q_off)
    return q_lat, q_pe, ckv, kpe, out, out_abs


def _check(got, out, out_abs, tag):
    ratio = ar.worst_ratio(got.permute(0, 2, 1, 3), out, out_abs)
    print(f"[err/tol] {tag}: {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("nh,T,q_off,splits", CASES)
def test_mla_prefill_vs_fp64(nh, T, q_off, splits):
    q_lat, q_pe, ckv, kpe, out, out_abs = _case(nh, T, q_off)
    args = (q_lat, q_pe, ckv[1], kpe[1], q_off, SCALE)
    got = ops.mla_prefill(*args, splits=splits)
    assert got.shape == (2, T, nh, 512) and got.dtype == BF16
    _check(got, out, out_abs, f"nh{nh} T{T} off{q_off} splits{splits}")
    assert torch.equal(got, ops.mla_prefill(*args, splits=splits))


def test_mla_prefill_slot_view():
    """The [:, 1:2] view MLAKVCache.slot(1) hands out: batch 1, the batch
    stride of the 2-row allocation."""
    q_lat, q_pe, ckv, kpe, out, out_abs = _case(16, 7, 122)
    cs, ks = ckv[:, 1:2][1], kpe[:, 1:2][1]
    assert cs.stride(0) == 320 * 512 and cs.shape[0] == 1
    got = ops.mla_prefill(q_lat[1:2].contiguous(), q_pe[1:2].contiguous(),
                          cs, ks, 122, SCALE, splits=2)
    assert got.shape == (1, 7, 16, 512) and got.dtype == BF16
    _check(got, out[1:2], out_abs[1:2], "slot view")


def test_mla_prefill_natural_splits():
    assert ops._mla_prefill_splits(2, 10, 16, 2000) > 1
    q_lat, q_pe, ckv, kpe, out, out_abs = _case(16, 10, 1990, smax=2048)
    got = ops.mla_prefill(q_lat, q_pe, ckv[1], kpe[1], 1990, SCALE)
    assert got.shape == (2, 10, 16, 512) and got.dtype == BF16
    _check(got, out, out_abs, "natural splits")
    assert torch.equal(got, ops.mla_prefill(q_lat, q_pe, ckv[1], kpe[1],
                                            1990, SCALE))


def test_deepseek_continuation_prefill_three_ways():
    """64 tokens at p0 = 0, then 6 more at p0 = 64, real MLA dims, latent
    cache: (a) expanded k/v through ops.attn_prefill, (b) expanded k/v
    through the hipBLASLt einsum attention, (c) ops.mla_prefill. (b) - (a)
    is the spread of two bf16 orderings of the same math; the absorbed
    kernel path, a third, stays within twice that (the factor of
    test_deepseek_latent_kernel_matches_perhead)."""
    from dnet_amd.models import ModelConfig, get_ring_model
    cfg = ModelConfig.from_hf(dict(
        model_type="deepseek_v2", hidden_size=256, num_hidden_layers=2,
        num_attention_heads=16, num_key_value_heads=16, vocab_size=256,
        intermediate_size=512, kv_lora_rank=512, qk_nope_head_dim=128,
        qk_rope_head_dim=64, v_head_dim=128, rope_theta=10000.0))
    toks = torch.randint(0, 256, (2, 70),
                         generator=torch.Generator().manual_seed(4)).to(DEV)

    def run(env, kernel_only=False):
        env = dict(env, DNET_MLA_PERHEAD="0")
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            m = get_ring_model("deepseek_v2")(cfg, range(2), "cuda:0", True,
                                              True, smax=256)
            m.init_random(3)
            kv = m.make_kv_cache(2, 256)
            m.prefill_window(m.embed_tokens(toks[:, :64]).clone(),
                             m.layer_ids, kv, 0)
            if kernel_only:
                def no_expand(*a, **k):
                    raise AssertionError("_expand_kv on the kernel path")
                m._expand_kv = no_expand
                m.MLA_PREFILL_MAX_T = 64   # whatever the default is
            h = m.prefill_window(m.embed_tokens(toks[:, 64:]).clone(),
                                 m.layer_ids, kv, 64)
            return h.float().cpu()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    a = run({"DNET_MLA_PREFILL": "0"})
    b = run({"DNET_MLA_PREFILL": "0", "DNET_EINSUM_PREFILL": "1"})
    c = run({"DNET_MLA_PREFILL": "1"}, kernel_only=True)
    d_ref = float((b - a).abs().max())
    d_ker = float((c - a).abs().max())
    print(f"[mla prefill model] d_ref {d_ref:.5f} kernel {d_ker:.5f} "
          f"ratio {d_ker / d_ref if d_ref else float('inf'):.3f}")
    assert d_ref > 0
    assert d_ker <= 2 * d_ref

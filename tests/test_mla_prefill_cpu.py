"""ops.mla_prefill on CPU tensors (the fp32 reference path)."""
import torch

import attn_reference as ar
import dnet_amd.ops as ops

BF16 = torch.bfloat16
SCALE = 192 ** -0.5
NH, T, Q_OFF, S = 4, 5, 3, 16


def _inputs():
    gen = torch.Generator().manual_seed(7)
    q_lat = torch.randn(2, T, NH, 512, generator=gen).to(BF16)
    q_pe = torch.randn(2, T, NH, 64, generator=gen).to(BF16)
    ckv = torch.randn(2, S, 512, generator=gen).to(BF16)
    kpe = torch.randn(2, S, 64, generator=gen).to(BF16)
    ckv[:, Q_OFF + T:] = float("nan")
    kpe[:, Q_OFF + T:] = float("nan")
    return q_lat, q_pe, ckv, kpe


def test_mla_prefill_cpu_vs_fp64():
    q_lat, q_pe, ckv, kpe = _inputs()
    got = ops.mla_prefill(q_lat, q_pe, ckv, kpe, Q_OFF, SCALE)
    assert got.shape == (2, T, NH, 512) and got.dtype == BF16
    out, out_abs = ar.attn_ref(
        torch.cat([q_lat, q_pe], -1).permute(0, 2, 1, 3),
        torch.cat([ckv, kpe], -1)[:, None], ckv[:, None], None, SCALE, 0,
        None, q_off=Q_OFF)
    assert ar.worst_ratio(got.permute(0, 2, 1, 3), out, out_abs) <= 1.0


def test_mla_prefill_cpu_rows_are_decode():
    q_lat, q_pe, ckv, kpe = _inputs()
    got = ops.mla_prefill(q_lat, q_pe, ckv, kpe, Q_OFF, SCALE)
    for t in range(T):
        lens = torch.full((2,), Q_OFF + t + 1, dtype=torch.int32)
        dec = ops.mla_decode(q_lat[:, t], q_pe[:, t], ckv, kpe, lens, SCALE)
        assert torch.equal(got[:, t], dec)

"""ops.mla_decode on CPU tensors (the fp32 reference path) against the fp64
reference and bound of tests/attn_reference.py."""
import pytest
import torch

import attn_reference as ar
import dnet_amd.ops as ops


@pytest.mark.parametrize("nh,lens", [(5, (3, 0, 40)), (16, (40, 17))])
def test_mla_decode_cpu_vs_fp64(nh, lens):
    B, S, scale = len(lens), 40, 192 ** -0.5
    gen = torch.Generator().manual_seed(nh)
    q_lat, q_pe, ckv, kpe = (
        torch.randn(*s, generator=gen).to(torch.bfloat16)
        for s in ((B, nh, 512), (B, nh, 64), (B, S, 512), (B, S, 64)))
    for b, ln in enumerate(lens):
        ckv[b, ln:] = float("nan")
        kpe[b, ln:] = float("nan")
    lens_t = torch.tensor(lens, dtype=torch.int32)
    got = ops.mla_decode(q_lat, q_pe, ckv, kpe, lens_t, scale)
    out, out_abs = ar.attn_ref(torch.cat([q_lat, q_pe], -1),
                               torch.cat([ckv, kpe], -1)[:, None],
                               ckv[:, None], lens_t, scale, 0, None)
    assert got.shape == (B, nh, 512) and got.dtype == torch.bfloat16
    assert ar.worst_ratio(got, out, out_abs) <= 1.0
    assert ops.mla_decode_supported(512, 64)
    assert not ops.mla_decode_supported(32, 8)

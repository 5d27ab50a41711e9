"""CPU reference of the token-routed MoE trio against the dense reference
pair (moe_gateup / moe_down) on the routed pairs."""
import pytest
import torch

import dnet_amd.ops as ops
from dnet_amd.ops import reference as ref

T, E, K, I, H, TOPK = 130, 8, 320, 192, 320, 3


@pytest.mark.parametrize("glu", [0, 1])
def test_rows_trio_matches_dense_reference(glu):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(T, K, generator=gen).to(torch.bfloat16)
    gw = (torch.randn(E, 2 * I, K, generator=gen) / 8).to(torch.bfloat16)
    dw = (torch.randn(E, H, I, generator=gen) / 8).to(torch.bfloat16)
    gb = torch.randn(E, 2 * I, generator=gen).to(torch.bfloat16)
    db = torch.randn(E, H, generator=gen).to(torch.bfloat16)
    val, idx = torch.rand(T, E, generator=gen).topk(TOPK, dim=1)
    we = torch.zeros(T, E).scatter_(1, idx, val)
    we[:, 1] = 0.0          # an empty expert, rows with two experts
    we[7] = 0.0             # an unrouted token
    # the gate the models use: mxfp4 only (uint8 alone is not enough:
    # grouped int4 banks are uint8 too)
    nib = torch.zeros(E, 2 * I, K // 2, dtype=torch.uint8)
    assert ops.moe_rows_supported(nib, K, I, H, 32, False)
    assert not ops.moe_rows_supported(nib, K, I, H, 128, True)
    assert not ops.moe_rows_supported(nib, K + 32, I, H, 32, False)
    assert not ops.moe_rows_supported(gw, K, I, H, 0, False)
    plan = ops.moe_route(we, TOPK)
    act = ops.moe_gateup_rows(x, gw, None, gb, plan, 0, False, glu)
    out = ops.moe_down_rows(act, dw, None, db, we, plan)
    dense = ref.moe_gateup(x, gw, None, gb, we, 0, False, glu)
    st = plan["slot_token"]
    live = int(plan["offsets"][E])
    assert live == int((we != 0).sum()) and (st[live:] == -1).all()
    spread = torch.zeros_like(dense)    # the trio's act in the dense layout
    for e in range(E):
        s0, s1 = int(plan["offsets"][e]), int(plan["offsets"][e + 1])
        # two f32 summation orders, then one bf16 rounding
        torch.testing.assert_close(act[s0:s1].float(),
                                   dense[e, st[s0:s1].long()].float(),
                                   rtol=2 ** -7, atol=1e-5)
        spread[e, st[s0:s1].long()] = act[s0:s1]
    # same inputs, two f32 orders of I + TOPK + 2 steps: one f32 ulp per
    # step of a magnitude sum that stays below 100 here
    want = ref.moe_down(spread, dw, None, db, we)
    torch.testing.assert_close(out, want, rtol=0,
                               atol=(I + TOPK + 2) * 2.0 ** -23 * 100)
    assert not out[7].any()

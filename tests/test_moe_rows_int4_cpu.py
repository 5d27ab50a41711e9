"""ops.moe_rows_int4_supported, and the CPU reference of the token-routed
trio on a packed int4 bank against the dense reference pair."""
import pytest
import torch

import dnet_amd.ops as ops
from dnet_amd.ops import reference as ref

T, E, K, I, H, G, TOPK = 70, 4, 256, 128, 64, 128, 2


@pytest.mark.parametrize("args,ok", [
    # accepted; then row-major, group % 128, K % 128, I % 128, K % group,
    # I % group, H % 64
    ((256, 128, 64, 128, True), True), ((256, 128, 64, 128, False), False),
    ((256, 128, 64, 64, True), False), ((320, 128, 64, 128, True), False),
    ((256, 192, 64, 128, True), False), ((384, 256, 64, 256, True), False),
    ((256, 384, 64, 256, True), False), ((256, 128, 96, 128, True), False),
])
def test_supported_truth_table(args, ok):
    assert ops.moe_rows_int4_supported(*args) is ok


def test_rows_trio_matches_dense_reference_int4():
    gen = torch.Generator().manual_seed(1)

    def bank(n, k):
        q, s = zip(*(ref.quantize_int4(torch.randn(n, k, generator=gen) / 8,
                                       G) for _ in range(E)))
        return torch.stack([ref.pack_int4_mfma(x) for x in q]), torch.stack(s)

    x = torch.randn(T, K, generator=gen).to(torch.bfloat16)
    (gw, gs), (dw, ds) = bank(2 * I, K), bank(H, I)
    val, idx = torch.rand(T, E, generator=gen).topk(TOPK, dim=1)
    we = torch.zeros(T, E).scatter_(1, idx, val)
    we[:, 1], we[7] = 0.0, 0.0      # an empty expert, an unrouted token
    plan = ops.moe_route(we, TOPK)
    act = ops.moe_gateup_rows(x, gw, gs, None, plan, G, True)
    out = ops.moe_down_rows(act, dw, ds, None, we, plan, G, True)
    dense = ref.moe_gateup(x, gw, gs, None, we, G, True)
    spread = torch.zeros_like(dense)    # the trio's act in the dense layout
    for e in range(E):
        s0, s1 = int(plan["offsets"][e]), int(plan["offsets"][e + 1])
        toks = plan["slot_token"][s0:s1].long()     # two f32 orders + bf16
        torch.testing.assert_close(act[s0:s1].float(), dense[e, toks].float(),
                                   rtol=2 ** -7, atol=1e-5)
        spread[e, toks] = act[s0:s1]
    # two f32 orders of I + TOPK + 2 steps, one ulp of a sum < 100 each
    torch.testing.assert_close(out, ref.moe_down(spread, dw, ds, None, we, G,
                                                 True), rtol=0,
                               atol=(I + TOPK + 2) * 2.0 ** -23 * 100)
    assert not out[7].any()

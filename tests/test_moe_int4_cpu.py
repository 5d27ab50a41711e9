"""int4 expert banks through the CPU reference ops: the pack_int4_mfma
inverse, and moe_gateup / moe_down against the einsum over dequant_int4."""
import pytest
import torch

import dnet_amd.ops as ops
from dnet_amd.ops import reference as ref

E, M, K, I, H, G = 3, 5, 256, 128, 48, 128


def _bank(n, k, gen):
    q = torch.randint(0, 256, (E, n, k // 2), generator=gen,
                      dtype=torch.int16).to(torch.uint8)
    s = (torch.rand(E, n, k // G, generator=gen) / 16 + 0.01).to(torch.bfloat16)
    wf = torch.stack([ref.dequant_int4(q[e], s[e], G) for e in range(E)])
    qp = torch.stack([ref.pack_int4_mfma(q[e]) for e in range(E)])
    return q, qp, s, wf.float()


def test_unpack_int4_mfma_inverts_pack():
    gen = torch.Generator().manual_seed(1)
    q = torch.randint(0, 256, (7, 192), generator=gen,
                      dtype=torch.int16).to(torch.uint8)
    qp = ref.pack_int4_mfma(q)
    assert not torch.equal(qp, q)
    assert torch.equal(ref.unpack_int4_mfma(qp), q)


@pytest.mark.parametrize("packed", [False, True])
def test_ref_moe_int4_equals_einsum(packed):
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    we = torch.rand(M, E, generator=gen)
    gq, gqp, gs, gwf = _bank(2 * I, K, gen)
    dq, dqp, ds, dwf = _bank(H, I, gen)
    act = ops.moe_gateup(x, gqp if packed else gq, gs, None, we, G, packed)
    gu = torch.einsum("mk,enk->emn", x.float(), gwf)
    want = (torch.nn.functional.silu(gu[..., :I]) * gu[..., I:]).to(
        torch.bfloat16)
    assert torch.equal(act, want)
    out = ops.moe_down(act, dqp if packed else dq, ds, None, we, G, packed)
    d = torch.einsum("emi,ehi->emh", act.float(), dwf)
    assert torch.equal(out, (we.t().unsqueeze(-1) * d).sum(0))

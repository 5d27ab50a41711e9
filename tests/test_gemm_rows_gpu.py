"""ops.gemm_rows, the fused-dequant MFMA prefill GEMM for packed int8 /
int4 linears (M > 64), against the fp64 reference and the derived bound of
tests/gemm_reference.py (err/tol <= 1.0), and its routing in Linear.

Shapes sit on the kernel's tile edges. The M tile is 128 rows: M = 65 (one
row past the decode limit), 128 (one exact tile), 129 (one row into the
second tile), 200 (a ragged second tile). The N tile is 64 columns at
these sizes, not 128, so next to the 72 / 128 / 200 of a 128-column tile
N also takes 40 (below one tile) and 64 (one exact tile); 72 and 200 are
ragged last tiles of either width. The 128-column tile is picked only
from 512 block tiles up, so it gets two cases of its own at
N = 256 * 128 + 72. int8 K = 64 and 320 end in a 64-k half stage.
"""
import itertools

import pytest
import torch

import gemm_reference as gr
import dnet_amd.ops as ops
from dnet_amd.models import base
from dnet_amd.models.config import QuantConfig

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
KG = {"int8": [(64, 64), (320, 64), (1152, 128), (1280, 256)],
      "int4": [(128, 128), (384, 128), (1280, 256)]}
CASES = [(f, m, n, k, g, b) for f in KG for (k, g) in KG[f]
         for m, n, b in itertools.product((65, 128, 129, 200),
                                          (40, 64, 72, 128, 200),
                                          (False, True))]
CASES += [("int8", 200, 32840, 320, 64, True),
          ("int4", 200, 32840, 384, 128, True)]


def _inputs(fmt, m, n, k, g, bias, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=gen).to(BF16)
    w = gr.make_weights(fmt, n, k, g, gen)
    b = torch.randn(n, generator=gen).to(BF16) if bias else None
    return x, w, b


def _rows(w, x, b):
    return ops.gemm_rows(x.cuda(), w["packed"].cuda(), w["scales"].cuda(),
                         w["G"], None if b is None else b.cuda(),
                         gr.BITS[w["fmt"]])


@pytest.mark.parametrize("fmt,m,n,k,g,bias", CASES)
def test_against_fp64(fmt, m, n, k, g, bias):
    x, w, b = _inputs(fmt, m, n, k, g, bias, 7000 + m + n + k)
    ref, mag = gr.gemm_ref(x, gr.contract_weights(w), b)
    r = gr.ratio(_rows(w, x, b), ref, gr.gemm_tol(ref, mag, k))
    print(f"[err/tol] gemm_rows {fmt}-M{m}-N{n}-K{k}-G{g}-b{int(bias)}: "
          f"{r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("fmt,k,g", [("int8", 320, 64), ("int4", 384, 128)])
def test_onehot_is_exact(fmt, k, g):
    """x = I_K in one call: row k comes back as bf16(w_contract[:, k])."""
    w = gr.make_weights(fmt, 72, k, g, torch.Generator().manual_seed(7100))
    got = _rows(w, torch.eye(k, dtype=BF16), None).cpu().float()
    want = gr.contract_weights(w).to(BF16).t().float()
    bad = int((got != want).sum())
    print(f"[onehot] gemm_rows {fmt}-K{k}: {bad} of {got.numel()} differ")
    assert bad == 0


@pytest.mark.parametrize("fmt", ["int8", "int4"])
def test_rows_are_independent_and_repeatable(fmt):
    x, w, b = _inputs(fmt, 200, 200, 1152, 128, True, 7200)
    full = _rows(w, x, b)
    assert torch.equal(full, _rows(w, x, b))
    assert torch.equal(full[:70], _rows(w, x[:70], b))


@pytest.mark.parametrize("bits", [8, 4])
def test_linear_routing(bits, monkeypatch):
    gen = torch.Generator().manual_seed(7300)
    wf = (torch.randn(200, 1152, generator=gen) / 30).to(BF16).cuda()
    bias = torch.randn(200, generator=gen).to(BF16).cuda()
    x = torch.randn(96, 1152, generator=gen).to(BF16).cuda()
    lin = base.Linear.make(wf, bias, QuantConfig(bits, 128))
    assert lin.bits == bits and lin.packed
    monkeypatch.setattr(base, "GEMM_ROWS_MAX_M", 128)
    assert torch.equal(lin(x), ops.gemm_rows(x, lin.w, lin.scales, 128, bias,
                                             bits))
    gemv = ops.gemv_int8 if bits == 8 else ops.gemv_int4
    assert torch.equal(lin(x[:64]),
                       gemv(x[:64], lin.w, lin.scales, 128, bias, True))
    sup = ops.gemm_rows_supported
    assert sup(96, 200, 1152, 128, bits, True)
    assert not sup(64, 200, 1152, 128, bits, True)
    assert not sup(96, 200, 1152, 128, bits, False)
    k, g = (96, 32) if bits == 8 else (192, 64)    # G divides K
    assert not sup(96, 200, k, g, bits, True)
    assert not sup(96, 200, k, 2 * g, bits, True)  # G aligned, K is not

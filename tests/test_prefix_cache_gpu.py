"""Prompt-prefix KV cache on the GPU: the HIP row-copy kernel bit for bit,
and the serving scenarios under hipGraph decode."""
from __future__ import annotations

import pytest
import torch

from dnet_amd import ops

import prefix_cache_cases as pcc
from prefix_cache_cases import P48, Rt, cold_tokens, env, suffix_avoiding

pytestmark = pytest.mark.gpu

_CASES = pcc.kernel_cases()


def _dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("c", _CASES, ids=pcc.case_id)
def test_kv_copy_rows_kernel_bit_exact(c):
    """Expected = a clone of dst with the torch slice assignment applied;
    every plane is compared whole through an integer view, so every byte
    outside rows [r0, r1) of dst_b is checked unchanged too."""
    assert ops.has_native()
    src = [p.to(_dev()) for p in pcc.make_planes(
        c["planes"], c["L"], c["Bs"], c["H"], c["S"], seed=1)]
    if c["alias"]:
        dst = src
    else:
        dst = [p.to(_dev()) for p in pcc.make_planes(
            c["planes"], c["L"], c["Bd"], c["H"], c["S"], seed=2)]
    r0, r1 = c["r0"], c["r1"]
    want = [d.clone() for d in dst]
    for w, s in zip(want, src):
        w[:, c["dst_b"], ..., r0:r1, :] = s[:, c["src_b"], ..., r0:r1, :]
    ops.kv_copy_rows(dst, c["dst_b"], src, c["src_b"], r0, r1)
    torch.cuda.synchronize()
    for d, w in zip(dst, want):
        assert torch.equal(pcc.as_int(d), pcc.as_int(w))


def test_kv_copy_rows_kernel_argument_checks():
    """Each violation raises from the argument checks alone: nothing is
    launched, dst keeps every byte."""
    src = [p.to(_dev()) for p in pcc.make_planes("int8_d64", 2, 3, 2, 50, 1)]
    dst = [p.to(_dev()) for p in pcc.make_planes("int8_d64", 2, 2, 2, 50, 2)]
    other = [p.to(_dev()) for p in pcc.make_planes("int8_d64", 2, 2, 2, 64, 3)]
    heads = [p.to(_dev()) for p in pcc.make_planes("int8_d64", 2, 2, 1, 50, 3)]
    before = [d.clone() for d in dst]
    bad = [
        (dst, 0, src, 0, 0, 51),          # r1 > S
        (dst, 0, src, 0, 9, 8),           # r0 > r1
        (dst, 0, src, 0, -1, 8),
        (dst, 2, src, 0, 0, 8),           # dst_b out of range
        (dst, 0, src, 3, 0, 8),           # src_b out of range
        (dst, -1, src, 0, 0, 8),
        (dst, 0, other, 0, 0, 8),         # geometry
        (dst, 0, heads, 0, 0, 8),
        (dst, 0, src[:2], 0, 0, 8),       # plane count
        (dst, 1, dst, 1, 0, 8),           # aliased, same batch index
        (dst, 0, [p.cpu() for p in src], 0, 0, 8),   # not on the GPU
    ]
    for a in bad:
        with pytest.raises(RuntimeError):
            ops.kv_copy_rows(*a)
    torch.cuda.synchronize()
    for d, b in zip(dst, before):
        assert torch.equal(pcc.as_int(d), pcc.as_int(b))


def _tiny_prefill_splits_k(ms) -> bool:
    """Does any of the tiny model's prefill GEMMs at M in `ms` run split-k
    (f32 atomics: summation order varies from run to run)?"""
    scratch = ops._get_scratch(_dev()).numel()
    shapes = [(384, 128), (128, 128), (512, 128), (128, 256)]  # (N, K)
    return any(ops._will_defer(m, n, k, 0, 16, scratch)
               for m in ms for n, k in shapes)


@pytest.mark.parametrize("kv_bits", [16, 8])
def test_prompt_reuse_token_exact_under_graphs(kv_bits):
    """B = P + S after A = P with hipGraph decode on: 48 rows come from the
    store, and B's tokens equal a cold run made operation for operation
    identical: cache off, DNET_PREFILL_CHUNK=48, so B prefills as [0, 48)
    then [48, 64) — the GEMM and attention shapes of the warm run."""
    repro = _tiny_prefill_splits_k((48, 16))
    if repro:
        ops.set_reproducible(True)
    try:
        with env(DNET_KV_PREFIX_MIN=16, DNET_PREFILL_CHUNK=48,
                 DNET_SLOTS_GRAPHS=None):
            w = Rt(kv_bits=kv_bits, prefix_entries=2)
            try:
                assert w.rt.executor.use_graphs
                w.put("A", P48, 4)
                w.run_all()
                a = w.toks("A")
                S = suffix_avoiding(a[0])
                w.put("B", P48 + S, 8)
                w.run_all()
                assert w.frames["B"][0]["cached_tokens"] == 48
                warm_b = w.toks("B")
                assert w.rt.executor._graphs      # decode really replayed
            finally:
                w.close()
            cold = cold_tokens(kv_bits, [("A", P48, 4), ("B", P48 + S, 8)],
                               chunk=48)
        assert cold["A"] == a and len(a) == 4
        assert warm_b == cold["B"] and len(warm_b) == 8
    finally:
        if repro:
            ops.set_reproducible(False)


def test_retirement_rows_bitwise_under_graphs():
    """Scenario 4 on the GPU, int8 KV (4 planes): the entry equals the
    retiring slot's rows bit for bit, survives the dummy appends and the
    in-flight step, and is what the next hit copies back."""
    with env(DNET_SLOTS_GRAPHS=None):
        pcc.retirement_scenario(8)

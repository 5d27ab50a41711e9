"""The CPU reference of the logprob contract (ops.logprobs_rows on CPU
tensors) against the fp64 reference of tests/logprob_reference.py, and the
fp64 reference against itself on what the issue states about ties.
"""
import math

import numpy as np
import pytest
import torch

import logprob_reference as lr
import sample_reference as sr
import dnet_amd.ops as ops

K = 20


def _torch_eps(V, L):
    """The CPU reference works in f32 with torch: the rounding of l - m,
    exp to 1 ulp, a sum of V positive terms in an unknown order ((V - 1) u
    at worst), the log to 1 ulp and the subtraction."""
    u = 2.0 ** -24
    return (V + 2) * u + 3 * u * (L + math.log(V))


def _check(logits, tok, n_top, k=K, **out):
    lp, tv, ti = ops.logprobs_rows(
        logits, torch.as_tensor(tok, dtype=torch.int64),
        torch.as_tensor(n_top, dtype=torch.int32), k, **out)
    want = lr.reference(logits.float().numpy(), tok, n_top, k)
    V = logits.shape[1]
    eps = _torch_eps(V, 40.0)
    for b, w in enumerate(want):
        if w is None:
            continue
        assert np.array_equal(ti[b].numpy(), w[2]), b
        assert lr.close(tv[b].numpy(), w[1], eps), b
        assert lr.close(lp[b:b + 1].numpy(), np.array([w[0]]), eps), b
    return lp, tv, ti


@pytest.mark.parametrize("V", [1000, 4099])
def test_reference_matches_fp64(V):
    logits, _, _ = sr.case(V)
    tok = logits.double().argmax(-1).numpy()
    tok[1::2] = 7
    _check(logits, tok, [(0, 1, 5, 20)[b % 4] for b in range(sr.B)])


def test_ties_inside_the_top_20_are_the_rule():
    """Why the order is part of the contract: bf16 logits at this
    vocabulary tie inside the top 20 on nearly every row."""
    for V in (4099, 32768):
        logits, _, _ = sr.case(V)
        tied = sum(len(torch.unique(r.float().topk(20).values)) < 20
                   for r in logits)
        assert tied >= 15


def test_reference_ties_skips_and_degenerate_rows():
    V = 300
    inf, nan = float("inf"), float("nan")
    rows = torch.randn(6, V, generator=torch.Generator().manual_seed(5))
    rows.clamp_(max=3.0)
    rows[0, [250, 4, 99]] = 9.0          # ties: by index
    rows[1] = nan
    rows[2, 45] = inf
    rows[3] = -inf
    rows[3, 77] = nan
    rows[4, ::2] = nan
    lp0 = torch.full((6,), 7.0)
    lp, tv, ti = _check(rows, [4, 0, 45, 1, 1, 2],
                        [20, 20, 2, 3, 20, -1], logp=lp0)
    assert ti[0, :3].tolist() == [4, 99, 250]
    assert (ti[1] == -1).all() and torch.isnan(tv[1]).all()
    assert ti[2, 0] == 45 and torch.isnan(lp[2])
    assert ti[3, :3].tolist() == [0, 1, 2] and torch.isnan(tv[3]).all()
    assert (ti[4] % 2 == 1).all()
    assert lp[5] == 7.0                   # skipped: untouched
    # tiny V: the tail is (-1, NaN)
    lp, tv, ti = _check(rows[:1, :5].contiguous(), [9], [20])
    assert (ti[0, 5:] == -1).all() and torch.isnan(lp[0])


def test_bound():
    assert lr.derive_logp_eps(152064, 40.0) <= 1e-4
    assert lr.derive_logp_eps(152064, 40.0) >= 2.0 ** -19   # l - m alone

"""fp64 reference and derived error bound for ``ops.logprobs_rows`` (the HIP
logprob kernel and its CPU reference). Helper for tests/test_logprobs_gpu.py
and tests/test_logprobs_cpu.py; not a test module.

Contract: NaN logits are absent; m is the largest non-NaN logit,
T = sum exp(l_i - m), logp(j) = (l_j - m) - ln T. The top list is ordered
by logit descending, then index ascending, on the exact input values.
"""
from __future__ import annotations

import math

import numpy as np


def derive_logp_eps(V: int, L: float) -> float:
    """Absolute bound on every finite value the kernel returns, where L
    bounds |l_j - m| over the row.

    Reduction shape of the kernel (logprobs.hip.cpp), term by term, with
    u = 2^-24:
      * d_j = fl32(l_j - m): one f32 rounding of a value of magnitude
        <= L, |error| <= u * L. (Exact for bf16 inputs; budgeted anyway.)
      * the exponential e_i = 2^(d_i * c), c = log2(e) held as an f32 pair
        (its error, 2^-48 relative, costs L * 2^-48) and the product formed
        by one fma: with the rounding of d_i that is two roundings,
        |da_i| <= 2u * |d_i| <= 2uL in natural units, a relative error of
        2uL on e_i; v_exp_f32 is good to 1 ulp, 2 ulp = 2^-22 budgeted.
      * the sum: e_i is truncated to a multiple of 2^-40, V * 2^-40 in all
        against T >= 1 (the max token has e = 1). The sum itself is a
        64-bit integer sum, exact in any order: no chunk-length or
        tree-depth term.
      So T carries a relative error delta = 2uL + 2^-22 + L*2^-48 + V*2^-40.
      * ln: |d ln T| <= delta / (1 - delta); the logarithm is evaluated in
        double on the exact integer, ln(V) * 2^-52.
      * the final subtraction d_j - ln T is formed in double and rounded
        to f32 once: u * (L + ln V).
    """
    u = 2.0 ** -24
    delta = 2 * u * L + 2.0 ** -22 + L * 2.0 ** -48 + V * 2.0 ** -40
    lnv = math.log(V)
    return (u * L + delta / (1 - delta) + lnv * 2.0 ** -52
            + u * (L + lnv))


def spread(l: np.ndarray) -> float:
    """L of one row: the largest |l_j - m| over its finite entries."""
    x = l.astype(np.float64)
    x = x[np.isfinite(x)]
    return float(x.max() - x.min()) if x.size else 0.0


def row_reference(l: np.ndarray, tok: int, n_top: int, K: int):
    """One row of logits -> (logp, topv [K], topi [K]) in fp64."""
    V = l.shape[0]
    x = l.astype(np.float64)
    nan = np.isnan(x)
    topv = np.full(K, np.nan)
    topi = np.full(K, -1, dtype=np.int64)
    xv = np.where(nan, -np.inf, x)
    m = xv.max()
    with np.errstate(all="ignore"):
        if nan.all() or m == -np.inf or m == np.inf:
            lp = np.full(V, np.nan)
        else:
            d = x - m
            lp = d - np.log(np.exp(np.where(nan, -np.inf, d)).sum())
    logp = lp[tok] if 0 <= tok < V else np.nan
    # stable: equal logits keep ascending index order
    order = np.argsort(-xv, kind="stable")
    order = order[~nan[order]]
    n = min(n_top, K, order.size)
    topi[:n] = order[:n]
    topv[:n] = lp[order[:n]]
    return logp, topv, topi


def reference(logits: np.ndarray, tok, n_top, K: int):
    """[B, V] -> (logp [B], topv [B, K], topi [B, K]); rows with
    n_top < 0 are None in all three lists."""
    out = [row_reference(logits[b], int(tok[b]), int(n_top[b]), K)
           if int(n_top[b]) >= 0 else None for b in range(logits.shape[0])]
    return out


def close(got: np.ndarray, want: np.ndarray, eps: float) -> bool:
    """NaN and +-inf must match exactly, finite values within eps."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    if not np.array_equal(got[~fin & ~np.isnan(want)],
                          want[~fin & ~np.isnan(want)]):
        return False
    return bool(np.all(np.abs(got[fin] - want[fin]) <= eps))

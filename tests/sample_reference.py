"""fp64 reference and derived error bound for the per-row token sampler
(``ops.sample_rows``: the fused HIP kernel and its CPU reference). Helper
for tests/test_sampler_gpu.py and tests/test_sampler_cpu.py; not a test
module.

The reference works per row on unique-value classes, so tokens with equal
values are kept or dropped together exactly as the contract says, and it
reports how close the row came to a different keep set (its margin).

Penalties are part of the contract *in f32* (they act on the raw logit
before anything else), so ``penalise`` with dtype float32 reproduces them
bit for bit with IEEE single operations; everything after is fp64.
"""
from __future__ import annotations

import functools
import itertools
import math

import numpy as np
import torch

COUNT_MASK = 0x3FFFFFFF
PROMPT_BIT = 0x40000000
U_MAX = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


# ------------------------------------------------------------------- bound

def derive_eps(V: int, D: float = 32.0) -> float:
    """Relative bound on every mass the sampler compares or draws from.

    Reduction shape of the kernel (sample.hip.cpp), term by term:
      * exponent a_i = fl(fl(l_i - l_max) * c) with c = log2(e) / temp
        held as an f32 pair (error 2^-48, negligible) and the product
        formed by one fma: two roundings, so |da_i| <= 2u * d_i with
        u = 2^-24 and d_i = |a_i| in natural units; a token with d_i <= D
        gets a relative error 2uD from it. (The CPU reference divides by
        temp instead: two roundings as well.)
      * 2^a: v_exp_f32 is good to 1 ulp; 2 ulp = 2^-22 budgeted (the
        CPU reference's torch.exp falls under the same budget).
      * tokens with d_i > D weigh e^-D each, V * e^-D in all, against a
        kept mass S >= 1 (the max token has e = 1 and is always kept).
      * fixed point: e_i is truncated to a multiple of 2^-40, V * 2^-40
        in all.
      * chunk length x 2^-24 and tree depth: zero. All sums (histogram
        bins, wave and block totals, prefix scans) are 64-bit integer
        sums of the fixed-point e_i, exact in any order.
    So any partial sum of kept masses is within delta * S of its fp64
    value, and T within delta * T. A comparison or the draw involves two
    such sums (cdf and u*S; mass_above and top_p*T), plus one fixed-point
    unit from the integer target / ceiling: eps = 2 * delta + 2^-39.
    min-p compares a single e_i with d_i = -ln(min_p) <= D, inside delta.
    """
    u = 2.0 ** -24
    delta = 2 * u * D + 2.0 ** -22 + V * math.exp(-D) + V * 2.0 ** -40
    return 2 * delta + 2.0 ** -39


# --------------------------------------------------------------- penalties

def penalise(l: np.ndarray, seen: np.ndarray, rep: float, pres: float,
             freq: float, dtype=np.float32) -> np.ndarray:
    """Contract step 1 on one row, in `dtype` arithmetic."""
    t = dtype
    l = l.astype(t)
    c = (seen & COUNT_MASK)
    s = (c > 0) | ((seen & PROMPT_BIT) != 0)
    if rep != 1.0:
        with np.errstate(all="ignore"):
            l = np.where(s, np.where(l > 0, l / t(np.float32(rep)),
                                     l * t(np.float32(rep))), l).astype(t)
    l = (l - (t(np.float32(freq)) * c.astype(t)).astype(t)).astype(t)
    return np.where(c > 0, (l - t(np.float32(pres))).astype(t), l).astype(t)


# --------------------------------------------------------------- reference

def row_reference(l: np.ndarray, temp: float, top_k: int, top_p: float,
                  min_p: float) -> dict:
    """One row of (penalised) logits -> fp64 keep set, weights and margin.

    Returns dict(token=..) for rows the contract decides without a draw
    (greedy, +inf, no finite value), else dict(keep, e, margin)."""
    V = l.shape[0]
    x = l.astype(np.float64)
    nan = np.isnan(x)
    xv = np.where(nan, -np.inf, x)
    m = xv.max()
    if m == -np.inf:
        return dict(token=int(np.argmax(nan)) if nan.any() else 0)
    if not temp > 0.0 or m == np.inf:
        return dict(token=int(np.argmax(xv)))
    xv = xv / np.float64(np.float32(temp))
    m = xv.max()
    e = np.exp(xv - m)
    e[nan] = 0.0
    T = e.sum()
    vals, inv, cnt = np.unique(-xv[~nan], return_inverse=True,
                               return_counts=True)   # classes, descending x
    e_ok = e[~nan]
    mass = np.bincount(inv, weights=e_ok, minlength=len(vals))
    e_cls = mass / cnt
    cnt_above = np.cumsum(cnt) - cnt
    mass_above = np.cumsum(mass) - mass
    keep_c = np.ones(len(vals), dtype=bool)
    margin = np.inf
    if 0 < top_k < V:
        keep_c &= cnt_above < top_k
    if top_p < 1.0:
        pT = max(np.float64(np.float32(top_p)), 0.0) * T
        kp = mass_above < pT
        kp[0] = True                     # the max token is always kept
        keep_c &= kp
        margin = min(margin, float(np.abs(mass_above - pT).min() / T))
    if min_p > 0.0:
        mp = min(np.float64(np.float32(min_p)), 1.0)
        keep_c &= e_cls >= mp
        margin = min(margin, float(np.abs(e_cls / mp - 1.0).min()))
    keep = np.zeros(V, dtype=bool)
    keep[~nan] = keep_c[inv]
    return dict(keep=keep, e=e, margin=margin)


def interval_ok(j: int, ref: dict, u: float, eps: float) -> bool:
    """Token j is a correct answer for uniform u: kept, and u*S within
    eps*S of j's cdf interval."""
    if not (0 <= j < ref["keep"].shape[0]) or not ref["keep"][j]:
        return False
    cdf = np.cumsum(np.where(ref["keep"], ref["e"], 0.0))
    S = cdf[-1]
    lo = cdf[j - 1] if j > 0 else 0.0
    return lo - eps * S <= u * S <= cdf[j] + eps * S


def near_step(ref: dict, u: float, eps: float) -> bool:
    """u*S lies within eps*S of a cdf step between two kept tokens: both
    neighbours are correct answers, two f32 pipelines may pick either."""
    cdf = np.cumsum(np.where(ref["keep"], ref["e"], 0.0))
    S = cdf[-1]
    return bool(np.abs(cdf[ref["keep"]][:-1] - u * S).min(initial=np.inf)
                <= eps * S)


# ------------------------------------------------------------------- cases

SHAPES = (1000, 4099, 32768, 152064)
B = 16
_TEMPS = (0.25, 0.7, 1.0, 1.3)
_TOPK = (0, 7, 50)
_TOPP = (1.0, 0.5, 0.9, 0.95)
_MINP = (0.0, 0.05)


def row_params(B: int = B) -> list[tuple]:
    """(temp, top_k, top_p, min_p) per row: row 0 has every filter off,
    row 1 is greedy, the rest stride through the product of the sets so
    every value of every set occurs."""
    prod = list(itertools.product(_TEMPS, _TOPK, _TOPP, _MINP))
    rows = [(1.0, 0, 1.0, 0.0), (0.0, 50, 0.9, 0.0)]
    i = 5
    while len(rows) < B:
        rows.append(prod[i % len(prod)])
        i += 37                                  # coprime to 96
    return rows[:B]


def uniforms(V: int, B: int = B) -> np.ndarray:
    """[8, B] f32: 0, the largest f32 below 1, and six seeded draws."""
    g = torch.Generator().manual_seed(99 + V)
    u = torch.rand(8, B, generator=g)
    u[0] = 0.0
    u[1] = U_MAX
    return u.numpy()


@functools.lru_cache(maxsize=None)
def case(V: int, B: int = B, dtype: str = "bf16"):
    """(logits [B, V], params, fp64 reference per row) for one shape; built
    once and shared by every test that needs it."""
    g = torch.Generator().manual_seed(1234 + V)
    logits = torch.randn(B, V, generator=g) * 3
    if dtype == "bf16":
        logits = logits.to(torch.bfloat16)
    params = row_params(B)
    refs = [row_reference(logits[b].float().numpy(), *params[b])
            for b in range(B)]
    return logits, params, refs


def param_tensors(params, device="cpu"):
    t = torch.tensor
    return (t([p[0] for p in params], dtype=torch.float32, device=device),
            t([p[1] for p in params], dtype=torch.int64, device=device),
            t([p[2] for p in params], dtype=torch.float32, device=device),
            t([p[3] for p in params], dtype=torch.float32, device=device))


def check_tokens(toks, refs, u_row, eps: float, cap: int = 1) -> int:
    """Interval check of one call's tokens; returns the rows skipped as
    ambiguous (margin <= eps) and asserts their number is within `cap`."""
    skipped = 0
    for b, r in enumerate(refs):
        j = int(toks[b])
        if "token" in r:
            assert j == r["token"], (b, j, r["token"])
            continue
        if r["margin"] <= eps:
            skipped += 1
            continue
        assert interval_ok(j, r, float(u_row[b]), eps), \
            (b, j, float(u_row[b]), r["margin"])
    assert skipped <= cap, f"{skipped} ambiguous rows (cap {cap})"
    return skipped

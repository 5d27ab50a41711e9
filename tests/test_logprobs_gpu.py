"""The HIP logprob kernel (ops.logprobs_rows on GPU tensors) against the fp64
reference of tests/logprob_reference.py.

The order of the top list is decided on the exact input values (logit
descending, index ascending), so the indices must equal the reference on
every row, ties included; values must lie within the bound derived from the
kernel's reduction shape (logprob_reference.derive_logp_eps).
"""
import math

import numpy as np
import pytest
import torch

import logprob_reference as lr
import sample_reference as sr
import dnet_amd.ops as ops
from dnet_amd.core.sampler import DecodingConfig, RowSampler, Sampler

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 20
N_TOP = (0, 1, 5, 20)


def _run(logits, tok, n_top, k=K, **out):
    lp, tv, ti = ops.logprobs_rows(
        logits, torch.as_tensor(tok, dtype=torch.int64).to(DEV),
        torch.as_tensor(n_top, dtype=torch.int32).to(DEV), k, **out)
    return lp.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy()


def _check(got, logits_cpu, tok, n_top, eps, k=K):
    lp, tv, ti = got
    want = lr.reference(logits_cpu.float().numpy(), tok, n_top, k)
    V = logits_cpu.shape[1]
    for b, w in enumerate(want):
        if w is None:
            continue
        assert np.array_equal(ti[b], w[2]), (b, ti[b], w[2])
        assert ((ti[b] >= -1) & (ti[b] < V)).all()
        assert lr.close(tv[b], w[1], eps), (b, tv[b], w[1])
        assert lr.close(lp[b:b + 1], np.array([w[0]]), eps), (b, lp[b], w[0])


def _tokens(logits, V):
    """fp64 argmax on even rows, a fixed random id on odd rows."""
    B = logits.shape[0]
    tok = torch.randint(0, V, (B,), generator=torch.Generator()
                        .manual_seed(555 + V))
    tok[::2] = logits.double().argmax(-1)[::2]
    return tok.numpy()


def test_bound_is_tight_enough():
    assert lr.derive_logp_eps(152064, 40.0) <= 1e-4


@pytest.mark.parametrize("V,dtype", [(V, "bf16") for V in sr.SHAPES]
                         + [(4099, "f32")])
def test_reference_shapes(V, dtype):
    logits, _, _ = sr.case(V, dtype=dtype)
    L = max(lr.spread(r.float().numpy()) for r in logits)
    assert L <= 40.0
    eps = lr.derive_logp_eps(V, L)
    tok = _tokens(logits, V)
    n_top = [N_TOP[b % 4] for b in range(sr.B)]
    _check(_run(logits.to(DEV), tok, n_top), logits, tok, n_top, eps)
    print(f"V={V} {dtype} L={L:.1f} eps={eps:.3g}")


def _tie_rows(V=4099):
    """Row 0: five tokens at 10.0, thirty at 9.0, the rest <= 8. Row 1: the
    thirty tied tokens are the maximum. The thirty are spread over different
    waves and several share one 16-byte slot."""
    g = torch.Generator().manual_seed(31)
    rows = (torch.randn(2, V, generator=g) * 2).clamp_(max=8.0)
    thirty = ([8, 9, 10, 11, 13, 17, 250, 251, 520, 521, 522, 523]
              + list(range(700, 4090, 200)) + [4097])
    assert len(thirty) == 30 and len(set(thirty)) == 30
    five = [4098, 3, 1999, 2000, 641]
    rows[0, thirty] = 9.0
    rows[0, five] = 10.0
    rows[1, thirty] = 9.0
    return rows.to(torch.bfloat16), sorted(five), sorted(thirty)


def test_ties_at_the_cut():
    V = 4099
    rows, five, thirty = _tie_rows(V)
    tok = [five[0], thirty[29]]
    got = _run(rows.to(DEV), tok, [20, 20])
    assert got[2][0].tolist() == five + thirty[:15]
    assert got[2][1].tolist() == thirty[:20]
    eps = lr.derive_logp_eps(V, max(lr.spread(r.float().numpy())
                                    for r in rows))
    _check(got, rows, tok, [20, 20], eps)


def test_strided_rows():
    """B = 3, V = 4099, row stride > V: rows start at every 16-byte phase."""
    V, B = 4099, 3
    logits, _, _ = sr.case(V, B)
    # odd stride; the padding holds winning logits, so a read past a row's
    # end or before its start changes the answer
    wide = torch.full((B, V + 12), 60.0, dtype=torch.bfloat16, device=DEV)
    view = wide[:, 3:V + 3]
    view.copy_(logits.to(DEV))
    assert view.stride(0) == V + 12 and view.stride(0) % 8 != 0
    eps = lr.derive_logp_eps(V, 40.0)
    tok = _tokens(logits, V)
    _check(_run(view, tok, [20, 5, 20]), logits, tok, [20, 5, 20], eps)
    # f32: 4-element slots; the odd stride puts the rows at phases 2, 3, 0
    wide = torch.full((B, V + 6), 60.0, device=DEV)
    assert wide.stride(0) % 4 == 1
    view = wide[:, 2:V + 2]
    view.copy_(logits.float().to(DEV))
    _check(_run(view, tok, [20, 5, 20]), logits, tok, [20, 5, 20], eps)


def test_tiny_v():
    """V = 1 and tiny V (shorter than one 16-byte slot, than a wave): the
    tail of the list is (-1, NaN)."""
    for V in (1, 5, 63, 129):
        logits = (torch.randn(4, V, generator=torch.Generator()
                              .manual_seed(V)) * 3).to(torch.bfloat16)
        tok = _tokens(logits, V)
        got = _run(logits.to(DEV), tok, [20] * 4)
        _check(got, logits, tok, [20] * 4, lr.derive_logp_eps(V, 40.0))
        n = min(V, 20)
        assert (got[2][:, n:] == -1).all() and np.isnan(got[1][:, n:]).all()
        assert (got[2][:, :n] >= 0).all()


def test_skipped_rows_stay_untouched():
    V, B = 4099, 6
    logits, _, _ = sr.case(V, B)
    n_top = [-1, 20, -1, 0, 3, -1]
    lp = torch.full((B,), 7.0, device=DEV)
    tv = torch.full((B, K), 8.0, device=DEV)
    ti = torch.full((B, K), 9, dtype=torch.int64, device=DEV)
    tok = _tokens(logits, V)
    got = _run(logits.to(DEV), tok, n_top, logp=lp, topv=tv, topi=ti)
    for b in (0, 2, 5):
        assert got[0][b] == 7.0 and (got[1][b] == 8.0).all() \
            and (got[2][b] == 9).all()
    _check(got, logits, tok, n_top, lr.derive_logp_eps(V, 40.0))


def test_out_of_range_token_is_nan():
    V = 1000
    logits, _, _ = sr.case(V, 4)
    got = _run(logits.to(DEV), [-1, V, 2 ** 40, 5], [0, 1, 20, 20])
    assert np.isnan(got[0][:3]).all() and np.isfinite(got[0][3])


def test_degenerate_rows():
    """The row set of test_sampler_gpu.test_degenerate_rows: indices follow
    the rule, values are NaN where the contract says so, no index is out
    of range."""
    V = 4099
    inf, nan = float("inf"), float("nan")
    rows = torch.randn(5, V, generator=torch.Generator().manual_seed(5))
    rows[0] = nan
    rows[1, 2345] = inf
    rows[1, 3000] = inf
    rows[2] = -inf
    rows[2, 4098] = -3.0
    rows[3] = -inf
    rows[3, 77] = nan
    rows[4, ::2] = nan
    tok = [0, 2345, 4098, 77, 1]
    for dt in (torch.bfloat16, torch.float32):
        r = rows.to(dt)
        got = _run(r.to(DEV), tok, [20] * 5)
        _check(got, r, tok, [20] * 5, lr.derive_logp_eps(V, 40.0))
        assert (got[2][0] == -1).all()                  # nothing non-NaN
        assert got[2][1][:2].tolist() == [2345, 3000]   # m = +inf
        assert np.isnan(got[1][1]).all() and np.isnan(got[0][1])
        assert got[2][2][0] == 4098 and got[0][2] == 0.0
        assert got[2][2][1:].tolist() == list(range(19))    # -inf, by index
        assert (got[1][2][1:] == -inf).all()
        assert np.isnan(got[1][3]).all()                # nothing above -inf
        assert got[2][3].tolist() == [i for i in range(21) if i != 77][:20]
        assert (got[2][4] % 2 == 1).all()               # NaN never listed


def test_reproducible():
    V = 152064
    logits, _, _ = sr.case(V)
    dl = logits.to(DEV)
    tok = _tokens(logits, V)
    a = _run(dl, tok, [20] * sr.B)
    for _ in range(2):
        b = _run(dl, tok, [20] * sr.B)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_row_sampler_fused_matches_torch_path():
    """RowSampler on CUDA logits, fused against fused off: same tokens, the
    same top indices on tie-free f32 logits, logprobs of both paths within
    their bounds of the fp64 reference and of each other."""
    V = 4099
    rows = [dict(temperature=0.7, top_k=50, top_p=0.9, logprobs=True,
                 top_logprobs=5),
            dict(logprobs=True, top_logprobs=20),
            dict(temperature=1.0),
            dict(logprobs=True),
            dict(temperature=1.3, top_p=0.5, logprobs=True, top_logprobs=1),
            dict()]
    B = len(rows)
    for seed in range(4242, 4342):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(B, V, generator=g) * 3
        if all(len(torch.unique(r)) == V for r in logits):
            break
    else:
        raise AssertionError("no tie-free logits")
    L = max(lr.spread(r.numpy()) for r in logits)
    eps = lr.derive_logp_eps(V, L)
    # the torch path: f32 rounding of l - lse, lse itself (exp to 1 ulp, a
    # sum of V positive terms in an unknown order: (V - 1) u at worst, the
    # log to 1 ulp) and the subtraction
    u = 2.0 ** -24
    eps_torch = (V + 2) * u + 2 * u * (L + math.log(V))
    sams = []
    for fused in (True, False):
        rs = RowSampler(B, device=DEV, vocab=V)
        rs.fused = fused
        for b, c in enumerate(rows):
            rs.set_row(b, DecodingConfig(**c),
                       seed=11 + b if c.get("temperature") else None)
        sams.append(rs)
    fus, tor = sams
    dl = logits.to(DEV)
    # the uniforms both samplers draw for their seeded rows
    gens = {b: torch.Generator(device=DEV).manual_seed(11 + b)
            for b, c in enumerate(rows) if c.get("temperature")}
    eps_s = sr.derive_eps(V)
    n_top = [(c.get("top_logprobs", 0) if c.get("logprobs") else -1)
             for c in rows]
    same = 0
    for step in range(3):
        a, t = fus.sample(dl).cpu().numpy(), tor.sample(dl).cpu().numpy()
        for b, c in enumerate(rows):
            if b in gens:     # equal wherever the reference has one answer
                u = float(torch.rand(1, 1, device=DEV, generator=gens[b]))
                r = sr.row_reference(logits[b].numpy(), c["temperature"],
                                     c.get("top_k", 0), c.get("top_p", 1.0),
                                     0.0)
                if r["margin"] <= eps_s or sr.near_step(r, u, eps_s):
                    continue
            assert a[b] == t[b], (step, b, a[b], t[b])
            same += 1
        want = lr.reference(logits.numpy(), a, n_top, K)
        want_t = lr.reference(logits.numpy(), t, n_top, K)
        flp, tlp = fus.last_logp.cpu().numpy(), tor.last_logp.cpu().numpy()
        assert fus.last_topi.shape == tor.last_topi.shape == (B, K)
        for b, w in enumerate(want):
            if w is None:
                continue
            assert abs(flp[b] - w[0]) <= eps, (b, flp[b], w[0])
            assert abs(tlp[b] - want_t[b][0]) <= eps_torch
            n = n_top[b]
            assert torch.equal(fus.last_topi[b, :n], tor.last_topi[b, :n])
            assert np.array_equal(fus.last_topi[b].cpu().numpy()[:n],
                                  w[2][:n])
            assert lr.close(fus.last_topv[b, :n].cpu().numpy(), w[1][:n], eps)
            assert (fus.last_topv[b, :n] - tor.last_topv[b, :n]).abs().max(
                ).item() <= eps + eps_torch if n else True
    assert same >= 3 * B - 2
    # an all-greedy batch takes the kernel too
    rs = RowSampler(2, device=DEV, vocab=V)
    rs.set_row(0, DecodingConfig(logprobs=True, top_logprobs=3))
    rs.set_row(1, DecodingConfig())
    tok = rs.sample(dl[:2])
    assert torch.equal(tok, dl[:2].argmax(-1))
    w = lr.row_reference(logits[0].numpy(), int(tok[0]), 3, 3)
    assert abs(float(rs.last_logp[0]) - w[0]) <= eps
    assert rs.last_topi[0].tolist() == w[2].tolist()
    # nobody wants logprobs: nothing is computed
    rs.set_row(0, DecodingConfig())
    rs.sample(dl[:2])
    assert rs.last_logp is None and rs.last_topi is None


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sampler_logprobs_take_the_kernel(dtype, monkeypatch):
    """Sampler (first token of a slot, serial path) on GPU logits as the
    callers hold them: logprobs come from the kernel on those logits, not
    from float() + logsumexp + topk."""
    V, B = 4099, 4
    logits, _, _ = sr.case(V, B, "bf16" if dtype == torch.bfloat16 else "f32")
    dl = logits.to(DEV)
    seen_dtypes = []
    real = ops.logprobs_rows

    def spy(lg, *a, **k):
        seen_dtypes.append(lg.dtype)
        return real(lg, *a, **k)

    monkeypatch.setattr(ops, "logprobs_rows", spy)
    monkeypatch.setattr(torch, "topk", None)      # the torch path would trip
    tok, lp, tops = Sampler(DecodingConfig(logprobs=True, top_logprobs=5)
                            ).sample(dl)
    assert seen_dtypes == [dtype]
    tok = tok.cpu().numpy()
    assert np.array_equal(tok, logits.double().argmax(-1).numpy())
    want = lr.reference(logits.float().numpy(), tok, [5] * B, 5)
    eps = lr.derive_logp_eps(V, 40.0)
    for b, w in enumerate(want):
        assert abs(float(lp[b]) - w[0]) <= eps
        assert list(tops[b]) == w[2].tolist()     # ordered, ties decided
        assert lr.close(np.array(list(tops[b].values())), w[1], eps)
    # logprobs without a top list
    tok, lp, tops = Sampler(DecodingConfig(logprobs=True)).sample(dl)
    assert tops is None and abs(float(lp[0]) - want[0][0]) <= eps

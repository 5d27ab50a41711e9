"""Attention decode / prefill, split-S combine and fused RoPE + KV append
against fp64 references (tests/attn_reference.py) with derived bounds.

Every checker takes a ``device``: "cuda" runs the HIP kernels (marked
``gpu``), "cpu" runs dnet_amd.ops' fp32 reference path through the very
same inputs, reference and bounds — so a machine without a GPU still
proves that the three are consistent. Each case prints its worst
err/tol ratio (1.0 is the limit) so the log records the headroom.
"""
import itertools
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import attn_reference as ar
import dnet_amd.ops as ops
from dnet_amd.ops import reference as ref

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
CUDA_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
BF16 = torch.bfloat16


def _report(name, ratio):
    print(f"[err/tol] {name}: {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err/tol = {ratio:.3f} > 1"


# ------------------------------------------------------- a. attn_decode

DECODE_CASES = ar.decode_cases()


def test_decode_case_matrix_covers_the_axes():
    """The pruned matrix keeps what it promises: all pairs of axis values,
    and every sinks x window combination on an int8 cache at splits > 1."""
    cs = DECODE_CASES
    assert 50 <= len(cs) <= 75, len(cs)
    keys = ["dims", "int8", "splits", "pos", "window", "sinks"]
    vals = [ar.DECODE_DIMS, [False, True], ar.DECODE_SPLITS, ar.DECODE_POS,
            ar.DECODE_WINDOWS, ar.SINK_KINDS]
    for (ka, va), (kb, vb) in itertools.combinations(zip(keys, vals), 2):
        for a, b in itertools.product(va, vb):
            assert any(c[ka] == a and c[kb] == b for c in cs), (ka, a, kb, b)
    for sk, w in itertools.product(ar.SINK_KINDS, ar.DECODE_WINDOWS):
        assert any(c["sinks"] == sk and c["window"] == w and c["int8"]
                   and c["splits"] > 1 for c in cs), (sk, w)
    assert len({c["seed"] for c in cs}) == len(cs)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", DECODE_CASES, ids=ar.case_id)
def test_attn_decode_matrix(case, device, monkeypatch):
    monkeypatch.setenv("DNET_ATTN_SPLITS", str(case["splits"]))
    ratio, got, _ = ar.run_decode_case(case, device)
    _report(ar.case_id(case), ratio)
    for b, ln in enumerate(case["pos"]):
        if ln == 0:     # nothing to attend: exactly zero, sinks or not
            assert got[b].float().abs().max().item() == 0.0


@pytest.mark.parametrize("device", DEVICES)
def test_attn_decode_natural_splits(device, monkeypatch):
    """DNET_ATTN_SPLITS unset: B=1, Hkv=1, Smax=1024 splits in two."""
    monkeypatch.delenv("DNET_ATTN_SPLITS", raising=False)
    c = ar.NATURAL_CASE
    assert ops._attn_splits(len(c["pos"]), c["dims"][3], c["smax"]) == 2
    ratio, _, _ = ar.run_decode_case(c, device)
    _report("natural-splits", ratio)


@pytest.mark.parametrize("device", CUDA_ONLY)
@pytest.mark.parametrize("d,hq,hkv", [(128, 17, 1), (96, 4, 2)])
def test_attn_decode_rejects_unsupported(d, hq, hkv, device):
    """A GQA group above 16 and an uninstantiated head dim must raise,
    not launch."""
    q = torch.zeros(1, hq, d, dtype=BF16, device=device)
    kc = torch.zeros(1, hkv, 64, d, dtype=BF16, device=device)
    pos = torch.tensor([3], dtype=torch.int32, device=device)
    with pytest.raises(RuntimeError):
        ops.attn_decode(q, kc, kc.clone(), pos, d ** -0.5)


# ------------------------------- b. attn_decode_partials + attn_combine

def _kv(shape, gen, device, int8):
    x = torch.randn(*shape, generator=gen).to(BF16)
    if int8:
        c, s = ref.quantize_kv_rows(x)
        return c.to(device), s.to(device)
    return x.to(device), None


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("use_sinks", [False, True])
@pytest.mark.parametrize("d,dv,hq,hkv,int8,splits", [
    (128, 128, 8, 2, False, 1), (128, 128, 8, 2, True, 2),
    (64, 64, 8, 2, False, 2), (64, 64, 16, 1, True, 1),
    (192, 128, 4, 1, False, 1), (192, 128, 4, 1, True, 4)])
def test_partials_combine_two_shards(d, dv, hq, hkv, int8, splits, use_sinks,
                                     device, monkeypatch):
    """Sequence-sharded decode: per-shard partials, concatenated and merged
    by attn_combine, equal full attention. Shard 1 is empty for two of the
    three sequences; rows past each local length are poisoned."""
    monkeypatch.setenv("DNET_ATTN_SPLITS", str(splits))
    gen = torch.Generator().manual_seed(31 + d + hq + int8)
    B, cap = 3, 128
    pos = torch.tensor([250, 45, 128], dtype=torch.int32)
    q = torch.randn(B, hq, d, generator=gen).to(BF16).to(device)
    k, ks = _kv((B, hkv, 2 * cap, d), gen, device, int8)
    v, vs = _kv((B, hkv, 2 * cap, dv), gen, device, int8)
    sinks = (torch.randn(hq, generator=gen).to(BF16).to(device)
             if use_sinks else None)
    scale = d ** -0.5
    out, out_abs = ar.attn_ref(q, k, v, pos, scale, 0, sinks, kscale=ks,
                               vscale=vs)
    parts = []
    for r in range(2):
        sl = slice(r * cap, (r + 1) * cap)
        ln = (pos - r * cap).clamp(0, cap).to(torch.int32)
        kr, vr = k[:, :, sl].contiguous(), v[:, :, sl].contiguous()
        ksr = vsr = None
        if int8:
            ksr, vsr = ks[:, :, sl].contiguous(), vs[:, :, sl].contiguous()
        for b in range(B):
            poison = (ksr, vsr) if int8 else (kr, vr)
            for t in poison:
                t[b, :, int(ln[b]):] = float("nan")
        p = ops.attn_decode_partials(q, kr, vr, ln.to(device), scale, ksr, vsr)
        assert p.shape[:2] == (B, hq) and p.shape[3] == dv + 2
        parts.append(p)
    got = ops.attn_combine(torch.cat(parts, dim=2), sinks)
    assert got.shape == (B, hq, dv)
    _report(f"combine d{d}v{dv} int8={int8} splits={splits} "
            f"sinks={use_sinks}", ar.worst_ratio(got, out, out_abs))


@pytest.mark.parametrize("device", CUDA_ONLY)
@pytest.mark.parametrize("use_sinks", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_combine_accepts_dead_shard_partials(d, use_sinks, device):
    """The torch partials of the windowed context-parallel path mark a
    shard entirely below the window with m = -inf, l = 0; the combine
    kernel (which starts its running max at -1e30) must ignore them."""
    from dnet_amd.parallel.context import _partials_windowed, local_lengths
    gen = torch.Generator().manual_seed(77 + d)
    B, hq, hkv, cap, window = 2, 8, 2, 64, 32
    pos = torch.tensor([100, 127])            # query positions (attend <=)
    q = torch.randn(B, hq, d, generator=gen).to(BF16).to(device)
    k = torch.randn(B, hkv, 2 * cap, d, generator=gen).to(BF16).to(device)
    v = torch.randn(B, hkv, 2 * cap, d, generator=gen).to(BF16).to(device)
    sinks = (torch.randn(hq, generator=gen).to(BF16).to(device)
             if use_sinks else None)
    scale = d ** -0.5
    parts = []
    for r in range(2):
        sl = slice(r * cap, (r + 1) * cap)
        ln = local_lengths((pos + 1).to(device), cap, r)
        parts.append(_partials_windowed(q, k[:, :, sl], v[:, :, sl], ln,
                                        scale, r * cap, pos.to(device),
                                        window))
    assert torch.isinf(parts[0][..., d]).all()      # shard 0 is dead
    assert (parts[0][..., d + 1] == 0).all()
    got = ops.attn_combine(torch.cat(parts, dim=2), sinks)
    assert torch.isfinite(got.float()).all()
    out, out_abs = ar.attn_ref(q, k, v, pos + 1, scale, window, sinks)
    _report(f"combine dead shard d{d} sinks={use_sinks}",
            ar.worst_ratio(got, out, out_abs))


# ------------------------------------------------ c. MFMA decode variant

@pytest.mark.parametrize("device", CUDA_ONLY)
def test_attn_decode_mfma_variant_in_child(device, monkeypatch):
    """DNET_ATTN_MFMA is latched on the first call of a process, so the
    MFMA decode kernel runs the whole case matrix in one fresh child. The
    only evidence that the other kernel ran is that its output bits differ
    from the scalar kernel's (bf16 P, another summation order). The child
    is started once; a signal, a timeout or a GPU fault fails the test."""
    monkeypatch.delenv("DNET_ATTN_SPLITS", raising=False)
    assert os.environ.get("DNET_ATTN_MFMA", "") != "1"
    _, got, _ = ar.run_decode_case(ar.NATURAL_CASE, device)
    parent_sum = ar.checksum(got)
    t0 = time.time()
    r = subprocess.run(
        [sys.executable, os.path.abspath(ar.__file__), "--decode-cases"],
        env={**os.environ, "DNET_ATTN_MFMA": "1"}, timeout=300,
        capture_output=True, text=True)
    print(f"[mfma child] {time.time() - t0:.1f} s of 300 s")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-2000:])
    lines = [json.loads(ln) for ln in r.stdout.splitlines()
             if ln.startswith("{")]
    assert len(lines) == len(DECODE_CASES) + 1
    worst = max(lines, key=lambda x: x["ratio"])
    print(f"[err/tol] mfma worst: {worst['ratio']:.3f} ({worst['case']})")
    bad = [x for x in lines if not x["ratio"] <= 1.0]
    assert not bad, bad
    assert lines[-1]["checksum"] != parent_sum, \
        "child output is bit-identical to the scalar kernel's"


# -------------------------------------------------------- d. rope_append

def _rope_setup(D, q8, wkind, device, gen):
    """Fused [B, (Hq+2Hkv)*D] buffer + sentinel-filled caches. Returns the
    pieces and, per batch row, the cache row that must be written (None =
    out of shard)."""
    B, Hq, Hkv, rows = 3, 4, 2, 48
    pos = torch.tensor([0, rows - 1, 20], dtype=torch.int32)
    if wkind == "none":
        smax, wpos, dst = rows, None, pos.tolist()
    else:
        smax = 16
        wpos = {"in": [3, 0, 15], "neg": [-1, 5, -1],
                "smax": [smax, 5, smax]}[wkind]
        dst = [w if 0 <= w < smax else None for w in wpos]
        wpos = torch.tensor(wpos, dtype=torch.int32)
    cos, sin = ops.rope_tables(rows, D, 10000.0)
    buf = torch.randn(B, (Hq + 2 * Hkv) * D, generator=gen).to(BF16)
    if q8:
        kc = torch.full((B, Hkv, smax, D), 77, dtype=torch.int8)
        ks = torch.full((B, Hkv, smax, D // 64), 3.0, dtype=BF16)
        vc, vs = kc.clone(), ks.clone()
    else:
        kc = torch.full((B, Hkv, smax, D), -7.0, dtype=BF16)
        vc, ks, vs = kc.clone(), None, None
    return dict(B=B, Hq=Hq, Hkv=Hkv, pos=pos, wpos=wpos, dst=dst, cos=cos,
                sin=sin, buf=buf, kc=kc, vc=vc, ks=ks, vs=vs)


def _check_cache(s, kc, vc, ks, vs, k_true, k_mag, v_true, v_exact):
    """Written rows hold k_true / v_true (fp64); every other row, scales
    included, is still the sentinel."""
    q8 = ks is not None
    kc, vc = kc.cpu(), vc.cpu()
    untouched = torch.ones(kc.shape[:3], dtype=torch.bool)
    for b, w in enumerate(s["dst"]):
        if w is None:
            continue
        untouched[b, :, w] = False
        if q8:
            ar.check_kv8(kc[b, :, w], ks.cpu()[b, :, w], k_true[b])
            ar.check_kv8(vc[b, :, w], vs.cpu()[b, :, w], v_true[b])
            continue
        err = (kc[b, :, w].double() - k_true[b]).abs()
        assert (err <= ar.rope_tol(k_true[b], k_mag[b])).all(), \
            float((err / ar.rope_tol(k_true[b], k_mag[b])).max())
        if v_exact:
            assert torch.equal(vc[b, :, w].double(), v_true[b])
        else:
            # bf16(f32(x + bias)): round-to-nearest is <= 2^-8 relative and
            # the f32 add can move a tie; one ulp (2^-7) holds both
            verr = (vc[b, :, w].double() - v_true[b]).abs()
            assert (verr <= 2.0 ** -7 * v_true[b].abs()).all()
    assert torch.equal(kc[untouched], s["kc"][untouched])
    assert torch.equal(vc[untouched], s["vc"][untouched])
    if q8:
        assert torch.equal(ks.cpu()[untouched], s["ks"][untouched])
        assert torch.equal(vs.cpu()[untouched], s["vs"][untouched])


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("wkind", ["none", "in", "neg", "smax"])
@pytest.mark.parametrize("q8", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_append(D, q8, wkind, device):
    gen = torch.Generator().manual_seed(5 + D + 2 * q8)
    s = _rope_setup(D, q8, wkind, device, gen)
    B, Hq, Hkv = s["B"], s["Hq"], s["Hkv"]
    buf = s["buf"].clone().to(device)
    q = buf[:, :Hq * D].view(B, Hq, D)
    k = buf[:, Hq * D:(Hq + Hkv) * D].view(B, Hkv, D)
    v = buf[:, (Hq + Hkv) * D:].view(B, Hkv, D)
    q0, k0, v0 = q.cpu().clone(), k.cpu().clone(), v.cpu().clone()
    dv = lambda t: None if t is None else t.clone().to(device)
    kc, vc, ks, vs = dv(s["kc"]), dv(s["vc"]), dv(s["ks"]), dv(s["vs"])
    ops.rope_append(q, k, v, kc, vc, s["pos"].to(device),
                    s["cos"].to(device), s["sin"].to(device), ks, vs,
                    wpos=dv(s["wpos"]))
    q_true, q_mag = ar.rope_ref(q0, s["cos"], s["sin"], s["pos"])
    k_true, k_mag = ar.rope_ref(k0, s["cos"], s["sin"], s["pos"])
    # q and k are rotated in place in the fused buffer, v is left alone
    assert ((q.cpu().double() - q_true).abs()
            <= ar.rope_tol(q_true, q_mag)).all()
    assert ((k.cpu().double() - k_true).abs()
            <= ar.rope_tol(k_true, k_mag)).all()
    assert torch.equal(v.cpu(), v0)
    _check_cache(s, kc, vc, ks, vs, k_true, k_mag, v0.double(), True)


# ---------------------------------------------------- e. rope_append_f32

@pytest.mark.parametrize("device", CUDA_ONLY)
@pytest.mark.parametrize("wkind", ["none", "neg"])
@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("q8", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_append_f32_scratch(D, q8, use_bias, wkind, device):
    """The split-k-fused variant reads q/k/v (f32, un-combined) from the
    shared scratch, adds the bias, and must hand the scratch back zeroed."""
    from dnet_amd.ops import _get_scratch, _native
    gen = torch.Generator().manual_seed(9 + D + 2 * q8 + 4 * use_bias)
    s = _rope_setup(D, q8, wkind, device, gen)
    B, Hq, Hkv = s["B"], s["Hq"], s["Hkv"]
    N = (Hq + 2 * Hkv) * D
    x = torch.randn(B, N, generator=gen)            # f32 GEMM result
    bias = torch.randn(N, generator=gen).to(BF16) if use_bias else None
    true = x.double() + (bias.double() if use_bias else 0.0)
    split = lambda t, a, b, h: t[:, a * D:b * D].reshape(B, h, D)
    q_true, q_mag = ar.rope_ref(split(true, 0, Hq, Hq), s["cos"], s["sin"],
                                s["pos"])
    k_true, k_mag = ar.rope_ref(split(true, Hq, Hq + Hkv, Hkv), s["cos"],
                                s["sin"], s["pos"])
    v_true = split(true, Hq + Hkv, Hq + 2 * Hkv, Hkv)
    dv = lambda t: None if t is None else t.clone().to(device)
    kc, vc, ks, vs = dv(s["kc"]), dv(s["vc"]), dv(s["ks"]), dv(s["vs"])
    scratch = _get_scratch(torch.device(device, 0))
    try:
        assert int(scratch.count_nonzero()) == 0, "scratch dirty on entry"
        scratch[:B * N] = x.reshape(-1).to(device)
        qout = torch.full((B, Hq, D), -7.0, dtype=BF16, device=device)
        _native().rope_append_f32(scratch, dv(bias), qout, Hkv, kc, vc,
                                  s["pos"].to(device), s["cos"].to(device),
                                  s["sin"].to(device), ks, vs, dv(s["wpos"]))
        assert int(scratch[:B * N].count_nonzero()) == 0, "not re-zeroed"
        assert int(scratch[B * N:].count_nonzero()) == 0, "wrote past B*N"
    finally:
        scratch.zero_()     # later split-k tests rely on it
    assert ((qout.cpu().double() - q_true).abs()
            <= ar.rope_tol(q_true, q_mag)).all()
    _check_cache(s, kc, vc, ks, vs, k_true, k_mag, v_true, False)


# ------------------------------------------------------- f. attn_prefill

PREFILL_DIMS = [(128, 128), (64, 64), (192, 128), (96, 96)]
PREFILL_T = [1, 15, 16, 17, 63, 64, 65]
PREFILL_QOFF = [0, 5, 32, 70]
PREFILL_WINDOWS = [0, 1, 31, 32, 33, 1000]


def _prefill_cases():
    axes = [PREFILL_DIMS, PREFILL_T, PREFILL_QOFF, PREFILL_WINDOWS,
            ar.SINK_KINDS]
    cases = [dict(dims=PREFILL_DIMS[d], T=PREFILL_T[t], q_off=PREFILL_QOFF[o],
                  window=PREFILL_WINDOWS[w], sinks=ar.SINK_KINDS[k], extra=0)
             for d, t, o, w, k in ar.pairwise(axes)]
    # keys past the last query (S > q_off + T), finite data
    cases.append(dict(dims=(128, 128), T=17, q_off=5, window=0,
                      sinks="randn", extra=40))
    cases.append(dict(dims=(64, 64), T=65, q_off=32, window=33,
                      sinks="none", extra=7))
    return cases


def _prefill_id(c):
    return (f"d{c['dims'][0]}v{c['dims'][1]}-T{c['T']}-o{c['q_off']}"
            f"-w{c['window']}-{c['sinks']}-x{c['extra']}")


def test_prefill_case_matrix_is_small_and_complete():
    cs = _prefill_cases()
    assert set(PREFILL_DIMS) == ops._PREFILL_DIMS
    assert 40 <= len(cs) <= 60, len(cs)
    for t, w in itertools.product(PREFILL_T, PREFILL_WINDOWS):
        assert any(c["T"] == t and c["window"] == w for c in cs)


@pytest.mark.parametrize("device", CUDA_ONLY)
@pytest.mark.parametrize("case", _prefill_cases(), ids=_prefill_id)
def test_attn_prefill_vs_fp64(case, device):
    """Flash prefill (causal + window + sinks, GQA G=5) vs fp64."""
    D, DV = case["dims"]
    B, Hq, Hkv, T, q_off = 2, 10, 2, case["T"], case["q_off"]
    S = q_off + T + case["extra"]
    gen = torch.Generator().manual_seed(D + 7 * T + q_off + case["window"])
    q = torch.randn(B, Hq, T, D, generator=gen).to(BF16).to(device)
    k = torch.randn(B, Hkv, S, D, generator=gen).to(BF16).to(device)
    v = torch.randn(B, Hkv, S, DV, generator=gen).to(BF16).to(device)
    sinks = ar.make_sinks(case["sinks"], Hq, gen)
    if sinks is not None:
        sinks = sinks.to(device)
    scale = D ** -0.5
    got = ops.attn_prefill(q, k, v, scale, q_off, case["window"], sinks)
    out, out_abs = ar.attn_ref(q, k, v, None, scale, case["window"], sinks,
                               q_off=q_off)
    assert got.shape == (B, Hq, T, DV)
    _report(_prefill_id(case), ar.worst_ratio(got, out, out_abs))

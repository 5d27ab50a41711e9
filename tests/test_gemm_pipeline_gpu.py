"""The pipelined K loop of the streamed int8/int4 decode GEMM
(gemm_m16_stream_kernel): prologue, steady state, epilogue and the short
last tile, at spans the sweep in test_gemm_gpu.py does not reach (it stops
at K = 2048 under deep default splits, so a block rarely sees more than two
full tiles).

With DNET_GEMM_SPLITK=1 the span of every block is K itself: 1 to 5 full
256-k tiles, each with and without a 64/128/192-k remainder. One-hot inputs
make every check exact; the generic kernel (DNET_GEMM_NOSTREAM=1), which
runs the same products in the same order, must give the same bits on
random data too. The switches are latched per process, so those runs are
children of this module (``python tests/test_gemm_pipeline_gpu.py
--child``), one after another, each under a time limit.
"""
import functools
import itertools
import json
import os
import subprocess
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_reference as gr  # noqa: E402

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
CUDA_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
BF16 = torch.bfloat16

K_G128 = (256, 384, 512, 640, 768, 896, 1024, 1280, 1408)
K_G64 = K_G128 + (320, 576, 832, 1216)      # 64-k and 192-k remainders
K_INT4 = (256, 640, 1024, 1408)
SPAN_M = (3, 17, 64)                        # one per MT tier
SPAN_N = 72                                 # the second block has OOB waves


@functools.lru_cache(maxsize=None)
def _span_cases() -> tuple:
    cs = []
    for fmt, g, ks in (("int8", 128, K_G128), ("int8", 64, K_G64),
                       ("int4", 128, K_INT4)):
        for k, m in itertools.product(ks, SPAN_M):
            cs.append(gr._case(fmt, m, SPAN_N, k, g))
    for i, c in enumerate(cs):
        c["seed"] = 6000 + i
    return tuple(cs)


def span_cases() -> list:
    return [dict(c) for c in _span_cases()]


SPAN_CASES = span_cases()


# ---------------------------------------------- default policy, in process

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", SPAN_CASES, ids=gr.case_id)
def test_span_onehot_default_policy(case, device):
    """x = rows of I_K under the default split policy: every k of every
    row of W comes back as bf16(q*s), exactly."""
    bad, got = gr.run_onehot(case, device)
    print(f"[err/tol] onehot {gr.case_id(case)}: "
          f"{'0.000' if bad == 0 else 'inf'} ({bad} of {got.numel()} differ)")
    assert bad == 0, f"{bad} of {got.numel()} elements differ"


@pytest.mark.parametrize("device", CUDA_ONLY)
def test_default_policy_splits_some_spans(device):
    """The default policy splits K = 1280 in two and leaves K = 1408
    whole, so the in-process sweep covers both kinds."""
    import dnet_amd.ops as ops
    scratch = ops._get_scratch(torch.device(device, 0)).numel()
    split = [gr.case_id(c) for c in SPAN_CASES if gr.splits_k(c)]
    print(f"[spans] {len(split)} of {len(SPAN_CASES)} cases split K")
    assert split and len(split) < len(SPAN_CASES)
    for m in SPAN_M:
        assert ops._will_defer(m, SPAN_N, 1280, 128, 8, scratch)
        assert not ops._will_defer(m, SPAN_N, 1408, 128, 8, scratch)


# ----------------------------------------- reproducible mode across splits

@pytest.fixture
def reproducible_mode():
    import dnet_amd.ops as ops
    ops.set_reproducible(True)
    try:
        yield
    finally:
        ops.set_reproducible(False)


@pytest.mark.parametrize("device", CUDA_ONLY)
@pytest.mark.parametrize("k", [1280, 2048])
@pytest.mark.parametrize("fmt", ["int8", "int4"])
def test_reproducible_mode_across_splits(fmt, k, device, reproducible_mode):
    """Four launches give the same bits, within tol + 2^-12 (at most 32
    splits x 2^-17 grid rounding)."""
    c = dict(gr._case(fmt, 64, SPAN_N, k, 128), seed=6500 + k)
    assert gr.splits_k(c), "shape no longer splits K"
    x, w, bias = gr.build_case(c)
    r64, mag = gr.case_reference(c, x, w, bias, device)
    assert float(r64.abs().max()) < 2.0 ** 8
    outs = [gr.gemm_call(w, x, bias, device) for _ in range(4)]
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    r = gr.ratio(outs[0], r64, gr.gemm_tol(r64, mag, k, 2.0 ** -12))
    print(f"[err/tol] reproducible {gr.case_id(c)}: {r:.3f}")
    assert r <= 1.0


# ------------------------------------------------------ stale image rows

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("m", SPAN_M)
def test_short_tile_ignores_stale_image(m, device):
    """K = 320 at G = 64 is one full tile and a 64-k remainder: three
    quarters of the last image are never staged. Every launch follows one
    of the same M whose x is all NaN, so whatever a short tile read past
    its own columns would show."""
    k = 320
    c = dict(gr._case("int8", m, SPAN_N, k, 64), seed=6600 + m)
    gen = torch.Generator().manual_seed(c["seed"])
    w = gr.make_weights("int8", SPAN_N, k, 64, gen)
    wd = dict(w, packed=w["packed"].to(device), plain=w["plain"].to(device),
              scales=w["scales"].to(device))
    launches = -(-k // m)
    eye = torch.zeros(launches * m, k, dtype=BF16)
    eye[:k] = torch.eye(k, dtype=BF16)
    eye = eye.to(device)
    nan_w = gr.make_weights("int8", SPAN_N, 512, 64, gen)
    nan_wd = dict(nan_w, packed=nan_w["packed"].to(device),
                  plain=nan_w["plain"].to(device),
                  scales=nan_w["scales"].to(device))
    nan_x = torch.full((m, 512), float("nan"), dtype=BF16, device=device)
    outs = []
    for j in range(launches):
        poisoned = gr.gemm_call(nan_wd, nan_x, None, device)
        assert bool(torch.isnan(poisoned.float()).all())
        outs.append(gr.gemm_call(wd, eye[j * m:(j + 1) * m], None, device))
    got = torch.cat(outs).cpu()
    want = torch.zeros(launches * m, SPAN_N, dtype=BF16)
    want[:k] = gr.contract_weights(w).to(BF16).t()
    assert torch.isfinite(got.float()).all()
    bad = int((got.float() != want.float()).sum())
    assert bad == 0, f"{bad} of {got.numel()} elements differ"


# ------------------------------------------- children: span = K, two kernels

def run_child_cases(device: str = "cuda") -> list:
    """One record per case: the one-hot sweep (ratio 0 if exact, else inf)
    and the same shapes on random data (err/tol), with the output bits'
    checksum and whether K is split in this process."""
    out = []
    for c in span_cases():
        bad, got = gr.run_onehot(c, device)
        out.append({"case": "onehot:" + gr.case_id(c),
                    "ratio": 0.0 if bad == 0 else float("inf"),
                    "split": bool(gr.splits_k(c)),
                    "checksum": gr.checksum(got)})
        r, got = gr.run_case(c, device)
        out.append({"case": "random:" + gr.case_id(c), "ratio": r,
                    "split": bool(gr.splits_k(c)),
                    "checksum": gr.checksum(got)})
    return out


_CHILD_DIED = []        # children that ended on a signal or a timeout
CHILD_LIMIT = 300


@pytest.fixture(autouse=True)
def _no_gpu_work_after_a_dead_child(request):
    """A child that died on a signal or ran into its time limit may have
    faulted the GPU: start nothing more on it from this module."""
    if _CHILD_DIED and "gpu" in request.keywords:
        pytest.fail(f"not started: child {_CHILD_DIED[0]} died earlier")


@functools.lru_cache(maxsize=None)
def _child_records(variables: tuple) -> dict:
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("DNET_GEMM_")}
    env.update(dict(v.split("=") for v in variables))
    name = " ".join(variables)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__),
                            "--child"], env=env, timeout=CHILD_LIMIT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(name)
        raise
    print(f"[{name} child] {time.time() - t0:.1f} s of {CHILD_LIMIT} s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _CHILD_DIED.append(name)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-2000:])
    recs = [json.loads(ln) for ln in r.stdout.splitlines()
            if ln.startswith("{")]
    assert len(recs) == 2 * len(SPAN_CASES)
    return {x["case"]: x for x in recs}


STREAM_CHILD = ("DNET_GEMM_SPLITK=1",)
GENERIC_CHILD = ("DNET_GEMM_SPLITK=1", "DNET_GEMM_NOSTREAM=1")


def _check_child(recs: dict, name: str):
    assert not [x["case"] for x in recs.values() if x["split"]], \
        "DNET_GEMM_SPLITK=1 must leave every K whole"
    for kind in ("onehot", "random"):
        worst = max((x for x in recs.values() if x["case"].startswith(kind)),
                    key=lambda x: x["ratio"])
        print(f"[err/tol] {name} {kind} worst: {worst['ratio']:.3f} "
              f"({worst['case']})")
    bad = [x for x in recs.values() if not x["ratio"] <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("device", CUDA_ONLY)
def test_unsplit_spans_streamed_child(device):
    """Span = K through the pipelined kernel: the one-hot sweep is exact
    and the random cases meet gemm_tol."""
    assert not [k for k in os.environ if k.startswith("DNET_GEMM_")]
    _check_child(_child_records(STREAM_CHILD), "streamed")


@pytest.mark.parametrize("device", CUDA_ONLY)
def test_unsplit_spans_same_bits_as_generic_child(device):
    """The generic kernel takes the same products in the same order:
    every case, one-hot and random, must give the streamed kernel's bits."""
    assert not [k for k in os.environ if k.startswith("DNET_GEMM_")]
    stream = _child_records(STREAM_CHILD)
    generic = _child_records(GENERIC_CHILD)
    _check_child(generic, "generic")
    assert stream.keys() == generic.keys()
    diff = [c for c in stream if stream[c]["checksum"] != generic[c]["checksum"]]
    print(f"[same bits] {len(stream) - len(diff)} of {len(stream)} cases "
          f"bit-identical between the streamed and the generic kernel")
    assert not diff, diff


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    if "--child" in sys.argv[1:]:
        for rec in run_child_cases("cuda"):
            print(json.dumps(rec), flush=True)
        torch.cuda.synchronize()
        sys.exit(0)
    sys.exit("usage: test_gemm_pipeline_gpu.py --child")

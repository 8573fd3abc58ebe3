"""GPU: the per-clip attention kernels (csrc/attention_clip.hip: forward, query-owner dQ, key-owner dK/dV; fp32 and bf16
storage) through the C ABI on the masks, score ranges and shapes that random Gaussian inputs with an independent random
mask never produce.  tests/clip_walk.py defines the cases; tests/test_clip_walk_cpu.py shows, without a GPU, which tile paths
each of them takes and which mutation of the forward walk each would catch.

  masks    lead-empty (whole leading key tiles invisible before a query has seen a key: the m_use = 0 path), prefix-64
           (the production padding pattern: a whole tile masked after the first; d = 128), all-invalid, one-slot,
           non-binary (`valid` values other than 0 and 1: visible iff > 0)
  scores   alt-x5 (|s| ~ 100), late-max (the running maximum arrives in the last tile), first-max (it arrives in the first:
           alpha == 1 on every lane, the rescale is skipped ever after) - with valid = NULL and a prefix mask
  shapes   N = 1, T = 1, N > 128, T = 64 - with valid = NULL and a random mask

fp32 goes through test_hip_layout_ops._clip_run (sentinel-filled buffers with guards), bf16 through
test_hip_clip_attention_bf16.run (bf16-representable inputs, NaN prefill).  The reference is oracle.clip_attention with
autograd in fp64 plus lse_want; the bars are the two modules' own, unchanged: vs_cpu32 and lse within 1e-5 (1 + |lse|) in
fp32; out rel-L2 1e-2 / 2^-6 of the largest value, gradients 2e-2 / 6e-2, lse 1e-5 in bf16.  bf16_model evaluates the bf16
kernels' documented rounding points in fp64 on the CPU (step_stages.clip_attention_fwd / _bwd with rnd = bf, O and dqkv
rounded once on store); its error against fp64 is printed next to the kernel's (DESIGN.md records both).

Exact checks: all-invalid (every token sees only itself: out == v, dv == dout bit for bit; dq, dk zero up to the difference
between two fp32 evaluations of one 64-term dot product) and the masks_are_exact pattern on the structured masks.
"""
import pytest
import torch

import clip_walk as W
import step_stages as SS
from helpers import vs_cpu32
from oracle import layout_spec as O
from test_hip_clip_attention_bf16 import lse_want, rel_l2, run as run_bf16
from test_hip_layout_ops import _clip_run
from test_hip_pixel_ops import within

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def case(name, bf16):
    """inputs and references of a case, computed once per storage: in = (qkv, gy, valid), out / grad in fp64 and by
    torch-CPU fp32, lse in fp64.  The bf16 kernels get (and are judged on) the inputs rounded to bf16."""
    key = (name, bf16)
    if key not in _REF:
        qkv, gy, valid = W.make_case(name)
        if bf16:
            qkv, gy = qkv.bfloat16().float(), gy.bfloat16().float()
        heads = qkv.shape[-1] // 192
        r = {"in": (qkv, gy, valid), "lse": lse_want(qkv, valid, heads)}
        for dt in (torch.float64, torch.float32):
            q = qkv.detach().to(dt, copy=True).requires_grad_(True)
            o = O.clip_attention(q, heads, valid.to(dt) if valid is not None else None)
            o.backward(gy.to(dt))
            r[dt] = (o.detach(), q.grad)
        _REF[key] = r
    return _REF[key]


def bf16_model(name):
    """{out, dqkv} (B,T,N,.) of the bf16 kernels' rounding points evaluated in fp64: P and dS rounded to bf16 as matrix
    operands, O and dQ / dK / dV rounded once on store, the backward reading the stored O and the saved lse."""
    qkv, gy, valid = case(name, True)["in"]
    B, T, N, _ = qkv.shape
    rows = SS.to_rows(qkv.double())
    v = valid.double() if valid is not None else None
    out, lse = SS.clip_attention_fwd(rows, v, B, T, N, rnd=SS.bf)
    out = SS.bf(out)
    dqkv, _ = SS.clip_attention_bwd(rows, SS.to_rows(gy.double()), out, lse, v, B, T, N, rnd=SS.bf)
    return {"out": SS.from_rows(out, B, T, N), "dqkv": SS.from_rows(SS.bf(dqkv), B, T, N)}


# dq and dk of all-invalid are exactly zero in fp64 and in torch-CPU fp32: no relative bar applies (vs_cpu32's would be 0, a
# rel-L2 divides by 0); test_clip_attention_all_invalid_is_the_identity holds them to the dot-product bound instead
ZERO_GRADIENTS = (("all-invalid", "dq"), ("all-invalid", "dk"))


def _parts(t, d):
    return (("dq", t[..., :d]), ("dk", t[..., d:2 * d]), ("dv", t[..., 2 * d:]))


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_clip_attention_edges_fp32(H, dev, name):
    r = case(name, False)
    qkv, gy, valid = r["in"]
    d = qkv.shape[-1] // 3
    got = _clip_run(H, dev, qkv, gy, valid)
    want, cpu = r[torch.float64], r[torch.float32]
    pairs = [("out", got["out"], want[0], cpu[0])]
    pairs += [(n, g, w, c) for (n, g), (_, w), (_, c) in zip(_parts(got["dqkv"], d), _parts(want[1], d), _parts(cpu[1], d))]
    pairs = [x for x in pairs if (name, x[0]) not in ZERO_GRADIENTS]
    lerr = (got["lse"].double() - r["lse"]).abs() / (1 + r["lse"].abs())
    print("\nfp32 %s: " % name + ", ".join("%s %.1e (bar %.1e)" % (
        n, float((g.double() - w).abs().max()), 4 * float((c.double() - w).abs().max()) + 2.0 ** -20 * float(w.abs().max()))
        for n, g, w, c in pairs) + ", lse %.1e (bar 1.0e-05)" % float(lerr.max()))
    assert bool(torch.isfinite(got["delta"]).all()), "delta not fully written"
    for n, g, w, c in pairs:
        vs_cpu32(g, w, c, "clip " + n)
    within(got["lse"], r["lse"], 1e-5 * (1 + r["lse"].abs()), "clip lse")


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_clip_attention_edges_bf16(H, name):
    r = case(name, True)
    qkv, gy, valid = r["in"]
    B, T, N, d3 = qkv.shape
    d = d3 // 3
    got = run_bf16(H, qkv, gy, valid, B, T, N, d)
    model = bf16_model(name)
    want = r[torch.float64]
    pairs = [("out", got["out"], model["out"], want[0], 1e-2, 2.0 ** -6)]
    pairs += [(n, g, m, w, 2e-2, 6e-2) for (n, g), (_, m), (_, w) in
              zip(_parts(got["dqkv"], d), _parts(model["dqkv"], d), _parts(want[1], d))]
    pairs = [x for x in pairs if (name, x[0]) not in ZERO_GRADIENTS]
    lerr = float((got["lse"].double() - r["lse"]).abs().max())
    print("\nbf16 %s: " % name + ", ".join("%s rel-L2 %.1e max %.1e (model %.1e %.1e; bars %.0e %.1e)" % (
        n, rel_l2(g, w), float((g.double() - w).abs().max()), rel_l2(m, w), float((m - w).abs().max()), b2,
        bm * float(w.abs().max())) for n, g, m, w, b2, bm in pairs) + ", lse %.1e" % lerr)
    for k in ("out", "lse", "delta", "dqkv"):
        assert bool(torch.isfinite(got[k]).all()), k + " not fully written"
    assert torch.allclose(got["lse"].double(), r["lse"], rtol=1e-5, atol=1e-5), lerr
    for n, g, m, w, b2, bm in pairs:
        e = rel_l2(g, w)
        assert e <= b2, (n, "rel L2", e)
        worst = float((g.double() - w).abs().max())
        assert worst <= bm * float(w.abs().max()), (n, "max err", worst)


def _runner(H, dev, bf16):
    if bf16:
        return lambda qkv, gy, valid: run_bf16(H, qkv, gy, valid, *qkv.shape[:3], qkv.shape[-1] // 3)
    return lambda qkv, gy, valid: _clip_run(H, dev, qkv, gy, valid)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_clip_attention_all_invalid_is_the_identity(H, dev, bf16):
    """valid = 0 everywhere: every token sees only itself.  P is exactly 1 and every other product is 0 x finite, so
    out == v and dv == dout bit for bit; lse is the token's own log2 score; dS = P (dP - delta) / 8 is the difference
    between two fp32 evaluations of the same 64-term dot product <v, dO> (the tile product and delta), so
    |dq_j| <= 0.125 * 64 * 2^-23 * sum_i |v_i dO_i| * |k_j| (dk: |q_j|), x 1.02 for the two bf16 roundings."""
    qkv, gy, valid = case("all-invalid", bf16)["in"]
    d = qkv.shape[-1] // 3
    got = _runner(H, dev, bf16)(qkv, gy, valid)
    for k in ("out", "lse", "delta", "dqkv"):
        assert bool(torch.isfinite(got[k]).all()), k + " not fully written"
    q, k, v = (t.double() for t in qkv.split(d, dim=-1))
    own = (q * k).sum(-1).reshape(-1) * (W.LOG2E / 8.0)               # one head, one clip: (b, head, token) is the token
    within(got["lse"], own, 1e-5 * (1 + own.abs()), "lse of a token that sees itself")
    bound = 0.125 * 64 * 2.0 ** -23 * (v * gy.double()).abs().sum(-1, keepdim=True) * (1.02 if bf16 else 1.0)
    dq, dk, dv = (t for _, t in _parts(got["dqkv"], d))
    print("\n%s all-invalid: max |dq| / bound %.3f, |dk| / bound %.3f" % (
        "bf16" if bf16 else "fp32", float((dq.double().abs() / (bound * k.abs())).max()),
        float((dk.double().abs() / (bound * q.abs())).max())))
    within(dq, torch.zeros_like(q), bound * k.abs(), "dq")
    within(dk, torch.zeros_like(q), bound * q.abs(), "dk")
    assert torch.equal(got["out"], qkv[..., 2 * d:]), "out != v"
    assert torch.equal(dv, gy), "dv != dout"


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["lead-empty", "prefix-64", "one-slot"])
def test_clip_attention_structured_masks_are_exact(H, dev, name, bf16):
    """No tolerance: two identical calls agree bit for bit, and overwriting q, k, v of every padded slot leaves out and dq
    of every valid token unchanged."""
    qkv, gy, valid = case(name, bf16)["in"]
    d = qkv.shape[-1] // 3
    call = _runner(H, dev, bf16)
    base, again = call(qkv, gy, valid), call(qkv, gy, valid)
    for k in ("out", "lse", "delta", "dqkv"):
        assert bool(torch.isfinite(base[k]).all()), k + " not fully written"
        assert torch.equal(base[k], again[k]), k + " is not reproducible"
    pad = valid == 0
    assert bool(pad.any()) and bool((~pad).any())
    q2 = qkv.clone()
    junk = torch.randn(int(pad.sum()), 3 * d, generator=torch.Generator().manual_seed(5)) * 3.0
    q2[pad] = junk.bfloat16().float() if bf16 else junk
    got = call(q2, gy, valid)
    keep = ~pad
    assert torch.equal(got["out"][keep], base["out"][keep]), "a padded slot's q, k, v reached a valid token's output"
    assert torch.equal(got["dqkv"][..., :d][keep], base["dqkv"][..., :d][keep]), "... a valid token's dq"
    assert not torch.equal(got["out"][pad], base["out"][pad])

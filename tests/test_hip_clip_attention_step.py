"""GPU: vlg_attention_clip_step / _bf16 - per-clip attention of the N queries of ONE frame p against the K/V cache - through
the C ABI, against tests/clip_step_ref.py (oracle.clip_attention on frames 0 .. p) in fp64.

Poison in every call unless said otherwise: the qkv rows of positions > p and valid[:, > p] hold NaN (neither may be read,
and the tail of the last 32-key tile must reach neither a load nor the P.V product), the output has a leading dimension
larger than d, more rows than B*N, and starts as NaN sentinels: the pad columns and the extra rows must stay NaN.

Bars, the project's own: fp32 helpers.vs_cpu32 (4 x torch-CPU fp32's own error against fp64 + 2^-20 of the largest value);
bf16 rel-L2 <= 1e-2 and max error <= 2^-6 of the largest value, as tests/test_hip_clip_attention_edges.py has them, with the
error of the bf16 rounding-point model (step_stages.clip_attention_fwd, rnd = bf, O rounded once) printed beside it."""
import pytest
import torch

import step_stages as SS
from clip_step_ref import MASKS, NAN, make_qkv, make_valid, step_ref
from helpers import vs_cpu32

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ERR_SHAPE, ERR_ALIGN = 1001, 1002
PAD, EXTRA = 8, 3                         # extra columns of the output's leading dimension, extra rows behind B*N

# (T, N): per-slot attention; tiny N; one partial key tile at p = 0; frame boundaries inside tiles; one full and one partial
# query tile; two query tiles and 16 key tiles at p = 7 (every wave of the key split has several); three query tiles
SHAPES = [(32, 1), (16, 2), (4, 8), (8, 12), (4, 40), (8, 64), (4, 72)]
_REF = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _name(bf16):
    return "vlg_attention_clip_step" + ("_bf16" if bf16 else "")


def positions(T):
    return sorted({0, 1, T // 2, T - 1})


def case(B, T, N, d, kind, bf16):
    """(qkv (B,T,N,3d), valid) of a case; the bf16 kernels get, and are judged on, inputs rounded to bf16"""
    key = (B, T, N, d, kind, bf16)
    if key not in _REF:
        _REF[key] = {"in": (make_qkv(B, T, N, d, seed=1000 * T + 10 * N + d + B, bf16=bf16), make_valid(kind, B, T, N, seed=T + N + B))}
    return _REF[key]


def refs(B, T, N, d, kind, bf16, p):
    """(fp64, torch-CPU fp32) references of a case at p, computed once"""
    r = case(B, T, N, d, kind, bf16)
    if p not in r:
        qkv, valid = r["in"]
        r[p] = (step_ref(qkv, valid, p, torch.float64), step_ref(qkv, valid, p, torch.float32))
    return r[p]


def run_step(dev, qkv, valid, p, bf16, poison=True):
    """one launch on device copies -> (B,N,d) fp32 on the CPU; checks that nothing but o[:B*N, :d] was written"""
    from vlg import hip
    B, T, N, d3 = qkv.shape
    d, dt = d3 // 3, BF if bf16 else torch.float32
    q = qkv.clone()
    v = valid.clone() if valid is not None else None
    if poison:
        q[:, p + 1:] = NAN
        if v is not None:
            v[:, p + 1:] = NAN
    qd = SS.to_rows(q).contiguous().to(dev).to(dt)
    vd = v.contiguous().to(dev) if v is not None else None
    o = torch.full((B * N + EXTRA, d + PAD), NAN, device=dev, dtype=dt)
    hip.call(_name(bf16), qd.data_ptr(), hip.ptr(vd), o.data_ptr(), B, T, N, d, p, d + PAD, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(o[:, d:]).all()), "the pad columns of o were written"
    assert bool(torch.isnan(o[B * N:]).all()), "rows past B*N of o were written"
    return o[:B * N, :d].float().cpu().view(B, N, d)


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def bf16_model(qkv, valid, p):
    """the bf16 kernels' rounding points in fp64 on frames 0 .. p: P rounded as the operand of P.V, O once on store"""
    B, _, N, _ = qkv.shape
    v = valid[:, :p + 1].double().contiguous() if valid is not None else None
    out, _ = SS.clip_attention_fwd(SS.to_rows(qkv[:, :p + 1].double().contiguous()), v, B, p + 1, N, rnd=SS.bf)
    return SS.from_rows(SS.bf(out), B, p + 1, N)[:, p]


def under_bar(got, w64, w32, bf16, what, model=None):
    if not bf16:
        print("%s: |err| vs fp64 %.3e, torch-CPU fp32's %.3e, max |fp64| %.3e" % (
            what, float((got.double() - w64).abs().max()), float((w32.double() - w64).abs().max()), float(w64.abs().max())))
        vs_cpu32(got, w64, w32, what)
        return
    assert bool(torch.isfinite(got).all()), what + ": not finite"
    e, worst, top = rel_l2(got, w64), float((got.double() - w64).abs().max()), float(w64.abs().max())
    print("%s: rel-L2 %.3e (bar 1e-2), max |err| %.3e (bar %.3e)%s" % (what, e, worst, 2.0 ** -6 * top, "" if model is None else
          "; model rel-L2 %.3e max %.3e" % (rel_l2(model, w64), float((model - w64).abs().max()))))
    assert e <= 1e-2, (what, "rel L2", e)
    assert worst <= 2.0 ** -6 * top, (what, "max err", worst)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,N", SHAPES)
def test_clip_step_vs_fp64(dev, T, N, B, d, bf16):
    """fp32: the step forms its scores in fp64 on the vector unit (ClipF32::step_scores).  With the forward's score product -
    one chain of 64 fp32 FMAs on v_mfma_f32_32x32x2_f32, off by 2e-5 .. 3.6e-5 at the log2-domain scores of |s| ~ 125 that
    the clips scaled x5 reach - the step was over this bar in 8 of these 448 fp32 (shape, mask, p) cases, by up to 2.96 x
    (1.79e-5 against 6.46e-6 at (1,4,8), d=64, p=2), and vlg_attention_clip_fwd is over it by the same amounts at those frames."""
    for kind in MASKS:
        qkv, valid = case(B, T, N, d, kind, bf16)["in"]
        for p in positions(T):
            got = run_step(dev, qkv, valid, p, bf16)
            w64, w32 = refs(B, T, N, d, kind, bf16, p)
            what = "clip step (%d,%d,%d) d=%d %s p=%d" % (B, T, N, d, kind, p)
            under_bar(got, w64, w32, bf16, what, bf16_model(qkv, valid, p) if bf16 else None)
            if kind == "clip-padded":             # every token of that clip sees only itself: P is exactly 1
                assert torch.equal(got[B - 1], qkv[B - 1, p, :, 2 * d:]), what + ": a fully padded clip's output is not its V rows"


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [64, 192])
def test_one_slot_agrees_with_the_per_slot_step(dev, d, bf16):
    """N = 1, no mask: vlg_attention_step computes the same thing; both under the bar against fp64"""
    from vlg import hip
    B, T, N = 3, 32, 1
    qkv, _ = case(B, T, N, d, "none", bf16)["in"]
    dt = BF if bf16 else torch.float32
    for p in positions(T):
        q = qkv.clone()
        q[:, p + 1:] = NAN
        qd = SS.to_rows(q).contiguous().to(dev).to(dt)
        o = torch.full((B, d), NAN, device=dev, dtype=dt)
        hip.call("vlg_attention_step" + ("_bf16" if bf16 else ""), qd.data_ptr(), o.data_ptr(), B, T, d, p, d, _stream())
        torch.cuda.synchronize()
        w64, w32 = refs(B, T, N, d, "none", bf16, p)
        under_bar(o.float().cpu().view(B, N, d), w64, w32, bf16, "per-slot step p=%d" % p)
        under_bar(run_step(dev, qkv, None, p, bf16), w64, w32, bf16, "clip step, N = 1, p=%d" % p)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["none", "random"])
@pytest.mark.parametrize("T,N", [(8, 12), (8, 64)])
def test_clip_step_agrees_with_the_full_kernel(dev, T, N, kind, bf16):
    """frame p of vlg_attention_clip_fwd on unpoisoned buffers and the step: each under its bar against fp64, and under
    that bar against each other (they sum in different orders, so they need not be bit-equal)"""
    from vlg import hip
    B, d = 3, 192
    qkv, valid = case(B, T, N, d, kind, bf16)["in"]
    dt = BF if bf16 else torch.float32
    qd = SS.to_rows(qkv).contiguous().to(dev).to(dt)
    vd = valid.to(dev) if valid is not None else None
    full = torch.full((B * N * T, d), NAN, device=dev, dtype=dt)
    lse = torch.full((B * (d // 64) * T * N,), NAN, device=dev)
    hip.call("vlg_attention_clip_fwd" + ("_bf16" if bf16 else ""), qd.data_ptr(), hip.ptr(vd), full.data_ptr(), lse.data_ptr(),
             B, T, N, d, _stream())
    torch.cuda.synchronize()
    full = SS.from_rows(full.float().cpu(), B, T, N)
    for p in positions(T):
        w64, w32 = refs(B, T, N, d, kind, bf16, p)
        step = run_step(dev, qkv, valid, p, bf16, poison=False)
        under_bar(step, w64, w32, bf16, "step p=%d" % p)
        under_bar(full[:, p], w64, w32, bf16, "fwd, frame %d" % p)
        if bf16:
            e, worst = rel_l2(step, full[:, p]), float((step - full[:, p]).abs().max())
            assert e <= 1e-2 and worst <= 2.0 ** -6 * float(w64.abs().max()), ("step vs fwd", p, e, worst)
        else:
            err = float((step.double() - full[:, p].double()).abs().max())
            bar = 4 * float((w32.double() - w64).abs().max()) + 2.0 ** -20 * float(w64.abs().max())
            assert err <= bar, "step vs fwd at p=%d: %.3e > %.3e" % (p, err, bar)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T,N", [(8, 12), (8, 64), (4, 72)])
def test_clip_step_is_reproducible(dev, T, N, bf16):
    """two calls give the same bits, and a clip's rows are the same bits alone (B = 1) and inside B = 3"""
    B, d = 3, 192
    for kind in ("none", "random"):
        qkv, valid = case(B, T, N, d, kind, bf16)["in"]
        for p in positions(T):
            a, again = run_step(dev, qkv, valid, p, bf16), run_step(dev, qkv, valid, p, bf16)
            assert bool(torch.isfinite(a).all()) and torch.equal(a, again), (kind, p)
            for b in range(B):
                alone = run_step(dev, qkv[b:b + 1], valid[b:b + 1] if valid is not None else None, p, bf16)
                assert torch.equal(alone[0], a[b]), (kind, p, b)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_refusals_enqueue_nothing(dev, bf16):
    from vlg import hip
    B, T, N, d = 2, 8, 12, 64
    dt = BF if bf16 else torch.float32
    f = getattr(hip.load(), _name(bf16))
    qd = torch.randn(B * N * T, 3 * d, device=dev).to(dt)
    vd = torch.ones(B, T, N, device=dev)
    o = torch.full((B * N + EXTRA, d + PAD), NAN, device=dev, dtype=dt)
    q, v, op, s = qd.data_ptr(), vd.data_ptr(), o.data_ptr(), _stream()
    bad = [((q, v, op, B, T, N, 96, 0, 96), ERR_SHAPE),                 # d % 64
           ((q, v, op, B, T, N, 0, 0, 64), ERR_SHAPE), ((q, v, op, B, T, N, 32, 0, 64), ERR_SHAPE),
           ((q, v, op, B, 5, 8, d, 0, d), ERR_SHAPE),                    # T*N % 32
           ((q, v, op, B, 0, N, d, 0, d), ERR_SHAPE), ((q, v, op, B, T, 0, d, 0, d), ERR_SHAPE),
           ((q, v, op, B, 1 << 15, 64, d, 0, d), ERR_SHAPE),             # T*N > 2^20
           ((q, v, op, 1 << 30, T, 12, d, 0, d), ERR_SHAPE),             # B*T*N >= 2^31
           ((q, v, op, 0, T, N, d, 0, d), ERR_SHAPE), ((q, v, op, -1, T, N, d, 0, d), ERR_SHAPE),
           ((q, v, op, B, T, N, d, -1, d), ERR_SHAPE), ((q, v, op, B, T, N, d, T, d), ERR_SHAPE),
           ((q, v, op, B, T, N, d, 0, d - 1), ERR_SHAPE),
           ((0, v, op, B, T, N, d, 0, d), ERR_ALIGN), ((q, v, 0, B, T, N, d, 0, d), ERR_ALIGN),
           ((q + 4, v, op, B, T, N, d, 0, d), ERR_ALIGN), ((q, v, op + 4, B, T, N, d, 0, d + PAD), ERR_ALIGN)]
    if bf16:
        bad.append(((q, v, op, B, T, N, d, 0, d + 2), ERR_ALIGN))        # 8-byte stores: rows must keep the alignment
    for args, want in bad:
        assert f(*args, s) == want, args
        torch.cuda.synchronize()
        assert bool(torch.isnan(o).all()), args
    for vp in (v, 0):                                                    # the same buffers are accepted; valid alone may be NULL
        o.fill_(NAN)
        assert f(q, vp, op, B, T, N, d, T - 1, d + PAD, s) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o[:B * N, :d]).all()) and bool(torch.isnan(o[:, d:]).all()) and bool(torch.isnan(o[B * N:]).all())

"""GPU: vlg_attention_frame_step / _bf16 - attention of the N queries of ONE frame p among the slots of that frame alone -
through the C ABI, against the fp64 frame attention of frame p (tests/factored_ref.py on that frame), at the bars of the
window kernels (fp32: helpers.vs_cpu32; bf16: rel-L2 1e-2, 2^-6 of the largest value, bf16-representable inputs).

The step needs no cache: every row of qkv at a position != p and the valid entries of those frames hold NaN, EARLIER
positions included.  Only the B*N output rows may be written: o has ldo > d and rows behind B*N, all NaN before the call."""
import pytest
import torch

import factored_ref as R
import step_stages as SS
from clip_step_ref import NAN, make_qkv, make_valid
from test_hip_clip_attention_step import BF, EXTRA, PAD, under_bar

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4, 8, 64), (3, 8, 4, 64), (1, 4, 40, 128), (2, 4, 72, 64)]       # the first four of test_hip_frame_attention.py
_REF = {}


def frame_step_ref(qkv, valid, p, dt):
    """(B,N,d): the frame attention of frame p, from that frame's tokens alone"""
    v = valid[:, p:p + 1].to(dt) if valid is not None else None
    return R.frame_attention(qkv[:, p:p + 1].to(dt), qkv.shape[-1] // 192, v)[:, 0]


def case(B, T, N, d, masked, bf16):
    key = (B, T, N, d, masked, bf16)
    if key not in _REF:
        qkv = make_qkv(B, T, N, d, seed=1000 * T + 10 * N + d + B, bf16=bf16)
        valid = make_valid("random", B, T, N, seed=T + N + B) if masked else None
        _REF[key] = (qkv, valid, {p: (frame_step_ref(qkv, valid, p, torch.float64), frame_step_ref(qkv, valid, p, torch.float32))
                                  for p in sorted({0, 1, T - 1})})
    return _REF[key]


def run_frame_step(dev, qkv, valid, p, bf16):
    from vlg import hip
    B, T, N, d3 = qkv.shape
    d, dt = d3 // 3, BF if bf16 else torch.float32
    q = torch.full_like(qkv, NAN)
    q[:, p] = qkv[:, p]
    v = None
    if valid is not None:
        v = torch.full_like(valid, NAN)
        v[:, p] = valid[:, p]
    qd = SS.to_rows(q).contiguous().to(dev).to(dt)
    vd = v.contiguous().to(dev) if v is not None else None
    o = torch.full((B * N + EXTRA, d + PAD), NAN, device=dev, dtype=dt)
    hip.call("vlg_attention_frame_step" + ("_bf16" if bf16 else ""), qd.data_ptr(), hip.ptr(vd), o.data_ptr(), B, T, N, d, p, d + PAD,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o[:, d:]).all()), "the pad columns of o were written"
    assert bool(torch.isnan(o[B * N:]).all()), "rows past B*N of o were written"
    return o[:B * N, :d].float().cpu().view(B, N, d)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("masked", [False, True], ids=["null", "valid"])
@pytest.mark.parametrize("B,T,N,d", SHAPES)
def test_frame_step_vs_fp64(dev, B, T, N, d, masked, bf16):
    qkv, valid, refs = case(B, T, N, d, masked, bf16)
    for p, (w64, w32) in refs.items():
        got = run_frame_step(dev, qkv, valid, p, bf16)
        under_bar(got, w64, w32, bf16, "frame step %s %s p=%d" % ((B, T, N, d), "valid" if masked else "null", p))
        assert torch.equal(got, run_frame_step(dev, qkv, valid, p, bf16)), "two calls differ"


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_frame_step_exact_properties(dev, bf16):
    """every slot padded: out == v bit for bit; a clip alone equals the clip inside a batch"""
    B, T, N, d = 2, 4, 40, 128
    qkv, valid, _ = case(B, T, N, d, True, bf16)
    for p in (0, T - 1):
        got = run_frame_step(dev, qkv, torch.zeros(B, T, N), p, bf16)
        assert torch.equal(got, qkv[:, p, :, 2 * d:]), "a token that sees only itself must return its V row"
        both = run_frame_step(dev, qkv, valid, p, bf16)
        alone = run_frame_step(dev, qkv[1:], valid[1:], p, bf16)
        assert torch.equal(both[1:], alone), "a clip's bits depend on the batch"


def test_frame_step_refusals(dev):
    from vlg import hip
    lib = hip.load()
    q = torch.zeros(32 * 3 * 64, device=dev)
    o = torch.full((8 * 64,), NAN, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for sfx in ("", "_bf16"):
        f = getattr(lib, "vlg_attention_frame_step" + sfx)
        assert f(q.data_ptr(), 0, o.data_ptr(), 1, 4, 8, 64, 4, 64, s) == 1001          # p outside [0, T)
        assert f(q.data_ptr(), 0, o.data_ptr(), 1, 4, 8, 64, -1, 64, s) == 1001
        assert f(q.data_ptr(), 0, o.data_ptr(), 1, 4, 8, 64, 0, 60, s) == 1001          # ldo < d
        assert f(q.data_ptr(), 0, o.data_ptr(), 1, 3, 5, 64, 0, 64, s) == 1001          # T*N not a multiple of 32
        assert f(0, 0, o.data_ptr(), 1, 4, 8, 64, 0, 64, s) == 1002
        assert f(q.data_ptr() + 2, 0, o.data_ptr(), 1, 4, 8, 64, 0, 64, s) == 1002
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()), "a refused call wrote something"

"""CPU: what generation from a prompt shorter than the window rests on.  (1) Causality: the specification's output at
position P-1 of a window padded with the reserved class id and zero boxes is its output on the P real frames alone, for
both attention settings, in fp64.  (2) The grow/slide schedule the engine follows (vlg.engine.grow_schedule).  (3) The
projection GEMMs plan the cached step's calls: B*N rows, the q k v product written into the cache with ldc = T*3d."""
import ctypes

import pytest
import torch

from oracle import layout_spec as O
from test_hip_gemm_paths import CALLS, EPI_A_BF16, EPI_B_BF16, EPI_BF16, EPI_BIAS, EPI_GELU, EPI_OUT_BF16, EPI_RESID, EPI_SPLIT3, _Plan
from vlg.engine import grow_schedule
from vlg.spec import LayoutConfig, param_shapes

NC = 20


def _model(T, N, d, n_layers, seed):
    cfg = LayoutConfig(B=2, T=T, N=N, d=d, n_layers=n_layers)
    p = {k: v.double() for k, v in O.init_params(param_shapes(cfg), seed=seed).items()}
    g = torch.Generator().manual_seed(seed + 1)
    cls = torch.randint(0, NC, (cfg.B, T, N), generator=g)
    box = torch.rand(cfg.B, T, N, 4, generator=g, dtype=torch.float64)
    return cfg, p, cls, box


@pytest.mark.parametrize("attention", ["slot", "clip"])
@pytest.mark.parametrize("P", [1, 3, 7])
def test_padded_window_agrees_with_the_real_frames_alone(attention, P):
    """fp64, bar 1e-12 of the output scale: the two evaluations differ in nothing but the order of a few sums (the softmax
    rows of positions < P see the same keys; -inf scores add exact zeros)."""
    cfg, p, cls, box = _model(8, 5, 64, 2, seed=11 + P)
    cls[0, 0, 2] = cls[1, :, 4] = NC                                    # reserved ids inside the prompt too
    hist_c, hist_b = cls[:, :P], box[:, :P]
    pad_c, pad_b = cls.clone(), box.clone()
    pad_c[:, P:] = NC
    pad_b[:, P:] = 0.0
    with torch.no_grad():
        wl, wr = O.forward(p, hist_c, hist_b, cfg.n_layers, attention=attention, valid=(hist_c < NC).double())
        gl, gr = O.forward(p, pad_c, pad_b, cfg.n_layers, attention=attention, valid=(pad_c < NC).double())
    assert bool(torch.isfinite(gl).all()) and bool(torch.isfinite(gr).all())        # the frames after the history stay finite
    scale = float(wl.abs().max())
    for t in range(P):                                                  # every real position, the last one is the one generation reads
        assert float((gl[:, t] - wl[:, t]).abs().max()) <= 1e-12 * scale, (attention, P, t)
        assert float((gr[:, t] - wr[:, t]).abs().max()) <= 1e-12 * scale, (attention, P, t)


@pytest.mark.parametrize("attention", ["slot", "clip"])
def test_later_frames_cannot_reach_an_earlier_position(attention):
    """whatever the frames after position t hold - here other classes and boxes, not padding - the output at t is the same"""
    cfg, p, cls, box = _model(8, 4, 64, 2, seed=5)
    other_c, other_b = cls.clone(), box.clone()
    other_c[:, 3:] = (cls[:, 3:] + 7) % NC
    other_b[:, 3:] = 1.0 - box[:, 3:]
    with torch.no_grad():
        a = O.forward(p, cls, box, cfg.n_layers, attention=attention, valid=torch.ones(cls.shape, dtype=torch.float64))
        b = O.forward(p, other_c, other_b, cfg.n_layers, attention=attention, valid=torch.ones(cls.shape, dtype=torch.float64))
    for x, y in zip(a, b):
        assert float((x[:, :3] - y[:, :3]).abs().max()) <= 1e-12 * float(x.abs().max())
        assert float((x[:, 3:] - y[:, 3:]).abs().max()) > 1e-3


def test_schedule_reads_the_newest_frame_and_slides_when_the_window_is_full():
    T = 8
    # P = 3, cached: the prompt pass encodes the window; positions 3 .. 7 are cached steps; the step at position T-1 is the
    # first that slides; every later step is the full-window one
    got = grow_schedule(3, T, 8, True)
    assert got == [("window", 2, 3), ("step", 3, 4), ("step", 4, 5), ("step", 5, 6), ("step", 6, 7), ("step", 7, None),
                   ("window", 7, None), ("window", 7, None)]
    assert grow_schedule(3, T, 8, False) == [("window", t, pos) for _, t, pos in got]
    # a full prompt: today's steps and nothing else, whatever `cached` says
    for cached in (False, True):
        assert grow_schedule(T, T, 4, cached) == [("window", T - 1, None)] * 4
    # P = T-1: one append by the prompt pass, then the hand-over
    assert grow_schedule(T - 1, T, 3, True) == [("window", T - 2, T - 1), ("step", T - 1, None), ("window", T - 1, None)]
    # a rollout that ends before the window fills never slides
    assert grow_schedule(1, T, 3, True) == [("window", 0, 1), ("step", 1, 2), ("step", 2, 3)]
    for P in range(1, T + 1):
        for steps in (1, 2, T + 3):
            for cached in (False, True):
                sched = grow_schedule(P, T, steps, cached)
                assert len(sched) == steps and sched[0][0] == "window"
                for i, (enc, t_read, pos) in enumerate(sched):
                    h = min(P + i, T)
                    assert t_read == h - 1 and pos == (h if h < T else None)
                    assert (enc == "step") == (cached and i > 0 and P + i <= T)
    for bad in ((0, T, 1), (T + 1, T, 1), (2, T, 0)):
        with pytest.raises(ValueError):
            grow_schedule(*bad, True)


@pytest.mark.parametrize("family,flags,act_bits", [("fp32", 0, 0), ("fp32x3", EPI_SPLIT3, 0),
                                                   ("bf16", EPI_BF16, EPI_A_BF16 | EPI_B_BF16 | EPI_OUT_BF16)])
@pytest.mark.parametrize("rows", [1, 24, 2048])
def test_gemm_plan_accepts_the_cached_steps_calls(family, flags, act_bits, rows):
    """every projection of a cached step, M = B*N rows: q k v into the cache (ldc = T*3d), proj and ff2 with the residual,
    ff1 with GELU; d = 256, T = 16 (the flagship shape) and d = 64, T = 8 (the tests')"""
    from vlg import hip
    lib = hip.load()
    want_family = {"fp32": 0, "bf16": 1, "fp32x3": 2}[family]
    for d, T in ((256, 16), (64, 8)):
        ff = 4 * d
        calls = [(3 * d, d, EPI_BIAS, T * 3 * d), (d, d, EPI_BIAS | EPI_RESID, d), (ff, d, EPI_BIAS | EPI_GELU, ff),
                 (d, ff, EPI_BIAS | EPI_RESID, d)]
        for n, k, epi, ldc in calls:
            out_bits = act_bits if not (epi & EPI_RESID) else act_bits & ~EPI_OUT_BF16       # the residual stream stays fp32
            plan = _Plan()
            rc = lib.vlg_linear_plan(CALLS["fwd"], rows, n, k, epi | flags | out_bits, k, k, ldc, 0, ctypes.byref(plan))
            assert rc == 0, (family, rows, n, k, ldc, rc)
            assert plan.family == want_family and plan.launches == 1 and plan.problems == 1
            prob = plan.p[0]
            assert prob.blocks >= 1 and prob.blocks == -(-rows // prob.bm) * (-(-n // prob.bn) // prob.run)
        # a leading dimension shorter than the row is still refused
        assert lib.vlg_linear_plan(CALLS["fwd"], rows, 3 * d, d, EPI_BIAS | flags | act_bits, d, d, 3 * d - 4, 0,
                                   ctypes.byref(_Plan())) == 1001

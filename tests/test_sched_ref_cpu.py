"""CPU: the restatement of scheduled sampling (tests/sched_ref.py) on its own - which tokens may be replaced, the integer
threshold and its ramp, the coins - the host-only plan entry point, the trainer's knobs, and the share of the GPU test's
sampled draws that lie close enough to a cumulative boundary for an fp32 evaluation to decide them differently."""
import argparse
import ctypes
import math

import numpy as np
import pytest
import torch

import decode_ref as D
import sched_ref as S

NC = S.NC


def test_frame_zero_and_padded_tokens_are_never_replaced():
    _, cls, _ = S.kernel_case(3, 8, 5, seed=1)
    assert bool((cls == NC).any()) and bool((cls[:, 1:] < NC).any())
    e = S.eligible(cls, NC)
    assert not bool(e[:, 0].any()) and not bool(e[cls >= NC].any()) and bool(e[:, 1:][cls[:, 1:] < NC].all())
    for k in (0, 7):
        rep = S.replaced(cls, NC, k, S.TWO24, 0, seed=5)                # eps_max = 1: every eligible token, and no other
        assert torch.equal(rep, e)
        assert not bool(S.replaced(cls, NC, k, 0, 0, seed=5).any())    # eps_max = 0: none
    out, cls, box = S.kernel_case(3, 8, 5, seed=1)
    mc, mb, rep, near = S.mix_inputs(out, cls, box, NC, 0, S.TWO24)
    assert torch.equal(mc[~rep], cls[~rep]) and torch.equal(mb[~rep], box.double()[~rep]) and not bool(near.any())
    assert bool((mc[rep] < NC).all()) and bool(torch.isfinite(mb).all())
    # the source row of token (b, t, n) is row (b*N + n)*T + t - 1
    b, t, n = 2, 5, 3
    row = out[(b * 5 + n) * 8 + t - 1]
    assert int(mc[b, t, n]) == int(row[:NC].argmax()) or not bool(rep[b, t, n])
    assert bool(rep[b, t, n]) == bool(cls[b, t, n] < NC)


def test_threshold_and_ramp_are_integers():
    assert S.thr_max(0.0) == 0 and S.thr_max(1.0) == 1 << 24 and S.thr_max(0.25) == 1 << 22 and S.thr_max(0.5) == 1 << 23
    assert S.thr_max(1e-9) == 0 and S.thr_max(0.1) == 1677722          # 1677721.6 rounds up
    for bad in (-0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            S.thr_max(bad)
    tm = 1677722
    assert S.thr(0, tm, 0) == S.thr(10 ** 9, tm, 0) == tm              # no ramp
    R = 1000
    assert S.thr(0, tm, R) == 1677                                     # 1677722 * 1 // 1000
    assert S.thr(R - 2, tm, R) == 1676044                              # 1677722 * 999 // 1000 = 1676044.278
    assert S.thr(R - 1, tm, R) == tm and S.thr(R, tm, R) == tm and S.thr(2 ** 31 - 1, tm, R) == tm
    assert S.thr(0, 1 << 24, 1) == 1 << 24
    big = 2 ** 31 - 1                                                   # the product needs 64 bits
    assert S.thr(big - 2, 1 << 24, big) == ((1 << 24) * (big - 1)) // big == (1 << 24) - 1


def test_plan_entry_point_states_the_same_threshold():
    """vlg_sched_plan is host only: the one place the product keeps the rounding rule"""
    from vlg import hip
    lib = hip.load()
    t = ctypes.c_uint32()
    for eps in (0.0, 1e-9, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.999999, 1.0):
        assert lib.vlg_sched_plan(eps, ctypes.byref(t)) == 0 and t.value == S.thr_max(eps), eps
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        assert lib.vlg_sched_plan(bad, ctypes.byref(t)) == 1001
    assert lib.vlg_sched_plan(0.5, None) == 1001


def test_coin_words_are_their_own_stream():
    tok = np.arange(4096)
    coin, draw = S.coin_words(tok, 3, seed=9), S.draw_words(tok, 3, seed=9)
    assert int((coin == draw).sum()) <= 1 and coin.max() < 1 << 24 and coin.min() >= 0
    # the draw stream is the one generation reads
    assert np.array_equal(draw.astype(np.float64) * 2.0 ** -24 + 2.0 ** -25, D.uniform(tok, 3, 9))
    a = coin < (1 << 22)
    assert not np.array_equal(a, S.coin_words(tok, 4, seed=9) < (1 << 22))           # another step
    assert not np.array_equal(a, S.coin_words(tok, 3, seed=10) < (1 << 22))          # another seed
    assert not np.array_equal(a, S.coin_words(tok, 3, seed=9 + (1 << 32)) < (1 << 22))   # the seed's high word counts
    assert np.array_equal(a, S.coin_words(tok, 3, seed=9) < (1 << 22))


def test_decode_tokens_is_the_generation_rule():
    l = (torch.randn(200, NC, generator=torch.Generator().manual_seed(3)) * 3).double().numpy()
    for temperature, top_k in ((0.0, 0), (1.0, 0), (0.7, 5)):
        a, na = S.decode_tokens(l, np.arange(200), 2, temperature, top_k, seed=11)
        b, nb = D.decode_step(l, 2, temperature, top_k, seed=11)
        assert np.array_equal(a, b) and np.array_equal(na, nb)
    shifted, _ = S.decode_tokens(l, np.arange(200) + 1000, 2, 1.0, 0, seed=11)
    assert not np.array_equal(shifted, S.decode_tokens(l, np.arange(200), 2, 1.0, 0, seed=11)[0])


def test_coin_share_at_a_quarter():
    """16 384 eligible tokens at eps_max = 0.25: the replaced share within 4.5 binomial standard deviations of 0.25"""
    cls = torch.zeros(1, 17, 1024, dtype=torch.int64)                   # 16 frames after the first, nothing padded
    e = S.eligible(cls, NC)
    n = int(e.sum())
    assert n == 16384
    bar = 4.5 * math.sqrt(0.25 * 0.75 / n)
    assert abs(bar - 0.0152) < 5e-5
    rep = S.replaced(cls, NC, 0, S.thr_max(0.25), 0, S.COIN_SEED)
    share = int(rep.sum()) / n
    print("\nreplaced share %.5f (0.25 +- %.4f)" % (share, bar))
    assert abs(share - 0.25) <= bar and not bool(rep[~e].any())


def _args(**kw):
    return argparse.Namespace(seed=1024, rank=0, **kw)


SCHED_ENV = ("VLG_SCHED_SAMPLING", "VLG_SCHED_RAMP_STEPS", "VLG_SCHED_TEMPERATURE", "VLG_SCHED_TOP_K", "VLG_SCHED_SEED")


def test_sched_knobs(monkeypatch):
    from trainer import sched_knobs
    for k in SCHED_ENV:
        monkeypatch.delenv(k, raising=False)
    assert sched_knobs(_args()) == {}
    monkeypatch.setenv("VLG_SCHED_RAMP_STEPS", "100")                  # the other knobs alone do not turn it on
    assert sched_knobs(_args()) == {}
    monkeypatch.setenv("VLG_SCHED_SAMPLING", "0.25")
    assert sched_knobs(_args()) == dict(sched_sampling=0.25, sched_ramp_steps=100, sched_temperature=0.0, sched_top_k=0,
                                        sched_seed=1024)
    a = _args()
    a.rank = 3
    assert sched_knobs(a)["sched_seed"] == 1027                         # ranks flip different coins
    monkeypatch.setenv("VLG_SCHED_SEED", "7")
    monkeypatch.setenv("VLG_SCHED_TEMPERATURE", "0.7")
    monkeypatch.setenv("VLG_SCHED_TOP_K", "5")
    got = sched_knobs(a)
    assert got["sched_seed"] == 10 and got["sched_temperature"] == 0.7 and got["sched_top_k"] == 5
    assert sched_knobs(_args(sched_sampling=0.0))["sched_sampling"] == 0.0      # 0 is ON (and replaces nothing); args win
    for env, bad in (("VLG_SCHED_SAMPLING", "1.5"), ("VLG_SCHED_SAMPLING", "-0.1"), ("VLG_SCHED_SAMPLING", "nan"),
                     ("VLG_SCHED_RAMP_STEPS", "-1"), ("VLG_SCHED_TEMPERATURE", "-1"), ("VLG_SCHED_TEMPERATURE", "inf"),
                     ("VLG_SCHED_TEMPERATURE", "nan"), ("VLG_SCHED_TOP_K", "21"), ("VLG_SCHED_TOP_K", "-1"), ("VLG_SCHED_SEED", "-1")):
        with monkeypatch.context() as m:
            m.setenv(env, bad)
            with pytest.raises(ValueError, match=env):
                sched_knobs(_args())


def test_sched_and_decode_rules_are_stated_once_and_name_their_caller():
    """vlg.spec.sched_options / decode_options: what LayoutEngine and rollout (keywords) and trainer.sched_knobs (environment
    variables) all call"""
    from vlg.spec import decode_options, sched_options
    assert sched_options(0.25) == (0.25, 0, 0.0, 0) and sched_options("1", 2 ** 31 - 1, 0.7, NC, NC) == (1.0, 2 ** 31 - 1, 0.7, NC)
    assert decode_options(0, 0) == (0.0, 0) and decode_options(1.5, NC, NC) == (1.5, NC)
    env = tuple(SCHED_ENV[:4])
    for kw, name in ((dict(eps_max=1.5), "sched_sampling"), (dict(eps_max=-0.1), "sched_sampling"),
                     (dict(eps_max=float("nan")), "sched_sampling"), (dict(eps_max=0.5, ramp_steps=-1), "sched_ramp_steps"),
                     (dict(eps_max=0.5, ramp_steps=2 ** 31), "sched_ramp_steps"), (dict(eps_max=0.5, temperature=-1.0), "sched_temperature"),
                     (dict(eps_max=0.5, temperature=float("inf")), "sched_temperature"),
                     (dict(eps_max=0.5, temperature=float("nan")), "sched_temperature"), (dict(eps_max=0.5, top_k=NC + 1), "sched_top_k"),
                     (dict(eps_max=0.5, top_k=-1), "sched_top_k")):
        with pytest.raises(ValueError, match=name):
            sched_options(n_classes=NC, **kw)
        with pytest.raises(ValueError, match="VLG_" + name.upper()):
            sched_options(n_classes=NC, names=env, **kw)
    for temperature, top_k in ((-1e-9, 0), (float("inf"), 0), (float("nan"), 0), (0.0, -1), (0.0, NC + 1)):
        with pytest.raises(ValueError, match=r"^temperature must be finite and >= 0, top_k in \[0, %d\]" % NC):
            decode_options(temperature, top_k, NC)


def test_near_draws_of_the_kernel_cases_stay_under_one_percent():
    """the exact seeds and shapes tests/test_hip_sched_mix.py samples with: draws whose u * S lies within 1e-5 * S of a
    cumulative boundary are excused there, and must stay under 1 % of the draws (the project's cap)"""
    for temperature, top_k in S.SAMPLING:
        draws = flagged = 0
        for (B, T, N) in S.SAMPLING_SHAPES:
            out, cls, box = S.kernel_case(B, T, N, seed=B * 100 + N)
            for k in S.SAMPLING_STEPS:
                _, _, rep, near = S.mix_inputs(out, cls, box, NC, k, S.TWO24, 0, temperature, top_k, S.CASE_SEED)
                assert not bool(near[~rep].any())
                draws += int(rep.sum())
                flagged += int(near.sum())
        print("\ntemperature %g top_k %d: %d of %d draws within 1e-5 S of a boundary" % (temperature, top_k, flagged, draws))
        assert draws > 500 and flagged < 0.01 * draws

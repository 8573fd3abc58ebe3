"""CPU: the restatement of the sampled futures (tests/samples_ref.py) against what it must mean - the sample counter against
decode_ref's draws, the batched decoding step's independence of the pass split, and the scores, diversity, selection and
record on planted cases.  The GPU tests (tests/test_hip_samples.py) hold the kernels to this restatement."""
import numpy as np
import torch

import decode_ref as D
import samples_ref as R

C, EPS, T0 = 20, 1e-7, 2


def test_sample_zero_draws_what_rollout_draws_and_samples_differ():
    tokens = np.arange(512)
    for step, seed in ((0, 0), (3, 0xC0FFEE12345), (7, 2 ** 63 + 5)):
        assert np.array_equal(R.uniform(tokens, step, seed, 0), D.uniform(tokens, step, seed))
        u = [R.uniform(tokens, step, seed, k) for k in range(5)]
        for j in range(5):
            for k in range(j + 1, 5):
                assert float(np.mean(u[j] == u[k])) < 0.01, (j, k)
        # the box stream's words with the sample word 0 are boxhead_ref's
        import philox_ref as P
        assert all(np.array_equal(a, b) for a, b in zip(R.words(tokens, step, P.BOX_NORMAL, seed, 0), P.words(tokens, step, P.BOX_NORMAL, seed)))


def test_a_later_sample_draws_the_distribution():
    row = D.distribution_row().double().numpy()
    logits = np.tile(row, (D.DIST_TOKENS, 1))
    for temperature, top_k in D.DIST_CASES:
        drawn = [R.decode_step(logits, step, temperature, top_k, D.DIST_SEED, clips_n=D.DIST_TOKENS, sample0=3)[0]
                 for step in range(D.DIST_STEPS)]
        D.check_distribution(np.stack(drawn), temperature, top_k)


def test_decoding_is_independent_of_the_pass_split():
    clips, N, K = 2, 8, 5
    g = torch.Generator().manual_seed(1)
    rows = (torch.randn(K * clips * N, C, generator=g) * 3).double().numpy()
    whole, _ = R.decode_step(rows, 2, 0.7, 5, 99, clips_n=clips * N, sample0=0)
    per = clips * N
    parts = [R.decode_step(rows[k0 * per:(k0 + k) * per], 2, 0.7, 5, 99, clips_n=per, sample0=k0)[0] for k0, k in ((0, 2), (2, 2), (4, 1))]
    assert np.array_equal(np.concatenate(parts), whole)
    # and a prompt's draw does not depend on where it sits in the batch: the same rows for both prompts give the same classes
    same = np.tile(rows[:N], (K * clips, 1))
    got, _ = R.decode_step(same, 2, 0.7, 5, 99, clips_n=per, sample0=0)
    got = got.reshape(K, clips, N)
    assert not np.array_equal(got[:, 0], got[:, 1])          # (different prompt tokens: different counters)
    alone, _ = R.decode_step(np.tile(rows[:N], (K, 1)), 2, 0.7, 5, 99, clips_n=N, sample0=0)
    assert np.array_equal(alone.reshape(K, N), got[:, 0])


def _scored(K=5, B=3, S=3, N=5, seed=4):
    gc, gb, cc, cb = R.score_case(K, B, S, N, seed)
    return gc, gb, cc, cb, R.scores(gc, gb, cc, cb, T0, C, EPS), R.diversity(gc, gb, cc, T0, C, EPS)


def test_a_planted_truth_sample_is_perfect_and_selected():
    gc, gb, cc, cb, sc, div = _scored()
    K = gc.shape[0]
    assert sc[K - 1, 0, R.IOU] >= 1 - 1e-4 and sc[K - 1, 0, R.ADE] == 0 and sc[K - 1, 0, R.FDE] == 0 and sc[K - 1, 0, R.ACC] == 1
    for crit in R.SCORE_COLS:
        assert R.select(sc, crit)[0] == K - 1, crit
    rec = R.summary(R.record(sc, div, R.IOU))
    # (clip 1 holds a NaN box: the means of iou and ade over its samples are NaN, their optima and the accuracy are not)
    assert rec["clips"] == 2 and rec["best_acc"] >= rec["mean_acc"] and rec["best_iou"] > 0.5 and rec["best_ade"] < 0.2
    assert rec["selected_iou"] == rec["best_iou"]            # selecting by iou reaches iou's own optimum


def test_ties_nan_and_unscored_clips():
    gc, gb, cc, cb, sc, div = _scored()
    K, B = sc.shape[:2]
    # samples 0 and 1 are copies in clip 2 - and clip 2 has no scored token: scores 0, counts 0, selects 0, not counted
    assert np.array_equal(sc[:, 2], np.zeros((K, R.COLS))) and all(R.select(sc, c)[2] == 0 for c in R.SCORE_COLS)
    assert np.array_equal(div[2], [0.0, 0.0])
    # the NaN box sits in sample K-2 of clip 1: its IoU and ADE are NaN and it is never chosen
    assert np.isnan(sc[K - 2, 1, R.IOU]) and np.isnan(sc[K - 2, 1, R.ADE]) and not np.isnan(sc[K - 2, 1, R.ACC])
    assert R.select(sc, R.IOU)[1] != K - 2 and R.select(sc, R.ADE)[1] != K - 2
    # of two identical samples the lower index wins; all NaN selects 0
    assert R.choose([0.5, 0.5, 0.25], R.IOU) == 0 and R.choose([0.5, 0.5, 0.75], R.ADE) == 0
    assert R.choose([float("nan"), 0.1, 0.1], R.ACC) == 1 and R.choose([float("nan")] * 3, R.FDE) == 0
    # in clip 0 samples 0 and 1 are copies: equal scores
    assert np.array_equal(sc[0, 0], sc[1, 0])
    rec = R.record(sc, div, R.ADE)
    assert rec[R.REC_CLIPS] == 2 and np.isnan(rec[R.REC_MEAN + R.ADE]) and not np.isnan(rec[R.REC_BEST + R.ADE])
    # a clip whose last frame has no scored token keeps its FDE terms out
    cc2 = cc.clone()
    cc2[1, T0 + gc.shape[2] - 1] = C
    sc2 = R.scores(gc, gb, cc2, cb, T0, C, EPS)
    rec2 = R.record(sc2, R.diversity(gc, gb, cc2, T0, C, EPS), R.ADE)
    assert rec2[R.REC_CLIPS] == 2 and rec2[R.REC_CLIPS_FDE] == 1 and np.array_equal(sc2[:, 1, R.FDE], np.zeros(K))


def test_identical_samples_have_no_diversity():
    gc, gb, cc, cb = R.score_case(1, 2, 3, 5, 7)
    K = 4
    div = R.diversity(gc.repeat(K, 1, 1, 1), gb.repeat(K, 1, 1, 1, 1), cc, T0, C, EPS)
    assert np.array_equal(div[:, 1], [0.0, 0.0]) and float(np.abs(div[:, 0]).max()) <= EPS / 0.01   # 1 - a / (a + eps), a >= 0.01
    assert np.array_equal(R.diversity(gc, gb, cc, T0, C, EPS), np.zeros((2, 2)))                     # K = 1
    gc5, gb5, cc5, _ = R.score_case(5, 3, 3, 5, 8)
    d5 = R.diversity(gc5, torch.nan_to_num(gb5, nan=0.5), cc5, T0, C, EPS)
    assert bool((d5[:2] > 0).all()) and bool((d5[:2] <= 1).all())
    assert np.isnan(R.diversity(gc5, gb5, cc5, T0, C, EPS)[1, 0])         # a NaN box shows in its clip's box diversity


def test_best_of_k_is_monotone_in_k():
    gc, gb, cc, cb = R.score_case(5, 3, 3, 64, 9)
    gb = torch.nan_to_num(gb, nan=0.5)
    prev = None
    for k in range(1, 6):
        sc = R.scores(gc[:k], gb[:k], cc, cb, T0, C, EPS)
        s = R.summary(R.record(sc, R.diversity(gc[:k], gb[:k], cc, T0, C, EPS), R.IOU))
        if prev is not None:
            assert s["best_iou"] >= prev["best_iou"] and s["best_acc"] >= prev["best_acc"]
            assert s["best_ade"] <= prev["best_ade"] and s["best_fde"] <= prev["best_fde"]
        prev = s
    assert prev["clips"] == 2 and prev["best_iou"] >= 0.5 * (1 - 1e-4)    # clip 0 holds the planted truth

"""GPU: K sampled futures per clip - the _samples decoding entries, the three kernels of csrc/samples.hip, and
LayoutEngine.rollout_samples / evaluate_samples with the Trainer's surface - against tests/samples_ref.py.  Every output
buffer starts as NaN / -1 sentinels.

Bars.  Classes equal the restatement except the draws it flags `near` (u * S within 1e-5 S of a cumulative boundary: an fp32
evaluation may decide them either way); at most max(1, 1 %) of a check's draws may be flagged (expected share 2 C 1e-5 = 4e-4;
the flags are the restatement's own, so the seeds below are known to stay inside on the CPU).  Boxes: atol 1e-6 without a
draw, boxhead_ref.box_bar with one - the bars of tests/test_hip_layout_decode.py and tests/test_hip_decode_box.py.  Scores and
diversity: atol 1e-5 against fp64 (a per-token value is ~10 fp32 operations on numbers in [0, 1.5]: error below 1e-6, and the
double-precision mean keeps it; one wrong token moves a mean by at least 1 / (S N) of a typical 0.1).  The record: rtol 1e-9
against the restatement on the device's own scores.  Engine logits: atol 1e-4 x max |logits| (fp32), relative Frobenius 5e-2
(bf16), the bars of tests/test_hip_rollout_short_prompt.py."""
import numpy as np
import pytest
import torch

import boxhead_ref as BH
import samples_ref as R
from helpers import check_close
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

NC = 20
ERR_SHAPE = 1001
NAN = float("nan")
STEPS, POS = 3, 2                     # the appending entry writes frame POS from frame POS - 1
KINDS = ("slide", "append")
IOU_EPS = 1e-7


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _near_bar(draws):
    return max(1, draws // 100)


# ------------------------------------------------------------------------------------------------------- the decode kernels
def _decode_inputs(B, T, N, seed):
    """rows (B*N, 32) = logits | raw mean | raw scale | NaN; a window with padded slots in the newest frame of both entries"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(B * N, 32, generator=g) * 3
    rows[:, NC + 4:NC + 8] = torch.randn(B * N, 4, generator=g) * 4
    rows[:, NC + 8:] = NAN
    cls = torch.randint(0, NC, (B, T, N), generator=g)
    box = torch.rand(B, T, N, 4, generator=g)
    pad = torch.rand(B, N, generator=g) < 0.2
    cls[:, T - 1][pad] = NC
    cls[:, POS - 1][pad] = NC
    return rows, cls, box


class Call:
    """buffers of one decoding call of either kind on (B,T,N), outputs pre-filled with sentinels"""

    def __init__(self, dev, kind, rows, cls, box):
        B, T, N = cls.shape
        self.kind, self.shape = kind, (B, T, N)
        self.rows, self.cls_in, self.box_in = rows.to(dev).contiguous(), cls.to(dev).contiguous(), box.to(dev).contiguous()
        self.gen_cls = torch.full((B, STEPS, N), -1, dtype=torch.int64, device=dev)
        self.gen_box = torch.full((B, STEPS, N, 4), NAN, device=dev)
        self.valid = torch.full((B, T, N), NAN, device=dev)
        if kind == "slide":
            self.cls_out = torch.full((B, T, N), -1, dtype=torch.int64, device=dev)
            self.box_out = torch.full((B, T, N, 4), NAN, device=dev)
        else:
            self.frame_cls = torch.full((B, N), -1, dtype=torch.int64, device=dev)
            self.frame_box = torch.full((B, N, 4), NAN, device=dev)

    def run(self, step, entry, clips=None, sample0=0, temperature=0.0, top_k=0, tau=0.0, seed=0, keep_padded=0, expect=0):
        """entry: "_ext" or "_samples" """
        from vlg import hip
        B, T, N = self.shape
        p = lambda x: x.data_ptr()
        tail = (temperature, top_k, tau, seed, keep_padded) + ((clips, sample0) if entry == "_samples" else ()) + (_stream(),)
        if self.kind == "slide":
            name = "vlg_layout_decode" + entry
            args = (p(self.rows), 32, p(self.cls_in), p(self.box_in), p(self.cls_out), p(self.box_out), p(self.valid),
                    p(self.gen_cls), p(self.gen_box), B, T, N, NC, STEPS, step) + tail
        else:
            name = "vlg_layout_decode_append" + entry
            args = (p(self.rows), 32, p(self.cls_in), p(self.box_in), p(self.valid), p(self.gen_cls), p(self.gen_box),
                    p(self.frame_cls), p(self.frame_box), B, T, N, NC, POS, STEPS, step) + tail
        code = getattr(hip.load(), name)(*args)
        torch.cuda.synchronize()
        assert code == expect, "%s returned %d, expected %d" % (name, code, expect)
        return self

    def outputs(self, clips=None):
        """every output, on the CPU; clips = (first, count) cuts the batch axis"""
        names = ("cls_out", "box_out", "valid", "gen_cls", "gen_box") if self.kind == "slide" else \
            ("cls_in", "box_in", "valid", "gen_cls", "gen_box", "frame_cls", "frame_box")
        out = [getattr(self, k).cpu() for k in names]
        return out if clips is None else [o[clips[0]:clips[0] + clips[1]] for o in out]

    def newest(self):
        return self.shape[1] - 1 if self.kind == "slide" else POS - 1


DECODE_CASES = [(1, 1, 1, 4), (3, 2, 8, 4), (5, 3, 70, 4)]           # (K, clips, N, T); the last: 1050 tokens, 17 blocks
DECODE_KNOBS = [dict(temperature=0.7, top_k=5, seed=0xC0FFEE12345, keep_padded=1), dict(temperature=1.0, top_k=0, seed=31, keep_padded=0)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,clips,N,T", DECODE_CASES)
def test_decode_samples_match_the_restatement(dev, kind, K, clips, N, T):
    B, sample0, step = K * clips, 2, 1
    rows, cls, box = _decode_inputs(B, T, N, seed=K * 100 + N)
    for kw in DECODE_KNOBS:
        for tau in (0.0, 1.0):
            got = Call(dev, kind, rows, cls, box).run(step, "_samples", clips=clips, sample0=sample0, tau=tau, **kw)
            t_new = got.newest()
            want_c, want_b, near = R.next_frame(rows[:, :NC + 8], cls[:, :t_new + 1], box[:, :t_new + 1], NC, step, kw["temperature"],
                                                kw["top_k"], kw["seed"], bool(kw["keep_padded"]), tau, clips=clips, sample0=sample0)
            gc, gb = got.gen_cls[:, step].cpu(), got.gen_box[:, step].cpu()
            print("\n%s K=%d clips=%d N=%d tau=%g: %d of %d draws near a boundary, largest |box - reference| %.3g"
                  % (kind, K, clips, N, tau, int(near.sum()), B * N, float((gb.double() - want_b).abs().max())))
            assert int(near.sum()) <= _near_bar(B * N)
            assert torch.equal(gc[~near], want_c[~near])
            check_close(gb, want_b, rtol=0, atol=1e-6 if tau == 0.0 else BH.box_bar(tau), what="boxes")
            if kw["keep_padded"]:
                pad = cls[:, t_new] >= NC
                assert bool(pad.any()) or B * N < 8
                assert torch.equal(gb[pad], box[:, t_new][pad]) and bool((gc[pad] == NC).all())
            # the drawn frame is what every output holds; the other steps' slots are untouched
            if kind == "slide":
                assert torch.equal(got.cls_out[:, -1].cpu(), gc) and torch.equal(got.box_out[:, -1].cpu(), gb)
                assert torch.equal(got.cls_out[:, :-1].cpu(), cls[:, 1:]) and torch.equal(got.box_out[:, :-1].cpu(), box[:, 1:])
                assert torch.equal(got.valid.cpu(), (got.cls_out.cpu() < NC).float())
            else:
                assert torch.equal(got.cls_in[:, POS].cpu(), gc) and torch.equal(got.frame_cls.cpu(), gc)
                assert torch.equal(got.box_in[:, POS].cpu(), gb) and torch.equal(got.frame_box.cpu(), gb)
            assert bool((got.gen_cls[:, [0, 2]] == -1).all())
            # a launch of sample k alone is slice k of the batched launch, bit for bit
            for k in range(K):
                sl = slice(k * clips, (k + 1) * clips)
                one = Call(dev, kind, rows[k * clips * N:(k + 1) * clips * N], cls[sl], box[sl]).run(
                    step, "_samples", clips=clips, sample0=sample0 + k, tau=tau, **kw)
                assert _same(one.outputs(), got.outputs((k * clips, clips))), (k, tau)
    # the same rows for every sample: the samples still differ, sample by sample, and sample 0 is the _ext call's draw
    if K > 1:
        kw = DECODE_KNOBS[0]
        same_rows, same_cls, same_box = rows[:clips * N].repeat(K, 1), cls[:clips].repeat(K, 1, 1), box[:clips].repeat(K, 1, 1, 1)
        got = Call(dev, kind, same_rows, same_cls, same_box).run(step, "_samples", clips=clips, sample0=0, tau=1.0, **kw)
        ext = Call(dev, kind, rows[:clips * N], cls[:clips], box[:clips]).run(step, "_ext", tau=1.0, **kw)
        assert _same(ext.outputs(), got.outputs((0, clips)))
        if clips * N >= 16:
            b = got.gen_box[:, step].cpu().view(K, clips, N, 4)
            assert all(not torch.equal(b[j], b[k]) for j in range(K) for k in range(j + 1, K))


@pytest.mark.parametrize("kind", KINDS)
def test_one_sample_per_clip_is_the_ext_entry(dev, kind):
    B, T, N = 3, 4, 23
    rows, cls, box = _decode_inputs(B, T, N, seed=5)
    for tau in (0.0, 0.5):
        kw = dict(temperature=0.9, top_k=5, seed=77, keep_padded=1, tau=tau)
        ext = Call(dev, kind, rows, cls, box).run(1, "_ext", **kw)
        smp = Call(dev, kind, rows, cls, box).run(1, "_samples", clips=B, sample0=0, **kw)
        assert _same(ext.outputs(), smp.outputs())
        other = Call(dev, kind, rows, cls, box).run(1, "_samples", clips=B, sample0=1, **kw)
        assert not torch.equal(other.gen_cls.cpu(), ext.gen_cls.cpu())


@pytest.mark.parametrize("kind", KINDS)
def test_decode_samples_refusals_write_nothing(dev, kind):
    rows, cls, box = _decode_inputs(6, 4, 5, seed=6)
    for bad in (dict(clips=0), dict(clips=-2), dict(clips=4), dict(clips=12), dict(clips=2, sample0=-1),
                dict(clips=2, sample0=2 ** 31 - 3), dict(clips=6, sample0=2 ** 31 - 1), dict(clips=2, tau=-1.0),
                dict(clips=2, temperature=NAN)):
        c = Call(dev, kind, rows, cls, box)
        before = c.outputs()
        c.run(1, "_samples", expect=ERR_SHAPE, **dict(dict(sample0=0), **bad))
        for x, y in zip(before, c.outputs()):
            assert torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0)), bad
    Call(dev, kind, rows, cls, box).run(1, "_samples", clips=2, sample0=2 ** 31 - 4)      # the last sample index that fits


# -------------------------------------------------------------------------------------------------------- the score kernels
class Scored:
    """buffers of the three launches on one case, outputs pre-filled with sentinels"""

    def __init__(self, dev, K, B, S, N, seed, t0=2):
        self.K, self.B, self.S, self.N, self.t0 = K, B, S, N, t0
        self.host = R.score_case(K, B, S, N, seed, NC, t0)
        self.gen_cls, self.gen_box, self.clip_class, self.clip_box = (t.to(dev) for t in self.host)
        self.tgt_T = self.clip_class.shape[1]
        self.scores = torch.full((K, B, R.COLS), NAN, device=dev)
        self.div = torch.full((B, 2), NAN, device=dev)
        self.best = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.best_cls = torch.full((B, S, N), -1, dtype=torch.int64, device=dev)
        self.best_box = torch.full((B, S, N, 4), NAN, device=dev)
        self.record = torch.zeros(R.REC_SLOTS, dtype=torch.float64, device=dev)

    def score(self, expect=0, **over):
        from vlg import hip
        a = dict(gen_cls=self.gen_cls.data_ptr(), gen_box=self.gen_box.data_ptr(), clip_class=self.clip_class.data_ptr(),
                 clip_box=self.clip_box.data_ptr(), scores=self.scores.data_ptr(), K=self.K, B=self.B, S=self.S, N=self.N,
                 tgt_T=self.tgt_T, t0=self.t0, n_classes=NC, iou_eps=IOU_EPS)
        a.update(over)
        code = hip.load().vlg_layout_sample_scores(*a.values(), _stream())
        d = dict(a, div=self.div.data_ptr())
        del d["clip_box"], d["scores"]
        d = {k: d[k] for k in ("gen_cls", "gen_box", "clip_class", "div", "K", "B", "S", "N", "tgt_T", "t0", "n_classes", "iou_eps")}
        code2 = hip.load().vlg_layout_sample_diversity(*d.values(), _stream())
        torch.cuda.synchronize()
        assert (code, code2) == (expect, expect), (code, code2, over)
        return self

    def select(self, criterion, expect=0, **over):
        from vlg import hip
        a = dict(scores=self.scores.data_ptr(), div=self.div.data_ptr(), gen_cls=self.gen_cls.data_ptr(), gen_box=self.gen_box.data_ptr(),
                 best=self.best.data_ptr(), best_cls=self.best_cls.data_ptr(), best_box=self.best_box.data_ptr(),
                 record=self.record.data_ptr(), K=self.K, B=self.B, S=self.S, N=self.N, criterion=criterion)
        a.update(over)
        code = hip.load().vlg_layout_sample_select(*a.values(), _stream())
        torch.cuda.synchronize()
        assert code == expect, (code, over)
        return self

    def untouched(self):
        return (bool(torch.isnan(self.scores).all()) and bool(torch.isnan(self.div).all()) and bool((self.best == -1).all())
                and bool((self.best_cls == -1).all()) and bool(torch.isnan(self.best_box).all()) and bool((self.record == 0).all()))


def _close_nan(got, want, atol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN in other places" % what
    err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
    assert float(err.max()) <= atol, "%s: largest error %.3e (bar %g)" % (what, float(err.max()), atol)
    return float(err.max())


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_scores_diversity_selection_and_record(dev, K, B):
    worst = 0.0
    for S in (1, 3):
        for N in (1, 5, 64):
            c = Scored(dev, K, B, S, N, seed=1000 * K + 100 * B + 10 * S + N).score()
            gc, gb, cc, cb = c.host
            what = "K=%d B=%d S=%d N=%d" % (K, B, S, N)
            sc, div = c.scores.cpu().double().numpy(), c.div.cpu().double().numpy()
            worst = max(worst, _close_nan(sc, R.scores(gc, gb, cc, cb, c.t0, NC, IOU_EPS), 1e-5, what + " scores"),
                        _close_nan(div, R.diversity(gc, gb, cc, c.t0, NC, IOU_EPS), 1e-5, what + " diversity"))
            if K >= 3:
                nan_clip = min(1, B - 1)
                assert np.isnan(sc[K - 2, nan_clip, R.IOU]) and np.isnan(sc[K - 2, nan_clip, R.ADE])
            if K >= 2:
                assert sc[K - 1, 0, R.IOU] >= 1 - 1e-4 and sc[K - 1, 0, R.ADE] == 0 and sc[K - 1, 0, R.ACC] == 1
            if B >= 2:
                assert not sc[:, B - 1].any() and not div[B - 1].any()
            total = np.zeros(R.REC_SLOTS)
            for crit in R.SCORE_COLS:
                c.select(crit)
                best = c.best.cpu().numpy()
                assert np.array_equal(best, R.select(sc, crit)), (what, crit)
                if K >= 2 and crit != R.ACC:                                  # (an earlier sample may also hit every class)
                    assert best[0] == K - 1                                   # the planted truth
                pick = torch.from_numpy(best).long()
                assert torch.equal(c.best_cls.cpu(), gc[pick, torch.arange(B)])
                assert torch.equal(_bits(c.best_box.cpu()), _bits(gb[pick, torch.arange(B)]))
                total = total + R.record(sc, div, crit)
                rec = c.record.cpu().numpy()
                assert np.array_equal(np.isnan(rec), np.isnan(total)), (what, crit)
                np.testing.assert_allclose(rec, total, rtol=1e-9, atol=0, equal_nan=True, err_msg=what)
            # a second call on the same record gives exactly twice the sums of the first
            fresh = Scored(dev, K, B, S, N, seed=1000 * K + 100 * B + 10 * S + N).score()
            once = fresh.select(R.ADE).record.cpu().numpy().copy()
            twice = fresh.select(R.ADE).record.cpu().numpy()
            assert np.array_equal(twice, 2 * once, equal_nan=True), what
            assert torch.equal(_bits(fresh.scores.cpu()), _bits(c.scores.cpu())) and torch.equal(_bits(fresh.div.cpu()), _bits(c.div.cpu()))
    print("\nK=%d B=%d: largest |score or diversity - fp64| %.3e" % (K, B, worst))


def test_score_refusals_write_nothing(dev):
    K, B, S, N = 3, 2, 3, 5
    for over in (dict(K=0), dict(B=0), dict(S=0), dict(N=0), dict(t0=-1), dict(t0=4), dict(n_classes=0), dict(n_classes=29),
                 dict(S=4096, N=4097, tgt_T=5000)):
        c = Scored(dev, K, B, S, N, seed=1).score(expect=ERR_SHAPE, **over)
        assert c.untouched(), over
    c = Scored(dev, K, B, S, N, seed=1)
    c.score(expect=1002, gen_box=c.gen_box.data_ptr() + 4)                     # misaligned; and NULL
    c.score(expect=1002, gen_cls=0)
    from vlg import hip
    assert hip.load().vlg_layout_sample_scores(c.gen_cls.data_ptr(), c.gen_box.data_ptr(), c.clip_class.data_ptr(), c.clip_box.data_ptr(),
                                               c.gen_box.data_ptr(), K, B, S, N, c.tgt_T, c.t0, NC, IOU_EPS, _stream()) == ERR_SHAPE
    assert c.untouched()
    c.score()
    for over in (dict(criterion=-1), dict(criterion=4), dict(criterion=7), dict(K=0), dict(best_box=c.gen_box.data_ptr()),
                 dict(best_cls=c.gen_cls.data_ptr() + 8), dict(record=c.scores.data_ptr())):
        c.select(over.pop("criterion", 0), expect=ERR_SHAPE, **over)
        assert bool((c.best == -1).all()) and bool((c.record == 0).all()) and bool(torch.isnan(c.best_box).all()), over
    c.select(0, expect=1002, best=0)
    assert hip.load().vlg_layout_sample_record_slots() == R.REC_SLOTS
    from vlg import samples as VS
    assert (VS.COLS, VS.IOU, VS.ADE, VS.FDE, VS.ACC, VS.N_SCORED, VS.N_SCORED_LAST) == (R.COLS, R.IOU, R.ADE, R.FDE, R.ACC, R.N_SCORED, R.N_SCORED_LAST)
    assert (VS.REC_BEST, VS.REC_MEAN, VS.REC_SELECTED, VS.REC_DIV_BOX, VS.REC_DIV_CLASS, VS.REC_CLIPS, VS.REC_CLIPS_FDE, VS.REC_SLOTS) == (
        R.REC_BEST, R.REC_MEAN, R.REC_SELECTED, R.REC_DIV_BOX, R.REC_DIV_CLASS, R.REC_CLIPS, R.REC_CLIPS_FDE, R.REC_SLOTS)


# ---------------------------------------------------------------------------------------------------------------- the engine
ENG = dict(T=4, N=8, d=64, n_layers=2)
PB, FIT, S_GEN, K_ENG = 2, 2, 3, 5       # prompts per call; samples the workspace holds; generated frames; samples asked for
GEN = dict(temperature=0.8, top_k=5, seed=7)


def _engine(dev, attention="slot", precision="fp32", box_head="point"):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    return LayoutEngine(LayoutConfig(B=PB * FIT, attention=attention, box_head=box_head, **ENG), dev, seed=1024, precision=precision)


def _prompt(P, seed=3, pad=False):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, NC, (PB, P, ENG["N"]), generator=g)
    if pad:
        cls[:, :, 6:] = NC
    return cls, torch.rand(PB, P, ENG["N"], 4, generator=g)


def _names(eng, fn):
    seen, launch = [], eng._timed

    def counting(family, flops, name, *a, nbytes=0.0):
        seen.append(name)
        launch(family, flops, name, *a, nbytes=nbytes)

    eng._timed = counting
    try:
        out = fn()
    finally:
        del eng._timed
    return seen, out


def _check_samples(eng, dev, P, attention, bf16=False, box_temperature=0.0, keep_padded=False):
    """K_ENG samples on an engine that holds FIT of them: every generated frame of every sample step by step - CPU logits
    from the device's own history, then the restated draw - and the call against the concatenation of its own passes"""
    cfg, T, N = eng.cfg, ENG["T"], ENG["N"]
    pc, pb = _prompt(P, pad=keep_padded)
    kw = dict(steps=S_GEN, keep_padded=keep_padded, box_temperature=box_temperature, **GEN)
    gen_c, gen_b, logits = eng.rollout_samples(pc.to(dev), pb.to(dev), samples=K_ENG, return_logits=True, **kw)
    assert tuple(gen_c.shape) == (K_ENG, PB, S_GEN, N) and tuple(gen_b.shape) == (K_ENG, PB, S_GEN, N, 4)
    assert tuple(logits.shape) == (K_ENG, S_GEN, PB * N, cfg.n_out)
    parts = [eng.rollout_samples(pc.to(dev), pb.to(dev), samples=k, sample0=k0, return_logits=True, **kw) for k0, k in ((0, 2), (2, 2), (4, 1))]
    for i, got in enumerate((gen_c, gen_b, logits)):
        assert torch.equal(_bits(got), _bits(torch.cat([p[i] for p in parts], 0))), i
    out_c, out_b, logits = gen_c.cpu(), gen_b.cpu(), logits.cpu()
    assert bool(torch.isfinite(out_b).all())
    assert all(not torch.equal(out_b[j], out_b[k]) or not torch.equal(out_c[j], out_c[k]) for j in range(K_ENG) for k in range(j + 1, K_ENG))
    params = {k: v.cpu() for k, v in eng.named_params().items()}
    n_near = 0
    with torch.no_grad():
        for k in range(K_ENG):
            hist_c, hist_b = pc.clone(), pb.clone()
            for i in range(S_GEN):
                wc_, wb_ = hist_c[:, -T:], hist_b[:, -T:]
                wl, wr = O.forward(params, wc_, wb_, cfg.n_layers, attention=attention, valid=(wc_ < NC).float())
                want = torch.cat([wl[:, -1], wr[:, -1]], dim=-1).reshape(PB * N, cfg.n_out)
                if bf16:
                    e = float((logits[k, i] - want).norm() / want.norm())
                    assert bool(torch.isfinite(logits[k, i]).all()) and e <= 5e-2, (k, i, e)
                else:
                    check_close(logits[k, i], want, rtol=0, atol=1e-4 * float(wl[:, -1].abs().max()), what="sample %d step %d [logits | raw box]" % (k, i))
                wc, wb, near = R.next_frame(logits[k, i], wc_, wb_, NC, i, keep_padded=keep_padded, box_temperature=box_temperature,
                                            clips=PB, sample0=k, **GEN)
                assert torch.equal(out_c[k, :, i][~near], wc[~near]), (k, i)
                check_close(out_b[k, :, i], wb, rtol=0, atol=1e-6 if box_temperature == 0.0 else BH.box_bar(box_temperature),
                            what="sample %d step %d boxes" % (k, i))
                n_near += int(near.sum())
                hist_c = torch.cat([hist_c, out_c[k, :, i:i + 1]], dim=1)
                hist_b = torch.cat([hist_b, out_b[k, :, i:i + 1]], dim=1)
    assert n_near <= _near_bar(K_ENG * S_GEN * PB * N)
    return pc, pb, out_c, out_b


@pytest.mark.parametrize("P", [2, ENG["T"]], ids=["grow-then-slide", "full-prompt"])
def test_engine_samples_slot(dev, P):
    eng = _engine(dev)
    pc, pb, out_c, out_b = _check_samples(eng, dev, P, "slot")
    # sample 0 draws rollout()'s random numbers: the first frame is rollout()'s (a batch of FIT * PB clips may take other GEMM
    # plans than one of PB, so the logits agree to rounding, not to the bit; later frames condition on the drawn ones)
    c0, b0 = eng.rollout(pc.to(dev), pb.to(dev), steps=S_GEN, **GEN)
    assert torch.equal(c0[:, 0].cpu(), out_c[0, :, 0])
    check_close(b0[:, 0], out_b[0, :, 0], rtol=0, atol=1e-5, what="sample 0, first frame, against rollout()")
    # ... and a prompt's samples do not depend on the prompt beside it, nor on how many samples were asked for
    other_c, other_b = pc.clone(), pb.clone()
    other_c[1], other_b[1] = (other_c[1] + 1) % NC, 1.0 - other_b[1]
    c2, b2 = eng.rollout_samples(other_c.to(dev), other_b.to(dev), steps=S_GEN, samples=2, **GEN)
    assert torch.equal(c2[:, 0].cpu(), out_c[:2, 0]) and torch.equal(b2[:, 0].cpu(), out_b[:2, 0])
    assert not torch.equal(c2[:, 1].cpu(), out_c[:2, 1])


def test_engine_samples_clip_with_padded_slots(dev):
    _check_samples(_engine(dev, attention="clip"), dev, 2, "clip", keep_padded=True)


def test_engine_samples_bf16(dev):
    _check_samples(_engine(dev, precision="bf16"), dev, 2, "slot", bf16=True)


def test_engine_samples_gaussian_head(dev):
    eng = _engine(dev, box_head="gaussian")
    _check_samples(eng, dev, 2, "slot", box_temperature=0.8)
    # box draws alone make samples: temperature 0, box_temperature > 0
    pc, pb = _prompt(2)
    c, b = eng.rollout_samples(pc.to(dev), pb.to(dev), steps=2, samples=2, box_temperature=1.0, seed=3)
    assert torch.equal(c[0, :, 0], c[1, :, 0]) and not torch.equal(b[0, :, 0], b[1, :, 0])


def test_launches_without_samples_are_the_old_ones(dev):
    eng = _engine(dev)
    for P in (2, ENG["T"]):
        pc, pb = (t.to(dev) for t in _prompt(P))
        old, a = _names(eng, lambda: eng.rollout(pc, pb, steps=4, **GEN))
        one, b = _names(eng, lambda: eng.rollout_samples(pc, pb, steps=4, samples=1, **GEN))
        two, _ = _names(eng, lambda: eng.rollout_samples(pc, pb, steps=4, samples=2, **GEN))
        assert old == one and torch.equal(a[0], b[0][0]) and torch.equal(a[1], b[1][0])
        assert not any("_samples" in n for n in old)
        grown = min(ENG["T"] - P, 4)
        assert old.count("vlg_layout_decode_append") == grown and old.count("vlg_layout_decode") == 4 - grown
        assert old.count("vlg_head_last_frame") + old.count("vlg_head_frame") == 4
        # K samples: the same launches, the decode entries swapped
        assert two == [{"vlg_layout_decode": "vlg_layout_decode_samples", "vlg_layout_decode_append": "vlg_layout_decode_append_samples"}.get(n, n)
                       for n in old]


def test_evaluate_samples_matches_the_restatement(dev):
    eng = _engine(dev)
    P, N, K = 2, ENG["N"], 4
    g = torch.Generator().manual_seed(11)
    clip_c = torch.randint(0, NC, (PB, P + S_GEN, N), generator=g)
    clip_c[1, P + 1, 5] = NC                                                   # one padded truth slot
    clip_b = torch.cat([0.2 + 0.6 * torch.rand(PB, P + S_GEN, N, 2, generator=g), 0.1 + 0.4 * torch.rand(PB, P + S_GEN, N, 2, generator=g)], -1)
    dc, db = clip_c.to(dev).contiguous(), clip_b.to(dev).contiguous()
    for select in ("iou", "ade", "fde", "acc"):
        names, (rec, out) = _names(eng, lambda: eng.evaluate_samples(dc, db, samples=K, select=select, prompt_frames=P, return_samples=True, **{
            "temperature": GEN["temperature"], "sample_top_k": GEN["top_k"], "seed": GEN["seed"]}))
        assert names[-3:] == ["vlg_layout_sample_scores", "vlg_layout_sample_diversity", "vlg_layout_sample_select"]
        gc, gb = out["gen_cls"].cpu(), out["gen_box"].cpu()
        want_c, want_b = eng.rollout_samples(dc[:, :P], db[:, :P], steps=S_GEN, samples=K, **GEN)
        assert torch.equal(gc, want_c.cpu()) and torch.equal(gb, want_b.cpu())
        sc, div = R.scores(gc, gb, clip_c, clip_b, P, NC, IOU_EPS), R.diversity(gc, gb, clip_c, P, NC, IOU_EPS)
        crit = {"iou": R.IOU, "ade": R.ADE, "fde": R.FDE, "acc": R.ACC}[select]
        want, got = R.summary(R.record(sc, div, crit)), rec.summary()
        assert sorted(got) == sorted(want) and got["clips"] == PB
        assert set(got) >= {"best_iou", "best_ade", "best_fde", "best_acc", "mean_iou", "selected_ade", "diversity_box", "diversity_class", "clips"}
        for key in want:
            assert abs(got[key] - want[key]) <= 2e-5, (select, key, got[key], want[key])
        assert np.array_equal(out["best"].cpu().numpy(), R.select(out["scores"].cpu().numpy(), crit))
        assert got["best_ade"] <= got["mean_ade"] and got["best_iou"] >= got["mean_iou"] and got["diversity_class"] > 0
    # a given record is added to
    rec2 = eng.evaluate_samples(dc, db, samples=K, select="acc", prompt_frames=P, record=rec, temperature=GEN["temperature"],
                                sample_top_k=GEN["top_k"], seed=GEN["seed"])
    assert rec2 is rec and rec.summary()["clips"] == 2 * PB


def test_engine_refusals_enqueue_nothing(dev):
    eng = _engine(dev)
    pc, pb = (t.to(dev) for t in _prompt(2))
    seen = []
    eng._timed = lambda family, flops, name, *a, nbytes=0.0: seen.append(name)
    try:
        with pytest.raises(ValueError, match="argmax"):
            eng.rollout_samples(pc, pb, steps=2, samples=2)                         # both temperatures 0
        with pytest.raises(ValueError, match="capacity"):                           # not even one sample fits
            eng.rollout_samples(pc.repeat(3, 1, 1), pb.repeat(3, 1, 1, 1), steps=2, samples=2, **GEN)
        for bad in (dict(samples=0), dict(samples=2, sample0=-1), dict(samples=2, sample0=2 ** 31 - 2), dict(samples=1.5)):
            with pytest.raises(ValueError):
                eng.rollout_samples(pc, pb, steps=2, **dict(GEN, **bad))
        with pytest.raises(ValueError):
            eng.rollout_samples(pc, pb, steps=2, samples=2, box_temperature=0.5, **GEN)     # a point head draws no boxes
        clip_c, clip_b = torch.cat([pc, pc], 1).contiguous(), torch.cat([pb, pb], 1).contiguous()
        with pytest.raises(ValueError, match="select"):
            eng.evaluate_samples(clip_c, clip_b, samples=2, select="best", prompt_frames=2, **{"temperature": 0.8})
    finally:
        del eng._timed
    assert seen == []


# ---------------------------------------------------------------------------------------------------------------- the trainer
def test_trainer_knobs_reach_the_engine(tmp_path, monkeypatch, dev):
    from test_hip_layout_decode import _trainer
    for k in ("VLG_GEN_SAMPLES", "VLG_GEN_SELECT"):
        monkeypatch.delenv(k, raising=False)
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "slot")
    import trainer as TR
    assert TR.sample_knobs(tr.args) == {"samples": 1, "select": "iou"}
    eng, dev_ = tr.engine, tr.device
    P, S = 3, 4
    pc, pb = cls0[:, :P].contiguous(), box0[:, :P].contiguous()
    # unset: generate_sequence / evaluate_rollout are what they were, and generate_samples is that one sequence
    want_c, want_b = eng.rollout(pc.to(dev_), pb.to(dev_), steps=S, **GEN)
    out_c, out_b = tr.generate_sequence(pc, pb, steps=S, **GEN)
    assert torch.equal(out_c, want_c.cpu()) and torch.equal(out_b, want_b.cpu())
    one_c, one_b = tr.generate_samples(pc, pb, steps=S, **GEN)
    assert tuple(one_c.shape) == (1,) + tuple(out_c.shape) and torch.equal(one_c[0], out_c) and torch.equal(one_b[0], out_b)
    clip_c, clip_b = cls0[:, :P + S].contiguous(), box0[:, :P + S].contiguous()
    base = tr.evaluate_rollout(clip_c, clip_b, prompt_frames=P, **GEN)
    monkeypatch.setenv("VLG_GEN_SAMPLES", "3")
    monkeypatch.setenv("VLG_GEN_SELECT", "ade")
    assert TR.sample_knobs(tr.args) == {"samples": 3, "select": "ade"}
    seen = {}
    real = eng.evaluate_samples

    def spy(*a, **kw):
        seen.update(kw)
        return real(*a, **kw)

    eng.evaluate_samples = spy
    try:
        got = tr.evaluate_samples(clip_c, clip_b, prompt_frames=P, **GEN)
    finally:
        del eng.evaluate_samples
    assert seen["samples"] == 3 and seen["select"] == "ade" and seen["temperature"] == GEN["temperature"] and seen["seed"] == GEN["seed"]
    assert got["clips"] == cls0.shape[0] and got["best_ade"] <= got["mean_ade"] and got["selected_ade"] == got["best_ade"]
    gen_c, gen_b = tr.generate_samples(pc, pb, steps=S, **GEN)
    want = eng.rollout_samples(pc.to(dev_), pb.to(dev_), steps=S, samples=3, **GEN)
    assert tuple(gen_c.shape) == (3,) + tuple(out_c.shape) and torch.equal(gen_c, want[0].cpu()) and torch.equal(gen_b, want[1].cpu())
    assert torch.equal(gen_c[0], out_c) and torch.equal(gen_b[0], out_b) and not torch.equal(gen_c[1], gen_c[0])
    # the knobs do not touch the single-future methods
    again_c, again_b = tr.generate_sequence(pc, pb, steps=S, **GEN)
    assert torch.equal(again_c, out_c) and torch.equal(again_b, out_b)
    assert [s["accuracy"] for s in tr.evaluate_rollout(clip_c, clip_b, prompt_frames=P, **GEN)] == [s["accuracy"] for s in base]
    monkeypatch.setenv("VLG_GEN_SELECT", "best")
    with pytest.raises(ValueError):
        tr.evaluate_samples(clip_c, clip_b, prompt_frames=P, **GEN)
    monkeypatch.setenv("VLG_GEN_SELECT", "iou")
    monkeypatch.setenv("VLG_GEN_SAMPLES", "0")
    with pytest.raises(ValueError):
        tr.generate_samples(pc, pb, steps=S, **GEN)

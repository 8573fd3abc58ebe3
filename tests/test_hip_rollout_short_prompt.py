"""GPU: generation from a prompt of P < T frames (LayoutEngine.rollout, Trainer.generate_sequence / evaluate_rollout) -
the prompt pass, the cached grow steps, the hand-over to the sliding window and two slides - teacher-forced on the
rollout's own history: each step's [logits | raw box] against the CPU specification on the UNPADDED history (the window
once it slides), each decision against the restated decoding rule (tests/decode_ref.py).  Bars are the project's rollout
bars (tests/test_hip_layout_decode.py): atol 1e-4 x max |logits| for fp32 and fp32x3, relative Frobenius 5e-2 for bf16."""
import pytest
import torch

import decode_ref as D
import metrics_ref as R
from helpers import check_close
from oracle import layout_spec as O
from test_hip_layout_decode import GEN, _trainer
from test_hip_layout_metrics import _check as check_record

pytestmark = pytest.mark.gpu

T = 8                                     # test_hip_layout_decode.LAYOUT_CFG: B = 3, T = 8, N = 8, d = 64, 2 layers
PROMPTS = [1, 3, T - 1]
NAN = float("nan")


def _history_window(hist_c, hist_b):
    """what the model sees: the whole history while it fits the window, its last T frames after"""
    return hist_c[:, -T:], hist_b[:, -T:]


def _check_short(tr, cls0, box0, P, attention, bf16=False, cache=None, keep_padded=False):
    """steps = T - P + 3: the prompt pass, the grow steps, the hand-over at position T-1 and two slides"""
    dev, nc, cfg = tr.device, tr.cfg.n_classes, tr.cfg
    B, _, N = cls0.shape
    steps = T - P + 3
    pc, pb = cls0[:, :P].contiguous(), box0[:, :P].contiguous()
    params = {k: v.cpu() for k, v in tr.engine.named_params().items()}
    gen_c, gen_b, logits = tr.engine.rollout(pc.to(dev), pb.to(dev), steps=steps, keep_padded=keep_padded, return_logits=True,
                                             cache=cache, **GEN)
    assert gen_c.is_cuda and tuple(gen_c.shape) == (B, steps, N) and tuple(logits.shape) == (steps, B * N, cfg.n_out)
    out_c, out_b, logits = gen_c.cpu(), gen_b.cpu(), logits.cpu()
    assert bool(torch.isfinite(out_b).all())
    hist_c, hist_b, n_near = pc.clone(), pb.clone(), 0
    with torch.no_grad():
        for i in range(steps):
            wc_, wb_ = _history_window(hist_c, hist_b)
            wl, wr = O.forward(params, wc_, wb_, cfg.n_layers, attention=attention, valid=(wc_ < nc).float())
            want = torch.cat([wl[:, -1], wr[:, -1]], dim=-1).reshape(B * N, cfg.n_out)
            if bf16:
                e = float((logits[i] - want).norm() / want.norm())
                print("step %d: relative Frobenius error %.3e" % (i, e))
                assert bool(torch.isfinite(logits[i]).all()) and e <= 5e-2, (i, e)
            else:
                print("step %d: max |err| %.3e, bar %.3e" % (i, float((logits[i] - want).abs().max()), 1e-4 * float(wl[:, -1].abs().max())))
                check_close(logits[i], want, rtol=0, atol=1e-4 * float(wl[:, -1].abs().max()), what="P=%d step %d [logits | raw box]" % (P, i))
            wc, wb, near = D.next_frame(logits[i], wc_, wb_, nc, i, keep_padded=keep_padded, **GEN)
            assert torch.equal(out_c[:, i][~near], wc[~near]), (P, i)
            check_close(out_b[:, i], wb, rtol=0, atol=1e-6, what="P=%d step %d boxes" % (P, i))
            n_near += int(near.sum())
            hist_c = torch.cat([hist_c, out_c[:, i:i + 1]], dim=1)
            hist_b = torch.cat([hist_b, out_b[:, i:i + 1]], dim=1)
    assert n_near <= 0.01 * steps * B * N
    if keep_padded:
        pad = pc[:, -1] >= nc
        assert bool(pad.any()) and bool((out_c.transpose(1, 2)[pad] == nc).all()) and bool((out_c.transpose(1, 2)[~pad] < nc).all())
    else:
        assert bool((out_c < nc).all())
    return out_c, out_b


@pytest.mark.parametrize("precision,cache", [("fp32", None), ("fp32x3", None), ("bf16", None), ("fp32", False), ("bf16_mfma", None)],
                         ids=["fp32", "fp32x3", "bf16", "fp32-reencode", "bf16_mfma"])
def test_short_prompt_slot(tmp_path, monkeypatch, dev, precision, cache):
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "slot", precision=precision)
    assert tr.engine.precision == precision
    for P in PROMPTS:
        # bf16_mfma rounds a subset of what bf16 rounds (projection operands, no stored activation): that mode's bar
        _check_short(tr, cls0, box0, P, "slot", bf16=precision in ("bf16", "bf16_mfma"), cache=cache)


def test_short_prompt_clip(tmp_path, monkeypatch, dev):
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "clip")
    for P in PROMPTS:
        _check_short(tr, cls0, box0, P, "clip")
    # reserved ids in the prompt switch the masks on (the engine was built for fixed N), keep_padded carries them forward
    assert not tr.engine.padded_slots
    cls0 = cls0.clone()
    cls0[:, :, 5:] = tr.cfg.n_classes                    # the last three of eight slots padded in every frame
    cls0[1, :2, 1] = tr.cfg.n_classes                    # and one slot of one clip in its first two frames only
    _check_short(tr, cls0, box0, 3, "clip", keep_padded=True)
    assert tr.engine._masked
    _check_short(tr, cls0, box0, 3, "clip")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_cached_agrees_with_reencoding(tmp_path, monkeypatch, dev, precision):
    """temperature 0, frame by frame while the two histories are the same (argmax feeds back: one near-tie decided the
    other way changes every later frame of that clip, so the comparison ends at the first frame that differs - and a
    frame may differ only in tokens whose top-2 margin is not clear)"""
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "slot", precision=precision)
    bf16 = precision == "bf16"
    eng, dev_ = tr.engine, tr.device
    for P in PROMPTS:
        steps = T - P + 3
        pc, pb = cls0[:, :P].to(dev_).contiguous(), box0[:, :P].to(dev_).contiguous()
        a_c, a_b, a_l = (t.cpu() for t in eng.rollout(pc, pb, steps=steps, return_logits=True))
        b_c, b_b, b_l = (t.cpu() for t in eng.rollout(pc, pb, steps=steps, return_logits=True, cache=False))
        compared = 0
        for i in range(steps):
            l = b_l[i][:, :tr.cfg.n_classes]
            top2 = l.topk(2, dim=-1).values
            clear = ((top2[:, 0] - top2[:, 1]) > (5e-2 if bf16 else 1e-4) * float(l.abs().max())).view(a_c[:, i].shape)
            print("P=%d step %d: %.3f of the margins clear, max box difference %.3e" % (
                P, i, float(clear.float().mean()), float((a_b[:, i] - b_b[:, i]).abs().max())))
            assert torch.equal(a_c[:, i][clear], b_c[:, i][clear]), (P, i)
            assert bf16 or float(clear.float().mean()) > 0.9, (P, i)
            if bf16:
                assert float((a_b[:, i] - b_b[:, i]).norm() / b_b[:, i].norm()) <= 5e-2, (P, i)
            else:
                check_close(a_b[:, i], b_b[:, i], rtol=0, atol=1e-5, what="P=%d step %d boxes, cached vs re-encoded" % (P, i))
            compared += 1
            if not torch.equal(a_c[:, i], b_c[:, i]):
                break
        assert compared >= 2                              # the prompt pass (the same launches) and at least one cached step


def test_cache_reads_only_what_the_call_wrote(tmp_path, monkeypatch, dev):
    """poison: NaN in every cache row of positions >= P, in the frames >= P of the second window buffer and in the compact
    buffers before the call - the results are the same, bit for bit"""
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "slot")
    eng, dev_ = tr.engine, tr.device
    B, _, N = cls0.shape
    for P in PROMPTS:
        steps = T - P + 3
        pc, pb = cls0[:, :P].to(dev_).contiguous(), box0[:, :P].to(dev_).contiguous()
        want = [t.clone() for t in eng.rollout(pc, pb, steps=steps, return_logits=True, **GEN)]
        M = B * T * N
        eng.qkv[:, :M].unflatten(1, (B * N, T))[:, :, P:] = NAN
        c1, b1, v1 = eng._windows()[1]
        c1[:M].view(B, T, N)[:, P:] = -1
        b1[:M].view(B, T, N, 4)[:, P:] = NAN
        v1[:M].view(B, T, N)[:, P:] = NAN
        for name, buf in eng._grow_buffers().items():
            buf.fill_(-1 if name == "cls" else NAN)
        got = eng.rollout(pc, pb, steps=steps, return_logits=True, **GEN)
        for g, w in zip(got, want):
            assert torch.equal(g, w), P


def test_full_prompt_is_untouched_by_a_short_one(tmp_path, monkeypatch, dev):
    """P == T before and after a short-prompt call from the same engine: the same bits (no state leaks), and its launches
    are the sliding ones alone"""
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "slot")
    eng, dev_ = tr.engine, tr.device
    fc, fb = cls0.to(dev_).contiguous(), box0.to(dev_).contiguous()
    seen = []
    launch = eng._timed

    def counting(family, flops, name, *a, nbytes=0.0):
        seen.append(name)
        launch(family, flops, name, *a, nbytes=nbytes)

    eng._timed = counting
    try:
        before = [t.clone() for t in eng.rollout(fc, fb, steps=4, return_logits=True, **GEN)]
    finally:
        del eng._timed
    assert not {"vlg_head_frame", "vlg_layout_decode_append", "vlg_attention_step"} & set(seen)
    assert seen.count("vlg_head_last_frame") == 4 and seen.count("vlg_layout_decode") == 4 and seen.count("vlg_embed_fwd") == 4
    eng.rollout(fc[:, :3].contiguous(), fb[:, :3].contiguous(), steps=T, **GEN)
    eng.rollout(fc[:, :1].contiguous(), fb[:, :1].contiguous(), steps=3, cache=False, **GEN)
    after = eng.rollout(fc, fb, steps=4, return_logits=True, **GEN)
    for a, b in zip(after, before):
        assert torch.equal(a, b)


def test_trainer_passes_short_prompts_through(tmp_path, monkeypatch, dev):
    from vlg.spec import IOU_EPS
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "slot")
    eng, dev_, cfg = tr.engine, tr.device, tr.cfg
    B, _, N = cls0.shape
    P, S, C = 3, T - 3 + 2, cfg.n_classes
    want_c, want_b = eng.rollout(cls0[:, :P].to(dev_), box0[:, :P].to(dev_), steps=S, **GEN)
    out_c, out_b = tr.generate_sequence(cls0[:, :P], box0[:, :P], steps=S, **GEN)
    assert not out_c.is_cuda and torch.equal(out_c, want_c.cpu()) and torch.equal(out_b, want_b.cpu())
    # evaluate_rollout: the clip is (B, P+S, N), record row i is scored against clip frame P+i
    g = torch.Generator().manual_seed(4)
    clip_c = torch.cat([cls0[:, :P], torch.randint(0, C, (B, S, N), generator=g)], 1).contiguous()
    clip_c[1, P + 1, 5] = C                                                # one padded truth slot: unscored at step 1
    tail = torch.cat([0.2 + 0.6 * torch.rand(B, S, N, 2, generator=g), 0.1 + 0.4 * torch.rand(B, S, N, 2, generator=g)], -1)
    clip_b = torch.cat([box0[:, :P], tail], 1).contiguous()
    rec, gen_c, gen_b, logits = eng.evaluate_rollout(clip_c.to(dev_), clip_b.to(dev_), top_k=5, iou_thr=0.3, return_logits=True,
                                                     temperature=GEN["temperature"], sample_top_k=GEN["top_k"], seed=GEN["seed"],
                                                     prompt_frames=P)
    assert rec.rows == S and torch.equal(gen_c, want_c) and torch.equal(gen_b, want_b)
    counts, sums = rec.counts.cpu(), rec.sums.cpu()
    for i in range(S):
        o = logits[i].cpu().view(B, 1, N, cfg.n_out)
        ref = R.metrics_ref(o[..., :C].contiguous(), o[..., C:].contiguous(), clip_c, clip_b, None, 5, 0.3, IOU_EPS, t0=P + i)
        check_record(counts[i], sums[i], ref, "short-prompt rollout step %d" % i, iou_thr=0.3, tokens=B * N)
        assert int(counts[i][R.UNSCORED]) == (1 if i == 1 else 0)
    out = tr.evaluate_rollout(clip_c, clip_b, prompt_frames=P, val_topk=5, val_iou_thr=0.3, **GEN)
    assert len(out) == S and [s["scored"] for s in out] == [int(counts[i][R.SCORED]) for i in range(S)]
    assert [s["accuracy"] for s in out] == [s["accuracy"] for s in rec.summary()]
    # the default keeps its meaning: the first T frames prompt
    full_c, full_b = torch.cat([cls0, clip_c[:, P:P + 2]], 1).contiguous(), torch.cat([box0, clip_b[:, P:P + 2]], 1).contiguous()
    assert len(tr.evaluate_rollout(full_c, full_b, **GEN)) == 2
    with pytest.raises(ValueError):
        eng.evaluate_rollout(clip_c.to(dev_), clip_b.to(dev_), prompt_frames=0)
    with pytest.raises(ValueError):
        eng.evaluate_rollout(clip_c.to(dev_), clip_b.to(dev_), prompt_frames=T + 1)


@pytest.mark.parametrize("attention", ["slot", "clip"])
def test_refusals_enqueue_nothing(tmp_path, monkeypatch, dev, attention):
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, attention)
    eng, dev_ = tr.engine, tr.device
    fc, fb = cls0.to(dev_).contiguous(), box0.to(dev_).contiguous()
    seen = []
    eng._timed = lambda family, flops, name, *a, nbytes=0.0: seen.append(name)
    try:
        with pytest.raises(ValueError):
            eng.rollout(fc[:, :0], fb[:, :0], steps=2)                                 # P = 0
        with pytest.raises(ValueError):
            eng.rollout(torch.cat([fc, fc[:, :1]], 1), torch.cat([fb, fb[:, :1]], 1), steps=2)     # P = T + 1
        if attention == "clip":
            with pytest.raises(ValueError):
                eng.rollout(fc[:, :3].contiguous(), fb[:, :3].contiguous(), steps=2, cache=True)
    finally:
        del eng._timed
    assert seen == []
    # the host loop of an engine without rollout() takes a full prompt only, and says so
    class NoRollout:
        def __init__(self, e):
            self.e = e

        def __getattr__(self, k):
            if k in ("rollout", "evaluate_rollout"):
                raise AttributeError(k)
            return getattr(self.e, k)

    tr.engine = NoRollout(eng)
    try:
        with pytest.raises(ValueError, match="prompt of 3 frames"):
            tr.generate_sequence(cls0[:, :3], box0[:, :3], steps=2)
    finally:
        tr.engine = eng

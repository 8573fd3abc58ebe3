"""GPU: generation with attention = "factored" at (2,4,8), d = 64, 2 layers - the prompt pass, the cached grow steps (even
layers vlg_attention_step against the K/V cache, odd layers vlg_attention_frame_step on the rows the projection just wrote),
the hand-over to the sliding window and two slides - by the method of test_hip_rollout_short_prompt.py, teacher-forced on the
rollout's own history, against tests/factored_ref.py in fp64 and the decoding rule restated in tests/decode_ref.py.

Share of tokens left out (fp64 decision within decode_ref's exclusion width, 1e-5 of the kept mass, of a cumulative
boundary), computed on the CPU by rolling the fp64 reference out ALONE from the prompts used here (seed 21, sampling knobs
GEN, steps = T - P + 3): 0 of 96 / 80 / 64 / 48 tokens for P = 1 / 2 / 3 / 4, and 0 of 80 for the variable-N prompt (P = 2,
keep_padded) - 0.0 %, under the 1 % the tests allow."""
import pytest
import torch

import decode_ref as D
import factored_ref as R
from helpers import check_close, reference_args
from oracle import layout_spec as O
from test_hip_layout_decode import GEN

pytestmark = pytest.mark.gpu

KW = dict(B=2, T=4, N=8, d=64, n_layers=2)
T, NC = KW["T"], 20
PROMPTS = [1, 2, T - 1, T]
NAN = float("nan")


def prompt(variable_n=False):
    b = O.synthetic_batch(KW["B"], T, KW["N"], seed=21)
    cls, box = b["slot_class"].clone(), b["slot_box"].clone()
    if variable_n:
        cls[:, :, 5:] = NC                               # the last three of eight slots padded in every frame
        cls[1, :1, 1] = NC                               # and one slot of one clip in its first frame only
    return cls, box


def engine(dev, **opts):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    return LayoutEngine(LayoutConfig(attention="factored", **KW), dev, seed=1024, padded_slots=False, **opts)


def reference_step(p64, hist_c, hist_b):
    """[logits | raw box] (B*N, n_out) in fp64 that predict the frame after the history (its last T frames once it slides)"""
    wc, wb = hist_c[:, -T:], hist_b[:, -T:]
    with torch.no_grad():
        wl, wr = R.forward(p64, wc, wb.double(), KW["n_layers"], valid=(wc < NC).double())
    return torch.cat([wl[:, -1], wr[:, -1]], dim=-1).reshape(-1, NC + 4), wc, wb


def check_short(eng, cls0, box0, P, cache=None, keep_padded=False):
    dev = eng.device
    B, _, N = cls0.shape
    steps = T - P + 3
    pc, pb = cls0[:, :P].contiguous(), box0[:, :P].contiguous()
    p64 = {k: v.cpu().double() for k, v in eng.named_params().items()}
    gen_c, gen_b, logits = eng.rollout(pc.to(dev), pb.to(dev), steps=steps, keep_padded=keep_padded, return_logits=True, cache=cache, **GEN)
    out_c, out_b, logits = gen_c.cpu(), gen_b.cpu(), logits.cpu()
    assert bool(torch.isfinite(out_b).all()) and bool(torch.isfinite(logits).all())
    hist_c, hist_b, n_near = pc.clone(), pb.clone(), 0
    for i in range(steps):
        want, wc, wb = reference_step(p64, hist_c, hist_b)
        bar = 1e-4 * float(want[:, :NC].abs().max())
        print("P=%d step %d: max |err| vs fp64 %.3e, bar %.3e" % (P, i, float((logits[i].double() - want).abs().max()), bar))
        check_close(logits[i], want, rtol=0, atol=bar, what="P=%d step %d [logits | raw box]" % (P, i))
        ref_c, _, near = D.next_frame(want, wc, wb, NC, i, keep_padded=keep_padded, **GEN)       # the fp64 reference's decision
        assert torch.equal(out_c[:, i][~near], ref_c[~near]), (P, i)
        _, own_b, _ = D.next_frame(logits[i], wc, wb, NC, i, keep_padded=keep_padded, **GEN)     # boxes: the rule on the engine's own output
        check_close(out_b[:, i], own_b, rtol=0, atol=1e-6, what="P=%d step %d boxes" % (P, i))
        n_near += int(near.sum())
        hist_c = torch.cat([hist_c, out_c[:, i:i + 1]], dim=1)
        hist_b = torch.cat([hist_b, out_b[:, i:i + 1]], dim=1)
    assert n_near <= 0.01 * steps * B * N
    if keep_padded:
        pad = pc[:, -1] >= NC
        assert bool(pad.any()) and bool((out_c.transpose(1, 2)[pad] == NC).all()) and bool((out_c.transpose(1, 2)[~pad] < NC).all())
    else:
        assert bool((out_c < NC).all())


@pytest.mark.parametrize("cache", [None, False], ids=["cached", "reencode"])
@pytest.mark.parametrize("P", PROMPTS)
def test_short_prompt_factored(dev, P, cache):
    cls0, box0 = prompt()
    check_short(engine(dev), cls0, box0, P, cache=cache)


@pytest.mark.parametrize("precision", ["fp32x3", "bf16", "bf16_mfma"])
def test_short_prompt_factored_other_precisions(dev, precision):
    """fp32x3 at the fp32 bar; bf16 at the project's rollout bar for that mode (relative Frobenius 5e-2 per step), and bf16_mfma,
    which rounds a subset of what bf16 rounds, at the same bar"""
    cls0, box0 = prompt()
    eng = engine(dev, precision=precision)
    if precision == "fp32x3":
        check_short(eng, cls0, box0, 2)
        return
    p64 = {k: v.cpu().double() for k, v in eng.named_params().items()}
    P, steps = 2, T - 2 + 3
    gen_c, gen_b, logits = (t.cpu() for t in eng.rollout(cls0[:, :P].to(dev), box0[:, :P].to(dev), steps=steps, return_logits=True, **GEN))
    hist_c, hist_b = cls0[:, :P].clone(), box0[:, :P].clone()
    for i in range(steps):
        want, _, _ = reference_step(p64, hist_c, hist_b)
        e = float((logits[i].double() - want).norm() / want.norm())
        print("%s step %d: relative Frobenius error %.3e" % (precision, i, e))
        assert bool(torch.isfinite(logits[i]).all()) and e <= 5e-2, (i, e)
        hist_c, hist_b = torch.cat([hist_c, gen_c[:, i:i + 1]], 1), torch.cat([hist_b, gen_b[:, i:i + 1]], 1)


def test_variable_n_prompt_with_keep_padded(dev):
    cls0, box0 = prompt(variable_n=True)
    eng = engine(dev)
    check_short(eng, cls0, box0, 2, keep_padded=True)
    assert eng._masked, "reserved ids in the prompt must switch the odd layers' masks on"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_cached_agrees_with_reencoding(dev, precision):
    """the first frame comes from the same launches: bit for bit.  After it, argmax feeds back, so frame by frame while the
    two histories are the same: equal class ids wherever the top-2 margin is clear (test_hip_rollout_short_prompt.py)"""
    cls0, box0 = prompt()
    eng, bf16 = engine(dev, precision=precision), precision == "bf16"
    for P in (1, 2, T - 1):
        steps = T - P + 3
        pc, pb = cls0[:, :P].to(dev).contiguous(), box0[:, :P].to(dev).contiguous()
        a_c, a_b, a_l = (t.cpu() for t in eng.rollout(pc, pb, steps=steps, return_logits=True))
        b_c, b_b, b_l = (t.cpu() for t in eng.rollout(pc, pb, steps=steps, return_logits=True, cache=False))
        assert torch.equal(a_c[:, 0], b_c[:, 0]) and torch.equal(a_b[:, 0], b_b[:, 0]) and torch.equal(a_l[0], b_l[0])
        compared = 0
        for i in range(steps):
            l = b_l[i][:, :NC]
            top2 = l.topk(2, dim=-1).values
            clear = ((top2[:, 0] - top2[:, 1]) > (5e-2 if bf16 else 1e-4) * float(l.abs().max())).view(a_c[:, i].shape)
            assert torch.equal(a_c[:, i][clear], b_c[:, i][clear]), (P, i)
            assert bf16 or float(clear.float().mean()) > 0.9, (P, i)
            compared += 1
            if not torch.equal(a_c[:, i], b_c[:, i]):
                break
        assert compared >= 2


def test_cache_reads_only_what_the_call_wrote(dev):
    """NaN in every cache row of positions >= P (every layer), in the frames >= P of the second window buffer and in the
    compact buffers before the call: the same bits"""
    cls0, box0 = prompt()
    eng = engine(dev)
    B, _, N = cls0.shape
    M = B * T * N
    for P in (1, 2, T - 1):
        steps = T - P + 3
        pc, pb = cls0[:, :P].to(dev).contiguous(), box0[:, :P].to(dev).contiguous()
        want = [t.clone() for t in eng.rollout(pc, pb, steps=steps, return_logits=True, **GEN)]
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


def _names(eng, *a, **kw):
    seen, launch = [], eng._timed

    def recording(family, flops, name, *args, nbytes=0.0):
        seen.append(name)
        launch(family, flops, name, *args, nbytes=nbytes)

    eng._timed = recording
    try:
        eng.rollout(*a, **kw)
    finally:
        del eng._timed
    return seen


def test_launches_of_a_rollout(dev):
    """P == T launches no step kernel.  P < T: each grown frame is 1 + 7 L encoder launches + head + decode (31 at L = 4), its
    attention vlg_attention_step in the even layers and vlg_attention_frame_step in the odd ones; cache=False re-encodes"""
    cls0, box0 = prompt()
    eng = engine(dev)
    fc, fb = cls0.to(dev), box0.to(dev)
    L = KW["n_layers"]
    seen = _names(eng, fc, fb, steps=3, **GEN)
    assert not {"vlg_attention_step", "vlg_attention_frame_step", "vlg_head_frame", "vlg_layout_decode_append"} & set(seen)
    assert seen.count("vlg_attention_fwd") == 3 * (L - L // 2) and seen.count("vlg_attention_frame_fwd") == 3 * (L // 2)
    seen = _names(eng, fc[:, :1].contiguous(), fb[:, :1].contiguous(), steps=T - 1, **GEN)     # the prompt pass + T - 2 grown frames
    first = seen.index("vlg_layout_decode_append") + 1
    grown = seen[first:]
    assert len(grown) == (T - 2) * (1 + 7 * L + 2)
    per = grown[:1 + 7 * L + 2]
    assert [n for n in per if "attention" in n] == ["vlg_attention_step" if l % 2 == 0 else "vlg_attention_frame_step" for l in range(L)]
    assert seen.count("vlg_attention_frame_fwd") == L // 2                                       # the prompt pass alone
    seen = _names(eng, fc[:, :1].contiguous(), fb[:, :1].contiguous(), steps=T - 1, cache=False, **GEN)
    assert "vlg_attention_frame_step" not in seen and seen.count("vlg_attention_frame_fwd") == (T - 1) * (L // 2)


def test_trainer_passes_through(tmp_path, monkeypatch, dev):
    """VLG_ATTENTION=factored reaches the engine; generate_sequence and evaluate_rollout are the engine's rollout"""
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    for k in ("VLG_MODEL", "VLG_VARIABLE_N", "VLG_GEN_TEMPERATURE", "VLG_GEN_TOP_K", "VLG_GEN_SEED", "VLG_GEN_KEEP_PADDED", "VLG_PRECISION"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VLG_ATTENTION", "factored")
    from trainer import Trainer
    tr = Trainer(reference_args(tmp_path / "exp", batch_size=2, epochs=1, print_freq=1, n_frames=T, n_slots=8, d_model=64, n_layers=2,
                                train_clips=4, val_clips=2))
    assert tr.cfg.attention == "factored" and tr.engine.cfg.attention == "factored"
    batch = next(iter(tr.val_loader))
    cls0, box0 = batch["slot_class"].cpu().clone(), batch["slot_box"].cpu().clone()
    eng, d = tr.engine, tr.device
    P, S = 2, T - 2 + 2
    want_c, want_b = eng.rollout(cls0[:, :P].to(d), box0[:, :P].to(d), steps=S, **GEN)
    out_c, out_b = tr.generate_sequence(cls0[:, :P], box0[:, :P], steps=S, **GEN)
    assert not out_c.is_cuda and torch.equal(out_c, want_c.cpu()) and torch.equal(out_b, want_b.cpu())
    clip_c = torch.cat([cls0[:, :P], want_c.cpu()], 1).contiguous()                  # the model's own frames as the truth
    clip_b = torch.cat([box0[:, :P], want_b.cpu()], 1).contiguous()
    out = tr.evaluate_rollout(clip_c, clip_b, prompt_frames=P, val_topk=5, val_iou_thr=0.3, **GEN)
    assert len(out) == S and all(s["scored"] == clip_c.shape[0] * clip_c.shape[2] for s in out)
    rec = eng.evaluate_rollout(clip_c.to(d), clip_b.to(d), prompt_frames=P, top_k=5, iou_thr=0.3, temperature=GEN["temperature"],
                               sample_top_k=GEN["top_k"], seed=GEN["seed"])
    assert [s["accuracy"] for s in out] == [s["accuracy"] for s in rec.summary()]
    val = tr.validate()
    assert val["loss"] > 0.0 and val["loss"] == val["loss"]

"""GPU: generation from a prompt of P < T frames with per-clip attention and the opt-in K/V-cached step
(LayoutEngine(clip_cache=True), VLG_GEN_CLIP_CACHE=1): the grow steps run the encoder on the newest frame's rows against the
cache, with vlg_attention_clip_step as their attention.  Teacher-forced on the rollout's own history against the CPU
specification (test_hip_rollout_short_prompt._check_short, its bars unchanged), the launches by name, the cached rollout
against the re-encoded one, poisoned buffers, and the option off."""
import pytest
import torch

from helpers import check_close
from test_hip_layout_decode import GEN, _trainer
from test_hip_rollout_short_prompt import PROMPTS, T, _check_short

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _cached_trainer(tmp_path, monkeypatch, precision=None):
    monkeypatch.setenv("VLG_GEN_CLIP_CACHE", "1")
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "clip", precision=precision)
    assert tr.engine.clip_cache and tr.engine.cfg.attention == "clip"
    return tr, cls0, box0


def _masked_prompt(tr, cls0):
    """test_short_prompt_clip's: the last three of eight slots padded in every frame, one slot of one clip in two frames"""
    cls0 = cls0.clone()
    cls0[:, :, 5:] = tr.cfg.n_classes
    cls0[1, :2, 1] = tr.cfg.n_classes
    return cls0


def _names(eng, fn):
    """the launches of fn(), by name and in order"""
    seen, launch = [], eng._timed

    def counting(family, flops, name, *a, nbytes=0.0):
        seen.append(name)
        launch(family, flops, name, *a, nbytes=nbytes)

    eng._timed = counting
    try:
        fn()
    finally:
        del eng._timed
    return seen


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_short_prompt_clip_cached(tmp_path, monkeypatch, dev, precision):
    tr, cls0, box0 = _cached_trainer(tmp_path, monkeypatch, precision)
    assert tr.engine.precision == precision
    bf16 = precision == "bf16"
    for P in PROMPTS:
        _check_short(tr, cls0, box0, P, "clip", bf16=bf16)
    # reserved ids in the prompt switch the masks on (the engine was built for fixed N): the step reads the window's valid
    assert not tr.engine.padded_slots
    masked = _masked_prompt(tr, cls0)
    _check_short(tr, masked, box0, 3, "clip", bf16=bf16, keep_padded=True)
    assert tr.engine._masked
    _check_short(tr, masked, box0, 3, "clip", bf16=bf16)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_launches_by_name(tmp_path, monkeypatch, dev, precision):
    """P = 3, steps = T: the prompt pass on the window, T - 3 cached steps (engine.grow_schedule: positions 3 .. T-1, the last
    of them the hand-over that reads position T-1), then two slides on the window"""
    from vlg.engine import grow_schedule
    tr, cls0, box0 = _cached_trainer(tmp_path, monkeypatch, precision)
    eng, dev_ = tr.engine, tr.device
    L, P, steps = tr.cfg.n_layers, 3, T - 3 + 3
    pc, pb = cls0[:, :P].to(dev_).contiguous(), box0[:, :P].to(dev_).contiguous()
    step, fwd = "vlg_attention_clip_step" + eng._sfx, "vlg_attention_clip_fwd" + eng._sfx
    sched = grow_schedule(P, T, steps, True)
    n_step = sum(e == "step" for e, _, _ in sched)
    assert n_step == T - P and [e for e, _, _ in sched] == ["window"] + ["step"] * n_step + ["window"] * (steps - 1 - n_step)
    for cache in (None, True):
        seen = _names(eng, lambda: eng.rollout(pc, pb, steps=steps, cache=cache, **GEN))
        assert seen.count(step) == L * n_step and seen.count(fwd) == L * (steps - n_step), cache
        att = [n for n in seen if n in (step, fwd)]
        assert att == [fwd] * L + [step] * (L * n_step) + [fwd] * (L * (steps - 1 - n_step))       # prompt pass, steps, slides
        assert "vlg_attention_step" + eng._sfx not in seen
    seen = _names(eng, lambda: eng.rollout(pc, pb, steps=steps, cache=False, **GEN))
    assert step not in seen and seen.count(fwd) == L * steps


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_cached_agrees_with_reencoding(tmp_path, monkeypatch, dev, precision):
    """as test_hip_rollout_short_prompt.test_cached_agrees_with_reencoding, with its margins: temperature 0, frame by frame
    while the two histories are the same"""
    tr, cls0, box0 = _cached_trainer(tmp_path, monkeypatch, precision)
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


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_cache_reads_only_what_the_call_wrote(tmp_path, monkeypatch, dev, masked):
    """poison: NaN in every cache row of positions >= P, in the frames >= P of the second window buffer and in the compact
    buffers before the call - the results are the same, bit for bit"""
    tr, cls0, box0 = _cached_trainer(tmp_path, monkeypatch)
    if masked:
        cls0 = _masked_prompt(tr, cls0)
    eng, dev_ = tr.engine, tr.device
    B, _, N = cls0.shape
    for P in PROMPTS:
        steps = T - P + 3
        pc, pb = cls0[:, :P].to(dev_).contiguous(), box0[:, :P].to(dev_).contiguous()
        want = [t.clone() for t in eng.rollout(pc, pb, steps=steps, return_logits=True, **GEN)]
        assert eng._masked == masked
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


def test_option_off_is_the_engine_as_it_was(tmp_path, monkeypatch, dev):
    monkeypatch.delenv("VLG_GEN_CLIP_CACHE", raising=False)
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "clip")
    eng, dev_ = tr.engine, tr.device
    assert not eng.clip_cache
    pc, pb = cls0[:, :3].to(dev_).contiguous(), box0[:, :3].to(dev_).contiguous()
    seen = []
    eng._timed = lambda family, flops, name, *a, nbytes=0.0: seen.append(name)
    try:
        with pytest.raises(ValueError, match="clip_cache"):
            eng.rollout(pc, pb, steps=2, cache=True)
    finally:
        del eng._timed
    assert seen == []
    seen = _names(eng, lambda: eng.rollout(pc, pb, steps=T, **GEN))
    assert "vlg_attention_clip_step" not in seen and seen.count("vlg_attention_clip_fwd") == tr.cfg.n_layers * T

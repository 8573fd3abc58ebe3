"""GPU: generation on the device - vlg_head_last_frame and vlg_layout_decode launch by launch against fp64 / the CPU
restatement of the decoding rule (tests/decode_ref.py), then LayoutEngine.rollout and Trainer.generate_sequence end to end,
teacher-forced on the rollout's own windows.  Every output buffer starts as NaN / -1 sentinels."""
import pytest
import torch
import torch.nn.functional as F

import decode_ref as D
from helpers import check_close, reference_args, vs_cpu32
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

NC = 20                     # classes; out_last rows are [20 logits | 4 raw box values]
ERR_SHAPE = 1001
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ vlg_head_last_frame
def _head_case(B, T, N, d, n_out, seed):
    g = torch.Generator().manual_seed(seed)
    M = B * N * T
    mean = (torch.rand(M, 1, generator=g) * 2 - 1) * 3                     # per-row mean up to +-3
    scale = 10.0 ** (torch.rand(M, 1, generator=g) * 2 - 1)                # per-row scale 0.1 .. 10
    x = torch.randn(M, d, generator=g) * scale + mean
    last = torch.arange(B * N) * T + (T - 1)
    keep = torch.zeros(M, dtype=torch.bool)
    keep[last] = True
    x[~keep] = NAN                                                         # a row that is not a last-frame row must not be read
    gamma, beta = 1 + 0.5 * torch.randn(d, generator=g), 0.5 * torch.randn(d, generator=g)
    w, b = torch.randn(n_out, d, generator=g) / d ** 0.5, torch.randn(n_out, generator=g)
    return x, gamma, beta, w, b, last


def _head_ref(x, gamma, beta, w, b, last, dt):
    xl = x[last].to(dt)
    return F.linear(F.layer_norm(xl, (x.shape[1],), gamma.to(dt), beta.to(dt), 1e-5), w.to(dt), b.to(dt))


@pytest.mark.parametrize("B,T,N,d", [(1, 4, 1, 64), (3, 8, 5, 64), (2, 16, 7, 192), (2, 4, 33, 256), (1, 32, 3, 512)])
def test_head_last_frame_vs_fp64(dev, B, T, N, d):
    from vlg import hip
    x, gamma, beta, w, b, last = _head_case(B, T, N, d, 24, seed=B * 1000 + d)
    out = torch.full((B * N, 24), NAN, device=dev)
    dv = [t.to(dev) for t in (x, gamma, beta, w, b)]
    hip.call("vlg_head_last_frame", *[t.data_ptr() for t in dv], out.data_ptr(), B, T, N, d, 24, 1e-5, _stream())
    vs_cpu32(out, _head_ref(x, gamma, beta, w, b, last, torch.float64), _head_ref(x, gamma, beta, w, b, last, torch.float32),
             "head on the last frame (%d,%d,%d) d=%d" % (B, T, N, d))


@pytest.mark.parametrize("d,n_out", [(96, 24), (64, 33)])
def test_head_last_frame_refuses_shapes(dev, d, n_out):
    from vlg import hip
    B, T, N = 2, 4, 3
    x = torch.randn(B * N * T, d, device=dev)
    gamma, beta = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    w, b = torch.randn(n_out, d, device=dev), torch.zeros(n_out + 3, device=dev)
    out = torch.full((B * N, n_out), NAN, device=dev)
    code = hip.load().vlg_head_last_frame(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr(), b.data_ptr(),
                                          out.data_ptr(), B, T, N, d, n_out, 1e-5, _stream())
    torch.cuda.synchronize()
    assert code == ERR_SHAPE and bool(torch.isnan(out).all())


# -------------------------------------------------------------------------------------------------- vlg_layout_decode
class Step:
    """buffers of one vlg_layout_decode call, outputs pre-filled with sentinels"""

    def __init__(self, dev, out_last, cls_in, box_in, steps):
        B, T, N = cls_in.shape
        self.shape, self.steps = (B, T, N), steps
        self.out_last, self.cls_in, self.box_in = out_last.to(dev).contiguous(), cls_in.to(dev).contiguous(), box_in.to(dev).contiguous()
        self.cls_out = torch.full((B, T, N), -1, dtype=torch.int64, device=dev)
        self.box_out = torch.full((B, T, N, 4), NAN, device=dev)
        self.valid_out = torch.full((B, T, N), NAN, device=dev)
        self.gen_cls = torch.full((B, steps, N), -1, dtype=torch.int64, device=dev)
        self.gen_box = torch.full((B, steps, N, 4), NAN, device=dev)

    def args(self, step, temperature=0.0, top_k=0, seed=0, keep_padded=0, n_classes=NC, **over):
        B, T, N = self.shape
        a = dict(out_last=self.out_last.data_ptr(), cls_in=self.cls_in.data_ptr(), box_in=self.box_in.data_ptr(),
                 cls_out=self.cls_out.data_ptr(), box_out=self.box_out.data_ptr(), valid_out=self.valid_out.data_ptr(),
                 gen_cls=self.gen_cls.data_ptr(), gen_box=self.gen_box.data_ptr(), B=B, T=T, N=N, n_classes=n_classes,
                 steps=self.steps, step=step, temperature=temperature, top_k=top_k, seed=seed, keep_padded=keep_padded)
        a.update(over)
        return list(a.values()) + [_stream()]

    def run(self, step, **kw):
        from vlg import hip
        hip.call("vlg_layout_decode", *self.args(step, **kw))
        return self.gen_cls[:, step].cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.cls_out == -1).all()) and bool(torch.isnan(self.box_out).all()) and bool(torch.isnan(self.valid_out).all())
                and bool((self.gen_cls == -1).all()) and bool(torch.isnan(self.gen_box).all()))


def _window(B, T, N, seed, vocab=NC + 1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, vocab, (B, T, N), generator=g), torch.rand(B, T, N, 4, generator=g)


def _rows(R, seed, scale=3.0):
    return torch.randn(R, NC + 4, generator=torch.Generator().manual_seed(seed)) * scale


def test_argmax_step(dev):
    B, T, N, steps, step = 3, 8, 5, 4, 2
    out_last = _rows(B * N, 1)
    out_last[4, 3] = out_last[4, 11] = 50.0                                # exact tie: the first maximum wins
    cls_in, box_in = _window(B, T, N, 2)                                   # holds the reserved id 20 here and there
    s = Step(dev, out_last, cls_in, box_in, steps)
    got = s.run(step)
    want = out_last[:, :NC].argmax(-1).view(B, N)
    assert int(want[0, 4]) == 3 and torch.equal(got, want)
    want_box = torch.sigmoid(out_last[:, NC:].double()).view(B, N, 4)
    check_close(s.gen_box[:, step], want_box, rtol=0, atol=1e-6, what="generated boxes")
    # the next window, bitwise
    new_box = s.gen_box[:, step].cpu()
    wc, wb = D.slide(cls_in, box_in, got, new_box)
    assert torch.equal(s.cls_out.cpu(), wc) and torch.equal(s.box_out.cpu(), wb)
    assert torch.equal(s.valid_out.cpu(), (wc < NC).float()) and bool((s.valid_out == 0).any())
    assert torch.equal(s.cls_in.cpu(), cls_in) and torch.equal(s.box_in.cpu(), box_in) and torch.equal(s.out_last.cpu(), out_last)
    other = [i for i in range(steps) if i != step]
    assert bool((s.gen_cls[:, other] == -1).all()) and bool(torch.isnan(s.gen_box[:, other]).all())
    # valid_out may be NULL
    s2 = Step(dev, out_last, cls_in, box_in, steps)
    assert torch.equal(s2.run(step, valid_out=0), want) and bool(torch.isnan(s2.valid_out).all())
    assert torch.equal(s2.cls_out.cpu(), wc)


@pytest.mark.parametrize("temperature", [1.0, 0.7, 2.5])
def test_sampling_matches_the_restatement(dev, temperature):
    B, N, T, steps, seed = 3, 37, 2, 4, 0xC0FFEE12345
    out_last = _rows(B * N, 3)
    out_last[5, 2] = out_last[5, 9] = out_last[5, 14] = 7.5                # equal logits at the top-k edge: lower index first
    cls_in, box_in = _window(B, T, N, 4, vocab=NC)
    l64 = out_last[:, :NC].double().numpy()
    s, flat, again, other = (Step(dev, out_last, c, b, steps) for c, b in
                             [(cls_in, box_in), (cls_in.view(1, T, B * N), box_in.view(1, T, B * N, 4))] + [(cls_in, box_in)] * 2)
    for top_k in (0, 1, 5, 20):
        n_near = 0
        for step in range(steps):
            got = s.run(step, temperature=temperature, top_k=top_k, seed=seed).view(-1)
            want, near = D.decode_step(l64, step, temperature, top_k, seed)
            want, clear = torch.from_numpy(want), torch.from_numpy(~near)
            assert torch.equal(got[clear], want[clear]), (top_k, step)
            assert bool(((got >= 0) & (got < NC)).all())
            n_near += int(near.sum())
            if top_k == 1:
                assert torch.equal(got, out_last[:, :NC].argmax(-1))
            # the counter is the token index, not the launch geometry; the same seed gives the same draw, another one does not
            assert torch.equal(flat.run(step, temperature=temperature, top_k=top_k, seed=seed).view(-1), got)
            assert torch.equal(again.run(step, temperature=temperature, top_k=top_k, seed=seed).view(-1), got)
            if top_k != 1:
                assert not torch.equal(other.run(step, temperature=temperature, top_k=top_k, seed=seed + 1).view(-1), got)
        print("\ntemperature %g top_k %d: %d of %d draws within 1e-5 S of a boundary" % (temperature, top_k, n_near, steps * B * N))
        assert n_near <= 0.01 * steps * B * N
    assert torch.equal(again.gen_box.cpu(), s.gen_box.cpu()) and torch.equal(again.cls_out.cpu(), s.cls_out.cpu())


@pytest.mark.parametrize("temperature,top_k", D.DIST_CASES)
def test_kernel_draws_the_distribution(dev, temperature, top_k):
    B = N = 64
    assert B * N == D.DIST_TOKENS
    out_last = torch.zeros(B * N, NC + 4)
    out_last[:, :NC] = D.distribution_row()
    cls_in, box_in = _window(B, 1, N, 5, vocab=NC)
    s = Step(dev, out_last, cls_in, box_in, D.DIST_STEPS)
    for step in range(D.DIST_STEPS):
        s.run(step, temperature=temperature, top_k=top_k, seed=D.DIST_SEED)
    D.check_distribution(s.gen_cls.cpu(), temperature, top_k)


def test_keep_padded(dev):
    B, T, N, steps = 3, 4, 5, 2
    out_last = _rows(B * N, 6)
    cls_in, box_in = _window(B, T, N, 7, vocab=NC)
    cls_in[0, -1, 1] = cls_in[2, -1, 4] = NC                               # padded in the last frame
    cls_in[1, 0, 2] = cls_in[1, 1, 2] = NC                                 # padded in earlier frames only
    pad = cls_in[:, -1] >= NC
    argmax = out_last[:, :NC].argmax(-1).view(B, N)
    on, off = Step(dev, out_last, cls_in, box_in, steps), Step(dev, out_last, cls_in, box_in, steps)
    got_on, got_off = on.run(1, keep_padded=1), off.run(1, keep_padded=0)
    assert torch.equal(got_off, argmax)                                   # off: every slot is decoded
    assert torch.equal(got_on[~pad], argmax[~pad]) and bool((got_on[pad] == NC).all())
    gb = on.gen_box[:, 1].cpu()
    assert torch.equal(gb[pad], box_in[:, -1][pad]) and torch.equal(gb[~pad], off.gen_box[:, 1].cpu()[~pad])
    assert torch.equal(on.cls_out[:, -1].cpu(), got_on) and torch.equal(on.box_out[:, -1].cpu(), gb)
    assert torch.equal(on.valid_out[:, -1].cpu(), (~pad).float()) and bool((off.valid_out[:, -1] == 1).all())
    # sampling keeps them too, and draws the other slots as the rule says
    got_s = Step(dev, out_last, cls_in, box_in, steps).run(0, temperature=1.3, top_k=7, seed=11, keep_padded=1)
    want, _, near = D.next_frame(out_last, cls_in, box_in, NC, 0, 1.3, 7, 11, keep_padded=True)
    assert torch.equal(got_s[~near], want[~near]) and bool((got_s[pad] == NC).all()) and int(near.sum()) <= 1
    # a reserved id in earlier frames only changes nothing in the generated frame
    plain = cls_in.clone()
    plain[1, 0, 2] = plain[1, 1, 2] = 0
    ref = Step(dev, out_last, plain, box_in, steps)
    assert torch.equal(ref.run(1, keep_padded=1), got_on) and torch.equal(ref.gen_box[:, 1].cpu(), gb)


def test_refusals_enqueue_nothing(dev):
    from vlg import hip
    B, T, N, steps = 2, 4, 6, 3
    cls_in, box_in = _window(B, T, N, 8)
    s = Step(dev, torch.zeros(B * N, 32), cls_in, box_in, steps)           # (rows wide enough for any n_classes below)
    f = hip.load().vlg_layout_decode
    bad = [dict(temperature=-0.5), dict(temperature=float("inf")), dict(temperature=NAN), dict(top_k=-1), dict(top_k=NC + 1),
           dict(n_classes=0), dict(n_classes=29), dict(step=-1), dict(step=steps), dict(B=0), dict(T=0), dict(N=0),
           dict(cls_out=s.cls_in.data_ptr()), dict(box_out=s.box_in.data_ptr()),                       # in == out
           dict(cls_out=s.cls_in.data_ptr() + 8 * N), dict(gen_box=s.box_in.data_ptr() + 16)]          # partial overlap
    for over in bad:
        step = over.pop("step", 1)
        assert f(*s.args(step, **over)) == ERR_SHAPE, over
        assert s.untouched(), over
    assert torch.equal(s.cls_in.cpu(), cls_in) and torch.equal(s.box_in.cpu(), box_in)
    assert f(*s.args(1)) == 0                                              # and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert not s.untouched()


# ------------------------------------------------------------------------------------------------------- end to end
LAYOUT_CFG = dict(batch_size=3, epochs=1, print_freq=1, n_frames=8, n_slots=8, d_model=64, n_layers=2, train_clips=6,
                  val_clips=3)
GEN = dict(temperature=0.8, top_k=5, seed=7)


def _host_step(tr, cls, box):
    """one frame of the host loop the Trainer ran before rollout(): the training forward on dummy targets, then
    outputs_btn() -> (logits (B,N,C), raw (B,N,4)) of the last frame"""
    dev = tr.device
    cls, box = cls.to(dev).contiguous(), box.to(dev).contiguous()
    valid = (cls < tr.cfg.n_classes).float()
    kw = {"padded_slots": True} if not tr.engine.padded_slots and bool((valid == 0).any()) else {}
    tr.engine.forward({"slot_class": cls, "slot_box": box, "valid": valid, "tgt_class": torch.zeros_like(cls),
                       "tgt_box": torch.zeros_like(box)}, **kw)
    logits, raw = tr.engine.outputs_btn()
    return logits[:, -1].cpu(), raw[:, -1].cpu()


def _check_rollout(tr, cls0, box0, attention, steps=8, keep_padded=False, bf16=False):
    """rollout(return_logits=True) and generate_sequence, teacher-forced on the rollout's own windows: each step's logits
    and raw boxes vs the CPU specification, its decisions vs the restated rule on the engine's own logits; then the
    argmax rollout vs the host loop it replaces."""
    dev, nc, cfg = tr.device, tr.cfg.n_classes, tr.cfg
    B, T, N = cls0.shape
    params = {k: v.cpu() for k, v in tr.engine.named_params().items()}
    gen_c, gen_b, logits = tr.engine.rollout(cls0.to(dev), box0.to(dev), steps=steps, keep_padded=keep_padded,
                                             return_logits=True, **GEN)
    assert gen_c.is_cuda and gen_b.is_cuda and tuple(logits.shape) == (steps, B * N, cfg.n_out)
    out_c, out_b = tr.generate_sequence(cls0, box0, steps=steps, keep_padded=keep_padded, **GEN)
    assert not out_c.is_cuda and out_c.dtype == torch.int64 and out_b.dtype == torch.float32
    assert out_c.shape == (B, steps, N) and out_b.shape == (B, steps, N, 4)
    assert torch.equal(out_c, gen_c.cpu()) and torch.equal(out_b, gen_b.cpu())
    assert bool(torch.isfinite(out_b).all())
    logits = logits.cpu()
    cls, box, n_near = cls0.clone(), box0.clone(), 0
    with torch.no_grad():
        for i in range(steps):
            wl, wr = O.forward(params, cls, box, cfg.n_layers, attention=attention, valid=(cls < nc).float())
            want = torch.cat([wl[:, -1], wr[:, -1]], dim=-1).reshape(B * N, cfg.n_out)
            if bf16:
                e = float((logits[i] - want).norm() / want.norm())
                assert bool(torch.isfinite(logits[i]).all()) and e <= 5e-2, (i, e)
            else:
                check_close(logits[i], want, rtol=0, atol=1e-4 * float(wl[:, -1].abs().max()), what="step %d [logits | raw box]" % i)
            wc, wb, near = D.next_frame(logits[i], cls, box, nc, i, keep_padded=keep_padded, **GEN)
            assert torch.equal(out_c[:, i][~near], wc[~near]), i
            check_close(out_b[:, i], wb, rtol=0, atol=1e-6, what="step %d boxes" % i)
            n_near += int(near.sum())
            cls, box = D.slide(cls, box, out_c[:, i], out_b[:, i])
    assert n_near <= 0.01 * steps * B * N
    if keep_padded:
        pad = cls0[:, -1] >= nc
        assert bool(pad.any()) and bool((out_c.transpose(1, 2)[pad] == nc).all()) and bool((out_c.transpose(1, 2)[~pad] < nc).all())
    else:
        assert bool((out_c < nc).all())
    # temperature 0 (the Trainer's default) vs the host loop, frame by frame on the rollout's own windows
    arg_c, arg_b = tr.generate_sequence(cls0, box0, steps=steps)
    cls, box = cls0.clone(), box0.clone()
    for i in range(steps):
        hl, hr = _host_step(tr, cls, box)
        top2 = hl.topk(2, dim=-1).values
        # (bf16: the host loop's final norm and head run on bf16 operands, rollout's on the fp32 masters - that mode's bars)
        clear = (top2[..., 0] - top2[..., 1]) > (5e-2 if bf16 else 1e-4) * float(hl.abs().max())
        assert bool((arg_c[:, i][clear] == hl.argmax(-1)[clear]).all()) and (bf16 or float(clear.float().mean()) > 0.9), i
        if bf16:
            assert float((arg_b[:, i] - torch.sigmoid(hr)).norm() / torch.sigmoid(hr).norm()) <= 5e-2, i
        else:
            check_close(arg_b[:, i], torch.sigmoid(hr), rtol=0, atol=1e-5, what="argmax rollout boxes, step %d" % i)
        cls, box = D.slide(cls, box, arg_c[:, i], arg_b[:, i])


def _trainer(tmp_path, monkeypatch, attention, precision=None):
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    for k in ("VLG_MODEL", "VLG_VARIABLE_N", "VLG_GEN_TEMPERATURE", "VLG_GEN_TOP_K", "VLG_GEN_SEED", "VLG_GEN_KEEP_PADDED"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VLG_ATTENTION", attention)
    monkeypatch.setenv("VLG_PRECISION", precision or "fp32")
    from trainer import Trainer
    tr = Trainer(reference_args(tmp_path / "exp", **LAYOUT_CFG))
    batch = next(iter(tr.val_loader))
    return tr, batch["slot_class"].cpu().clone(), batch["slot_box"].cpu().clone()


@pytest.mark.parametrize("attention", ["slot", "clip"])
def test_rollout_end_to_end(tmp_path, monkeypatch, dev, attention):
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, attention)
    _check_rollout(tr, cls0, box0, attention)


def test_rollout_clip_with_reserved_ids_at_fixed_n(tmp_path, monkeypatch, dev):
    """the engine was built without masks (fixed N): the prompt's reserved ids switch them on before the loop, the decode
    kernel's valid_out carries them from window to window"""
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "clip")
    assert not tr.engine.padded_slots
    cls0[:, :, 5:] = tr.cfg.n_classes                    # the last three of eight slots padded in every frame
    cls0[1, :3, 1] = tr.cfg.n_classes                    # and one slot of one clip in its first three frames only
    _check_rollout(tr, cls0, box0, "clip")
    _check_rollout(tr, cls0, box0, "clip", keep_padded=True)


def test_rollout_bf16(tmp_path, monkeypatch, dev):
    tr, cls0, box0 = _trainer(tmp_path, monkeypatch, "clip", precision="bf16")
    assert tr.engine.precision == "bf16"
    _check_rollout(tr, cls0, box0, "clip", bf16=True)

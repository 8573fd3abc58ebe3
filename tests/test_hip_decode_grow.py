"""GPU: the generation tail while the history grows - vlg_head_frame (the head on any frame of the window) against fp64,
and vlg_layout_decode_append (decode in place, nothing slides) against the CPU restatement of the decoding rule
(tests/decode_ref.py) and against vlg_layout_decode on the same rows.  Every output buffer starts as NaN / -1 sentinels."""
import pytest
import torch

import decode_ref as D
from helpers import check_close, vs_cpu32
from test_hip_layout_decode import NC, Step, _head_ref, _rows, _window

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ALIGN = 1001, 1002
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------------------------- vlg_head_frame
def _head_case(B, T, N, d, n_out, t_read, seed):
    """test_hip_layout_decode._head_case with the kept rows at frame t_read: every other row holds NaN"""
    g = torch.Generator().manual_seed(seed)
    M = B * N * T
    mean = (torch.rand(M, 1, generator=g) * 2 - 1) * 3
    scale = 10.0 ** (torch.rand(M, 1, generator=g) * 2 - 1)
    x = torch.randn(M, d, generator=g) * scale + mean
    rows = torch.arange(B * N) * T + t_read
    keep = torch.zeros(M, dtype=torch.bool)
    keep[rows] = True
    x[~keep] = NAN
    gamma, beta = 1 + 0.5 * torch.randn(d, generator=g), 0.5 * torch.randn(d, generator=g)
    w, b = torch.randn(n_out, d, generator=g) / d ** 0.5, torch.randn(n_out, generator=g)
    return x, gamma, beta, w, b, rows


@pytest.mark.parametrize("B,T,N,d", [(1, 4, 1, 64), (3, 8, 5, 64), (2, 16, 7, 192), (2, 4, 33, 256), (1, 32, 3, 512)])
def test_head_frame_vs_fp64(dev, B, T, N, d):
    from vlg import hip
    for t_read in sorted({0, T // 2, T - 1}):
        x, gamma, beta, w, b, rows = _head_case(B, T, N, d, 24, t_read, seed=B * 1000 + d + t_read)
        out = torch.full((B * N, 24), NAN, device=dev)
        dv = [t.to(dev) for t in (x, gamma, beta, w, b)]
        hip.call("vlg_head_frame", *[t.data_ptr() for t in dv], out.data_ptr(), B, T, N, d, 24, t_read, 1e-5, _stream())
        vs_cpu32(out, _head_ref(x, gamma, beta, w, b, rows, torch.float64), _head_ref(x, gamma, beta, w, b, rows, torch.float32),
                 "head on frame %d of (%d,%d,%d) d=%d" % (t_read, B, T, N, d))
        if t_read == T - 1:                                                # the last frame: vlg_head_last_frame, bit for bit
            last = torch.full((B * N, 24), NAN, device=dev)
            hip.call("vlg_head_last_frame", *[t.data_ptr() for t in dv], last.data_ptr(), B, T, N, d, 24, 1e-5, _stream())
            assert torch.equal(last, out)


def test_head_frame_refuses_t_read_outside_the_window(dev):
    from vlg import hip
    B, T, N, d = 2, 4, 3, 64
    x = torch.randn(B * N * T, d, device=dev)
    gamma, beta, w, b = torch.ones(d, device=dev), torch.zeros(d, device=dev), torch.randn(24, d, device=dev), torch.zeros(24, device=dev)
    out = torch.full((B * N, 24), NAN, device=dev)
    for t_read in (-1, T, T + 3):
        code = hip.load().vlg_head_frame(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr(), b.data_ptr(),
                                         out.data_ptr(), B, T, N, d, 24, t_read, 1e-5, _stream())
        torch.cuda.synchronize()
        assert code == ERR_SHAPE and bool(torch.isnan(out).all()), t_read


# -------------------------------------------------------------------------------------------- vlg_layout_decode_append
class Append:
    """buffers of one vlg_layout_decode_append call: the window holds real frames before `pos` and sentinels from it on"""

    def __init__(self, dev, out_last, cls, box, pos, steps):
        B, T, N = cls.shape
        self.shape, self.steps, self.pos = (B, T, N), steps, pos
        self.out_last = out_last.to(dev).contiguous()
        cls, box = cls.clone(), box.clone()
        cls[:, pos:] = -1
        box[:, pos:] = NAN
        self.cls0, self.box0 = cls, box
        self.cls, self.box = cls.to(dev).contiguous(), box.to(dev).contiguous()
        self.valid = torch.full((B, T, N), NAN, device=dev)
        self.gen_cls = torch.full((B, steps, N), -1, dtype=torch.int64, device=dev)
        self.gen_box = torch.full((B, steps, N, 4), NAN, device=dev)
        self.frame_cls = torch.full((B, N), -1, dtype=torch.int64, device=dev)
        self.frame_box = torch.full((B, N, 4), NAN, device=dev)

    def args(self, step, temperature=0.0, top_k=0, seed=0, keep_padded=0, n_classes=NC, **over):
        B, T, N = self.shape
        a = dict(out_last=self.out_last.data_ptr(), cls=self.cls.data_ptr(), box=self.box.data_ptr(), valid=self.valid.data_ptr(),
                 gen_cls=self.gen_cls.data_ptr(), gen_box=self.gen_box.data_ptr(), frame_cls=self.frame_cls.data_ptr(),
                 frame_box=self.frame_box.data_ptr(), B=B, T=T, N=N, n_classes=n_classes, pos=self.pos, steps=self.steps, step=step,
                 temperature=temperature, top_k=top_k, seed=seed, keep_padded=keep_padded)
        a.update(over)
        return list(a.values()) + [_stream()]

    def run(self, step, **kw):
        from vlg import hip
        hip.call("vlg_layout_decode_append", *self.args(step, **kw))
        return self.gen_cls[:, step].cpu()

    def untouched(self):
        torch.cuda.synchronize()
        same = lambda a, b: torch.equal(a.cpu().view(-1).view(torch.int32), b.view(-1).view(torch.int32))     # bitwise, NaN included
        return (same(self.cls, self.cls0) and same(self.box, self.box0) and bool(torch.isnan(self.valid).all())
                and bool((self.gen_cls == -1).all()) and bool(torch.isnan(self.gen_box).all())
                and bool((self.frame_cls == -1).all()) and bool(torch.isnan(self.frame_box).all()))

    def check_written(self, step, what):
        """frame pos = gen[:, step] = the compact copy; valid follows the class; everything else bitwise as it was"""
        B, T, N = self.shape
        pos, steps = self.pos, self.steps
        cls, box, valid = self.cls.cpu(), self.box.cpu(), self.valid.cpu()
        gc, gb = self.gen_cls.cpu(), self.gen_box.cpu()
        assert torch.equal(cls[:, pos], gc[:, step]) and torch.equal(box[:, pos], gb[:, step]), what
        assert torch.equal(self.frame_cls.cpu(), gc[:, step]) and torch.equal(self.frame_box.cpu(), gb[:, step]), what
        assert bool(torch.isfinite(gb[:, step]).all()) and bool((gc[:, step] >= 0).all()), what
        assert torch.equal(valid[:, pos], (cls[:, pos] < NC).float()), what
        others = [t for t in range(T) if t != pos]
        assert torch.equal(cls[:, others], self.cls0[:, others]), what
        assert torch.equal(box[:, others].view(torch.int32), self.box0[:, others].view(torch.int32)), what
        assert bool(torch.isnan(valid[:, others]).all()), what
        other = [i for i in range(steps) if i != step]
        assert bool((gc[:, other] == -1).all()) and bool(torch.isnan(gb[:, other]).all()), what


@pytest.mark.parametrize("pos", [1, 4, 7])
def test_append_argmax(dev, pos):
    B, T, N, steps, step = 3, 8, 5, 4, 2
    out_last = _rows(B * N, 1)
    out_last[4, 3] = out_last[4, 11] = 50.0                                # exact tie: the first maximum wins
    cls, box = _window(B, T, N, 2)                                         # holds the reserved id 20 here and there
    a = Append(dev, out_last, cls, box, pos, steps)
    got = a.run(step)
    wc, wb, _ = D.next_frame(out_last, cls[:, :pos], box[:, :pos], NC, step)
    assert int(wc[0, 4]) == 3 and torch.equal(got, wc)
    check_close(a.gen_box[:, step], wb, rtol=0, atol=1e-6, what="generated boxes")
    a.check_written(step, "argmax pos %d" % pos)
    # the sliding kernel on the same rows draws the same frame, bit for bit
    s = Step(dev, out_last, cls, box, steps)
    assert torch.equal(s.run(step), got) and torch.equal(s.gen_box[:, step].cpu(), a.gen_box[:, step].cpu())
    # valid may be NULL
    a2 = Append(dev, out_last, cls, box, pos, steps)
    assert torch.equal(a2.run(step, valid=0), got) and bool(torch.isnan(a2.valid).all())


@pytest.mark.parametrize("temperature", [1.0, 0.7, 2.5])
def test_append_sampling_matches_the_restatement(dev, temperature):
    B, N, T, steps, seed, pos = 3, 37, 4, 4, 0xC0FFEE12345, 2
    out_last = _rows(B * N, 3)
    out_last[5, 2] = out_last[5, 9] = out_last[5, 14] = 7.5                # equal logits at the top-k edge: lower index first
    cls, box = _window(B, T, N, 4, vocab=NC)
    for top_k in (0, 1, 5, 20):
        n_near = 0
        for step in range(steps):
            a, s = Append(dev, out_last, cls, box, pos, steps), Step(dev, out_last, cls, box, steps)
            got = a.run(step, temperature=temperature, top_k=top_k, seed=seed)
            want, _, near = D.next_frame(out_last, cls[:, :pos], box[:, :pos], NC, step, temperature, top_k, seed)
            assert torch.equal(got[~near], want[~near]), (top_k, step)
            assert bool(((got >= 0) & (got < NC)).all())
            n_near += int(near.sum())
            a.check_written(step, "sampling top_k %d step %d" % (top_k, step))
            # one device function: the sliding entry draws the same class for the same (out_last, step, seed), near or not
            assert torch.equal(s.run(step, temperature=temperature, top_k=top_k, seed=seed), got), (top_k, step)
            assert torch.equal(s.gen_box[:, step].cpu(), a.gen_box[:, step].cpu())
            if top_k != 1:
                other = Append(dev, out_last, cls, box, pos, steps).run(step, temperature=temperature, top_k=top_k, seed=seed + 1)
                assert not torch.equal(other, got)
        print("\ntemperature %g top_k %d: %d of %d draws within 1e-5 S of a boundary" % (temperature, top_k, n_near, steps * B * N))
        assert n_near <= 0.01 * steps * B * N


def test_append_keep_padded_looks_at_the_newest_frame(dev):
    B, T, N, steps, pos = 3, 8, 5, 2, 3
    out_last = _rows(B * N, 6)
    cls, box = _window(B, T, N, 7, vocab=NC)
    cls[0, pos - 1, 1] = cls[2, pos - 1, 4] = NC                           # padded in the newest frame
    cls[1, 0, 2] = cls[1, 1, 2] = NC                                       # padded in earlier frames only
    cls[1, pos:, 3] = NC                                                   # (frames the history has not reached: overwritten by sentinels)
    pad = cls[:, pos - 1] >= NC
    argmax = out_last[:, :NC].argmax(-1).view(B, N)
    on, off = Append(dev, out_last, cls, box, pos, steps), Append(dev, out_last, cls, box, pos, steps)
    got_on, got_off = on.run(1, keep_padded=1), off.run(1, keep_padded=0)
    assert torch.equal(got_off, argmax)
    assert torch.equal(got_on[~pad], argmax[~pad]) and bool((got_on[pad] == NC).all()) and int(pad.sum()) == 2
    gb = on.gen_box[:, 1].cpu()
    assert torch.equal(gb[pad], box[:, pos - 1][pad]) and torch.equal(gb[~pad], off.gen_box[:, 1].cpu()[~pad])
    on.check_written(1, "keep_padded on")
    off.check_written(1, "keep_padded off")
    assert torch.equal(on.valid[:, pos].cpu(), (~pad).float()) and bool((off.valid[:, pos] == 1).all())
    wc, wb, near = D.next_frame(out_last, cls[:, :pos], box[:, :pos], NC, 0, 1.3, 7, 11, keep_padded=True)
    got_s = Append(dev, out_last, cls, box, pos, steps).run(0, temperature=1.3, top_k=7, seed=11, keep_padded=1)
    assert torch.equal(got_s[~near], wc[~near]) and bool((got_s[pad] == NC).all()) and int(near.sum()) <= 1


def test_append_refusals_enqueue_nothing(dev):
    from vlg import hip
    B, T, N, steps, pos = 2, 4, 6, 3, 2
    cls, box = _window(B, T, N, 8)
    a = Append(dev, torch.zeros(B * N, 32), cls, box, pos, steps)          # (rows wide enough for any n_classes below)
    f = hip.load().vlg_layout_decode_append
    bad = [dict(temperature=-0.5), dict(temperature=float("inf")), dict(temperature=NAN), dict(top_k=-1), dict(top_k=NC + 1),
           dict(n_classes=0), dict(n_classes=29), dict(step=-1), dict(step=steps), dict(B=0), dict(T=0), dict(N=0),
           dict(pos=0), dict(pos=T), dict(pos=-1), dict(pos=T + 1),
           dict(frame_cls=0), dict(frame_box=0), dict(cls=0), dict(gen_box=0),
           dict(frame_cls=a.cls.data_ptr()), dict(frame_box=a.box.data_ptr() + 16), dict(gen_cls=a.cls.data_ptr() + 8 * N),
           dict(gen_box=a.frame_box.data_ptr())]
    for over in bad:
        step = over.pop("step", 1)
        assert f(*a.args(step, **over)) == ERR_SHAPE, over
        assert a.untouched(), over
    for over in (dict(box=a.box.data_ptr() + 4), dict(frame_box=a.frame_box.data_ptr() + 8), dict(cls=a.cls.data_ptr() + 4),
                 dict(valid=a.valid.data_ptr() + 2)):
        assert f(*a.args(1, **over)) == ERR_ALIGN, over
        assert a.untouched(), over
    assert f(*a.args(1)) == 0                                              # and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert not a.untouched()
    a.check_written(1, "accepted call")

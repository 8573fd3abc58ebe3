"""GPU: vlg_layout_mix_inputs through the C ABI against the CPU restatement of scheduled sampling (tests/sched_ref.py).
Every output buffer starts as -1 / NaN sentinels; the rows of `out` at t = T-1, which feed nothing, hold NaN."""
import pytest
import torch

import sched_ref as S
from helpers import vs_cpu32

pytestmark = pytest.mark.gpu

NC = S.NC
ERR_SHAPE, ERR_ALIGN = 1001, 1002
NAN = float("nan")
FULL = S.TWO24


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Mix:
    """buffers of one vlg_layout_mix_inputs call, outputs pre-filled with sentinels"""

    def __init__(self, dev, out, cls, box, counter=0):
        self.shape = tuple(cls.shape)
        B, T, N = self.shape
        self.ld = out.shape[1]
        self.out, self.cls, self.box = out.to(dev).contiguous(), cls.to(dev).contiguous(), box.to(dev).contiguous()
        self.mix_cls = torch.full((B, T, N), -1, dtype=torch.int64, device=dev)
        self.mix_box = torch.full((B, T, N, 4), NAN, device=dev)
        self.step = torch.full((1,), counter, dtype=torch.int32, device=dev)

    def args(self, thr_max=FULL, ramp_steps=0, temperature=0.0, top_k=0, seed=0, n_classes=NC, **over):
        B, T, N = self.shape
        a = dict(out=self.out.data_ptr(), ld=self.ld, cls=self.cls.data_ptr(), box=self.box.data_ptr(),
                 mix_cls=self.mix_cls.data_ptr(), mix_box=self.mix_box.data_ptr(), step=self.step.data_ptr(), B=B, T=T, N=N,
                 n_classes=n_classes, thr_max=thr_max, ramp_steps=ramp_steps, temperature=temperature, top_k=top_k, seed=seed)
        a.update(over)
        return list(a.values()) + [_stream()]

    def run(self, **kw):
        from vlg import hip
        hip.call("vlg_layout_mix_inputs", *self.args(**kw))
        return self.mix_cls.cpu(), self.mix_box.cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.mix_cls == -1).all()) and bool(torch.isnan(self.mix_box).all())


def _check(m, out, cls, box, k, thr_max=FULL, ramp_steps=0, temperature=0.0, top_k=0, seed=0, what=""):
    """one launch against the restatement: classes exact off the flagged draws, boxes of replaced tokens vs the fp64 sigmoid
    at helpers.vs_cpu32's bar, every other token bit-equal to the truth, inputs not modified -> (replaced, near)"""
    got_c, got_b = m.run(thr_max=thr_max, ramp_steps=ramp_steps, temperature=temperature, top_k=top_k, seed=seed)
    want_c, want_b, rep, near = S.mix_inputs(out, cls, box, NC, k, thr_max, ramp_steps, temperature, top_k, seed)
    assert torch.equal(got_c[~near], want_c[~near]), what
    assert bool(((got_c[rep] >= 0) & (got_c[rep] < NC)).all()), what
    assert torch.equal(got_c[~rep], cls[~rep]) and torch.equal(got_b[~rep], box[~rep]), what + ": untouched tokens"
    if bool(rep.any()):
        raw = out[:, NC:NC + 4]
        src32 = torch.sigmoid(raw.float())                              # torch-CPU fp32 yardstick, gathered like the fp64 value
        B, T, N = cls.shape
        b, t, n = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(N), indexing="ij")
        rows = ((b * N + n) * T + (t - 1))[rep]
        vs_cpu32(got_b[rep], want_b[rep], src32[rows], what + ": boxes of replaced tokens")
    assert torch.equal(m.cls.cpu(), cls) and torch.equal(m.box.cpu(), box)
    assert torch.equal(m.step.cpu(), torch.tensor([k], dtype=torch.int32))
    return rep, near


@pytest.mark.parametrize("B,T,N", S.SHAPES)
def test_argmax_mix_matches_the_restatement(dev, B, T, N):
    """eps_max = 1, temperature 0: every eligible token takes the first maximum of its source row and sigmoid(raw)"""
    out, cls, box = S.kernel_case(B, T, N, seed=B * 100 + N)            # holds the reserved id here and there
    if T > 1:
        cls[0, 1, 0] = 0                                                # (an eligible token whose source row holds
        out[0, 3] = out[0, 11] = 50.0                                   # an exact tie: the first maximum wins)
    m = Mix(dev, out, cls, box)
    rep, _ = _check(m, out, cls, box, 0, what="(%d,%d,%d)" % (B, T, N))
    assert torch.equal(rep, S.eligible(cls, NC))
    if T > 1:
        assert bool(rep[0, 1, 0]) and int(m.mix_cls[0, 1, 0]) == 3
    else:
        assert not bool(rep.any())                                      # pure copy
    # eps_max = 0: a copy of the truth, bit for bit
    z = Mix(dev, out, cls, box)
    c0, b0 = z.run(thr_max=0)
    assert torch.equal(c0, cls) and torch.equal(b0, box)


def test_wider_leading_dimension(dev):
    """ld = 32 > n_classes + 4: the columns past the row's 24 values hold NaN and are not read"""
    B, T, N = 2, 4, 33
    out, cls, box = S.kernel_case(B, T, N, seed=9, ld=32)
    narrow = out[:, :NC + 4].contiguous()
    a, b = Mix(dev, out, cls, box), Mix(dev, narrow, cls, box)
    _check(a, out, cls, box, 0, what="ld 32")
    ca, ba = a.mix_cls.cpu(), a.mix_box.cpu()
    cb, bb = b.run()
    assert torch.equal(ca, cb) and torch.equal(ba, bb)
    _check(Mix(dev, out, cls, box, counter=2), out, cls, box, 2, temperature=0.9, top_k=4, seed=5, what="ld 32 sampled")


@pytest.mark.parametrize("temperature,top_k", S.SAMPLING)
def test_sampled_mix_matches_the_restatement(dev, temperature, top_k):
    draws = flagged = 0
    for (B, T, N) in S.SAMPLING_SHAPES:
        out, cls, box = S.kernel_case(B, T, N, seed=B * 100 + N)
        for k in S.SAMPLING_STEPS:
            m = Mix(dev, out, cls, box, counter=k)
            rep, near = _check(m, out, cls, box, k, temperature=temperature, top_k=top_k, seed=S.CASE_SEED,
                               what="(%d,%d,%d) step %d" % (B, T, N, k))
            draws += int(rep.sum())
            flagged += int(near.sum())
    print("\ntemperature %g top_k %d: %d of %d draws within 1e-5 S of a boundary" % (temperature, top_k, flagged, draws))
    assert flagged < 0.01 * draws


def test_counter_and_ramp_are_read_on_the_device(dev):
    B, T, N = 2, 4, 33
    out, cls, box = S.kernel_case(B, T, N, seed=21)
    quarter = S.thr_max(0.25)
    reps = []
    for k in (0, 5):                                                    # the device counter chooses the coins
        rep, _ = _check(Mix(dev, out, cls, box, counter=k), out, cls, box, k, thr_max=quarter, seed=77, what="counter %d" % k)
        reps.append(rep)
    assert bool(reps[0].any()) and not torch.equal(reps[0], reps[1])
    other, _ = _check(Mix(dev, out, cls, box, counter=5), out, cls, box, 5, thr_max=quarter, seed=78, what="another seed")
    assert not torch.equal(other, reps[1])
    # the ramp: thr(k) = thr_max * min(k + 1, ramp) // ramp, computed in the kernel from the counter
    counts = []
    for k in (0, 3, 7, 8, 40):
        rep, _ = _check(Mix(dev, out, cls, box, counter=k), out, cls, box, k, thr_max=FULL, ramp_steps=8, seed=77,
                        what="ramp at step %d" % k)
        counts.append(int(rep.sum()))
    n = int(S.eligible(cls, NC).sum())
    assert 0 < counts[0] < counts[1] < counts[2] == counts[3] == counts[4] == n
    # sampling reads the same counter for its draws
    a, _ = Mix(dev, out, cls, box, counter=0).run(temperature=1.0, seed=3)
    b, _ = Mix(dev, out, cls, box, counter=5).run(temperature=1.0, seed=3)
    assert not torch.equal(a, b)


def test_refusals_enqueue_nothing(dev):
    from vlg import hip
    B, T, N = 2, 4, 6
    _, cls, box = S.kernel_case(B, T, N, seed=8)
    m = Mix(dev, torch.zeros(B * N * T, 32), cls, box)                  # (rows wide enough for any n_classes below)
    f = hip.load().vlg_layout_mix_inputs
    shape = [dict(temperature=-0.5), dict(temperature=float("inf")), dict(temperature=NAN), dict(top_k=-1), dict(top_k=NC + 1),
             dict(n_classes=0), dict(n_classes=29), dict(ld=NC + 3), dict(thr_max=FULL + 1), dict(ramp_steps=-1),
             dict(B=0), dict(T=0), dict(N=0), dict(step=0), dict(out=0),
             dict(mix_cls=m.cls.data_ptr()), dict(mix_box=m.box.data_ptr()),                       # in == out
             dict(mix_cls=m.cls.data_ptr() + 8 * N), dict(mix_box=m.out.data_ptr() + 16),          # partial overlap
             dict(mix_cls=m.mix_box.data_ptr())]                                                   # the two outputs
    for over in shape:
        assert f(*m.args(**over)) == ERR_SHAPE, over
        assert m.untouched(), over
    for over in (dict(mix_box=m.mix_box.data_ptr() + 4), dict(mix_cls=m.mix_cls.data_ptr() + 4), dict(out=m.out.data_ptr() + 4),
                 dict(box=m.box.data_ptr() + 8), dict(cls=m.cls.data_ptr() + 4)):
        assert f(*m.args(**over)) == ERR_ALIGN, over
        assert m.untouched(), over
    assert torch.equal(m.cls.cpu(), cls) and torch.equal(m.box.cpu(), box)
    assert f(*m.args()) == 0                                              # and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert not m.untouched()

"""CPU: the specification of attention = "factored" (tests/factored_ref.py, composed from the pinned oracle) has the
properties the mode is built for, and LayoutConfig takes the mode.  fp64 unless said otherwise."""
import pytest
import torch

import factored_ref as R
from oracle import layout_spec as O
from vlg.spec import LayoutConfig, param_shapes, step_flops

NC = 20


def _model(B, T, N, d, n_layers, seed, dtype=torch.float64):
    cfg = LayoutConfig(B=B, T=T, N=N, d=d, n_layers=n_layers, attention="factored")
    p = {k: v.to(dtype) for k, v in O.init_params(param_shapes(cfg), seed=seed).items()}
    g = torch.Generator().manual_seed(seed + 1)
    cls = torch.randint(0, NC, (B, T, N), generator=g)
    box = torch.rand(B, T, N, 4, generator=g, dtype=torch.float64).to(dtype)
    return cfg, p, cls, box


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_one_layer_is_the_slot_mode(dtype):
    cfg, p, cls, box = _model(2, 4, 8, 64, 1, seed=3, dtype=dtype)
    with torch.no_grad():
        a = R.forward(p, cls, box, 1, valid=torch.ones(cls.shape))
        b = O.forward(p, cls, box, 1, attention="slot")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    batch = O.synthetic_batch(2, 4, 8, seed=5)
    pa, ga = R.loss_and_grads(p, batch, 1)
    if dtype == torch.float32:
        pb, gb = O.loss_and_grads(p, batch, 1)
        assert pa == pb and all(torch.equal(ga[k], gb[k]) for k in ga)


def test_later_frames_cannot_reach_an_earlier_position():
    cfg, p, cls, box = _model(2, 4, 8, 64, 2, seed=5)
    t = 2
    other_c, other_b = cls.clone(), box.clone()
    other_c[:, t + 1:] = (cls[:, t + 1:] + 7) % NC
    other_b[:, t + 1:] = 1.0 - box[:, t + 1:]
    with torch.no_grad():
        a = R.forward(p, cls, box, 2)
        b = R.forward(p, other_c, other_b, 2)
    for x, y in zip(a, b):
        assert float((x[:, :t + 1] - y[:, :t + 1]).abs().max()) == 0.0
        assert float((x[:, t + 1:] - y[:, t + 1:]).abs().max()) > 1e-3


@pytest.mark.parametrize("h", [1, 3, 7])
def test_grow_rule_the_history_alone_is_the_padded_window(h):
    """as test_rollout_grow_cpu.py has it for the other modes: position h-1 of the h real frames alone is position h-1 of the
    window padded with the reserved class id and zero boxes (bar 1e-12 of the output scale)"""
    cfg, p, cls, box = _model(2, 8, 4, 64, 3, seed=11 + h)
    cls[0, 0, 2] = cls[1, :, 3] = NC
    pad_c, pad_b = cls.clone(), box.clone()
    pad_c[:, h:] = NC
    pad_b[:, h:] = 0.0
    with torch.no_grad():
        wl, wr = R.forward(p, cls[:, :h], box[:, :h], 3, valid=(cls[:, :h] < NC).double())
        gl, gr = R.forward(p, pad_c, pad_b, 3, valid=(pad_c < NC).double())
    assert bool(torch.isfinite(gl).all()) and bool(torch.isfinite(gr).all())
    scale = float(wl.abs().max())
    for t in range(h):
        assert float((gl[:, t] - wl[:, t]).abs().max()) <= 1e-12 * scale
        assert float((gr[:, t] - wr[:, t]).abs().max()) <= 1e-12 * scale


def test_slots_of_a_frame_see_each_other_here_and_not_in_the_slot_mode():
    cfg, p, cls, box = _model(2, 4, 8, 64, 2, seed=9)
    t, n = 1, 0
    c2, b2 = cls.clone(), box.clone()
    c2[:, t, n] = (cls[:, t, n] + 3) % NC
    b2[:, t, n] = 1.0 - box[:, t, n]
    with torch.no_grad():
        fa, fb = R.forward(p, cls, box, 2)[0], R.forward(p, c2, b2, 2)[0]
        sa, sb = O.forward(p, cls, box, 2)[0], O.forward(p, c2, b2, 2)[0]
    others = [m for m in range(8) if m != n]
    assert float((sa[:, :, others] - sb[:, :, others]).abs().max()) == 0.0
    assert float((fa[:, :t, others] - fb[:, :t, others]).abs().max()) == 0.0       # nothing reaches earlier frames
    for tt in range(t, 4):                                                          # ... and every later frame is reached
        assert float((fa[:, tt, others] - fb[:, tt, others]).abs().max()) > 1e-4, tt


def test_a_padded_slot_reaches_no_other_token_and_an_all_padded_frame_returns_v():
    g = torch.Generator().manual_seed(2)
    B, T, N, d = 2, 4, 8, 128
    qkv = torch.randn(B, T, N, 3 * d, generator=g, dtype=torch.float64)
    valid = (torch.rand(B, T, N, generator=g) > 0.3).double()
    valid[1, 2] = 0.0                                           # a frame whose slots are all padded
    pad = valid == 0
    base = R.frame_attention(qkv, 2, valid)
    q2 = qkv.clone()
    q2[pad] = torch.randn(int(pad.sum()), 3 * d, generator=g, dtype=torch.float64) * 3.0
    got = R.frame_attention(q2, 2, valid)
    assert torch.equal(got[~pad], base[~pad])
    assert torch.equal(base[1, 2], qkv[1, 2, :, 2 * d:])
    # against a direct statement of the rule
    s = torch.einsum("btnhe,btmhe->bthnm", qkv[..., :d].reshape(B, T, N, 2, 64), qkv[..., d:2 * d].reshape(B, T, N, 2, 64)) / 8.0
    ok = (valid[:, :, None, None, :] > 0) | torch.eye(N, dtype=torch.bool)
    a = torch.softmax(s.masked_fill(~ok, float("-inf")), dim=-1)
    want = torch.einsum("bthnm,btmhe->btnhe", a, qkv[..., 2 * d:].reshape(B, T, N, 2, 64)).reshape(B, T, N, d)
    assert float((base - want).abs().max()) <= 1e-12


def test_config_takes_the_mode_and_refuses_bad_shapes():
    cfg = LayoutConfig(B=2, T=4, N=8, d=64, n_layers=3, attention="factored")
    cfg.validate()
    assert [cfg.frame_layer(l) for l in range(3)] == [False, True, False] and cfg.n_frame_layers == 1
    assert "factored" in cfg.describe()["attention"]
    LayoutConfig(B=1, T=4, N=8, d=64, n_layers=1, attention="factored").validate()          # one layer: allowed, = "slot"
    assert not LayoutConfig(attention="slot").frame_layer(1) and not LayoutConfig(attention="clip").frame_layer(1)
    with pytest.raises(ValueError, match="multiple of 32"):
        LayoutConfig(B=1, T=4, N=5, d=64, attention="factored").validate()
    with pytest.raises(ValueError, match="T must be"):
        LayoutConfig(B=1, T=64, N=8, d=64, attention="factored").validate()
    with pytest.raises(ValueError, match="factored"):
        LayoutConfig(attention="frame").validate()
    # same parameters and layout in every mode: a checkpoint moves between them
    shapes = [list(param_shapes(LayoutConfig(B=2, T=4, N=8, d=64, n_layers=2, attention=a)).items()) for a in ("slot", "clip", "factored")]
    assert shapes[0] == shapes[1] == shapes[2]
    # the FLOP count lies between the other two
    f = {a: step_flops(LayoutConfig(attention=a))["fwd_bwd"] for a in ("slot", "clip", "factored")}
    assert f["slot"] < f["factored"] < f["clip"]

"""GPU: vlg_layout_metrics launch by launch against the fp64 restatement (tests/metrics_ref.py), then through
LayoutEngine.accumulate_metrics / evaluate_rollout and the Trainer.

Inputs are built on the CPU from a seeded generator so that both outcomes of every counter are common: raw boxes are
logit(target) + 0.3 randn on half the tokens and 2 randn on the rest, logits are 3 randn with +4 on the target class for
half the tokens (random inputs alone give 5 % accuracy and IoU >= 0.5 on 0.4 % of the tokens).  Record buffers start from
non-zero sentinels: the kernel must ADD.  One scratch buffer, zeroed once, serves every launch of the module, so each test
also checks that the launch before it left the ticket at zero.

Bars.  Integer slots are exact, except IOU_HIT / BOTH_HIT, which may differ by the number of tokens whose fp64 IoU lies
within 1e-5 of the threshold (fp32 and fp64 IoU differ by < 1e-6); that band must hold under 1 % of the scored tokens.
Per-token values are fp32, accumulated in double: each sum / SCORED within 1e-5 of the reference, NLL 1e-5 + 1e-5 |ref|."""
import functools

import pytest
import torch

import metrics_ref as R
from helpers import reference_args

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
IOU_EPS = 1e-7
ERR_SHAPE, ERR_ALIGN = 1001, 1002
GRID_STRIDE = (9, 32, 128)          # 36 864 tokens > 128 tokens per pass x 256 blocks: the grid-stride loop runs a second pass


def _stream():
    return torch.cuda.current_stream().cuda_stream


_SCRATCH = {}


def _scratch(dev):
    from vlg import hip
    if dev not in _SCRATCH:
        _SCRATCH[dev] = torch.zeros(hip.load().vlg_layout_metrics_scratch(), dtype=torch.float64, device=dev)
    return _SCRATCH[dev]


@functools.lru_cache(maxsize=None)
def _case(B, T, N, C, ld, masked, tgt_T=None, t0=0, seed=0):
    """public-order inputs: out (B,T,N,ld) with NaN in the padding columns, targets over tgt_T frames"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * T + N + C + ld)
    tgt_T = tgt_T or T
    tgt_class = torch.randint(0, C + 1, (B, tgt_T, N), generator=g)                  # C = the reserved id: about 1 in C + 1 unscored
    cxy = 0.2 + 0.6 * torch.rand(B, tgt_T, N, 2, generator=g)
    wh = 0.1 + 0.4 * torch.rand(B, tgt_T, N, 2, generator=g)
    tgt_box = torch.cat([cxy, wh], -1).contiguous()
    valid = (torch.rand(B, tgt_T, N, generator=g) > 0.3).float() if masked else None
    tb, tc = tgt_box[:, t0:t0 + T], tgt_class[:, t0:t0 + T]
    near = torch.rand(B, T, N, 1, generator=g) < 0.5
    raw = torch.where(near, torch.logit(tb) + 0.3 * torch.randn(B, T, N, 4, generator=g), 2 * torch.randn(B, T, N, 4, generator=g))
    logits = 3 * torch.randn(B, T, N, C, generator=g)
    boost = (torch.rand(B, T, N, generator=g) < 0.5) & (tc < C)
    logits[boost] += 4 * torch.nn.functional.one_hot(tc[boost], C)
    out = torch.full((B, T, N, ld), NAN)
    out[..., :C], out[..., C:C + 4] = logits, raw
    return dict(out=out, tgt_class=tgt_class, tgt_box=tgt_box, valid=valid, C=C, ld=ld, t0=t0)


def _ref(case, top_k, iou_thr=0.5):
    C = case["C"]
    return R.metrics_ref(case["out"][..., :C], case["out"][..., C:C + 4], case["tgt_class"], case["tgt_box"], case["valid"],
                         top_k, iou_thr, IOU_EPS, t0=case["t0"])


class Record:
    """a `rows`-row record on the device, filled with non-zero sentinels"""

    def __init__(self, dev, C, rows=1):
        nc, ns = R.CONF + C * C, R.IOU_BY_CLASS + C
        self.counts0 = (1000 + 7 * torch.arange(rows * nc)).view(rows, nc)
        self.sums0 = (0.5 + 0.25 * torch.arange(rows * ns, dtype=torch.float64)).view(rows, ns)
        self.counts, self.sums = self.counts0.to(dev), self.sums0.to(dev)

    def added(self, row=0):
        return self.counts[row].cpu() - self.counts0[row], self.sums[row].cpu() - self.sums0[row]

    def untouched(self, rows):
        return all(torch.equal(self.counts[r].cpu(), self.counts0[r]) and torch.equal(self.sums[r].cpu(), self.sums0[r]) for r in rows)


def _device_inputs(dev, case, b0=0, b1=None):
    """clips b0 .. b1 of a case on the device: out in the INTERNAL row order m = (b*N + n)*T + t, targets in the public one"""
    sl = slice(b0, b1)
    out = case["out"][sl]
    B, T, N, ld = out.shape
    d = dict(out=out.permute(0, 2, 1, 3).contiguous().view(B * N * T, ld).to(dev), tgt_class=case["tgt_class"][sl].contiguous().to(dev),
             tgt_box=case["tgt_box"][sl].contiguous().to(dev), valid=None if case["valid"] is None else case["valid"][sl].contiguous().to(dev))
    return d, (B, T, N)


def _args(d, shape, case, rec, row, k, thr, dev, **over):
    B, T, N = shape
    a = dict(out=d["out"].data_ptr(), ld=case["ld"], tgt_class=d["tgt_class"].data_ptr(), tgt_box=d["tgt_box"].data_ptr(),
             valid=0 if d["valid"] is None else d["valid"].data_ptr(), tgt_T=d["tgt_class"].shape[1], t0=case["t0"],
             counts=rec.counts[row].data_ptr(), sums=rec.sums[row].data_ptr(), scratch=_scratch(dev).data_ptr(),
             B=B, T=T, N=N, n_classes=case["C"], top_k=k, iou_thr=thr, iou_eps=IOU_EPS)
    a.update(over)
    return list(a.values()) + [_stream()]


def _launch(dev, case, rec, top_k, row=0, iou_thr=0.5, b0=0, b1=None):
    from vlg import hip
    d, shape = _device_inputs(dev, case, b0, b1)
    hip.call("vlg_layout_metrics", *_args(d, shape, case, rec, row, top_k, iou_thr, dev))
    torch.cuda.synchronize()


def _check(got_counts, got_sums, ref, what, iou_thr=0.5, tokens=None):
    """the module docstring's bars; prints every figure before it asserts"""
    want_counts, want_sums, iou = ref
    scored = int(want_counts[R.SCORED])
    band = int(((iou - iou_thr).abs() <= 1e-5).sum())
    print("\n%s: scored %d, counts got %s want %s, band %d" % (what, scored, got_counts[:7].tolist(), want_counts[:7].tolist(), band))
    assert band <= 0.01 * scored, "%s: %d of %d tokens within 1e-5 of the IoU threshold" % (what, band, scored)
    for k, name in enumerate(R.COUNT_NAMES):
        slack = band if k in (R.IOU_HIT, R.BOTH_HIT) else 0
        assert abs(int(got_counts[k]) - int(want_counts[k])) <= slack, "%s: %s %d, reference %d (+-%d)" % (
            what, name, int(got_counts[k]), int(want_counts[k]), slack)
    assert int(got_counts[7]) == 0
    assert torch.equal(got_counts[R.CONF:], want_counts[R.CONF:]), what + ": confusion matrix"
    if tokens is not None:
        assert int(got_counts[R.SCORED] + got_counts[R.NONFINITE] + got_counts[R.UNSCORED]) == tokens
    assert bool(torch.isfinite(got_sums).all()), what + ": sums not finite"
    n = max(scored, 1)
    err = ((got_sums - want_sums) / n).abs()
    print("  sums / scored: got %s\n  |err| %s" % ((got_sums[:3] / n).tolist(), err.tolist()))
    assert float(err[R.NLL]) <= 1e-5 + 1e-5 * abs(float(want_sums[R.NLL]) / n), "%s: NLL off by %.3e per token" % (what, float(err[R.NLL]))
    assert float(err[1:].max()) <= 1e-5, "%s: a sum is off by %.3e per scored token" % (what, float(err[1:].max()))


# ------------------------------------------------------------------------------------------------ 1. launch vs fp64
LAUNCHES = [  # (B,T,N), ld, masked, C, top_k, (tgt_T, t0)
    ((1, 1, 1), 24, False, 20, 1, None), ((1, 4, 3), 24, True, 20, 5, None), ((1, 4, 3), 8, False, 1, 1, None),
    ((2, 8, 8), 28, True, 20, 20, None), ((2, 8, 8), 24, False, 7, 5, None),
    ((3, 4, 11), 24, False, 20, 5, None), ((3, 4, 11), 28, True, 7, 1, None), ((3, 4, 11), 32, True, 28, 5, None),
    ((5, 16, 13), 24, True, 7, 7, None), ((5, 16, 13), 28, False, 20, 1, None),
    ((7, 1, 9), 24, True, 20, 5, (5, 3)), ((7, 1, 9), 24, False, 7, 5, (5, 3)), ((7, 1, 9), 28, False, 20, 20, (5, 3)),
    (GRID_STRIDE, 24, True, 20, 5, None), (GRID_STRIDE, 28, False, 7, 7, None),
]


@pytest.mark.parametrize("shape,ld,masked,C,top_k,frames", LAUNCHES)
def test_launch_vs_fp64(dev, shape, ld, masked, C, top_k, frames):
    B, T, N = shape
    tgt_T, t0 = frames or (T, 0)
    case = _case(B, T, N, C, ld, masked, tgt_T, t0)
    rec = Record(dev, C)
    _launch(dev, case, rec, top_k)
    _check(*rec.added(), _ref(case, top_k), "(%d,%d,%d) ld %d C %d top_k %d" % (B, T, N, ld, C, top_k), tokens=B * T * N)


def test_both_outcomes_of_every_counter_are_common():
    """the inputs do what the module docstring says (checked on the reference alone)"""
    counts = _ref(_case(5, 16, 13, 20, 24, True), 5)[0]
    scored = int(counts[R.SCORED])
    for k in (R.TOP1, R.TOPK, R.IOU_HIT, R.BOTH_HIT):
        assert 0.03 * scored < int(counts[k]) < 0.97 * scored, R.COUNT_NAMES[k]      # (BOTH_HIT, the rarest: about 1 in 18)
    assert int(counts[R.UNSCORED]) > 0.2 * 5 * 16 * 13


# ------------------------------------------------------------------------------------------------ 2. accumulation
def test_two_halves_equal_the_whole(dev):
    case = _case(4, 16, 13, 20, 24, True)
    whole, halves = Record(dev, 20), Record(dev, 20)
    _launch(dev, case, whole, 5)
    _launch(dev, case, halves, 5, b0=0, b1=2)
    _launch(dev, case, halves, 5, b0=2, b1=4)
    (wc, ws), (hc, hs) = whole.added(), halves.added()
    assert torch.equal(wc, hc)
    assert bool(((ws - hs).abs() <= 1e-12 * ws.abs() + 1e-12).all()), (ws - hs).abs().max()
    _check(hc, hs, _ref(case, 5), "two halves", tokens=4 * 16 * 13)


def test_a_row_of_a_record_leaves_the_others_alone(dev):
    case = _case(3, 4, 11, 20, 24, True)
    rec = Record(dev, 20, rows=3)
    _launch(dev, case, rec, 5, row=1)
    assert rec.untouched((0, 2))
    _check(*rec.added(1), _ref(case, 5), "row 1 of 3", tokens=3 * 4 * 11)


# ------------------------------------------------------------------------------------------------ 3. reproducibility
@pytest.mark.parametrize("shape", [(5, 16, 13), GRID_STRIDE])
def test_same_launch_same_bits(dev, shape):
    case = _case(*shape, 20, 24, True)
    a, b = Record(dev, 20), Record(dev, 20)
    _launch(dev, case, a, 5)
    _launch(dev, case, b, 5)
    assert torch.equal(a.counts.cpu(), b.counts.cpu()) and torch.equal(a.sums.cpu(), b.sums.cpu())
    assert not a.untouched((0,))


# ------------------------------------------------------------------------------------------------ 4. ties
@pytest.mark.parametrize("top_k", [1, 2])
def test_ties(dev, top_k):
    """integer-valued logits: repeated maxima and repeated target values in most rows"""
    B, T, N, C = 3, 4, 11, 7
    case = dict(_case(B, T, N, C, 24, False))
    out = case["out"].clone()
    out[..., :C] = torch.randint(0, 3, (B, T, N, C), generator=torch.Generator().manual_seed(5)).float()
    case["out"] = out
    l = out[..., :C]
    assert float(((l == l.max(-1, keepdim=True).values).sum(-1) > 1).float().mean()) > 0.5
    rec = Record(dev, C)
    _launch(dev, case, rec, top_k)
    ref = _ref(case, top_k)
    _check(*rec.added(), ref, "ties, top_k %d" % top_k, tokens=B * T * N)
    if top_k == 1:
        assert int(ref[0][R.TOPK]) == int(ref[0][R.TOP1])                           # rank 0 is the first maximum


# ------------------------------------------------------------------------------------------------ 5. non-finite, unscored
def test_nonfinite_and_unscored(dev):
    B, T, N, C = 5, 16, 13, 20
    base = _case(B, T, N, C, 24, True)
    want = Record(dev, C)
    _launch(dev, base, want, 5)
    ok = (base["tgt_class"] < C) & (base["valid"] != 0)
    # NaN / inf in the outputs of UNSCORED tokens change nothing, bit for bit
    case = dict(base, out=base["out"].clone())
    fill = torch.tensor([NAN, INF, -INF]).repeat(8)
    case["out"][~ok] = fill
    rec = Record(dev, C)
    _launch(dev, case, rec, 5)
    assert torch.equal(rec.counts.cpu(), want.counts.cpu()) and torch.equal(rec.sums.cpu(), want.sums.cpu())
    # in SCORED tokens they move exactly those tokens to NONFINITE (a logit, the target's logit, a raw box value; NaN, inf, -inf)
    pos = ok.nonzero()[torch.randperm(int(ok.sum()), generator=torch.Generator().manual_seed(3))[:40]]
    for i, (b, t, n) in enumerate(pos.tolist()):
        col = (int(base["tgt_class"][b, t, n]), (i * 7) % C, C + i % 4)[i % 3]
        case["out"][b, t, n, col] = (NAN, INF, -INF)[(i // 3) % 3]
    rec2 = Record(dev, C)
    _launch(dev, case, rec2, 5)
    got_c, got_s = rec2.added()
    ref = _ref(case, 5)
    assert int(ref[0][R.NONFINITE]) == 40 and int(got_c[R.NONFINITE]) == 40
    assert int(got_c[R.SCORED]) == int(want.added()[0][R.SCORED]) - 40 and int(got_c[R.UNSCORED]) == int((~ok).sum())
    _check(got_c, got_s, ref, "40 non-finite tokens", tokens=B * T * N)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_on_the_device(dev):
    from vlg import hip
    f = hip.load().vlg_layout_metrics
    case = _case(3, 4, 11, 20, 24, True)
    d, shape = _device_inputs(dev, case)
    rec = Record(dev, 20)
    shape_bad = [dict(top_k=0), dict(top_k=21), dict(n_classes=29), dict(n_classes=0), dict(t0=1), dict(t0=-1), dict(tgt_T=3),
                 dict(ld=22), dict(ld=20), dict(B=0), dict(T=0), dict(N=0), dict(iou_thr=INF), dict(iou_thr=NAN)]
    align_bad = [dict(out=d["out"].data_ptr() + 4), dict(out=0), dict(tgt_box=d["tgt_box"].data_ptr() + 8), dict(tgt_box=0),
                 dict(scratch=_scratch(dev).data_ptr() + 8), dict(scratch=0), dict(sums=rec.sums.data_ptr() + 4), dict(sums=0),
                 dict(tgt_class=d["tgt_class"].data_ptr() + 4), dict(tgt_class=0), dict(counts=rec.counts.data_ptr() + 4),
                 dict(counts=0), dict(valid=d["valid"].data_ptr() + 2)]
    for want, overs in ((ERR_SHAPE, shape_bad), (ERR_ALIGN, align_bad)):
        for over in overs:
            assert f(*_args(d, shape, case, rec, 0, 5, 0.5, dev, **over)) == want, over
    torch.cuda.synchronize()
    assert rec.untouched((0,)) and not bool(_scratch(dev)[:2].any())
    # the same buffers are accepted as they are, and the result is right: the ticket was left at zero
    assert f(*_args(d, shape, case, rec, 0, 5, 0.5, dev)) == 0
    torch.cuda.synchronize()
    _check(*rec.added(), _ref(case, 5), "after the refusals", tokens=3 * 4 * 11)


# ------------------------------------------------------------------------------------------------ 7. engine
def _engine_batch(cfg, seed, all_valid):
    g = torch.Generator().manual_seed(seed)
    B, T, N, C = cfg.B, cfg.T, cfg.N, cfg.n_classes
    cls = torch.randint(0, C, (B, T + 1, N), generator=g)
    box = torch.cat([0.2 + 0.6 * torch.rand(B, T + 1, N, 2, generator=g), 0.1 + 0.4 * torch.rand(B, T + 1, N, 2, generator=g)], -1)
    valid = torch.ones(B, T, N) if all_valid else (torch.rand(B, T, N, generator=g) > 0.3).float()
    return {"slot_class": cls[:, :T].contiguous(), "slot_box": box[:, :T].contiguous(), "tgt_class": cls[:, 1:].contiguous(),
            "tgt_box": box[:, 1:].contiguous(), "valid": valid}


@pytest.mark.parametrize("attention", ["slot", "clip"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_engine_accumulate_metrics(dev, precision, attention):
    from vlg import metrics as M
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    cfg = LayoutConfig(B=2, T=4, N=8, d=64, n_layers=1, attention=attention)
    eng = LayoutEngine(cfg, dev, seed=11, precision=precision)
    rec = eng.metrics_record(rows=2)
    assert isinstance(rec, M.MetricsRecord) and rec.counts.is_cuda and rec.counts.shape == (2, 408) and rec.sums.shape == (2, 24)
    # a masked batch vs the restatement on the engine's own outputs
    batch = _engine_batch(cfg, 1, all_valid=False)
    eng.forward({k: v.to(dev) for k, v in batch.items()})
    eng.accumulate_metrics({k: v.to(dev) for k, v in batch.items()}, rec, row=1, top_k=3, iou_thr=0.3)
    logits, raw = (t.cpu().contiguous() for t in eng.outputs_btn())
    ref = R.metrics_ref(logits, raw, batch["tgt_class"], batch["tgt_box"], batch["valid"], 3, 0.3, IOU_EPS)
    _check(rec.counts[1].cpu(), rec.sums[1].cpu(), ref, "engine %s %s" % (precision, attention), iou_thr=0.3, tokens=cfg.tokens)
    assert not bool(rec.counts[0].any()) and not bool(rec.sums[0].any())
    # all-ones valid: the record's means are the loss kernel's cross-entropy and 1 - IoU terms
    ones = {k: v.to(dev) for k, v in _engine_batch(cfg, 2, all_valid=True).items()}
    loss = eng.forward(ones).cpu().double()
    eng.accumulate_metrics(ones, rec, row=0)
    s = rec.summary()[0]
    assert s["scored"] == cfg.tokens and s["unscored"] == 0 and s["nonfinite"] == 0
    print("\nnll %.8f vs loss ce %.8f; 1 - mean_iou %.8f vs loss iou %.8f" % (s["nll"], loss[3], 1 - s["mean_iou"], loss[2]))
    assert abs(s["nll"] - float(loss[3])) <= 1e-5 * abs(float(loss[3]))
    assert abs((1 - s["mean_iou"]) - float(loss[2])) <= 1e-5 * abs(float(loss[2]))
    with pytest.raises(ValueError):
        eng.accumulate_metrics(ones, M.MetricsRecord(20))                            # a CPU record
    with pytest.raises(ValueError):
        eng.accumulate_metrics(ones, rec, row=2)


# ------------------------------------------------------------------------------------------------ 8. rollout
@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_engine_evaluate_rollout(dev, temperature):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    cfg = LayoutConfig(B=2, T=4, N=8, d=64, n_layers=1, attention="clip")
    eng = LayoutEngine(cfg, dev, seed=11)
    B, T, N, C, S = cfg.B, cfg.T, cfg.N, cfg.n_classes, 3
    g = torch.Generator().manual_seed(9)
    clip_class = torch.randint(0, C, (B, T + S, N), generator=g)
    clip_class[1, T + 1, 5] = C                                                      # one padded truth slot: unscored at step 1
    clip_box = torch.cat([0.2 + 0.6 * torch.rand(B, T + S, N, 2, generator=g), 0.1 + 0.4 * torch.rand(B, T + S, N, 2, generator=g)], -1)
    knobs = dict(temperature=temperature, seed=1234)
    rec, gen_c, gen_b, logits = eng.evaluate_rollout(clip_class.to(dev), clip_box.to(dev), top_k=5, iou_thr=0.3,
                                                     return_logits=True, sample_top_k=6, **knobs)
    assert rec.rows == S and tuple(logits.shape) == (S, B * N, cfg.n_out)
    want_c, want_b = eng.rollout(clip_class[:, :T].to(dev), clip_box[:, :T].to(dev), steps=S, top_k=6, **knobs)
    assert torch.equal(gen_c, want_c) and torch.equal(gen_b, want_b)
    counts, sums = rec.counts.cpu(), rec.sums.cpu()
    for i in range(S):
        o = logits[i].cpu().view(B, 1, N, cfg.n_out)
        ref = R.metrics_ref(o[..., :C].contiguous(), o[..., C:].contiguous(), clip_class, clip_box, None, 5, 0.3, IOU_EPS, t0=T + i)
        _check(counts[i], sums[i], ref, "rollout step %d, temperature %g" % (i, temperature), iou_thr=0.3, tokens=B * N)
        assert int(counts[i][R.UNSCORED]) == (1 if i == 1 else 0)
    # a given record is added to; without return_logits the record alone comes back
    again = eng.evaluate_rollout(clip_class.to(dev), clip_box.to(dev), record=rec, top_k=5, iou_thr=0.3, sample_top_k=6, **knobs)
    assert again is rec and torch.equal(rec.counts.cpu(), 2 * counts)
    with pytest.raises(ValueError):
        eng.evaluate_rollout(clip_class[:, :T].to(dev), clip_box[:, :T].to(dev))     # no frame to score


# ------------------------------------------------------------------------------------------------ 9. trainer
LAYOUT_CFG = dict(batch_size=2, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1, train_clips=4, val_clips=6)
SUMMARY_KEYS = {"scored", "nonfinite", "unscored", "accuracy", "topk_accuracy", "nll", "perplexity", "mean_iou", "iou_hit",
                "both_hit", "box_l1", "per_class_accuracy", "per_class_iou", "macro_accuracy", "macro_iou", "confusion"}


def test_trainer_validate_and_evaluate_rollout(tmp_path, monkeypatch, dev):
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    for k in ("VLG_MODEL", "VLG_VARIABLE_N", "VLG_VAL_METRICS", "VLG_VAL_TOPK", "VLG_VAL_IOU_THR", "VLG_GEN_TEMPERATURE",
              "VLG_GEN_TOP_K", "VLG_GEN_SEED", "VLG_GEN_KEEP_PADDED", "VLG_ATTENTION", "VLG_PRECISION"):
        monkeypatch.delenv(k, raising=False)
    from trainer import Trainer
    tr = Trainer(reference_args(tmp_path / "exp", **LAYOUT_CFG))
    tr.set_epoch(0)
    off = tr.validate()
    assert list(off) == ["loss"]
    monkeypatch.setenv("VLG_VAL_METRICS", "1")
    tr.set_epoch(0)
    on = tr.validate()
    assert set(on) == SUMMARY_KEYS | {"loss"} and on["loss"] == off["loss"]
    assert on["scored"] == 6 * 4 * 8 and on["unscored"] == 0 and on["nonfinite"] == 0
    assert 0.0 <= on["accuracy"] <= on["topk_accuracy"] <= 1.0 and 0.0 <= on["mean_iou"] <= 1.0 and on["nll"] > 0
    assert sum(sum(r) for r in on["confusion"]) == on["scored"]
    scalars = open(tmp_path / "exp" / "scalars.tsv").read() if (tmp_path / "exp" / "scalars.tsv").exists() else None
    if scalars is not None:
        assert all("val/" + k in scalars for k in ("accuracy", "mean_iou", "nll", "iou_hit"))
    monkeypatch.delenv("VLG_VAL_METRICS")
    tr.set_epoch(0)
    assert tr.validate() == off
    # horizon: CPU tensors in, S summaries out
    batch = next(iter(tr.val_loader))
    S = 3
    clip_class = torch.cat([batch["slot_class"].cpu(), batch["tgt_class"].cpu()[:, -1:].expand(-1, S, -1)], 1)
    clip_box = torch.cat([batch["slot_box"].cpu(), batch["tgt_box"].cpu()[:, -1:].expand(-1, S, -1, -1)], 1)
    out = tr.evaluate_rollout(clip_class, clip_box, temperature=0.8, top_k=5, seed=3)
    assert len(out) == S
    for s in out:
        assert set(s) == SUMMARY_KEYS and s["scored"] == 2 * 8 and 0.0 <= s["accuracy"] <= 1.0

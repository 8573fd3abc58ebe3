"""CPU: the validation metrics without a GPU - the fp64 restatement (tests/metrics_ref.py) on a case worked out by hand,
MetricsRecord.summary() from hand-filled counts, the library's planners and its refusals (decided before any HIP call),
and the Trainer's knobs on an engine that has no metrics kernel."""
import ctypes
import math

import pytest
import torch

import metrics_ref as R
from helpers import oracle_factory, reference_args

NAN = float("nan")
SMALL = dict(batch_size=4, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1, train_clips=8, val_clips=4)


def _hand_case():
    """C = 3, (B,T,N) = (1,2,3), top_k = 2, iou_thr = 0.5, iou_eps = 0.  Every raw box is 0, so p = (.5,.5,.5,.5): the box
    [.25,.75] x [.25,.75] of area 1/4.
      (t0,n0) logits [3,0,0], target 0, box (.5,.5,.5,.5): pred 0, rank 0; IoU 1, L1 0; NLL = log(1 + 2 e^-3)
      (t0,n1) logits [2,2,0], target 1 - A TIE: the first maximum is 0, so top-1 misses; rank = 0 larger + 1 equal with a
              lower index = 1 < 2, so top-2 hits; box (.5,.5,.5,.25): inter = .5 * .25 = 1/8, union = 1/4 + 1/8 - 1/8,
              IoU = 0.5 EXACTLY AT THE THRESHOLD (>=: a hit); L1 = (0+0+0+.25)/4 = 1/16; NLL = log(2 e^2 + 1) - 2
      (t0,n2) target 3 = the reserved id, A PADDED TARGET: unscored, its NaN outputs are not examined
      (t1,n0) logits [NaN,0,0], target 2, valid: A NaN ROW: non-finite, contributes to nothing else
      (t1,n1) target 1 but valid = 0: unscored
      (t1,n2) logits [0,1,5], target 0: pred 2, rank 2 (not in the top 2); box (.25,.25,.25,.25) = [.125,.375]^2:
              inter = (.375 - .25)^2 = 1/64, union = 1/4 + 1/16 - 1/64 = 19/64, IoU = 1/19; all four coordinates differ
              by .25: L1 = 1/4; NLL = 5 + log(1 + e^-4 + e^-5)
    Counts: SCORED 3, TOP1 1, TOPK 2, IOU_HIT 2, BOTH_HIT 1, NONFINITE 1, UNSCORED 2; CONF[0][0] = CONF[1][0] = CONF[0][2] = 1.
    Sums: IOU = 1 + 1/2 + 1/19, BOX_L1 = 0 + 1/16 + 1/4, IOU_BY_CLASS = [1 + 1/19, 1/2, 0]."""
    logits = torch.tensor([[[[3.0, 0, 0], [2, 2, 0], [NAN, NAN, NAN]], [[NAN, 0, 0], [1, 2, 3], [0, 1, 5]]]])
    raw = torch.zeros(1, 2, 3, 4)
    raw[0, 0, 2] = NAN
    tgt_class = torch.tensor([[[0, 1, 3], [2, 1, 0]]])
    tgt_box = torch.full((1, 2, 3, 4), 0.5)
    tgt_box[0, 0, 1, 3] = 0.25
    tgt_box[0, 1, 2] = 0.25
    valid = torch.tensor([[[1.0, 1, 1], [1, 0, 1]]])
    return logits, raw, tgt_class, tgt_box, valid


def test_restatement_on_the_hand_case():
    counts, sums, iou = R.metrics_ref(*_hand_case(), top_k=2, iou_thr=0.5, iou_eps=0.0)
    assert counts[:7].tolist() == [3, 1, 2, 2, 1, 1, 2] and int(counts[7]) == 0
    assert counts[R.CONF:].view(3, 3).tolist() == [[1, 0, 1], [1, 0, 0], [0, 0, 0]]
    want_nll = math.log(1 + 2 * math.exp(-3)) + (math.log(2 * math.exp(2) + 1) - 2) + (5 + math.log(1 + math.exp(-4) + math.exp(-5)))
    assert abs(float(sums[R.NLL]) - want_nll) < 1e-12
    assert abs(float(sums[R.IOU]) - (1 + 0.5 + 1 / 19)) < 1e-12 and abs(float(sums[R.BOX_L1]) - (1 / 16 + 1 / 4)) < 1e-12
    assert float(sums[3]) == 0.0
    by_class = sums[R.IOU_BY_CLASS:].tolist()
    assert abs(by_class[0] - (1 + 1 / 19)) < 1e-12 and by_class[1] == 0.5 and by_class[2] == 0.0
    assert float(iou[0, 0, 1]) == 0.5 and float(iou[0, 0, 0]) == 1.0                  # the threshold case is exact
    assert torch.isnan(iou).view(-1).tolist() == [False, False, True, True, True, False]
    # top_k = 1 is top-1; top_k = C takes every scored token; a threshold just above 1/2 loses the exact hit
    assert int(R.metrics_ref(*_hand_case(), top_k=1, iou_thr=0.5, iou_eps=0.0)[0][R.TOPK]) == 1
    assert int(R.metrics_ref(*_hand_case(), top_k=3, iou_thr=0.5, iou_eps=0.0)[0][R.TOPK]) == 3
    c2 = R.metrics_ref(*_hand_case(), top_k=2, iou_thr=0.5 + 1e-9, iou_eps=0.0)[0]
    assert int(c2[R.IOU_HIT]) == 1 and int(c2[R.BOTH_HIT]) == 1
    # valid = None: the masked token is scored too (logits [1,2,3], target 1: pred 2, rank 1)
    c3 = R.metrics_ref(*_hand_case()[:4], None, top_k=2, iou_thr=0.5, iou_eps=0.0)[0]
    assert c3[:7].tolist() == [4, 1, 3, 3, 1, 1, 1]
    # t0: the second target frame against one output frame
    lg, rw, tc, tb, va = _hand_case()
    c4 = R.metrics_ref(lg[:, 1:], rw[:, 1:], tc, tb, va, top_k=2, iou_thr=0.5, iou_eps=0.0, t0=1)[0]
    assert c4[:7].tolist() == [1, 0, 0, 0, 0, 1, 1]


def test_record_summary_from_hand_filled_counts():
    from vlg import metrics as M
    assert (M.SCORED, M.TOP1, M.TOPK, M.IOU_HIT, M.BOTH_HIT, M.NONFINITE, M.UNSCORED, M.CONF) == (0, 1, 2, 3, 4, 5, 6, 8)
    assert (M.NLL, M.IOU, M.BOX_L1, M.IOU_BY_CLASS) == (0, 1, 2, 4)
    rec = M.MetricsRecord(3, rows=2)
    assert rec.counts.shape == (2, 17) and rec.counts.dtype == torch.int64 and not bool(rec.counts.any())
    assert rec.sums.shape == (2, 7) and rec.sums.dtype == torch.float64 and not bool(rec.sums.any())
    # row 0: 10 scored tokens, 6 of class 0 (4 right, 2 taken for class 2), 4 of class 1 (3 right, 1 taken for class 0), none of class 2
    c = rec.counts[0]
    c[M.SCORED], c[M.TOP1], c[M.TOPK], c[M.IOU_HIT], c[M.BOTH_HIT], c[M.NONFINITE], c[M.UNSCORED] = 10, 7, 9, 5, 4, 2, 3
    c[M.CONF:] = torch.tensor([4, 0, 2, 1, 3, 0, 0, 0, 0])
    s = rec.sums[0]
    s[M.NLL], s[M.IOU], s[M.BOX_L1] = 5.0, 4.0, 1.0
    s[M.IOU_BY_CLASS:] = torch.tensor([3.0, 1.0, 0.0])
    top, empty = rec.summary()
    assert (top["scored"], top["nonfinite"], top["unscored"]) == (10, 2, 3)
    assert top["accuracy"] == 0.7 and top["topk_accuracy"] == 0.9 and top["iou_hit"] == 0.5 and top["both_hit"] == 0.4
    assert top["nll"] == 0.5 and top["perplexity"] == math.exp(0.5) and top["mean_iou"] == 0.4 and top["box_l1"] == 0.1
    assert top["per_class_accuracy"] == [4 / 6, 0.75, None] and top["per_class_iou"] == [0.5, 0.25, None]
    assert top["macro_accuracy"] == (4 / 6 + 0.75) / 2 and top["macro_iou"] == 0.375
    assert top["confusion"] == [[4, 0, 2], [1, 3, 0], [0, 0, 0]]
    # row 1: nothing scored - every ratio is None, nothing divides by zero
    assert (empty["scored"], empty["nonfinite"], empty["unscored"]) == (0, 0, 0)
    for k in ("accuracy", "topk_accuracy", "nll", "perplexity", "mean_iou", "iou_hit", "both_hit", "box_l1", "macro_accuracy", "macro_iou"):
        assert empty[k] is None, k
    assert empty["per_class_accuracy"] == [None] * 3 and empty["per_class_iou"] == [None] * 3
    assert empty["confusion"] == [[0] * 3] * 3
    # all_reduce hands both tensors to the callable; two ranks with the same record double it
    def two_ranks(tensors):
        for t in tensors:
            t.mul_(2)
    rec.all_reduce(two_ranks)
    twice = rec.summary()[0]
    assert twice["scored"] == 20 and twice["accuracy"] == 0.7 and twice["nll"] == 0.5 and twice["per_class_iou"] == [0.5, 0.25, None]
    rec.reset()
    assert not bool(rec.counts.any()) and not bool(rec.sums.any())
    with pytest.raises(ValueError):
        M.MetricsRecord(0)


def test_planners_without_a_gpu():
    from vlg import hip, metrics as M
    lib = hip.load()
    assert lib.vlg_layout_metrics_counts(20) == 408 == M.n_counts(20)
    assert lib.vlg_layout_metrics_sums(20) == 24 == M.n_sums(20)
    assert lib.vlg_layout_metrics_counts(7) == 57 and lib.vlg_layout_metrics_sums(7) == 11
    assert lib.vlg_layout_metrics_scratch() > 0


def test_refusals_are_decided_before_any_hip_call():
    """Dummy addresses, NULL stream, no GPU: a refused call returns its code without touching HIP or the pointers."""
    from vlg import hip
    f = hip.load().vlg_layout_metrics
    buf = (ctypes.c_char * 256)()
    a = (ctypes.addressof(buf) + 15) & ~15                                          # a 16-byte-aligned host address, never dereferenced
    good = dict(out=a, ld=24, tgt_class=a, tgt_box=a, valid=a, tgt_T=4, t0=0, counts=a, sums=a, scratch=a,
                B=2, T=4, N=3, n_classes=20, top_k=5, iou_thr=0.5, iou_eps=1e-7)

    def code(**over):
        return f(*list(dict(good, **over).values()), None)

    for over in (dict(top_k=0), dict(top_k=21), dict(n_classes=29), dict(n_classes=0, top_k=1), dict(t0=1), dict(tgt_T=3),
                 dict(t0=-1), dict(ld=22), dict(ld=20), dict(B=0), dict(T=0), dict(N=0), dict(iou_thr=float("inf")),
                 dict(iou_thr=NAN)):
        assert code(**over) == 1001, over
    for over in (dict(out=a + 4), dict(out=0), dict(tgt_box=a + 8), dict(scratch=a + 8), dict(scratch=0), dict(sums=a + 4),
                 dict(sums=0), dict(tgt_class=a + 4), dict(tgt_class=0), dict(counts=a + 4), dict(counts=0), dict(valid=a + 2)):
        assert code(**over) == 1002, over
    assert code(ld=22, out=a + 4) == 1001                                           # shape grounds come first


def test_trainer_knobs_and_the_refusal_without_a_metrics_kernel(tmp_path, monkeypatch):
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    for k in ("VLG_MODEL", "VLG_VAL_METRICS", "VLG_VAL_TOPK", "VLG_VAL_IOU_THR"):
        monkeypatch.delenv(k, raising=False)
    from trainer import Trainer, metrics_knobs
    a = reference_args(tmp_path / "exp", **SMALL)
    assert metrics_knobs(a) == {"on": False, "top_k": 5, "iou_thr": 0.5}
    tr = Trainer(a, engine_factory=oracle_factory)
    tr.set_epoch(0)
    off = tr.validate()
    assert list(off) == ["loss"]                                                    # off: exactly what it returned before
    monkeypatch.setenv("VLG_VAL_METRICS", "1")
    monkeypatch.setenv("VLG_VAL_TOPK", "3")
    monkeypatch.setenv("VLG_VAL_IOU_THR", "0.75")
    assert metrics_knobs(a) == {"on": True, "top_k": 3, "iou_thr": 0.75}
    b = reference_args(tmp_path / "exp", val_metrics=0, val_topk=2, val_iou_thr=0.25, **SMALL)
    assert metrics_knobs(b) == {"on": False, "top_k": 2, "iou_thr": 0.25}           # an args attribute wins
    with pytest.raises(ValueError, match="VLG_VAL_METRICS"):
        tr.validate()                                                               # OracleEngine has no accumulate_metrics
    batch = next(iter(tr.val_loader))
    with pytest.raises(ValueError, match="evaluate_rollout"):
        tr.evaluate_rollout(batch["slot_class"], batch["slot_box"])

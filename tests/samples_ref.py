"""CPU restatement of the sampled futures in fp64 (include/vlg_hip.h: vlg_layout_decode_samples and "sampled futures"; DESIGN.md
"Sampled futures"): the sample counter, the batched decoding step, and the scores, diversity, selection and record of
csrc/samples.hip.  Plain module: test infrastructure, nothing collected.

Counter.  A batch of B clips holds B / clips samples of `clips` prompts, sample-major: batch clip b is prompt b % clips, sample
k = sample0 + b / clips.  Token (b, n) draws with Philox counter (r0, step, stream, k), r0 = (b % clips)*N + n.  philox_ref.words
fixes the fourth word at 0, so the counter is built here on philox_ref.philox4x32_10 itself.
Decoding.  decode_ref.decode_step's rule, word for word - the function itself runs, handed the sample's uniforms.
Scores.  A token is scored when its truth class is in [0, C).  iou = IoU of the (cx,cy,w,h) boxes, inter / (union + eps), min / max
ignoring a NaN operand as fminf / fmaxf do, 0 when the generated class is >= C; disp = the distance of the two centres; hit =
classes equal.  Per (sample, clip): IOU, ADE, ACC = means over the clip's scored tokens, FDE = the mean of disp over those of
the last frame, the two counts, two zeros; a mean over nothing is 0.  Diversity per clip, over pairs j < k and scored tokens:
mean of 1 - IoU(box_j, box_k), share of cls_j != cls_k; 0 for K = 1.  Selection: the first sample that is not NaN and strictly
better than every earlier one (IOU, ACC larger; ADE, FDE smaller), 0 if all are NaN.  Record: sums over the clips with a scored
token of each score column's own optimum, its mean over K and its value at the selected sample, the two diversities and 1; the
FDE terms only for clips with a scored token in the last frame, counted apart."""
import numpy as np
import torch

import boxhead_ref as BH
import decode_ref as D
import philox_ref as P

COLS, IOU, ADE, FDE, ACC, N_SCORED, N_SCORED_LAST = 8, 0, 1, 2, 3, 4, 5
REC_BEST, REC_MEAN, REC_SELECTED, REC_DIV_BOX, REC_DIV_CLASS, REC_CLIPS, REC_CLIPS_FDE, REC_SLOTS = 0, 4, 8, 12, 13, 14, 15, 16
SCORE_COLS = (IOU, ADE, FDE, ACC)
MINIMISED = (ADE, FDE)


# ---- the counter ------------------------------------------------------------------------------------------------------------
def words(index, step, stream, seed, sample):
    """the four Philox words of counter (index, step, stream, sample) under the seed's key; index and sample broadcast"""
    index, sample = np.broadcast_arrays(np.asarray(index, dtype=np.uint64), np.asarray(sample, dtype=np.uint64))
    z = np.zeros_like(index)
    k0, k1 = P.key(seed)
    return P.philox4x32_10((index, z + np.uint64(step), z + np.uint64(stream), sample), (z + np.uint64(k0), z + np.uint64(k1)))


def uniform(tokens, step, seed, sample):
    """u of the class draw of prompt tokens `tokens` at `step` in sample `sample`: float64 inside (0, 1)"""
    return P.unit64(words(tokens, step, P.CLASS_DRAW, seed, sample)[0])


def batch_counter(R, clips_n, sample0):
    """rows r = b*N + n of a sample-major batch -> (prompt token r0, sample index k); clips_n = clips * N"""
    r = np.arange(R)
    return r % clips_n, sample0 + r // clips_n


# ---- the batched decoding step ------------------------------------------------------------------------------------------------
def decode_step(logits64, step, temperature, top_k, seed, clips_n, sample0=0, margin=1e-5):
    """decode_ref.decode_step on the rows of a sample-major batch: (classes (R,), near (R,)).  The rule is decode_ref's own
    function; only the uniforms it is handed are the samples'."""
    R = np.asarray(logits64).shape[0]
    r0, k = batch_counter(R, clips_n, sample0)
    u = uniform(r0, step, seed, k)
    saved = D.uniform
    D.uniform = lambda tokens, step_, seed_: u
    try:
        return D.decode_step(logits64, step, temperature, top_k, seed, margin)
    finally:
        D.uniform = saved


def sampled_boxes(out_last, n_classes, step, box_temperature, seed, clips_n, sample0=0):
    """boxhead_ref.sampled_boxes with the sample word: rows [logits | raw mean | raw scale | ...] -> boxes (R, 4) float64"""
    o = out_last.detach().cpu().double()
    C = n_classes
    mu = torch.sigmoid(o[:, C:C + 4])
    if box_temperature == 0:
        return mu
    sigma = torch.exp(BH.S_MIN + (BH.S_MAX - BH.S_MIN) * torch.sigmoid(o[:, C + 4:C + 8]))
    r0, k = batch_counter(o.shape[0], clips_n, sample0)
    z = torch.from_numpy(BH.normals_of_words(words(r0, step, BH.BOX_STREAM, seed, k)))
    return (mu + float(np.float32(box_temperature)) * sigma * z).clamp(0.0, 1.0)


def next_frame(out_last, cls_in, box_in, n_classes, step, temperature=0.0, top_k=0, seed=0, keep_padded=False,
               box_temperature=0.0, clips=None, sample0=0):
    """the frame a _samples decoding step generates from out_last (B*N, >= C+4) and the newest frame of the window
    cls_in (B,T,N) / box_in (B,T,N,4): (classes (B,N) int64, boxes (B,N,4) float64, near (B,N) bool).  clips None: B."""
    B, T, N = cls_in.shape
    clips_n = (B if clips is None else clips) * N
    o = out_last.detach().cpu().double()
    cls, near = decode_step(o[:, :n_classes].numpy(), step, temperature, top_k, seed, clips_n, sample0)
    cls, near = torch.from_numpy(cls).view(B, N), torch.from_numpy(near).view(B, N)
    box = sampled_boxes(out_last, n_classes, step, box_temperature, seed, clips_n, sample0).view(B, N, 4)
    if keep_padded:
        pad = cls_in[:, -1] >= n_classes
        cls = torch.where(pad, cls_in[:, -1], cls)
        box = torch.where(pad[..., None], box_in[:, -1].double(), box)
        near = near & ~pad
    return cls, box, near


# ---- scores -------------------------------------------------------------------------------------------------------------------
def _np(x, dt):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(dt)


def iou(a, b, eps):
    """IoU of (..., 4) boxes (cx, cy, w, h); np.fmin / np.fmax ignore a NaN operand as fminf / fmaxf do"""
    ax1, ax2, ay1, ay2 = a[..., 0] - 0.5 * a[..., 2], a[..., 0] + 0.5 * a[..., 2], a[..., 1] - 0.5 * a[..., 3], a[..., 1] + 0.5 * a[..., 3]
    bx1, bx2, by1, by2 = b[..., 0] - 0.5 * b[..., 2], b[..., 0] + 0.5 * b[..., 2], b[..., 1] - 0.5 * b[..., 3], b[..., 1] + 0.5 * b[..., 3]
    iw = np.fmax(np.fmin(ax2, bx2) - np.fmax(ax1, bx1), 0.0)
    ih = np.fmax(np.fmin(ay2, by2) - np.fmax(ay1, by1), 0.0)
    inter = iw * ih
    return inter / (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter + eps)


def token_values(gen_cls, gen_box, clip_class, clip_box, t0, n_classes, iou_eps):
    """gen (K,B,S,N[,4]) against frames t0 .. t0+S-1 of the clip -> dict of (K,B,S,N) float64 iou, disp, hit and (B,S,N) bool scored"""
    gc, gb = _np(gen_cls, np.int64), _np(gen_box, np.float64)
    S = gc.shape[2]
    tc, tb = _np(clip_class, np.int64)[:, t0:t0 + S], _np(clip_box, np.float64)[:, t0:t0 + S]
    with np.errstate(invalid="ignore"):
        v = np.where(gc >= n_classes, 0.0, iou(gb, tb[None], float(np.float32(iou_eps))))
        disp = np.sqrt((gb[..., 0] - tb[None, ..., 0]) ** 2 + (gb[..., 1] - tb[None, ..., 1]) ** 2)
    return dict(iou=v, disp=disp, hit=(gc == tc[None]).astype(np.float64), scored=(tc >= 0) & (tc < n_classes))


def scores(gen_cls, gen_box, clip_class, clip_box, t0, n_classes, iou_eps):
    """(K,B,COLS) float64"""
    t = token_values(gen_cls, gen_box, clip_class, clip_box, t0, n_classes, iou_eps)
    K, B, S, N = t["iou"].shape
    out = np.zeros((K, B, COLS))
    for b in range(B):
        m = t["scored"][b]
        n, n_last = int(m.sum()), int(m[-1].sum())
        out[:, b, N_SCORED], out[:, b, N_SCORED_LAST] = n, n_last
        for k in range(K):
            if n:
                out[k, b, IOU], out[k, b, ADE], out[k, b, ACC] = t["iou"][k, b][m].mean(), t["disp"][k, b][m].mean(), t["hit"][k, b][m].mean()
            if n_last:
                out[k, b, FDE] = t["disp"][k, b, -1][m[-1]].mean()
    return out


def diversity(gen_cls, gen_box, clip_class, t0, n_classes, iou_eps):
    """(B,2) float64"""
    gc, gb = _np(gen_cls, np.int64), _np(gen_box, np.float64)
    K, B, S, N = gc.shape
    tc = _np(clip_class, np.int64)[:, t0:t0 + S]
    scored = (tc >= 0) & (tc < n_classes)
    out = np.zeros((B, 2))
    for b in range(B):
        m = scored[b]
        terms = int(m.sum()) * (K * (K - 1) // 2)
        if terms == 0:
            continue
        box = cls = 0.0
        for j in range(K):
            for k in range(j + 1, K):
                with np.errstate(invalid="ignore"):
                    box += float((1.0 - iou(gb[j, b][m], gb[k, b][m], float(np.float32(iou_eps)))).sum())
                cls += float((gc[j, b][m] != gc[k, b][m]).sum())
        out[b] = box / terms, cls / terms
    return out


def choose(values, col):
    """the selection rule on one clip's K scores of column col"""
    pick, best = -1, 0.0
    for k, v in enumerate(values):
        v = float(v)
        if v != v:
            continue
        if pick < 0 or (v < best if col in MINIMISED else v > best):
            pick, best = k, v
    return max(pick, 0)


def select(sc, criterion):
    """best (B,) int64 from scores (K,B,COLS)"""
    sc = _np(sc, np.float64)
    return np.array([choose(sc[:, b, criterion], criterion) for b in range(sc.shape[1])], dtype=np.int64)


def record(sc, div, criterion):
    """what one vlg_layout_sample_select call adds to a record: REC_SLOTS float64"""
    sc, div = _np(sc, np.float64), _np(div, np.float64)
    K, B, _ = sc.shape
    best, rec = select(sc, criterion), np.zeros(REC_SLOTS)
    for b in range(B):
        if not sc[0, b, N_SCORED] > 0:
            continue
        last = sc[0, b, N_SCORED_LAST] > 0
        for col in SCORE_COLS:
            if col == FDE and not last:
                continue
            rec[REC_BEST + col] += sc[choose(sc[:, b, col], col), b, col]
            rec[REC_MEAN + col] += sc[:, b, col].sum() / K
            rec[REC_SELECTED + col] += sc[best[b], b, col]
        rec[REC_DIV_BOX] += div[b, 0]
        rec[REC_DIV_CLASS] += div[b, 1]
        rec[REC_CLIPS] += 1
        rec[REC_CLIPS_FDE] += 1 if last else 0
    return rec


def score_case(K, B, S, N, seed, n_classes=20, t0=2):
    """Samples and a truth for the score kernels: (gen_cls (K,B,S,N), gen_box (K,B,S,N,4), clip_class (B,t0+S+1,N), clip_box).
    Truth and samples hold the reserved id n_classes here and there (unscored tokens; generated padding scores IoU 0).
    B >= 2: the last clip has no scored token.  K >= 2: sample K-1 of clip 0 IS the truth.  K >= 3: sample 1 is a copy of
    sample 0 in every clip, and after that one box of sample K-2 of clip min(1, B-1), on a scored token, is NaN."""
    g = torch.Generator().manual_seed(seed)
    C, TT = n_classes, t0 + S + 1

    def boxes(*shape):
        return torch.cat([0.2 + 0.6 * torch.rand(*shape, 2, generator=g), 0.1 + 0.4 * torch.rand(*shape, 2, generator=g)], -1)

    clip_class, clip_box = torch.randint(0, C + 1, (B, TT, N), generator=g), boxes(B, TT, N)
    gen_cls, gen_box = torch.randint(0, C + 1, (K, B, S, N), generator=g), boxes(K, B, S, N)
    near = torch.rand(K, B, S, N, generator=g) < 0.5                       # half the samples' tokens near the truth: real overlaps
    truth_c, truth_b = clip_class[:, t0:t0 + S], clip_box[:, t0:t0 + S]
    gen_box = torch.where(near[..., None], (truth_b[None] + 0.05 * torch.randn(K, B, S, N, 4, generator=g)).clamp(0.02, 1.0), gen_box)
    gen_cls = torch.where(near, truth_c[None].expand(K, B, S, N), gen_cls)
    nan_clip = min(1, B - 1)
    clip_class[nan_clip, t0, 0] = 3                                        # the token that gets the NaN box is scored
    clip_class[0, t0 + S - 1, N - 1] = 5                                   # and clip 0 has a scored token in its last frame
    if B >= 2:
        clip_class[B - 1, t0:t0 + S] = C
    if K >= 2:
        gen_cls[K - 1, 0], gen_box[K - 1, 0] = clip_class[0, t0:t0 + S], clip_box[0, t0:t0 + S]
    if K >= 3:
        gen_cls[1], gen_box[1] = gen_cls[0], gen_box[0]
        gen_box[K - 2, nan_clip, 0, 0] = float("nan")
        gen_cls[K - 2, nan_clip, 0, 0] = 3                                 # (a generated padding id would score IoU 0 whatever the box)
    return gen_cls.contiguous(), gen_box.contiguous(), clip_class.contiguous(), clip_box.contiguous()


def summary(rec):
    """vlg.samples.SampleRecord.summary() of a record given as REC_SLOTS numbers"""
    from vlg.samples import SampleRecord
    r = SampleRecord()
    r.sums.copy_(torch.as_tensor(np.asarray(rec, dtype=np.float64)))
    return r.summary()

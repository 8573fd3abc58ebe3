#!/usr/bin/env python
"""Development tool: the per-clip attention kernels (csrc/attention_clip.hip) alone at the metric shape.
    python tools/clip_attn_bench.py [B] [T] [N] [d] [--valid] [--bf16] [--step] [--frame]
--frame: the frame-local instantiations instead (vlg_attention_frame_*, the odd layers of attention = "factored"): work =
N^2 T pairs per clip and head forward, N^2 per step.
--bf16: the fp32 and the bf16-storage kernels on the same shape, timed alternately in one process (bf16 rates against the
2.5 PF/s bf16 MFMA peak).  --step: the generation step kernel instead, at p = 0, T/2, T-1, both storages."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg import hip

FRAME = "--frame" in sys.argv
E = "vlg_attention_frame_" if FRAME else "vlg_attention_clip_"        # the entry points' common prefix
KIND = "frame" if FRAME else "clip"

def step_bench(B, T, N, d, valid):
    """the generation step (vlg_attention_clip_step) alone at p = 0, T/2, T-1, fp32 and bf16 alternately; work = the visible
    (query, key) pairs of frame p: 4 * 64 flop x N * N (p + 1) per clip and head"""
    dev, st = torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream
    qkv = torch.randn(B * T * N, 3 * d, device=dev) * 0.7
    q16 = qkv.bfloat16()
    o, o16 = torch.empty(B * N, d, device=dev), torch.empty(B * N, d, device=dev, dtype=torch.bfloat16)
    vp = valid.data_ptr() if valid is not None else 0
    runs = []
    for p in sorted({0, T // 2, T - 1}):
        fl = 4.0 * B * d * N * N * (1 if FRAME else p + 1)
        runs.append(("step p=%d" % p, lambda p=p: hip.call(E + "step", qkv.data_ptr(), vp, o.data_ptr(), B, T, N, d, p, d, st),
                     fl, 157.3))
        runs.append(("step bf16 p=%d" % p, lambda p=p: hip.call(E + "step_bf16", q16.data_ptr(), vp, o16.data_ptr(), B, T, N,
                                                               d, p, d, st), fl, 2500.0))
    for _, fn, _, _ in runs:
        for _ in range(3):
            fn()
    ts = {name: [] for name, _, _, _ in runs}
    for _ in range(5):                               # rounds: every kernel once per round
        for name, fn, _, _ in runs:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(20):
                fn()
            e.record()
            torch.cuda.synchronize()
            ts[name].append(s.elapsed_time(e) / 20)
    for name, _, work, peak in runs:
        t = sorted(ts[name])
        print(KIND + " attention %s  (B,T,N,d)=(%d,%d,%d,%d)%s: %.1f us (min %.1f max %.1f; 20 launches back to back)  %.1f TFLOP/s "
              "(%.3f of %.1f)" % (name, B, T, N, d, " +valid" if valid is not None else "", t[2] * 1e3, t[0] * 1e3, t[-1] * 1e3,
                                  work / t[2] / 1e9, work / t[2] / 1e9 / peak, peak))


a = [x for x in sys.argv[1:] if not x.startswith("--")]
B, T, N, d = (int(a[i]) if len(a) > i else v for i, v in enumerate((32, 16, 64, 256)))
dev = torch.device("cuda:0")
hip.load()
M, S, heads = B * T * N, T * N, d // 64
qkv, dout = torch.randn(M, 3 * d, device=dev) * 0.7, torch.randn(M, d, device=dev)
out, dqkv = torch.empty(M, d, device=dev), torch.empty(M, 3 * d, device=dev)
lse, delta = torch.empty(B * heads * S, device=dev), torch.empty(B * heads * S, device=dev)
valid = torch.ones(B, T, N, device=dev) if "--valid" in sys.argv else None
if "--step" in sys.argv:
    step_bench(B, T, N, d, valid)
    sys.exit(0)
P = lambda t: 0 if t is None else t.data_ptr()
st = torch.cuda.current_stream().cuda_stream
fwd = lambda: hip.call(E + "fwd", P(qkv), P(valid), P(out), P(lse), B, T, N, d, st)
bwd = lambda: hip.call(E + "bwd", P(qkv), P(valid), P(out), P(dout), P(lse), P(delta), P(dqkv), B, T, N, d, st)
fl = 4.0 * B * d * N * N * T * (1.0 if FRAME else (T + 1) / 2.0)
kernels = [("fwd", fwd, fl, 157.3), ("bwd", bwd, 2.5 * fl, 157.3)]
if "--bf16" in sys.argv:
    q16, g16 = qkv.bfloat16(), dout.bfloat16()
    o16, dq16 = torch.empty(M, d, device=dev, dtype=torch.bfloat16), torch.empty(M, 3 * d, device=dev, dtype=torch.bfloat16)
    fwd16 = lambda: hip.call(E + "fwd_bf16", P(q16), P(valid), P(o16), P(lse), B, T, N, d, st)
    bwd16 = lambda: hip.call(E + "bwd_bf16", P(q16), P(valid), P(o16), P(g16), P(lse), P(delta), P(dq16),
                             B, T, N, d, st)
    kernels = [("fwd", fwd, fl, 157.3), ("fwd bf16", fwd16, fl, 2500.0), ("bwd", bwd, 2.5 * fl, 157.3),
               ("bwd bf16", bwd16, 2.5 * fl, 2500.0)]
for _, fn, _, _ in kernels:
    for _ in range(3):
        fn()
ts = {name: [] for name, _, _, _ in kernels}
for _ in range(5):                                   # rounds: every kernel once per round, so drift hits all alike
    for name, fn, _, _ in kernels:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(5):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts[name].append(s.elapsed_time(e) / 5)
for name, _, work, peak in kernels:
    lo, t, hi = sorted(ts[name])[0], sorted(ts[name])[2], sorted(ts[name])[-1]
    print(KIND + " attention %s  (B,T,N,d)=(%d,%d,%d,%d)%s: %.1f us (min %.1f max %.1f)  %.1f TFLOP/s algorithmic (%.3f of %.1f)" % (
        name, B, T, N, d, " +valid" if valid is not None else "", t * 1e3, lo * 1e3, hi * 1e3, work / t / 1e9, work / t / 1e9 / peak, peak))

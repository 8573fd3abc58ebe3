#!/usr/bin/env python
"""Development tool: the per-clip attention kernels (csrc/attention_clip.hip) alone at the metric shape.
    python tools/clip_attn_bench.py [B] [T] [N] [d] [--valid] [--bf16] [--step] [--frame]
--frame: the frame-local instantiations instead (vlg_attention_frame_*, the odd layers of attention = "factored").  Work =
the kind's visible (query, key) pairs (vlg/attention.py), 4 * 64 flop each per clip and head.
--bf16: the fp32 and the bf16-storage kernels on the same shape, timed alternately in one process (bf16 rates against the
2.5 PF/s bf16 MFMA peak).  --step: the generation step kernel instead, at p = 0, T/2, T-1, both storages."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg import attention, hip

K = attention.FRAME if "--frame" in sys.argv else attention.CLIP      # entry points, pair counts: vlg/attention.py
E = K.stem + "_"                                                      # the entry points' common prefix
KIND = "frame" if K is attention.FRAME else "clip"


def bench(runs, reps, note, what):
    """runs: (name, launch, flop, peak TFLOP/s).  Five rounds, every kernel once per round (`reps` launches back to back), so
    drift hits all alike; prints the median round of each"""
    for _, fn, _, _ in runs:
        for _ in range(3):
            fn()
    ts = {name: [] for name, _, _, _ in runs}
    for _ in range(5):
        for name, fn, _, _ in runs:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            ts[name].append(s.elapsed_time(e) / reps)
    for name, _, work, peak in runs:
        t = sorted(ts[name])
        print(KIND + " attention %s  (B,T,N,d)=(%d,%d,%d,%d)%s: %.1f us (min %.1f max %.1f%s)  %.1f TFLOP/s %s(%.3f of %.1f)" % (
            name, B, T, N, d, " +valid" if valid is not None else "", t[2] * 1e3, t[0] * 1e3, t[-1] * 1e3, note, work / t[2] / 1e9,
            what, work / t[2] / 1e9 / peak, peak))


a = [x for x in sys.argv[1:] if not x.startswith("--")]
B, T, N, d = (int(a[i]) if len(a) > i else v for i, v in enumerate((32, 16, 64, 256)))
dev = torch.device("cuda:0")
hip.load()
M, S, heads = B * T * N, T * N, d // 64
qkv, dout = torch.randn(M, 3 * d, device=dev) * 0.7, torch.randn(M, d, device=dev)
q16, g16 = qkv.bfloat16(), dout.bfloat16()
valid = torch.ones(B, T, N, device=dev) if "--valid" in sys.argv else None
P = lambda t: 0 if t is None else t.data_ptr()
st = torch.cuda.current_stream().cuda_stream
if "--step" in sys.argv:       # the generation step alone at p = 0, T/2, T-1, fp32 and bf16 alternately
    o, o16 = torch.empty(B * N, d, device=dev), torch.empty(B * N, d, device=dev, dtype=torch.bfloat16)
    runs = []
    for p in sorted({0, T // 2, T - 1}):
        fl = 4.0 * B * d * K.step_pairs(N, p)
        runs.append(("step p=%d" % p, lambda p=p: hip.call(E + "step", P(qkv), P(valid), P(o), B, T, N, d, p, d, st), fl, 157.3))
        runs.append(("step bf16 p=%d" % p, lambda p=p: hip.call(E + "step_bf16", P(q16), P(valid), P(o16), B, T, N, d, p, d, st),
                     fl, 2500.0))
    bench(runs, 20, "; 20 launches back to back", "")
    sys.exit(0)
out, dqkv = torch.empty(M, d, device=dev), torch.empty(M, 3 * d, device=dev)
lse, delta = torch.empty(B * heads * S, device=dev), torch.empty(B * heads * S, device=dev)
fl = 4.0 * B * d * K.pairs(T, N)
runs = [("fwd", lambda: hip.call(E + "fwd", P(qkv), P(valid), P(out), P(lse), B, T, N, d, st), fl, 157.3),
        ("bwd", lambda: hip.call(E + "bwd", P(qkv), P(valid), P(out), P(dout), P(lse), P(delta), P(dqkv), B, T, N, d, st), 2.5 * fl, 157.3)]
if "--bf16" in sys.argv:
    o16, dq16 = torch.empty(M, d, device=dev, dtype=torch.bfloat16), torch.empty(M, 3 * d, device=dev, dtype=torch.bfloat16)
    runs[1:1] = [("fwd bf16", lambda: hip.call(E + "fwd_bf16", P(q16), P(valid), P(o16), P(lse), B, T, N, d, st), fl, 2500.0)]
    runs.append(("bwd bf16", lambda: hip.call(E + "bwd_bf16", P(q16), P(valid), P(o16), P(g16), P(lse), P(delta), P(dq16),
                                              B, T, N, d, st), 2.5 * fl, 2500.0))
bench(runs, 5, "", "algorithmic ")

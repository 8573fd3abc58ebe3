#!/usr/bin/env python
"""Development tool: whole layout training steps with the per-clip attention option, two precisions timed alternately in one
process on the same batch (default: bf16 against bf16_mfma, the two modes with bf16 projections).
    python tools/clip_step_bench.py [B] [T] [N] [d] [--layers L] [--precisions bf16,bf16_mfma]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg.data import synthetic_clips, to_device
from vlg.engine import LayoutEngine
from vlg.spec import LayoutConfig


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


skip = {i + 1 for i, x in enumerate(sys.argv) if x in ("--layers", "--precisions")}
a = [x for i, x in enumerate(sys.argv[1:], 1) if not x.startswith("--") and i not in skip]
B, T, N, d = (int(a[i]) if len(a) > i else v for i, v in enumerate((32, 16, 64, 256)))
cfg = LayoutConfig(B=B, T=T, N=N, d=d, n_layers=int(opt("--layers", 4)), attention="clip")
dev = torch.device("cuda:0")
batch = to_device(synthetic_clips(B, T, N, seed=3), dev)
engines = {p: LayoutEngine(cfg, dev, precision=p) for p in opt("--precisions", "bf16,bf16_mfma").split(",")}
for eng in engines.values():
    for _ in range(3):
        eng.train_step(batch)
torch.cuda.synchronize()
ts = {p: [] for p in engines}
for _ in range(7):                                   # rounds: every precision once per round
    for p, eng in engines.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(10):
            eng.train_step(batch)
        e.record()
        torch.cuda.synchronize()
        ts[p].append(s.elapsed_time(e) / 10)
for p in engines:
    t = sorted(ts[p])[3]
    print("clip step %-9s (B,T,N,d)=(%d,%d,%d,%d) %d layers: %.3f ms/step  %.0f clips/s  (min %.3f max %.3f)" % (
        p, B, T, N, d, cfg.n_layers, t, B / t * 1e3, min(ts[p]), max(ts[p])))

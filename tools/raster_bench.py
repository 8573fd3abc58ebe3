#!/usr/bin/env python
"""Development tool: what the rasterised layouts cost ("Rasterised layouts").
    python tools/raster_bench.py [B] [T] [N] [--launches K] [--no-rollout]
1. vlg_layout_rasterize in its three output kinds and vlg_label_confusion, on synthetic_clips at 128x256 and 256x512 and
   on an adversarial input in which every box covers the whole image (the cull removes nothing), alternated in one process
   through one ctypes call each, each launch bracketed by HIP events behind a large fill that keeps the queue busy while
   the host enqueues (so the events bracket the kernel, on cold caches): median, min and max of K launches after warm-up,
   against the store floor (bytes written / 6.2 TB/s) or the read floor (bytes read / 6.2 TB/s).
2. LayoutEngine.evaluate_rollout wall-clock with and without a pixel record, alternated."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg import hip
from vlg.data import synthetic_clips
from vlg.engine import LayoutEngine
from vlg.spec import LayoutConfig

FLOOR_TBS = 6.2                        # what plain streaming stores and loads reach on this chip


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


skip = {i + 1 for i, x in enumerate(sys.argv) if x in ("--launches",)}
a = [x for i, x in enumerate(sys.argv[1:], 1) if not x.startswith("--") and i not in skip]
B, T, N = (int(a[i]) if len(a) > i else v for i, v in enumerate((32, 16, 64)))
K = int(opt("--launches", 50))
dev = torch.device("cuda:0")
lib = hip.load()
s = torch.cuda.current_stream().cuda_stream
C = 20
clips = synthetic_clips(B, T, N, seed=3)
cls, box = clips["slot_class"].to(dev), clips["slot_box"].to(dev)
full = torch.tensor([0.5, 0.5, 1.0, 1.0], device=dev).expand(B, T, N, 4).contiguous()          # every box covers the image
KINDS = (("u8", hip.LABEL_U8, torch.uint8), ("f32", hip.LABEL_F32, torch.float32), ("i64", hip.LABEL_I64, torch.int64))

paths, nbytes, keep = {}, {}, []
for H, W in ((128, 256), (256, 512)):
    for tag, boxes in (("synthetic", box), ("all-cover", full)):
        for name, kind, dtype in KINDS:
            out = torch.empty(B, T, H, W, dtype=dtype, device=dev)
            args = (cls.data_ptr(), boxes.data_ptr(), 0, out.data_ptr(), B, T, 0, T, N, C, H, W, kind, hip.RASTER_CLASS, C, s)
            key = "raster %s %dx%d %s" % (name, H, W, tag)
            paths[key] = (lambda args=args: hip.check(lib.vlg_layout_rasterize(*args), "vlg_layout_rasterize"))
            nbytes[key] = float(out.numel() * out.element_size())
            keep.append(out)
            if name == "u8" and tag == "synthetic":
                pred = out
    # the confusion of the drawn clip against itself shifted by one clip: two different piecewise-constant maps
    truth = torch.empty_like(pred)
    counts = torch.zeros(T, (C + 1) * (C + 1) + 1, dtype=torch.int64, device=dev)
    cargs = (pred.data_ptr(), truth.data_ptr(), counts.data_ptr(), B, T, H * W, C + 1, 1, s)
    key = "confusion %dx%d per_frame" % (H, W)
    paths[key] = (lambda cargs=cargs: hip.check(lib.vlg_label_confusion(*cargs), "vlg_label_confusion"))
    nbytes[key] = 2.0 * pred.numel()
    keep += [truth, counts, (pred, truth)]
for fn in paths.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
for item in keep:
    if isinstance(item, tuple):
        item[1].copy_(torch.roll(item[0], 1, 0))
torch.cuda.synchronize()
blocker = torch.empty(128 << 20, dtype=torch.float32, device=dev)
ev = {k: [] for k in paths}
for _ in range(K):
    for k, fn in paths.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        blocker.zero_()
        e0.record()
        fn()
        e1.record()
        ev[k].append((e0, e1))
torch.cuda.synchronize()
for k in paths:
    t = sorted(x.elapsed_time(y) * 1e3 for x, y in ev[k])
    med, floor = t[len(t) // 2], nbytes[k] / (FLOOR_TBS * 1e6)
    print("%-36s (B,T,N)=(%d,%d,%d): median %8.1f us of %d (min %.1f max %.1f); %7.1f MB, floor %6.1f us, %.2f x floor, %.2f TB/s"
          % (k, B, T, N, med, K, t[0], t[-1], nbytes[k] / 1e6, floor, med / floor, nbytes[k] / med / 1e6))
del keep, blocker

if "--no-rollout" not in sys.argv:
    # ---- evaluate_rollout with and without a pixel record, alternated (4 layers, d = 256, 8 steps after a full window)
    cfg = LayoutConfig(B=B, T=T, N=N, d=256, n_layers=4)
    eng = LayoutEngine(cfg, dev, padded_slots=False)
    S = 8
    long = synthetic_clips(B, T + S, N, seed=5)
    cc, cb = long["slot_class"].to(dev), long["slot_box"].to(dev)
    rec, pix = eng.metrics_record(S), eng.pixel_record(S)
    for size in ((128, 256), (256, 512)):
        runs = {"off": {}, "on": dict(pixel_record=pix, pixel_size=size)}
        for kw in runs.values():
            eng.evaluate_rollout(cc, cb, record=rec, **kw)              # warm-up (allocates the label buffers)
        for rnd in range(3):
            for name, kw in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    eng.evaluate_rollout(cc, cb, record=rec, **kw)
                torch.cuda.synchronize()
                print("round %d evaluate_rollout %d steps, pixel record %s (%dx%d): %.3f ms per call" % (
                    rnd, S, name, size[0], size[1], (time.perf_counter() - t0) * 1e3 / 5))
    print("pixel summary of step 0:", {k: v for k, v in pix.summary()[0].items() if k in ("pixels", "pixel_accuracy", "miou", "background_iou")})

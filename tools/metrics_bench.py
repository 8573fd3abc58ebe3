#!/usr/bin/env python
"""Development tool: what the validation metrics cost ("Validation metrics").
    python tools/metrics_bench.py [B] [T] [N] [d] [--layers L] [--launches K] [--val-clips C] [--one-bin]
1. The vlg_layout_metrics launch against the vlg_layout_loss launch on the same head outputs and targets, alternately in
   one process through the same host path (one ctypes call), each bracketed by HIP events behind a large fill that keeps
   the queue busy while the host enqueues (so the events bracket the kernel, on cold caches): median, min and max of K
   launches after warm-up.  Both read the same rows; the loss also writes them back (dout), the metrics write nothing per token.
2. Trainer.validate() wall-clock with VLG_VAL_METRICS off and on over the same loader, two alternating rounds: the
   expected difference is one launch-bound kernel per batch and one small copy per pass."""
import logging, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd"), os.path.join(ROOT, "tests")]
import torch
from vlg import hip
from vlg.data import synthetic_clips, to_device
from vlg.engine import LayoutEngine
from vlg.spec import IOU_EPS, LOSS_W_CE, LOSS_W_REG, LOSS_W_STRUCT, SMOOTH_L1_BETA, LayoutConfig


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


skip = {i + 1 for i, x in enumerate(sys.argv) if x in ("--layers", "--launches", "--val-clips")}
a = [x for i, x in enumerate(sys.argv[1:], 1) if not x.startswith("--") and i not in skip]
B, T, N, d = (int(a[i]) if len(a) > i else v for i, v in enumerate((32, 16, 64, 256)))
layers, K, val_clips = int(opt("--layers", 4)), int(opt("--launches", 50)), int(opt("--val-clips", 256))
dev = torch.device("cuda:0")
cfg = LayoutConfig(B=B, T=T, N=N, d=d, n_layers=layers)
eng = LayoutEngine(cfg, dev, padded_slots=False)
batch = to_device(synthetic_clips(B, T, N, seed=3), dev)
eng.forward(batch)
rec = eng.metrics_record()
s = torch.cuda.current_stream().cuda_stream
M = cfg.tokens


lib = hip.load()
loss_args = (eng.out.data_ptr(), cfg.n_out, batch["tgt_class"].data_ptr(), batch["tgt_box"].data_ptr(), batch["valid"].data_ptr(),
             eng.dout.data_ptr(), eng.loss_out.data_ptr(), eng.loss_scratch.data_ptr(), B, T, N, cfg.n_classes, SMOOTH_L1_BETA,
             IOU_EPS, LOSS_W_REG, LOSS_W_STRUCT, LOSS_W_CE, s)
metrics_args = (eng.out.data_ptr(), cfg.n_out, batch["tgt_class"].data_ptr(), batch["tgt_box"].data_ptr(), batch["valid"].data_ptr(),
                T, 0, rec.counts.data_ptr(), rec.sums.data_ptr(), eng.metrics_scratch.data_ptr(), B, T, N, cfg.n_classes, 5, 0.5,
                IOU_EPS, s)
# the same host path for both: one ctypes call with arguments built once (what accumulate_metrics launches)
paths = {"vlg_layout_loss": lambda: hip.check(lib.vlg_layout_loss(*loss_args), "vlg_layout_loss"),
         "vlg_layout_metrics": lambda: hip.check(lib.vlg_layout_metrics(*metrics_args), "vlg_layout_metrics")}
if "--one-bin" in sys.argv:
    # the same launch on outputs and targets that fill ONE confusion bin (every target and every prediction class 0):
    # a block then flushes 1 non-zero bin instead of ~100, everything else is unchanged
    out1, tgt1, rec1 = eng.out.clone(), torch.zeros_like(batch["tgt_class"]), eng.metrics_record()
    out1[:, 0] += 100.0
    one_args = (out1.data_ptr(),) + metrics_args[1:2] + (tgt1.data_ptr(),) + metrics_args[3:7] + (rec1.counts.data_ptr(), rec1.sums.data_ptr()) + metrics_args[9:]
    paths["metrics, one bin"] = lambda: hip.check(lib.vlg_layout_metrics(*one_args), "vlg_layout_metrics")
for fn in paths.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
# a launch-bound kernel finishes before the host has enqueued the closing event: a 512 MB fill in front keeps the queue
# busy while event, launch and event are enqueued, so the two events bracket the kernel and not the host
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
nbytes = {"vlg_layout_loss": (2.0 * 4 * cfg.n_out + 28) * M, "vlg_layout_metrics": (4.0 * cfg.n_out + 28) * M,
          "metrics, one bin": (4.0 * cfg.n_out + 28) * M}
for k in paths:
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[k])
    print("%-19s (B,T,N)=(%d,%d,%d) %d tokens: median %.1f us of %d launches (min %.1f max %.1f); %.2f MB algorithmic = %.0f GB/s at the median"
          % (k, B, T, N, M, t[len(t) // 2], K, t[0], t[-1], nbytes[k] / 1e6, nbytes[k] / t[len(t) // 2] / 1e3))
print("record after %d launches: %s" % (K + 5, {k: v for k, v in rec.summary()[0].items() if k in ("scored", "accuracy", "nll", "mean_iou")}))
del eng

# ---- validate() with the knob off and on
from helpers import reference_args
from trainer import Trainer
tmp = tempfile.mkdtemp()
os.makedirs(os.path.join(tmp, "src"))
os.chdir(os.path.join(tmp, "src"))
args = reference_args(os.path.join(tmp, "exp"), batch_size=B, epochs=1, print_freq=10 ** 9, n_frames=T, n_slots=N, d_model=d,
                      n_layers=layers, train_clips=B, val_clips=val_clips)
args.logger.setLevel(logging.WARNING)
tr = Trainer(args)
tr.set_epoch(0)
tr.validate()                                        # warm-up
for rnd in range(2):
    for on in (0, 1):
        args.val_metrics = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tr.validate()
        torch.cuda.synchronize()
        print("round %d validate() VLG_VAL_METRICS=%d: %.2f ms over %d batches of %d clips (loss %.6f%s)" % (
            rnd, on, (time.perf_counter() - t0) * 1e3, len(tr.val_loader), B, out["loss"],
            ", accuracy %.4f mean_iou %.4f" % (out["accuracy"], out["mean_iou"]) if on else ""))

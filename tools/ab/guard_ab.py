"""Cost of the guarded optimiser step (clip_grad + skip_nonfinite, vlg/optim.py) against the default step: whole-step
time of two engines in ONE process, rounds interleaved A B A B on the same box, fp32 and bf16, at the metric shape
(32,16,64) d=256 L=4 and at the 4-clip shard.  Prints one line per (shape, precision): medians and their difference."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg.data import synthetic_clips, to_device
from vlg.engine import LayoutEngine
from vlg.spec import LayoutConfig, SEED

dev = torch.device("cuda:0")
ROUNDS, STEPS = 9, 20


def timed(eng, batch):
    for _ in range(3):
        eng.train_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        eng.train_step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


for B in (32, 4):
    for precision in ("fp32", "bf16"):
        cfg = LayoutConfig(B=B, T=16, N=64, d=256, n_layers=4)
        batch = to_device(synthetic_clips(cfg.B, cfg.T, cfg.N, seed=SEED), dev)
        engines = {"default": LayoutEngine(cfg, dev, seed=SEED, precision=precision),
                   "guarded": LayoutEngine(cfg, dev, seed=SEED, precision=precision, clip_grad=1.0, skip_nonfinite=True)}
        res = {k: [] for k in engines}
        for rnd in range(ROUNDS):
            for k, eng in engines.items():
                t = timed(eng, batch)
                if rnd:                                   # the first round warms clocks and caches
                    res[k].append(t)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        st = engines["guarded"].optimizer_stats()
        print("B=%d %s: default %.3f ms  guarded %.3f ms  (+%.1f us, %+.2f %%)  params %d  skipped %d" % (
            B, precision, med["default"], med["guarded"], (med["guarded"] - med["default"]) * 1e3,
            (med["guarded"] / med["default"] - 1) * 100, engines["guarded"].n_params, st["skipped_steps"]), flush=True)
        del engines

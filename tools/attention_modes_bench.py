#!/usr/bin/env python
"""Development tool: the training step and the grown frame of a short-prompt rollout under attention = slot | clip | factored,
alternately in ONE process at the metric shape, fp32 and bf16.
    python tools/attention_modes_bench.py [B] [T] [N] [d] [--layers L] [--rounds R]
Per round every mode runs once (so drift hits all alike): 15 training steps after 3 of warm-up, and the rollout from a
one-frame prompt with its cached grow steps ("clip" through the engine option clip_cache) - ms per grown frame =
(the T-1-frame call - the prompt pass alone) / (T - 2), host wall-clock around calls that end with the frames on the CPU, as
tools/rollout_bench.py measures.  Prints per mode the median of the rounds with min .. max."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg.attention import MODES, cached_by_default
from vlg.data import synthetic_clips, to_device
from vlg.engine import LayoutEngine
from vlg.spec import LayoutConfig, SEED


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


skip = {i + 1 for i, x in enumerate(sys.argv) if x in ("--layers", "--rounds")}
a = [x for i, x in enumerate(sys.argv) if i and i not in skip and not x.startswith("--")]
B, T, N, d = (int(a[i]) if len(a) > i else v for i, v in enumerate((32, 16, 64, 256)))
L, rounds = opt("--layers", 4), opt("--rounds", 5)
dev = torch.device("cuda:0")
batch = to_device(synthetic_clips(B, T, N, seed=SEED), dev)
pc, pb = batch["slot_class"][:, :1].contiguous(), batch["slot_box"][:, :1].contiguous()
for precision in ("fp32", "bf16"):
    engines = {m: LayoutEngine(LayoutConfig(B=B, T=T, N=N, d=d, n_layers=L, attention=m), dev, seed=SEED, precision=precision,
                               padded_slots=False, clip_cache=not cached_by_default(m)) for m in MODES}
    roll = lambda e, steps: [t.cpu() for t in e.rollout(pc, pb, steps=steps)]
    for e in engines.values():
        for _ in range(3):
            e.train_step(batch)
        roll(e, T - 1)
    step = {m: [] for m in MODES}
    grown = {m: [] for m in MODES}
    for _ in range(rounds):
        for m, e in engines.items():
            for _ in range(3):
                e.train_step(batch)
            step[m].append(wall(lambda: e.train_step(batch), 15))
        for m, e in engines.items():
            roll(e, T - 1)
            grown[m].append((wall(lambda: roll(e, T - 1), 4) - wall(lambda: roll(e, 1), 4)) / (T - 2))
    for what, res in (("training step", step), ("grown frame (cached)", grown)):
        for m in MODES:
            t = sorted(res[m])
            print("%s %-8s %s (B,T,N,d,L)=(%d,%d,%d,%d,%d): %.3f ms  (min %.3f .. max %.3f over %d rounds)" % (
                precision, m, what, B, T, N, d, L, t[len(t) // 2], t[0], t[-1], rounds))
    del engines

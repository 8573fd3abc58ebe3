"""Cost of the training recipe (weight decay + warm-up + EMA on the guarded step, vlg/optim.py) against the default step and
against the guard alone: whole-step time of the three variants in ONE process, rounds interleaved A B C A B C on the same
box, at the metric shape (32,16,64) d=256 L=4 in fp32 and bf16.  Two engines that are built alike do not time alike: where
their buffers land moves the whole step by tens of microseconds, more than the effect looked for, while one engine repeats
to a few.  So every variant is built INSTANCES times, each instance gives the median of its rounds, and a variant is
reported as the median of its instances with their min..max; differences are between those.  Then the Adam launch alone
(HIP events around it, guard against recipe: the two forms whose Adam launch the kernel timer brackets, one instance each)
with its algorithmic bytes, to set against the byte ratio - the figure that does not depend on placement."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg.data import synthetic_clips, to_device
from vlg.engine import KernelTimer, LayoutEngine
from vlg.spec import LayoutConfig, SEED

dev = torch.device("cuda:0")
ROUNDS, STEPS, INSTANCES = 7, 20, 3
RECIPE = dict(weight_decay=0.1, warmup_steps=500, ema_decay=0.999, ema_warmup=True)


def timed(eng, batch):
    for _ in range(3):
        eng.train_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        eng.train_step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


def spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


for precision in ("fp32", "bf16"):
    cfg = LayoutConfig(B=32, T=16, N=64, d=256, n_layers=4)
    batch = to_device(synthetic_clips(cfg.B, cfg.T, cfg.N, seed=SEED), dev)
    variants = {"off": {}, "guard": dict(clip_grad=1.0, skip_nonfinite=True),
                "recipe": dict(clip_grad=1.0, skip_nonfinite=True, **RECIPE)}
    built = [(k, LayoutEngine(cfg, dev, seed=SEED, precision=precision, **kw)) for _ in range(INSTANCES) for k, kw in variants.items()]
    res = [[] for _ in built]
    for rnd in range(ROUNDS):
        for i, (k, eng) in enumerate(built):
            t = timed(eng, batch)
            if rnd:                                   # the first round warms clocks and caches
                res[i].append(t)
    s = {k: spread([spread(r)[0] for (kk, _), r in zip(built, res) if kk == k]) for k in variants}
    within = max(max(r) - min(r) for r in res)
    print("%s step, ms, median (min..max) over %d instances, each the median of %d rounds x %d steps: " % (
        precision, INSTANCES, ROUNDS - 1, STEPS) + "  ".join("%s %.3f (%.3f..%.3f)" % ((k,) + s[k]) for k in variants) +
        "   largest min..max inside one instance %.1f us" % (within * 1e3), flush=True)
    engines = {k: next(e for kk, e in built if kk == k) for k in variants}
    print("%s   guard - off %+.1f us   recipe - guard %+.1f us   recipe - off %+.1f us (%+.2f %%)   params %d  skipped %d" % (
        precision, (s["guard"][0] - s["off"][0]) * 1e3, (s["recipe"][0] - s["guard"][0]) * 1e3,
        (s["recipe"][0] - s["off"][0]) * 1e3, (s["recipe"][0] / s["off"][0] - 1) * 100, engines["recipe"].n_params,
        engines["recipe"].optimizer_stats()["skipped_steps"]), flush=True)
    # the Adam launch alone: events around it, the two engines alternating step by step
    for k in ("guard", "recipe"):
        engines[k].timer = KernelTimer(only=("adam",))
    for _ in range(ROUNDS * STEPS):
        for k in ("guard", "recipe"):
            engines[k].train_step(batch)
    torch.cuda.synchronize()
    adam = {}
    for k in ("guard", "recipe"):
        recs = engines[k].timer.records["adam"][STEPS:]
        us = sorted(a.elapsed_time(b) * 1e3 for a, b, _, _ in recs)
        adam[k] = (us[len(us) // 2], us[0], us[-1], recs[0][3])
    print("%s   Adam launch, us, median (min..max) of %d: " % (precision, len(us)) +
          "  ".join("%s %.2f (%.2f..%.2f) %.2f B/param %.0f GB/s" % (k, a[0], a[1], a[2], a[3] / engines[k].n_params, a[3] / a[0] * 1e-3)
                    for k, a in adam.items()) +
          "   time ratio %.3f  byte ratio %.3f" % (adam["recipe"][0] / adam["guard"][0], adam["recipe"][3] / adam["guard"][3]),
          flush=True)
    del engines, built

"""Cost of dropout (csrc/dropout.hip, DESIGN.md "Dropout") at the metric shape (32,16,64) d=256 L=4, fp32 and bf16.

1. Whole-step time, dropout = 0 against dropout = 0.1, in ONE process on one box: every variant is built INSTANCES times
   (where an engine's buffers land moves its step by more than the effect looked for, tools/ab/recipe_ab.py), rounds
   alternate off on off on, an instance gives the median of its rounds, a variant the median of its instances (min..max).
2. The two fused kernels alone next to the launches they replace, cold: a fill larger than the last-level cache runs
   before every timed launch, HIP events bracket that launch only, algorithmic bytes over the median against 8 TB/s.
    python tools/ab/dropout_ab.py [--p 0.1]"""
import argparse, ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg import hip
from vlg.data import synthetic_clips, to_device
from vlg.engine import LayoutEngine
from vlg.spec import LayoutConfig, SEED

ap = argparse.ArgumentParser()
ap.add_argument("--p", type=float, default=0.1)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--instances", type=int, default=2)
ap.add_argument("--kernel-reps", type=int, default=30)
a = ap.parse_args()
dev = torch.device("cuda:0")
cfg = LayoutConfig(B=32, T=16, N=64, d=256, n_layers=4)


def timed(eng, batch):
    for _ in range(3):
        eng.train_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        eng.train_step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.steps * 1e3


def spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


for precision in ("fp32", "bf16"):
    batch = to_device(synthetic_clips(cfg.B, cfg.T, cfg.N, seed=SEED), dev)
    variants = {"off": {}, "on": dict(dropout=a.p, dropout_seed=SEED)}
    built = [(k, LayoutEngine(cfg, dev, seed=SEED, precision=precision, **kw)) for _ in range(a.instances) for k, kw in variants.items()]
    res = [[] for _ in built]
    for rnd in range(a.rounds):
        for i, (k, eng) in enumerate(built):
            t = timed(eng, batch)
            if rnd:                                   # the first round warms clocks and caches
                res[i].append(t)
    s = {k: spread([spread(r)[0] for (kk, _), r in zip(built, res) if kk == k]) for k in variants}
    within = max(max(r) - min(r) for r in res)
    print("%s step, ms, median (min..max) over %d instances, each the median of %d rounds x %d steps: " % (
        precision, a.instances, a.rounds - 1, a.steps) + "  ".join("%s %.3f (%.3f..%.3f)" % ((k,) + s[k]) for k in variants) +
        "   dropout %g - off %+.1f us (%+.2f %%)   largest min..max inside one instance %.1f us" % (
        a.p, (s["on"][0] - s["off"][0]) * 1e3, (s["on"][0] / s["off"][0] - 1) * 100, within * 1e3), flush=True)
    del built

# ------------------------------------------------------------------------------------------------- the kernels alone
lib = hip.load()
S = torch.cuda.current_stream().cuda_stream
M, d = cfg.tokens, cfg.d
thr, scale = ctypes.c_uint32(), ctypes.c_float()
hip.check(lib.vlg_dropout_plan(a.p, ctypes.byref(thr), ctypes.byref(scale)), "vlg_dropout_plan")
thr, scale = thr.value, scale.value
r = lambda *s: torch.randn(*s, device=dev)
y, resid, x_out, h, dy, dx, dd = (r(M, d) for _ in range(7))
h16, dy16 = h.to(torch.bfloat16), dy.to(torch.bfloat16)
g, b, stats = r(d), r(d), r(2, M).abs() + 0.5
ns = lib.vlg_layernorm_bwd_slabs(M)
slabs = torch.empty(ns * 2 * d, device=dev)
step = torch.zeros(1, dtype=torch.int32, device=dev)
flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)          # 2x the 256 MB last-level cache
P = lambda t: t.data_ptr()
E = float(M) * d
cases = [
    ("layernorm fwd", 8 * E, lambda: hip.call("vlg_layernorm_fwd", P(y), P(g), P(b), P(h), P(stats[0]), P(stats[1]), M, d, 1e-5, S)),
    ("dropout+add+layernorm fwd", 16 * E, lambda: hip.call("vlg_dropout_add_layernorm_fwd", P(y), P(resid), P(g), P(b), P(x_out), P(h),
                                                        P(stats[0]), P(stats[1]), M, d, 1e-5, thr, scale, SEED, 1, P(step), S)),
    ("layernorm fwd ->bf16", 6 * E, lambda: hip.call("vlg_layernorm_fwd_bf16", P(y), P(g), P(b), P(h16), P(stats[0]), P(stats[1]), M, d, 1e-5, S)),
    ("dropout+add+layernorm fwd ->bf16", 14 * E, lambda: hip.call("vlg_dropout_add_layernorm_fwd_bf16", P(y), P(resid), P(g), P(b), P(x_out),
                                                               P(h16), P(stats[0]), P(stats[1]), M, d, 1e-5, thr, scale, SEED, 1, P(step), S)),
    ("layernorm bwd", 16 * E, lambda: hip.call("vlg_layernorm_bwd", P(dy), P(y), P(stats[0]), P(stats[1]), P(g), P(dx), P(dx), P(slabs), 2 * d,
                                            slabs.numel(), M, d, S)),
    ("layernorm bwd + dropout", 20 * E, lambda: hip.call("vlg_layernorm_bwd_dropout", P(dy), P(y), P(stats[0]), P(stats[1]), P(g), P(dx), P(dx),
                                                      P(dd), P(slabs), 2 * d, slabs.numel(), M, d, thr, scale, SEED, 1, P(step), S)),
    ("layernorm bwd bf16 dy", 14 * E, lambda: hip.call("vlg_layernorm_bwd_bf16", P(dy16), P(y), P(stats[0]), P(stats[1]), P(g), P(dx), P(dx),
                                                    P(slabs), 2 * d, slabs.numel(), M, d, S)),
    ("layernorm bwd + dropout bf16 dy", 18 * E, lambda: hip.call("vlg_layernorm_bwd_dropout_bf16", P(dy16), P(y), P(stats[0]), P(stats[1]), P(g),
                                                              P(dx), P(dx), P(dd), P(slabs), 2 * d, slabs.numel(), M, d, thr, scale, SEED, 1,
                                                              P(step), S)),
]
times = {c[0]: [] for c in cases}
for rep in range(a.kernel_reps + 2):
    for name, nbytes, fn in cases:
        dx.normal_()                                   # (the in-place backward would otherwise grow it without bound)
        flush.zero_()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if rep >= 2:
            times[name].append(s.elapsed_time(e) * 1e3)
print("kernels alone at %d rows x %d, cold (a %d MB fill before each), us, median (min..max) of %d:" % (M, d, flush.numel() >> 20, a.kernel_reps))
for name, nbytes, fn in cases:
    med, lo, hi = spread(times[name])
    print("  %-34s %7.1f (%6.1f..%6.1f)  %5.1f MB  %5.0f GB/s = %.2f of 8 TB/s" % (name, med, lo, hi, nbytes / 1e6, nbytes / med * 1e-3,
                                                                               nbytes / med * 1e-3 / 8000), flush=True)

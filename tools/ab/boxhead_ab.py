"""Cost of the Gaussian box head (csrc/box_nll.hip, csrc/decode.hip; DESIGN.md "Gaussian box head") at the metric shape
(32,16,64) d=256 L=4, fp32 and bf16.

  python tools/ab/boxhead_ab.py trees OTHER_TREE [--rounds 3]
      Option OFF, this tree against another checkout built beside it (the parent commit): one process per tree, precision
      and round, alternating; a process gives the median of its timed rounds, a tree the median (min..max) of its
      processes.  Each process also records the entry points one default train_step launches: the two lists must be equal.
  python tools/ab/boxhead_ab.py on
      Option ON against off in this tree, ONE process: engines built INSTANCES times each, rounds alternate off on off on
      (tools/ab/augment_ab.py's scheme); then rollout() ms per generated frame of the Gaussian-head engine at
      box_temperature 0 against 1, alternating; then vlg_layout_box_nll alone, cold (a fill larger than the last-level cache
      before every timed launch), next to vlg_layout_loss at ld = 32 in the same loop.
  python tools/ab/boxhead_ab.py one --tree TREE --precision P      (what `trees` starts: one JSON line)"""
import argparse, json, os, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("trees", "on", "one"))
ap.add_argument("other", nargs="?")
ap.add_argument("--tree", default=HERE)
ap.add_argument("--precision", default="fp32")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--inner", type=int, default=6)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--instances", type=int, default=2)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--kernel-reps", type=int, default=30)
a = ap.parse_args()


def spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


if a.mode == "trees":
    trees = {"this": HERE, "other": os.path.abspath(a.other)}
    got = {(t, p): [] for t in trees for p in ("fp32", "bf16")}
    own = {(t, p): [] for t in trees for p in ("fp32", "bf16")}
    launches = {}
    for rnd in range(a.rounds):
        for t, path in trees.items():
            for p in ("fp32", "bf16"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "one", "--tree", path, "--precision", p, "--inner",
                                    str(a.inner), "--steps", str(a.steps)], stdout=subprocess.PIPE, text=True, timeout=300)
                if r.returncode != 0:
                    sys.exit("a timing process of tree %s ended with status %d" % (t, r.returncode))
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                got[(t, p)].append(rec["median_ms"])
                own[(t, p)] += [rec["min_ms"], rec["max_ms"]]
                launches.setdefault((t, p), rec["launches"])
                print("round %d %s %s: %.3f ms (%.3f..%.3f)" % (rnd, t, p, rec["median_ms"], rec["min_ms"], rec["max_ms"]), flush=True)
    for p in ("fp32", "bf16"):
        s = {t: spread(got[(t, p)]) for t in trees}
        same = launches[("this", p)] == launches[("other", p)]
        diff, width = (s["this"][0] - s["other"][0]) * 1e3, (s["other"][2] - s["other"][1]) * 1e3
        print("%s default step (point head), ms, median (min..max) of %d processes: " % (p, a.rounds) +
              "  ".join("%s %.3f (%.3f..%.3f)" % ((t,) + s[t]) for t in trees) +
              "   this - other %+.1f us (%+.2f %%), the other tree's own spread %.1f us over its processes, %.1f us over every "
              "round: %s   launch lists %s (%d launches)" % (
              diff, (s["this"][0] / s["other"][0] - 1) * 100, width, (max(own[("other", p)]) - min(own[("other", p)])) * 1e3,
              "INSIDE" if abs(diff) <= width else "OUTSIDE the spread of its processes",
              "EQUAL" if same else "DIFFER", len(launches[("this", p)])), flush=True)
    sys.exit(0)

sys.path[:0] = [a.tree, os.path.join(a.tree, "video-layout-generation_amd")]
import torch
from vlg import hip
from vlg.data import synthetic_clips, to_device
from vlg.engine import LayoutEngine
from vlg.spec import LayoutConfig, SEED

dev = torch.device("cuda:0")
SHAPE = dict(B=32, T=16, N=64, d=256, n_layers=4)
cfg = LayoutConfig(**SHAPE)


def timed(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def names_of(fn):
    names = []
    hip.tracer = lambda name, args: names.append(name)
    fn()
    hip.tracer = None
    return names


if a.mode == "one":
    eng = LayoutEngine(cfg, dev, seed=SEED, precision=a.precision)
    batch = to_device(synthetic_clips(cfg.B, cfg.T, cfg.N, seed=SEED), dev)
    names = names_of(lambda: eng.train_step(batch))
    res = [timed(lambda: eng.train_step(batch), a.steps) for _ in range(a.inner)][1:]      # the first round warms clocks and caches
    med, lo, hi = spread(res)
    print(json.dumps({"tree": a.tree, "precision": a.precision, "median_ms": med, "min_ms": lo, "max_ms": hi, "launches": names}))
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ on against off, one process
gauss = LayoutConfig(box_head="gaussian", **SHAPE)
batch = to_device(synthetic_clips(cfg.B, cfg.T, cfg.N, seed=SEED), dev)
for precision in ("fp32", "bf16"):
    variants = {"off": cfg, "on": gauss}
    built = [(k, LayoutEngine(c, dev, seed=SEED, precision=precision)) for _ in range(a.instances) for k, c in variants.items()]
    res = [[] for _ in built]
    for rnd in range(a.inner + 1):
        for i, (k, eng) in enumerate(built):
            t = timed(lambda: eng.train_step(batch), a.steps)
            if rnd:
                res[i].append(t)
    s = {k: spread([spread(r)[0] for (kk, _), r in zip(built, res) if kk == k]) for k in variants}
    n_off, n_on = names_of(lambda: built[0][1].train_step(batch)), names_of(lambda: built[1][1].train_step(batch))
    print("%s step, ms, median (min..max) over %d instances, each the median of %d rounds x %d steps: " % (
        precision, a.instances, a.inner, a.steps) + "  ".join("%s %.3f (%.3f..%.3f)" % ((k,) + s[k]) for k in variants) +
        "   on - off %+.1f us (%+.2f %%)   %d launches off, %d on" % (
        (s["on"][0] - s["off"][0]) * 1e3, (s["on"][0] / s["off"][0] - 1) * 100, len(n_off), len(n_on)), flush=True)
    # rollout of the Gaussian-head engine: mean boxes against drawn ones, alternating
    eng = built[1][1]
    cls, box = batch["slot_class"], batch["slot_box"]
    taus = (0.0, 1.0)
    per = {tau: [] for tau in taus}

    def roll(tau):
        c, b = eng.rollout(cls, box, steps=a.frames, temperature=1.0, seed=SEED, box_temperature=tau)
        return c.cpu(), b.cpu()

    for rnd in range(a.inner + 1):
        for tau in taus:
            t = timed(lambda: roll(tau), 4) / a.frames
            if rnd:
                per[tau].append(t)
    print("%s rollout (Gaussian head, temperature 1), ms per generated frame, median (min..max) of %d rounds: " % (precision, a.inner) +
          "  ".join("box_temperature %g: %.3f (%.3f..%.3f)" % ((tau,) + spread(per[tau])) for tau in taus) +
          "   1 - 0: %+.1f us per frame" % ((spread(per[1.0])[0] - spread(per[0.0])[0]) * 1e3), flush=True)
    del built, eng

# ------------------------------------------------------------------------- the NLL kernel alone, next to the loss kernel
S = torch.cuda.current_stream().cuda_stream
B, T, N, C = cfg.B, cfg.T, cfg.N, cfg.n_classes
M = B * T * N
lib = hip.load()
out = torch.randn(M, 32, device=dev)
dout = torch.empty(M, 32, device=dev)
loss_io = torch.zeros(8, device=dev)
scratch = torch.zeros(lib.vlg_layout_loss_scratch(), device=dev)
nll_scratch = torch.zeros(lib.vlg_layout_box_nll_scratch(), device=dev)
flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)              # 2x the 256 MB last-level cache
cases = [("vlg_layout_loss ld 32", (2.0 * 4 * 24 + 28) * M,
          lambda: hip.call("vlg_layout_loss", out.data_ptr(), 32, batch["tgt_class"].data_ptr(), batch["tgt_box"].data_ptr(),
                           batch["valid"].data_ptr(), dout.data_ptr(), loss_io.data_ptr(), scratch.data_ptr(), B, T, N, C, 0.1, 1e-7,
                           40.0, 20.0, 10.0, S)),
         ("vlg_layout_box_nll ld 32", (52.0 + 32.0) * M,
          lambda: hip.call("vlg_layout_box_nll", out.data_ptr(), 32, batch["tgt_box"].data_ptr(), batch["valid"].data_ptr(),
                           dout.data_ptr(), loss_io.data_ptr(), nll_scratch.data_ptr(), B, T, N, C, -7.0, 0.0, 1.0, S))]
for warm in (False, True):
    times = [[] for _ in cases]
    for rep in range(a.kernel_reps + 2):                                    # one loop: the kernels take turns under the same conditions
        for i, (_, _, launch) in enumerate(cases):
            if not warm:
                flush.zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            launch()
            e.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[i].append(s.elapsed_time(e) * 1e3)
    for (label, nbytes, _), t in zip(cases, times):
        med, lo, hi = spread(t)
        print("(%d,%d,%d) %s, %s, us, median (min..max) of %d: %.1f (%.1f..%.1f)  %.2f MB  %.0f GB/s (launch-bound: not a bandwidth figure)" % (
            B, T, N, label, "warm" if warm else "cold", a.kernel_reps, med, lo, hi, nbytes / 1e6, nbytes / med * 1e-3), flush=True)

"""Cost of the loss options (csrc/loss.hip, DESIGN.md "Loss options"): vlg_layout_loss next to vlg_layout_loss_ext with each
option set, the kernel alone at the metric shape (32,16,64), in ONE process.  tools/kernel_bench.py's method: HIP events
around `iters` back-to-back launches (warm: the 6.9 MB of rows, gradient and targets stay in the last-level cache),
interleaved rounds, the first round dropped; median (min..max) over the rounds, and each variant against the plain entry.
    python tools/ab/loss_ab.py [--rounds 9] [--iters 50]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-layout-generation_amd")]
import torch
from vlg import hip

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--shape", type=int, nargs=3, default=[32, 16, 64])
a = ap.parse_args()
dev = torch.device("cuda:0")
lib = hip.load()
S = torch.cuda.current_stream().cuda_stream
B, T, N = a.shape
M = B * T * N
P = lambda t: t.data_ptr()
out, dout = torch.randn(M, 24, device=dev), torch.empty(M, 24, device=dev)
tcls, tbox = torch.randint(0, 20, (B, T, N), device=dev), torch.rand(B, T, N, 4, device=dev) * 0.5 + 0.25
valid = (torch.rand(B, T, N, device=dev) < 0.9).float()
w = torch.rand(20, device=dev) * 3
scr, lout = torch.zeros(lib.vlg_layout_loss_scratch(), device=dev), torch.zeros(4, device=dev)
tail = (P(dout), P(lout), P(scr), B, T, N, 20, 0.1, 1e-7, 40.0, 20.0, 10.0)


def ext(weights, eps, flags):
    return lambda: hip.call("vlg_layout_loss_ext", P(out), 24, P(tcls), P(tbox), P(valid), hip.ptr(weights), *tail, eps, flags, S)


cases = [("plain entry", lambda: hip.call("vlg_layout_loss", P(out), 24, P(tcls), P(tbox), P(valid), *tail, S)),
         ("ext, options neutral", ext(None, 0.0, 0)), ("weights", ext(w, 0.0, 0)), ("eps = 0.1", ext(None, 0.1, 0)),
         ("giou", ext(None, 0.0, hip.LOSS_GIOU)), ("weights + eps", ext(w, 0.1, 0)), ("weights + eps + giou", ext(w, 0.1, hip.LOSS_GIOU))]
times = {c[0]: [] for c in cases}
for rnd in range(a.rounds + 1):
    for name, fn in cases:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        if rnd:
            times[name].append(s.elapsed_time(e) / a.iters * 1e3)
base = sorted(times["plain entry"])[a.rounds // 2]
print("layout loss alone at (%d,%d,%d), us per launch, median (min..max) of %d rounds x %d launches" % (B, T, N, a.rounds, a.iters))
for name, _ in cases:
    t = sorted(times[name])
    print("  %-22s %6.2f (%6.2f..%6.2f)   %+5.2f us against the plain entry" % (name, t[len(t) // 2], t[0], t[-1], t[len(t) // 2] - base))

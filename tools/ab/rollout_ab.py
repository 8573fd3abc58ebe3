"""A/B of the full-prompt rollout between SOURCE TREES on one box: this checkout against another one - e.g. the parent
commit exported (git archive) and built next to it - where both the library and the Python around it may differ.
    python tools/ab/rollout_ab.py TREE_A TREE_B [--rounds 5] [--steps 8]
One child process per tree and round, alternating A B A B ..., never two at a time; a child imports the package from its
tree, rolls out (32,16,64), d = 256, 4 layers from a full T-frame prompt in fp32 and bf16 and reports ms per generated
frame (host wall-clock around calls that end with the frames on the CPU, as tools/rollout_bench.py measures).  Prints per
tree and precision the median of the rounds with their spread.  A child that fails ends the run: nothing is started after it.
VLG_ATTENTION=clip | factored in the environment rolls out with per-clip / factored attention (default: per-slot)."""
import json
import os
import subprocess
import sys
import time


def child(tree, steps):
    sys.path[:0] = [tree, os.path.join(tree, "video-layout-generation_amd")]
    os.environ.pop("VLG_HIP_LIB", None)                       # each tree loads its own library
    import torch
    from vlg.data import synthetic_clips, to_device
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    B, T, N, d = 32, 16, 64, 256
    dev = torch.device("cuda:0")
    cfg = LayoutConfig(B=B, T=T, N=N, d=d, n_layers=4, attention=os.environ.get("VLG_ATTENTION", "slot"))
    batch = to_device(synthetic_clips(B, T, N, seed=3), dev)
    cls, box = batch["slot_class"], batch["slot_box"]
    out = {}
    for precision in ("fp32", "bf16"):
        eng = LayoutEngine(cfg, dev, precision=precision, padded_slots=False)

        def run():
            c, b = eng.rollout(cls, box, steps=steps)
            return c.cpu(), b.cpu()

        for _ in range(3):
            run()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(4):
                run()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / (4 * steps))
        out[precision] = sorted(ts)[2]
    print("RESULT " + json.dumps(out))


def main():
    args = [a for a in sys.argv[1:]]
    opt = lambda name, default: int(args[args.index(name) + 1]) if name in args else default
    steps, rounds = opt("--steps", 8), opt("--rounds", 5)
    if "--child" in args:
        return child(os.path.abspath(args[args.index("--child") + 1]), steps)
    trees = [os.path.abspath(a) for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] not in ("--steps", "--rounds"))]
    if len(trees) < 2:
        sys.exit(__doc__)
    res = {t: {"fp32": [], "bf16": []} for t in trees}
    for r in range(rounds):
        for t in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", t, "--steps", str(steps)], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True, timeout=300)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit("child for %s failed (exit %d):\n%s" % (t, p.returncode, p.stdout[-2000:]))
            for k, v in json.loads(line[0][7:]).items():
                res[t][k].append(v)
            print("round %d %s %s" % (r, t, line[0][7:]), flush=True)
    for k in ("fp32", "bf16"):
        for t in trees:
            v = sorted(res[t][k])
            print("%-4s %-40s %.3f ms/frame (median of %d rounds; min %.3f max %.3f)" % (k, os.path.relpath(t), v[len(v) // 2], len(v), v[0], v[-1]))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Generates tests/golden/pinned_digests.json: digests of the reference's own GridNet and HNED outputs computed in the
pinned CPU arithmetic of oracle/pinned_cpu.py, for the bit-for-bit restatement tests (tests/test_oracle_golden.py).

Run in the build container only (needs /root/reference):   PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_pinned.py

The inputs and weights are the ones oracle/make_golden.py uses for gridnet_small.npz, gridnet_full64.npz and hned.npz
(stored inputs where the fixture keeps them, else the same seeds; name-seeded test_params weights).  Those fixtures were
made in the build machine's default arithmetic and serve the tolerance-based tests; digests of the pinned outputs let
the exact tests hold on any x86-64 CPU without storing a second copy of the arrays.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pinned_cpu  # noqa: E402

pinned_cpu.apply()        # before MKL's first call

import numpy as np  # noqa: E402
import torch  # noqa: E402

REF = "/root/reference/src"
GOLDEN = os.path.join(ROOT, "tests", "golden")

# fixture -> (filters, seed, input seed or None for the stored input, input shape); as in oracle/make_golden.py
GRIDNET_CASES = {
    "gridnet_small.npz": ((8, 16, 24), 1, None, None),
    "gridnet_full64.npz": ((32, 64, 96), 2, 4, (1, 10, 64, 64)),
}


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import models as ref_models      # noqa: E402
    from oracle import gridnet_spec as G
    from oracle import hned_spec as HS
    out = {"arithmetic": dict(pinned_cpu.ENV, mkldnn="off", torch_threads=1), "sha256": {}}
    for fixture, (filters, seed, xseed, shape) in GRIDNET_CASES.items():
        z = np.load(os.path.join(GOLDEN, fixture))
        x = torch.from_numpy(z["x"]) if xseed is None else torch.randn(shape, generator=torch.Generator().manual_seed(xseed))
        rec = {}
        for tag, linear in (("", False), ("lin_", True)):
            model = ref_models.GridNet(10, filters_level=list(filters))
            model.load_state_dict(G.test_params(G.param_shapes(10, filters), seed=seed, linear=linear))
            seg, img = model(x.clone().requires_grad_(True))
            rec[tag + "seg"], rec[tag + "img"] = pinned_cpu.digest(seg.detach()), pinned_cpu.digest(img.detach())
        out["sha256"][fixture] = rec
    z = np.load(os.path.join(GOLDEN, "hned.npz"))
    hed = ref_models.HNED()
    hed.load_state_dict(HS.test_params(seed=0))
    rec = {}
    for tag in "ab":
        with torch.no_grad():
            outs = hed(torch.from_numpy(z[tag + "_x"]))
        rec[tag + "_out"] = pinned_cpu.digest(torch.stack([o[:, 0] for o in outs]))
    out["sha256"]["hned.npz"] = rec
    with open(os.path.join(GOLDEN, "pinned_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote pinned_digests.json")


if __name__ == "__main__":
    main()

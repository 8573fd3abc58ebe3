"""TEST INFRASTRUCTURE ONLY - the CPU arithmetic the bit-for-bit golden fixtures are made and checked with.

torch's CPU convolutions give different bits on different machines: oneDNN picks kernels and blockings by ISA, cache
sizes and thread count, and MKL's sgemm takes a different code path on a CPU of another vendor or generation.  Pinned:
oneDNN off (ATen's im2col + MKL sgemm), one thread, and MKL in its conditional numerical reproducibility mode
(MKL_CBWR=COMPATIBLE: the same results on any x86-64 CPU).  MKL reads MKL_CBWR once, on its first call, so apply()
must run before anything touches MKL - in practice before `import torch` in a fresh interpreter.  The outputs are
stored as digest()s (tests/golden/pinned_digests.json, oracle/make_golden_pinned.py).
"""
import os

ENV = {"MKL_CBWR": "COMPATIBLE", "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}


def apply():
    os.environ.update(ENV)
    import torch
    torch.set_num_threads(1)
    torch.backends.mkldnn.enabled = False


def digest(a) -> str:
    """sha256 of an array's float32 bytes (C order): equal digests <=> bit-identical arrays."""
    import hashlib
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()

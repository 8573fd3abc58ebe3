"""GPU: the head's three products at N = 32 - the Gaussian box head's n_out (20 logits + 4 means + 4 scales + 4 of padding)
where the point head has 24 - in the three precision families, with the operand storage the step hands them, against fp64.

The runners, guards and bars are test_hip_gemm_paths.py's (run_fwd / run_dgrad / run_wgrad: rtol 1e-4 / atol 1e-5, BF_OUT for
bf16 outputs, the weight gradient scaled by sqrt(M), native fp32 also within 4x torch-CPU fp32's error): nothing new."""
import pytest

from test_hip_gemm_paths import (EPI_B_BF16, EPI_BF16, EPI_BIAS, EPI_NONE, EPI_SPLIT3, IO3, IO6, H, run_dgrad, run_fwd,  # noqa: F401
                                 run_wgrad)

pytestmark = pytest.mark.gpu

N, K = 32, 64
ROWS = (276, 4100)             # (B,T,N) = (3,4,23) tokens; and more than one row tile of every kernel, not a multiple of any
# per call: native fp32, fp32x3, bf16 - as LayoutEngine launches the head (forward: bf16 xf and weight shadow, fp32 out; data
# gradient: fp32 dout, bf16 weights and dh; weight gradient: fp32 dout, bf16 xf)
FLAGS = {"fwd": (EPI_BIAS, EPI_SPLIT3 | EPI_BIAS, EPI_BF16 | IO3 | EPI_BIAS),
         "dgrad": (EPI_NONE, EPI_SPLIT3, EPI_BF16 | IO6),
         "wgrad": (0, EPI_SPLIT3, EPI_BF16 | EPI_B_BF16)}
RUN = {"fwd": run_fwd, "dgrad": run_dgrad, "wgrad": run_wgrad}


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("precision", [0, 1, 2], ids=["fp32", "fp32x3", "bf16"])
@pytest.mark.parametrize("call", ["fwd", "dgrad", "wgrad"])
def test_head_product_at_n32(H, dev, call, precision, M):
    RUN[call](H, dev, M, N, K, FLAGS[call][precision])

"""Former home of the guarded optimiser step; it lives in vlg/optim.py with the rest of the optimiser."""
from .optim import (APPLY, CLIP_COEF, CTL_FLOATS, GRAD_MULT, GRAD_NORM, LR, SKIPPED, SQRT_BC2, STEP, STEP_SIZE,  # noqa: F401
                    OptimControl, decayed_lr)

"""ctypes binding of libvlg_hip.so (C ABI declared in include/vlg_hip.h).

There is deliberately NO fallback: if the shared library is missing or a kernel
launch reports an error this module raises.  The product path never computes on
the CPU and never imports anything from oracle/.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# VLG_HIP_LIB: development override (A/B runs of two builds in one gpurun call, tools/kernel_bench.py); still no fallback
LIB_PATH = os.environ.get("VLG_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "libvlg_hip.so")

EPI_NONE, EPI_BIAS, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_BF16 = 0, 1, 2, 4, 8, 16
EPI_A_BF16, EPI_B_BF16, EPI_OUT_BF16, EPI_SPLIT3 = 32, 64, 128, 256      # bf16 activation storage (include/vlg_hip.h)
EPI_ACT_GELU = 512                                                       # activation operand = gelu(stored), applied on load
EPI_GELU_GRAD, EPI_MUL = 1024, 2048                                      # aux_out = gelu'(pre);  dgrad: C = acc * aux_in

P, I, L, F = c_void_p, c_int, c_int64, c_float

# name -> (restype, argtypes); must list every symbol include/vlg_hip.h declares
SIGNATURES = {
    "vlg_abi_version": (I, []),
    "vlg_build_arch": (c_char_p, []),
    "vlg_embed_fwd": (I, [P, P, P, P, P, P, P, I, I, I, I, I, P]),
    "vlg_embed_bwd_slabs": (I, []),
    "vlg_embed_bwd_slabs_for": (I, [I, I, I, I, I]),
    "vlg_embed_bwd": (I, [P, P, P, P, L, L, I, I, I, I, I, P]),
    "vlg_layernorm_fwd": (I, [P, P, P, P, P, P, L, I, F, P]),
    "vlg_layernorm_fwd_bf16": (I, [P, P, P, P, P, P, L, I, F, P]),
    "vlg_layernorm_bwd_slabs": (I, [L]),
    "vlg_layernorm_bwd": (I, [P, P, P, P, P, P, P, P, L, L, L, I, P]),
    "vlg_layernorm_bwd_bf16": (I, [P, P, P, P, P, P, P, P, L, L, L, I, P]),
    "vlg_dropout_plan": (I, [c_double, P, P]),                   # host only: (p, uint32* thr, float* scale)
    "vlg_dropout_add_layernorm_fwd": (I, [P, P, P, P, P, P, P, P, L, I, F, c_uint32, F, c_uint64, I, P, P]),
    "vlg_dropout_add_layernorm_fwd_bf16": (I, [P, P, P, P, P, P, P, P, L, I, F, c_uint32, F, c_uint64, I, P, P]),
    "vlg_layernorm_bwd_dropout": (I, [P, P, P, P, P, P, P, P, P, L, L, L, I, c_uint32, F, c_uint64, I, P, P]),
    "vlg_layernorm_bwd_dropout_bf16": (I, [P, P, P, P, P, P, P, P, P, L, L, L, I, c_uint32, F, c_uint64, I, P, P]),
    "vlg_dropout_step_advance": (I, [P, P]),
    "vlg_linear_fwd": (I, [P, I, P, I, P, P, I, P, P, L, I, I, I, P]),
    "vlg_linear_dgrad": (I, [P, I, P, I, P, I, P, L, I, I, I, P]),
    "vlg_linear_wgrad_slabs": (I, [L, I, I]),
    "vlg_linear_dgrad_wgrad": (I, [P, I, P, I, P, I, P, P, I, P, L, L, L, I, I, I, P, I, P]),
    "vlg_linear_wgrad_slabs_for": (I, [L, I, I, I]),
    "vlg_linear_wgrad": (I, [P, I, P, I, P, L, L, L, I, I, I, P]),
    "vlg_linear_plan": (I, [I, L, I, I, I, I, I, I, I, P]),      # host-side planner; fills a vlg_gemm_plan
    "vlg_attention_fwd": (I, [P, P, L, I, I, P]),
    "vlg_attention_bwd": (I, [P, P, P, L, I, I, P]),
    "vlg_attention_fwd_bf16": (I, [P, P, L, I, I, P]),
    "vlg_attention_bwd_bf16": (I, [P, P, P, L, I, I, P]),
    "vlg_attention_step": (I, [P, P, L, I, I, I, L, P]),           # (qkv, o, n_seq, T, d, p, ldo, stream)
    "vlg_attention_step_bf16": (I, [P, P, L, I, I, I, L, P]),
    "vlg_attention_clip_fwd": (I, [P, P, P, P, L, I, I, I, P]),
    "vlg_attention_clip_bwd": (I, [P, P, P, P, P, P, P, L, I, I, I, P]),
    "vlg_attention_clip_fwd_bf16": (I, [P, P, P, P, L, I, I, I, P]),
    "vlg_attention_clip_bwd_bf16": (I, [P, P, P, P, P, P, P, L, I, I, I, P]),
    "vlg_attention_clip_step": (I, [P, P, P, L, I, I, I, I, L, P]),      # (qkv, valid, o, B, T, N, d, p, ldo, stream)
    "vlg_attention_clip_step_bf16": (I, [P, P, P, L, I, I, I, I, L, P]),
    "vlg_attention_frame_fwd": (I, [P, P, P, P, L, I, I, I, P]),         # attention inside a frame: the per-clip argument lists
    "vlg_attention_frame_bwd": (I, [P, P, P, P, P, P, P, L, I, I, I, P]),
    "vlg_attention_frame_fwd_bf16": (I, [P, P, P, P, L, I, I, I, P]),
    "vlg_attention_frame_bwd_bf16": (I, [P, P, P, P, P, P, P, L, I, I, I, P]),
    "vlg_attention_frame_step": (I, [P, P, P, L, I, I, I, I, L, P]),
    "vlg_attention_frame_step_bf16": (I, [P, P, P, L, I, I, I, I, L, P]),
    "vlg_layout_loss_scratch": (I, []),
    "vlg_layout_loss": (I, [P, I, P, P, P, P, P, P, I, I, I, I, F, F, F, F, F, P]),
    # (out, ld, tgt_class, tgt_box, valid, class_weight | NULL, dout, loss_out, scratch, B, T, N, C, beta, iou_eps, 3 weights, eps, flags, stream)
    "vlg_layout_loss_ext": (I, [P, I, P, P, P, P, P, P, P, I, I, I, I, F, F, F, F, F, F, I, P]),
    "vlg_layout_box_nll_scratch": (I, []),
    # (out, ld, tgt_box, valid, dout, loss_io, scratch, B, T, N, C, s_min, s_max, w_nll, stream)
    "vlg_layout_box_nll": (I, [P, I, P, P, P, P, P, I, I, I, I, F, F, F, P]),
    # the plain decode entries + ld after out_last and box_temperature after top_k
    "vlg_layout_decode_ext": (I, [P, I, P, P, P, P, P, P, P, I, I, I, I, I, I, F, I, F, c_uint64, I, P]),
    "vlg_layout_decode_append_ext": (I, [P, I, P, P, P, P, P, P, P, I, I, I, I, I, I, I, F, I, F, c_uint64, I, P]),
    "vlg_head_last_frame": (I, [P, P, P, P, P, P, I, I, I, I, I, F, P]),
    "vlg_head_frame": (I, [P, P, P, P, P, P, I, I, I, I, I, I, F, P]),
    "vlg_layout_decode": (I, [P, P, P, P, P, P, P, P, I, I, I, I, I, I, F, I, c_uint64, I, P]),
    "vlg_layout_decode_append": (I, [P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, F, I, c_uint64, I, P]),
    "vlg_sched_plan": (I, [c_double, P]),                        # host only: (eps_max, uint32* thr_max)
    # (out, ld, cls, box, mix_cls, mix_box, step, B, T, N, C, thr_max, ramp_steps, temperature, top_k, seed, stream)
    "vlg_layout_mix_inputs": (I, [P, I, P, P, P, P, P, I, I, I, I, c_uint32, I, F, I, c_uint64, P]),
    "vlg_augment_plan": (I, [c_double, P]),                      # host only: (p, uint32* thr)
    # (cls, box, tgt_box, valid, aug_cls, aug_box, aug_tgt_box, aug_valid, step, B, T, N, C, thr_flip, thr_drop, zoom, shift, jitter, seed, stream)
    "vlg_layout_augment": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, c_uint32, c_uint32, F, F, F, c_uint64, P]),
    "vlg_layout_metrics_counts": (I, [I]),
    "vlg_layout_metrics_sums": (I, [I]),
    "vlg_layout_metrics_scratch": (I, []),
    "vlg_layout_metrics": (I, [P, I, P, P, P, I, I, P, P, P, I, I, I, I, I, F, F, P]),
    "vlg_layout_rasterize": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P]),
    "vlg_label_confusion": (I, [P, P, P, I, I, L, I, I, P]),
    "vlg_reduce_slabs": (I, [P, L, I, P, L, P]),
    "vlg_reduce_slabs_table": (I, [P, I, I, P]),
    "vlg_sum_partials_table": (I, [P, I, P]),
    "vlg_adam_step": (I, [P, P, P, P, L, I, F, F, F, F, F, P]),
    "vlg_adam_step_graph": (I, [P, P, P, P, P, L, P, I, F, F, F, F, F, P]),
    "vlg_adam_step_bf16": (I, [P, P, P, P, P, L, I, F, F, F, F, F, P]),
    "vlg_grad_sumsq_blocks": (I, [L]),
    "vlg_grad_sumsq": (I, [P, L, P, P]),
    "vlg_optim_control": (I, [P, P, I, F, F, F, F, P]),
    "vlg_adam_step_ctl": (I, [P, P, P, P, P, L, P, F, F, F, P]),
    "vlg_optim_control_ext": (I, [P, P, P, I, F, F, F, F, P]),
    "vlg_adamw_ema_step_ctl": (I, [P, P, P, P, P, P, P, P, L, P, P, F, F, F, P]),
    "vlg_image_loss_scratch": (I, []),
    "vlg_ce_nchw": (I, [P, P, P, P, P, I, I, L, F, P]),
    "vlg_l1_mean": (I, [P, P, P, P, P, L, F, P]),
    "vlg_gradient_loss": (I, [P, P, P, P, P, I, I, I, F, P]),
    "vlg_ssim_loss": (I, [P, P, P, P, P, I, I, I, I, F, P]),
    "vlg_affine_nchw": (I, [P, P, I, I, L, P, P, P]),
    "vlg_prep_input": (I, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, P]),
    "vlg_argmax_nchw": (I, [P, P, I, I, L, P]),
    "vlg_rollout_input": (I, [P, P, P, P, P, P, P, I, L, P]),
    "vlg_conv3x3_fwd": (I, [P, P, P, P, P, P, P, P, L, I, I, I, I, I, I, P, L, P]),
    "vlg_conv3x3_fwd_splits": (I, [L, I, I, I]),
    "vlg_conv3x3_fwd_workspace": (L, [L, I, I, I]),
    "vlg_conv3x3_dgrad_slabs": (I, [L, I]),
    "vlg_conv3x3_dgrad": (I, [P, P, P, P, P, P, P, P, L, L, I, I, I, I, I, P, L, I, P]),
    "vlg_conv3x3_dgrad_splits": (I, [L, I, I]),
    "vlg_conv3x3_dgrad_workspace": (L, [L, I, I]),
    "vlg_conv3x3_wgrad_slabs": (I, [L, I, I]),
    "vlg_conv3x3_wgrad": (I, [P, P, P, L, L, P, P, L, I, I, I, I, P]),
    "vlg_conv3x3_fwd_bf16": (I, [P, P, P, P, P, P, P, P, L, I, I, I, I, I, I, P, L, P]),
    "vlg_conv3x3_fwd_bf16_splits": (I, [L, I, I, I]),
    "vlg_conv3x3_fwd_bf16_workspace": (L, [L, I, I, I]),
    "vlg_conv3x3_dgrad_bf16_slabs": (I, [L, I]),
    "vlg_conv3x3_dgrad_bf16": (I, [P, P, P, P, P, P, P, P, L, L, I, I, I, I, I, P, L, I, P]),
    "vlg_conv3x3_dgrad_bf16_splits": (I, [L, I, I]),
    "vlg_conv3x3_dgrad_bf16_workspace": (L, [L, I, I]),
    "vlg_conv3x3_wgrad_bf16_slabs": (I, [L, I, I]),
    "vlg_conv3x3_wgrad_bf16": (I, [P, P, P, L, L, P, P, L, I, I, I, I, P]),
    "vlg_nchw_to_padded": (I, [P, P, I, I, I, I, I, I, P]),
    "vlg_padded_to_nchw": (I, [P, P, I, I, I, I, I, P]),
    "vlg_fill_coords": (I, [P, I, I, I, I, I, P]),
    "vlg_upsample2x_fwd": (I, [P, P, I, I, I, I, P]),
    "vlg_upsample2x_bwd": (I, [P, P, I, I, I, I, I, P]),
    "vlg_maxpool2x2": (I, [P, P, I, I, I, I, P]),
    "vlg_score1x1_relu": (I, [P, P, P, P, I, I, I, I, I, P]),
    "vlg_hed_head": (I, [P, P, P, P, P, P, P, P, I, I, I, P]),
    "vlg_maxpool2x2_bwd": (I, [P, P, P, I, I, I, I, P]),
    "vlg_l1_relu_padded": (I, [P, P, P, P, P, L, I, L, F, P]),
    "vlg_add_rows": (I, [P, P, L, I, P]),
    "vlg_sum_partials": (I, [P, I, P, I, P]),
}
# entry points of the DIAGNOSTIC build only (make -C csrc diag; VLG_HIP_LIB=.../libvlg_hip_diag.so): typed when present
DIAG_SIGNATURES = {
    "vlg_debug_set_clock_probe": (None, [P]),
    "vlg_debug_set_conv_probe": (None, [P]),
    "vlg_debug_set_gemm_bk": (None, [I]),
    "vlg_debug_set_gemm_run": (None, [I]),
}
LOSS_GIOU = 1                          # vlg_layout_loss_ext flags (VLG_LOSS_GIOU)
LABEL_U8, LABEL_I64, LABEL_F32 = 0, 1, 2   # vlg_layout_rasterize out_kind (VLG_LABEL_*)
RASTER_CLASS, RASTER_SLOT = 0, 1           # ... and what (VLG_RASTER_*)
CEPI_BIAS, CEPI_RESID, CEPI_PRELU, CEPI_DPRELU, CEPI_ACCUM, CEPI_CIN4 = 1, 2, 4, 8, 16, 32
CONV_PRECISIONS = ("fp32", "bf16")     # 3x3 convolutions: fp32 MFMA (conv.hip) or bf16-operand MFMA (conv_bf16.hip)


def conv_sym(name: str, precision: str) -> str:
    """Entry point / planner query of a 3x3 convolution in `precision`: vlg_conv3x3_fwd -> vlg_conv3x3_fwd_bf16,
    vlg_conv3x3_fwd_workspace -> vlg_conv3x3_fwd_bf16_workspace."""
    if precision not in CONV_PRECISIONS:
        raise ValueError("conv precision must be one of %s, not %r" % (CONV_PRECISIONS, precision))
    if precision == "fp32":
        return name
    op = name.split("_")[2]                     # fwd | dgrad | wgrad
    pre = "vlg_conv3x3_" + op
    return pre + "_bf16" + name[len(pre):]

_lib = None


class HipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """dlopen libvlg_hip.so and type every entry point; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipError(
            "libvlg_hip.so not found at %s - run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C video-layout-generation_amd/csrc`); there is no CPU fallback" % LIB_PATH)
    # PyTorch-ROCm ships its own libamdhip64.so; it must be in the process BEFORE libvlg_hip.so is dlopen'ed so that both
    # bind to ONE HIP runtime (torch streams and device pointers are handed to the kernels).  Loaded the other way
    # round the library pulls /opt/rocm's runtime first and every launch fails with hipErrorNoDevice.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in DIAG_SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def require_diag() -> ctypes.CDLL:
    """Development tools only: the diagnostic build of the library (vlg_debug_set_* switches)."""
    lib = load()
    if not hasattr(lib, "vlg_debug_set_clock_probe"):
        raise HipError("this tool needs the diagnostic build: `make -C video-layout-generation_amd/csrc diag` and run with "
                       "VLG_HIP_LIB=<repo>/video-layout-generation_amd/libvlg_hip_diag.so (the product library has no debug switches)")
    return lib


_ERR = {1001: "VLG_ERR_SHAPE (unsupported or inconsistent shape)", 1002: "VLG_ERR_ALIGN (pointer / leading dimension not 16-byte aligned)"}


def check(code: int, what: str) -> None:
    if code != 0:
        raise HipError("%s failed: %s" % (what, _ERR.get(code, "hipError_t %d" % code)))


def ptr(t) -> int:
    """Device pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


tracer = None     # optional callable(name, args) -> context manager | None: measurement hook (bench.py brackets launches with events)


def call(name: str, *args) -> None:
    cm = tracer(name, args) if tracer is not None else None
    if cm is None:
        check(getattr(load(), name)(*args), name)
        return
    with cm:
        check(getattr(load(), name)(*args), name)

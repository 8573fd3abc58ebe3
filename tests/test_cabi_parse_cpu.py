"""CPU: vlg.cabi, the strict reader of include/vlg_hip.h that the ctypes binding, the parameter positions and every Python
constant are derived from.  Inline snippets pin the grammar (each accepted form's exact result, each refusal); the real
header is checked prototype by prototype, against a hand-written sample of ctypes lists that between them use every type,
and against the argument positions the tests used to hard-code (the one place those numbers remain)."""
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_uint64, c_void_p

import pytest

from conftest import PKG
from vlg import cabi, hip

P, I, L = c_void_p, c_int, c_int64
F, D, U32, U64 = c_float, c_double, c_uint32, c_uint64
HDR = cabi.header()


# ------------------------------------------------------------------------------------------------ inline snippets
def test_accepted_forms_parse_to_exactly_this():
    h = cabi.parse("""
        /* a comment with int f(long); and #if inside */
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        typedef uint16_t vlg_bf16;
        typedef struct vlg_plan { int a; int64_t b[2]; } vlg_plan;
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define VLG_A 3
        #define VLG_NEG -2   /* trailing comment */
        #define VLG_S_MIN (-7.0f)
        #define VLG_S_MAX (0.0f)
        enum vlg_kind { VLG_K0 = 0, VLG_K5 = 5 };
        int         vlg_version(void);
        const char* vlg_arch(void);
        const char *vlg_arch2(void);
        int64_t vlg_size(int64_t rows, int d);
        void vlg_all(const float* x, vlg_bf16* y, const vlg_plan* plan, const uint8_t *mask, unsigned long long* ticks,
                     int i, int64_t l, uint32_t u, uint64_t s, float f /* inline */, double p, void* stream);
        #ifdef VLG_DIAG
        void vlg_debug_set_x(int bk);
        #endif
        #ifdef __cplusplus
        }
        #endif
        #endif /* X_H */
    """)
    assert h.functions == {
        "vlg_version": (c_int, ()),
        "vlg_arch": (c_char_p, ()),
        "vlg_arch2": (c_char_p, ()),
        "vlg_size": (c_int64, ((c_int64, "rows"), (c_int, "d"))),
        "vlg_all": (None, ((P, "x"), (P, "y"), (P, "plan"), (P, "mask"), (P, "ticks"), (c_int, "i"), (c_int64, "l"),
                           (c_uint32, "u"), (c_uint64, "s"), (c_float, "f"), (c_double, "p"), (P, "stream"))),
    }
    assert h.diag_functions == {"vlg_debug_set_x": (None, ((c_int, "bk"),))}
    assert h.constants == {"VLG_A": 3, "VLG_NEG": -2, "VLG_S_MIN": -7.0, "VLG_S_MAX": 0.0}
    assert [type(h.constants[k]) for k in ("VLG_A", "VLG_S_MAX")] == [int, float]
    assert h.enums == {"vlg_kind": {"VLG_K0": 0, "VLG_K5": 5}}


REFUSED = {
    "unnamed scalar parameter": "int f(int);",
    "unnamed pointer parameter": "int f(int n, const float*);",
    "long": "int f(long n);",
    "unsigned": "int f(unsigned n);",
    "unsigned int": "int f(unsigned int n);",
    "size_t": "int f(size_t n);",
    "long return": "long f(int n);",
    "pointer return": "float* f(int n);",
    "struct by value": "typedef struct s { int a; } s_t;\nint f(s_t plan);",
    "struct keyword by value": "int f(struct s plan);",
    "typedef by value": "typedef uint16_t vlg_bf16;\nint f(vlg_bf16 x);",
    "pointer to an undeclared type": "int f(hipStream_t* s);",
    "array parameter": "int f(int n[4]);",
    "function pointer": "int f(int (*cb)(int), void* stream);",
    "variadic": "int f(const char* fmt, ...);",
    "function-like macro": "#define VLG_MAX(a, b) 3",
    "define of an expression": "#define VLG_X 1 + 2",
    "define of a shift": "#define VLG_X (1 << 3)",
    "define of a name": "#define VLG_X VLG_Y",
    "define without a value": "#define VLG_X",
    "define of an unsuffixed float": "#define VLG_X (1.5)",
    "#if with an expression": "#if VLG_X > 1\nint f(int n);\n#endif",
    "#elif": "#ifdef VLG_DIAG\n#elif VLG_X\n#endif",
    "#else": "#ifdef VLG_DIAG\n#else\n#endif",
    "#ifdef of another name": "#ifdef VLG_OTHER\n#endif",
    "#include of another file": "#include <stdio.h>",
    "#endif without #if": "#endif",
    "unterminated #ifdef": "#ifdef VLG_DIAG\nint f(int n);",
    "enum member without a value": "enum e { VLG_A = 0, VLG_B };",
    "enum member of an expression": "enum e { VLG_A = 1 << 2 };",
    "stream not last": "int f(void* stream, int n);",
    "function declared twice": "int f(int n);\nint f(int n);",
    "function declared twice, once under VLG_DIAG": "int f(int n);\n#ifdef VLG_DIAG\nint f(int n);\n#endif",
    "constant declared twice": "#define VLG_X 1\n#define VLG_X 1",
    "// comment": "int f(int n);   // no",
    "a definition": "int f(int n) { return n; }",
    "a declaration without its semicolon": "int f(int n)",
    "a global": "int vlg_state;",
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_forms_raise_value_error_naming_the_text(what):
    with pytest.raises(ValueError, match="vlg_hip.h grammar"):
        cabi.parse(REFUSED[what])


def test_typedefs_only_make_pointer_targets():
    src = "typedef struct p { int a; } plan_t;\ntypedef uint16_t half_t;\nint f(plan_t* plan, const half_t* x);"
    assert cabi.parse(src).functions == {"f": (c_int, ((P, "plan"), (P, "x")))}
    with pytest.raises(ValueError):
        cabi.parse("typedef unknown_t half_t;")


# ------------------------------------------------------------------------------------------------ the real header
def test_every_prototype_of_the_header_is_regular():
    assert len(HDR.functions) == len(hip.SIGNATURES) >= 114 and len(HDR.diag_functions) == len(hip.DIAG_SIGNATURES)
    assert not set(HDR.functions) & set(HDR.diag_functions)
    assert sorted(HDR.diag_functions) == ["vlg_debug_set_clock_probe", "vlg_debug_set_conv_probe", "vlg_debug_set_gemm_bk",
                                          "vlg_debug_set_gemm_run"]
    scalars = (c_int, c_int64, c_uint32, c_uint64, c_float, c_double)
    for name, (res, params) in {**HDR.functions, **HDR.diag_functions}.items():
        assert res in (c_int, c_int64, None, c_char_p), name
        names = [n for _, n in params]
        assert "stream" not in names[:-1] and len(set(names)) == len(names), name
        assert all(t is P or t in scalars for t, _ in params), name
        assert hip.PARAMS[name] == tuple(names)
        assert (hip.SIGNATURES.get(name) or hip.DIAG_SIGNATURES[name]) == (res, [t for t, _ in params])
    assert all(res is None for res, _ in HDR.diag_functions.values())


SAMPLE = {      # typed by hand from include/vlg_hip.h; between them: every restype and every scalar type
    "vlg_build_arch": (c_char_p, []),
    "vlg_dropout_plan": (I, [D, P, P]),
    "vlg_dropout_add_layernorm_fwd": (I, [P, P, P, P, P, P, P, P, L, I, F, U32, F, U64, I, P, P]),
    "vlg_conv3x3_fwd_workspace": (L, [L, I, I, I]),
    "vlg_linear_plan": (I, [I, L, I, I, I, I, I, I, I, P]),
    "vlg_layout_augment": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, U32, U32, F, F, F, U64, P]),
    "vlg_adamw_ema_step_ctl": (I, [P, P, P, P, P, P, P, P, L, P, P, F, F, F, P]),
    "vlg_debug_set_gemm_bk": (None, [I]),
}


@pytest.mark.parametrize("name", sorted(SAMPLE))
def test_sample_of_signatures_typed_by_hand(name):
    assert {**hip.SIGNATURES, **hip.DIAG_SIGNATURES}[name] == SAMPLE[name]


POSITIONS = {   # the positions the tests' tables held before they looked parameters up by name
    "vlg_linear_fwd": dict(epilogue=12),
    "vlg_linear_dgrad": dict(epilogue=10),
    "vlg_linear_wgrad": dict(slabs=4, slab_stride=5, flags=10),
    "vlg_linear_dgrad_wgrad": dict(epilogue=15),
    "vlg_layout_loss_ext": dict(label_smoothing=18, flags=19),
    "vlg_layout_box_nll": dict(s_min=11, s_max=12, w_nll=13),
    "vlg_layout_mix_inputs": dict(thr_max=11, ramp_steps=12, temperature=13, top_k=14, seed=15),
    "vlg_layout_augment": dict(thr_flip=13, thr_drop=14, zoom=15, shift=16, jitter=17, seed=18),
    "vlg_conv3x3_fwd": dict(epilogue=14),
    "vlg_conv3x3_fwd_bf16": dict(epilogue=14),
    "vlg_conv3x3_dgrad": dict(epilogue=14),
    "vlg_conv3x3_dgrad_bf16": dict(epilogue=14),
    "vlg_conv3x3_wgrad": dict(slabs=2, slab_stride=3),
    "vlg_conv3x3_wgrad_bf16": dict(slabs=2, slab_stride=3),
    "vlg_upsample2x_bwd": dict(accumulate=6),
    "vlg_add_rows": dict(accumulate=3),
    "vlg_prep_input": dict(flip=14),
    "vlg_adamw_ema_step_ctl": dict(ema=5, ema_shadow=6, decay_mask=7),
    "vlg_dropout_add_layernorm_fwd": dict(thr=11, scale=12, seed=13, site=14),
    "vlg_layernorm_bwd_dropout": dict(thr=13, scale=14, seed=15, site=16),
}


@pytest.mark.parametrize("name", sorted(POSITIONS))
def test_param_index_returns_the_positions_the_tests_relied_on(name):
    assert {p: hip.param_index(name, p) for p in POSITIONS[name]} == POSITIONS[name]


def test_param_index_refuses_unknown_names():
    with pytest.raises(KeyError):
        hip.param_index("vlg_linear_fwd", "flags")            # its flags word is called `epilogue`
    with pytest.raises(KeyError):
        hip.param_index("vlg_no_such_entry", "stream")


def test_constants_are_the_headers():
    from vlg import metrics, optim, spec
    C = HDR.constants
    assert all(type(v) in (int, float) for v in C.values())
    assert optim.CTL_FLOATS == optim.EXT_FLOATS == 16
    epi = [C[k] for k in C if k.startswith("VLG_EPI_") and k != "VLG_EPI_NONE"]
    assert len(epi) == 12 and len(set(epi)) == 12 and all(v > 0 and v & (v - 1) == 0 for v in epi) and hip.EPI_NONE == 0
    assert {getattr(hip, k[4:]) for k in C if k.startswith("VLG_EPI_")} == set(epi) | {0}      # every EPI bit is bound
    cepi = [C[k] for k in C if k.startswith("VLG_CEPI_")]
    assert len(set(cepi)) == 6 and all(v & (v - 1) == 0 for v in cepi)
    assert (hip.CALL_FWD, hip.CALL_DGRAD, hip.CALL_WGRAD, hip.CALL_PAIR) == (0, 1, 2, 3)
    assert cabi.values("VLG_MET_", "CONF", "IOU_BY_CLASS") == (8, 4)
    assert sorted(hip._ERR) == [C["VLG_ERR_SHAPE"], C["VLG_ERR_ALIGN"]] == [1001, 1002]
    assert (spec.BOX_S_MIN, spec.BOX_S_MAX) == (-7.0, 0.0) and type(spec.BOX_S_MAX) is float
    ctl = [optim.STEP_SIZE, optim.SQRT_BC2, optim.STEP, optim.APPLY, optim.GRAD_MULT, optim.GRAD_NORM, optim.LR, optim.SKIPPED,
           optim.CLIP_COEF]
    ext = [optim.EXT_WEIGHT_DECAY, optim.EXT_WARMUP_STEPS, optim.EXT_EMA_DECAY, optim.EXT_EMA_WARMUP, optim.EXT_LR_EFF,
           optim.EXT_DECAY_MULT, optim.EXT_EMA_OMD]
    assert len(set(ctl)) == 9 and max(ctl) < optim.CTL_FLOATS and len(set(ext)) == 7 and max(ext) < optim.EXT_FLOATS
    counts = [metrics.SCORED, metrics.TOP1, metrics.TOPK, metrics.IOU_HIT, metrics.BOTH_HIT, metrics.NONFINITE, metrics.UNSCORED]
    sums = [metrics.NLL, metrics.IOU, metrics.BOX_L1]
    assert len(set(counts)) == 7 and max(counts) < metrics.CONF and len(set(sums)) == 3 and max(sums) < metrics.IOU_BY_CLASS
    assert HDR.enums["vlg_rng_stream"]["VLG_RNG_BOX_NORMAL"] == 5


def test_a_missing_header_is_a_hip_error(tmp_path):
    """No fallback table: without include/vlg_hip.h, importing the binding raises HipError, as a missing library does.
    In a fresh interpreter (no torch: tens of milliseconds), so that this process's binding is never half-imported."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from vlg import cabi\n"
            "cabi.HEADER_PATH = %r; cabi.header.cache_clear()\n"
            "try:\n    import vlg.hip\nexcept Exception as e:\n    print(type(e).__name__, e)\n" % (PKG, str(tmp_path / "vlg_hip.h")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("HipError include/vlg_hip.h not found"), out.stdout + out.stderr

"""CPU: the planner queries of the bf16-MFMA convolutions (vlg_conv3x3_*_bf16_*, csrc/conv.hip) are host code -
callable without a GPU - and the entry points check the capacities the caller passes against exactly those queries,
refusing one float (one partial, one slab) less with VLG_ERR_SHAPE before anything is launched.  (That the queried
amounts themselves are accepted is a launch: tests/test_hip_conv_bf16.py.)"""
import ctypes

import pytest

VLG_ERR_SHAPE, VLG_ERR_ALIGN = 1001, 1002
# stand-in device pointers: 16-byte aligned, never dereferenced - every call below is refused on the host
FAKE = 1 << 40


def _lib():
    from vlg import hip
    return hip.load()


def _rows(b, H, W):
    return b * (H + 2) * (W + 2)


@pytest.mark.parametrize("b,H,W,cin_p,cout_p", [(1, 16, 16, 128, 128), (2, 8, 8, 256, 256), (1, 16, 16, 128, 256),
                                               (1, 8, 8, 512, 512), (4, 32, 32, 512, 512), (4, 64, 64, 256, 256)])
def test_split_k_workspace_is_exact(b, H, W, cin_p, cout_p):
    lib = _lib()
    rows = _rows(b, H, W)
    sp = lib.vlg_conv3x3_fwd_bf16_splits(rows, cin_p, cout_p, cout_p)
    need = lib.vlg_conv3x3_fwd_bf16_workspace(rows, cin_p, cout_p, cout_p)
    if sp > 1:
        assert need == sp * rows * cout_p
        rc = lib.vlg_conv3x3_fwd_bf16(FAKE, FAKE, 0, FAKE, 0, 0, 0, 0, rows, cin_p, cout_p, cout_p, W + 2, cin_p, 0,
                                      FAKE, need - 1, None)
        assert rc == VLG_ERR_SHAPE
        # a misaligned workspace, or a PReLU epilogue, is refused like the fp32 entry point refuses it
        assert lib.vlg_conv3x3_fwd_bf16(FAKE, FAKE, 0, FAKE, 0, 0, 0, 0, rows, cin_p, cout_p, cout_p, W + 2, cin_p, 0,
                                        FAKE + 4, need, None) == VLG_ERR_ALIGN
    else:
        assert need == 0
    dsp = lib.vlg_conv3x3_dgrad_bf16_splits(rows, cin_p, cout_p)
    dneed = lib.vlg_conv3x3_dgrad_bf16_workspace(rows, cin_p, cout_p)
    if dsp > 1:
        assert dneed == dsp * rows * cin_p
        rc = lib.vlg_conv3x3_dgrad_bf16(FAKE, FAKE, FAKE, FAKE, 0, 0, 0, 0, 0, rows, cin_p, cout_p, W + 2, cin_p, 0,
                                        FAKE, dneed - 1, 0, None)
        assert rc == VLG_ERR_SHAPE
    else:
        assert dneed == 0


def test_coarse_trunk_levels_split():
    lib = _lib()
    # the 512 -> 512 levels of VGG19 / HED at b = 4: 32 x 32 and 16 x 16 pixels give a handful of 128 x 128 tiles
    for hw in (32, 16):
        assert lib.vlg_conv3x3_fwd_bf16_splits(_rows(4, hw, hw), 512, 512, 512) > 1
    # the 32-channel GridNet rows at full size do not split
    assert lib.vlg_conv3x3_fwd_bf16_splits(_rows(4, 256, 256), 32, 32, 32) == 1
    assert lib.vlg_conv3x3_fwd_bf16_workspace(_rows(4, 256, 256), 32, 32, 32) == 0


@pytest.mark.parametrize("b,H,W,cin_p,cout_p", [(2, 12, 20, 32, 32), (2, 40, 44, 64, 64), (4, 256, 256, 32, 32),
                                               (4, 64, 64, 96, 96), (2, 16, 16, 64, 128)])
def test_slope_partials_and_slabs_are_exact(b, H, W, cin_p, cout_p):
    lib = _lib()
    rows = _rows(b, H, W)
    n_da = lib.vlg_conv3x3_dgrad_bf16_slabs(rows, cin_p)
    assert n_da >= 1
    rc = lib.vlg_conv3x3_dgrad_bf16(FAKE, FAKE, FAKE, FAKE, 0, FAKE, FAKE, 0, 0, rows, cin_p, cout_p, W + 2, cin_p, 8,
                                    0, 0, n_da - 1, None)
    assert rc == VLG_ERR_SHAPE
    n_slabs = lib.vlg_conv3x3_wgrad_bf16_slabs(rows, cin_p, cout_p)
    assert n_slabs >= 1
    stride = cout_p * 9 * cin_p + cout_p
    rc = lib.vlg_conv3x3_wgrad_bf16(FAKE, FAKE, FAKE, stride, n_slabs * stride - 1, 0, 0, rows, cin_p, cout_p, W + 2,
                                    cin_p, None)
    assert rc == VLG_ERR_SHAPE
    assert lib.vlg_conv3x3_wgrad_bf16(FAKE, FAKE, FAKE, stride - 1, 10 ** 12, 0, 0, rows, cin_p, cout_p, W + 2,
                                      cin_p, None) == VLG_ERR_SHAPE


def test_shape_and_alignment_refusals_match_fp32():
    """Validation order and return codes of the bf16 entry points are those of the fp32 ones."""
    lib = _lib()
    rows = _rows(1, 8, 8)
    calls = [
        ("fwd", (FAKE, FAKE, 0, FAKE, 0, 0, 0, 0, rows, 48, 32, 32, 10, 48, 0, 0, 0, None)),        # cin_p not 32k
        ("fwd", (FAKE + 4, FAKE, 0, FAKE, 0, 0, 0, 0, rows, 32, 32, 32, 10, 32, 0, 0, 0, None)),    # misaligned input
        ("fwd", (FAKE, FAKE, 0, FAKE, 0, 0, 0, 0, rows, 32, 33, 32, 10, 32, 0, 0, 0, None)),        # cout > cout_p
        ("fwd", (FAKE, FAKE, 0, FAKE, 0, 0, 0, 0, rows, 32, 32, 32, 10, 32, 2, 0, 0, None)),        # RESID without resid
        ("fwd", (FAKE, FAKE, 0, FAKE, 0, 0, FAKE, 0, rows, 32, 32, 32, 10, 32, 32, 0, 0, None)),    # CIN4 with a slope
        ("dgrad", (FAKE, FAKE, FAKE, 0, 0, 0, 0, 0, 0, rows, 160, 32, 10, 160, 0, 0, 0, 0, None)),  # wide cin not 128k
        ("dgrad", (FAKE, FAKE, FAKE, 0, 0, 0, 0, 0, 0, rows, 32, 32, 10, 32, 8, 0, 0, 0, None)),    # DPRELU without x_in
        ("dgrad", (FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, rows, 32, 32, 10, 32, 0, 0, 0, 0, None)),  # misaligned din
        ("wgrad", (FAKE, FAKE, FAKE, 100, 10 ** 9, 0, 0, rows, 32, 32, 10, 32, None)),             # short slab stride
        ("wgrad", (FAKE, FAKE + 4, FAKE, 10 ** 4, 10 ** 9, 0, 0, rows, 32, 32, 10, 32, None)),     # misaligned input
        ("wgrad", (FAKE, FAKE, FAKE, 10 ** 4, 10 ** 9, 0, 0, 0, 32, 32, 10, 32, None)),            # no rows
    ]
    for op, args in calls:
        want = getattr(lib, "vlg_conv3x3_%s" % op)(*args)
        got = getattr(lib, "vlg_conv3x3_%s_bf16" % op)(*args)
        assert want in (VLG_ERR_SHAPE, VLG_ERR_ALIGN) and got == want, (op, args, want, got)


def test_conv_sym_names_every_bf16_symbol():
    from vlg import hip
    names = ["vlg_conv3x3_fwd", "vlg_conv3x3_fwd_splits", "vlg_conv3x3_fwd_workspace", "vlg_conv3x3_dgrad",
             "vlg_conv3x3_dgrad_splits", "vlg_conv3x3_dgrad_workspace", "vlg_conv3x3_dgrad_slabs", "vlg_conv3x3_wgrad",
             "vlg_conv3x3_wgrad_slabs"]
    for n in names:
        assert hip.conv_sym(n, "fp32") == n
        b = hip.conv_sym(n, "bf16")
        assert b in hip.SIGNATURES and b.startswith(n[:len("vlg_conv3x3_") + len(n.split("_")[2])] + "_bf16"), b
    with pytest.raises(ValueError):
        hip.conv_sym("vlg_conv3x3_fwd", "fp16")

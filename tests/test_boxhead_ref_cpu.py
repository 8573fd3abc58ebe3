"""CPU: the Gaussian box head's restatement (tests/boxhead_ref.py) checked on its own - closed-form gradient against fp64
autograd of the definition, coverage on calibrated residuals, the normal draws' moments, the u rounding case - and the
host side of the option: LayoutConfig, init_params, grow_box_head, the option rules, the trainer's knobs."""
import dataclasses
import math
import types

import numpy as np
import pytest
import torch

import boxhead_ref as R
import decode_ref as D
from vlg import spec
from vlg.spec import LayoutConfig, param_layout, param_shapes

C = 20


def _case(B=3, T=4, N=23, ld=32, seed=0, spread=6.0):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(B * N * T, ld, generator=g, dtype=torch.float64) * spread
    tgt = torch.rand(B, T, N, 4, generator=g, dtype=torch.float64)
    valid = (torch.rand(B, T, N, generator=g) > 0.3).double()
    return out, tgt, valid, B, T, N


def test_constants_agree_with_the_spec():
    assert (R.S_MIN, R.S_MAX) == (spec.BOX_S_MIN, spec.BOX_S_MAX) == (-7.0, 0.0)


@pytest.mark.parametrize("w_nll", [1.0, 0.37])
def test_closed_form_gradient_is_autograd_of_the_definition(w_nll):
    out, tgt, valid, B, T, N = _case()
    out.requires_grad_(True)
    nll, _ = R.box_nll(out, tgt, valid, B, T, N, C)
    (w_nll * nll).backward()
    ref = R.box_nll_closed(out.detach(), tgt, valid, B, T, N, C, w_nll)
    grad = out.grad
    scale = grad[:, C + 4:C + 8].abs().max()
    assert float((grad[:, C + 4:C + 8] - ref["dscale"]).abs().max()) <= 1e-12 * float(scale)
    assert float(ref["nll"]) == pytest.approx(float(nll.detach()), rel=1e-14)
    # the mean is detached, the logits and the padding columns are not read: exactly 0
    assert bool((grad[:, :C + 4] == 0).all()) and bool((grad[:, C + 8:] == 0).all())
    assert bool((ref["dscale"][R.rows_of(valid, B, T, N)[:, 0] == 0] == 0).all())


def test_all_invalid_clamps_the_count_and_gives_zero():
    out, tgt, valid, B, T, N = _case()
    ref = R.box_nll_closed(out, tgt, torch.zeros_like(valid), B, T, N, C)
    assert float(ref["nll"]) == 0.0 and float(ref["cover"]) == 0.0 and bool((ref["dscale"] == 0).all()) and ref["cnt"] == 1.0


def test_cover_of_calibrated_residuals_is_0683():
    B, T, N = 8, 16, 64
    g = torch.Generator().manual_seed(3)
    M = B * T * N
    out = torch.zeros(M, 32, dtype=torch.float64)
    out[:, C:C + 4] = torch.randn(M, 4, generator=g, dtype=torch.float64) * 0.3            # means near the middle
    out[:, C + 4:C + 8] = torch.randn(M, 4, generator=g, dtype=torch.float64) - 1.0        # sigma around e^-5: nothing clamps
    mu = torch.sigmoid(out[:, C:C + 4])
    sigma = torch.exp(R.S_MIN + (R.S_MAX - R.S_MIN) * torch.sigmoid(out[:, C + 4:C + 8]))
    tgt_rows = mu + sigma * torch.randn(M, 4, generator=g, dtype=torch.float64)
    tgt = tgt_rows.view(B, N, T, 4).permute(0, 2, 1, 3).contiguous()                       # rows -> the public order
    _, cover = R.box_nll(out, tgt, torch.ones(B, T, N, dtype=torch.float64), B, T, N, C)
    p = math.erf(1.0 / math.sqrt(2.0))
    n = 4 * M
    assert abs(float(cover) - p) <= 3.0 * math.sqrt(p * (1.0 - p) / n), (float(cover), p)
    assert abs(p - 0.683) < 5e-4


def test_normal_draws_have_zero_mean_and_unit_variance():
    n_tok = 1 << 20                                                                        # 1 048 576 tokens, 4 draws each
    z = R.normals(np.arange(n_tok), 3, 20240229)
    assert z.shape == (n_tok, 4) and np.isfinite(z).all()
    n = z.size
    assert abs(z.mean()) <= 5.0 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    for k in range(4):                                                                     # and each of the four on its own
        assert abs(z[:, k].mean()) <= 5.0 / math.sqrt(n_tok) and abs(z[:, k].var() - 1.0) <= 5.0 * math.sqrt(2.0 / n_tok)
    # the stream is the box draw's own: word 0 differs from the class draw's (stream 0) for the same token and step
    assert not np.array_equal(R.normals(np.arange(64), 3, 7), R.normals(np.arange(64), 4, 7))


def test_u_rounds_in_fp32_and_the_extreme_word_gives_a_finite_z():
    ones = np.array([0xFFFFFFFF], dtype=np.uint64)
    u = R.uniforms32(ones)
    assert u[0] == 1.0                                      # (2^24 - 1) * 2^-24 + 2^-25 rounds to 1.0 in fp32 (the fp64 value is below 1)
    assert (0xFFFFFFFF >> 8) * 2.0 ** -24 + 2.0 ** -25 < 1.0
    z = R.normals_of_words([ones, ones, ones, ones])
    assert np.isfinite(z).all() and np.all(z[:, [0, 2]] == 0.0) and np.all(np.abs(z) == 0.0)
    zero = np.zeros(1, dtype=np.uint64)
    z0 = R.normals_of_words([zero, zero, zero, zero])       # the smallest u: the largest radius, sqrt(-2 ln 2^-25) = 5.887
    assert np.isfinite(z0).all() and abs(abs(z0[0, 0]) - math.sqrt(50.0 * math.log(2.0))) < 1e-4
    # below 2^23 the fp32 sum is exact
    w = np.array([0x7FFFFF00, 0x12345600], dtype=np.uint64)
    assert np.array_equal(R.uniforms32(w), (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 + 2.0 ** -25)


def test_class_draw_is_untouched_by_the_box_temperature():
    B, T, N = 2, 4, 9
    g = torch.Generator().manual_seed(5)
    out_last = torch.randn(B * N, 32, generator=g) * 3
    cls_in = torch.randint(0, C + 1, (B, T, N), generator=g)
    box_in = torch.rand(B, T, N, 4, generator=g)
    want, mean_box, _ = D.next_frame(out_last[:, :C + 4], cls_in, box_in, C, 2, 0.8, 5, 11, keep_padded=True)
    for tau in (0.0, 0.5, 2.0):
        cls, box, _ = R.next_frame(out_last, cls_in, box_in, C, 2, 0.8, 5, 11, keep_padded=True, box_temperature=tau)
        assert torch.equal(cls, want)
        assert bool(((box >= 0) & (box <= 1)).all())
        pad = cls_in[:, -1] >= C
        assert torch.equal(box[pad], box_in[:, -1].double()[pad])
        assert torch.equal(box, mean_box) == (tau == 0.0)


# ---------------------------------------------------------------------------------------------------- the model option
def test_n_out_and_param_layout():
    point, gauss = LayoutConfig(B=2, T=4, N=8, d=64, n_layers=2), LayoutConfig(B=2, T=4, N=8, d=64, n_layers=2, box_head="gaussian")
    assert point.n_out == 24 and gauss.n_out == 32 and point.loss_tail == 4 and gauss.loss_tail == 8
    assert LayoutConfig().box_head == "point"
    # the point head's layout is what it was: the same as a config that never heard of the option
    assert param_layout(point) == param_layout(dataclasses.replace(point, box_head="point"))
    assert param_shapes(point)["head_w"] == (24, 64) and param_shapes(gauss)["head_w"] == (32, 64)
    lp, lg = param_layout(point), param_layout(gauss)
    assert all(lp[0][k] == lg[0][k] for k in lp[0] if not k.startswith("head_")) and lg[1] == lp[1] + 8 * 64 + 8
    assert "box_head" not in point.describe() and "box_head" in gauss.describe()
    assert {k: v for k, v in gauss.describe().items() if k != "box_head"} == point.describe()
    with pytest.raises(ValueError):
        LayoutConfig(box_head="laplace").validate()


def test_init_params_and_grow_box_head_agree_bit_for_bit():
    from vlg.engine import init_params
    point, gauss = LayoutConfig(B=2, T=4, N=8, d=64, n_layers=2), LayoutConfig(B=2, T=4, N=8, d=64, n_layers=2, box_head="gaussian")
    p, q = init_params(point, 1024), init_params(gauss, 1024)
    grown = spec.grow_box_head(p, gauss)
    assert set(grown) == set(q)
    for name in q:
        assert grown[name].shape == q[name].shape and torch.equal(grown[name], q[name]), name
    assert bool((q["head_w"][C + 4:] == 0).all()) and bool((q["head_b"][C + 4:] == 0).all())
    assert torch.equal(q["head_w"][:C + 4], p["head_w"]) and torch.equal(q["head_b"][:C + 4], p["head_b"])
    with pytest.raises(ValueError):
        spec.grow_box_head(p, point)                      # the config names the head to grow to
    with pytest.raises(ValueError):
        spec.grow_box_head(q, gauss)                      # already grown


def test_option_rules():
    assert spec.box_options() == ("point", 1.0) and spec.box_options("gaussian") == ("gaussian", 1.0)
    assert spec.box_options("gaussian", 0.25) == ("gaussian", 0.25) and spec.box_options("gaussian", 0) == ("gaussian", 0.0)
    for bad in (("laplace", None), ("point", 0.5), ("gaussian", -1.0), ("gaussian", float("nan")), ("gaussian", float("inf")),
                ("gaussian", "much")):
        with pytest.raises(ValueError):
            spec.box_options(*bad)
    assert spec.box_temperature_options(0.0) == 0.0 and spec.box_temperature_options(1.5, "gaussian") == 1.5
    for bad in ((0.5, "point"), (-0.1, "gaussian"), (float("nan"), "gaussian"), (float("inf"), "gaussian")):
        with pytest.raises(ValueError):
            spec.box_temperature_options(*bad)


def test_trainer_knobs(monkeypatch):
    import trainer
    for k in ("VLG_BOX_HEAD", "VLG_BOX_NLL_WEIGHT", "VLG_GEN_BOX_TEMPERATURE", "VLG_GEN_TEMPERATURE", "VLG_GEN_TOP_K", "VLG_GEN_SEED",
              "VLG_GEN_KEEP_PADDED"):
        monkeypatch.delenv(k, raising=False)
    a = types.SimpleNamespace(seed=5)
    assert trainer.box_knobs(a) == {}
    assert trainer.generation_knobs(a) == {"temperature": 0.0, "top_k": 0, "seed": 5, "keep_padded": False}
    monkeypatch.setenv("VLG_BOX_NLL_WEIGHT", "0.5")
    with pytest.raises(ValueError):
        trainer.box_knobs(a)                              # the weight without the head
    monkeypatch.setenv("VLG_BOX_HEAD", "gaussian")
    assert trainer.box_knobs(a) == {"box_head": "gaussian", "box_nll_weight": 0.5}
    monkeypatch.setenv("VLG_GEN_BOX_TEMPERATURE", "0.8")
    assert trainer.generation_knobs(a)["box_temperature"] == 0.8
    assert trainer.generation_knobs(types.SimpleNamespace(seed=5, gen_box_temperature=1.25))["box_temperature"] == 1.25
    monkeypatch.setenv("VLG_BOX_HEAD", "point")
    monkeypatch.delenv("VLG_BOX_NLL_WEIGHT")
    with pytest.raises(ValueError):
        trainer.generation_knobs(a)                       # a box temperature with the point head
    monkeypatch.setenv("VLG_BOX_HEAD", "cauchy")
    with pytest.raises(ValueError):
        trainer.box_knobs(a)


def test_bucket_ranges_take_the_tail_length():
    from vlg.dp import bucket_ranges
    gauss = LayoutConfig(B=2, T=4, N=8, d=64, n_layers=2, box_head="gaussian")
    layout, n = param_layout(gauss)
    b = bucket_ranges(layout, n, gauss.n_layers, tail_extra=gauss.loss_tail)
    assert b[0][2] == n + 8 and sorted(s for _, s, _ in b)[0] == 0

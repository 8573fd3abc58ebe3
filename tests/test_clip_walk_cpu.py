"""CPU: what the edge cases of tests/test_hip_clip_attention_edges.py reach in the per-clip attention kernels, and what they
would catch - shown on clip_walk's restatement of the forward walk of csrc/attention_clip.hip, so it runs anywhere.

  1. the restatement, unmutated in fp64, IS the specification: oracle.layout_spec.clip_attention and the fp64 lse
  2. every case reaches the tile paths it is named for (clip_walk.census, assertions per case below)
  3. every mutation of the walk - one per line of the kernel that no earlier test would miss - fails the fp32 bar of the GPU
     tests (helpers.vs_cpu32 against fp64 with torch-CPU fp32 as the yardstick, lse within 1e-5 (1 + |lse|)) on a named case
  4. the record of the gap: on the inputs of every kernel-level case that existed before, dropping the `m_use` guard changes
     nothing - no query of theirs meets a fully masked key tile before it has seen a key
"""
import pytest
import torch

import clip_walk as W
from helpers import vs_cpu32
from oracle import layout_spec as O
from test_hip_clip_attention_bf16 import SHAPES as BF16_SHAPES, inputs as bf16_inputs, lse_want
from test_hip_pixel_ops import within

_REF = {}


def reference(name):
    """{"in": (qkv, gy, valid), "out64", "out32", "lse64"} of a case, computed once"""
    if name not in _REF:
        qkv, gy, valid = W.make_case(name)
        _REF[name] = dict({"in": (qkv, gy, valid)}, **_reference(qkv, valid))
    return _REF[name]


def _reference(qkv, valid):
    heads = qkv.shape[-1] // 192
    r = {"lse64": lse_want(qkv, valid, heads)}
    for dt, key in ((torch.float64, "out64"), (torch.float32, "out32")):
        r[key] = O.clip_attention(qkv.to(dt), heads, valid.to(dt) if valid is not None else None)
    return r


def fp32_bar(out, lse, r, what):
    """the forward half of the GPU tests' fp32 bars"""
    vs_cpu32(out, r["out64"], r["out32"], what + " out")
    within(lse, r["lse64"], 1e-5 * (1 + r["lse64"].abs()), what + " lse")


def _census(name):
    B, T, N, d, _, _ = W.CASES[name]
    qkv, _, valid = reference(name)["in"]
    return W.census(B, T, N, valid, W.log2_scores(qkv, d // 64))


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_the_walk_is_the_specification(name):
    r = reference(name)
    qkv, _, valid = r["in"]
    heads = qkv.shape[-1] // 192
    out, lse = W.walk_forward(qkv, valid, heads, torch.float64)
    assert float((out - r["out64"]).abs().max()) <= 1e-12
    assert float((lse - r["lse64"]).abs().max()) <= 1e-12
    out, lse = W.walk_forward(qkv, valid, heads, torch.float32)      # and in fp32 it meets the bar it is mutated under
    fp32_bar(out, lse, r, name)


def test_every_case_reaches_what_it_is_named_for():
    c = {n: _census(n) for n in W.CASES}
    print()
    for n in W.CASES:
        print("%-16s %s" % (n, " ".join("%s=%d" % kv for kv in c[n].items())))
    computed = lambda n: c[n]["whole"] + c[n]["elementwise"]
    # the m_use = 0 path: a lane's whole first tile(s) invisible, in both clips of lead-empty
    assert c["lead-empty"]["first_all_masked"] >= 2
    assert c["all-invalid"]["first_all_masked"] >= 1 and c["one-slot"]["first_all_masked"] >= 1
    # the production padding pattern: a fully masked tile AFTER the lane has seen keys, never before
    assert c["prefix-64"]["later_all_masked"] > 0 and c["prefix-64"]["first_all_masked"] == 0
    for m in ("null", "prefix"):
        # the running maximum arrives in the first tile: alpha == 1 on every lane, the rescale is skipped
        assert c["first-max/" + m]["max_moved"] == 0 and c["first-max/" + m]["rescale_skipped"] > 0
        for s in ("late-max/", "alt-x5/"):                           # ... and keeps moving
            assert 2 * c[s + m]["max_moved"] > c[s + m]["scored"], (s + m, c[s + m])
    for n in ("1x1x160/null", "1x2x160/null"):                       # a frame spans several 128-query blocks
        assert c[n]["elementwise"] == 0 and c[n]["whole"] > 0
    assert c["1x1x160/null"]["hidden"] == 0 and c["1x1x160/null"]["inactive_wave"] == 3
    assert c["1x32x1/null"]["whole"] == 0 and c["1x32x1/null"]["hidden"] == 0 and c["1x32x1/null"]["elementwise"] == 1
    n = c["2x64x2/null"]                                             # T = 64: everything at once, all waves active
    assert min(n["hidden"], n["whole"], n["elementwise"]) > 0 and n["inactive_wave"] == 0
    for n in W.CASES:                                                # a mask makes every computed tile element-wise
        if W.CASES[n][4] != "null":
            assert c[n]["whole"] == 0 and computed(n) > 0
    # the key-owner walk: hidden and computed query tiles, waves whose own keys are all padded
    k = W.census_keys(2, 8, 8, reference("lead-empty")["in"][2])
    assert k["own_all_padded"] == 2 and k["hidden"] > 0 and k["computed"] > 0
    k = W.census_keys(4, 2, 64, reference("prefix-64")["in"][2])
    assert k["own_all_padded"] == 6 and k["hidden"] == 16 and k["computed"] == 48
    k = W.census_keys(1, 2, 160, None)
    assert k["not_staged"] > 0 and k["hidden"] > 0 and k["inactive_wave"] == 2


# mutation -> the case that fails it (DESIGN.md has the whole mutation x case table)
CAUGHT_BY = {"no_guard": "lead-empty", "skip_rescale": "late-max/null", "whole_when_elementwise": "prefix-64",
             "no_self": "all-invalid", "invalid_lt0": "non-binary", "kend_one_frame_short": "1x3x96/null"}


@pytest.mark.parametrize("mutation", W.MUTATIONS)
def test_every_mutation_fails_at_a_named_case(mutation):
    name = CAUGHT_BY[mutation]
    r = reference(name)
    qkv, _, valid = r["in"]
    out, lse = W.walk_forward(qkv, valid, qkv.shape[-1] // 192, torch.float32, mutate=mutation)
    with pytest.raises(AssertionError):
        fp32_bar(out, lse, r, name)


def test_mutation_table():
    """Printed for DESIGN.md: which cases fail which mutation under the fp32 bar."""
    print()
    for mutation in W.MUTATIONS:
        caught = []
        for name in sorted(W.CASES):
            r = reference(name)
            qkv, _, valid = r["in"]
            out, lse = W.walk_forward(qkv, valid, qkv.shape[-1] // 192, torch.float32, mutate=mutation)
            try:
                fp32_bar(out, lse, r, name)
            except AssertionError:
                caught.append(name)
        print("%-24s %s" % (mutation, ", ".join(caught)))
        assert CAUGHT_BY[mutation] in caught


def _existing_cases():
    """(id, qkv, valid) of every kernel-level case the suite had, by the modules' own seeds and mask recipes"""
    from test_hip_layout_ops import CLIP
    for p in CLIP:                                                   # test_hip_layout_ops.test_clip_attention_fp32
        B, T, N, d = p.values if hasattr(p, "values") else p
        for mode in ("null", "ones", "masked"):
            g = torch.Generator().manual_seed(B * 100 + T * N + d)
            qkv = torch.randn(B, T, N, 3 * d, generator=g) * 1.5
            torch.randn(B, T, N, d, generator=g)
            valid = {"null": None, "ones": torch.ones(B, T, N), "masked": (torch.rand(B, T, N, generator=g) > 0.3).float()}[mode]
            yield "fp32 %s %s" % ((B, T, N, d), mode), qkv, valid
    for B, T, N, d in [(2, 16, 24, 64), (1, 32, 64, 128), (2, 8, 16, 512)]:
        g = torch.Generator().manual_seed(77 + N)                    # ..._fp32_masks_are_exact
        qkv = torch.randn(B, T, N, 3 * d, generator=g) * 0.7
        torch.randn(B, T, N, d, generator=g)
        yield "fp32 exact %s" % ((B, T, N, d),), qkv, (torch.rand(B, T, N, generator=g) > 0.3).float()
        qkv, _, valid = bf16_inputs(B, T, N, d, True, seed=77 + N)   # ..._bf16_masks_are_exact
        yield "bf16 exact %s" % ((B, T, N, d),), qkv, valid
    for B, T, N, d, masked in BF16_SHAPES:                           # test_clip_attention_bf16_against_fp64
        qkv, _, valid = bf16_inputs(B, T, N, d, masked, seed=B * 1000 + T * N + d)
        yield "bf16 %s %s" % ((B, T, N, d), masked), qkv, valid


def test_no_earlier_case_would_miss_the_guard():
    n = 0
    for what, qkv, valid in _existing_cases():
        B, T, N, _ = qkv.shape
        heads = qkv.shape[-1] // 192
        c = W.census(B, T, N, valid)
        assert c["first_all_masked"] == 0, what
        got = W.walk_forward(qkv, valid, heads, torch.float32, mutate="no_guard")
        same = W.walk_forward(qkv, valid, heads, torch.float32)
        assert torch.equal(got[0], same[0]) and torch.equal(got[1], same[1]), what
        fp32_bar(got[0], got[1], _reference(qkv, valid), what)
        n += 1
    assert n == 12 + 6 + len(BF16_SHAPES)

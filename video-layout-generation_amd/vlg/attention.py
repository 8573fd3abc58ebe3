"""The attention kinds of the layout-token encoder, stated once: what a layer's attention launch is called, which argument
shape it takes, how many (query, key) pairs it visits, whether grown frames are cached by default.  Pure Python, no import
of vlg, no device, no library: vlg/spec.py, vlg/engine.py and the attention tools under tools/ all read these rows."""
from __future__ import annotations

import dataclasses
from typing import Tuple


@dataclasses.dataclass(frozen=True)
class AttentionKind:
    stem: str           # entry points: stem + "_fwd" | "_bwd" | "_step" (+ "_bf16", which the caller appends by storage mode)
    family: str         # timer families: family + "_fwd" | "_bwd" | "_step"
    # per-clip kernels take `valid` and (B, T, N, d), save lse and use delta, and a query sees every slot of a visible frame;
    # per-slot kernels take (n_seq, T, d) and a query sees its own slot alone
    per_clip: bool
    causal: bool        # a query of frame t sees the frames <= t; else frame t alone
    cached: bool        # grown frames of a short-prompt rollout go through the cached step by default

    def step_frames(self, p: int) -> int:
        """frames whose keys a generation step at position p reads"""
        return p + 1 if self.causal else 1

    def pairs(self, T: int, N: int) -> int:
        """visible (query, key) pairs per clip and head of a full forward"""
        return (N * N if self.per_clip else N) * (T * (T + 1) // 2 if self.causal else T)

    def step_pairs(self, N: int, p: int) -> int:
        """the same for the generation step at position p: the queries of frame p alone"""
        return (N * N if self.per_clip else N) * self.step_frames(p)


SLOT = AttentionKind("vlg_attention", "attn", per_clip=False, causal=True, cached=True)                # along time, per (clip, slot)
CLIP = AttentionKind("vlg_attention_clip", "attn_clip", per_clip=True, causal=True, cached=False)      # block-causal over a clip; cached with clip_cache alone
FRAME = AttentionKind("vlg_attention_frame", "attn_frame", per_clip=True, causal=False, cached=True)   # across the slots of one frame
MODES = {"slot": (SLOT,), "clip": (CLIP,), "factored": (SLOT, FRAME)}      # attention mode -> the kinds its layers cycle through


def layer_kinds(attention: str, n_layers: int) -> Tuple[AttentionKind, ...]:
    """the kind of every layer: all SLOT, all CLIP, or - "factored" - SLOT on even layers and FRAME on odd ones"""
    cycle = MODES[attention]
    return tuple(cycle[l % len(cycle)] for l in range(n_layers))


def cached_by_default(attention: str) -> bool:
    """whether a short prompt's grown frames have the cached step without the engine option clip_cache"""
    return all(k.cached for k in MODES[attention])


def lse_rows(kinds: Tuple[AttentionKind, ...]) -> Tuple[int, ...]:
    """per layer, the number of per-clip layers below it: the row of the lse workspace a per-clip layer saves into"""
    return tuple(sum(k.per_clip for k in kinds[:l]) for l in range(len(kinds)))

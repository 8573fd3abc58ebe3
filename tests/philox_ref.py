"""The device's random draws restated once on the CPU (csrc/philox.h; include/vlg_hip.h, "random draws"): Philox4x32-10 in
numpy integers, the table of counter streams, the seed's key and the ways a word becomes a number.  Plain module: test
infrastructure, nothing collected.  decode_ref, dropout_ref, sched_ref, augment_ref and boxhead_ref all draw from here."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)
_8 = np.uint64(8)
TWO24 = 1 << 24

# enum vlg_rng_stream of include/vlg_hip.h (tests/test_rng_streams_cpu.py holds the two together): the third counter word
STREAMS = {
    "CLASS_DRAW": 0,        # u of a sampled class
    "SCHED_COIN": 1,        # scheduled sampling: truth or prediction
    "CLIP_DRAW": 2,         # augmentation, per clip
    "TRACK_DROP": 3,        # augmentation, per track
    "TOKEN_JITTER": 4,      # augmentation, per input token
    "BOX_NORMAL": 5,        # the sampled box of the Gaussian box head
}
CLASS_DRAW, SCHED_COIN, CLIP_DRAW, TRACK_DROP, TOKEN_JITTER, BOX_NORMAL = (
    STREAMS[n] for n in ("CLASS_DRAW", "SCHED_COIN", "CLIP_DRAW", "TRACK_DROP", "TOKEN_JITTER", "BOX_NORMAL"))


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (ints or equal-shaped integer arrays) -> the 4 output words as uint64 arrays < 2^32.
    Random123's round: c' = [hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)], key += (W0, W1) between rounds."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & _MASK for x in key]
    for r in range(10):
        if r > 0:
            k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]              # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _32) ^ c[3] ^ k[1], p0 & _MASK]
    return c


def key(seed):
    """(k0, k1) = (seed & 0xffffffff, seed >> 32) of a 64-bit seed"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def words(index, step, stream, seed):
    """the four Philox words of counter (index, step, stream, 0) under the seed's key, uint64 arrays < 2^32"""
    index = np.asarray(index, dtype=np.uint64)
    z = np.zeros_like(index)
    k0, k1 = key(seed)
    return philox4x32_10((index, z + np.uint64(step), z + np.uint64(stream), z), (z + np.uint64(k0), z + np.uint64(k1)))


# ---- one word -> a number: the upper 24 bits
def bits24(x):
    """x >> 8 as int64: what a coin compares"""
    return (np.asarray(x, dtype=np.uint64) >> _8).astype(np.int64)


def unit64(x):
    """(x >> 8) * 2^-24 + 2^-25, the rule in exact arithmetic: float64, strictly inside (0, 1)"""
    return (np.asarray(x, dtype=np.uint64) >> _8).astype(np.float64) * 2.0 ** -24 + 2.0 ** -25


def unit32(x):
    """the same as the kernels form it: fp32 arithmetic (x >> 8 is exact, the sum rounds above 2^23 and may give 1.0), as float64"""
    v = (np.asarray(x, dtype=np.uint64) >> _8).astype(np.float32)
    return (v * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)).astype(np.float64)


def signed32(x):
    """(float)(x >> 8) * 2^-23 - 1: fp32 in [-1, 1), every step exact"""
    return (x >> _8).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)


def coin(x, thr):
    return bits24(x) < int(thr)


def coin_threshold(p):
    """round(p * 2^24): what vlg_sched_plan and vlg_augment_plan compute"""
    return int(np.floor(np.float64(p) * TWO24 + 0.5))

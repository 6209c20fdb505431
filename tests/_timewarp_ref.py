"""Test-only restatement of SpecAugment's time warp (include/st_hip.h, st_specaug_plan_warp): the draw and the map in Python
integers, the blend in fp64 (and, for the one test that needs bits, the kernel's fp32 formula with numpy), warped and masked
arrays built with numpy, and the seeds / lengths / policies the GPU tests (tests/test_timewarp_gpu.py) use - chosen HERE, on
the CPU, where tests/test_timewarp_cpu.py checks that each of them warps something and leaves something alone.

Nothing in this file calls the package's kernels or wrappers: it reads a policy's plain attributes at most."""
import numpy as np

from tests._specaug_ref import M32, hash32, pick, stack_src, t_raw
from tests import _specaug_ref as sref

WARP_KEY = 0x77617270


# ---- the draw -------------------------------------------------------------------------------------------------------------------
def warp_plan(seed, salt, raw_lengths, W):
    """-> int32 [B, 2] of (c, c'); (0, 0): not warped."""
    key = hash32(((seed & M32) + (salt & M32) * 0x9E3779B9) & M32)
    wkey = hash32(key ^ WARP_KEY)
    out = np.zeros((len(raw_lengths), 2), dtype=np.int32)
    for b, n in enumerate(int(v) for v in raw_lengths):
        if W < 1 or n < 2 * W + 3:
            continue
        bits = [hash32(((b * 2 + d) & M32) ^ wkey) for d in (0, 1)]
        c = W + 1 + pick(bits[0], n - 2 * W - 2)
        out[b] = (c, c - W + pick(bits[1], 2 * W + 1))
    return out


def raw_lengths_of(aug, lengths, stacked):
    interval, right = (aug.interval, aug.right) if stacked else (1, 0)
    return [t_raw(n, interval, right) for n in lengths]


def warp_of(aug, seed, lengths, stacked):
    """warp_plan() for a policy object (its plain attributes only); lengths as _specaug_ref.plan_of."""
    return warp_plan(seed, aug.salt, raw_lengths_of(aug, lengths, stacked), aug.time_warp)


# ---- the map --------------------------------------------------------------------------------------------------------------------
def position(u, n, c, cp):
    """Output frame u of an utterance of n raw frames under the pair (c, c') -> (g, fr): source frame and 16-bit fraction."""
    if (c, cp) == (0, 0):
        return u, 0
    if u < cp:
        num, den = u * c, cp
    else:
        num, den = c * (n - 1 - cp) + (u - cp) * (n - 1 - c), n - 1 - cp
    q = num * 65536 // den
    return q >> 16, q & 0xFFFF


def positions(n, c, cp):
    """-> (g, fr): int64 [n] each, for every output frame."""
    p = [position(u, n, int(c), int(cp)) for u in range(n)]
    return np.array([a for a, _ in p], dtype=np.int64), np.array([f for _, f in p], dtype=np.int64)


def stacked_lookup(g, left, interval):
    """(row, slot) of the stacked input (right == 0, left >= interval - 1) that holds raw frame g."""
    row = -(-g // interval)
    return row, left - (row * interval - g)


def warp64(raw, c, cp):
    """raw fp64 [n, F] -> the warped utterance, fp64 [n, F]: x[g] + (fr / 65536) * (x[g + 1] - x[g]); x[g + 1] is not touched
    where fr == 0."""
    raw = np.asarray(raw, dtype=np.float64)
    g, fr = positions(raw.shape[0], c, cp)
    out = raw[g].copy()
    m = fr > 0
    out[m] += (fr[m, None] / 65536.0) * (raw[g[m] + 1] - raw[g[m]])
    return out


def warp32(raw, c, cp):
    """The kernel's own formula on fp32 [n, F]: difference, product and sum each rounded to fp32 (no fused multiply-add)."""
    raw = np.asarray(raw, dtype=np.float32)
    g, fr = positions(raw.shape[0], c, cp)
    out = raw[g].copy()
    m = fr > 0
    w = (fr[m, None].astype(np.float32) * np.float32(1.0 / 65536.0)).astype(np.float32)
    d = (raw[g[m] + 1] - raw[g[m]]).astype(np.float32)
    out[m] = (raw[g[m]] + (w * d).astype(np.float32)).astype(np.float32)
    return out


def bf16_round(v):
    """fp64 -> the nearest bfloat16 (ties to even) as fp64, in one rounding (normal range)."""
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(v)
    return np.ldexp(np.rint(np.ldexp(m, 8)), e - 8)


def bf16_bits(v):
    """int32 bit patterns of bf16_round(v) (exact: the values fit fp32's upper half)."""
    return (bf16_round(v).astype(np.float32).view(np.uint32) >> 16).astype(np.int32)


def stack_rows(raw, n_rows, left, right, interval, fill=None):
    """raw [n, F] -> stacked rows [n_rows, (1 + left + right) * F] by the stacking rule; a slot without a source frame keeps
    ``fill`` ([n_rows, slots * F]) or 0."""
    n, F = raw.shape
    slots = 1 + left + right
    out = np.zeros((n_rows, slots * F), dtype=raw.dtype) if fill is None else np.array(fill, dtype=raw.dtype)
    for r in range(n_rows):
        for k in range(slots):
            src = stack_src(k, r * interval, left, right, n)
            if src >= 0:
                out[r, k * F:(k + 1) * F] = raw[src]
    return out


def shown_frame(n_rows, mel_bins, left, right, interval, n):
    """int64 [n_rows, slots * mel_bins]: the output frame every element of the stacked rows shows (-1: none)."""
    slots = 1 + left + right
    out = np.full((n_rows, slots, mel_bins), -1, dtype=np.int64)
    for r in range(n_rows):
        for k in range(slots):
            out[r, k] = stack_src(k, r * interval, left, right, n)
    return out.reshape(n_rows, -1)


# ---- what the GPU tests run (seeds and salts: those of _specaug_ref's tests of the same name) ---------------------------------------
PLAN_WARPS = (2, 40)                                       # with sref.PLAN_SEED / PLAN_SALT / PLAN_LENGTHS
PLAN_POLICY = dict(mel_bins=80)
STACK_WARP = 5
STACK_EXTRA = 9                                            # a fourth utterance below 2 W + 3 = 13 frames: never warped
STACK_LENGTHS = sref.STACK_LENGTHS + [STACK_EXTRA]
PACK_WARP = 5
PACK_CASES = [(4, 0, 0, 10, 300), (80, 0, 0, 10, 41), (80, 3, 0, 30, 41), (80, 15, 0, 10, 41)]      # (mel_bins, left, right, rate, T)
RAMP_SEED, RAMP_SALT, RAMP_WARP = 4321, 925, 5
RAMP_CASES = [(0, 10, [32, 20, 5]), (3, 30, [11, 7, 2])]   # (left, rate, rows): raw frames <= 32, so 8 * frame is exact in bf16
AGREE_WARP = 5
AGREE_ROWS = sref.AGREE["rows"] + [3]                      # raw lengths 40, 16, 28 and 7 (< 13: never warped)
ENCODER_WARP = 8
STEP_WARP = 40
BUCKET_WARP = 8


def pack_policy(mel_bins, left, right, rate):
    return dict(sref.pack_policy(mel_bins, left, right, rate), time_warp=PACK_WARP)


def agree_policy():
    return dict(sref.agree_policy(), time_warp=AGREE_WARP)

"""Test-only restatement of the SpecAugment draw (include/st_hip.h, st_specaug_plan) in Python integers, the masks applied to
raw and to stacked arrays with numpy, and the seeds / shapes / policies the GPU tests use - chosen HERE, on the CPU, where
tests/test_specaug_cpu.py checks that none of them draws only empty masks.

Nothing in this file calls the package's kernels or wrappers: it reads a policy's plain attributes at most."""
import numpy as np

M32 = 0xFFFFFFFF


def hash32(x):
    """The "lowbias32" finaliser of csrc/st_common.cuh (st_hash32), on a Python int."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def pick(bits, n):
    return (bits * n) >> 32


def t_raw(length, interval=1, right=0):
    """Raw frames the masks are drawn for: the raw length itself (1, 0), or the last raw frame a stacked row can show, plus one."""
    return (int(length) - 1) * interval + 1 + right if int(length) >= 1 else 0


def plan(seed, salt, raw_lengths, mel_bins, n_time, time_width, permille, n_freq, freq_width):
    """-> int32 [B, n_time + n_freq, 2] of (start, width): time masks first."""
    key = hash32(((seed & M32) + (salt & M32) * 0x9E3779B9) & M32)
    out = np.zeros((len(raw_lengths), n_time + n_freq, 2), dtype=np.int32)
    for b, T in enumerate(int(v) for v in raw_lengths):
        for j in range(n_time + n_freq):
            bits = [hash32((((b * 64 + j) * 2 + d) & M32) ^ key) for d in (0, 1)]
            n, cap = (T, min(time_width, T * permille // 1000)) if j < n_time else (mel_bins, min(freq_width, mel_bins))
            width = pick(bits[0], cap + 1)
            out[b, j] = (pick(bits[1], n - width + 1), width)
    return out


def plan_of(aug, seed, lengths, stacked):
    """plan() for a policy object (its plain attributes only); lengths: raw frames, or - stacked - rows of the stacked input."""
    interval, right = (aug.interval, aug.right) if stacked else (1, 0)
    return plan(seed, aug.salt, [t_raw(n, interval, right) for n in lengths], aug.mel_bins, aug.n_time_masks, aug.time_width,
                aug.time_ratio_permille, aug.n_freq_masks, aug.freq_width)


def stack_src(k, t, left, right, length):
    """Raw frame in context slot k of the stacked row at raw frame t (-1: none) - the reference's write order (Dataset.py
    :121-143: middle, left contexts, right contexts indexed with the RIGHT width; later writes win), as loops."""
    src = -1
    if k == left:
        src = t
    for i in range(left):
        if k == left - i - 1 and t >= i + 1:
            src = t - i - 1
    for i in range(right):
        if k == right + i + 1 and t + i + 1 < length:
            src = t + i + 1
    return src


def raw_mask(table_b, n_time, T, F):
    """bool [T, F]: the raw (frame, bin) elements under a mask of one utterance's table."""
    m = np.zeros((T, F), dtype=bool)
    for j, (start, width) in enumerate(table_b.tolist()):
        if j < n_time:
            m[start:start + width, :] = True
        else:
            m[:, start:start + width] = True
    return m


def stacked_mask(table_b, n_time, n_rows, mel_bins, left, right, interval, raw_length):
    """bool [n_rows, mel_bins * (1 + left + right)]: the elements of one utterance's stacked rows under a mask - the source
    frame of (row, slot) under a time mask, or the bin under a frequency mask (a slot without a source only the latter)."""
    time = [(s, w) for s, w in table_b[:n_time].tolist()]
    fm = raw_mask(table_b[n_time:], 0, 1, mel_bins)[0]
    m = np.zeros((n_rows, 1 + left + right, mel_bins), dtype=bool)
    for r in range(n_rows):
        for k in range(1 + left + right):
            src = stack_src(k, r * interval, left, right, raw_length)
            m[r, k] = fm | (src >= 0 and any(s <= src < s + w for s, w in time))
    return m.reshape(n_rows, -1)


# ---- what the GPU tests run: seeds, lengths and policies (constructor keywords) --------------------------------------------------
PLAN_SEED, PLAN_SALT = 1234, 900          # (policy i of the list takes salt PLAN_SALT + i)
PLAN_LENGTHS = [1, 2, 7, 40, 133]
PLAN_POLICIES = [
    dict(mel_bins=80),                                                      # 1: the default
    dict(mel_bins=80, time_width=200, time_ratio_permille=1000),            # 2: wider than every utterance
    dict(mel_bins=80, time_ratio_permille=0),                               # 3: every time width 0
    dict(mel_bins=80, freq_width=100),                                      # 4: freq_width >= mel_bins
    dict(mel_bins=80, n_time_masks=0),                                      # 5: no mask of one kind ...
    dict(mel_bins=80, n_freq_masks=0),                                      #    ... or of the other
    dict(mel_bins=80, n_time_masks=40, n_freq_masks=24),                    # 6: 64 masks in all
    dict(mel_bins=40, left=3, right=2, frame_rate=30),                      # 7: lengths of stacked rows (stacked=True)
]
STACK_SEED, STACK_SALT = 77, 910
STACK_TRIPLES = [(3, 0, 10), (3, 0, 30), (2, 2, 10), (2, 1, 20), (0, 0, 10)]       # those of test_feat_stack_kernel (its _case: 8 bins,
STACK_LENGTHS = [41, 17, 30]                                                       # these lengths)
STACK_POLICY = dict(mel_bins=8, time_width=10, time_ratio_permille=500, freq_width=3)
PACK_SEED, PACK_SALT = 4321, 920
# (mel_bins, left, right, frame_rate, T): F = 4 (one chunk, 256 rows per workgroup), 80 (12 rows), 320 twice (3 rows; once with the
# right-width quirk), 1280 (320 chunks: more than the 256 lanes of a pass); T never a multiple of the rows per workgroup
PACK_CASES = [(4, 0, 0, 10, 300), (80, 0, 0, 10, 41), (80, 3, 0, 30, 41), (80, 2, 1, 20, 41), (80, 8, 7, 10, 41)]
PACK_POLICY = dict(time_width=10, time_ratio_permille=500)


def pack_lengths(T):
    return [T, 1, 17, T - 3]           # one utterance fills T exactly, one has a single row


def pack_policy(mel_bins, left, right, rate):
    return dict(PACK_POLICY, mel_bins=mel_bins, freq_width=min(27, mel_bins // 2), left=left, right=right, frame_rate=rate)


AGREE_SEED, AGREE_SALT = 99, 930
AGREE = dict(left=3, right=0, frame_rate=30, rows=[14, 6, 10])          # raw lengths (n - 1) * 3 + 1 = 40, 16, 28
ENCODER_SEED, ENCODER_SALT = 31, 940
ENCODER_LENGTHS = [50, 23, 1]
ENCODER_POLICY = dict(mel_bins=80, time_width=12, time_ratio_permille=400)
STEP_SEED, STEP_SALT = 500, 950
STEP_POLICY = dict(mel_bins=80)
STEP_BATCH = dict(bsz=4, t_max=160, l_max=20, feat=80, vocab=30, seed=1, t_min=60, l_min=6)       # st_amd.synthetic.make_batch: the batch of
                                                                                                   # test_graph_step_matches_eager_step
BUCKET_SEED, BUCKET_SALT = 700, 960
BUCKET = dict(T_cap=96, L_cap=12, batches=[(96, 80, 21), (96, 80, 22), (96, 80, 23), (40, 20, 24), (33, 9, 25)])     # (t_max, t_min, batch seed)


def agree_policy():
    return dict({k: v for k, v in STACK_POLICY.items()}, left=AGREE["left"], right=AGREE["right"], frame_rate=AGREE["frame_rate"])

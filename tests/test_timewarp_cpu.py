"""-m "not gpu": the host side of SpecAugment's time warp - the policy's new keyword, the geometry refusal of ``pack``, the new
entry points in the C ABI, the wrappers' checks, and the Python restatement of the draw and the map (tests/_timewarp_ref.py)
with the seeds the GPU tests (tests/test_timewarp_gpu.py) run with.  No kernel is launched here."""
import numpy as np
import pytest
import torch

from st_amd import build, native
from st_amd.augment import SpecAugment
from tests import _specaug_ref as sref
from tests import _timewarp_ref as ref

I32 = torch.int32


# ---- 1. the policy object ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [-1, 2.5, "80", None, -0.5, 40000])
def test_constructor_refuses_a_bad_time_warp(w):
    with pytest.raises(ValueError, match="SpecAugment: "):
        SpecAugment(80, time_warp=w)


def test_constructor_defaults():
    a = SpecAugment(80)
    assert a.time_warp == 0 and a.last_warp is None and a.last_masks is None
    b = SpecAugment(80, 2, 40, 200, 2, 27, 3, 0, 30, 7, 80)          # time_warp is the LAST positional, after salt
    assert (b.salt, b.time_warp, b.interval) == (7, 80, 3) and b.last_warp is None
    assert SpecAugment(80, time_warp=5.0).time_warp == 5 and isinstance(SpecAugment(80, time_warp=5.0).time_warp, int)


# ---- 2. pack refuses a geometry whose rows do not show every raw frame, before any launch ----------------------------------------
@pytest.mark.parametrize("left,right,rate", [(2, 1, 20), (1, 0, 30)])
def test_pack_refuses_the_geometry_before_any_launch(left, right, rate):
    aug = SpecAugment(8, left=left, right=right, frame_rate=rate, time_warp=3)
    x = torch.zeros(2, 12, 8 * (1 + left + right))                  # a HOST tensor: a launch - even a wrapper's check - would raise RuntimeError
    with pytest.raises(ValueError, match=r"stack_frames\(\.\.\., augment=aug\)"):
        aug.pack(x, None)
    assert aug.last_warp is None and aug.last_masks is None          # not even the plan ran


# ---- 3. the entry points ---------------------------------------------------------------------------------------------------------
def test_timewarp_entry_points_of_the_abi():
    import os
    import re
    names = {"st_specaug_plan_warp", "st_pack_rows_warp", "st_feat_stack_warp"}
    assert names <= set(native.SIGNATURES)
    assert "st_augment.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "st_augment.hip")).read()
    assert set(re.findall(r'extern\s+"C"\s+int\s+(st\w+)\s*\(', src)) == names | {"st_feat_stack", "st_specaug_plan", "st_pack_rows_aug",
                                                                                   "st_feat_stack_aug"}
    # the table pointers sit where the wrappers pass them
    S = native.SIGNATURES
    assert len(S["st_specaug_plan_warp"]) == len(S["st_specaug_plan"]) + 2
    assert len(S["st_pack_rows_warp"]) == len(S["st_pack_rows_aug"]) + 1
    assert len(S["st_feat_stack_warp"]) == len(S["st_feat_stack_aug"]) + 1


# ---- 4. the wrappers raise before any launch -------------------------------------------------------------------------------------
def test_wrapper_argument_checks_raise_before_any_launch():
    B, T, F0 = 3, 10, 8
    table, warp = torch.zeros(B, 4, 2, dtype=I32), torch.zeros(B, 2, dtype=I32)
    seed, lens = torch.zeros(1, dtype=I32), torch.full((B,), T, dtype=I32)
    plan = dict(seed=seed, salt=1, length=lens, table=table, warp=warp, n_time=2, time_width=5, time_ratio_permille=200, n_freq=2,
                freq_width=3, mel_bins=F0, time_warp=2)
    for bad in (dict(n_time=-1), dict(n_freq=-1), dict(n_time=40, n_freq=25), dict(time_width=-1), dict(freq_width=-1), dict(mel_bins=0),
                dict(time_ratio_permille=1001), dict(time_ratio_permille=-1), dict(interval=0), dict(right=-1), dict(time_warp=-1),
                dict(time_warp=1.5), dict(time_warp=32768)):
        with pytest.raises(ValueError, match="specaug_plan_warp"):
            native.specaug_plan_warp(**dict(plan, **bad))
    x, off = torch.zeros(B, T, 4 * F0), torch.arange(B, dtype=I32) * T
    out = torch.zeros(B * T, 4 * F0, dtype=torch.bfloat16)
    pack = dict(x=x, off=off, length=lens, out=out, table=table, warp=warp, n_time=2, n_freq=2, mel_bins=F0, left=3, right=0, interval=3)
    for bad in (dict(mel_bins=6), dict(mel_bins=0), dict(left=2), dict(left=2, right=1), dict(right=-1), dict(interval=0), dict(n_time=63),
                dict(n_freq=-1), dict(x=x[0]), dict(mel_bins=16), dict(interval=5), dict(x=torch.zeros(B, 11000, 4 * F0)[:, :, :])):
        with pytest.raises(ValueError, match="pack_rows_warp"):
            native.pack_rows_warp(**dict(pack, **bad))
    raw, wide = torch.zeros(B, T, F0), torch.zeros(B * T, 4 * F0, dtype=torch.bfloat16)
    stack = dict(x=raw, in_len=lens, stats=None, left=2, right=1, interval=1, out_off=off, out_len=lens, max_out_len=T, out=wide, table=table,
                 warp=warp, n_time=2, n_freq=2)
    for bad in (dict(left=0), dict(right=-1), dict(interval=0), dict(n_time=70), dict(n_freq=-2), dict(x=raw[0]),
                dict(x=torch.zeros(1, 32768, F0).expand(B, 32768, F0))):
        with pytest.raises(ValueError, match="feat_stack_warp"):
            native.feat_stack_warp(**dict(stack, **bad))
    # ... and with every number in order, host tensors are refused: there is no CPU path
    for fn, kw in ((native.specaug_plan_warp, plan), (native.pack_rows_warp, pack), (native.feat_stack_warp, stack)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            fn(**kw)


# ---- 5. the restatement itself ---------------------------------------------------------------------------------------------------
def test_reference_map_properties():
    """1,000 (seed, length, W) triples: the pair in range; the map monotone, its ends and its anchor exact, and no read past the
    utterance; the 32-bit evaluation the kernels use equals the definition."""
    g = torch.Generator().manual_seed(11)
    seeds = torch.randint(0, 2 ** 31 - 1, (1000,), generator=g).tolist()
    lengths = torch.randint(1, 420, (1000,), generator=g).tolist()
    lengths[:10] = [1, 2, 4, 5, 6, 13, 163, 164, 419, 83]
    warps = [(1, 2, 5, 40, 80)[i % 5] for i in range(1000)]
    warped = moved = 0
    for i, (seed, n, W) in enumerate(zip(seeds, lengths, warps)):
        c, cp = ref.warp_plan(seed, 0x80000000 + i % 3, [3, n], W)[1].tolist()             # (utterance 1: b enters the counter)
        if n < 2 * W + 3:
            assert (c, cp) == (0, 0), (seed, n, W)
            assert ref.position(n - 1, n, 0, 0) == (n - 1, 0)
            continue
        warped += 1
        moved += c != cp
        assert W + 1 <= c <= n - 2 - W and abs(cp - c) <= W and 1 <= cp <= n - 2, (seed, n, W, c, cp)
        gs, frs = ref.positions(n, c, cp)
        q = gs * 65536 + frs
        assert (np.diff(q) >= 0).all(), (seed, n, W)
        assert (gs[0], frs[0]) == (0, 0) and (gs[cp], frs[cp]) == (c, 0) and (gs[n - 1], frs[n - 1]) == (n - 1, 0)
        assert gs.min() >= 0 and gs.max() <= n - 1 and (gs[frs > 0] + 1 <= n - 1).all()
        for u in (0, 1, cp - 1, cp, cp + 1, n - 2, n - 1):
            num, den = (u * c, cp) if u < cp else (c * (n - 1 - cp) + (u - cp) * (n - 1 - c), n - 1 - cp)
            assert num < 2 ** 31 and ((num % den) << 16) < 2 ** 32
            assert (num // den, ((num - num // den * den) << 16) // den) == ref.position(u, n, c, cp)
    assert warped > 300 and moved > 250
    # the longest utterance the kernels take: the 32-bit evaluation is still the definition
    n, W = 32767, 80
    for c, cp in ((W + 1, 1), (n - 2 - W, n - 2), (16000, 16080)):
        for u in (0, 1, cp, cp + 1, n - 2, n - 1, 20000):
            num, den = (u * c, cp) if u < cp else (c * (n - 1 - cp) + (u - cp) * (n - 1 - c), n - 1 - cp)
            assert num < 2 ** 31 and ((num % den) << 16) < 2 ** 31
            assert (num // den, ((num % den) << 16) // den) == ref.position(u, n, c, cp)


def test_reference_blend_and_rounding():
    raw = np.arange(20, dtype=np.float64)[:, None] * 8 + np.zeros((1, 4))
    out = ref.warp64(raw, 7, 4)
    gs, frs = ref.positions(20, 7, 4)
    assert np.array_equal(out[:, 0], 8 * (gs + frs / 65536.0)) and out[4, 0] == 56 and out[19, 0] == 152
    assert np.array_equal(ref.warp64(raw, 0, 0), raw)
    assert np.array_equal(ref.warp32(raw, 7, 4).astype(np.float64), out)               # (exact here: small integers over 8192)
    v = np.array([1.0, 1.00390625, 1.01171875, 1.0 + 2 ** -9, 257.0, 259.0, 3.0e-3])
    want = torch.tensor(v, dtype=torch.float64).float().bfloat16().double().numpy()
    assert np.array_equal(ref.bf16_round(v), want)
    assert ref.bf16_bits(np.array([1.0, 2.0])).tolist() == [0x3F80, 0x4000]


# ---- 6. the stacked lookup -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left,interval", [(3, 3), (2, 3), (0, 1), (3, 1), (1, 2)])
def test_stacked_lookup_equals_the_stacking_rule(left, interval):
    for rows in (1, 2, 5, 14, 41):
        n = sref.t_raw(rows, interval, 0)
        for g in range(n):
            r, k = ref.stacked_lookup(g, left, interval)
            assert 0 <= r < rows and 0 <= k <= left, (rows, g, r, k)
            assert sref.stack_src(k, r * interval, left, 0, n) == g, (rows, g, r, k)


# ---- 7. the GPU tests' inputs ----------------------------------------------------------------------------------------------------
def _mixed(table, what):
    t = table.tolist()
    assert any(c != cp for c, cp in t), "%s: no utterance is moved: %s" % (what, t)
    assert any((c, cp) == (0, 0) for c, cp in t), "%s: no identity utterance: %s" % (what, t)
    return t


def test_gpu_test_inputs_warp_something_and_leave_something_alone():
    """... and the draw gives the entries written down when the feature was specified."""
    p = {W: _mixed(ref.warp_plan(sref.PLAN_SEED, sref.PLAN_SALT, sref.PLAN_LENGTHS, W), "plan W %d" % W) for W in ref.PLAN_WARPS}
    assert p[2] == [[0, 0], [0, 0], [3, 4], [4, 6], [112, 112]]
    assert p[40] == [[0, 0], [0, 0], [0, 0], [0, 0], [84, 82]]
    _mixed(ref.warp_plan(sref.PLAN_SEED + 1, sref.PLAN_SALT, sref.PLAN_LENGTHS, 2), "plan after advance()")
    t = _mixed(ref.warp_plan(sref.STACK_SEED, sref.STACK_SALT, ref.STACK_LENGTHS, ref.STACK_WARP), "stack")
    assert t == [[28, 33], [6, 2], [23, 27], [0, 0]]
    for F0, left, right, rate, T in ref.PACK_CASES:
        aug = SpecAugment(salt=sref.PACK_SALT, **ref.pack_policy(F0, left, right, rate))
        t = _mixed(ref.warp_of(aug, sref.PACK_SEED, sref.pack_lengths(T), True), "pack %s" % ((F0, left, right, rate, T),))
        if (rate, T) == (30, 41):
            assert t == [[80, 76], [0, 0], [11, 6], [31, 30]]
        if T == 300:
            assert t == [[202, 198], [0, 0], [6, 1], [78, 77]]
    for left, rate, rows in ref.RAMP_CASES:
        aug = SpecAugment(8, 0, 0, 0, 0, 0, left, 0, rate, ref.RAMP_SALT, ref.RAMP_WARP)
        _mixed(ref.warp_of(aug, ref.RAMP_SEED, rows, True), "ramp")
        assert max(ref.raw_lengths_of(aug, rows, True)) <= 32
    aug = SpecAugment(salt=sref.AGREE_SALT, **ref.agree_policy())
    assert _mixed(ref.warp_of(aug, sref.AGREE_SEED, ref.AGREE_ROWS, True), "agree") == [[7, 2], [7, 11], [17, 12], [0, 0]]
    aug = SpecAugment(salt=sref.ENCODER_SALT, time_warp=ref.ENCODER_WARP, **sref.ENCODER_POLICY)
    assert _mixed(ref.warp_of(aug, sref.ENCODER_SEED, sref.ENCODER_LENGTHS, True), "encoder") == [[35, 28], [9, 16], [0, 0]]
    # the captured step and bucket mode: something moves at every seed, and the advancing seed changes the table
    from oracle import speech_transformer_oracle as orc
    from st_amd import synthetic
    lengths = synthetic.make_batch(**sref.STEP_BATCH)[2].tolist()
    aug = SpecAugment(salt=sref.STEP_SALT, time_warp=ref.STEP_WARP, **sref.STEP_POLICY)
    tables = [ref.warp_of(aug, sref.STEP_SEED + k, lengths, True) for k in range(1, 5)]
    assert all(any(c != cp for c, cp in t.tolist()) for t in tables)
    assert all((tables[k] != tables[k + 1]).any() for k in range(3))
    bk = sref.BUCKET
    aug = SpecAugment(salt=sref.BUCKET_SALT, time_warp=ref.BUCKET_WARP, **sref.STEP_POLICY)
    for k, (t_max, t_min, seed) in enumerate(bk["batches"]):
        lengths = orc.synthetic_batch(4, t_max, bk["L_cap"], 80, 30, seed=seed, t_min=t_min, l_min=4)["in_len"].tolist()
        assert any(c != cp for c, cp in ref.warp_of(aug, sref.BUCKET_SEED + k + 1, lengths, True).tolist()), k


def test_a_warping_policy_draws_the_masks_of_the_plain_one():
    """The restatement of the masks does not know time_warp at all: plan_of reads the same attributes from both policies."""
    a, b = SpecAugment(80, salt=5), SpecAugment(80, salt=5, time_warp=80)
    assert np.array_equal(sref.plan_of(a, 9, [300, 50], True), sref.plan_of(b, 9, [300, 50], True))

"""-m "not gpu": SpecAugment's host side - the policy object's argument checks, its entry points in the C ABI, the wrappers'
checks, the Python restatement of the draw (tests/_specaug_ref.py) and the seeds the GPU tests (tests/test_specaug_gpu.py)
run with.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from st_amd import augment, build, native, rng
from st_amd.augment import SpecAugment
from tests import _specaug_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = torch.int32


# ---- 1. the policy object ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(n_time_masks=40, n_freq_masks=25), dict(n_time_masks=65, n_freq_masks=0),
                                dict(n_time_masks=-1), dict(time_width=-1), dict(time_ratio_permille=-1), dict(n_freq_masks=-1),
                                dict(freq_width=-3), dict(left=-1), dict(right=-1, left=0), dict(frame_rate=-10), dict(mel_bins=-80),
                                dict(salt=-5), dict(left=1, right=2), dict(mel_bins=82), dict(mel_bins=0), dict(mel_bins=2),
                                dict(time_ratio_permille=1001)])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError, match="SpecAugment"):
        SpecAugment(**dict(dict(mel_bins=80), **kw))


def test_constructor_defaults_and_salts():
    a, b = SpecAugment(80), SpecAugment(80)
    assert (a.n_time_masks, a.time_width, a.time_ratio_permille, a.n_freq_masks, a.freq_width) == (2, 40, 200, 2, 27)
    assert (a.left, a.right, a.frame_rate, a.interval, a.last_masks) == (0, 0, 10, 1, None)
    assert SpecAugment(80, n_time_masks=40, n_freq_masks=24).n_masks == 64
    assert [SpecAugment(8, frame_rate=r).interval for r in (10, 20, 30, 35)] == [1, 2, 3, 3]      # int(rate / 10), as stack_frames
    # default salts: a counter of their own from 2^31 up - and no dropout salt is consumed
    assert a.salt >= 0x80000000 and b.salt == a.salt + 1 and SpecAugment(80, salt=7).salt == 7
    before = rng._salt
    SpecAugment(80)
    assert rng._salt == before


def test_encoder_attribute_is_plain():
    from transformer.Models import Encoder
    enc = Encoder(80, 50, n_layers=1, n_head=2, d_k=32, d_v=32, d_model=64, d_inner_hid=128)
    assert enc.spec_augment is None
    keys = set(enc.state_dict())
    enc.spec_augment = SpecAugment(80)
    assert set(enc.state_dict()) == keys and not any("spec" in k for k in keys)


# ---- 2. the entry points in the ABI (header == binding == library == sources: tests/test_abi_cpu.py, for every entry point) -------
def test_specaug_entry_points_of_the_abi():
    assert {"st_specaug_plan", "st_pack_rows_aug", "st_feat_stack_aug"} <= set(native.SIGNATURES)
    assert "st_augment.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "st_augment.hip")).read()
    assert set(re.findall(r'extern\s+"C"\s+int\s+(st\w+)\s*\(', src)) == {          # the whole feature kernel family
        "st_feat_stack", "st_specaug_plan", "st_pack_rows_aug", "st_feat_stack_aug", "st_specaug_plan_warp", "st_pack_rows_warp",
        "st_feat_stack_warp"}


# ---- 3. the wrappers raise before any launch -------------------------------------------------------------------------------------
def test_wrapper_argument_checks_raise_before_any_launch():
    B, T, F0 = 3, 10, 8
    table = torch.zeros(B, 4, 2, dtype=I32)
    seed, lens = torch.zeros(1, dtype=I32), torch.full((B,), T, dtype=I32)
    plan = dict(seed=seed, salt=1, length=lens, table=table, n_time=2, time_width=5, time_ratio_permille=200, n_freq=2, freq_width=3,
                mel_bins=F0)
    for bad in (dict(n_time=-1), dict(n_freq=-1), dict(n_time=40, n_freq=25), dict(time_width=-1), dict(freq_width=-1), dict(mel_bins=0),
                dict(time_ratio_permille=1001), dict(time_ratio_permille=-1), dict(interval=0), dict(right=-1)):
        with pytest.raises(ValueError, match="specaug_plan"):
            native.specaug_plan(**dict(plan, **bad))
    x, off = torch.zeros(B, T, 4 * F0), torch.arange(B, dtype=I32) * T
    out = torch.zeros(B * T, 4 * F0, dtype=torch.bfloat16)
    pack = dict(x=x, off=off, length=lens, out=out, table=table, n_time=2, n_freq=2, mel_bins=F0, left=2, right=1, interval=1)
    for bad in (dict(mel_bins=6), dict(mel_bins=0), dict(left=3), dict(left=0, right=3), dict(right=-1), dict(interval=0), dict(n_time=63),
                dict(n_freq=-1), dict(x=x[0]), dict(mel_bins=16)):
        with pytest.raises(ValueError, match="pack_rows_aug"):
            native.pack_rows_aug(**dict(pack, **bad))
    raw, wide = torch.zeros(B, T, F0), torch.zeros(B * T, 4 * F0, dtype=torch.bfloat16)
    stack = dict(x=raw, in_len=lens, stats=None, left=2, right=1, interval=1, out_off=off, out_len=lens, max_out_len=T, out=wide, table=table,
                 n_time=2, n_freq=2)
    for bad in (dict(left=0), dict(right=-1), dict(interval=0), dict(n_time=70), dict(n_freq=-2), dict(x=raw[0])):
        with pytest.raises(ValueError, match="feat_stack_aug"):
            native.feat_stack_aug(**dict(stack, **bad))
    # ... and with every number in order, host tensors are refused: there is no CPU path
    for fn, kw in ((native.specaug_plan, plan), (native.pack_rows_aug, pack), (native.feat_stack_aug, stack)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            fn(**kw)


def test_policy_checks_raise_before_any_launch():
    from st_amd.features import stack_frames
    aug = SpecAugment(8, left=2, right=1, frame_rate=20)
    x, lens = torch.zeros(2, 12, 8), torch.tensor([12, 7])
    for left, right, rate in ((2, 0, 20), (3, 1, 20), (2, 1, 10)):
        with pytest.raises(ValueError, match="stack_frames: the policy"):
            stack_frames(x, lens, left, right, rate, augment=aug)
    with pytest.raises(ValueError, match="stack_frames: the policy"):
        stack_frames(torch.zeros(2, 12, 16), lens, 2, 1, 20, augment=aug)
    with pytest.raises(ValueError, match="columns"):
        aug.pack(torch.zeros(2, 12, 24), None)
    with pytest.raises(ValueError, match="gradient"):
        aug.pack(torch.zeros(2, 12, 32, requires_grad=True), None)


# ---- 4. the restatement itself ---------------------------------------------------------------------------------------------------
def test_reference_masks_lie_inside_the_utterance():
    """1,000 (seed, length) pairs: every mask inside [0, T_raw) / [0, F0), every width within its cap."""
    g = torch.Generator().manual_seed(7)
    seeds = torch.randint(0, 2 ** 31 - 1, (1000,), generator=g).tolist()
    lengths = torch.randint(1, 1500, (1000,), generator=g).tolist()
    lengths[:8] = [1, 2, 3, 4, 5, 9, 10, 1499]
    widths = 0
    for i, (seed, T) in enumerate(zip(seeds, lengths)):
        F0, tw, pm, fw = (80, 40, 200, 27) if i % 2 == 0 else (40, 100, 1000, 60)
        t = ref.plan(seed, 0x80000000 + i % 3, [T], F0, 3, tw, pm, 2, fw)[0]
        for j, (start, width) in enumerate(t.tolist()):
            n, cap = (T, min(tw, T * pm // 1000)) if j < 3 else (F0, min(fw, F0))
            assert 0 <= width <= cap and 0 <= start and start + width <= n, (seed, T, j, start, width)
            widths += width
    assert widths > 0
    assert ref.pick(0xFFFFFFFF, 10) == 9 and ref.pick(0, 10) == 0 and ref.pick(0x80000000, 3) == 1
    # the hash is the dropout hash: the tensor restatement the dropout tests use gives the same values
    from tests import _emul as em
    xs = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF] + seeds[:50]
    assert em._hash32(torch.tensor(xs, dtype=torch.int64)).tolist() == [ref.hash32(x) for x in xs]


def test_reference_stacking_rule_matches_the_feature_oracle():
    """stack_src (the rule both augmenting kernels share) against oracle/feature_oracle.py's concat_frame + subsampling."""
    import numpy as np
    from oracle import feature_oracle as fo
    for left, right, rate in ref.STACK_TRIPLES + [(8, 7, 10), (3, 1, 30)]:
        interval = 1 if rate == 10 else int(rate / 10)
        for T in (T for T in (1, 2, 5, 9, 23) if T > right):              # (the reference's own slicing needs T > right)
            x = (np.arange(T, dtype=np.float32)[:, None] + 1) * np.ones((1, 4), dtype=np.float32)        # frame t holds t + 1
            want = fo.subsampling(fo.concat_frame(x, left, right), rate)
            for r in range(want.shape[0]):
                for k in range(1 + left + right):
                    assert want[r, 4 * k] == ref.stack_src(k, r * interval, left, right, T) + 1, (left, right, rate, T, r, k)


def _some_width(tables, lo, hi):
    return any(int(t[:, lo:hi, 1].max(initial=0)) > 0 for t in tables)


def test_gpu_test_seeds_draw_masks():
    """For the seeds and shapes of tests/test_specaug_gpu.py: every policy whose caps allow it draws at least one time mask and
    one frequency mask of width > 0 (so none of those tests passes on empty masks) - at the seed and, where the test advances, the
    seeds after it."""
    def drawn(aug, seed, lengths, stacked):
        t = ref.plan_of(aug, seed, lengths, stacked)
        nt = aug.n_time_masks
        caps = [min(aug.time_width, ref.t_raw(n, *((aug.interval, aug.right) if stacked else (1, 0))) * aug.time_ratio_permille // 1000)
                for n in lengths]
        if nt and max(caps) > 0:
            assert _some_width([t], 0, nt), ("no time mask", seed)
        if aug.n_freq_masks and min(aug.freq_width, aug.mel_bins) > 0:
            assert _some_width([t], nt, aug.n_masks), ("no frequency mask", seed)
        return t
    for i, kw in enumerate(ref.PLAN_POLICIES):
        for seed in (ref.PLAN_SEED, ref.PLAN_SEED + 1):
            t = drawn(SpecAugment(salt=ref.PLAN_SALT + i, **kw), seed, ref.PLAN_LENGTHS, stacked="left" in kw)
            if kw.get("time_ratio_permille") == 0:
                assert int(t[:, :2, 1].max()) == 0
    for left, right, rate in ref.STACK_TRIPLES:
        drawn(SpecAugment(left=left, right=right, frame_rate=rate, salt=ref.STACK_SALT, **ref.STACK_POLICY), ref.STACK_SEED, ref.STACK_LENGTHS, False)
    for F0, left, right, rate, T in ref.PACK_CASES:
        drawn(SpecAugment(salt=ref.PACK_SALT, **ref.pack_policy(F0, left, right, rate)), ref.PACK_SEED, ref.pack_lengths(T), True)
    a = ref.AGREE
    drawn(SpecAugment(salt=ref.AGREE_SALT, **ref.agree_policy()), ref.AGREE_SEED, a["rows"], True)
    drawn(SpecAugment(salt=ref.ENCODER_SALT, **ref.ENCODER_POLICY), ref.ENCODER_SEED, ref.ENCODER_LENGTHS, True)
    from oracle import speech_transformer_oracle as orc
    from st_amd import synthetic
    lengths = synthetic.make_batch(**ref.STEP_BATCH)[2].tolist()
    tables = [drawn(SpecAugment(salt=ref.STEP_SALT, **ref.STEP_POLICY), ref.STEP_SEED + k, lengths, True) for k in range(1, 6)]
    assert all((tables[k] != tables[k + 1]).any() for k in range(4))         # the advancing seed changes the plan
    bk = ref.BUCKET
    for k, (t_max, t_min, seed) in enumerate(bk["batches"]):
        lengths = orc.synthetic_batch(4, t_max, bk["L_cap"], 80, 30, seed=seed, t_min=t_min, l_min=4)["in_len"].tolist()
        drawn(SpecAugment(salt=ref.BUCKET_SALT, **ref.STEP_POLICY), ref.BUCKET_SEED + k + 1, lengths, True)

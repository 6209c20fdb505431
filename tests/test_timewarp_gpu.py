"""-m gpu: SpecAugment's time warp on a real MI355X - the plan launch against the Python restatement of the draw
(tests/_timewarp_ref.py), the two warping feature kernels against its fp64 blend, and the policy inside the Encoder, a
captured TrainStep and bucket mode.

The tables are integers and compared exactly.  A warped element is the fp32 blend of two frames rounded to bf16: against the
fp64 blend rounded to bf16 it may differ by ONE bf16 ulp and no more - the fp32 blend is within ~2^-22 (relative) of the fp64
one, half a bf16 ulp is 2^-9, so the only possible difference is a rounding decision that fell the other way.  Where the map
has no fraction (fr == 0), and in every utterance that is not warped, the bits are those of the unwarped kernels.  Seeds, shapes
and policies come from tests/_timewarp_ref.py; tests/test_timewarp_cpu.py checks there that each input moves something."""
import numpy as np
import pytest
import torch

from st_amd import native as nv
from st_amd import rng
from st_amd.augment import SpecAugment
from st_amd.functional import Rows
from tests import _specaug_ref as sref
from tests import _timewarp_ref as ref
from tests._local import Guarded

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _device():
    return torch.device("cuda", torch.cuda.current_device())       # (rng keeps one seed per device NAME: the one tensors report)


def _seed(s):
    rng.manual_seed(s)
    assert int(rng.seed_tensor(_device())) == s
    return s


def _bits(t):
    """bf16 tensor -> int32 numpy array of its bit patterns (0 .. 65535)."""
    return (t.contiguous().view(torch.int16).cpu().numpy().astype(np.int32)) & 0xFFFF


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _tables_are(aug, seed, lengths, stacked, what):
    """last_masks and last_warp against the restatement -> (mask table, warp table)."""
    want_m, want_w = sref.plan_of(aug, seed, lengths, stacked), ref.warp_of(aug, seed, lengths, stacked)
    got_m, got_w = aug.last_masks.cpu().numpy(), aug.last_warp.cpu().numpy()
    assert got_w.dtype == np.int32 and got_w.shape == want_w.shape, (what, got_w.shape, want_w.shape)
    assert np.array_equal(got_w, want_w), "%s: the warp table %s differs from the restatement %s" % (what, got_w.tolist(), want_w.tolist())
    assert np.array_equal(got_m, want_m), "%s: the mask table differs from the restatement" % what
    return want_m, want_w


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", ref.PLAN_WARPS)
def test_plan_writes_both_tables(W):
    lengths, B = sref.PLAN_LENGTHS, len(sref.PLAN_LENGTHS)
    aug = SpecAugment(salt=sref.PLAN_SALT, time_warp=W, **ref.PLAN_POLICY)
    plain = SpecAugment(salt=sref.PLAN_SALT, **ref.PLAN_POLICY)
    lens = torch.tensor(lengths, dtype=I32, device="cuda")
    s = _seed(sref.PLAN_SEED)
    gm, gw = Guarded.vec(B * aug.n_masks * 2, I32, "cuda"), Guarded.vec(B * 2, I32, "cuda")
    table, warp = gm.view.view(B, aug.n_masks, 2), gw.view.view(B, 2)
    nv.specaug_plan_warp(rng.seed_tensor(_device()), aug.salt, lens, table, warp, aug.n_time_masks, aug.time_width,
                         aug.time_ratio_permille, aug.n_freq_masks, aug.freq_width, aug.mel_bins, W)
    want_w = ref.warp_of(aug, s, lengths, False)
    assert np.array_equal(warp.cpu().numpy(), want_w), (warp.tolist(), want_w.tolist())
    assert np.array_equal(table.cpu().numpy(), sref.plan_of(aug, s, lengths, False))
    gm.assert_intact("specaug_plan_warp: mask table"), gw.assert_intact("specaug_plan_warp: warp table")
    # the masks are those of the same policy without a warp, from its own entry point
    assert plain.plan(lens, stacked=False) is plain.last_masks and plain.last_warp is None
    assert torch.equal(plain.last_masks, table)
    # the policy's own launch, and the next step's
    aug.plan(lens, stacked=False)
    _tables_are(aug, s, lengths, False, "W %d" % W)
    rng.advance()
    aug.plan(lens, stacked=False)
    _, after = _tables_are(aug, s + 1, lengths, False, "W %d after advance()" % W)
    assert not np.array_equal(after, want_w)
    # no masks at all: the warp table alone
    bare = SpecAugment(80, n_time_masks=0, n_freq_masks=0, salt=sref.PLAN_SALT, time_warp=W)
    bare.plan(lens, stacked=False)
    assert np.array_equal(bare.last_warp.cpu().numpy(), after) and bare.last_masks.shape == (B, 0, 2)


# ---- the pack ---------------------------------------------------------------------------------------------------------------------
def _pack_input(F0, left, interval, lens, T, gen):
    """-> (x fp32 [B, T, Fd] uniform in [1, 2) everywhere, the sourced slots of every utterance a consistent stacking of its raw
    frames; the list of those raw frames, fp32 [n, F0] each)."""
    B, Fd = len(lens), F0 * (1 + left)
    x = torch.rand(B, T, Fd, generator=gen) + 1.0
    raws = []
    for b, l in enumerate(lens):
        n = sref.t_raw(l, interval, 0)
        raw = (torch.rand(n, F0, generator=gen) + 1.0).numpy()
        x[b, :l] = torch.from_numpy(ref.stack_rows(raw, l, left, 0, interval, fill=x[b, :l].numpy()))
        raws.append(raw)
    return x, raws


def _expected_pack(x, raws, lens, aug, masks, warps):
    """The restatement of the warping pack in fp64 -> (want fp64 [rows, Fd], exact bool [rows, Fd]: elements that take no blend,
    masked bool [rows, Fd], shown int64 [rows, Fd]: b * 2^20 + output frame, -1 without a source)."""
    F0, left, interval = aug.mel_bins, aug.left, aug.interval
    want, exact, masked, shown = [], [], [], []
    for b, l in enumerate(lens):
        n = raws[b].shape[0]
        c, cp = warps[b].tolist()
        g, fr = ref.positions(n, c, cp)
        rows = ref.stack_rows(ref.warp64(raws[b], c, cp), l, left, 0, interval, fill=x[b, :l].double().numpy())
        sh = ref.shown_frame(l, F0, left, 0, interval, n)
        m = sref.stacked_mask(masks[b], aug.n_time_masks, l, F0, left, 0, interval, n)
        rows[m] = 0.0
        want.append(rows), masked.append(m)
        exact.append((sh < 0) | (np.append(fr, 0)[sh] == 0))
        shown.append(np.where(sh >= 0, sh + (b << 20), -1))
    return np.concatenate(want), np.concatenate(exact), np.concatenate(masked), np.concatenate(shown)


@pytest.mark.parametrize("ci", range(len(ref.PACK_CASES)))
def test_pack_rows_warp_values(ci):
    F0, left, right, rate, T = ref.PACK_CASES[ci]
    lens = sref.pack_lengths(T)
    aug = SpecAugment(salt=sref.PACK_SALT, **ref.pack_policy(F0, left, right, rate))
    interval, Fd = aug.interval, F0 * (1 + left)
    x, raws = _pack_input(F0, left, interval, lens, T, torch.Generator().manual_seed(200 + ci))
    rows = Rows.packed(torch.tensor(lens), "cuda")
    s = _seed(sref.PACK_SEED)
    gd = Guarded(rows.total, Fd, BF16, "cuda", pad_rows=4, pad_cols=(0, 0))
    table = aug.plan(rows.len, stacked=True)
    masks, warps = _tables_are(aug, s, lens, True, "pack case %d" % ci)
    nv.pack_rows_warp(x.cuda(), rows.off, rows.len, gd.view, table, aug.last_warp, aug.n_time_masks, aug.n_freq_masks, F0, left, 0, interval)
    want, exact, masked, shown = _expected_pack(x, raws, lens, aug, masks, warps)
    got = _bits(gd.view)
    diff = np.abs(got - ref.bf16_bits(np.where(masked, 1.0, want)))            # (all values lie in [1, 2]: bit patterns are ordered)
    diff[masked] = 0
    print("pack_rows_warp F %d (%d bins, left %d, interval %d): %d of %d elements differ from the fp64 blend (max %d ulp), %d masked, %d without a blend"
          % (Fd, F0, left, interval, int((diff > 0).sum()), diff.size, int(diff.max()), int(masked.sum()), int(exact.sum())))
    assert int(diff.max()) <= 1, "an element is %d bf16 ulps from the fp64 blend, at (row, column) %s" % (int(diff.max()), np.argwhere(diff > 1)[:4].tolist())
    assert 0 < int(masked.sum()) < want.size and int((~exact).sum()) > 0
    # masked elements are +0.0 and nothing else is zero
    assert (got[masked] == 0).all() and int((got == 0).sum()) == int(masked.sum())
    # no blend (identity utterances, fr == 0, slots without a source): the bits of st_pack_rows on the host-warped, host-masked input
    plain = torch.full((rows.total, Fd), float("nan"), dtype=BF16, device="cuda")
    host = torch.zeros(len(lens), T, Fd)
    o = 0
    for b, l in enumerate(lens):
        host[b, :l] = torch.from_numpy(want[o:o + l].astype(np.float32))
        o += l
    nv.pack_rows(host.cuda(), rows.off, rows.len, plain)
    n_exact_diff = int((got[exact] != _bits(plain)[exact]).sum())
    assert n_exact_diff == 0, "%d elements that take no blend differ from st_pack_rows" % n_exact_diff
    o = 0
    for b, l in enumerate(lens):
        if warps[b].tolist() == [0, 0]:
            assert np.array_equal(got[o:o + l], _bits(plain)[o:o + l]), "identity utterance %d" % b
        o += l
    gd.assert_intact("pack_rows_warp case %d" % ci)
    # every (row, slot) that shows the same output frame holds the same bits
    if left:
        first = {}
        g3, s3 = got.reshape(-1, 1 + left, F0), shown.reshape(-1, 1 + left, F0)[:, :, 0]
        for r, k in zip(*np.nonzero(s3 >= 0)):
            other = first.setdefault(int(s3[r, k]), (r, k))
            assert np.array_equal(g3[r, k], g3[other]), "frame %d differs between (row, slot) %s and %s" % (int(s3[r, k]) & 0xFFFFF, (r, k), other)
        assert len(first) < int((s3 >= 0).sum())


@pytest.mark.parametrize("ci", range(len(ref.RAMP_CASES)))
def test_pack_rows_warp_positions(ci):
    """Input frame t holds 8 t in every bin, no masks: output frame u is bf16(8 (g + fr / 65536)) EXACTLY (8 g + fr / 8192 fits
    fp32 for g < 32, so the blend itself is exact) - a small error in fr, which the value test's ulp hides, shows here."""
    left, rate, lens = ref.RAMP_CASES[ci]
    F0 = 8
    aug = SpecAugment(F0, 0, 0, 0, 0, 0, left, 0, rate, ref.RAMP_SALT, ref.RAMP_WARP)
    interval, Fd, T = aug.interval, F0 * (1 + left), max(lens) + 1
    x = torch.zeros(len(lens), T, Fd)
    for b, l in enumerate(lens):
        n = sref.t_raw(l, interval, 0)
        raw = (8.0 * np.arange(n, dtype=np.float32))[:, None] * np.ones((1, F0), dtype=np.float32)
        x[b, :l] = torch.from_numpy(ref.stack_rows(raw, l, left, 0, interval))
    rows = Rows.packed(torch.tensor(lens), "cuda")
    s = _seed(ref.RAMP_SEED)
    gd = Guarded(rows.total, Fd, BF16, "cuda", pad_rows=4, pad_cols=(0, 0))
    packed = aug.pack(x.cuda(), rows)
    _, warps = _tables_are(aug, s, lens, True, "ramp case %d" % ci)
    nv.pack_rows_warp(x.cuda(), rows.off, rows.len, gd.view, aug.last_masks, aug.last_warp, 0, 0, F0, left, 0, interval)
    assert _same_bits(packed, gd.view)
    gd.assert_intact("pack_rows_warp, ramp case %d" % ci)
    got, o, moved = gd.view.float().cpu().numpy().astype(np.float64), 0, 0
    for b, l in enumerate(lens):
        n = sref.t_raw(l, interval, 0)
        g, fr = ref.positions(n, *warps[b].tolist())
        frames = ref.bf16_round(np.maximum(8.0 * (g + fr / 65536.0), 2.0 ** -100))
        frames[(g == 0) & (fr == 0)] = 0.0
        assert (np.diff(frames) >= 0).all()
        want = ref.stack_rows(frames[:, None] * np.ones((1, F0)), l, left, 0, interval)
        assert np.array_equal(got[o:o + l], want), "utterance %d: pair %s, first wrong (row, column) %s" % (
            b, warps[b].tolist(), np.argwhere(got[o:o + l] != want)[:4].tolist())
        moved += int((fr > 0).sum())
        o += l
    assert moved > 0


# ---- the front-end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(sref.STACK_TRIPLES)))
@pytest.mark.parametrize("with_stats", [False, True])
def test_feat_stack_warp_against_the_restatement(ci, with_stats):
    """CMVN in fp64, then the blend, then the masks, then the stacking.  With statistics the bound is one bf16 ulp at the LARGER
    normalised operand, 2^-7 max(|a'|, |b'|): after CMVN the operands may cancel, and a bound relative to the result would mean
    nothing.  Without statistics the per-result bound of the pack test applies - one bf16 ulp against the fp64 blend rounded to
    bf16 -, and as there its derivation needs operands that do not cancel: those runs take |x| + 1 for the input.  An utterance
    that is not warped equals st_feat_stack's rows, masked, bit for bit."""
    from st_amd.features import stack_frames
    from tests import test_features_cpu as tf
    left, right, rate = sref.STACK_TRIPLES[ci]
    x3, lens3, stats3 = tf._case(left, right, rate, with_stats, 10 + ci)
    assert lens3.tolist() == sref.STACK_LENGTHS
    B, T, F = len(ref.STACK_LENGTHS), x3.shape[1], x3.shape[2]
    g = torch.Generator().manual_seed(50 + ci)
    x = torch.cat([x3, torch.randn(1, T, F, generator=g) * 2 + 0.5])
    if not with_stats:
        x = x.abs() + 1.0
    for b, n in enumerate(ref.STACK_LENGTHS):
        x[b, n:] = 0
    lens = torch.tensor(ref.STACK_LENGTHS)
    stats = None if stats3 is None else torch.cat([stats3, stats3[:1]])
    aug = SpecAugment(left=left, right=right, frame_rate=rate, salt=sref.STACK_SALT, time_warp=ref.STACK_WARP, **sref.STACK_POLICY)
    interval = aug.interval
    s = _seed(sref.STACK_SEED)
    xd, sd = x.cuda(), None if stats is None else stats.cuda()
    got_api, rows = stack_frames(xd, lens, left, right, rate, sd, augment=aug)
    masks, warps = _tables_are(aug, s, lens.tolist(), False, "stack_frames(augment=...)")
    width = F * (1 + left + right)
    gd = Guarded(rows.total, width, BF16, "cuda")
    gd.view.zero_()
    nv.feat_stack_warp(xd, lens.to("cuda", I32), sd, left, right, interval, rows.off, rows.len, rows.max_len, gd.view, aug.last_masks,
                       aug.last_warp, aug.n_time_masks, aug.n_freq_masks)
    gd.assert_intact("feat_stack_warp (%d, %d, %d)" % (left, right, rate))
    assert _same_bits(got_api, gd.view)
    got_all = gd.view.float().cpu().numpy().astype(np.float64)
    # the plain kernel on the same input: what an element that takes no blend must equal, bit for bit
    plain, _ = stack_frames(xd, lens, left, right, rate, sd)
    plain_all = plain.float().cpu().numpy().astype(np.float64)
    o, worst, blended, hit, n_ulp = 0, 0.0, 0, 0, 0
    for b, (n, l) in enumerate(zip(lens.tolist(), rows.lens_host.tolist())):
        raw = x[b, :n].double().numpy()
        if stats is not None:
            st = stats[b].double().numpy()
            mean = st[0, :F] / st[0, F]
            raw = (raw - mean) / np.sqrt(st[1, :F] / st[0, F] - mean * mean)
        c, cp = warps[b].tolist()
        gs, fr = ref.positions(n, c, cp)
        nxt = raw[np.minimum(gs + 1, n - 1)]
        scale = np.maximum(np.abs(raw[gs]), np.where(fr[:, None] > 0, np.abs(nxt), 0.0))           # max(|a'|, |b'|) per output frame
        m = sref.raw_mask(masks[b], aug.n_time_masks, n, F)
        warped = np.where(m, 0.0, ref.warp64(raw, c, cp))
        want = ref.stack_rows(warped, l, left, right, interval)
        bound = ref.stack_rows(np.where(m, 0.0, scale) * 2.0 ** -7, l, left, right, interval)
        got = got_all[o:o + l]
        mm = ref.stack_rows(m.astype(np.float64), l, left, right, interval) > 0
        sh = ref.shown_frame(l, F, left, right, interval, n)
        noblend = (sh < 0) | (np.append(fr, 0)[sh] == 0)
        if with_stats:
            err = np.abs(got - want)
            assert (err <= bound).all(), "utterance %d: |got - want| %.3e > %.3e at (row, column) %s" % (
                b, err[err > bound].max(), bound[err > bound].min(), np.argwhere(err > bound)[:4].tolist())
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        else:
            live = want > 0                                    # (every input is >= 1: what is 0 is masked or has no source frame)
            ulps = np.abs(_bits(gd.view[o:o + l]) - ref.bf16_bits(np.where(live, want, 1.0)))
            ulps[~live] = _bits(gd.view[o:o + l])[~live]       # ... and must be +0.0
            assert int(ulps.max()) <= 1, "utterance %d: %d bf16 ulps from the fp64 blend at (row, column) %s" % (
                b, int(ulps.max()), np.argwhere(ulps > 1)[:4].tolist())
            n_ulp += int((ulps > 0).sum())
            worst = max(worst, float(ulps.max()))
        assert (_bits(gd.view[o:o + l])[mm] == 0).all()        # masked: +0.0
        if (c, cp) == (0, 0):
            same = plain_all[o:o + l].copy()
            same[mm] = 0.0
            assert np.array_equal(got, same), "identity utterance %d differs from st_feat_stack" % b
        blended += int((~noblend & ~mm).sum())
        hit += int(mm.sum())
        o += l
    print("feat_stack_warp (%d, %d, %d) stats %s: worst %s %.3f, %d blended elements (%d differ by an ulp), %d masked"
          % (left, right, rate, with_stats, "|err| / bound" if with_stats else "ulps", worst, blended, n_ulp, hit))
    assert blended > 0 and hit > 0


# ---- the two paths agree ------------------------------------------------------------------------------------------------------------
def test_the_two_paths_agree():
    """right = 0, raw length (rows - 1) * interval + 1, raw input rounded to bf16 first (so the plainly stacked rows hold the raw
    values exactly): warping the raw frames in the front-end == warping the stacked rows in the pack, at one seed and salt."""
    from st_amd.features import stack_frames
    a = sref.AGREE
    aug = SpecAugment(salt=sref.AGREE_SALT, **ref.agree_policy())
    raw_lens = torch.tensor([(n - 1) * aug.interval + 1 for n in ref.AGREE_ROWS])
    B, T, F = len(ref.AGREE_ROWS), int(raw_lens.max()) + 1, aug.mel_bins
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, T, F, generator=g) + 3.0).bfloat16().float()
    for b in range(B):
        x[b, raw_lens[b]:] = 0
    s = _seed(sref.AGREE_SEED)
    front, rows = stack_frames(x.cuda(), raw_lens, a["left"], a["right"], a["frame_rate"], augment=aug)
    t_front, w_front = aug.last_masks.clone(), aug.last_warp.clone()
    assert rows.lens_host.tolist() == ref.AGREE_ROWS
    _tables_are(aug, s, raw_lens.tolist(), False, "front-end path")
    plain, _ = stack_frames(x.cuda(), raw_lens, a["left"], a["right"], a["frame_rate"])
    padded = torch.zeros(B, rows.max_len, plain.shape[1], device="cuda")
    for b, (o, n) in enumerate(zip(rows.off.tolist(), ref.AGREE_ROWS)):
        padded[b, :n] = plain[o:o + n].float()
    packed = aug.pack(padded, rows)
    assert torch.equal(aug.last_masks, t_front) and torch.equal(aug.last_warp, w_front)
    _tables_are(aug, s, ref.AGREE_ROWS, True, "pack path")
    assert _same_bits(packed, front.contiguous())
    # both differ from the unwarped rows - masked or not
    unwarped = SpecAugment(salt=sref.AGREE_SALT, **sref.agree_policy())
    _seed(sref.AGREE_SEED)
    assert not _same_bits(packed, unwarped.pack(padded, rows)) and not _same_bits(packed, plain.contiguous())
    assert torch.equal(unwarped.last_masks, t_front) and unwarped.last_warp is None


# ---- the Encoder --------------------------------------------------------------------------------------------------------------------
def _encoder():
    from transformer.Models import Encoder
    torch.manual_seed(3)
    return Encoder(80, 64, n_layers=2, n_head=4, d_k=64, d_v=64, d_model=256, d_inner_hid=512, dropout=0.1).cuda()


def test_encoder_eval_ignores_the_policy_and_train_warps_the_input():
    """train(): the policy on x == no policy on the host-warped, host-masked x under the same seed, bit for bit.  The host input
    is warped with the kernel's fp32 formula (_timewarp_ref.warp32: difference, product and sum rounded one by one, which is
    what st_warp_blend does), so the mirror is exact and the encoder is fed through its ordinary padded input."""
    enc = _encoder()
    lens = torch.tensor(sref.ENCODER_LENGTHS)
    B, T = len(lens), int(lens.max())
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, T, 80, generator=g) + 3.0
    for b in range(B):
        x[b, lens[b]:] = 0
    x = x.cuda()
    aug = SpecAugment(salt=sref.ENCODER_SALT, time_warp=ref.ENCODER_WARP, **sref.ENCODER_POLICY)
    enc.eval()
    with torch.no_grad():
        plain = enc(x, lens)[0]
        enc.spec_augment = aug
        assert torch.equal(enc(x, lens)[0], plain) and aug.last_masks is None and aug.last_warp is None      # bit for bit, and no plan launch
    enc.train()
    enc.use_row_chains = False
    s = _seed(sref.ENCODER_SEED)
    with torch.no_grad():
        got = enc(x, lens)[0]
    masks, warps = _tables_are(aug, s, sref.ENCODER_LENGTHS, True, "Encoder.forward_rows")
    xh, xm = x.cpu(), x.cpu().clone()
    for b, n in enumerate(sref.ENCODER_LENGTHS):
        w = ref.warp32(xh[b, :n].numpy(), *warps[b].tolist())
        w[sref.raw_mask(masks[b], aug.n_time_masks, n, 80)] = 0.0
        xm[b, :n] = torch.from_numpy(w)
    assert not torch.equal(xm, xh)
    enc.spec_augment = None
    _seed(sref.ENCODER_SEED)
    with torch.no_grad():
        want = enc(xm.cuda(), lens)[0]
        _seed(sref.ENCODER_SEED)
        unwarped = enc(x, lens)[0]
    assert torch.equal(got, want), "rel %.3e" % float((got - want).norm() / want.norm())
    assert not torch.equal(got, unwarped)
    # ... and not the masks alone
    enc.spec_augment = SpecAugment(salt=sref.ENCODER_SALT, **sref.ENCODER_POLICY)
    _seed(sref.ENCODER_SEED)
    with torch.no_grad():
        assert not torch.equal(enc(x, lens)[0], got)
    assert torch.equal(enc.spec_augment.last_masks.cpu(), torch.from_numpy(masks))


# ---- the step drivers -----------------------------------------------------------------------------------------------------------------
def _small_step(policy_salt, time_warp, **step_kw):
    """(The small model of tests/test_specaug_gpu.py::_small_step, with a warping policy.)"""
    from st_amd.trainer import TrainStep
    from transformer.Models import Transformer
    from transformer.Optim import ScheduledOptim
    from transformer.Utils import AttrDict, init_parameters
    cfg = AttrDict(dict(feature_dim=80, max_inputs_length=200, max_target_length=32, num_enc_layer=2, num_dec_layer=2, n_heads=4, d_k=32,
                        d_v=32, d_model=128, d_inner_hid=256, dropout=0.1, vocab_size=30))
    torch.manual_seed(0)
    model = Transformer(cfg).cuda()
    init_parameters(model)
    model.train()
    aug = model.encoder.spec_augment = SpecAugment(salt=policy_salt, time_warp=time_warp, **sref.STEP_POLICY)
    opt = ScheduledOptim(model, 128, AttrDict(n_warmup_steps=4000))
    return model, aug, TrainStep(model, opt, 30, 5.0, use_graph=True, graph_warmup=1, **step_kw)


def test_captured_step_draws_a_new_warp_on_every_replay():
    from st_amd import synthetic
    inputs, targets, in_len, tgt_len, truth = synthetic.make_batch(**sref.STEP_BATCH)
    model, aug, step = _small_step(sref.STEP_SALT, ref.STEP_WARP)
    x, t, gt = inputs.cuda(), targets.cuda(), truth.cuda()
    _seed(sref.STEP_SEED)
    tables, static = [], None
    for k in range(1, 5):                       # one eager step, then the capture and two replays
        loss, _ = step(x, in_len, t, tgt_len, gt)
        assert np.isfinite(float(loss)), (k, float(loss))
        s = int(rng.seed_tensor(_device()))
        assert s == sref.STEP_SEED + k
        _tables_are(aug, s, in_len.tolist(), True, "step %d" % k)
        if k >= 2:
            assert static is None or aug.last_warp.data_ptr() == static        # a static tensor that every replay rewrites
            static = aug.last_warp.data_ptr()
            tables.append(aug.last_warp.cpu().clone())
    assert len(step._graphs) == 1
    assert len({tuple(t.flatten().tolist()) for t in tables}) >= 2


def test_bucket_mode_reads_the_lengths_from_the_device():
    from oracle import speech_transformer_oracle as orc
    bk = sref.BUCKET
    model, aug, step = _small_step(sref.BUCKET_SALT, ref.BUCKET_WARP, bucket=(bk["T_cap"], bk["L_cap"]))
    _seed(sref.BUCKET_SEED)
    for k, (t_max, t_min, seed) in enumerate(bk["batches"]):
        b = orc.synthetic_batch(4, t_max, bk["L_cap"], 80, 30, seed=seed, t_min=t_min, l_min=4)
        T, L = int(b["in_len"].max()), int(b["tgt_len"].max())
        loss, _ = step(b["x"][:, :T].cuda(), b["in_len"], b["tokens"][:, :L].cuda(), b["tgt_len"], b["gt"][:, :L].cuda())
        assert np.isfinite(float(loss)), (k, float(loss))
        s = int(rng.seed_tensor(_device()))
        assert s == sref.BUCKET_SEED + k + 1
        table = aug.last_warp.cpu().tolist()
        for u, n in enumerate(b["in_len"].tolist()):
            c, cp = table[u]
            assert (c, cp) == (0, 0) or (1 <= cp <= n - 2 and 1 <= c <= n - 2), (k, u, n, c, cp)
        _tables_are(aug, s, b["in_len"].tolist(), True, "bucket batch %d" % k)
    assert sum(st.cap is not None for st in step._buckets.values()) >= 1

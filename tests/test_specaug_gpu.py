"""-m gpu: SpecAugment on a real MI355X - the plan launch against the Python restatement of the draw (tests/_specaug_ref.py),
the two augmenting feature kernels against the plain kernels on host-masked input, and the policy inside the Encoder, a
captured TrainStep and bucket mode.

Every comparison is bit for bit: the masks are integers, and an unmasked element takes exactly the conversions it takes in
st_pack_rows / st_feat_stack (a masked one is +0.0 in both).  Seeds, shapes and policies come from tests/_specaug_ref.py;
tests/test_specaug_cpu.py::test_gpu_test_seeds_draw_masks checks there that none of them draws only empty masks."""
import numpy as np
import pytest
import torch

from st_amd import native as nv
from st_amd import rng
from st_amd.augment import SpecAugment
from st_amd.functional import Rows
from tests import _specaug_ref as ref
from tests._local import Guarded

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _device():
    return torch.device("cuda", torch.cuda.current_device())       # (rng keeps one seed per device NAME: the one tensors report)


def _seed(s):
    rng.manual_seed(s)
    assert int(rng.seed_tensor(_device())) == s
    return s


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _table_is(aug, want, what):
    got = aug.last_masks.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: the plan differs from the restatement at %s" % (what, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("i", range(len(ref.PLAN_POLICIES)))
def test_plan_matches_the_restatement(i):
    kw = ref.PLAN_POLICIES[i]
    aug, stacked = SpecAugment(salt=ref.PLAN_SALT + i, **kw), "left" in kw
    lens = torch.tensor(ref.PLAN_LENGTHS, dtype=I32, device="cuda")
    s = _seed(ref.PLAN_SEED)
    # the table inside a guarded buffer: the launch writes its B * masks * 2 integers and nothing else
    gd = Guarded.vec(len(ref.PLAN_LENGTHS) * aug.n_masks * 2, I32, "cuda")
    table = gd.view.view(len(ref.PLAN_LENGTHS), aug.n_masks, 2)
    geometry = dict(interval=aug.interval, right=aug.right) if stacked else {}
    nv.specaug_plan(rng.seed_tensor(_device()), aug.salt, lens, table, aug.n_time_masks, aug.time_width, aug.time_ratio_permille,
                    aug.n_freq_masks, aug.freq_width, aug.mel_bins, **geometry)
    want = ref.plan_of(aug, s, ref.PLAN_LENGTHS, stacked)
    assert np.array_equal(table.cpu().numpy(), want), "policy %d: guarded plan differs" % i
    gd.assert_intact("specaug_plan, policy %d" % i)
    # the policy's own launch, and the next step's
    assert aug.plan(lens, stacked) is aug.last_masks
    _table_is(aug, want, "policy %d" % i)
    rng.advance()
    aug.plan(lens, stacked)
    after = ref.plan_of(aug, s + 1, ref.PLAN_LENGTHS, stacked)
    _table_is(aug, after, "policy %d after advance()" % i)
    if aug.n_masks and not (kw.get("time_ratio_permille") == 0 and aug.n_freq_masks == 0):
        assert not np.array_equal(want, after)
    if kw.get("time_ratio_permille") == 0:
        assert int(aug.last_masks[:, :aug.n_time_masks, 1].max()) == 0


@pytest.mark.parametrize("ci", range(len(ref.STACK_TRIPLES)))
@pytest.mark.parametrize("with_stats", [False, True])
def test_feat_stack_aug_equals_feat_stack_of_masked_input(ci, with_stats):
    """st_feat_stack_aug(x) == st_feat_stack(host-masked x), into a strided guarded view.  Host-masked: a masked element is 0
    - with CMVN statistics it is the fp32 mean st_feat_stack itself computes (sum / count: one correctly rounded division on
    either side), which CMVN maps to exactly +0.0, the value the mask stands for (the mean after CMVN)."""
    from st_amd.features import stack_frames
    from tests import test_features_cpu as tf
    left, right, rate = ref.STACK_TRIPLES[ci]
    interval = 1 if rate == 10 else int(rate / 10)
    x, lens, stats = tf._case(left, right, rate, with_stats, 10 + ci)
    assert lens.tolist() == ref.STACK_LENGTHS
    B, T, F = x.shape
    aug = SpecAugment(left=left, right=right, frame_rate=rate, salt=ref.STACK_SALT, **ref.STACK_POLICY)
    s = _seed(ref.STACK_SEED)
    xd, sd = x.cuda(), None if stats is None else stats.cuda()
    got_api, rows = stack_frames(xd, lens, left, right, rate, sd, augment=aug)
    want_table = ref.plan_of(aug, s, lens.tolist(), stacked=False)
    _table_is(aug, want_table, "stack_frames(augment=...)")
    xm = xd.clone()
    for b in range(B):
        m = torch.from_numpy(ref.raw_mask(want_table[b], aug.n_time_masks, T, F)).cuda()
        fill = torch.zeros(T, F, device="cuda") if sd is None else (sd[b, 0, :F] / sd[b, 0, F]).expand(T, F)
        xm[b] = torch.where(m, fill, xm[b])
    want, rows2 = stack_frames(xm, lens, left, right, rate, sd)
    width = F * (1 + left + right)
    gd = Guarded(rows.total, width, BF16, "cuda")
    gd.view.zero_()
    nv.feat_stack_aug(xd, lens.to("cuda", I32), sd, left, right, interval, rows.off, rows.len, rows.max_len, gd.view, aug.last_masks,
                      aug.n_time_masks, aug.n_freq_masks)
    n_diff = int((gd.view.view(torch.int16) != want.contiguous().view(torch.int16)).sum()) if gd.view.shape == want.shape else -1
    print("feat_stack_aug (%d, %d, %d) stats %s: %d elements differ" % (left, right, rate, with_stats, n_diff))
    assert _same_bits(gd.view, want), "feat_stack_aug differs from feat_stack of the masked input (%d, %d, %d): %d elements" % (left, right, rate, n_diff)
    gd.assert_intact("feat_stack_aug (%d, %d, %d)" % (left, right, rate))
    assert _same_bits(got_api, want)
    # ... and what lies under a mask is +0.0, whatever the statistics; something does
    o, hit = 0, 0
    for b, n in enumerate(rows.lens_host.tolist()):
        m = torch.from_numpy(ref.stacked_mask(want_table[b], aug.n_time_masks, n, F, left, right, interval, int(lens[b])))
        under = gd.view[o:o + n].cpu().view(torch.int16)[m]
        assert not bool((under != 0).any())
        hit += int(m.sum())
        o += n
    assert hit > 0


@pytest.mark.parametrize("ci", range(len(ref.PACK_CASES)))
def test_pack_rows_aug_equals_pack_rows_of_masked_input(ci):
    F0, left, right, rate, T = ref.PACK_CASES[ci]
    interval = 1 if rate == 10 else int(rate / 10)
    lens = ref.pack_lengths(T)
    B, Fd = len(lens), F0 * (1 + left + right)
    aug = SpecAugment(salt=ref.PACK_SALT, **ref.pack_policy(F0, left, right, rate))
    g = torch.Generator().manual_seed(100 + ci)
    x = torch.randn(B, T, Fd, generator=g) + 3.0           # no zero anywhere, padding frames included: every zero in the output is a mask
    rows = Rows.packed(torch.tensor(lens), "cuda")
    s = _seed(ref.PACK_SEED)
    gd = Guarded(rows.total, Fd, BF16, "cuda", pad_rows=4, pad_cols=(0, 0))
    table = aug.plan(rows.len, stacked=True)
    want_table = ref.plan_of(aug, s, lens, stacked=True)
    _table_is(aug, want_table, "pack case %d" % ci)
    nv.pack_rows_aug(x.cuda(), rows.off, rows.len, gd.view, table, aug.n_time_masks, aug.n_freq_masks, F0, left, right, interval)
    xm, hit = x.clone(), 0
    for b, n in enumerate(lens):
        m = torch.from_numpy(ref.stacked_mask(want_table[b], aug.n_time_masks, n, F0, left, right, interval, ref.t_raw(n, interval, right)))
        xm[b, :n][m] = 0.0
        hit += int(m.sum())
    assert 0 < hit < sum(lens) * Fd
    want = torch.full((rows.total, Fd), float("nan"), dtype=BF16, device="cuda")
    nv.pack_rows(xm.cuda(), rows.off, rows.len, want)
    n_diff = int((gd.view.view(torch.int16) != want.view(torch.int16)).sum())
    print("pack_rows_aug F %d (%d bins, left %d, right %d, interval %d): %d masked elements, %d differ" % (Fd, F0, left, right, interval, hit, n_diff))
    assert _same_bits(gd.view, want), "pack_rows_aug differs from pack_rows of the masked input: %d elements" % n_diff
    gd.assert_intact("pack_rows_aug case %d" % ci)
    assert int((gd.view == 0).sum()) == hit


def test_the_two_paths_agree():
    """right = 0, raw length (n - 1) * interval + 1: masking the raw frames in the front-end == masking the stacked rows in
    the pack, at one seed and salt."""
    from st_amd.features import stack_frames
    a = ref.AGREE
    aug = SpecAugment(salt=ref.AGREE_SALT, **ref.agree_policy())
    raw_lens = torch.tensor([(n - 1) * aug.interval + 1 for n in a["rows"]])
    B, T, F = len(a["rows"]), int(raw_lens.max()) + 1, aug.mel_bins
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, F, generator=g) + 3.0
    for b in range(B):
        x[b, raw_lens[b]:] = 0
    s = _seed(ref.AGREE_SEED)
    front, rows = stack_frames(x.cuda(), raw_lens, a["left"], a["right"], a["frame_rate"], augment=aug)
    t_front = aug.last_masks.clone()
    assert rows.lens_host.tolist() == a["rows"]
    plain, _ = stack_frames(x.cuda(), raw_lens, a["left"], a["right"], a["frame_rate"])
    padded = torch.zeros(B, rows.max_len, plain.shape[1], device="cuda")
    for b, (o, n) in enumerate(zip(rows.off.tolist(), a["rows"])):
        padded[b, :n] = plain[o:o + n].float()
    packed = aug.pack(padded, rows)
    assert torch.equal(aug.last_masks, t_front)
    _table_is(aug, ref.plan_of(aug, s, a["rows"], stacked=True), "pack path")
    assert _same_bits(packed, front.contiguous())
    assert not _same_bits(packed, plain.contiguous())


def _encoder():
    from transformer.Models import Encoder
    torch.manual_seed(3)
    return Encoder(80, 64, n_layers=2, n_head=4, d_k=64, d_v=64, d_model=256, d_inner_hid=512, dropout=0.1).cuda()


def test_encoder_eval_ignores_the_policy_and_train_masks_the_input():
    enc = _encoder()
    lens = torch.tensor(ref.ENCODER_LENGTHS)
    B, T = len(lens), int(lens.max())
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, T, 80, generator=g) + 3.0
    for b in range(B):
        x[b, lens[b]:] = 0
    x = x.cuda()
    aug = SpecAugment(salt=ref.ENCODER_SALT, **ref.ENCODER_POLICY)
    enc.eval()
    with torch.no_grad():
        plain = enc(x, lens)[0]
        enc.spec_augment = aug
        assert torch.equal(enc(x, lens)[0], plain) and aug.last_masks is None        # bit for bit, and no plan launch
    # train(): the policy on x == no policy on the host-masked x under the same seed (the dropout salts are not disturbed).
    # The per-GEMM path: its forward has one accumulation order.
    enc.train()
    enc.use_row_chains = False
    s = _seed(ref.ENCODER_SEED)
    with torch.no_grad():
        got = enc(x, lens)[0]
    want_table = ref.plan_of(aug, s, ref.ENCODER_LENGTHS, stacked=True)
    _table_is(aug, want_table, "Encoder.forward_rows")
    xm, hit = x.clone(), 0
    for b, n in enumerate(ref.ENCODER_LENGTHS):
        m = torch.from_numpy(ref.raw_mask(want_table[b], aug.n_time_masks, n, 80)).cuda()
        xm[b, :n][m] = 0.0
        hit += int(m.sum())
    assert hit > 0
    enc.spec_augment = None
    _seed(ref.ENCODER_SEED)
    with torch.no_grad():
        want = enc(xm, lens)[0]
        _seed(ref.ENCODER_SEED)
        unmasked = enc(x, lens)[0]
    assert torch.equal(got, want), "rel %.3e" % float((got - want).norm() / want.norm())
    assert not torch.equal(got, unmasked)
    # an input that wants a gradient, or another width, is refused
    enc.spec_augment = aug
    with pytest.raises(ValueError, match="gradient"):
        enc(x.clone().requires_grad_(True), lens)
    enc.spec_augment = SpecAugment(40)
    with pytest.raises(ValueError, match="columns"):
        enc(x, lens)


def _small_step(policy_salt, **step_kw):
    from st_amd.trainer import TrainStep
    from transformer.Models import Transformer
    from transformer.Optim import ScheduledOptim
    from transformer.Utils import AttrDict, init_parameters
    cfg = AttrDict(dict(feature_dim=80, max_inputs_length=200, max_target_length=32, num_enc_layer=2, num_dec_layer=2, n_heads=4, d_k=32,
                        d_v=32, d_model=128, d_inner_hid=256, dropout=0.1, vocab_size=30))          # test_graph_step_matches_eager_step's
    torch.manual_seed(0)
    model = Transformer(cfg).cuda()
    init_parameters(model)
    model.train()
    aug = model.encoder.spec_augment = SpecAugment(salt=policy_salt, **ref.STEP_POLICY)
    opt = ScheduledOptim(model, 128, AttrDict(n_warmup_steps=4000))
    return model, aug, TrainStep(model, opt, 30, 5.0, use_graph=True, graph_warmup=1, **step_kw)


def test_captured_step_draws_new_masks_on_every_replay():
    from st_amd import synthetic
    inputs, targets, in_len, tgt_len, truth = synthetic.make_batch(**ref.STEP_BATCH)
    model, aug, step = _small_step(ref.STEP_SALT)
    x, t, gt = inputs.cuda(), targets.cuda(), truth.cuda()
    _seed(ref.STEP_SEED)
    tables, static = [], None
    for k in range(1, 5):                       # one eager step, then the capture and three replays in all
        loss, _ = step(x, in_len, t, tgt_len, gt)
        assert np.isfinite(float(loss)), (k, float(loss))
        s = int(rng.seed_tensor(_device()))
        assert s == ref.STEP_SEED + k           # advanced once per step, captured or not
        _table_is(aug, ref.plan_of(aug, s, in_len.tolist(), stacked=True), "step %d" % k)
        if k >= 2:
            assert static is None or aug.last_masks.data_ptr() == static       # a static tensor that every replay rewrites
            static = aug.last_masks.data_ptr()
            tables.append(aug.last_masks.cpu().clone())
    assert len(step._graphs) == 1
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(tables[1], tables[2]) and not torch.equal(tables[0], tables[2])


def test_bucket_mode_reads_the_lengths_from_the_device():
    """One captured bucket step, then batches of shorter utterances: every time mask lies within the utterance it was drawn
    for - the plan launch reads the layout's device lengths, not what the capture saw."""
    from oracle import speech_transformer_oracle as orc
    bk = ref.BUCKET
    model, aug, step = _small_step(ref.BUCKET_SALT, bucket=(bk["T_cap"], bk["L_cap"]))
    _seed(ref.BUCKET_SEED)
    for k, (t_max, t_min, seed) in enumerate(bk["batches"]):
        b = orc.synthetic_batch(4, t_max, bk["L_cap"], 80, 30, seed=seed, t_min=t_min, l_min=4)
        T, L = int(b["in_len"].max()), int(b["tgt_len"].max())
        loss, _ = step(b["x"][:, :T].cuda(), b["in_len"], b["tokens"][:, :L].cuda(), b["tgt_len"], b["gt"][:, :L].cuda())
        assert np.isfinite(float(loss)), (k, float(loss))
        s = int(rng.seed_tensor(_device()))
        assert s == ref.BUCKET_SEED + k + 1
        table = aug.last_masks.cpu()
        for u, n in enumerate(b["in_len"].tolist()):
            tm = table[u, :aug.n_time_masks]
            assert int((tm[:, 0] + tm[:, 1]).max()) <= n and int(tm.min()) >= 0, (k, u, n, tm.tolist())
        _table_is(aug, ref.plan_of(aug, s, b["in_len"].tolist(), stacked=True), "bucket batch %d" % k)
    assert sum(st.cap is not None for st in step._buckets.values()) >= 1

"""-m gpu: the instantiations of one feature kernel body (csrc/st_augment.hip) agree, bit for bit, where the feature that
separates them is switched off by DATA - no masks in the table, an all-zero warp table.  A wrong ``if constexpr`` or a wrong LDS
index in a shared body shows here; what each variant computes is pinned by tests/test_specaug_gpu.py, tests/test_timewarp_gpu.py
and the feat_stack test of tests/test_kernels_gpu.py.  Outputs go into guarded views.  No tolerance anywhere."""
import pytest
import torch

from st_amd import native as nv
from st_amd import rng
from st_amd.functional import Rows
from tests import _specaug_ref as sref
from tests._local import Guarded

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32

LENGTHS = (12, 7, 1)                    # B = 3: several rows per workgroup, an odd count, a single row
BINS, T = 8, 12
SEED, SALT = 2025, 930                  # with MASKS below: every utterance has a frequency mask, the two longer ones time masks (checked below)
MASKS = dict(n_time=2, time_width=10, time_ratio_permille=500, n_freq=2, freq_width=3, mel_bins=BINS)
PACK_GEOMETRIES = [(3, 0, 3), (0, 0, 1)]          # (left, right, interval): the reference's stacking, and plain frames


def _bits(t):
    return t.contiguous().view(torch.int16)


def _plan(lengths, interval, right):
    """The masks of specaug_plan for these lengths -> (table on the device, masks)."""
    rng.manual_seed(SEED)
    dev = torch.device("cuda", torch.cuda.current_device())
    table = torch.zeros(len(LENGTHS), MASKS["n_time"] + MASKS["n_freq"], 2, dtype=I32, device="cuda")
    nv.specaug_plan(rng.seed_tensor(dev), SALT, lengths, table, interval=interval, right=right, **MASKS)
    widths = table[:, :, 1].cpu()
    assert int(widths[:, :2].max()) > 0 and int(widths[:, 2:].max()) > 0, "the plan drew no mask: %s" % table.tolist()
    return table


def _masked_some(masked, plain, what):
    """The masks zeroed some elements that stand non-zero without them, and left others."""
    zeroed = int(((_bits(masked) == 0) & (_bits(plain) != 0)).sum())
    kept = int((_bits(masked) != 0).sum())
    print("%s: %d elements zeroed by the masks, %d non-zero" % (what, zeroed, kept))
    assert zeroed > 0 and kept > 0, (what, zeroed, kept)


def _raw(generator_seed, width):
    g = torch.Generator().manual_seed(generator_seed)
    return (torch.randn(len(LENGTHS), T, width, generator=g) + 3.0).cuda()          # no zero anywhere, padding frames included


def _stats(F):
    """Kaldi statistics [B, 2, F + 1] with a mean and a positive variance of their own per (utterance, bin)."""
    g = torch.Generator().manual_seed(5)
    mean, sd = torch.randn(len(LENGTHS), F, generator=g) + 3.0, torch.rand(len(LENGTHS), F, generator=g) + 0.5
    cnt = torch.tensor(LENGTHS, dtype=F32)[:, None]
    st = torch.zeros(len(LENGTHS), 2, F + 1)
    st[:, 0, :F], st[:, 0, F], st[:, 1, :F] = cnt * mean, cnt[:, 0], cnt * (mean * mean + sd * sd)
    return st.cuda()


def _feat(fn, x, stats, left, right, interval, extra, what):
    in_len = torch.tensor(LENGTHS, dtype=I32, device="cuda")
    rows = Rows.packed((torch.tensor(LENGTHS) + interval - 1) // interval, "cuda")
    gd = Guarded(rows.total, BINS * (1 + left + right), BF16, "cuda")
    gd.view.zero_()
    fn(x, in_len, stats, left, right, interval, rows.off, rows.len, rows.max_len, gd.view, *extra)
    gd.assert_intact(what)
    return gd.view.clone()


@pytest.mark.parametrize("ci", range(len(sref.STACK_TRIPLES)))
@pytest.mark.parametrize("with_stats", [False, True])
def test_feat_stack_variants_agree(ci, with_stats):
    left, right, rate = sref.STACK_TRIPLES[ci]
    interval = 1 if rate == 10 else int(rate / 10)
    what = "(%d, %d, %d) stats %s" % (left, right, interval, with_stats)
    x, stats = _raw(20 + ci, BINS), _stats(BINS) if with_stats else None
    # 1. masks, none in the table == plain
    none = torch.zeros(len(LENGTHS), 0, 2, dtype=I32, device="cuda")
    plain = _feat(nv.feat_stack, x, stats, left, right, interval, (), "feat_stack " + what)
    unmasked = _feat(nv.feat_stack_aug, x, stats, left, right, interval, (none, 0, 0), "feat_stack_aug without masks " + what)
    assert int((_bits(plain) != 0).sum()) > 0
    n_diff = int((_bits(unmasked) != _bits(plain)).sum())
    print("feat_stack_aug without masks %s: %d elements differ from feat_stack" % (what, n_diff))
    assert n_diff == 0
    # 2. masks + warp, nothing warped == masks
    table = _plan(torch.tensor(LENGTHS, dtype=I32, device="cuda"), 1, 0)
    still = torch.zeros(len(LENGTHS), 2, dtype=I32, device="cuda")
    counts = (MASKS["n_time"], MASKS["n_freq"])
    masked = _feat(nv.feat_stack_aug, x, stats, left, right, interval, (table,) + counts, "feat_stack_aug " + what)
    warped = _feat(nv.feat_stack_warp, x, stats, left, right, interval, (table, still) + counts, "feat_stack_warp, nothing warped " + what)
    _masked_some(masked, plain, "feat_stack_aug " + what)
    n_diff = int((_bits(warped) != _bits(masked)).sum())
    print("feat_stack_warp, nothing warped %s: %d elements differ from feat_stack_aug" % (what, n_diff))
    assert n_diff == 0


@pytest.mark.parametrize("left,right,interval", PACK_GEOMETRIES)
def test_pack_variants_agree(left, right, interval):
    what = "(%d, %d, %d)" % (left, right, interval)
    Fd = BINS * (1 + left + right)
    x = _raw(40 + left, Fd)
    rows = Rows.packed(torch.tensor(LENGTHS), "cuda")
    table = _plan(rows.len, interval, right)
    still = torch.zeros(len(LENGTHS), 2, dtype=I32, device="cuda")
    out = {}
    for name, call in (("plain", lambda o: nv.pack_rows(x, rows.off, rows.len, o)),
                       ("masks", lambda o: nv.pack_rows_aug(x, rows.off, rows.len, o, table, MASKS["n_time"], MASKS["n_freq"], BINS, left,
                                                            right, interval)),
                       ("warp", lambda o: nv.pack_rows_warp(x, rows.off, rows.len, o, table, still, MASKS["n_time"], MASKS["n_freq"], BINS,
                                                            left, right, interval))):
        gd = Guarded(rows.total, Fd, BF16, "cuda", pad_rows=4, pad_cols=(0, 0))
        call(gd.view)
        gd.assert_intact("pack, %s %s" % (name, what))
        out[name] = gd.view.clone()
    _masked_some(out["masks"], out["plain"], "pack_rows_aug " + what)
    n_diff = int((_bits(out["warp"]) != _bits(out["masks"])).sum())
    print("pack_rows_warp, nothing warped %s: %d elements differ from pack_rows_aug" % (what, n_diff))
    assert n_diff == 0

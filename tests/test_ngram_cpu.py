"""-m "not gpu": the host side of the n-gram language model (st_amd/ngram.py): the fp64 definition against a hand-computed
example, ARPA parsing, completion (suffix closure) changing no probability, the float32 emulation of the kernels' trie walk
(tests/_emul_ngram.py) against the definition within a derived bound, the estimator summing to one, the ABI entries, the
constructor checks of Decode and the extra term of the two-pass combine."""
import ctypes
import itertools
import math
import types

import numpy as np
import pytest
import torch

from st_amd import ngram
from st_amd.ngram import LN10, NGramLM
from tests import _emul_ngram as emul

BOS, EOS = 2, 3
OOV = -99.0 * LN10

# the hand example: order 3 over 8 tokens; 7 has no unigram; (2) = BOS carries only a back-off
HAND = {
    (2,): (OOV, -0.1), (3,): (-1.5, 0.0), (4,): (-1.0, -0.5), (5,): (-2.0, -0.25), (6,): (-3.0, 0.0),
    (4, 5): (-0.4, -0.3), (5, 6): (-0.7, -0.2), (2, 4): (-0.2, -0.6),
    (4, 5, 6): (-0.1, 0.0), (2, 4, 5): (-0.05, 0.0),
}


def test_logp_hand_computed_trigram_example():
    lm = NGramLM.from_table(HAND, 3, 8)
    assert lm.logp([4, 5], 6) == -0.1                                            # stored
    assert lm.logp([5, 4, 5], 6) == -0.1                                         # only the last N - 1 tokens count
    assert lm.logp([4, 5], 4) == pytest.approx(-0.3 + -0.25 + -1.0, abs=1e-15)   # back-off through two levels
    assert lm.logp([6, 4], 5) == pytest.approx(-0.4, abs=1e-15)                  # the context (6, 4) is not stored: back-off 0
    assert lm.logp([2, 4], 6) == pytest.approx(-0.6 + -0.5 + -3.0, abs=1e-15)
    assert lm.logp([4, 5], 7) == pytest.approx(-0.3 + -0.25 + OOV, abs=1e-12)    # no unigram: oov_logp in the unigram slot
    assert lm.logp([], 7) == OOV and lm.logp([], 4) == -1.0
    assert lm.logp([2], 4) == -0.2
    assert lm.score_list([4, 5, 6, 3]) == pytest.approx(-0.2 + -0.05 + -0.1 + (-0.2 + 0.0 + -1.5), abs=1e-15)
    veto = NGramLM.from_table(HAND, 3, 8, oov_logp=float("-inf"))
    assert veto.logp([4, 5], 7) == float("-inf") and veto.logp([4, 5], 6) == -0.1


@pytest.mark.parametrize("order,V", [(1, 8), (6, 8), (3, 5121), (3, 0)])
def test_order_and_vocabulary_limits(order, V):
    with pytest.raises(ValueError):
        NGramLM.from_table({}, order, V)
    with pytest.raises(ValueError):
        NGramLM.estimate([[4, 5]], order, V)


def test_table_entries_are_checked():
    for bad in ({(8,): (-1.0, 0.0)}, {(4, 5, 6, 4): (-1.0, 0.0)}, {(4,): (float("nan"), 0.0)}, {(4,): (-1.0, float("inf"))}):
        with pytest.raises(ValueError):
            NGramLM.from_table(bad, 3, 8)
    with pytest.raises(ValueError):
        NGramLM.from_table(HAND, 3, 8, oov_logp=0.5)


# ---- ARPA ---------------------------------------------------------------------------------------------------------------------------
NAMES = {2: "<s>", 3: "</s>", 4: "a", 5: "b", 6: "c"}


def _arpa(table, order, names=NAMES, extra=()):
    lines = ["", "\\data\\"]
    per = {m: [g for g in sorted(table) if len(g) == m] for m in range(1, order + 1)}
    extra = {m: [e for e in extra if len(e[1]) == m] for m in range(1, order + 1)}
    for m in range(1, order + 1):
        lines.append("ngram %d=%d" % (m, len(per[m]) + len(extra[m])))
    for m in range(1, order + 1):
        lines += ["", "\\%d-grams:" % m]
        for g in per[m]:
            lp, bo = table[g]
            f = ["%.17g" % (lp / LN10)] + [names[k] for k in g]
            if m < order:
                f.append("%.17g" % (bo / LN10))
            lines.append("\t".join(f))
        for lp, words in extra[m]:
            lines.append(" ".join(["%g" % lp] + list(words)))
    return lines + ["", "\\end\\"]


def test_arpa_round_trip_and_dropped_words(tmp_path):
    symbols = {"a": 4, "b": 5, "c": 6}
    lines = _arpa(HAND, 3, extra=[(-1.25, ("zzz",)), (-0.5, ("a", "zzz")), (-0.5, ("zzz", "a", "b"))])
    lm = NGramLM.from_arpa(lines, symbols, bos=BOS, eos=EOS, V=8)
    assert lm.order == 3 and lm.V == 8 and lm.dropped == 3
    assert set(lm.table) == set(HAND)
    for g, (lp, bo) in HAND.items():
        assert lm.table[g][0] == pytest.approx(lp, abs=1e-12) and lm.table[g][1] == pytest.approx(bo, abs=1e-12), g
    path = tmp_path / "lm.arpa"
    path.write_text("\n".join(lines) + "\n")
    again = NGramLM.from_arpa(str(path), symbols, bos=BOS, eos=EOS)
    assert again.table == lm.table and again.V == 7 and again.dropped == 3     # V defaults to 1 + the largest id
    assert lm.logp([4, 5], 4) == pytest.approx(-1.55, abs=1e-12)


def _line_of(lines, text):
    return 1 + lines.index(text)


def test_arpa_malformed_files_name_the_line():
    symbols = {"a": 4, "b": 5, "c": 6}
    good = _arpa(HAND, 3)
    NGramLM.from_arpa(good, symbols, bos=BOS, eos=EOS)
    bad = list(good)
    at = _line_of(bad, "ngram 2=3")
    bad[at - 1] = "ngram 2=three"
    with pytest.raises(ValueError, match=r"line %d\b" % at):
        NGramLM.from_arpa(bad, symbols, bos=BOS, eos=EOS)
    bad = list(good)
    at = 1 + [i for i, x in enumerate(bad) if x.split("\t")[1:3] == ["a", "b"] and len(x.split("\t")) == 4][0]
    bad[at - 1] = bad[at - 1] + "\t0.5"                                        # a bigram line with five fields
    with pytest.raises(ValueError, match=r"line %d\b" % at):
        NGramLM.from_arpa(bad, symbols, bos=BOS, eos=EOS)
    bad = list(good)
    bad[at - 1] = "\t".join(["minus-one"] + bad[at - 1].split("\t")[1:])       # a number that does not parse
    with pytest.raises(ValueError, match=r"line %d\b" % at):
        NGramLM.from_arpa(bad, symbols, bos=BOS, eos=EOS)
    cut = [x for x in good if x != "\\end\\"]
    with pytest.raises(ValueError, match=r"line %d\b.*end" % len(cut)):
        NGramLM.from_arpa(cut, symbols, bos=BOS, eos=EOS)
    short = list(good)
    del short[at - 1]                                                           # the count line promises one more bigram
    with pytest.raises(ValueError, match="ngram 2=3"):
        NGramLM.from_arpa(short, symbols, bos=BOS, eos=EOS)


# ---- completion -----------------------------------------------------------------------------------------------------------------------
def _random_table(V, order, seed, density=0.25, no_unigram=()):
    """A sparse table that violates suffix closure: every order is drawn independently."""
    rng = np.random.default_rng(seed)
    table = {}
    for m in range(1, order + 1):
        space = V ** m
        for flat in rng.choice(space, size=max(1, min(space, int(density * min(space, 400)))), replace=False):
            g = tuple(int(flat // V ** i % V) for i in range(m))
            if g[-1] in no_unigram:                    # (as a context it may appear; nothing ends in it, so completion adds no unigram)
                continue
            table[g] = (-float(rng.random()) * 5.0 - 0.01, -float(rng.random()) * 2.0 if m < order else 0.0)
    return table


def _closed(table):
    return all(len(g) == 1 or g[1:] in table for g in table)


@pytest.mark.parametrize("V,order", [(5, 2), (6, 3), (12, 4), (4, 5)])
def test_completion_changes_no_probability(V, order):
    table = _random_table(V, order, 100 * V + order, no_unigram=(1,))
    assert not _closed(table)
    raw = NGramLM.from_table(table, order, V)
    full = NGramLM.from_table(raw.completed(), order, V)
    assert _closed(full.table) and len(full.table) > len(table)
    assert all(full.table[g] == v for g, v in raw.table.items())
    worst = 0.0
    for k in range(order):
        for h in itertools.product(range(V), repeat=k):
            for c in range(V):
                a, b = raw.logp(h, c), full.logp(h, c)
                worst = max(worst, abs(a - b))
    assert worst <= 1e-12, worst


# ---- the float32 trie walk against the definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,order,oov", [(6, 2, OOV), (7, 3, OOV), (6, 4, float("-inf")), (4, 5, OOV)])
def test_emulated_trie_walk_matches_fp64_within_the_derived_bound(V, order, oov):
    table = _random_table(V, order, 7 * V + order, density=0.4, no_unigram=(1,))
    lm = NGramLM.from_table(table, order, V, oov_logp=oov)
    trie = ngram.DeviceTrie(lm, "cpu")
    h = trie.host
    assert h["child_lo"].dtype == np.int32 and h["tok"].dtype == np.int32 and h["logp"].dtype == np.float32
    assert h["child_lo"].shape == (trie.nodes + 1,) and h["child_lo"][0] == V and h["child_lo"][-1] == trie.nodes
    assert np.all(np.diff(h["child_lo"]) >= 0) and np.array_equal(h["tok"][:V], np.arange(V))
    for node in range(trie.nodes):
        kids = h["tok"][h["child_lo"][node]:h["child_lo"][node + 1]]
        assert np.all(np.diff(kids) > 0)                                        # sorted within a parent, no duplicates
    assert h["logp"][1] == np.inf                                               # token 1 has no unigram
    ref = trie.rounded_model()                                                  # the SAME rounded values, in fp64
    assert set(ref.table) == set(lm.completed())
    n_cmp, worst = 0, 0.0
    for k in range(order):
        for hist in itertools.product(range(-1, V), repeat=k):
            padded = [-1] * (order - 1 - k) + list(hist)
            valid = emul.valid_history(trie, padded)[::-1]
            for c in range(V):
                terms = []
                got = float(emul.score(trie, padded, c, terms))
                want = ref.logp(valid, c)
                if math.isinf(want):
                    assert got == want
                    continue
                bound = emul.walk_bound(order, terms)
                assert abs(got - want) <= bound, (hist, c, got, want, bound)
                worst = max(worst, abs(got - want) / max(bound, 1e-300))
                n_cmp += 1
    assert n_cmp > 40
    assert emul.score(trie, [-1] * (order - 1), -1) == -np.inf and emul.score(trie, [-1] * (order - 1), V) == -np.inf


# ---- the estimator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3, 4])
def test_estimate_sums_to_one_and_is_suffix_closed(order):
    rng = np.random.default_rng(order)
    V = 11
    lists = [[int(t) for t in rng.integers(4, V, rng.integers(1, 9))] for _ in range(30)]
    lm = NGramLM.estimate(lists, order, V)
    assert _closed(lm.table)
    kept = [c for c in range(V) if c not in (0, BOS)]
    assert all((c,) in lm.table for c in kept) and (0,) not in lm.table
    contexts = [()] + [g for g in lm.table if len(g) < order] + [(9, 9, 9)[:order - 1]]
    assert (BOS,) in contexts and any(len(g) == order - 1 for g in contexts[1:-1])
    if order > 2:
        assert contexts[-1] not in lm.table                                     # the unseen context
    for h in contexts:
        total = sum(math.exp(lm.logp(h, c)) for c in kept)
        assert abs(total - 1.0) <= 1e-9, (h, total)
    # the discounting formula itself, on one seen bigram: p(c | a) = (n(a, c) - D) / n(a) + gamma(a) p(c)
    a, c = lists[0][0], lists[0][1] if len(lists[0]) > 1 else EOS
    seqs = [[BOS] + l + [EOS] for l in lists]
    n_ac = sum(1 for s in seqs for i in range(1, len(s)) if s[i - 1] == a and s[i] == c)
    follow = [s[i] for s in seqs for i in range(1, len(s)) if s[i - 1] == a]
    if order == 2:
        want = (n_ac - 0.75) / len(follow) + 0.75 * len(set(follow)) / len(follow) * math.exp(lm.logp([], c))
        assert math.exp(lm.logp([a], c)) == pytest.approx(want, rel=1e-12)
        assert lm.table[(a,)][1] == pytest.approx(math.log(0.75 * len(set(follow)) / len(follow)), abs=1e-12)
    with pytest.raises(ValueError):
        NGramLM.estimate([[4, BOS]], order, V)


# ---- ABI, wrappers, options --------------------------------------------------------------------------------------------------------------
def test_abi_has_the_three_entries():
    from st_amd import build, native
    assert "st_ngram.hip" in build.SOURCES
    S = native.SIGNATURES
    assert len(S["st_ngram_score"]) == 20 and len(S["st_ngram_advance"]) == 9 and len(S["st_ngram_score_seq"]) == 15
    assert S["st_ngram_score"][8] is ctypes.c_float and S["st_ngram_score"][16:18] == [ctypes.c_float, ctypes.c_float]
    assert S["st_ngram_score_seq"][8] is ctypes.c_float and S["st_ngram_advance"][1] is ctypes.c_void_p
    lib = native.load()
    assert all(hasattr(lib, k) for k in ("st_ngram_score", "st_ngram_advance", "st_ngram_score_seq"))
    assert lib.st_version() == native.ABI_VERSION == native.abi_fingerprint(open(build.ABI_HEADER).read())


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from st_amd import native as nv
    lm = NGramLM.from_table(HAND, 3, 8).to("cpu")
    hist = ngram.initial_history(4, 3, "cpu")
    assert hist.tolist() == [[-1, BOS]] * 4
    with pytest.raises(RuntimeError, match="GPU"):
        nv.ngram_score(lm.trie, hist, torch.zeros(4, 3, dtype=torch.int32), None, EOS, lm_out=torch.zeros(4, 3))
    with pytest.raises(ValueError):
        nv.ngram_score(lm.trie, hist, torch.zeros(4, 65, dtype=torch.int32), None, EOS)
    with pytest.raises(ValueError):
        nv.ngram_advance(torch.zeros(4, 5, dtype=torch.int32), torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long), None, EOS, 2)
    with pytest.raises(ValueError):
        nv.ngram_advance(hist, torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long), None, EOS, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        nv.ngram_score_seq(lm.trie, torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), BOS, torch.zeros(2, 3))


def test_decode_options_are_checked_at_construction():
    model = types.SimpleNamespace(vocab_size=8)
    opt = lambda **kw: types.SimpleNamespace(beam_size=4, **kw)
    lm = NGramLM.from_table(HAND, 3, 8).to("cpu")
    assert ngram.check_options(opt(), None, model, "cpu", 4, joint=False) == (0.0, 0.0, None)
    assert ngram.check_options(opt(lm_weight=0.5, lm_length_bonus=0.25), lm, model, "cpu", 4, joint=True) == (0.5, 0.25, None)
    assert ngram.check_options(opt(lm_weight=0.5), lm, model, "cpu", 4, joint=False) == (0.5, 0.0, 6)
    assert ngram.check_options(opt(lm_weight=0.5, ctc_pre_beam=8), lm, model, "cpu", 4, joint=False) == (0.5, 0.0, 8)
    assert ngram.check_options(opt(), lm, model, "cpu", 4, joint=False) == (0.0, 0.0, None)
    with pytest.raises(ValueError, match="lm_weight"):
        ngram.check_options(opt(lm_weight=-0.1), lm, model, "cpu", 4, joint=False)
    with pytest.raises(ValueError, match="vocabulary"):
        ngram.check_options(opt(lm_weight=0.5), lm, types.SimpleNamespace(vocab_size=9), "cpu", 4, joint=False)
    with pytest.raises(ValueError, match="lives on"):
        ngram.check_options(opt(lm_weight=0.5), NGramLM.from_table(HAND, 3, 8), model, "cpu", 4, joint=False)   # never moved: no trie
    with pytest.raises(ValueError, match="lives on"):
        ngram.check_options(opt(lm_weight=0.5), lm, model, "cuda", 4, joint=False)
    with pytest.raises(ValueError, match="ctc_pre_beam"):
        ngram.check_options(opt(lm_weight=0.5, ctc_pre_beam=3), lm, model, "cpu", 4, joint=False)
    lm.order = 6
    with pytest.raises(ValueError, match="order"):
        ngram.check_options(opt(lm_weight=0.5), lm, model, "cpu", 4, joint=False)


def test_decode_constructor_takes_the_language_model():
    from tests.test_decode_cpu import _model, _params
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    model = _model(_params(), "cpu")
    lm = NGramLM.estimate([[4, 5, 6], [5, 5]], 3, 30).to("cpu")
    dec = Decode(AttrDict(dict(beam_size=4, n_best=1, lm_weight=0.5, lm_length_bonus=0.1)), "cpu", model=model, lm=lm)
    assert (dec.lm_weight, dec.lm_length_bonus, dec.lm_pre_beam, dec._lm_on) == (0.5, 0.1, 6, True)
    assert not Decode(AttrDict(dict(beam_size=4, n_best=1)), "cpu", model=model, lm=lm)._lm_on
    with pytest.raises(ValueError, match="vocabulary"):
        Decode(AttrDict(dict(beam_size=4, n_best=1, lm_weight=0.5)), "cpu", model=model, lm=NGramLM.from_table(HAND, 3, 8).to("cpu"))
    with pytest.raises(ValueError, match="lm_weight"):
        Decode(AttrDict(dict(beam_size=4, n_best=1, lm_weight=-1.0)), "cpu", model=model, lm=lm)
    with pytest.raises(ValueError, match="language model"):
        Decode(AttrDict(dict(beam_size=4, n_best=1)), "cpu", model=model).lm_score([[[4]]])


def test_two_pass_combine_with_the_extra_term():
    from st_amd import ctc_beam
    hyps = [[[4, 5], [6], []]]
    ctc = torch.tensor([[-1.0, -2.0, float("-inf")]])
    att = torch.tensor([[-3.0, -1.0, float("-inf")]])
    base_h, base_s = ctc_beam.combine(hyps, ctc, att, 0.5, 3, EOS)
    same_h, same_s = ctc_beam.combine(hyps, ctc, att, 0.5, 3, EOS, extra=None)
    assert base_h == same_h == [[[6, EOS], [4, 5, EOS], []]] and torch.equal(base_s, same_s)
    h, s = ctc_beam.combine(hyps, ctc, att, 0.5, 3, EOS, extra=torch.tensor([[0.0, -4.0, float("-inf")]]))
    assert h == [[[4, 5, EOS], [6, EOS], []]]
    assert s.tolist() == [[-2.0, -5.5, float("-inf")]]
    with pytest.raises(ValueError):
        ctc_beam.combine(hyps, ctc, att, 0.5, 3, EOS, extra=torch.zeros(1, 2))

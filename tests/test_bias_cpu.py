"""Contextual biasing on the host (st_amd/biasing.py, tests/_emul_bias.py): the automaton's increments against the brute-force
reward (exact with dyadic weights, within the emulation's own derived bound with general ones), the per-position identity
running sum = reward + Phi, limits and validation, the ABI entries, and one emulated search step after another (pre-beam -> bias
-> joint advance -> follow) keeping the states consistent with the hypotheses the advance chose."""
import ctypes
import types

import numpy as np
import pytest
import torch

from st_amd import biasing
from st_amd.biasing import ContextBias
from tests import _bias_cases as cases
from tests import _emul_bias as emul

BOS, EOS = cases.BOS, cases.EOS
DYADIC = (0.25, 0.5, 1.0, 1.5, 2.0)


def random_set(rng, v, dyadic):
    """Phrases over the tokens 4 .. 4 + v - 1: random ones plus a nested pair, a prefix pair, a duplicate with another weight and
    a repeated-token phrase."""
    toks = list(range(4, 4 + v))
    a, b = toks[0], toks[1]
    c, d = toks[2 % v], toks[3 % v]
    phrases = [[int(rng.choice(toks)) for _ in range(int(rng.integers(1, 7)))] for _ in range(int(rng.integers(1, 6)))]
    phrases += [[a, b, c, d], [b, c], [a, b], [a, a, a], [b, c]]
    w = (lambda: float(rng.choice(DYADIC))) if dyadic else (lambda: float(0.1 + 2.9 * rng.random()))
    keep = rng.random(len(phrases)) < 0.7
    keep[-1] = keep[-4] = True                             # the duplicate pair stays
    picked = [p for p, k in zip(phrases, keep) if k]
    return ContextBias.from_phrases(picked, weights=[w() for _ in picked]), toks


def emulated(tables, h):
    """-> (f32 increments of h . EOS, the operand lists of the positions)."""
    row = np.array([list(h) + [EOS]], dtype=np.int32)
    terms = []
    out = emul.score_seq(tables, row, np.array([row.shape[1]]), EOS, terms)
    return out[0], terms


@pytest.mark.parametrize("v", [2, 3, 5])
def test_dyadic_increments_sum_to_the_brute_force_reward_exactly(v):
    rng = np.random.default_rng(v)
    n_pos = 0
    for _ in range(60):
        bias, toks = random_set(rng, v, dyadic=True)
        tables = bias.to("cpu").tables
        auto = bias.automaton
        for _ in range(6):
            h = [int(rng.choice(toks)) for _ in range(int(rng.integers(0, 21)))]
            inc, _ = emulated(tables, h)
            assert float(inc.astype(np.float64).sum()) == bias.reward(h), (bias.phrases, h)
            assert auto.increments(h + [EOS]) == [float(x) for x in inc]
            assert auto.reward(h) == bias.reward(h)
            # per position: the running sum is the reward so far plus the provisional part of the match in progress
            run = 0.0
            for t in range(len(h)):
                run += float(inc[t])
                assert run == bias.reward(h[:t + 1]) + float(auto.phi[auto.state(h[:t + 1])]), (bias.phrases, h, t)
                n_pos += 1
    assert n_pos > 1000


def test_duplicate_phrase_keeps_the_larger_weight_and_all_occurrences_count():
    bias = ContextBias.from_phrases([[5, 6], [5, 6], [4, 5, 6, 7], [4, 4, 4]], weights=[0.5, 0.75, 1.0, 2.0])
    assert bias.phrases[(5, 6)] == 0.75
    assert bias.reward([4, 5, 6, 7]) == 4.0 + 1.5                          # nested
    assert bias.reward([4, 4, 4, 4, 4]) == 3 * 6.0                         # overlapping occurrences
    assert bias.reward([5, 6, 9, 5, 6]) == 3.0 and bias.reward([]) == 0.0 and bias.reward([6, 5]) == 0.0
    assert ContextBias.from_phrases([[5, 6]], weight=2.0).reward([5, 6]) == 4.0


@pytest.mark.parametrize("v", [2, 3, 5])
def test_general_weights_stay_within_the_emulations_own_bound(v):
    """fp32 increments summed in fp64 against the fp64 definition over the ROUNDED tables: per position walk_bound of its
    operands, plus the fp64 summation's own (positions x 2^-53 x sum |increments|); and against the unrounded brute force with the
    tables' rounding on top - 2^-24 |cash| per visited state (the phi values telescope away whatever their rounding)."""
    rng = np.random.default_rng(100 + v)
    worst = 0.0
    for _ in range(40):
        bias, toks = random_set(rng, v, dyadic=False)
        tables = bias.to("cpu").tables
        ref = tables.rounded_model()
        for _ in range(6):
            h = [int(rng.choice(toks)) for _ in range(int(rng.integers(1, 21)))]
            inc, terms = emulated(tables, h)
            got = float(inc.astype(np.float64).sum())
            bound = sum(emul.walk_bound(p) for p in terms) + len(inc) * 2.0 ** -53 * float(np.abs(inc).astype(np.float64).sum())
            assert abs(got - ref.reward(h)) <= bound, (bias.phrases, h, got, ref.reward(h), bound)
            s, table_err = 0, 0.0
            for c in h:
                s = ref.next(s, c)
                table_err += 2.0 ** -24 * float(ref.cash[s])
            truth = bias.reward(h)
            assert abs(got - truth) <= bound + table_err + 2.0 ** -50 * abs(truth), (bias.phrases, h, got, truth)
            worst = max(worst, abs(got - truth))
    print("largest |fp32 walk - brute force| met: %.3e" % worst)


def test_tables_are_breadth_first_with_sorted_consecutive_children():
    t = cases.seven().to("cpu").tables
    h = t.host
    assert h["child_lo"][0] == 1 and h["child_lo"][-1] == t.S and h["fail"][0] == 0 and h["depth"][0] == 0
    assert (np.diff(h["depth"]) >= 0).all()
    for s in range(t.S):
        lo, hi = int(h["child_lo"][s]), int(h["child_lo"][s + 1])
        assert (np.diff(h["tok"][lo:hi]) > 0).all() and (h["depth"][lo:hi] == h["depth"][s] + 1).all()
    assert (h["depth"][h["fail"][1:]] < h["depth"][1:]).all()
    assert h["cash"].dtype == np.float32 and h["phi"].dtype == np.float32 and h["fail"].dtype == np.int32
    ref = t.rounded_model()
    assert ref.reward([cases.A, cases.B_, cases.C, cases.D]) == 4.0 + 2 * 0.75 + 2 * 0.25


def test_limits_and_validation():
    with pytest.raises(ValueError, match="1..32"):
        ContextBias.from_phrases([[5] * 33])
    ContextBias.from_phrases([[5] * 32])
    with pytest.raises(ValueError, match="1..32"):
        ContextBias.from_phrases([[4, 5], []])
    for w in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight"):
            ContextBias.from_phrases([[4, 5]], weight=w)
        with pytest.raises(ValueError, match="weight"):
            ContextBias.from_phrases([[4, 5], [6]], weights=[1.0, w])
    with pytest.raises(ValueError, match=">= 0"):
        ContextBias.from_phrases([[4, -1]])
    with pytest.raises(ValueError, match="weights for"):
        ContextBias.from_phrases([[4], [5]], weights=[1.0])
    with pytest.raises(ValueError, match="states"):
        ContextBias.from_phrases([[k] * 32 for k in range(2049)])           # 1 + 2049 x 32 = 65,569 states
    bias = cases.seven()
    broken = ContextBias.__new__(ContextBias)
    broken.__dict__.update(bias.__dict__)
    a = bias.automaton
    fail = a.fail.copy()
    deep = int(np.argmax(a.depth))
    fail[1] = deep                                                         # a fail link to a DEEPER node: the walk could cycle
    broken.automaton = biasing.Automaton(a.child_lo, a.tok, fail, a.depth, a.cash, a.phi)
    with pytest.raises(ValueError, match="shallower"):
        broken.to("cpu")


def test_decode_options_are_checked_at_construction():
    model = types.SimpleNamespace(vocab_size=30)
    opt = lambda **kw: types.SimpleNamespace(beam_size=4, **kw)
    bias = cases.seven().to("cpu")
    assert biasing.check_options(opt(), None, model, "cpu", 4, joint=False) == (1.0, None)
    assert biasing.check_options(opt(), bias, model, "cpu", 4, joint=True) == (1.0, None)
    assert biasing.check_options(opt(bias_weight=0.5), bias, model, "cpu", 4, joint=False) == (0.5, 6)
    assert biasing.check_options(opt(bias_weight=2.0, ctc_pre_beam=8), bias, model, "cpu", 4, joint=False) == (2.0, 8)
    assert biasing.check_options(opt(bias_weight=0.0), bias, model, "cpu", 4, joint=False) == (0.0, None)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bias_weight"):
            biasing.check_options(opt(bias_weight=bad), bias, model, "cpu", 4, joint=False)
    with pytest.raises(ValueError, match="bias_weight"):
        biasing.check_options(opt(bias_weight=-1.0), None, model, "cpu", 4, joint=False)
    with pytest.raises(ValueError, match="lives on"):
        biasing.check_options(opt(), cases.seven(), model, "cpu", 4, joint=False)      # never moved: no tables
    with pytest.raises(ValueError, match="lives on"):
        biasing.check_options(opt(), bias, model, "cuda", 4, joint=False)
    with pytest.raises(ValueError, match="ctc_pre_beam"):
        biasing.check_options(opt(ctc_pre_beam=3), bias, model, "cpu", 4, joint=False)
    with pytest.raises(ValueError, match="beam_size"):
        biasing.check_options(types.SimpleNamespace(beam_size=17), bias, model, "cpu", 17, joint=False)


def test_decode_constructor_takes_the_context_bias():
    from tests.test_decode_cpu import _model, _params
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    model = _model(_params(), "cpu")
    bias = cases.seven().to("cpu")
    dec = Decode(AttrDict(dict(beam_size=4, n_best=1, bias_weight=0.5)), "cpu", model=model, bias=bias)
    assert (dec.bias_weight, dec.bias_pre_beam, dec._bias_on, dec._lm_on) == (0.5, 6, True, False)
    plain = Decode(AttrDict(dict(beam_size=4, n_best=1)), "cpu", model=model)
    assert (plain.bias_weight, plain.bias_pre_beam, plain._bias_on) == (1.0, None, False)
    assert not Decode(AttrDict(dict(beam_size=4, n_best=1, bias_weight=0.0)), "cpu", model=model, bias=bias)._bias_on
    with pytest.raises(ValueError, match="bias_weight"):
        Decode(AttrDict(dict(beam_size=4, n_best=1, bias_weight=-1.0)), "cpu", model=model, bias=bias)
    with pytest.raises(ValueError, match="lives on"):
        Decode(AttrDict(dict(beam_size=4, n_best=1)), "cuda", model=model, bias=bias)
    with pytest.raises(ValueError, match="context bias"):
        plain.bias_score([[[4]]])


def test_abi_has_the_three_entries():
    from st_amd import build, native
    assert "st_bias.hip" in build.SOURCES
    S = native.SIGNATURES
    assert len(S["st_bias_score"]) == 17 and len(S["st_bias_advance"]) == 12 and len(S["st_bias_score_seq"]) == 13
    assert S["st_bias_score"][14] is ctypes.c_float and S["st_bias_score"][6] is ctypes.c_int
    lib = native.load()
    assert all(hasattr(lib, k) for k in ("st_bias_score", "st_bias_advance", "st_bias_score_seq"))
    assert lib.st_version() == native.ABI_VERSION == native.abi_fingerprint(open(build.ABI_HEADER).read())


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from st_amd import native as nv
    t = cases.seven().to("cpu").tables
    state = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        nv.bias_score(t, state, torch.zeros(4, 3, dtype=torch.int32), None, EOS, raw=torch.zeros(4, 3))
    with pytest.raises(ValueError):
        nv.bias_score(t, state, torch.zeros(4, 65, dtype=torch.int32), None, EOS)
    with pytest.raises(ValueError):
        nv.bias_advance(t, state, torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long), None, EOS, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        nv.bias_score_seq(t, torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), EOS, torch.zeros(2, 3))


@pytest.mark.parametrize("w", [0.3, 0.0])
def test_emulated_search_steps_keep_the_states_consistent_with_the_hypotheses(w):
    """Five steps of pre-beam (the K best of the log-softmax) -> emulated st_bias_score -> the torch joint advance -> emulated
    st_bias_advance.  After every step the state of every slot is the automaton state of the hypothesis the trellis spells for
    it (-1 once it holds EOS), and its score carries scale x (1 - w) x (reward + Phi) of that hypothesis on top of the unbiased
    terms.  Met on the way: two children of one parent, a parent overwritten by its own child, a row frozen after EOS."""
    from tests.test_ngram_gpu import chain_logits, chain_state
    Bn, beam, K, V, S = 3, 4, 6, 30, 6
    bias = cases.chain_bias(V, 5)
    tables = bias.to("cpu").tables
    auto = bias.automaton
    scale = 0.5 / (1 - w)
    n = Bn * beam
    g = torch.Generator().manual_seed(11)
    st = chain_state(Bn, beam, S)
    state = np.zeros(n, dtype=np.int32)
    plain = torch.zeros(Bn, beam, dtype=torch.float64)      # the unbiased part of every slot's score, carried along
    seen = dict(two_children=False, overwritten=False, frozen=False, boosted=False)
    for t in range(S - 1):
        logits = chain_logits(V, n, t, g)
        lsm = torch.log_softmax(logits[:, :V].double(), -1)
        lp, ids = lsm.topk(K, -1)
        lp = lp.float()
        delta = -torch.rand(n, K, generator=g) * 3 if w > 0 else torch.zeros(n, K)
        full = dict(st, cand_gam=torch.zeros(n, K, 2, 2), cand_psi=torch.zeros(n, K))
        done_before = st["done"].clone()
        want, state2, _ = cases.chain_reference(full, state, ids.int(), lp, delta, tables, scale, w, beam, K, t)
        new_plain = plain.clone()
        for b in range(Bn):
            if bool(done_before[b]):
                assert np.array_equal(state2[b * beam:(b + 1) * beam], state[b * beam:(b + 1) * beam])
                continue
            parents = [int(p) for p in want["order"][b * beam:(b + 1) * beam]]
            seen["two_children"] |= len(set(parents)) < beam
            seen["overwritten"] |= any(p != b * beam + s and p in range(b * beam, b * beam + beam) for s, p in enumerate(parents))
            for s in range(beam):
                if not np.isfinite(float(want["scores"][b, s])):
                    continue
                hyp = cases.hypothesis_of(want, b, s, t)
                row, o = b * beam + s, parents[s] - b * beam
                j = int((ids[parents[s]] == hyp[-1]).nonzero()[0])
                first_eos = hyp.index(EOS) if EOS in hyp else len(hyp)
                labels = hyp[:first_eos]
                closed = first_eos < len(hyp)
                if not bool(want["done"][b]):               # (an utterance that finished in this step: its states are not moved)
                    assert state2[row] == (-1 if closed else auto.state(labels)), (t, b, s, hyp)
                seen["frozen"] |= closed and not bool(want["done"][b])      # (a closed hypothesis below the top of a live utterance)
                new_plain[b, s] = plain[b, o] + (1 - w) * float(lp[parents[s], j]) + (w * float(delta[parents[s], j]) if w > 0 else 0.0)
                carried = bias.reward(labels) + (0.0 if closed else float(auto.phi[auto.state(labels)]))
                seen["boosted"] |= carried > 0
                total = float(new_plain[b, s]) + (1 - w) * float(np.float32(scale)) * carried
                # (the trellis keeps scores in fp32: one rounding of the running score per step)
                assert abs(float(want["scores"][b, s]) - total) <= (t + 1) * 2.0 ** -23 * max(1.0, abs(total)), (t, b, s, hyp, carried)
        st = {k: want[k] for k in st}
        state, plain = state2, new_plain
    assert all(seen.values()), seen

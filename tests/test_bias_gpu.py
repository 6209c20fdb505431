"""-m gpu: contextual biasing on the device (csrc/st_bias.hip, st_amd/biasing.py, transformer/Decode.py with ``bias=``):
st_bias_score / st_bias_score_seq BIT-equal to the float32 emulation of tests/_emul_bias.py (the deepest fail chain, the widest
node), st_bias_advance against the NumPy permutation, five chained search steps against the torch formulation of the joint
advance, the biased search on the small decode model against fp64 truth + bias_weight x reward (joint, bias-only and LM + bias
routes, graph replay), a phrase that turns the runner-up into the winner, swapped bias objects, and two-pass rescoring."""
import math

import numpy as np
import pytest
import torch

from st_amd.biasing import ContextBias
from tests import _bias_cases as cases
from tests import _emul_bias as emul
from tests._local import Guarded

pytestmark = pytest.mark.gpu

BOS, EOS = cases.BOS, cases.EOS
F32, I32 = torch.float32, torch.int32


def _nv():
    from st_amd import native as nv
    nv.load(build_if_missing=False)
    return nv


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


_SEVEN = {}


def _seven():
    if not _SEVEN:
        _SEVEN["bias"] = cases.seven().to("cuda")
    return _SEVEN["bias"]


GRID = [(1, 1, 1), (5, 4, 6), (3, 16, 64)]


@pytest.mark.parametrize("Bn,beam,K", GRID)
def test_bias_score_raw_is_bit_equal_to_the_emulation(Bn, beam, K):
    nv = _nv()
    t = _seven().tables
    state, cand, done = cases.score_case(t, Bn, beam, K, 100 * Bn + K)
    n = Bn * beam
    want = emul.score_rows(t, state, cand, EOS, done, beam)
    out = Guarded(n, K, F32, "cuda", pad_rows=8, pad_cols=(0, 0))
    nv.bias_score(t, torch.from_numpy(state).cuda(), torch.from_numpy(cand).cuda(), torch.from_numpy(done).cuda(), EOS, raw=out.view)
    torch.cuda.synchronize()
    out.assert_intact("st_bias_score: raw")
    skipped = np.repeat(done, beam)
    out.assert_untouched(skipped, "st_bias_score: rows of a done utterance")
    got = out.view.cpu().numpy()
    live = ~skipped
    assert not np.isnan(got[live]).any()
    bad = np.argwhere(_bits(got[live]) != _bits(want[live]))
    assert bad.size == 0, (bad[:5], got[live][tuple(bad[0])], want[live][tuple(bad[0])])
    if n > 1:                                               # the cases the grid promises, counted on the reference side
        assert (cand == EOS).any() and (cand == -1).any() and (state < 0).any() and done.any()
        assert (want[live] > 0).any() and (want[live] < 0).any() and (want[live] == 0).any()


@pytest.mark.parametrize("Bn,beam,K", GRID)
def test_bias_score_in_place_is_bit_equal_to_the_emulation(Bn, beam, K):
    """lp = fmaf(scale, Delta, lp): dyadic operands, so the emulation's single rounding is fmaf's; a -inf lp stays -inf; frozen
    rows and done utterances keep their lp bit for bit."""
    nv = _nv()
    t = _seven().tables
    state, cand, done = cases.score_case(t, Bn, beam, K, 100 * Bn + K)
    n = Bn * beam
    rng = np.random.default_rng(3 + n)
    lp0 = (-np.round(rng.random((n, K)) * 9.0 * 1024) / 1024).astype(np.float32)
    lp0[rng.random((n, K)) < 0.15] = -np.inf
    lp0[0, 0] = -np.inf
    scale = 0.625
    raw = emul.score_rows(t, state, cand, EOS, done, beam)
    keep = np.repeat(done, beam) | (state < 0)
    want = np.where(keep[:, None], lp0, emul.fuse(lp0, scale, np.where(np.isnan(raw), 0.0, raw)))
    lp = Guarded(n, K, F32, "cuda", pad_rows=8, pad_cols=(0, 0))
    lp.view.copy_(torch.from_numpy(lp0))
    nv.bias_score(t, torch.from_numpy(state).cuda(), torch.from_numpy(cand).cuda(), torch.from_numpy(done).cuda(), EOS, scale, lp=lp.view)
    torch.cuda.synchronize()
    lp.assert_intact("st_bias_score: lp")
    got = lp.view.cpu().numpy()
    assert not np.isnan(got).any() and np.array_equal(np.isneginf(got), np.isneginf(lp0))
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    if n > 1:
        assert keep.any() and (got[~keep] != lp0[~keep]).any()


def test_maximum_depth_fail_chain_through_score_seq():
    """a x 32 and a x 31 . b; a x 40 . b walks 32 -> 31 -> 32 at every a past the 32nd, a x 40 . c falls through all 32 fail
    links to the root: every position bit-equal to the emulation, and the sums equal the brute-force reward exactly."""
    nv = _nv()
    a, b, c = 4, 5, 6
    bias = ContextBias.from_phrases([[a] * 32, [a] * 31 + [b]], weights=[0.5, 0.25]).to("cuda")
    t = bias.tables
    assert int(t.host["depth"].max()) == 32
    lists = [[a] * 40 + [b], [a] * 40 + [c], [a] * 7]
    L = 42
    tokens = np.full((3, L), 99, dtype=np.int32)
    lens = np.zeros(3, dtype=np.int32)
    for m, h in enumerate(lists):
        tokens[m, :len(h) + 1] = h + [EOS]
        lens[m] = len(h) + 1
    want = emul.score_seq(t, tokens, lens, EOS)
    out = Guarded(3, L, F32, "cuda", pad_rows=8, pad_cols=(0, 0))
    nv.bias_score_seq(t, torch.from_numpy(tokens).cuda(), torch.from_numpy(lens).cuda(), EOS, out.view)
    torch.cuda.synchronize()
    out.assert_intact("st_bias_score_seq: out")
    got = out.view.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    for m, h in enumerate(lists):
        assert float(got[m].astype(np.float64).sum()) == bias.reward(h), (m, got[m])
    assert bias.reward(lists[0]) == 9 * 16.0 + 8.0 and bias.reward(lists[1]) == 9 * 16.0 and bias.reward(lists[2]) == 0.0
    assert got[0, 40] == 8.0 and got[1, 40] == 0.0 and got[1, 41] == 0.0              # (the a x 32 state has nothing provisional)
    assert got[2, 7] == -3.5 and (got[2, 8:] == 0).all()                              # the provisional part taken back by EOS


def test_widest_node_every_token_of_5120_is_rewarded():
    """5,120 one-token phrases: the root's child search takes 13 rounds; every token collects its weight, token 5120 nothing."""
    nv = _nv()
    V = 5120
    bias = ContextBias.from_phrases([[k] for k in range(V)], weights=[0.25 * (1 + k % 4) for k in range(V)]).to("cuda")
    t = bias.tables
    assert t.S == V + 1 and int(t.host["child_lo"][1]) == V + 1
    tokens = np.concatenate([np.arange(V), np.full(64, V)]).astype(np.int32).reshape(81, 64)
    lens = np.full(81, 64, dtype=np.int32)
    no_eos = 6000                                           # (EOS = 3 is one of the phrases here)
    out = Guarded(81, 64, F32, "cuda", pad_rows=8, pad_cols=(0, 0))
    nv.bias_score_seq(t, torch.from_numpy(tokens).cuda(), torch.from_numpy(lens).cuda(), no_eos, out.view)
    torch.cuda.synchronize()
    out.assert_intact("st_bias_score_seq: out")
    got = out.view.cpu().numpy()
    want = np.concatenate([0.25 * (1 + np.arange(V) % 4), np.zeros(64)]).astype(np.float32).reshape(81, 64)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got), _bits(emul.score_seq(t, tokens, lens, no_eos)))


@pytest.mark.parametrize("Bn,beam", [(1, 1), (5, 4), (3, 16)])
def test_bias_advance_equals_the_numpy_permutation(Bn, beam):
    nv = _nv()
    t = _seven().tables
    state, order, tokens, done = cases.advance_case(t, Bn, beam, 10 * Bn + beam)
    want = emul.advance(t, state, order, tokens, EOS, beam, done)
    if Bn > 1:
        live = ~np.repeat(done, beam)
        assert np.array_equal(want[-beam:], state[-beam:]) and (state[order[live]] < 0).any() and (tokens[live] == EOS).any()
        assert len(set(order[:beam])) == beam and (order[:beam] != np.arange(beam)).all()        # every parent overwritten
        assert len(set(order[beam:2 * beam])) < beam                                              # duplicated parents
        assert (want[live] > 0).any()
    gd = Guarded.vec(Bn * beam, I32, "cuda")
    gd.view.copy_(torch.from_numpy(state))
    nv.bias_advance(t, gd.view, torch.from_numpy(order).cuda(), torch.from_numpy(tokens).cuda(), torch.from_numpy(done).cuda(), EOS, beam)
    torch.cuda.synchronize()
    gd.assert_intact("st_bias_advance: state")
    assert np.array_equal(gd.view.cpu().numpy(), want)


@pytest.mark.parametrize("w", [0.3, 0.0])
def test_five_chained_steps_match_the_torch_formulation(w):
    from tests.test_ngram_gpu import chain_logits, chain_state
    nv = _nv()
    Bn, beam, K, V, S = 3, 4, 6, 30, 6
    scale = 0.5 / (1 - w)
    bias = cases.chain_bias(V, 9).to("cuda")            # (a phrase set under which the draws below meet every case asserted at the end)
    t = bias.tables
    n = Bn * beam
    g = torch.Generator().manual_seed(11)
    st = chain_state(Bn, beam, S)
    dev = {k: v.cuda() for k, v in st.items()}
    state = torch.zeros(n, dtype=I32, device="cuda")
    step = torch.zeros(1, dtype=torch.long, device="cuda")
    ticket = torch.zeros(1, dtype=torch.long, device="cuda")
    ids = torch.empty(n, K, dtype=I32, device="cuda")
    lp = torch.empty(n, K, device="cuda")
    seen_frozen = seen_boost = False
    for step_no in range(S - 1):
        for attempt in range(4):
            logits = chain_logits(V, n, step_no, g)
            nv.beam_pre_beam(logits.cuda(), V, ids, lp)
            delta = -torch.rand(n, K, generator=g) * 3
            delta[torch.rand(n, K, generator=g) < 0.1] = float("-inf")
            full = dict(st, cand_gam=torch.zeros(n, K, 2, 2), cand_psi=torch.zeros(n, K))
            state_h = state.cpu().numpy()
            want, state_want, margin = cases.chain_reference(full, state_h, ids.cpu(), lp.cpu(), delta if w > 0 else torch.zeros_like(delta),
                                                             t, scale, w, beam, K, step_no)
            if margin > 4.0:                               # every selection boundary is wider than 4x the comparison's tolerance
                break
        assert margin > 4.0, "no well-separated draw in 1 + 3 attempts"
        seen_frozen = seen_frozen or bool(((state_h < 0) & ~np.repeat(st["done"].numpy(), beam)).any())
        nv.bias_score(t, state, ids, dev["done"], EOS, scale, lp=lp)
        nv.beam_advance_joint(ids, lp, delta.cuda(), w, beam, step, EOS, dev["scores"], dev["tokens"], dev["done"], dev["lengths"],
                              dev["hist"], dev["back"], dev["toks"], dev["order"], anc=dev["anc"], advance_step=True, ticket=ticket)
        nv.bias_advance(t, state, dev["order"], dev["tokens"], dev["done"], EOS, beam)
        assert int(step) == step_no + 1
        for k in ("back", "toks", "order", "tokens", "lengths", "done", "anc"):
            assert torch.equal(dev[k].cpu(), want[k].to(dev[k].dtype)), (step_no, k)
        assert np.array_equal(state.cpu().numpy(), state_want), step_no
        seen_boost = seen_boost or bool((state_want > 0).any())
        for k in ("scores", "hist"):
            a, b = dev[k].cpu(), want[k].float()
            fin = torch.isfinite(b)
            assert torch.equal(torch.isfinite(a), fin) and torch.allclose(a[fin], b[fin], atol=1e-5, rtol=1e-6), (step_no, k)
        st = {k: dev[k].cpu() for k in st}
    assert seen_frozen and seen_boost and bool(st["done"][0]) and not bool(st["done"].all())


# ---- search on the small decode model -------------------------------------------------------------------------------------------------
def _small():
    from tests.test_ngram_gpu import _small as small
    return small()


def _decode(m, head=True, lm=None, bias=None, use_graph=None, **opt):
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    o = dict(beam_size=4, n_best=2, max_steps=16, ctc_weight=0.3)
    o.update(opt)
    if use_graph is not None:
        o["use_graph"] = use_graph
    return Decode(AttrDict(o), "cuda", model=m["model"], ctc_head=m["head"] if head else None, lm=lm, bias=bias)


_BIAS = {}


def _target_bias(m):
    """Phrases of 2-4 tokens with dyadic weights, cut from what the unbiased searches return (joint, head-less, CTC first pass:
    lists the pre-beam certainly proposes) and from the batch's targets, plus strangers."""
    if not _BIAS:
        rng = np.random.default_rng(8)
        phrases, weights = [], []
        src = (m["x"], m["in_len"])
        found = [h[0][:-1] for h in _decode(m).decode_batch(src)[0]] + [h[0][:-1] for h in _decode(m, head=False).decode_batch(src)[0]]
        found += [h[0] for h in _decode(m).ctc_beam(src)[0]]
        for h in [list(x) for x in found if len(x) >= 2] + m["lists"]:
            for _ in range(2):
                k = int(rng.integers(2, 5))
                i = int(rng.integers(0, max(1, len(h) - k + 1)))
                phrases.append(h[i:i + k])
                weights.append(float(rng.choice([0.25, 0.5, 0.75])))
        for _ in range(10):
            phrases.append([int(x) for x in rng.integers(4, 30, rng.integers(1, 5))])
            weights.append(0.5)
        _BIAS["bias"] = ContextBias.from_phrases(phrases, weights=weights).to("cuda")
    return _BIAS["bias"]


def _truth(m, b, hyp, w, bias, bw, lm=None, lam=0.0):
    """fp64: the joint (or attention) score of ``hyp`` + bias_weight x what a hypothesis carries (its reward, plus the provisional
    part while no EOS has closed it) + lambda x the LM sum."""
    from oracle import beam_oracle as bo
    from tests.test_joint_decode_gpu import _joint_truth
    x, in_len = m["x"], m["in_len"]
    att = bo.score_hypothesis(m["p"], x[b:b + 1].double(), in_len[b:b + 1], 4, hyp)
    truth = _joint_truth(att, m["ctc_lp"][b], in_len[b], hyp, w) if w > 0 else att
    if bias is not None:
        labels = hyp[:-1] if hyp[-1] == EOS else hyp
        truth += bw * bias.reward(labels)
        if hyp[-1] != EOS:
            truth += bw * float(bias.automaton.phi[bias.automaton.state(labels)])
    if lm is not None:
        truth += lam * lm.score_list(hyp)
    return truth


def _check_search_scores(m, h, s, w, bias, bw, lm=None, lam=0.0):
    n_cmp = n_rewarded = 0
    for b in range(m["x"].shape[0]):
        for k in range(len(h[b])):
            hyp = h[b][k]
            if EOS in hyp[:-1]:
                continue                                    # (extended past an EOS below the top: frozen CTC, LM and bias parts -
                                                            #  whether or not a second EOS closes the list)
            truth = _truth(m, b, hyp, w, bias, bw, lm, lam)
            print("utterance %d hypothesis %d: reported %.4f, fp64 %.4f (reward %.3f)" % (b, k, float(s[b][k]), truth, bias.reward(hyp)))
            assert abs(float(s[b][k]) - truth) <= max(0.16, 5e-2 * abs(truth)), (b, k, hyp, float(s[b][k]), truth)
            n_cmp += 1
            n_rewarded += bias.reward(hyp) > 0
    assert n_rewarded > 0, "no returned hypothesis holds a phrase: the comparison would not see the bias term"
    return n_cmp


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_search_joint_route_scores_match_fp64_and_graph_replay_is_exact():
    m = _small()
    src = (m["x"], m["in_len"])
    bias = _target_bias(m)
    graph = _decode(m, bias=bias, bias_weight=0.5, use_graph=True)
    assert graph._bias_on and graph.bias_pre_beam is None and graph.ctc_pre_beam == 6
    outs = [graph.decode_batch(src), graph.decode_batch(src), _decode(m, bias=bias, bias_weight=0.5, use_graph=False).decode_batch(src)]
    assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])
    assert _check_search_scores(m, outs[0][0], outs[0][1], 0.3, bias, 0.5) >= 5


def test_search_bias_only_route_scores_match_fp64_and_graph_replay_is_exact():
    m = _small()
    src = (m["x"], m["in_len"])
    bias = _target_bias(m)
    graph = _decode(m, head=False, bias=bias, bias_weight=0.5, use_graph=True)
    assert graph.bias_pre_beam == 6 and graph.ctc_pre_beam is None and graph.lm_pre_beam is None
    outs = [graph.decode_batch(src), graph.decode_batch(src),
            _decode(m, head=False, bias=bias, bias_weight=0.5, use_graph=False).decode_batch(src)]
    assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])
    assert _check_search_scores(m, outs[0][0], outs[0][1], 0.0, bias, 0.5) >= 5


@pytest.mark.parametrize("head", [True, False])
def test_search_with_lm_and_bias_has_both_terms(head):
    m = _small()
    src = (m["x"], m["in_len"])
    bias = _target_bias(m)
    dec = _decode(m, head=head, lm=m["lm"], bias=bias, lm_weight=0.5, bias_weight=0.5)
    assert dec._lm_on and dec._bias_on
    h, s = dec.decode_batch(src)
    assert _check_search_scores(m, h, s, 0.3 if head else 0.0, bias, 0.5, m["lm"], 0.5) >= 5


def _sub_list(a, b):
    return any(b[i:i + len(a)] == a for i in range(len(b) - len(a) + 1))


@pytest.mark.parametrize("head", [True, False])
def test_a_phrase_turns_the_runner_up_into_the_winner(head):
    """Unbiased n_best = 2; the runner-up (without EOS) becomes the only phrase, weighted so that w |p| exceeds the score gap by
    twice the search bound: the biased search returns a best hypothesis that holds the phrase, at truth + reward.  And with
    bias_weight = 0 or bias = None the search is bit-equal to the unbiased one.  (On the joint route the small model's lists
    run into the step budget without an EOS: the runner-up is then the phrase as it stands.)"""
    m = _small()
    src = (m["x"], m["in_len"])
    w_ctc = 0.3 if head else 0.0
    h0, s0 = _decode(m, head=head).decode_batch(src)
    pick = None
    for b in range(len(h0)):
        win, run = h0[b][0], h0[b][1]
        if EOS in win[:-1] or EOS in run[:-1] or not math.isfinite(float(s0[b][1])):
            continue                                        # (a list extended past an EOS is outside the definition)
        win, run = [k for k in win if k != EOS], [k for k in run if k != EOS]
        if run and not _sub_list(run, win) and not _sub_list(win, run):
            pick = b
            break
    assert pick is not None, "no utterance with two separate hypotheses"
    phrase = [k for k in h0[pick][1] if k != EOS]
    gap = float(s0[pick][0]) - float(s0[pick][1])
    bound = max(0.16, 5e-2 * max(abs(float(s0[pick][0])), abs(float(s0[pick][1]))))
    w = math.ceil(8.0 * (gap + 2.0 * bound) / len(phrase) + 1.0) / 8.0
    assert w * len(phrase) >= gap + 2.0 * bound
    bias = ContextBias.from_phrases([phrase], weight=w).to("cuda")
    h, s = _decode(m, head=head, bias=bias).decode_batch(src)
    best = h[pick][0]
    print("utterance %d: unbiased %s (%.3f) / %s (%.3f); phrase weight %.3f; biased best %s (%.3f)"
          % (pick, h0[pick][0], float(s0[pick][0]), h0[pick][1], float(s0[pick][1]), w, best, float(s[pick][0])))
    assert _sub_list(phrase, best) and best != h0[pick][0]
    truth = _truth(m, pick, best, w_ctc, bias, 1.0)
    assert abs(float(s[pick][0]) - truth) <= max(0.16, 5e-2 * abs(truth)), (float(s[pick][0]), truth)
    assert float(s[pick][0]) > float(s0[pick][0])
    for dec in (_decode(m, head=head, bias=bias, bias_weight=0.0), _decode(m, head=head, bias=None, bias_weight=2.0)):
        assert not dec._bias_on
        assert _same(dec.decode_batch(src), (h0, s0))


def test_two_pass_without_bias_or_with_zero_weight_is_bit_equal():
    m = _small()
    src = (m["x"], m["in_len"])
    bias = _target_bias(m)
    plain = _decode(m, n_best=3).decode_two_pass(src, beam=4)
    assert _same(_decode(m, n_best=3, bias=bias).decode_two_pass(src, beam=4, bias_weight=0.0), plain)
    assert _same(_decode(m, n_best=3, bias=bias, bias_weight=0.0).decode_two_pass(src, beam=4), plain)
    assert _same(_decode(m, n_best=3, bias=None, bias_weight=3.0).decode_two_pass(src, beam=4), plain)
    with pytest.raises(ValueError, match="context bias"):
        _decode(m, n_best=3).decode_two_pass(src, beam=4, bias_weight=1.0)


def test_swapping_bias_objects_under_graph_replay_gives_each_its_own_result():
    """decode_batch captures its step per call, with the tables of the bias it was given: A, then B, then A again on ONE Decode
    equal what fresh objects return, and A and B differ."""
    m = _small()
    src = (m["x"], m["in_len"])
    a = _target_bias(m)
    h0, _ = _decode(m).decode_batch(src)
    other = [h0[b][1][:-1] for b in range(len(h0)) if len(h0[b][1]) > 2]
    b_ = ContextBias.from_phrases(other, weight=2.0).to("cuda")
    dec = _decode(m, bias=a, use_graph=True)
    first = dec.decode_batch(src)
    dec.set_bias(b_)
    second = dec.decode_batch(src)
    dec.set_bias(a)
    third = dec.decode_batch(src)
    dec.set_bias(None)
    fourth = dec.decode_batch(src)
    assert _same(first, _decode(m, bias=a, use_graph=True).decode_batch(src)) and _same(first, third)
    assert _same(second, _decode(m, bias=b_, use_graph=True).decode_batch(src))
    assert _same(fourth, _decode(m, use_graph=True).decode_batch(src))
    assert not _same(first, second) and not _same(second, fourth)
    with pytest.raises(ValueError, match="lives on"):
        dec.set_bias(cases.seven())


def test_decode_two_pass_with_bias_combines_the_scores():
    """decode_two_pass with an LM and a bias: every score is (1 - w) score_nbest + w ctc_beam's + lambda lm_score + beta (len + 1) +
    bias_weight bias_score of its hypothesis, computed separately, within fp32 rounding of the sum (2^-23 x the terms'
    magnitudes); sorted; and bias_score equals the fp64 definition over the rounded tables within the walk's bound summed over the
    positions (+ the fp64 sum's and the final fp32 rounding's)."""
    from st_amd import ctc_beam
    from st_amd.arena import arena_of
    m = _small()
    src = (m["x"], m["in_len"])
    bias = _target_bias(m)
    w, lam, beta, bw, beam = 0.3, 0.5, 0.25, 0.75, 4
    for with_lm in (True, False):
        dec = _decode(m, lm=m["lm"] if with_lm else None, bias=bias, n_best=3, lm_weight=lam, lm_length_bonus=beta, bias_weight=bw)
        hyps, scores = dec.decode_two_pass(src, beam=beam)
        with arena_of(dec.model).scope():
            enc, in_rows = dec._encode(src)
            first, ctc = ctc_beam.search_rows(m["head"], enc, in_rows, beam, max_len=15).lists()
        att = dec.score_nbest(src, first).double().cpu()
        lms = dec.lm_score(first).double().cpu() if with_lm else None
        bs = dec.bias_score(first)
        assert bs.dtype == F32 and tuple(bs.shape) == (5, beam) and bs.is_cuda
        bs = bs.double().cpu()
        ref = bias.tables.rounded_model()
        n_cmp = n_rewarded = 0
        for b in range(5):
            s = scores[b].double().cpu()
            assert all(s[i] >= s[i + 1] for i in range(2)), (b, s)
            want = {}
            for j, hyp in enumerate(first[b]):
                if ctc[b, j] == float("-inf"):
                    continue
                terms = [(1.0 - w) * float(att[b, j]), w * float(ctc[b, j]), bw * float(bs[b, j])]
                if with_lm:
                    terms += [lam * float(lms[b, j]), beta * (len(hyp) + 1)]
                want[tuple(hyp)] = (sum(terms), sum(abs(v) for v in terms))
                pos = []
                inc = emul.score_seq(bias.tables, np.array([hyp + [EOS]], dtype=np.int32), np.array([len(hyp) + 1]), EOS, pos)[0]
                total = ref.reward(hyp)
                bound = (sum(emul.walk_bound(p) for p in pos) + len(inc) * 2.0 ** -53 * float(np.abs(inc).astype(np.float64).sum())
                         + 2.0 ** -24 * abs(total))
                assert abs(float(bs[b, j]) - total) <= bound, (b, j, float(bs[b, j]), total, bound)
                assert abs(total - bias.reward(hyp)) <= 2.0 ** -23 * max(1.0, total) * len(hyp)
                n_rewarded += total > 0
            for i, hyp in enumerate(hyps[b]):
                if s[i] == float("-inf"):
                    assert hyp == [] and i >= len(want)
                    continue
                exp, mag = want[tuple(hyp[:-1])]
                assert hyp[-1] == EOS and abs(float(s[i]) - exp) <= 2.0 ** -23 * mag, (b, i, float(s[i]), exp)
                n_cmp += 1
        assert n_cmp >= 5 and n_rewarded > 0

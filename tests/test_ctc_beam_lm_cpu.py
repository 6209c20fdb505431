"""CPU side of the n-gram fusion inside the CTC prefix beam search: the fp64 reference (tests/_ctc_beam_lm_ref.py) against brute
force on tiny lattices, the pinned scan that shows the fused search is not a reordering of the LM-less n-best, the frame-local
check against the reference's own trace and against planted faults, and the option / argument errors of the Python layer (they
are raised before any launch, so CPU tensors reach them)."""
import itertools

import numpy as np
import pytest
import torch

import transformer.Constants as C
from st_amd import ctc_beam, native
from st_amd.ngram import NGramLM
from tests import _ctc_beam_lm_ref as lmr
from tests import _ctc_beam_ref as ref

NINF = float("-inf")
I32, F32 = torch.int32, torch.float32


def _scorer(order=3, lam=0.8, beta=0.5, V=12):
    return lmr.Scorer(lmr.estimated(order, V).trie, lam, beta, C.BOS, C.EOS)


def _tiny(T, seed, classes=(0, 5, 7), V=12):
    """A lattice over 3 classes (the blank and two labels the model knows) inside a vocabulary of V: the others at -inf."""
    x = lmr.lsm(np.random.default_rng(seed).standard_normal((T, 3)) * 2.0)
    lpf = np.full((T, V), -np.inf, dtype=np.float32)
    lpf[:, list(classes)] = x
    return lpf


@pytest.mark.parametrize("T", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("order,final_eos", [(2, True), (3, True), (4, False)])
def test_reference_best_is_the_brute_force_argmax_on_tiny_lattices(T, order, final_eos):
    sc = _scorer(order)
    for seed in range(4):
        lpf = _tiny(T, 100 * T + seed)
        ids, lp, lpb = ref.inputs_of(lpf, 3, 0) if T else (np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
        res = lmr.search(ids, lp, lpb, 0, 64, 255, sc, final_eos=final_eos)      # 2^(T + 1) - 1 <= 63 label sequences: none pruned
        want = {}
        for n in range(T + 1):
            for labels in itertools.product((5, 7), repeat=n):
                like = ref.ctc_likelihood(lpf, labels, 0)
                if like > NINF:
                    want[labels] = (like, sc.G(labels) + (sc.eos_term(labels) if final_eos else 0.0))
        assert set(h[0] for h in res.hyps) == set(want), (T, seed)
        for labels, score, fused in res.hyps:
            assert abs(score - want[labels][0]) <= 1e-12 * max(1.0, abs(score)) and abs(fused - want[labels][1]) <= 1e-12 * max(1.0, abs(fused))
        ranks = [s + f for _, s, f in res.hyps]
        assert ranks == sorted(ranks, reverse=True)
        best = max(want, key=lambda k: want[k][0] + want[k][1])
        assert res.hyps[0][0] == best, (T, seed, res.hyps[0][0], best)
        assert res.margin == float("inf")


def test_zero_weights_reduce_to_the_lm_less_reference():
    sc = _scorer(lam=0.0, beta=0.0)
    for seed in range(3):
        lpf = lmr.sticky(40, 12, seed)
        ids, lp, lpb = ref.inputs_of(lpf, 4, 0)
        a, b = lmr.search(ids, lp, lpb, 0, 3, 255, sc), ref.search(ids, lp, lpb, 0, 3, 255)
        assert [(h[0], h[1]) for h in a.hyps] == b.hyps and a.norms == b.norms and all(h[2] == 0.0 for h in a.hyps)
        assert [[r[:4] for r in fr] for fr in a.trace] == b.trace


def test_the_pinned_seeds_qualify_and_the_fused_best_beats_the_rescored_best():
    S = lmr.SCAN
    sc = _scorer(S["order"], S["lam"], S["beta"], S["V"])
    assert len(lmr.PINNED) >= 4
    for seed in lmr.PINNED:
        lpf, (ids, lp, lpb) = lmr.scan_case(seed)
        res = lmr.search(ids, lp, lpb, S["blank"], S["beam"], S["L_cap"], sc)
        assert lmr.margin_ok(res), "seed %d: margins %.3e / %.3e, 100 x bounds %.3e" % (
            seed, res.margin, res.final_margin, 100.0 * (res.bound + res.gbound))
        best = res.hyps[0][0]
        fused_obj = lmr.objective(lpf, best, S["blank"], sc)
        labels, _ = lmr.rescored_best(ids, lp, lpb, S["blank"], S["beam"], S["L_cap"], sc)
        rescored_obj = lmr.objective(lpf, labels, S["blank"], sc)
        print("seed %d: fused best %r objective %.4f, rescored best %r objective %.4f, margin %.4f" % (
            seed, best, fused_obj, labels, rescored_obj, min(res.margin, res.final_margin)))
        assert tuple(labels) != tuple(best) and fused_obj > rescored_obj + 100.0 * (res.bound + res.gbound)


def _own_trace(seed, beam=3, K=4, order=3, final_eos=True, L_cap=255):
    sc = _scorer(order)
    lpf = lmr.sticky(40, 12, seed)
    ids, lp, lpb = ref.inputs_of(lpf, K, 0)
    res = lmr.search(ids, lp, lpb, 0, beam, L_cap, sc, final_eos=final_eos)
    return (ids, lp, lpb, 0, beam, L_cap, sc), list(lmr.trace_arrays(res, beam)), res


@pytest.mark.parametrize("final_eos", [True, False])
def test_check_trace_accepts_the_references_own_trace(final_eos):
    for seed in range(3):
        args, arrs, _ = _own_trace(seed, final_eos=final_eos)
        worst, worst_g, acc = lmr.check_trace(*args, *arrs, final_eos=final_eos)
        assert worst <= 1e-6 and worst_g <= 1e-6 and acc > 0.0
    args, arrs, res = _own_trace(0, L_cap=4)
    lmr.check_trace(*args, *arrs)
    assert max(len(h[0]) for h in res.hyps) <= 4


def test_check_trace_reports_planted_faults():
    args, arrs, res = _own_trace(1)
    recs, tg, norms, score, fused, tokens, lens = arrs
    t_ext = next(t for t, fr in enumerate(res.trace) if any(r[1] >= 0 for r in fr) and t > 3)
    s_ext = next(s for s, r in enumerate(res.trace[t_ext]) if r[1] >= 0)

    def broken(**kw):
        a = dict(recs=[list(fr) for fr in recs], tg=[list(fr) for fr in tg], norms=list(norms), score=list(score), fused=list(fused),
                 tokens=[list(r) for r in tokens], lens=list(lens))
        for k, fn in kw.items():
            fn(a[k])
        return [a[k] for k in ("recs", "tg", "norms", "score", "fused", "tokens", "lens")]

    def g_off(tg_):                        # a new slot's g without the length bonus
        tg_[t_ext][s_ext] -= 0.5

    def g_moved(tg_):                      # a kept prefix whose g changed by one ulp-ish step
        t = next(t for t, fr in enumerate(res.trace) if fr[0][1] < 0 and t > 0)
        tg_[t][0] = float(np.nextafter(np.float32(tg_[t][0]), np.float32(1e9))) if tg_[t][0] != 0.0 else 1e-30

    def fused_plain(f):                    # the EOS term forgotten
        f[0] = res.trace[-1][0][4] if res.hyps[0][0] == () else f[0] - 1.0

    def swapped(a):                        # the final order not by rank
        a[0], a[-1] = a[-1], a[0]

    with pytest.raises(AssertionError, match="g "):
        lmr.check_trace(*args, *broken(tg=g_off))
    with pytest.raises(AssertionError, match="kept prefix"):
        lmr.check_trace(*args, *broken(tg=g_moved))
    with pytest.raises(AssertionError, match="fused"):
        lmr.check_trace(*args, *broken(fused=fused_plain))
    with pytest.raises(AssertionError, match="final order"):
        lmr.check_trace(*args, *broken(score=swapped, fused=swapped, tokens=swapped, lens=swapped))
    # the LM-less selection offered as the fused one: a frame keeps a candidate the rank drops
    ids, lp, lpb = args[:3]
    plain = ref.search(ids, lp, lpb, 0, 3, 255)
    if [h[0] for h in plain.hyps] != [h[0] for h in res.hyps]:
        sc = args[-1]
        p_recs, p_norms, _ = ref.trace_arrays(plain, 3)
        labels_at = [[()]]
        for fr in plain.trace:
            labels_at.append([labels_at[-1][r[0]] + ((r[1],) if r[1] >= 0 else ()) for r in fr])
        p_tg = [[sc.G(h) for h in row] + [NINF] * (3 - len(row)) for row in labels_at[1:]]
        with pytest.raises(AssertionError):
            lmr.check_trace(*args, p_recs, p_tg, p_norms, score, fused, tokens, lens)


# ---- the Python layer: options and arguments ------------------------------------------------------------------------------------------
def test_check_lm_options():
    lm = lmr.estimated(3, 12)
    assert ctc_beam.check_lm(None, None, None) == (0.0, 0.0, False)
    assert ctc_beam.check_lm(lm, 0.0, 0.0) == (0.0, 0.0, False)
    assert ctc_beam.check_lm(None, 0.0, 0.0, V=99) == (0.0, 0.0, False)
    assert ctc_beam.check_lm(lm, 0.5, None, V=12, device="cpu") == (0.5, 0.0, True)
    assert ctc_beam.check_lm(lm, 0.0, -0.25) == (0.0, -0.25, True)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_weight"):
            ctc_beam.check_lm(lm, bad, 0.0)
    with pytest.raises(ValueError, match="lm_weight"):
        ctc_beam.check_lm(lm, 0.5, float("inf"))
    for lam, beta in ((0.5, 0.0), (0.0, 0.5)):
        with pytest.raises(ValueError, match="need a language model"):
            ctc_beam.check_lm(None, lam, beta)
    with pytest.raises(ValueError, match="vocabulary"):
        ctc_beam.check_lm(lm, 0.5, 0.0, V=30)
    with pytest.raises(ValueError, match="device trie"):
        ctc_beam.check_lm(NGramLM.estimate([[4, 5]], 2, 12), 0.5, 0.0)
    with pytest.raises(ValueError, match="lives on"):
        ctc_beam.check_lm(lm, 0.5, 0.0, device="cuda")


def test_nbest_carries_fused_and_cuts_it_with_the_lists():
    t, n, s, f = torch.zeros(2, 4, 5, dtype=I32), torch.ones(2, 4, dtype=I32), torch.zeros(2, 4), torch.arange(8.0).view(2, 4)
    plain = ctc_beam.NBest(t, n, s)
    assert plain.fused is None and plain.head(2).fused is None and plain.head(4) is plain
    cut = ctc_beam.NBest(t, n, s, f).head(3)
    assert tuple(cut.fused.shape) == (2, 3) and tuple(cut.tokens.shape) == (2, 3, 5) and torch.equal(cut.fused, f[:, :3])


def test_decode_first_pass_options():
    from transformer.Decode import Decode
    lm = lmr.estimated(3, 12)
    dec = Decode.__new__(Decode)
    dec.lm, dec.ctc_lm_weight, dec.ctc_lm_length_bonus = None, 0.0, 0.0
    assert dec._first_pass_lm("ctc_beam", None, None) == (0.0, 0.0)
    with pytest.raises(ValueError, match="need a language model"):
        dec._first_pass_lm("ctc_beam", 0.5, None)
    dec.lm = lm
    assert dec._first_pass_lm("ctc_beam", None, None) == (0.0, 0.0)          # (NOT opt.lm_weight: the first pass is off by default)
    assert dec._first_pass_lm("ctc_beam", 0.5, None) == (0.5, 0.0)
    dec.ctc_lm_weight, dec.ctc_lm_length_bonus = 0.25, 0.5
    assert dec._first_pass_lm("decode_two_pass", None, None) == (0.25, 0.5)
    assert dec._first_pass_lm("decode_two_pass", 0.0, 0.0) == (0.0, 0.0)
    with pytest.raises(ValueError, match="decode_two_pass: lm_weight"):
        dec._first_pass_lm("decode_two_pass", -1.0, None)


def _args(B=2, R=10, K=3, beam=4, L=6):
    return dict(ids=torch.zeros(R, K, dtype=I32), lp=torch.zeros(R, K), lpb=torch.zeros(R), off=torch.zeros(B, dtype=I32),
                length=torch.zeros(B, dtype=I32), blank=0, tokens=torch.zeros(B, beam, L, dtype=I32), lens=torch.zeros(B, beam, dtype=I32),
                score=torch.zeros(B, beam), trie=lmr.estimated(3, 12).trie, bos=C.BOS, eos=C.EOS, scale=0.5, bias=0.0,
                fused=torch.zeros(B, beam))


def test_wrapper_argument_checks():
    """Every check of ctc_beam_search_lm is made before the library is touched: CPU tensors pass the shape checks and stop at
    'must live on the GPU'."""
    call = native.ctc_beam_search_lm
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        call(**_args())
    with pytest.raises(ValueError, match="beam and K"):
        call(**_args(beam=17))
    with pytest.raises(ValueError, match="lp must be"):
        call(**dict(_args(), lp=torch.zeros(10, 4)))
    with pytest.raises(ValueError, match="go together"):
        call(**dict(_args(), trace=torch.zeros(2, 5, 4, 16, dtype=torch.uint8)))
    assert "ctc_beam_search_lm" in [n[3:] for n in native.SIGNATURES]
    assert len(native.SIGNATURES["st_ctc_beam_search_lm"]) == len(native.SIGNATURES["st_ctc_beam_search"]) + 15

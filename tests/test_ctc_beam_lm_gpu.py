"""-m gpu: st_ctc_beam_search_lm (csrc/st_ctc_beam.hip with the n-gram model fused into the search) against the fp64 reference of
tests/_ctc_beam_lm_ref.py, and the decode entry points that reach it (Decode.ctc_beam / decode_two_pass with a first-pass weight).

As for the LM-less kernel, the search is checked FRAME BY FRAME through its trace (``lmr.check_trace``: the beam before a frame is
the kernel's own - labels, pb, pnb and g as it wrote them - and membership, values, g, the selection by rank and the normaliser
are held to the bounds DERIVED in the reference's docstring); whole hypotheses are compared only where the reference's margins are
at least 100 times the accumulated bounds.  The LM side has exact checks of its own: with lambda = 1, beta = 0 every g is the
NumPy float32 running sum of tests/_emul_ngram.py's scores bit for bit (lookups, per-prefix history and cache), with lambda =
beta = 0 every output is the LM-less kernel's bit for bit.  All seven buffers of a launch sit between guard bands."""
import numpy as np
import pytest
import torch

import transformer.Constants as C
from tests import _ctc_beam_lm_ref as lmr
from tests import _ctc_beam_ref as ref
from tests import _emul_ngram as emul
from tests._local import Guarded
from tests.test_ctc_beam_gpu import Case, _launch, _nv, _ragged

pytestmark = pytest.mark.gpu

I32, F32 = torch.int32, torch.float32
NINF = float("-inf")


def _launch_lm(case, beam, L_cap, trie, lam, beta, final_eos=True, trace=True, dev=None):
    """One st_ctc_beam_search_lm launch into guarded buffers -> dict of numpy arrays, guards checked."""
    nv = _nv()
    B, T = case.B, max(case.T, 1)
    g_tok = Guarded.vec(B * beam * L_cap, I32, "cuda")
    g_len = Guarded.vec(B * beam, I32, "cuda")
    g_sc = Guarded.vec(B * beam, F32, "cuda")
    g_fu = Guarded.vec(B * beam, F32, "cuda")
    g_tr = Guarded.vec(B * T * beam * 16, torch.uint8, "cuda", pad=64)
    g_nm = Guarded.vec(B * T, torch.float64, "cuda")
    g_tg = Guarded.vec(B * T * beam, F32, "cuda")
    tokens, lens, score, fused = (g_tok.view.view(B, beam, L_cap), g_len.view.view(B, beam), g_sc.view.view(B, beam),
                                  g_fu.view.view(B, beam))
    tr, nm, tg = g_tr.view.view(B, T, beam, 16), g_nm.view.view(B, T), g_tg.view.view(B, T, beam)
    ids, lp, lpb, off, length = dev if dev is not None else case.device()
    nv.ctc_beam_search_lm(ids, lp, lpb, off, length, case.blank, tokens, lens, score, trie, C.BOS, C.EOS, lam, beta, fused,
                          final_eos=final_eos, trace=tr if trace else None, trace_norm=nm if trace else None,
                          trace_g=tg if trace else None)
    torch.cuda.synchronize()
    for gd, what in ((g_tok, "tokens"), (g_len, "lens"), (g_sc, "score"), (g_fu, "fused"), (g_tr, "trace"), (g_nm, "trace_norm"),
                     (g_tg, "trace_g")):
        gd.assert_intact("st_ctc_beam_search_lm: " + what)
    raw = tr.cpu().numpy()
    return dict(tokens=tokens.cpu().numpy(), lens=lens.cpu().numpy(), score=score.cpu().numpy(), fused=fused.cpu().numpy(),
                rec_i=raw.view(np.int32).reshape(B, T, beam, 4), rec_f=raw.view(np.float32).reshape(B, T, beam, 4),
                norms=nm.cpu().numpy(), tg=tg.cpu().numpy())


def _trace_of(out, b, n, beam):
    ri, rf = out["rec_i"][b], out["rec_f"][b]
    return [[(int(ri[t, s, 0]), int(ri[t, s, 1]), float(rf[t, s, 2]), float(rf[t, s, 3])) for s in range(beam)] for t in range(n)]


def _check_utterance(case, out, b, beam, L_cap, scorer, final_eos=True):
    n = case.lens[b]
    ids, lp, lpb = case.per[b]
    try:
        return lmr.check_trace(ids, lp, lpb, case.blank, beam, L_cap, scorer, _trace_of(out, b, n, beam), out["tg"][b, :n],
                               out["norms"][b, :n], out["score"][b], out["fused"][b], out["tokens"][b], out["lens"][b], final_eos=final_eos)
    except AssertionError as e:
        raise AssertionError("utterance %d (len %d): %s" % (b, n, e)) from None


def _mix(T, B, V, seed, period, lens=None, sharp=2.0):
    lens = _ragged(T, B, seed) if lens is None else lens
    lpf = np.stack([lmr.sticky(T, V, 1000 * seed + b, period=period, sharp=sharp) for b in range(B)])
    return lpf, lens


def _short(T, B, seed):
    """A ragged mix that holds the lengths 0, 1 and 2."""
    rng = np.random.default_rng(seed)
    return ([T, 0, 1, 2, T - 1] + [int(rng.integers(0, T + 1)) for _ in range(B)])[:B]


def _no_nan(out):
    for k in ("score", "fused"):
        assert not np.isnan(out[k]).any(), k + " holds a NaN"


# ---- 1. lambda = beta = 0 with a model bound: the LM-less kernel bit for bit -------------------------------------------------------
@pytest.mark.parametrize("T,beam,K,V", [(40, 3, 4, 12), (24, 16, 16, 40)])
def test_zero_weights_with_a_model_are_bit_equal_to_the_lm_less_kernel(T, beam, K, V):
    B = 10
    lpf, lens = _mix(T, B, V, T + beam, 4, _short(T, B, T))
    case = Case(lpf, lens, K)
    trie = lmr.estimated(3, V, device="cuda").trie
    plain = _launch(case, beam, 255)
    for final_eos in (True, False):
        out = _launch_lm(case, beam, 255, trie, 0.0, 0.0, final_eos=final_eos)
        for k in ("tokens", "lens", "score", "norms"):
            a, b_ = out[k], plain[k]
            if k == "norms":
                a, b_ = (np.concatenate([x[i, :n] for i, n in enumerate(lens)]) for x in (a, b_))
            assert np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b_).view(np.int32)), k
        for b, n in enumerate(lens):
            assert np.array_equal(out["rec_i"][b, :n], plain["rec_i"][b, :n]), "the trace of utterance %d differs" % b
            live = out["rec_i"][b, :n, :, 0] >= 0
            assert (out["tg"][b, :n][live] == 0.0).all() and (out["tg"][b, :n][~live] == NINF).all()
        assert ((out["fused"] == 0.0) == (out["score"] > NINF)).all() and ((out["fused"] == NINF) == (out["score"] == NINF)).all()


# ---- 2. lambda = 1, beta = 0: g is the float32 running sum of the emulation's scores -----------------------------------------------
@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_g_is_bit_equal_to_the_float32_running_sum_of_the_emulated_scores(order):
    T, B, V, beam, K = 40, 6, 40, 8, 8
    lpf, lens = _mix(T, B, V, 50 + order, 4)
    case = Case(lpf, lens, K)
    trie = lmr.estimated(order, V, device="cuda").trie
    out = _launch_lm(case, beam, 255, trie, 1.0, 0.0)
    sums, n_cmp, longest = {(): np.float32(0.0)}, 0, 0

    def g32(labels):
        if labels not in sums:
            hist = ([-1] * 4 + [C.BOS] + list(labels[:-1]))[-(order - 1):]
            with np.errstate(invalid="ignore"):
                sums[labels] = np.float32(g32(labels[:-1]) + emul.score(trie, hist, labels[-1]))
        return sums[labels]

    for b, n in enumerate(lens):
        prev = [()]
        for t in range(n):
            cur = []
            for s in range(beam):
                p, tok = int(out["rec_i"][b, t, s, 0]), int(out["rec_i"][b, t, s, 1])
                if p < 0:
                    assert out["tg"][b, t, s] == NINF
                    continue
                labels = prev[p] + ((tok,) if tok >= 0 else ())
                cur.append(labels)
                assert np.float32(out["tg"][b, t, s]).view(np.int32) == g32(labels).view(np.int32), (b, t, s, labels, out["tg"][b, t, s], g32(labels))
                n_cmp += 1
                longest = max(longest, len(labels))
            prev = cur
    print("order %d: %d values of g compared, prefixes up to %d labels" % (order, n_cmp, longest))
    assert n_cmp > 500 and longest >= order


# ---- 3. the frame-local check on ragged mixes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [16, 1])
@pytest.mark.parametrize("T,beam,K,V,order", [(40, 3, 4, 12, 2), (64, 10, 10, 60, 4), (32, 16, 16, 40, 5), (24, 1, 1, 8, 3)])
def test_every_frame_of_a_ragged_mix_passes_the_frame_local_check(T, beam, K, V, order, period):
    B = 9
    lpf, lens = _mix(T, B, V, T + order + period, period, sharp=2.0 if K > 1 else 0.0)
    case = Case(lpf, lens, K)
    lm = lmr.estimated(order, V, device="cuda")
    sc = lmr.Scorer(lm.trie, 0.8, 0.5, C.BOS, C.EOS)
    out = _launch_lm(case, beam, 255, lm.trie, 0.8, 0.5)
    _no_nan(out)
    worst = worst_g = 0.0
    for b in range(B):
        w, wg, _ = _check_utterance(case, out, b, beam, 255, sc)
        worst, worst_g = max(worst, w), max(worst_g, wg)
        if lens[b] == 0:
            assert out["score"][b, 0] == 0.0 and out["lens"][b, 0] == 0 and (out["score"][b, 1:] == NINF).all()
    print("T %d beam %d K %d V %d order %d period %d: worst CTC error / bound %.3f, worst g error / bound %.3f, longest %d" % (
        T, beam, K, V, order, period, worst, worst_g, out["lens"].max()))
    assert out["lens"].max() >= 2


# ---- 4. the pinned seeds of the CPU scan ---------------------------------------------------------------------------------------------
def test_pinned_seeds_return_the_references_hypotheses_in_its_order():
    S = lmr.SCAN
    lm = lmr.estimated(S["order"], S["V"], device="cuda")
    sc = lmr.Scorer(lm.trie, S["lam"], S["beta"], C.BOS, C.EOS)
    lpf = np.stack([lmr.scan_case(seed)[0] for seed in lmr.PINNED])
    case = Case(lpf, [S["T"]] * len(lmr.PINNED), S["K"])
    out = _launch_lm(case, S["beam"], S["L_cap"], lm.trie, S["lam"], S["beta"])
    plain = _launch(case, S["beam"], S["L_cap"])
    moved = 0
    for b, seed in enumerate(lmr.PINNED):
        ids, lp, lpb = case.per[b]
        res = lmr.search(ids, lp, lpb, 0, S["beam"], S["L_cap"], sc)
        assert lmr.margin_ok(res), seed
        got = [tuple(int(k) for k in out["tokens"][b, j, :out["lens"][b, j]]) for j in range(S["beam"]) if out["score"][b, j] > NINF]
        assert got == [h[0] for h in res.hyps], "seed %d: %r, the reference %r" % (seed, got, [h[0] for h in res.hyps])
        for j, (labels, score, fused) in enumerate(res.hyps):
            tol = res.bound + 2.0 * ref.EPS * max(1.0, abs(score)) + (5.0 + abs(score - res.norms[-1])) * ref.EPS
            assert abs(float(out["score"][b, j]) - score) <= tol, (seed, j, float(out["score"][b, j]), score, tol)
            ftol = sc.gbound(labels) + lmr.gb(sc.eos_term(labels), fused)
            assert abs(float(out["fused"][b, j]) - fused) <= ftol, (seed, j, float(out["fused"][b, j]), fused, ftol)
        moved += got[0] != tuple(int(k) for k in plain["tokens"][b, 0, :plain["lens"][b, 0]])
    assert moved >= len(lmr.PINNED) // 2, "the fused search returns the LM-less best almost everywhere: %d of %d moved" % (moved, len(lmr.PINNED))


# ---- 5. a vetoed token ---------------------------------------------------------------------------------------------------------------
def test_a_token_without_a_unigram_and_oov_minus_inf_is_in_no_returned_list():
    from st_amd.ngram import NGramLM
    T, B, V, beam, K = 40, 6, 12, 4, 4
    lpf, lens = _mix(T, B, V, 77, 4, [T] * B)
    case = Case(lpf, lens, K)
    plain = _launch(case, beam, 255)
    used = sorted(set(int(k) for k in plain["tokens"][:, 0].ravel() if k >= 4))
    assert used, "the LM-less best lists hold no label of the model"
    tok = used[0]
    base = lmr.estimated(3, V)
    veto = NGramLM.from_table({g: v for g, v in base.table.items() if tok not in g}, 3, V, oov_logp=NINF).to("cuda")
    out = _launch_lm(case, beam, 255, veto.trie, 0.8, 0.5)
    _no_nan(out)
    assert not np.isnan(out["tg"][:, :T]).any() and not np.isnan(out["rec_f"][:, :T, :, 2:]).any() and not np.isnan(out["norms"]).any()
    assert (plain["tokens"] == tok).any() and not (out["tokens"] == tok).any()
    assert (out["score"][:, 0] > NINF).all() and (out["fused"][:, 0] > NINF).all()
    sc = lmr.Scorer(veto.trie, 0.8, 0.5, C.BOS, C.EOS)
    for b in range(B):
        _check_utterance(case, out, b, beam, 255, sc)


# ---- 6. the EOS term -----------------------------------------------------------------------------------------------------------------
EOS_SEEDS = [152, 202, 252, 283]       # a reference scan of lmr.sticky(48, 12, seed), seeds 0 .. 299: the EOS term reorders the final beam, margins hold


def test_the_eos_term_reorders_the_final_beam_as_the_reference_says():
    S = lmr.SCAN
    lm = lmr.estimated(S["order"], S["V"], device="cuda")
    sc = lmr.Scorer(lm.trie, S["lam"], S["beta"], C.BOS, C.EOS)
    lpf = np.stack([lmr.sticky(S["T"], S["V"], seed) for seed in EOS_SEEDS])
    case = Case(lpf, [S["T"]] * len(EOS_SEEDS), S["K"])
    orders = {}
    for final_eos in (False, True):
        out = _launch_lm(case, S["beam"], 255, lm.trie, S["lam"], S["beta"], final_eos=final_eos)
        for b, seed in enumerate(EOS_SEEDS):
            res = lmr.search(*case.per[b], 0, S["beam"], 255, sc, final_eos=final_eos)
            assert lmr.margin_ok(res), (seed, final_eos)
            got = [tuple(int(k) for k in out["tokens"][b, j, :out["lens"][b, j]]) for j in range(S["beam"]) if out["score"][b, j] > NINF]
            assert got == [h[0] for h in res.hyps], (seed, final_eos, got, [h[0] for h in res.hyps])
            for j, (labels, score, fused) in enumerate(res.hyps):
                ftol = sc.gbound(labels) + lmr.gb(sc.eos_term(labels), fused)
                assert abs(float(out["fused"][b, j]) - fused) <= ftol, (seed, final_eos, j)
            _check_utterance(case, out, b, S["beam"], 255, sc, final_eos=final_eos)
            orders[(seed, final_eos)] = got
    for seed in EOS_SEEDS:
        assert sorted(orders[(seed, False)]) == sorted(orders[(seed, True)]) and orders[(seed, False)] != orders[(seed, True)], seed


# ---- 7. the label capacity -----------------------------------------------------------------------------------------------------------
def test_label_capacity_four_with_longer_posteriors():
    T, B, V, beam, K, L_cap = 40, 6, 12, 4, 4, 4
    lpf, lens = _mix(T, B, V, 91, 4)
    case = Case(lpf, lens, K)
    lm = lmr.estimated(3, V, device="cuda")
    sc = lmr.Scorer(lm.trie, 0.8, 0.5, C.BOS, C.EOS)
    out = _launch_lm(case, beam, L_cap, lm.trie, 0.8, 0.5)
    free = _launch_lm(case, beam, 255, lm.trie, 0.8, 0.5)
    assert out["lens"].max() == L_cap and free["lens"].max() > L_cap
    for b in range(B):
        _check_utterance(case, out, b, beam, L_cap, sc)


# ---- 8. one long utterance -----------------------------------------------------------------------------------------------------------
def test_one_long_utterance_of_2048_frames():
    T, V, beam, K, order, lam, beta = 2048, 40, 4, 4, 4, 0.8, 0.5
    lpf = lmr.sticky(T, V, 5, period=16)[None]
    case = Case(lpf, [T], K)
    lm = lmr.estimated(order, V, device="cuda")
    sc = lmr.Scorer(lm.trie, lam, beta, C.BOS, C.EOS)
    out = _launch_lm(case, beam, 255, lm.trie, lam, beta)
    _no_nan(out)
    worst, worst_g, acc = _check_utterance(case, out, 0, beam, 255, sc)
    exact = lm.trie.rounded_model()
    n_cmp = 0
    for j in range(beam):
        if out["score"][0, j] == NINF:
            continue
        h = [int(k) for k in out["tokens"][0, j, :out["lens"][0, j]]]
        toks, walk = h + [C.EOS], 0.0
        for i, c in enumerate(toks):
            terms = []
            emul.score(lm.trie, ([-1] * 4 + [C.BOS] + toks[:i])[-(order - 1):], c, terms)
            walk += emul.walk_bound(order, terms)
        want = sc.lam * exact.score_list(toks) + sc.beta * (len(h) + 1)
        tol = sc.gbound(tuple(h)) + lmr.gb(sc.eos_term(tuple(h)), want) + sc.lam * walk + 1e-12 * abs(want)
        assert abs(float(out["fused"][0, j]) - want) <= tol, (j, float(out["fused"][0, j]), want, tol)
        n_cmp += 1
    print("T 2048: worst CTC error / bound %.3f, worst g error / bound %.3f, %d labels in the best list" % (worst, worst_g, out["lens"][0, 0]))
    assert n_cmp >= 1 and out["lens"][0, 0] >= 64


# ---- 9. launches and capture ---------------------------------------------------------------------------------------------------------
def test_two_launches_are_bit_equal_and_a_captured_launch_follows_refilled_buffers():
    nv = _nv()
    B, T, V, beam, K, L_cap = 8, 120, 30, 8, 8, 40
    c1 = Case(*_mix(T, B, V, 1, 4), K)
    c2 = Case(*_mix(T, B, V, 2, 1), K)
    trie = lmr.estimated(4, V, device="cuda").trie
    e1, again, e2 = (_launch_lm(c, beam, L_cap, trie, 0.8, 0.5) for c in (c1, c1, c2))
    for k in ("tokens", "lens", "score", "fused"):
        assert np.array_equal(e1[k].view(np.int32), again[k].view(np.int32)), k + " differs between two launches"
    for b, n in enumerate(c1.lens):
        assert np.array_equal(e1["rec_i"][b, :n], again["rec_i"][b, :n]) and np.array_equal(e1["tg"][b, :n].view(np.int32), again["tg"][b, :n].view(np.int32))
        assert np.array_equal(e1["norms"][b, :n], again["norms"][b, :n])
    assert not np.array_equal(e1["tokens"], e2["tokens"])
    bufs = c1.device()
    tokens = torch.zeros(B, beam, L_cap, dtype=I32, device="cuda")
    lens = torch.zeros(B, beam, dtype=I32, device="cuda")
    score = torch.zeros(B, beam, dtype=F32, device="cuda")
    fused = torch.zeros(B, beam, dtype=F32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nv.ctc_beam_search_lm(*bufs, 0, tokens, lens, score, trie, C.BOS, C.EOS, 0.8, 0.5, fused)
    for want, case in ((e1, c1), (e2, c2), (e1, c1)):
        for dst, src in zip(bufs, case.device()):
            dst.copy_(src)
        for t in (tokens, lens, score, fused):
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(tokens.cpu().numpy(), want["tokens"]) and np.array_equal(lens.cpu().numpy(), want["lens"])
        assert np.array_equal(score.cpu().numpy().view(np.int32), want["score"].view(np.int32))
        assert np.array_equal(fused.cpu().numpy().view(np.int32), want["fused"].view(np.int32))


def test_the_c_entry_refuses_bad_arguments():
    nv = _nv()
    case = Case(*_mix(8, 2, 12, 3, 4, [8, 8]), 4)
    trie = lmr.estimated(3, 12, device="cuda").trie
    tokens, lens, score, fused = (torch.zeros(2, 3, 8, dtype=I32, device="cuda"), torch.zeros(2, 3, dtype=I32, device="cuda"),
                                  torch.zeros(2, 3, device="cuda"), torch.zeros(2, 3, device="cuda"))
    for scale, bias in ((-0.5, 0.0), (float("nan"), 0.0), (0.5, float("inf"))):
        with pytest.raises(ValueError, match="scale"):
            nv.ctc_beam_search_lm(*case.device(), 0, tokens, lens, score, trie, C.BOS, C.EOS, scale, bias, fused)
    with pytest.raises(ValueError, match="trace_g goes with"):
        nv.ctc_beam_search_lm(*case.device(), 0, tokens, lens, score, trie, C.BOS, C.EOS, 0.5, 0.0, fused,
                              trace_g=torch.zeros(2, 8, 3, device="cuda"))
    with pytest.raises(ValueError, match="fused"):
        nv.ctc_beam_search_lm(*case.device(), 0, tokens, lens, score, trie, C.BOS, C.EOS, 0.5, 0.0, torch.zeros(2, 4, device="cuda"))
    lib, a = nv.load(), case.device()
    args = [nv._stream(), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), a[4].data_ptr(), 2, 4, 3, 0, 8,
            tokens.data_ptr(), lens.data_ptr(), score.data_ptr(), None, None, 0, trie.child_lo.data_ptr(), trie.tok.data_ptr(),
            trie.logp.data_ptr(), trie.bo.data_ptr(), trie.nodes, trie.V, trie.order, trie.oov_logp, C.BOS, C.EOS, 0.5, 0.0, 1]
    assert lib.st_ctc_beam_search_lm(*args, fused.data_ptr(), None) == 0
    assert lib.st_ctc_beam_search_lm(*args, None, None) == -1                                  # fused NULL
    assert lib.st_ctc_beam_search_lm(*args, fused.data_ptr(), fused.data_ptr()) == -1          # trace_g without trace
    bad = list(args)
    bad[27] = -1.0
    assert lib.st_ctc_beam_search_lm(*bad, fused.data_ptr(), None) == -1                       # scale < 0
    bad[27] = float("nan")
    assert lib.st_ctc_beam_search_lm(*bad, fused.data_ptr(), None) == -1
    bad = list(args)
    bad[23] = 6
    assert lib.st_ctc_beam_search_lm(*bad, fused.data_ptr(), None) == -1                       # order 6
    torch.cuda.synchronize()


# ---- 10. the Decode level ------------------------------------------------------------------------------------------------------------
def test_decode_defaults_are_the_lm_less_first_pass_and_a_weight_sorts_by_the_fused_rank():
    from tests.test_ngram_gpu import _decode, _small
    m = _small()
    src = (m["x"], m["in_len"])
    plain, with_lm = _decode(m, n_best=3), _decode(m, lm=m["lm"], n_best=3, lm_weight=0.5)
    # defaults: opt.lm_weight is NOT the first pass' weight
    a, b = plain.ctc_beam(src), with_lm.ctc_beam(src)
    assert len(b) == 2 and a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    a, b = plain.decode_two_pass(src), _decode(m, lm=m["lm"], n_best=3).decode_two_pass(src)
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    with pytest.raises(ValueError, match="need a language model"):
        plain.ctc_beam(src, lm_weight=0.5)
    with pytest.raises(ValueError, match="lm_weight"):
        with_lm.ctc_beam(src, lm_weight=-0.5)
    with pytest.raises(ValueError, match="need a language model"):
        _decode(m, ctc_lm_weight=0.5)
    # a weight: sorted by score + fused, fused = lambda log p_lm(h . EOS) + beta (|h| + 1) in fp64 over the trie's rounded values
    lam, beta = 0.5, 0.25
    exact = m["lm"].trie.rounded_model()
    for dec, kw in ((with_lm, dict(lm_weight=lam, lm_length_bonus=beta)), (_decode(m, lm=m["lm"], n_best=3, ctc_lm_weight=lam, ctc_lm_length_bonus=beta), {})):
        hyps, scores, fused = dec.ctc_beam(src, **kw)
        n_cmp = 0
        for bi in range(5):
            s, f = scores[bi].double().cpu(), fused[bi].double().cpu()
            assert f.shape == (3,) and fused[bi].is_cuda
            for j, h in enumerate(hyps[bi]):
                if s[j] == NINF:
                    assert f[j] == NINF
                    continue
                want = lam * exact.score_list(list(h) + [C.EOS]) + beta * (len(h) + 1)
                assert abs(float(f[j]) - want) <= 1e-5 * max(1.0, abs(want)), (bi, j, float(f[j]), want)
                n_cmp += 1
            rank = [float(s[j] + f[j]) for j in range(3) if s[j] > NINF]
            assert all(x >= y - 1e-5 * max(1.0, abs(x)) for x, y in zip(rank, rank[1:])), (bi, rank)
        assert n_cmp >= 5


def test_decode_two_pass_with_first_pass_fusion_keeps_the_three_term_score():
    from st_amd import ctc_beam
    from st_amd.arena import arena_of
    from tests.test_ngram_gpu import _decode, _small
    m = _small()
    src = (m["x"], m["in_len"])
    w, lam, beta, beam, lam1 = 0.3, 0.5, 0.25, 4, 0.5
    dec = _decode(m, lm=m["lm"], n_best=3, lm_weight=lam, lm_length_bonus=beta)
    hyps, scores = dec.decode_two_pass(src, beam=beam, first_pass_lm_weight=lam1)
    with arena_of(dec.model).scope():
        enc, in_rows = dec._encode(src)
        nb = ctc_beam.search_rows(m["head"], enc, in_rows, beam, max_len=15, lm=m["lm"], lm_weight=lam1)
        first, ctc = nb.lists()
    assert nb.fused is not None
    att = dec.score_nbest(src, first).double().cpu()
    lms = dec.lm_score(first).double().cpu()
    n_cmp = 0
    for b in range(5):
        s = scores[b].double().cpu()
        assert all(s[i] >= s[i + 1] for i in range(2)), (b, s)
        want = {}
        for j, hyp in enumerate(first[b]):
            if ctc[b, j] == NINF:
                continue
            terms = [(1.0 - w) * float(att[b, j]), w * float(ctc[b, j]), lam * float(lms[b, j]), beta * (len(hyp) + 1)]
            want[tuple(hyp)] = (sum(terms), sum(abs(v) for v in terms))
        ranked = sorted((v[0] for v in want.values()), reverse=True)
        for i, hyp in enumerate(hyps[b]):
            if s[i] == NINF:
                assert hyp == [] and i >= len(want)
                continue
            exp, mag = want[tuple(hyp[:-1])]
            assert hyp[-1] == C.EOS and abs(float(s[i]) - exp) <= 2.0 ** -23 * mag, (b, i, float(s[i]), exp)
            assert abs(float(s[i]) - ranked[i]) <= 2.0 ** -23 * mag, (b, i, float(s[i]), ranked[i])
            n_cmp += 1
    assert n_cmp >= 5
    off = dec.decode_two_pass(src, beam=beam, first_pass_lm_weight=0.0)
    base = dec.decode_two_pass(src, beam=beam)
    assert off[0] == base[0] and all(torch.equal(x, y) for x, y in zip(off[1], base[1]))

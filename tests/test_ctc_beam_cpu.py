"""CPU side of the CTC prefix beam search: the fp64 reference (tests/_ctc_beam_ref.py) against brute force, the frame-local
check against the reference's own trace and against planted faults, the argument checks of the new wrappers (they run before
any launch, so CPU tensors reach them), and the second-pass ranking of decode_two_pass on fabricated scores."""
import itertools
import math

import numpy as np
import pytest
import torch

from st_amd import ctc_beam, native
from tests import _ctc_beam_ref as ref

NINF = float("-inf")


def _lsm(x):
    x = x - x.max(1, keepdims=True)
    return x - np.log(np.exp(x).sum(1, keepdims=True))


def _lattice(V, T, seed, scale=2.0):
    return _lsm(np.random.default_rng(seed).standard_normal((T, V)) * scale).astype(np.float32)


def _brute(lp_full, blank):
    """{labels: log of the summed probability of every alignment that collapses to them}."""
    T, V = lp_full.shape
    out = {}
    for path in itertools.product(range(V), repeat=T):
        labels, prev = [], None
        for k in path:
            if k != prev and k != blank:
                labels.append(k)
            prev = k
        lpp = float(sum(float(lp_full[t, k]) for t, k in enumerate(path)))
        key = tuple(labels)
        out[key] = ref.logadd(out.get(key, NINF), lpp)
    return out


@pytest.mark.parametrize("T", [0, 1, 2, 3])
@pytest.mark.parametrize("blank", [0, 2])
def test_reference_equals_brute_force_where_nothing_is_pruned(T, blank):
    for seed in range(6):
        lpf = _lattice(3, T, 10 * T + seed)
        ids, lp, lpb = ref.inputs_of(lpf, 3, blank)
        res = ref.search(ids, lp, lpb, blank, 16, 255)
        want = _brute(lpf, blank)
        got = dict(res.hyps)
        assert set(got) == set(want), (T, seed, sorted(got), sorted(want))
        for labels, s in got.items():
            assert abs(s - want[labels]) <= 1e-12 * max(1.0, abs(s)), (labels, s, want[labels])
            assert abs(s - ref.ctc_likelihood(lpf, labels, blank)) <= 1e-12 * max(1.0, abs(s))
        scores = [s for _, s in res.hyps]
        assert scores == sorted(scores, reverse=True) and res.margin == float("inf")


def test_reference_label_capacity_and_tie_rule():
    # a flat lattice: every class equally likely - ties everywhere, the lower candidate number (stay before extension, lower
    # slot, lower j) wins; with L_cap = 1 no prefix grows past one label
    lpf = np.full((4, 3), math.log(1.0 / 3.0), dtype=np.float32)
    ids, lp, lpb = ref.inputs_of(lpf, 3, 0)
    assert ids[0].tolist() == [0, 1, 2]
    res = ref.search(ids, lp, lpb, 0, 2, 1)
    assert all(len(h) <= 1 for h, _ in res.hyps)
    first = ref.search(ids[:1], lp[:1], lpb[:1], 0, 2, 255)
    assert [h for h, _ in first.hyps] == [(), (1,)]                 # candidates 0 (stay), 2 + 0 * 3 + 1 (label 1) before label 2
    cap = ref.search(ids, lp, lpb, 0, 16, 1)
    assert sorted(h for h, _ in cap.hyps) == [(), (1,), (2,)]


def _merge_case(V, T, beam, K, seed):
    lpf = _lattice(V, T, seed)
    ids, lp, lpb = ref.inputs_of(lpf, K, 0)
    return ids, lp, lpb, ref.search(ids, lp, lpb, 0, beam, 255)


def test_reference_counts_recreation_merges_and_reports_the_margin():
    ids, lp, lpb, res = _merge_case(3, 40, 3, 3, 41)
    assert res.recreations == 10 and 0.0 < res.margin < 1.0 and res.bound > 40 * 25 * ref.EPS
    assert not ref.margin_ok(res)
    ids, lp, lpb, res = _merge_case(3, 40, 3, 3, 78)
    assert res.recreations >= 1 and ref.margin_ok(res)
    labels = [h for h, _ in res.hyps]
    assert len(set(labels)) == len(labels)


@pytest.mark.parametrize("V,T,beam,K,seed", [(3, 40, 3, 3, 41), (4, 50, 4, 4, 143), (5, 60, 5, 5, 63), (3, 60, 8, 3, 33), (5, 7, 16, 2, 1)])
def test_check_trace_accepts_the_reference_trace(V, T, beam, K, seed):
    ids, lp, lpb, res = _merge_case(V, T, beam, K, seed)
    recs, norms, score = ref.trace_arrays(res, beam)
    worst, acc = ref.check_trace(ids, lp, lpb, 0, beam, 255, recs, norms, score)
    assert worst < 1e-6 and abs(acc - res.bound) <= 1e-9 * acc          # (fp64 against itself; the same accumulated bound)


def _planted():
    ids, lp, lpb, res = _merge_case(4, 50, 4, 4, 143)
    recs, norms, score = ref.trace_arrays(res, 4)
    return ids, lp, lpb, [list(fr) for fr in recs], norms, score


def test_check_trace_rejects_a_duplicated_prefix_with_split_mass():
    ids, lp, lpb, recs, norms, score = _planted()
    t = 20
    prev, token, pb, pnb = recs[t][0]
    half = math.log(0.5)
    split = [list(fr) for fr in recs]
    split[t][0] = (prev, token, pb + half, pnb + half)
    split[t][3] = (prev, token, pb + half, pnb + half)
    with pytest.raises(AssertionError, match="fp64"):              # (each half carries the wrong mass: caught at the first of them)
        ref.check_trace(ids, lp, lpb, 0, 4, 255, split, norms, score)
    recs[t][3] = (prev, token, pb, pnb)                             # ... and even with the right mass a label sequence stands once
    with pytest.raises(AssertionError, match="appears twice"):
        ref.check_trace(ids, lp, lpb, 0, 4, 255, recs, norms, score)


def test_check_trace_rejects_a_swapped_selection_beyond_the_bound():
    ids, lp, lpb, recs, norms, score = _planted()
    # rebuild the beam before frame t from the trace, take the best DROPPED candidate of frame t and put it into the last slot
    t = 20
    entries = [((), 0.0, NINF)]
    for fr in recs[:t]:
        entries = [(entries[p][0] + ((k,) if k >= 0 else ()), pb, pnb) for p, k, pb, pnb in fr if p >= 0]
    cands = ref.frame_candidates(entries, ids[t], [float(x) for x in lp[t]], float(lpb[t]), 0, 4, 255)
    kept, dropped = ref.select(cands, 4)
    assert dropped and kept[-1].total - dropped[0].total > 100 * ref.bound_of(10.0)
    d, best = dropped[0], kept[0].total
    recs[t][3] = (d.slot, d.token, d.pb - best, d.pnb - best)
    with pytest.raises(AssertionError, match="dropped candidate beats a kept one"):
        ref.check_trace(ids, lp, lpb, 0, 4, 255, recs[:t + 1], norms[:t + 1], [NINF] * 4)


def test_check_trace_rejects_a_wrong_normaliser():
    ids, lp, lpb, recs, norms, score = _planted()
    bad = list(norms)
    bad[30] += 1e-3
    with pytest.raises(AssertionError, match="normaliser"):
        ref.check_trace(ids, lp, lpb, 0, 4, 255, recs, bad, score)
    bad = [x + (1e-3 if t >= 49 else 0.0) for t, x in enumerate(norms)]       # (only the last frame: the scores no longer telescope)
    with pytest.raises(AssertionError, match="normaliser"):
        ref.check_trace(ids, lp, lpb, 0, 4, 255, recs, bad, score)
    ref.check_trace(ids, lp, lpb, 0, 4, 255, recs, norms, score)
    with pytest.raises(AssertionError, match="score"):
        ref.check_trace(ids, lp, lpb, 0, 4, 255, recs, norms, [score[0] + 1e-3] + score[1:])


def test_binding_argument_checks_raise_before_any_launch():
    B, R, K, beam, L = 3, 20, 4, 5, 7
    i32, f32 = torch.int32, torch.float32
    ok = dict(ids=torch.zeros(R, K, dtype=i32), lp=torch.zeros(R, K), lpb=torch.zeros(R), off=torch.zeros(B, dtype=i32),
              length=torch.zeros(B, dtype=i32), blank=0, tokens=torch.zeros(B, beam, L, dtype=i32), lens=torch.zeros(B, beam, dtype=i32),
              score=torch.zeros(B, beam))
    tr = dict(trace=torch.zeros(B, 9, beam, 16, dtype=torch.uint8), trace_norm=torch.zeros(B, 9, dtype=torch.float64))
    bad = [dict(ids=torch.zeros(R, K, dtype=torch.int64)), dict(ids=torch.zeros(R, 2 * K, dtype=i32)[:, ::2]), dict(ids=torch.zeros(R * K, dtype=i32)),
           dict(ids=torch.zeros(R, 17, dtype=i32), lp=torch.zeros(R, 17)), dict(lp=torch.zeros(R, K, dtype=torch.float64)),
           dict(lp=torch.zeros(R + 1, K)), dict(lpb=torch.zeros(R, 1)), dict(lpb=torch.zeros(R + 1)), dict(off=torch.zeros(B, dtype=torch.int64)),
           dict(off=torch.zeros(B + 1, dtype=i32)), dict(length=torch.zeros(B + 1, dtype=i32)), dict(length=torch.zeros(B, dtype=torch.int64)),
           dict(tokens=torch.zeros(B, beam, L, dtype=torch.int64)), dict(tokens=torch.zeros(B, beam * L, dtype=i32)),
           dict(tokens=torch.zeros(B, 17, L, dtype=i32), lens=torch.zeros(B, 17, dtype=i32), score=torch.zeros(B, 17)),
           dict(tokens=torch.zeros(B, beam, 256, dtype=i32)), dict(tokens=torch.zeros(B, beam, 0, dtype=i32)),
           dict(tokens=torch.zeros(B, L, beam, dtype=i32).transpose(1, 2)), dict(lens=torch.zeros(B, beam, dtype=torch.int64)),
           dict(lens=torch.zeros(B, beam + 1, dtype=i32)), dict(score=torch.zeros(B, beam, dtype=torch.float64)), dict(score=torch.zeros(B * beam)),
           dict(blank=-1), dict(trace=tr["trace"]), dict(trace_norm=tr["trace_norm"]),
           dict(tr, trace=torch.zeros(B, 9, beam, 4, dtype=f32)), dict(tr, trace=torch.zeros(B, 9, beam + 1, 16, dtype=torch.uint8)),
           dict(tr, trace=torch.zeros(B, 0, beam, 16, dtype=torch.uint8), trace_norm=torch.zeros(B, 0, dtype=torch.float64)),
           dict(tr, trace_norm=torch.zeros(B, 9)), dict(tr, trace_norm=torch.zeros(B, 8, dtype=torch.float64))]
    for change in bad:
        with pytest.raises(ValueError):
            native.ctc_beam_search(**{**ok, **change})
    for good in (ok, dict(ok, **tr)):               # well-formed, but not on the GPU: refused as everywhere in the binding
        with pytest.raises(RuntimeError):
            native.ctc_beam_search(**good)
    # the host-only workspace query: nothing for every supported shape (the label sequences live in LDS)
    assert native.ctc_beam_ws_bytes(32, 2048, 16, 255) == 0 and native.ctc_beam_ws_bytes(1, 100000, 1, 1) == 0
    for args in ((32, 100, 17, 50), (32, 100, 0, 50), (32, 100, 8, 256), (32, 100, 8, 0), (-1, 100, 8, 50), (4, -1, 8, 50)):
        with pytest.raises(ValueError):
            native.ctc_beam_ws_bytes(*args)
    raw = native.load()._cdll.st_ctc_beam_ws_kib
    assert raw(32, 2048, 16, 255) == 0 and raw(32, 10, 17, 255) == -1 and raw(32, 10, 16, 256) == -1 and raw(-1, 10, 4, 4) == -1
    assert "st_ctc_beam.hip" in __import__("st_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "st_ctc_beam_search" in native.SIGNATURES and len(native.SIGNATURES["st_ctc_beam_search"]) == 17


def test_search_width_checks():
    assert ctc_beam.check_widths(30, 4) == (4, 4, 4) and ctc_beam.check_widths(4337, 10, 16, 3) == (10, 16, 3)
    for args in ((5121, 4), (30, 0), (30, 17), (30, 4, 0), (30, 4, 17), (3, 4, 4), (30, 4, None, 5), (30, 4, None, 0)):
        with pytest.raises(ValueError):
            ctc_beam.check_widths(*args)
    assert ctc_beam.label_capacity(1000) == 255 and ctc_beam.label_capacity(7) == 7 and ctc_beam.label_capacity(0) == 1
    assert ctc_beam.label_capacity(1000, 15) == 15
    for cap in (0, 256):
        with pytest.raises(ValueError):
            ctc_beam.label_capacity(100, cap)


def test_two_pass_combine_sorts_by_the_joint_score():
    EOS = 2
    hyps = [[[5, 6], [5], [7, 7, 8], []], [[9], [], [], []]]
    ctc = torch.tensor([[-1.0, -2.0, -3.0, NINF], [-0.5, -4.0, NINF, NINF]])
    att = torch.tensor([[-9.0, -1.0, -2.0, NINF], [-3.0, -1.0, NINF, NINF]])
    w = 0.3
    out, scores = ctc_beam.combine(hyps, ctc, att, w, 3, EOS)
    want0 = sorted([(0.7 * -9.0 + 0.3 * -1.0, [5, 6, EOS]), (0.7 * -1.0 + 0.3 * -2.0, [5, EOS]), (0.7 * -2.0 + 0.3 * -3.0, [7, 7, 8, EOS])],
                   reverse=True)
    assert out[0] == [h for _, h in want0]
    assert torch.allclose(scores[0], torch.tensor([s for s, _ in want0], dtype=torch.float32), rtol=0, atol=1e-6)
    # utterance 1: two live hypotheses (the second one the EMPTY label list: EOS alone), the third slot has none
    assert out[1] == [[EOS], [9, EOS], []]
    assert torch.allclose(scores[1, :2], torch.tensor([0.7 * -1.0 + 0.3 * -4.0, 0.7 * -3.0 + 0.3 * -0.5]), rtol=0, atol=1e-6)
    assert scores[1, 2] == NINF and scores.dtype == torch.float32 and tuple(scores.shape) == (2, 3)
    # w = 0: the attention score alone, even where the CTC score is large; ties keep the first pass' order
    out0, s0 = ctc_beam.combine(hyps, ctc, att, 0.0, 1, EOS)
    assert out0 == [[[5, EOS]], [[EOS]]] and s0[:, 0].tolist() == [-1.0, -1.0]
    tie, st = ctc_beam.combine([[[3], [4]]], torch.tensor([[-1.0, -1.0]]), torch.tensor([[-2.0, -2.0]]), 0.5, 2, EOS)
    assert tie == [[[3, EOS], [4, EOS]]]
    for bad in (dict(weight=1.0), dict(weight=-0.1), dict(n_best=5), dict(n_best=0), dict(att_scores=att[:, :3])):
        with pytest.raises(ValueError):
            ctc_beam.combine(**{**dict(hyps=hyps, ctc_scores=ctc, att_scores=att, weight=w, n_best=2, eos=EOS), **bad})


def test_decode_entry_points_need_the_head_and_sane_widths():
    import oracle as orc
    import transformer.Models as M
    import transformer.Utils as U
    from transformer.Decode import Decode
    from transformer.Loss import CTCAttentionLoss
    p = orc.xavier_init_(orc.make_params(80, 30, 128, 256, 1, 1, 100, 20, dtype=torch.float64), seed=1)
    cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=100, max_target_length=20, num_enc_layer=1, num_dec_layer=1, n_heads=4,
                          d_k=32, d_v=32, d_model=128, d_inner_hid=256, dropout=0.0, vocab_size=30))
    model = M.Transformer(cfg)
    model.load_state_dict({k: v.float() for k, v in p.items()})
    opt = U.AttrDict(dict(beam_size=4, n_best=2, max_steps=10, use_graph=False))
    src = (torch.zeros(2, 12, 80), torch.tensor([12, 9]))
    no_head = Decode(opt, "cpu", model=model.eval())
    for call in (lambda: no_head.ctc_beam(src), lambda: no_head.decode_two_pass(src)):
        with pytest.raises(ValueError, match="CTC head"):
            call()
    dec = Decode(opt, "cpu", model=model, ctc_head=CTCAttentionLoss(128, 30).eval())
    for call in (lambda: dec.ctc_beam(src, beam=17), lambda: dec.ctc_beam(src, n_best=5), lambda: dec.decode_two_pass(src, ctc_weight=1.0),
                 lambda: dec.decode_two_pass(src, beam=0)):
        with pytest.raises(ValueError):
            call()

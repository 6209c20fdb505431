"""-m gpu: st_ctc_beam_search (csrc/st_ctc_beam.hip) against the fp64 reference of tests/_ctc_beam_ref.py, and the decode entry
points built on it (Decode.ctc_beam / score_nbest / decode_two_pass).

The kernel is checked FRAME BY FRAME through its trace (``ref.check_trace``: the beam before a frame is rebuilt from the kernel's own
records, the fp64 candidates of the frame are formed, and membership, uniqueness, values, selection and the normaliser are held to
the bound DERIVED in the reference's docstring) - so a comparison never depends on which of two near-equal candidates fp32 happened
to keep.  Whole hypotheses are compared with the reference only where its selection margin is at least 100 times the accumulated
bound, which the test asserts first.  All five buffers of a launch sit between guard bands and are pre-filled with a bit pattern;
rows that belong to no utterance hold NaN and junk ids.

The kernel keeps the beam's label sequences in LDS and no state that grows with the frame count: it has no chunk or LDS threshold
in T and no largest supported frame count.  Its internal strides are the 64 labels a wave compares or copies per pass - the
200-frame cases over 30 classes grow prefixes through 64 (flat) and 128 (peaked) labels - and the three-frame prefetch
(T = 1, 2, 3)."""
import itertools

import numpy as np
import pytest
import torch

from tests import _ctc_beam_ref as ref
from tests._local import Guarded

pytestmark = pytest.mark.gpu

I32, F32 = torch.int32, torch.float32


def _nv():
    from st_amd import native as nv
    nv.load(build_if_missing=False)
    return nv


def _lsm(x):
    x = x - x.max(-1, keepdims=True)
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


class Case(object):
    """B utterances, utterance b in rows b * T .. b * T + lens[b] - 1 of the packed inputs; every other row poisoned."""

    def __init__(self, lpf, lens, K, blank=0):
        B, T, V = lpf.shape
        self.B, self.T, self.K, self.blank, self.lens, self.lpf = B, T, K, blank, [int(n) for n in lens], lpf
        self.ids = np.full((B * T, K), 0x7ffffff0, dtype=np.int32)
        self.lp = np.full((B * T, K), np.nan, dtype=np.float32)
        self.lpb = np.full((B * T,), np.nan, dtype=np.float32)
        self.per = []
        for b, n in enumerate(self.lens):
            ids, lp, lpb = ref.inputs_of(lpf[b, :n], K, blank) if n else (np.zeros((0, K), np.int32), np.zeros((0, K), np.float32), np.zeros(0, np.float32))
            self.ids[b * T:b * T + n], self.lp[b * T:b * T + n], self.lpb[b * T:b * T + n] = ids, lp, lpb
            self.per.append((ids, lp, lpb))
        self.off = np.arange(B, dtype=np.int32) * T

    def device(self):
        return [torch.from_numpy(a).cuda() for a in (self.ids, self.lp, self.lpb, self.off, np.asarray(self.lens, dtype=np.int32))]


def _launch(case, beam, L_cap, trace=True, dev=None):
    """One st_ctc_beam_search launch into guarded buffers -> dict of numpy arrays, guards checked."""
    nv = _nv()
    B, T = case.B, max(case.T, 1)
    g_tok = Guarded.vec(B * beam * L_cap, I32, "cuda")
    g_len = Guarded.vec(B * beam, I32, "cuda")
    g_sc = Guarded.vec(B * beam, F32, "cuda")
    g_tr = Guarded.vec(B * T * beam * 16, torch.uint8, "cuda", pad=64)
    g_nm = Guarded.vec(B * T, torch.float64, "cuda")
    tokens, lens, score = g_tok.view.view(B, beam, L_cap), g_len.view.view(B, beam), g_sc.view.view(B, beam)
    tr, nm = g_tr.view.view(B, T, beam, 16), g_nm.view.view(B, T)
    ids, lp, lpb, off, length = dev if dev is not None else case.device()
    nv.ctc_beam_search(ids, lp, lpb, off, length, case.blank, tokens, lens, score, trace=tr if trace else None,
                       trace_norm=nm if trace else None)
    torch.cuda.synchronize()
    for gd, what in ((g_tok, "tokens"), (g_len, "lens"), (g_sc, "score"), (g_tr, "trace"), (g_nm, "trace_norm")):
        gd.assert_intact("st_ctc_beam_search: " + what)
    raw = tr.cpu().numpy()
    return dict(tokens=tokens.cpu().numpy(), lens=lens.cpu().numpy(), score=score.cpu().numpy(),
                rec_i=raw.view(np.int32).reshape(B, T, beam, 4), rec_f=raw.view(np.float32).reshape(B, T, beam, 4),
                norms=nm.cpu().numpy())


def _check_utterance(case, out, b, beam, L_cap):
    n = case.lens[b]
    ids, lp, lpb = case.per[b]
    ri, rf = out["rec_i"][b], out["rec_f"][b]
    trace = [[(int(ri[t, s, 0]), int(ri[t, s, 1]), float(rf[t, s, 2]), float(rf[t, s, 3])) for s in range(beam)] for t in range(n)]
    return ref.check_trace(ids, lp, lpb, case.blank, beam, L_cap, trace, out["norms"][b, :n], out["score"][b], out["tokens"][b],
                           out["lens"][b])


def _ragged(T, B, seed):
    rng = np.random.default_rng(seed)
    walk = [T, T - 1, 0, 1]
    return [min(max(walk[b % 8] if b % 8 < 4 else int(rng.integers(0, T + 1)), 0), T) for b in range(B)]


#        T_max beam K   V  scale L_cap
CASES = [(1, 1, 1, 3, 0.1, 255), (2, 2, 3, 3, 5.0, 255), (3, 3, 3, 3, 0.1, 255), (3, 16, 16, 30, 5.0, 2), (7, 8, 8, 30, 5.0, 255),
         (7, 16, 16, 30, 0.1, 3), (63, 3, 3, 3, 0.1, 255), (63, 16, 16, 30, 0.1, 255), (64, 2, 3, 5, 5.0, 4), (64, 16, 4, 5, 0.1, 255),
         (65, 4, 16, 30, 5.0, 255), (65, 8, 8, 30, 0.1, 4), (200, 3, 3, 3, 5.0, 255), (200, 2, 3, 5, 0.1, 255), (200, 1, 1, 30, 5.0, 255),
         (200, 16, 4, 5, 5.0, 255), (200, 4, 16, 30, 0.1, 255), (200, 8, 8, 30, 0.1, 70), (200, 8, 8, 30, 5.0, 255)]


@pytest.mark.parametrize("T,beam,K,V,scale,L_cap", CASES)
def test_every_frame_of_a_ragged_mix_passes_the_frame_local_check(T, beam, K, V, scale, L_cap):
    B = 33
    rng = np.random.default_rng(1000 * T + 16 * beam + K + V)
    case = Case(_lsm(rng.standard_normal((B, T, V)) * scale).astype(np.float32), _ragged(T, B, T + V), K, blank=0 if V != 5 else 2)
    out = _launch(case, beam, L_cap)
    worst, capped = 0.0, 0
    for b in range(B):
        try:
            worst = max(worst, _check_utterance(case, out, b, beam, L_cap)[0])
        except AssertionError as e:
            raise AssertionError("utterance %d (len %d): %s" % (b, case.lens[b], e)) from None
        if case.lens[b] == 0:
            assert out["score"][b, 0] == 0.0 and out["lens"][b, 0] == 0 and (out["score"][b, 1:] == -np.inf).all()
        capped += int((out["lens"][b] == L_cap).any())
        assert (out["lens"][b] <= L_cap).all()
    print("T %d beam %d K %d V %d scale %g: worst error / bound %.3f, utterances at the label capacity %d" % (T, beam, K, V, scale, worst, capped))
    if L_cap < 100 and T >= 7:
        assert capped > 0, "the case is meant to reach the label capacity"
    if (T, V, L_cap) == (200, 30, 255) and beam > 1:      # (flat: about a label every other frame; peaked: nearly one per frame)
        assert out["lens"].max() > (64 if scale < 1 else 128), "the case is meant to grow prefixes through 64 / 128 labels"


MERGE = [(3, 40, 3, 3, 14), (3, 40, 3, 3, 78), (3, 40, 3, 3, 101), (4, 50, 4, 4, 143), (4, 50, 4, 4, 438), (5, 60, 5, 5, 63), (5, 60, 5, 5, 161),
         (3, 60, 8, 3, 33), (3, 60, 8, 3, 107), (5, 40, 6, 4, 557), (5, 40, 6, 4, 690)]


def test_prefixes_recreated_through_their_parent_merge_with_their_children():
    """Pinned inputs (a CPU seed scan of numpy.random.default_rng(seed).standard_normal((T, V)) * 2.0, blank 0) for which the
    reference counts at least one RE-CREATION merge - an extension landing on a beam entry whose recorded parent is another entry -
    and whose selection margin is at least 100 times the accumulated bound: hypotheses and lengths must equal the reference's,
    scores within the accumulated bound (plus the one rounding of the returned f32), no label list twice.  An identity by (parent
    node, token) leaves two entries for one label sequence here and fails."""
    groups = {}
    for V, T, beam, K, seed in MERGE:
        groups.setdefault((V, T, beam, K), []).append(seed)
    events = 0
    for (V, T, beam, K), seeds in groups.items():
        lpf = np.stack([_lsm(np.random.default_rng(s).standard_normal((T, V)) * 2.0).astype(np.float32) for s in seeds])
        case = Case(lpf, [T] * len(seeds), K)
        out = _launch(case, beam, 255)
        for b, seed in enumerate(seeds):
            res = ref.search(*case.per[b], 0, beam, 255)
            assert res.recreations >= 1 and ref.margin_ok(res), (V, T, beam, K, seed, res.recreations, res.margin, res.bound)
            events += res.recreations
            got = [tuple(out["tokens"][b, s, :out["lens"][b, s]].tolist()) for s in range(beam) if out["score"][b, s] > -np.inf]
            assert len(set(got)) == len(got), ("a label list appears twice", V, T, beam, K, seed, got)
            assert got == [h for h, _ in res.hyps], (V, T, beam, K, seed, got, [h for h, _ in res.hyps])
            for s, (_, want) in enumerate(res.hyps):
                tol = res.bound + 2.0 * ref.EPS * abs(want)
                assert abs(float(out["score"][b, s]) - want) <= tol, (seed, s, float(out["score"][b, s]), want, tol)
            _check_utterance(case, out, b, beam, 255)
    print("re-creation merges covered: %d" % events)


def test_tiny_lattices_return_every_label_sequence_with_its_ctc_likelihood():
    """V = 3, T <= 3, beam 16, K = 3: nothing is pruned - every feasible label sequence comes back, its score the fp64 CTC forward
    likelihood of its labels within the accumulated bound."""
    seeds = list(range(24))
    lens = [1 + s % 3 for s in seeds]
    lpf = np.stack([_lsm(np.random.default_rng(100 + s).standard_normal((3, 3)) * 2.0).astype(np.float32) for s in seeds])
    case = Case(lpf, lens, 3)
    out = _launch(case, 16, 255)
    feasible = {n: {tuple(k for i, k in enumerate(path) if k and (i == 0 or path[i - 1] != k)) for path in itertools.product(range(3), repeat=n)}
                for n in (1, 2, 3)}      # the label sequences that n frames can spell: 3, 5 and 9 of them
    for b, n in enumerate(lens):
        _, acc = _check_utterance(case, out, b, 16, 255)
        live = [s for s in range(16) if out["score"][b, s] > -np.inf]
        assert {tuple(out["tokens"][b, s, :out["lens"][b, s]].tolist()) for s in live} == feasible[n] and len(live) == len(feasible[n])
        for s in live:
            labels = out["tokens"][b, s, :out["lens"][b, s]].tolist()
            want = ref.ctc_likelihood(lpf[b, :n].astype(np.float64), labels, 0)
            tol = acc + 2.0 * ref.EPS * max(1.0, abs(want))
            assert abs(float(out["score"][b, s]) - want) <= tol, (b, labels, float(out["score"][b, s]), want, tol)


def _sticky(T, V, seed, period=16):
    """Peaked posteriors of a plausible utterance: blank frames with a label spike every ``period`` frames."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, V))
    x[:, 0] += 5.0
    for t in range(period // 2, T, period):
        x[t, 0] -= 5.0
        x[t, int(rng.integers(1, V))] += 5.0
        if rng.random() < 0.3 and t + 1 < T:                     # the label held for a second frame
            x[t + 1] = x[t] + 0.1 * rng.standard_normal(V)
    return _lsm(x).astype(np.float32)


def test_long_utterances_against_the_loss_and_the_alignment_kernels():
    """T = 2,048 and 4,096 (the kernel has no largest frame count: 4,096 stands for 'larger'), B = 4, beam 8, K = 8, peaked.
    check_trace passes on every frame, and for the best hypothesis h of every utterance:
    * score(h) <= log p_ctc(h) + bound - a pruned sum of alignments cannot exceed the full sum.  Asserted unconditionally, with
      log p_ctc from torch's fp64 CTC loss (bound = the accumulated bound of check_trace + the f32 rounding of the score) and from
      st_ctc_loss_fwd (whose own fp32 error the alignment tests grant 1e-3 |nll|);
    * score(h) >= the st_ctc_align score of h - one path cannot exceed the sum over the kept paths.  Asserted for an utterance
      whose Viterbi path was KEPT: at every frame the class the path emits is among the row's K, and the path's label prefix is in
      the kernel's beam (rebuilt from the trace) with a finite mass on the side the path ends on (blank / label); the test requires
      that this holds for at least one utterance."""
    nv = _nv()
    B, T, V, beam, K, L_cap = 4, 4096, 30, 8, 8, 255
    lens = [2048, 2047, 4096, 1000]
    lpf = np.stack([_sticky(T, V, 7 + b) for b in range(B)])
    case = Case(lpf, lens, K)
    out = _launch(case, beam, L_cap)
    acc = [_check_utterance(case, out, b, beam, L_cap)[1] for b in range(B)]
    best = [out["tokens"][b, 0, :out["lens"][b, 0]].tolist() for b in range(B)]
    assert all(len(h) > 40 for h in best)
    L = max(len(h) for h in best)
    cls = torch.zeros(B, L, dtype=torch.int64)
    for b, h in enumerate(best):
        cls[b, :len(h)] = torch.tensor(h)
    lp_d = torch.from_numpy(lpf).cuda()
    il, tl = torch.tensor(lens, dtype=I32).cuda(), torch.tensor([len(h) for h in best], dtype=I32).cuda()
    ws = torch.empty(nv.ctc_loss_ws_bytes(B, T, L), dtype=torch.uint8, device="cuda")
    nll = nv.ctc_loss_fwd(lp_d, cls.cuda(), il, tl, ws, torch.empty(B, dtype=F32, device="cuda")).cpu().numpy()
    nll64 = torch.nn.functional.ctc_loss(torch.from_numpy(lpf).double().transpose(0, 1), cls, torch.tensor(lens), tl.cpu().long(),
                                         blank=0, reduction="none").numpy()
    ws2 = torch.empty(nv.ctc_align_ws_bytes(B, T, L), dtype=torch.uint8, device="cuda")
    path = torch.empty(B, T, dtype=I32, device="cuda")
    spans = torch.empty(B, L, 2, dtype=I32, device="cuda")
    vit = torch.empty(B, dtype=F32, device="cuda")
    nv.ctc_align(lp_d, cls.cuda(), il, tl, ws2, path, spans, vit)
    path, vit = path.cpu().numpy(), vit.cpu().numpy()
    kept_paths = 0
    for b in range(B):
        sc = float(out["score"][b, 0])
        tol = acc[b] + 2.0 * ref.EPS * abs(sc)
        print("utterance %d (T %d, %d labels): score %.4f, -nll fp64 %.4f, -nll st_ctc_loss_fwd %.4f, Viterbi %.4f, bound %.2e"
              % (b, lens[b], len(best[b]), sc, -nll64[b], -nll[b], vit[b], tol))
        assert sc <= -nll64[b] + tol, (b, sc, -nll64[b], tol)
        assert sc <= -nll[b] + tol + 1e-3 * abs(nll[b]), (b, sc, -nll[b])
        # was the Viterbi path kept?  rebuild the beam of every frame from the trace and follow the path's prefix
        ri, rf = out["rec_i"][b], out["rec_f"][b]
        entries, kept, n_lab = [()], True, 0
        for t in range(lens[b]):
            entries = [entries[int(ri[t, s, 0])] + ((int(ri[t, s, 1]),) if ri[t, s, 1] >= 0 else ()) for s in range(beam) if ri[t, s, 0] >= 0]
            pos = int(path[b, t])
            n_lab = max(n_lab, pos + 1)
            want = tuple(best[b][:n_lab])
            if pos >= 0 and best[b][pos] not in case.per[b][0][t]:          # (the path's class must be among the row's K)
                kept = False
                break
            if want not in entries or not rf[t, entries.index(want), 2 if pos < 0 else 3] > -np.inf:
                kept = False
                break
        if kept:
            kept_paths += 1
            assert sc >= float(vit[b]) - tol - 2.0 * ref.EPS * abs(float(vit[b])), (b, sc, float(vit[b]), tol)
    assert kept_paths >= 1, "no utterance kept the Viterbi path of its best hypothesis: the lower bound was never asserted"


def test_two_launches_are_bit_equal_and_a_captured_launch_follows_refilled_buffers():
    nv = _nv()
    B, T, V, beam, K, L_cap = 8, 120, 30, 8, 8, 40
    rng = np.random.default_rng(5)
    c1 = Case(_lsm(rng.standard_normal((B, T, V)) * 2.0).astype(np.float32), _ragged(T, B, 1), K)
    c2 = Case(_lsm(rng.standard_normal((B, T, V)) * 0.5).astype(np.float32), list(reversed(_ragged(T, B, 2))), K)
    e1, again, e2 = _launch(c1, beam, L_cap), _launch(c1, beam, L_cap), _launch(c2, beam, L_cap, trace=False)
    for k in ("tokens", "lens", "score", "norms"):
        assert np.array_equal(e1[k].view(np.int32), again[k].view(np.int32)), k + " differs between two launches"
    for b in range(B):                     # (rows of the trace past a length are never written: compare the frames that are)
        n = c1.lens[b]
        assert np.array_equal(e1["rec_i"][b, :n], again["rec_i"][b, :n]), "the trace differs between two launches"
    assert not np.array_equal(e1["tokens"], e2["tokens"])
    bufs = c1.device()
    tokens = torch.zeros(B, beam, L_cap, dtype=I32, device="cuda")
    lens = torch.zeros(B, beam, dtype=I32, device="cuda")
    score = torch.zeros(B, beam, dtype=F32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nv.ctc_beam_search(*bufs, 0, tokens, lens, score)
    for want, case in ((e1, c1), (e2, c2), (e1, c1)):
        for dst, src in zip(bufs, case.device()):
            dst.copy_(src)
        tokens.fill_(77)
        lens.fill_(77)
        score.fill_(77.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(tokens.cpu().numpy(), want["tokens"]) and np.array_equal(lens.cpu().numpy(), want["lens"])
        assert np.array_equal(score.cpu().numpy().view(np.int32), want["score"].view(np.int32))


# ---- the decode entry points on a small joint model ---------------------------------------------------------------------------------
_MODEL = {}


def _joint_model():
    """The 2+2-layer d_model-256 joint model of test_ctc_align_gpu.py (V = 30, head weights x 8), built once."""
    if not _MODEL:
        import oracle as orc
        import transformer.Models as M
        import transformer.Utils as U
        from transformer.Loss import CTCAttentionLoss
        p = orc.xavier_init_(orc.make_params(80, 30, 256, 512, 2, 2, 100, 20, dtype=torch.float64), seed=3)
        cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=100, max_target_length=20, num_enc_layer=2, num_dec_layer=2, n_heads=4,
                              d_k=64, d_v=64, d_model=256, d_inner_hid=512, dropout=0.0, vocab_size=30))
        model = M.Transformer(cfg)
        model.load_state_dict({k: v.float() for k, v in p.items()})
        torch.manual_seed(1)
        head = CTCAttentionLoss(256, 30)
        with torch.no_grad():
            head.ctc_proj.weight.mul_(8.0)
        batch = orc.synthetic_batch(5, 80, 10, 80, 30, seed=2, t_min=30, l_min=5)
        _MODEL.update(p=p, model=model.eval().cuda(), head=head.cuda(), src=(batch["x"], batch["in_len"]))
    return _MODEL


def _decoder(**opt):
    import transformer.Utils as U
    from transformer.Decode import Decode
    m = _joint_model()
    return Decode(U.AttrDict(dict(dict(beam_size=4, n_best=1, max_steps=16, ctc_weight=0.3), **opt)), "cuda", model=m["model"], ctc_head=m["head"])


def _head_lp(dec, src):
    """The head's log-probabilities as [B, T, V] f32 on the device (rows past a length: 0) and the lengths."""
    from st_amd import ctc_decode
    from st_amd.arena import arena_of
    in_len = src[1].tolist()
    with arena_of(dec.model).scope():
        enc, in_rows = dec._encode(src)
        lp = torch.log_softmax(ctc_decode.head_logits(dec.ctc_head, enc)[:, :30].double(), -1).float()
    out = torch.zeros(len(in_len), max(in_len), 30, dtype=F32, device="cuda")
    o = 0
    for b, n in enumerate(in_len):
        out[b, :n] = lp[o:o + n]
        o += n
    return out, in_len


def _nll(lp, in_len, lists):
    nv = _nv()
    B, T, _ = lp.shape
    L = max(1, max(len(h) for h in lists))
    cls = torch.zeros(B, L, dtype=torch.int64)
    for b, h in enumerate(lists):
        cls[b, :len(h)] = torch.tensor(h, dtype=torch.int64)
    ws = torch.empty(nv.ctc_loss_ws_bytes(B, T, L), dtype=torch.uint8, device="cuda")
    return nv.ctc_loss_fwd(lp, cls.cuda(), torch.tensor(in_len, dtype=I32).cuda(), torch.tensor([len(h) for h in lists], dtype=I32).cuda(),
                           ws, torch.empty(B, dtype=F32, device="cuda")).cpu().numpy()


def test_ctc_beam_of_width_one_is_no_worse_than_ctc_greedy():
    """Beam 1 over the 16 best classes per row (the kernel's widest pre-beam; the head is peaked, the frame arg-max of ctc_greedy is
    always among them): the label list scores at least what ctc_greedy's list scores under st_ctc_loss_fwd (1e-3 |nll| for that
    kernel's fp32, as in test_ctc_align_gpu.py)."""
    dec = _decoder(ctc_beam_pre_beam=16)
    src = _joint_model()["src"]
    hyps, scores = dec.ctc_beam(src, beam=1, n_best=1)
    greedy = dec.ctc_greedy(src)
    assert len(hyps) == 5 and all(len(h) == 1 for h in hyps) and all(s.shape == (1,) and s.is_cuda for s in scores)
    lp, in_len = _head_lp(dec, src)
    keep = [b for b in range(5) if max(len(hyps[b][0]), len(greedy[b])) <= 255]
    ours = _nll(lp, in_len, [hyps[b][0] if b in keep else [] for b in range(5)])
    theirs = _nll(lp, in_len, [greedy[b] if b in keep else [] for b in range(5)])
    assert keep
    for b in keep:
        print("utterance %d: beam-1 %d labels, log p %.4f (search score %.4f); greedy %d labels, log p %.4f"
              % (b, len(hyps[b][0]), -ours[b], float(scores[b][0]), len(greedy[b]), -theirs[b]))
        assert all(0 < k < 30 for k in hyps[b][0])
        assert -ours[b] >= -theirs[b] - 1e-3 * abs(theirs[b]), (b, -ours[b], -theirs[b])
        assert float(scores[b][0]) <= -ours[b] + 1e-3 * abs(ours[b])             # (a pruned sum)


def test_score_nbest_agrees_with_score_hypotheses_and_fp64():
    """Column j of score_nbest against score_hypotheses on the same lists (N = 1 rows per utterance) and against the fp64 oracle,
    by the route and with the bound of test_joint_decode_gpu.py::test_score_hypotheses_joint_small_model_vs_fp64."""
    from oracle import beam_oracle as bo
    m = _joint_model()
    dec = _decoder()
    x, in_len = m["src"]
    g = torch.Generator().manual_seed(3)
    nbest = [[torch.randint(4, 30, (int(k),), generator=g).tolist() for k in ks] for ks in ((3, 5, 1), (5, 2), (6, 6, 4), (8,), (4, 0, 7))]
    nbest[2][1][2] = nbest[2][1][1]                             # a repeated label
    got = dec.score_nbest((x, in_len), nbest)
    assert got.dtype == F32 and tuple(got.shape) == (5, 3)
    got = got.double().cpu()
    for j in range(3):
        have = [b for b in range(5) if j < len(nbest[b])]
        lists = [(nbest[b][j] if b in have else []) + [bo.EOS] for b in range(5)]
        one = dec.score_hypotheses((x, in_len), lists).double().cpu()
        for b in range(5):
            if b not in have:
                assert got[b, j] == float("-inf")
                continue
            truth = bo.score_hypothesis(m["p"], x[b:b + 1].double(), in_len[b:b + 1], 4, lists[b])
            bound = max(0.16, 5e-2 * abs(truth))
            print("utterance %d list %d: score_nbest %.4f, score_hypotheses %.4f, fp64 %.4f" % (b, j, float(got[b, j]), float(one[b]), truth))
            assert abs(float(got[b, j]) - truth) <= bound, (b, j, float(got[b, j]), truth)
            assert abs(float(got[b, j]) - float(one[b])) <= bound, (b, j, float(got[b, j]), float(one[b]))
    with pytest.raises(ValueError):
        dec.score_nbest((x, in_len), [[list(range(4, 20))]] * 5)            # 16 labels + EOS exceed max_steps = 16
    with pytest.raises(ValueError):
        dec.score_nbest((x, in_len), nbest[:4])


def test_decode_two_pass_combines_both_passes_and_feeds_align():
    import transformer.Constants as Constants
    from st_amd import ctc_beam
    from st_amd.arena import arena_of
    m = _joint_model()
    src = m["src"]
    w, beam = 0.3, 4
    dec = _decoder(n_best=3)
    hyps, scores = dec.decode_two_pass(src, beam=beam)
    assert len(hyps) == 5 and all(len(h) == 3 for h in hyps)
    # the two passes on their own: the first pass with the label capacity decode_two_pass uses (max_steps - 1)
    with arena_of(dec.model).scope():
        enc, in_rows = dec._encode(src)
        first, ctc = ctc_beam.search_rows(m["head"], enc, in_rows, beam, max_len=15).lists()
    att = dec.score_nbest(src, first).double().cpu()
    for b in range(5):
        s = scores[b].double().cpu()
        assert s.shape == (3,) and all(s[i] >= s[i + 1] for i in range(2)), (b, s)
        want = {}
        for j, h in enumerate(first[b]):
            if ctc[b, j] > float("-inf"):
                want[tuple(h)] = (1.0 - w) * float(att[b, j]) + w * float(ctc[b, j])
        ranked = sorted(want.values(), reverse=True)
        for i, h in enumerate(hyps[b]):
            if s[i] == float("-inf"):
                assert h == [] and i >= len(want)
                continue
            assert h[-1] == Constants.EOS and Constants.EOS not in h[:-1] and len(h) <= 16
            exp = want[tuple(h[:-1])]
            assert abs(float(s[i]) - exp) <= 1e-5 * max(1.0, abs(exp)), (b, i, float(s[i]), exp)
            assert abs(float(s[i]) - ranked[i]) <= 1e-5 * max(1.0, abs(exp)), (b, i, float(s[i]), ranked[i])
    assert any(len(h[0]) > 2 for h in hyps)
    # the default weight is opt.ctc_weight; another weight ranks by its own combination
    h0, s0 = dec.decode_two_pass(src, ctc_weight=0.0, beam=beam, n_best=1)
    for b in range(5):
        j = int(torch.argmax(torch.where(torch.isfinite(ctc[b].double()), att[b], torch.full_like(att[b], float("-inf")))))
        assert abs(float(s0[b][0]) - float(att[b, j])) <= 1e-5 * max(1.0, abs(float(att[b, j])))
    out = dec.align(src, [h[0] for h in hyps])
    assert len(out) == 5
    for b, (items, sc) in enumerate(out):
        if sc > float("-inf"):
            assert [it[0] for it in items] == hyps[b][0][:-1]
    assert any(sc > float("-inf") and items for items, sc in out)

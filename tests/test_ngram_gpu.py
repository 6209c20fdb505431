"""-m gpu: the n-gram language model on the device (csrc/st_ngram.hip, st_amd/ngram.py, transformer/Decode.py with ``lm=``):
st_ngram_score / st_ngram_score_seq BIT-equal to the float32 emulation of tests/_emul_ngram.py, the in-place fusion against
fp64, st_ngram_advance against the NumPy permutation, five chained search steps against the torch formulation of the joint
advance, shallow fusion on the small decode model against fp64 truth (joint and LM-only routes, graph replay, the veto), two-pass
rescoring with the LM term, and one run at the config-5 shape."""
import math

import numpy as np
import pytest
import torch

from st_amd import ngram
from st_amd.ngram import NGramLM
from tests import _emul_ngram as emul
from tests._local import Guarded

pytestmark = pytest.mark.gpu

BOS, EOS, OOV_TOK = 2, 3, 1
F32, I32 = torch.float32, torch.int32


def _nv():
    from st_amd import native as nv
    nv.load(build_if_missing=False)
    return nv


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- models with chosen fan-outs -----------------------------------------------------------------------------------------------------
def build_model(order, V, seed, oov_logp=ngram.OOV_LOGP):
    """-> (lm, special): unigrams for every token but OOV_TOK; the reverse-trie nodes of the tokens 4, 5, .. get 0, 1, 2, 63, 64, 65
    and V children (the fan-outs that fit V), i.e. that many bigrams (x, c); deeper levels hang off random stored n-grams, one
    node per level with 65 children where V allows, and two n-grams whose suffix is NOT stored (completion has work to do).
    ``special``: {c: sorted x of its children}."""
    rng = np.random.default_rng(seed)

    def val(m):
        return (-float(rng.random()) * 8.0 - 0.01, -float(rng.random()) * 2.0 if m < order else 0.0)

    table = {(v,): val(1) for v in range(V) if v != OOV_TOK}
    special = {}
    for i, k in enumerate(f for f in (0, 1, 2, 63, 64, 65, V) if f <= V):
        c = 4 + i
        xs = np.arange(V) if k == V else np.sort(rng.choice(np.setdiff1d(np.arange(V), [OOV_TOK]), size=k, replace=False))
        special[c] = [int(x) for x in xs]
        for x in xs:
            table[(int(x), c)] = val(2)
    for c in rng.choice(np.arange(12, V), size=min(V - 12, 40), replace=False):
        for x in rng.choice(V, size=int(rng.integers(1, 4)), replace=False):
            table[(int(x), int(c))] = val(2)
    for d in range(3, order + 1):
        prev = [g for g in table if len(g) == d - 1]
        for gi in rng.choice(len(prev), size=min(len(prev), 60), replace=False):
            for y in rng.choice(V, size=int(rng.integers(1, 4)), replace=False):
                table[(int(y),) + prev[gi]] = val(d)
        if V >= 80:
            g = prev[int(rng.integers(len(prev)))]
            for y in rng.choice(V, size=65, replace=False):
                table[(int(y),) + g] = val(d)
    if order >= 3:                                          # suffix (20, 21) / (22, 23) is not stored
        table.pop((20, 21), None), table.pop((22, 23), None)
        table[(19, 20, 21)] = val(3)
        table[(OOV_TOK, 22, 23)] = val(3)
    return NGramLM.from_table(table, order, V, oov_logp=oov_logp), special


def build_case(lm, special, B, beam, K, seed):
    """Histories and candidates of n = B x beam rows: histories taken from stored n-grams (deep walks), from the first / last
    child of the special nodes and the tokens below, between and above their children, shortened by -1 entries, with OOV tokens,
    frozen rows (most recent token EOS) and one done utterance; candidates: the special tokens, the tokens that end the stored
    n-gram of the row, OOV_TOK, -1, V and random ones."""
    rng = np.random.default_rng(seed)
    V, H, n = lm.V, lm.order - 1, B * beam
    stored = [g for g in lm.table if len(g) >= 2]
    h1_pool = []
    for c, xs in special.items():
        if not xs:
            continue
        picks = [xs[0], xs[-1], xs[0] - 1, xs[-1] + 1] + [x + 1 for x in xs[:-1] if x + 1 not in xs][:1]
        h1_pool += [(p, c) for p in picks if 0 <= p < V]
    order_of = rng.permutation(len(h1_pool))
    hist = np.full((n, H), -1, dtype=np.int32)
    cand = rng.integers(0, V, (n, K)).astype(np.int32)
    pool = list(special) + [OOV_TOK, -1, V, EOS]
    for i in range(n):
        for j in range(K):
            if rng.random() < 0.5:
                cand[i, j] = pool[(i * K + j) % len(pool)]
    for i in range(n):
        kind = i % 4
        if kind in (0, 1):                                  # a stored n-gram: its context as the history, its last token a candidate
            g = stored[int(rng.integers(len(stored)))]
            ctx = list(g[:-1])[-H:]
            hist[i, H - len(ctx):] = ctx
            if kind == 1 and H > len(ctx):                  # older tokens that no stored n-gram continues
                hist[i, :H - len(ctx)] = rng.integers(0, V, H - len(ctx))
            cand[i, int(rng.integers(K))] = g[-1]
        elif kind == 2:                                     # h_1 against the children of a special node
            p, c = h1_pool[order_of[(i // 4) % len(h1_pool)]]
            hist[i] = rng.integers(0, V, H)
            hist[i, -1] = p
            cand[i, int(rng.integers(K))] = c
        else:                                               # short, broken and OOV histories; candidates -1, V and the OOV token
            hist[i] = rng.integers(0, V, H)
            if H > 1:
                hist[i, int(rng.integers(H - 1))] = -1      # a -1 inside: the history ends there
            if i % 8 == 3:
                hist[i, -1] = OOV_TOK
            for j in range(min(K, 3)):
                cand[i, j] = (-1, V, OOV_TOK)[(i // 4 + j) % 3]
    frozen = np.zeros(n, dtype=bool)
    frozen[rng.choice(n, size=max(1, n // 6), replace=False)] = True
    frozen[0] = True                                        # (utterance 0 is never the done one)
    hist[frozen, -1] = EOS
    if n > 2:
        hist[2] = -1                                        # no history at all
    done = np.zeros(B, dtype=bool)
    if B > 1:
        done[1] = True
    return hist, cand, done


_MODELS = {}


def _model_on_gpu(order, V):
    if (order, V) not in _MODELS:
        lm, special = build_model(order, V, 17 * order + V)
        _MODELS[(order, V)] = (lm.to("cuda"), special)
    return _MODELS[(order, V)]


GRID = [(2, 30, 7, 1, 16), (3, 30, 5, 8, 1), (5, 80, 3, 4, 64), (4, 5120, 5, 1, 10), (3, 4337, 3, 11, 15)]     # order, V, B, beam, K


@pytest.mark.parametrize("order,V,B,beam,K", GRID)
def test_ngram_score_raw_is_bit_equal_to_the_emulation(order, V, B, beam, K):
    """(order, V, n = B x beam, K) = (2, 30, 7, 16), (3, 30, 40, 1), (5, 80, 12, 64), (4, 5120, 5, 10), (3, 4337, 33, 15)."""
    nv = _nv()
    lm, special = _model_on_gpu(order, V)
    hist, cand, done = build_case(lm, special, B, beam, K, 1000 * order + V + K)
    n = B * beam
    want = emul.score_rows(lm.trie, hist, cand, EOS, done, beam)
    out = Guarded(n, K, F32, "cuda", pad_rows=8, pad_cols=(0, 0))
    nv.ngram_score(lm.trie, torch.from_numpy(hist).cuda(), torch.from_numpy(cand).cuda(), torch.from_numpy(done).cuda(), EOS, lm_out=out.view)
    torch.cuda.synchronize()
    out.assert_intact("st_ngram_score: lm_out")
    skipped = np.repeat(done, beam)
    out.assert_untouched(skipped, "st_ngram_score: rows of a done utterance")
    got = out.view.cpu().numpy()
    live = ~skipped
    assert not np.isnan(got[live]).any() and np.isnan(want[skipped]).all()
    bad = np.argwhere(_bits(got[live]) != _bits(want[live]))
    assert bad.size == 0, (bad[:5], got[live][tuple(bad[0])], want[live][tuple(bad[0])])
    # the cases the grid promises, counted on the reference side
    assert np.isneginf(want[live]).any() and (want[live] == 0.0).any()
    assert (hist[:, -1] == EOS).any() and (cand == OOV_TOK).any() and (cand == -1).any() and (cand == V).any()


@pytest.mark.parametrize("oov", [ngram.OOV_LOGP, float("-inf")])
def test_ngram_score_in_place_fusion(oov):
    """lp += scale lm + bias against fp64 within 2^-23 (|lp| + |scale lm| + |bias|); -inf stays -inf (an -inf lp, a candidate out of
    range, an OOV token under oov_logp = -inf), never NaN; frozen rows and done utterances keep their lp bit for bit."""
    nv = _nv()
    order, V, B, beam, K = 4, 80, 4, 5, 12
    base, special = build_model(order, V, 5, oov_logp=oov)
    lm = base.to("cuda")
    hist, cand, done = build_case(lm, special, B, beam, K, 77)
    n = B * beam
    rng = np.random.default_rng(3)
    lp0 = (-rng.random((n, K)) * 9.0).astype(np.float32)
    lp0[rng.random((n, K)) < 0.1] = -np.inf
    scale, bias = np.float32(0.7), np.float32(0.3)
    raw = emul.score_rows(lm.trie, hist, cand, EOS, done, beam)
    lp = Guarded(n, K, F32, "cuda", pad_rows=8, pad_cols=(0, 0))
    lp.view.copy_(torch.from_numpy(lp0))
    nv.ngram_score(lm.trie, torch.from_numpy(hist).cuda(), torch.from_numpy(cand).cuda(), torch.from_numpy(done).cuda(), EOS,
                   float(scale), float(bias), lp=lp.view)
    torch.cuda.synchronize()
    lp.assert_intact("st_ngram_score: lp")
    got = lp.view.cpu().numpy()
    assert not np.isnan(got).any()
    keep = np.repeat(done, beam) | (hist[:, -1] == EOS)
    assert keep.any() and np.array_equal(_bits(got[keep]), _bits(lp0[keep]))
    n_inf = 0
    for i in np.nonzero(~keep)[0]:
        for j in range(K):
            lm64, l64 = float(raw[i, j]), float(lp0[i, j])
            if math.isinf(lm64) or math.isinf(l64):
                assert got[i, j] == -np.inf, (i, j, got[i, j])
                n_inf += 1
                continue
            want = l64 + float(scale) * lm64 + float(bias)
            bound = 2.0 ** -23 * (abs(l64) + abs(float(scale) * lm64) + abs(float(bias)))
            assert abs(float(got[i, j]) - want) <= bound, (i, j, float(got[i, j]), want, bound)
    assert n_inf > 0
    if math.isinf(oov):
        assert any(np.isneginf(raw[i, j]) and cand[i, j] == OOV_TOK for i in np.nonzero(~keep)[0] for j in range(K))


def advance_case(B, beam, H, seed):
    rng = np.random.default_rng(seed)
    n = B * beam
    hist = rng.integers(4, 30, (n, H)).astype(np.int32)
    hist[rng.random((n, H)) < 0.1] = -1
    order = np.zeros(n, dtype=np.int64)
    for b in range(B):
        base = b * beam
        if b % 3 == 0:
            order[base:base + beam] = base + (np.arange(beam) + 1) % beam          # a cycle: every parent is overwritten
        elif b % 3 == 1:
            order[base:base + beam] = base + np.arange(beam) // 2                 # two children per parent
        else:
            order[base:base + beam] = base + rng.integers(0, beam, beam)
    frozen = rng.random(n) < 0.25
    frozen[0] = B * beam > 1 and beam > 1
    hist[frozen, -1] = EOS
    tokens = rng.integers(3, 30, n).astype(np.int64)
    done = np.zeros(B, dtype=bool)
    if B > 1:
        done[B - 1] = True
    return hist, order, tokens, done


@pytest.mark.parametrize("B,beam,H", [(1, 1, 1), (5, 4, 2), (3, 16, 4)])
def test_ngram_advance_equals_the_numpy_permutation(B, beam, H):
    nv = _nv()
    hist, order, tokens, done = advance_case(B, beam, H, 10 * B + beam + H)
    want = emul.advance(hist, order, tokens, EOS, beam, done)
    if B > 1:
        assert np.array_equal(want[-beam:], hist[-beam:]) and (hist[order[~np.repeat(done, beam)], -1] == EOS).any()
    gd = Guarded(B * beam, H, I32, "cuda", pad_rows=8, pad_cols=(0, 0))
    gd.view.copy_(torch.from_numpy(hist))
    nv.ngram_advance(gd.view, torch.from_numpy(order).cuda(), torch.from_numpy(tokens).cuda(), torch.from_numpy(done).cuda(), EOS, beam)
    torch.cuda.synchronize()
    gd.assert_intact("st_ngram_advance: hist")
    assert np.array_equal(gd.view.cpu().numpy(), want)


def test_ngram_score_seq_is_bit_equal_to_the_emulation():
    nv = _nv()
    M, L = 7, 9
    for order, V in ((3, 30), (5, 80)):
        lm, special = _model_on_gpu(order, V)
        rng = np.random.default_rng(order)
        lens = np.array([1, L, 3, 5, L, 2, 7], dtype=np.int32)
        tokens = rng.integers(3, V, (M, L)).astype(np.int32)
        stored = [g for g in lm.table if len(g) == order]
        for m in (1, 4):                                   # stored n-grams inside the full-length lists: deep walks
            g = stored[int(rng.integers(len(stored)))]
            tokens[m, 2:2 + order] = g
        tokens[3, 1] = OOV_TOK
        tokens[6, 3] = V                                   # outside the vocabulary: -inf there, and the later histories end at it
        for m in range(M):
            tokens[m, lens[m]:] = V + 7                    # never read
        want = emul.score_seq(lm.trie, tokens, lens, BOS)
        out = Guarded(M, L, F32, "cuda", pad_rows=8, pad_cols=(0, 0))
        nv.ngram_score_seq(lm.trie, torch.from_numpy(tokens).cuda(), torch.from_numpy(lens).cuda(), BOS, out.view)
        torch.cuda.synchronize()
        out.assert_intact("st_ngram_score_seq: out")
        got = out.view.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (order, got, want)
        assert want[6, 3] == -np.inf and all((want[m, lens[m]:] == 0).all() for m in range(M)) and (want[1] < 0).all()


# ---- five chained steps: pre-beam -> score -> st_beam_advance_joint -> advance ----------------------------------------------------------------
def chain_reference(st, hist, ids, lp, delta, lm, scale, bias, w, beam, K, t):
    """One step of the torch side: the existing joint formulation (tests/test_joint_decode_gpu.py::_joint_torch) over
    lp + scale lm + bias.  -> (state after, histories after, the smallest gap at a selection boundary relative to its tolerance)."""
    from tests.test_joint_decode_gpu import _joint_torch
    B = st["scores"].shape[0]
    done = st["done"].numpy()
    raw = emul.score_rows(lm.trie, hist, ids.numpy(), EOS, done, beam)
    raw = np.where(np.isnan(raw), 0.0, raw)
    frozen = hist[:, -1] == EOS
    add = np.where(frozen[:, None], 0.0, np.float64(np.float32(scale)) * raw.astype(np.float64) + np.float64(np.float32(bias)))
    fused = lp.double() + torch.from_numpy(add)
    want = _joint_torch(st, ids, fused, delta.double(), w, beam, K, EOS, t)
    margin = float("inf")
    for b in range(B):
        if done[b]:
            continue
        rows = slice(b * beam, (b + 1) * beam)
        val = (st["scores"][b].double().unsqueeze(1) + (1 - w) * fused[rows] + (w * delta[rows].double() if w > 0 else 0.0)).reshape(-1)
        top = torch.sort(val, descending=True)[0][:beam + 1]
        for a, c in zip(top[:-1].tolist(), top[1:].tolist()):
            if math.isinf(a) or math.isinf(c):
                continue
            margin = min(margin, (a - c) / (1e-5 + 1e-6 * max(abs(a), abs(c))))
    hist2 = emul.advance(hist, want["order"].numpy(), want["tokens"].numpy(), EOS, beam, want["done"].numpy())
    return want, hist2, margin


def chain_state(B, beam, S):
    n = B * beam
    sc = torch.full((B, beam), float("-inf"))
    sc[:, 0] = 0.0
    # (the CTC-state entries only feed _joint_torch's bookkeeping: this chain moves no CTC state)
    return dict(scores=sc, tokens=torch.full((n,), BOS, dtype=torch.long), done=torch.zeros(B, dtype=torch.bool),
                lengths=torch.zeros(B, dtype=torch.long), hist=torch.zeros(S, B, beam), back=torch.zeros(S, B, beam, dtype=torch.long),
                toks=torch.zeros(S, B, beam, dtype=torch.long), order=torch.zeros(n, dtype=torch.long),
                anc=torch.arange(n, dtype=torch.int32).unsqueeze(1).repeat(1, S).contiguous(),
                gam=torch.zeros(n, 2, 2), psi=torch.zeros(n), last=torch.zeros(n, dtype=torch.int32), frozen=torch.zeros(n, dtype=torch.bool))


def chain_logits(V, n, t, g):
    ld = (V + 7) // 8 * 8
    logits = torch.full((n, ld), -1e30)
    logits[:, :V] = torch.randn(n, V, generator=g) * 3
    logits[:, :3] = -30.0                                  # PAD / UNK / BOS are never proposed
    if t == 1:
        logits[4, 7] = 30.0                                # utterance 1: slot 0 goes on with token 7, slot 1 emits EOS below
        logits[5, EOS] = 6.5                               # the top -> a frozen hypothesis in a live utterance
    if t >= 3:
        logits[0, EOS] = 30.0                              # utterance 0: the top emits EOS -> done
    return logits


@pytest.mark.parametrize("w", [0.3, 0.0])
def test_five_chained_steps_match_the_torch_formulation(w):
    nv = _nv()
    B, beam, K, V, S, order = 3, 4, 6, 30, 6, 3
    lam, beta = 0.5, 0.2
    scale, bias = lam / (1 - w), beta / (1 - w)
    rng = np.random.default_rng(4)
    lists = [[int(k) for k in rng.integers(4, V, rng.integers(3, 9))] for _ in range(40)]
    lm = NGramLM.estimate(lists, order, V).to("cuda")
    n = B * beam
    g = torch.Generator().manual_seed(11)
    st = chain_state(B, beam, S)
    dev = {k: v.cuda() for k, v in st.items()}
    hist = ngram.initial_history(n, order, "cuda")
    assert hist.cpu().tolist() == [[-1, BOS]] * n
    step = torch.zeros(1, dtype=torch.long, device="cuda")
    ticket = torch.zeros(1, dtype=torch.long, device="cuda")
    ids = torch.empty(n, K, dtype=I32, device="cuda")
    lp = torch.empty(n, K, device="cuda")
    seen_frozen = False
    for t in range(S - 1):
        for attempt in range(4):
            logits = chain_logits(V, n, t, g)
            nv.beam_pre_beam(logits.cuda(), V, ids, lp)
            delta = -torch.rand(n, K, generator=g) * 3
            delta[torch.rand(n, K, generator=g) < 0.1] = float("-inf")
            full = dict(st, cand_gam=torch.zeros(n, K, 2, 2), cand_psi=torch.zeros(n, K))
            hist_h = hist.cpu().numpy()
            want, hist_want, margin = chain_reference(full, hist_h, ids.cpu(), lp.cpu(), delta if w > 0 else torch.zeros_like(delta), lm,
                                                      scale, bias, w, beam, K, t)
            if margin > 4.0:                               # every selection boundary is wider than 4x the comparison's tolerance
                break
        assert margin > 4.0, "no well-separated draw in 1 + 3 attempts"
        assert torch.equal(ids.cpu().long(), torch.log_softmax(logits[:, :V].double(), -1).topk(K, -1)[1])
        seen_frozen = seen_frozen or bool(((hist_h[:, -1] == EOS) & ~np.repeat(st["done"].numpy(), beam)).any())
        nv.ngram_score(lm.trie, hist, ids, dev["done"], EOS, scale, bias, lp=lp)
        nv.beam_advance_joint(ids, lp, delta.cuda(), w, beam, step, EOS, dev["scores"], dev["tokens"], dev["done"], dev["lengths"],
                              dev["hist"], dev["back"], dev["toks"], dev["order"], anc=dev["anc"], advance_step=True, ticket=ticket)
        nv.ngram_advance(hist, dev["order"], dev["tokens"], dev["done"], EOS, beam)
        assert int(step) == t + 1
        for k in ("back", "toks", "order", "tokens", "lengths", "done", "anc"):
            assert torch.equal(dev[k].cpu(), want[k].to(dev[k].dtype)), (t, k)
        assert np.array_equal(hist.cpu().numpy(), hist_want), t
        for k in ("scores", "hist"):
            a, b = dev[k].cpu(), want[k].float()
            fin = torch.isfinite(b)
            assert torch.equal(torch.isfinite(a), fin) and torch.allclose(a[fin], b[fin], atol=1e-5, rtol=1e-6), (t, k)
        st = {k: dev[k].cpu() for k in st}
    assert seen_frozen and bool(st["done"][0]) and not bool(st["done"].all())


# ---- search on the small decode model -------------------------------------------------------------------------------------------------
_SMALL = {}


def _small():
    """The small decode model, the peaky head and the synthetic batch of tests/test_joint_decode_gpu.py, an order-3 model
    estimated from the batch's targets, and the LM-less joint result - made once."""
    if not _SMALL:
        import oracle as orc
        from tests.test_joint_decode_gpu import _ctc_lp64, _head
        from tests.test_joint_decode_gpu import _small as small_model
        p, model = small_model("cuda")
        head = _head(30, 128, 8.0, 1, "cuda")
        batch = orc.synthetic_batch(5, 80, 10, 80, 30, seed=2, t_min=30, l_min=5)
        x, in_len = batch["x"], batch["in_len"]
        lists = [batch["tokens"][b, :int(batch["tgt_len"][b])].tolist() for b in range(5)]
        _SMALL.update(p=p, model=model, head=head, x=x, in_len=in_len, lists=lists, lm=NGramLM.estimate(lists, 3, 30).to("cuda"),
                      ctc_lp=_ctc_lp64(p, head, x.double(), in_len, 4))
    return _SMALL


def _decode(m, head=True, lm=None, use_graph=None, **opt):
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    o = dict(beam_size=4, n_best=2, max_steps=16, ctc_weight=0.3)
    o.update(opt)
    if use_graph is not None:
        o["use_graph"] = use_graph
    return Decode(AttrDict(o), "cuda", model=m["model"], ctc_head=m["head"] if head else None, lm=lm)


def _check_search_scores(m, h, s, w, lam, lm):
    """Every returned hypothesis's score against the fp64 joint truth + lambda x the fp64 LM sum; -> the number of comparisons."""
    from oracle import beam_oracle as bo
    from tests.test_joint_decode_gpu import _joint_truth
    x, in_len = m["x"], m["in_len"]
    n_cmp = 0
    for b in range(x.shape[0]):
        for k in range(len(h[b])):
            hyp = h[b][k]
            if hyp[-1] != bo.EOS and bo.EOS in hyp:
                continue                                    # (extended past an EOS below the top: frozen CTC and LM parts)
            att = bo.score_hypothesis(m["p"], x[b:b + 1].double(), in_len[b:b + 1], 4, hyp)
            truth = _joint_truth(att, m["ctc_lp"][b], in_len[b], hyp, w) if w > 0 else att
            truth += lam * lm.score_list(hyp)
            print("utterance %d hypothesis %d: reported %.4f, fp64 %.4f" % (b, k, float(s[b][k]), truth))
            assert abs(float(s[b][k]) - truth) <= max(0.16, 5e-2 * abs(truth)), (b, k, hyp, float(s[b][k]), truth)
            n_cmp += 1
    return n_cmp


def test_search_with_lm_scores_match_fp64_and_graph_replay_is_exact():
    m = _small()
    src = (m["x"], m["in_len"])
    graph = _decode(m, lm=m["lm"], lm_weight=0.5, use_graph=True)
    outs = [graph.decode_batch(src), graph.decode_batch(src), _decode(m, lm=m["lm"], lm_weight=0.5, use_graph=False).decode_batch(src)]
    h, s = outs[0]
    for hh, ss in outs[1:]:
        assert hh == h and all(torch.equal(a, b) for a, b in zip(ss, s))
    assert _check_search_scores(m, h, s, 0.3, 0.5, m["lm"]) >= 5
    h0, _ = _decode(m).decode_batch(src)
    print("best hypotheses with the LM %s, without %s" % ([x[0] for x in h], [x[0] for x in h0]))


def test_search_without_lm_or_with_zero_weights_is_bit_equal_to_the_lm_less_search():
    m = _small()
    src = (m["x"], m["in_len"])
    h0, s0 = _decode(m).decode_batch(src)
    for dec in (_decode(m, lm=None, lm_weight=0.5), _decode(m, lm=m["lm"]), _decode(m, lm=m["lm"], lm_weight=0.0, lm_length_bonus=0.0)):
        assert not dec._lm_on
        h, s = dec.decode_batch(src)
        assert h == h0 and all(torch.equal(a, b) for a, b in zip(s, s0))
    a0 = _decode(m, head=False).decode_batch(src)
    a1 = _decode(m, head=False, lm=m["lm"]).decode_batch(src)
    assert a0[0] == a1[0] and all(torch.equal(a, b) for a, b in zip(a0[1], a1[1]))


def test_search_veto_removes_a_token():
    m = _small()
    src = (m["x"], m["in_len"])
    h0, _ = _decode(m).decode_batch(src)
    used = sorted({k for hyps in h0 for k in hyps[0] if k != EOS})
    assert used, "the LM-less best hypotheses hold no token but EOS"
    tok = used[0]
    table = {g: v for g, v in m["lm"].table.items() if tok not in g}
    veto = NGramLM.from_table(table, 3, 30, oov_logp=float("-inf")).to("cuda")
    h, s = _decode(m, lm=veto, lm_weight=0.5).decode_batch(src)
    for b in range(5):
        assert all(tok not in hyp for hyp in h[b]), (b, tok, h[b])
        assert math.isfinite(float(s[b][0])), (b, s[b])


def test_search_lm_only_route_scores_match_fp64_and_graph_replay_is_exact():
    m = _small()
    src = (m["x"], m["in_len"])
    graph = _decode(m, head=False, lm=m["lm"], lm_weight=0.5, use_graph=True)
    assert graph.lm_pre_beam == 6 and graph.ctc_pre_beam is None
    outs = [graph.decode_batch(src), graph.decode_batch(src),
            _decode(m, head=False, lm=m["lm"], lm_weight=0.5, use_graph=False).decode_batch(src)]
    h, s = outs[0]
    for hh, ss in outs[1:]:
        assert hh == h and all(torch.equal(a, b) for a, b in zip(ss, s))
    assert _check_search_scores(m, h, s, 0.0, 0.5, m["lm"]) >= 5


def test_decode_two_pass_with_lm_combines_three_scores():
    """decode_two_pass with lambda = 0.5 (and a length bonus): every score is (1 - w) score_nbest + w ctc_beam's + lambda lm_score +
    beta (len + 1) of its hypothesis, computed separately, within fp32 rounding of the sum; sorted; and lm_score equals the fp64
    definition over the trie's rounded values within the walk's bound summed over the positions."""
    from st_amd import ctc_beam
    from st_amd.arena import arena_of
    m = _small()
    src = (m["x"], m["in_len"])
    w, lam, beta, beam = 0.3, 0.5, 0.25, 4
    dec = _decode(m, lm=m["lm"], n_best=3, lm_weight=lam, lm_length_bonus=beta)
    hyps, scores = dec.decode_two_pass(src, beam=beam)
    with arena_of(dec.model).scope():
        enc, in_rows = dec._encode(src)
        first, ctc = ctc_beam.search_rows(m["head"], enc, in_rows, beam, max_len=15).lists()
    att = dec.score_nbest(src, first).double().cpu()
    lms = dec.lm_score(first)
    assert lms.dtype == F32 and tuple(lms.shape) == (5, beam) and lms.is_cuda
    lms = lms.double().cpu()
    ref = m["lm"].trie.rounded_model()
    n_cmp = 0
    for b in range(5):
        s = scores[b].double().cpu()
        assert all(s[i] >= s[i + 1] for i in range(2)), (b, s)
        want = {}
        for j, hyp in enumerate(first[b]):
            if ctc[b, j] == float("-inf"):
                continue
            terms = [(1.0 - w) * float(att[b, j]), w * float(ctc[b, j]), lam * float(lms[b, j]), beta * (len(hyp) + 1)]
            want[tuple(hyp)] = (sum(terms), sum(abs(v) for v in terms))
            # lm_score against the fp64 definition: per position the walk's bound, summed in fp64, rounded to fp32 once
            toks, bound, total = hyp + [EOS], 0.0, 0.0
            for t, c in enumerate(toks):
                pos = []
                emul.score(m["lm"].trie, ([-1, -1, BOS] + toks[:t])[-2:], c, pos)
                bound += emul.walk_bound(3, pos)
                total += ref.logp([BOS] + toks[:t], c)
            assert abs(float(lms[b, j]) - total) <= bound + 2.0 ** -24 * abs(total), (b, j, float(lms[b, j]), total, bound)
        ranked = sorted((v[0] for v in want.values()), reverse=True)
        for i, hyp in enumerate(hyps[b]):
            if s[i] == float("-inf"):
                assert hyp == [] and i >= len(want)
                continue
            exp, mag = want[tuple(hyp[:-1])]
            assert hyp[-1] == EOS and abs(float(s[i]) - exp) <= 2.0 ** -23 * mag, (b, i, float(s[i]), exp)
            assert abs(float(s[i]) - ranked[i]) <= 2.0 ** -23 * mag, (b, i, float(s[i]), ranked[i])
            n_cmp += 1
    assert n_cmp >= 5
    # lambda = 0 and beta = 0 on the call: the LM-less ranking
    plain = _decode(m, n_best=3).decode_two_pass(src, beam=beam)
    same = _decode(m, lm=m["lm"], n_best=3).decode_two_pass(src, beam=beam, lm_weight=0.0)
    assert plain[0] == same[0] and all(torch.equal(a, b) for a, b in zip(plain[1], same[1]))


def test_joint_decode_with_lm_at_config5_shape_graph_replay():
    """The benchmarked decode shape (seed-0 batch of st_amd.synthetic, 6+6 layers, d 256, V 4337, beam 10, B 32) joint-decoded for
    20 steps under graph replay with an order-4 model estimated from the batch's targets: every score finite, hypotheses within the
    step budget."""
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import synthetic
    from tests.test_joint_decode_gpu import C5, _head
    from transformer.Decode import Decode
    cfg = C5
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(cfg))
    U.init_parameters(model)
    model = model.eval().cuda()
    head = _head(cfg["vocab_size"], cfg["d_model"], 1.0, 3, "cuda")
    x, tokens, in_len, tgt_len, _ = synthetic.make_batch(32, 1000, 50, cfg["feature_dim"], cfg["vocab_size"], seed=0, t_min=500, l_min=25)
    lm = NGramLM.estimate([tokens[b, :int(tgt_len[b])].tolist() for b in range(32)], 4, cfg["vocab_size"]).to("cuda")
    dec = Decode(U.AttrDict(beam_size=10, n_best=2, max_steps=20, ctc_weight=0.3, lm_weight=0.5), "cuda", model=model, ctc_head=head, lm=lm)
    assert dec.use_graph and dec._lm_on
    hyps, scores = dec.decode_batch((x.cuda(), in_len))
    assert len(hyps) == 32
    for b in range(32):
        assert torch.isfinite(scores[b]).all(), (b, scores[b])
        assert 1 <= len(hyps[b][0]) <= 20

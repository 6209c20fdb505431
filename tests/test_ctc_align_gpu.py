"""-m gpu: st_ctc_align (csrc/st_ctc_align.hip) against the fp64 Viterbi of tests/_ctc_align_ref.py.

Exact cases: lp is integer-valued f32 in [-8, -1] - every add, compare and renormalising subtract of the kernel is exact, sums
stay far below 2^24 and ties are frequent - so path, spans and score must equal the reference BIT FOR BIT, tie rule included.
All four buffers of a launch (path, spans, score, workspace) sit between guard bands that must stay intact (tests/LOCAL_BOUNDS.md,
"Guards"); the outputs are pre-filled with a bit pattern, so equality also shows that every byte was written.

Real-valued cases (log-softmax of flat and peaked logits): the returned path must be a valid alignment, its score the fp64 sum
of lp along it, and that sum within a DERIVED bound of the fp64 optimum: each path takes one fp32 add per frame plus one
renormalising subtract per 8 frames on values of magnitude at most M = max(|optimum|, |score|), and two paths are compared:
2 (1 + 1/8) T 2^-24 M = 2.25 T 2^-24 M."""
import numpy as np
import pytest
import torch

from tests import _ctc_align_ref as ref
from tests._local import Guarded

pytestmark = pytest.mark.gpu

LDS_FRAMES = {63: 2048, 127: 2048, 255: 1024}       # frames of back-pointers the kernel keeps in LDS, by label capacity
CHUNK = {63: 16, 127: 16, 255: 8}                   # prefetch chunk of the forward sweep
TL = {63: [0, 1, 2, 3, 31, 62, 63], 127: [0, 1, 2, 63, 64, 65, 126, 127], 255: [0, 1, 3, 63, 64, 65, 127, 128, 129, 254, 255]}


def _nv():
    from st_amd import native as nv
    nv.load(build_if_missing=False)
    return nv


def _need(cls, tl):
    return tl + sum(int(cls[j] == cls[j - 1]) for j in range(1, tl))


def _launch(lp, cls, il, tl, ws_extra=0):
    """One st_ctc_align launch into guarded buffers -> (path, spans, score) as numpy, guards checked."""
    nv = _nv()
    B, T, _ = lp.shape
    L = cls.shape[1]
    g_path = Guarded.vec(B * T, torch.int32, "cuda")
    g_spans = Guarded.vec(B * L * 2, torch.int32, "cuda")
    g_score = Guarded.vec(B, torch.float32, "cuda")
    g_ws = Guarded.vec(nv.ctc_align_ws_bytes(B, T, L) + ws_extra, torch.uint8, "cuda")
    path, spans, score = g_path.view.view(B, T), g_spans.view.view(B, L, 2), g_score.view
    nv.ctc_align(lp.cuda(), cls.cuda(), il.to("cuda", torch.int32), tl.to("cuda", torch.int32), g_ws.view, path, spans, score)
    torch.cuda.synchronize()
    for gd, what in ((g_path, "path"), (g_spans, "spans"), (g_score, "score"), (g_ws, "workspace")):
        gd.assert_intact("st_ctc_align: " + what)
    return path.cpu().numpy(), spans.cpu().numpy(), score.cpu().numpy()


def _int_mix(T, L, B, seed, C=6):
    """A ragged mix of utterances that share one launch: integer emissions in [-8, -1]; classes drawn from C - 1 labels plus
    class 0 (adjacent repeats at ~1 position in 6, labels equal to class 0), junk past every target length; tl walks the values
    either side of the lane / template boundaries; in_len walks T, T - 1, T - 2, 0, tl + repeats (the unique path), tl + repeats
    - 1 (infeasible) and random values."""
    rng = np.random.default_rng(seed)
    lp = torch.from_numpy(rng.integers(-8, 0, size=(B, T, C)).astype(np.float32))
    cls = torch.from_numpy(rng.integers(0, C, size=(B, L)).astype(np.int64))
    tls = [t for t in TL[L]]
    small = [t for t in tls if t + t // 4 <= T] or [0]
    il, tl = [], []
    for b in range(B):
        t_b = tls[b % len(tls)] if b % 2 == 0 else small[(b // 2) % len(small)]       # half of them can be feasible at a small T
        need = _need(cls[b].tolist(), t_b)
        choice = [T, T - 1, need, T - 2, need - 1, 0, int(rng.integers(0, T + 1))][(b // 2 + b % 2 * 3) % 7]
        il.append(min(max(choice, 0), T))
        tl.append(t_b)
        cls[b, t_b:] = torch.from_numpy(rng.choice([-7, 999, 1 << 40, 3], size=L - t_b))      # never read
    return lp, cls, torch.tensor(il), torch.tensor(tl)


def _cases():
    out = []
    for L in (63, 127, 255):
        ch, f = CHUNK[L], LDS_FRAMES[L]
        small = sorted({1, 2, 7, 8, 9, ch - 1, ch, ch + 1, 100})
        out += [(T, L, 33) for T in small]
        out += [(T, L, 7) for T in sorted({f - 1, f, f + 1, 2048})]
    return out


@pytest.mark.parametrize("T,L,B", _cases())
def test_integer_emissions_equal_the_reference_bit_for_bit(T, L, B):
    lp, cls, il, tl = _int_mix(T, L, B, seed=1000 * L + T)
    if T > LDS_FRAMES[L]:                              # both homes of the back-pointers in one launch, either side of the threshold
        il[0], il[1], il[2] = T, LDS_FRAMES[L], LDS_FRAMES[L] + 1
        tl[0], tl[1], tl[2] = L, L, L - 1
        cls[:3] = torch.from_numpy(np.random.default_rng(T).integers(0, 6, size=(3, L)))      # (valid up to the new lengths)
    want = ref.align_batch(lp.numpy(), cls.numpy(), il.tolist(), tl.tolist())
    got = _launch(lp, cls, il, tl)
    feasible = np.isfinite(want[2])
    if T >= 100:
        assert feasible.any() and (~feasible).any(), "the mix must hold utterances with and without an alignment"
    for b in range(B):
        what = "utterance %d (in_len %d, tl %d, T %d, L %d)" % (b, int(il[b]), int(tl[b]), T, L)
        assert np.array_equal(got[0][b], want[0][b]), what + ": path"
        assert np.array_equal(got[1][b], want[1][b]), what + ": spans"
        assert got[2][b] == want[2][b], what + ": score %r, reference %r" % (got[2][b], want[2][b])
        assert (got[0][b, int(il[b]):] == -1).all() and (got[1][b, int(tl[b]):] == -1).all(), what
        if not feasible[b]:
            assert (got[0][b] == -1).all() and (got[1][b] == -1).all() and got[2][b] == -np.inf, what


def test_small_alphabet_junk_past_the_lengths_and_oversized_workspace():
    """L = 5 with tgt_len < L everywhere, class junk past it, lp poisoned with NaN past every in_len, in_len < T, in_len = 0,
    the unique path and the infeasible length one below it; a workspace larger than asked for."""
    B, T, L, C = 12, 40, 5, 4
    rng = np.random.default_rng(7)
    lp = torch.from_numpy(rng.integers(-8, 0, size=(B, T, C)).astype(np.float32))
    cls = torch.from_numpy(rng.integers(0, C, size=(B, L)).astype(np.int64))
    cls[0, :4] = torch.tensor([2, 2, 0, 0])          # adjacent repeats, of a label and of class 0
    tl = torch.tensor([4, 4, 4, 3, 2, 1, 0, 0, 4, 3, 2, 1])
    need = [_need(cls[b].tolist(), int(tl[b])) for b in range(B)]
    il = torch.tensor([need[0], need[1] - 1, 40, 39, 17, 1, 0, 9, 0, need[9], need[10] - 1, 8])
    for b in range(B):
        lp[b, int(il[b]):] = float("nan")
        cls[b, int(tl[b]):] = 1 << 33
    want = ref.align_batch(torch.nan_to_num(lp, nan=0.0).numpy(), cls.numpy(), il.tolist(), tl.tolist())
    got = _launch(lp, cls, il, tl, ws_extra=4096)
    for k, what in enumerate(("path", "spans", "score")):
        assert np.array_equal(got[k], want[k]), what
    assert np.isfinite(want[2][0]) and want[2][1] == -np.inf and want[2][6] == -np.inf and want[2][8] == -np.inf
    assert want[0][0, :need[0]].tolist() == [0, -1, 1, 2, -1, 3]          # the unique path of [2, 2, 0, 0] in 6 frames


def _real_case(T, L, B, scale, seed):
    g = torch.Generator().manual_seed(seed)
    C = L + 1
    lp = torch.log_softmax(torch.randn(B, T, C, generator=g, dtype=torch.float64) * scale, -1).float()
    cls = torch.randint(1, C, (B, L), generator=g)
    cls[:, 1::5] = cls[:, 0::5][:, :cls[:, 1::5].shape[1]]       # adjacent repeats
    cls[:, 7] = 0                                                 # a label equal to class 0
    tl = torch.randint(L // 2, L + 1, (B,), generator=g)
    tl[0] = L
    need = torch.tensor([_need(cls[b].tolist(), int(tl[b])) for b in range(B)])
    il = torch.maximum(torch.randint(T // 2, T + 1, (B,), generator=g), need)
    il[0], il[1] = T, need[1]                                     # (utterance 1: the unique path)
    return lp, cls, il, tl


@pytest.mark.parametrize("T", [200, 1000])
@pytest.mark.parametrize("scale,kind", [(0.1, "flat"), (5.0, "peaked")])
def test_real_valued_alignment_is_valid_and_optimal_within_the_derived_bound(T, scale, kind):
    B, L = 8, 50
    lp, cls, il, tl = _real_case(T, L, B, scale, seed=T + int(10 * scale))
    want = ref.align_batch(lp.numpy(), cls.numpy(), il.tolist(), tl.tolist())
    path, spans, score = _launch(lp, cls, il, tl)
    lp64 = lp.double().numpy()
    for b in range(B):
        Tb, t_b = int(il[b]), int(tl[b])
        S = 2 * t_b + 1
        states = ref.states_of(path[b], Tb)
        ext, skip = ref.extended(cls[b, :t_b].tolist())
        # a valid alignment: starts in state 0 or 1, moves by 0 / +1 / an allowed +2, ends in S-1 or S-2, collapses to the labels
        assert states[0] <= 1 and states[-1] >= S - 2 and states[-1] <= S - 1, (b, states[0], states[-1])
        for a, c in zip(states, states[1:]):
            assert c == a or c == a + 1 or (c == a + 2 and skip[c]), (b, a, c)
        seen = [j for t, j in enumerate(path[b, :Tb]) if j >= 0 and (t == 0 or path[b, t - 1] != j)]
        assert seen == list(range(t_b)) and (path[b, Tb:] == -1).all()
        for j in range(t_b):
            s, e = spans[b, j]
            assert 0 <= s < e <= Tb and (path[b, s:e] == j).all() and (path[b, :s] != j).all() and (path[b, e:Tb] != j).all()
        assert (spans[b, t_b:] == -1).all()
        # the score is the fp64 sum of lp along the returned path
        along = float(sum(lp64[b, t, ext[s]] for t, s in enumerate(states)))
        print("%s T %d utterance %d: score %.6f, along the path %.6f, fp64 optimum %.6f" % (kind, T, b, score[b], along, want[3][b]))
        assert abs(float(score[b]) - along) <= 1e-6 * abs(along), (b, score[b], along)
        # optimality within the derived bound
        M = max(abs(want[3][b]), abs(float(score[b])))
        assert want[3][b] - along <= 2.25 * Tb * 2.0 ** -24 * M, (b, want[3][b], along, 2.25 * Tb * 2.0 ** -24 * M)
    # the unique path (in_len = tl + repeats) matches the reference exactly
    assert np.array_equal(path[1], want[0][1]) and np.array_equal(spans[1], want[1][1]) and score[1] == want[2][1]


def test_score_is_below_the_loss_likelihood_and_two_launches_are_bit_equal():
    """On the same lp: the best path cannot beat the sum over all paths, score <= -nll + 1e-3 |nll| with nll from
    st_ctc_loss_fwd; and two launches agree bit for bit."""
    nv = _nv()
    B, T, L = 8, 200, 50
    lp, cls, il, tl = _real_case(T, L, B, 2.0, seed=3)
    il[2] = int(tl[2]) - 1                                        # one utterance without an alignment: nll +inf, score -inf
    a = _launch(lp, cls, il, tl)
    b = _launch(lp, cls, il, tl)
    for x, y, what in zip(a, b, ("path", "spans", "score")):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), what + " differs between two launches"
    ws = torch.empty(nv.ctc_loss_ws_bytes(B, T, L), dtype=torch.uint8, device="cuda")
    nll = nv.ctc_loss_fwd(lp.cuda(), cls.cuda(), il.to("cuda", torch.int32), tl.to("cuda", torch.int32), ws,
                          torch.empty(B, dtype=torch.float32, device="cuda")).cpu().numpy()
    for u in range(B):
        if u == 2:
            assert nll[u] == np.inf and a[2][u] == -np.inf
        else:
            assert np.isfinite(nll[u]) and a[2][u] <= -nll[u] + 1e-3 * abs(nll[u]), (u, a[2][u], nll[u])
            # (nor can it fall further below: at most 3^T paths, so -nll <= score + T ln 3)
            assert a[2][u] >= -nll[u] - 1.1 * int(il[u]), (u, a[2][u], nll[u])


def test_ctc_align_under_graph_capture_follows_refilled_buffers():
    """One torch.cuda.graph capture of st_ctc_align: the replay equals the eager launch, and a replay after lp, labels and both
    length vectors were refilled IN PLACE follows the new contents (nothing was baked in at capture)."""
    nv = _nv()
    B, T, L = 8, 200, 50
    lp1, cls1, il1, tl1 = _real_case(T, L, B, 2.0, seed=21)
    lp2, cls2, il2, tl2 = _real_case(T, L, B, 0.5, seed=22)
    il2[3], tl2[4] = 0, 0
    e1, e2 = _launch(lp1, cls1, il1, tl1), _launch(lp2, cls2, il2, tl2)
    lp_s, cls_s = lp1.cuda(), cls1.cuda()
    il_s, tl_s = il1.to("cuda", torch.int32), tl1.to("cuda", torch.int32)
    ws = torch.empty(nv.ctc_align_ws_bytes(B, T, L), dtype=torch.uint8, device="cuda")
    path = torch.zeros(B, T, dtype=torch.int32, device="cuda")
    spans = torch.zeros(B, L, 2, dtype=torch.int32, device="cuda")
    score = torch.zeros(B, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nv.ctc_align(lp_s, cls_s, il_s, tl_s, ws, path, spans, score)
    for want, (lp, cls, il, tl) in ((e1, (lp1, cls1, il1, tl1)), (e2, (lp2, cls2, il2, tl2))):
        lp_s.copy_(lp)
        cls_s.copy_(cls)
        il_s.copy_(il)
        tl_s.copy_(tl)
        path.fill_(77)
        spans.fill_(77)
        score.fill_(77.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(path.cpu().numpy(), want[0]) and np.array_equal(spans.cpu().numpy(), want[1])
        assert np.array_equal(score.cpu().numpy().view(np.int32), want[2].view(np.int32))
    assert not np.array_equal(e1[0], e2[0])


def test_decode_align_on_a_small_joint_model():
    """Decode.align on a 2+2-layer d_model-256 joint model with the hypotheses decode_batch returns: spans contiguous, ordered and
    inside [0, in_len); the tokens' logp plus the blank rows' sum to the score (blank rows belong to no token, so the per-token
    sums alone stop short of it by exactly that term); and path / spans / score equal the reference run on the lp the plan holds."""
    import oracle as orc
    import transformer.Constants as Constants
    import transformer.Models as M
    import transformer.Utils as U
    from transformer.Decode import Decode
    from transformer.Loss import CTCAttentionLoss
    p = orc.xavier_init_(orc.make_params(80, 30, 256, 512, 2, 2, 100, 20, dtype=torch.float64), seed=3)
    cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=100, max_target_length=20, num_enc_layer=2, num_dec_layer=2, n_heads=4,
                          d_k=64, d_v=64, d_model=256, d_inner_hid=512, dropout=0.0, vocab_size=30))
    model = M.Transformer(cfg)
    model.load_state_dict({k: v.float() for k, v in p.items()})
    model = model.eval().cuda()
    torch.manual_seed(1)
    head = CTCAttentionLoss(256, 30)
    with torch.no_grad():
        head.ctc_proj.weight.mul_(8.0)
    head = head.cuda()
    batch = orc.synthetic_batch(5, 80, 10, 80, 30, seed=2, t_min=30, l_min=5)
    src = (batch["x"], batch["in_len"])
    dec = Decode(U.AttrDict(dict(beam_size=4, n_best=1, max_steps=16, ctc_weight=0.3)), "cuda", model=model, ctc_head=head)
    hyps = [h[0] for h in dec.decode_batch(src)[0]]
    assert any(len(h) > 1 for h in hyps)
    out = dec.align(src, hyps)
    al = dec.alignment
    plan = al.plan
    in_len = batch["in_len"].tolist()
    tl = plan.tgt_len_dev.cpu().tolist()
    want = ref.align_batch(plan.lp.cpu().numpy(), plan.classes.cpu().numpy(), in_len, tl)
    path, spans, score = al.path.cpu().numpy(), al.spans.cpu().numpy(), al.score.cpu().numpy()
    lp64 = plan.lp.double().cpu().numpy()
    n_items = 0
    for b, (items, sc) in enumerate(out):
        labels = hyps[b][:-1] if hyps[b] and hyps[b][-1] == Constants.EOS else hyps[b]
        assert len(labels) == tl[b]
        if want[2][b] == -np.inf:
            assert items == [] and sc == float("-inf")
            continue
        assert [it[0] for it in items] == labels and sc == float(score[b])
        end = 0
        for j, (tok, s, e, logp) in enumerate(items):
            assert end <= s < e <= in_len[b] and [s, e] == spans[b, j].tolist() and (path[b, s:e] == j).all()
            end = e
            n_items += 1
        blank = float(sum(lp64[b, t, 0] for t in range(in_len[b]) if path[b, t] < 0))
        total = sum(it[3] for it in items) + blank
        assert abs(total - sc) <= 1e-5 * abs(sc), (b, total, sc)
        assert abs(float(al.blank_logp[b]) - blank) <= 1e-5 * max(1.0, abs(blank))
        # against the reference on the plan's lp
        ext, _ = ref.extended(plan.classes[b, :tl[b]].cpu().tolist())
        along = float(sum(lp64[b, t, ext[s]] for t, s in enumerate(ref.states_of(path[b], in_len[b]))))
        print("utterance %d: score %.6f, along the path %.6f, fp64 optimum %.6f" % (b, sc, along, want[3][b]))
        assert np.array_equal(path[b], want[0][b]), (b, path[b], want[0][b])
        assert np.array_equal(spans[b], want[1][b]) and abs(sc - float(want[2][b])) <= 1e-6 * abs(sc)
    assert n_items > 0

"""-m gpu: joint CTC / attention beam search (csrc/st_ctc_decode.hip, st_amd/ctc_decode.py, transformer/Decode.py with a CTC
head) against torch and the fp64 restatements: the CTC table, the prefix scorer over a grid of batch / beam / pre-beam / frame
counts, the pre-beam and the joint advance against torch formulations, teacher-forced joint scores against the fp64 oracle,
search parity on the small decode model, graph replay, a config-5-shape joint decode and greedy CTC decoding."""
import math
import os

import numpy as np
import pytest
import torch

import oracle as orc
from oracle import beam_oracle as bo
from tests import _ctc_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK = 0
C5 = dict(feature_dim=80, max_inputs_length=1000, max_target_length=50, num_enc_layer=6, num_dec_layer=6, n_heads=4,
          d_k=64, d_v=64, d_model=256, d_inner_hid=1024, dropout=0.1, vocab_size=4337)


def _nv():
    from st_amd import native as nv
    nv.load(build_if_missing=False)
    return nv


def _report(name, lines):
    """Append measured errors to profile_out/<name> (the untracked output directory of tools/profile_round.sh)."""
    out = os.path.join(ROOT, "profile_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, name), "a") as f:
        f.write("\n".join(lines) + "\n")


def _lengths(B, T, g):
    lens = torch.randint(max(1, T // 2), T + 1, (B,), generator=g)
    lens[0] = T
    return lens


def test_ctc_vocab_lp_matches_log_softmax():
    nv = _nv()
    from st_amd.ctc_decode import frame_capacity
    g = torch.Generator().manual_seed(0)
    V, v_pad = 301, 312
    lens = torch.tensor([70, 1, 129, 64])
    R = int(lens.sum())
    logits = torch.full((R, v_pad), -1e30)
    logits[:, :V] = torch.randn(R, V, generator=g) * 4
    off = torch.cumsum(lens, 0) - lens
    T_cap = frame_capacity(int(lens.max()))
    lpT = torch.full((4, V, T_cap), 7.0, device="cuda")
    lse = torch.empty(R, device="cuda")
    nv.ctc_vocab_lp(logits.cuda(), V, off.int().cuda(), lens.int().cuda(), T_cap, lse, lpT)
    want = torch.log_softmax(logits[:, :V].double(), -1)
    assert torch.allclose(lse.cpu().double(), torch.logsumexp(logits[:, :V].double(), -1), atol=2e-5, rtol=0)
    got = lpT.cpu()
    for b in range(4):
        o, T = int(off[b]), int(lens[b])
        assert (got[b, :, :T].double().t() - want[o:o + T]).abs().max() <= 2e-5
        assert torch.all(got[b, :, T:] == 0)


def _grid():
    out = []
    for B, beam, K, T in [(1, 1, 1, 1), (1, 1, 16, 7), (5, 4, 4, 7), (5, 4, 9, 128), (5, 10, 16, 1000), (32, 10, 15, 1000),
                          (32, 4, 4, 128), (32, 1, 16, 1), (1, 10, 10, 1000), (5, 1, 3, 128)]:
        out.append((B, beam, K, T))
    return out


@pytest.mark.parametrize("B,beam,K,T", _grid())
def test_ctc_prefix_score_matches_fp64(B, beam, K, T):
    """st_ctc_prefix_score against the fp64 restatement: random peaky log-probabilities, ragged lengths, hypotheses with random
    prefixes of 0..3 labels (states made by the fp64 recursion), candidates covering the empty prefix, c == last(g), EOS and
    blank; frozen hypotheses get increment 0 and the hypotheses of done utterances are left bit-unchanged."""
    nv = _nv()
    from st_amd.ctc_decode import frame_capacity
    g = torch.Generator().manual_seed(1000 * B + 100 * beam + K + T)
    rng = np.random.default_rng(B * 7 + beam * 3 + K + T)
    V, eos = 40, 2
    lens = _lengths(B, T, g)
    T_cap = frame_capacity(T)
    x = torch.log_softmax(torch.randn(B, T_cap, V, generator=g, dtype=torch.float64) * 3.0, -1)
    x32 = x.float()
    xd = x32.double().numpy()                            # the fp64 side reads the same fp32-rounded table
    lpT = x32.transpose(1, 2).contiguous()
    for b in range(B):
        lpT[b, :, int(lens[b]):] = 0.0
    n = B * beam
    # hypothesis states: the fp64 recursion over random prefixes
    gn = np.full((n, T_cap), -np.inf)
    gb = np.full((n, T_cap), -np.inf)
    psi = np.zeros(n)
    last = np.full(n, -1)
    ub = np.arange(n) // beam
    plen = rng.integers(0, 4, n)
    plen[::beam] = 0                                     # slot 0: the empty prefix
    for i in range(n):
        gb[i, :lens[ub[i]]] = np.cumsum(xd[ub[i], :lens[ub[i]], BLANK])
    Tn = lens.numpy()[ub]
    for p in range(3):
        rows = np.nonzero(plen > p)[0]
        if rows.size == 0:
            continue
        c = rng.integers(3, V, rows.size)
        c = np.where(rng.random(rows.size) < 0.3, np.where(last[rows] >= 3, last[rows], c), c)       # immediate repeats
        p_h, hn, hb = ref.extend_batch(xd[ub[rows], :, :][np.arange(rows.size), :, c], xd[ub[rows], :, BLANK], gn[rows], gb[rows],
                                       last[rows], c, Tn[rows], BLANK, eos)
        gn[rows], gb[rows], psi[rows], last[rows] = hn, hb, p_h, c
    frozen = rng.random(n) < 0.15
    done = np.zeros(B, dtype=bool)
    if B > 1:
        done[1] = True
    cand = rng.integers(3, V, (n, K))
    cand[:, 0] = np.where(last >= 0, last, cand[:, 0])  # c == last(g)
    if K > 1:
        cand[:, 1] = eos
    if K > 2:
        cand[:, 2] = BLANK
    dev = "cuda"
    gam = torch.from_numpy(np.stack([gn, gb], 1)).float().contiguous()
    args = dict(gam=gam.to(dev), psi=torch.from_numpy(psi).float().to(dev), last=torch.from_numpy(last).int().to(dev),
                frozen=torch.from_numpy(frozen).to(dev))
    cand_gam = torch.full((n, K, 2, T_cap), 12345.0, device=dev)
    cand_psi = torch.full((n, K), 12345.0, device=dev)
    delta = torch.full((n, K), 12345.0, device=dev)
    nv.ctc_prefix_score(lpT.to(dev), lens.int().to(dev), beam, BLANK, eos, torch.from_numpy(cand).int().to(dev), args["gam"], args["psi"],
                        args["last"], args["frozen"], torch.from_numpy(done).to(dev), cand_gam, cand_psi, delta)
    cg, cp, dl = cand_gam.cpu(), cand_psi.cpu().double().numpy(), delta.cpu().double().numpy()
    # the fp64 side starts from the fp32-rounded states the kernel read
    gn32, gb32, psi32 = gam[:, 0].double().numpy(), gam[:, 1].double().numpy(), gam.new_tensor(psi).float().double().numpy()
    ii = np.repeat(np.arange(n), K)
    cc = cand.reshape(-1)
    p_ref, hn_ref, hb_ref = ref.extend_batch(xd[ub[ii], :, :][np.arange(ii.size), :, cc], xd[ub[ii], :, BLANK], gn32[ii], gb32[ii],
                                             last[ii], cc, Tn[ii], BLANK, eos)
    d_ref = np.where(np.isneginf(p_ref), -np.inf, p_ref - psi32[ii])
    worst, n_cmp = 0.0, 0
    for w in range(n * K):
        i, j = divmod(w, K)
        if done[ub[i]]:
            assert cp[i, j] == 12345.0 and dl[i, j] == 12345.0 and torch.all(cg[i, j] == 12345.0), (i, j)
            continue
        if frozen[i]:
            assert dl[i, j] == 0.0 and cp[i, j] == np.float32(psi[i]), (i, j)
            assert torch.all(cg[i, j] == 12345.0)
            continue
        if np.isneginf(d_ref[w]):
            assert np.isneginf(dl[i, j]), (i, j, dl[i, j])
            continue
        err = abs(dl[i, j] - d_ref[w])
        # measured on the MI355X: worst |err| / (1e-3 + 1e-5 |psi|) = 0.0086 over the grid (B 32, beam 10, K 15, T 1000; fp32
        # rounding of psi ~ -8,000 in the difference psi(h) - psi(g)); the bound is 4x that
        bound = 0.035 * (1e-3 + 1e-5 * abs(p_ref[w]))
        worst = max(worst, err / (1e-3 + 1e-5 * abs(p_ref[w])))
        n_cmp += 1
        assert err <= bound, (i, j, cc[w], dl[i, j], d_ref[w])
        if cc[w] not in (eos, BLANK):
            T_i = int(Tn[i])
            for row, want in ((0, hn_ref[w, :T_i]), (1, hb_ref[w, :T_i])):
                got = cg[i, j, row, :T_i].double().numpy()
                fin = np.isfinite(want)
                assert np.array_equal(fin, np.isfinite(got)), (i, j, row)
                assert np.all(np.abs(got[fin] - want[fin]) <= 1e-3 + 1e-5 * np.abs(want[fin])), (i, j, row)
    assert n_cmp > 0
    _report("ctc_prefix_score_err.txt", ["B %d beam %d K %d T %d: %d increments, worst |err| / (1e-3 + 1e-5 |psi|) = %.4f"
                                         % (B, beam, K, T, n_cmp, worst)])


@pytest.mark.parametrize("n,V,K", [(7, 30, 16), (40, 4337, 15), (3, 4337, 64), (5, 5120, 10)])
def test_beam_pre_beam_matches_torch(n, V, K):
    nv = _nv()
    g = torch.Generator().manual_seed(n + V + K)
    ld = (V + 7) // 8 * 8
    logits = torch.full((n, ld), -1e30)
    logits[:, :V] = torch.randn(n, V, generator=g) * 5
    ids = torch.empty(n, K, dtype=torch.int32, device="cuda")
    lp = torch.empty(n, K, device="cuda")
    nv.beam_pre_beam(logits.cuda(), V, ids, lp)
    want = torch.log_softmax(logits[:, :V].double(), -1)
    v, i = want.topk(K, -1)
    assert torch.equal(ids.cpu().long(), i)
    assert (lp.cpu().double() - v).abs().max() <= 2e-5


def _joint_torch(st, ids, lp, delta, w, beam, K, eos, step):
    """The torch formulation of st_beam_advance_joint (one step, all utterances)."""
    B = st["scores"].shape[0]
    out = {k: v.clone() for k, v in st.items()}
    for b in range(B):
        rows = slice(b * beam, (b + 1) * beam)
        if bool(st["done"][b]):
            out["back"][step, b] = torch.arange(beam)
            out["toks"][step, b] = st["tokens"][rows]
            out["hist"][step, b] = st["scores"][b]
            out["order"][rows] = torch.arange(beam) + b * beam
            continue
        inc = (1 - w) * lp[rows] + (w * delta[rows] if w > 0 else 0.0)
        val = (st["scores"][b].unsqueeze(1) + inc).reshape(-1)
        keys = sorted(range(beam * K), key=lambda f: (-float(val[f]), f))[:beam]
        for s, f in enumerate(keys):
            o, j = divmod(f, K)
            tk = int(ids[b * beam + o, j])
            out["hist"][step, b, s] = st["scores"][b, s]
            out["back"][step, b, s] = o
            out["toks"][step, b, s] = tk
            out["order"][b * beam + s] = o + b * beam
            out["scores"][b, s] = val[f]
            out["tokens"][b * beam + s] = tk
            src = b * beam + o
            pf = bool(st["frozen"][src])
            out["psi"][b * beam + s] = st["psi"][src] if pf else st["cand_psi"][src, j]
            out["last"][b * beam + s] = st["last"][src] if pf else tk
            out["frozen"][b * beam + s] = pf or tk == eos
            if not pf and tk != eos:
                out["gam"][b * beam + s] = st["cand_gam"][src, j]
            T = step
            out["anc"][b * beam + s, :T] = st["anc"][src, :T]
            out["anc"][b * beam + s, T] = src
        out["lengths"][b] += 1
        if int(out["tokens"][b * beam]) == eos:
            out["done"][b] = True
    return out


@pytest.mark.parametrize("B,beam,K,w", [(5, 4, 6, 0.3), (3, 10, 15, 0.5), (2, 16, 64, 0.3), (4, 1, 2, 0.0)])
def test_beam_advance_joint_matches_torch_formulation(B, beam, K, w):
    """st_beam_advance_joint against a torch formulation over several steps: -inf slots at step 0, -inf increments (blank /
    impossible prefixes), EOS (a done utterance is frozen), frozen hypotheses, the moved CTC state and the lineage table."""
    nv = _nv()
    g = torch.Generator().manual_seed(B * 100 + beam + K)
    S, T_cap, eos, V = 6, 64, 2, 80
    n = B * beam
    sc = torch.full((B, beam), float("-inf"))
    sc[:, 0] = 0.0
    st = dict(scores=sc, tokens=torch.full((n,), 1, dtype=torch.long), done=torch.zeros(B, dtype=torch.bool),
              lengths=torch.zeros(B, dtype=torch.long), hist=torch.zeros(S, B, beam), back=torch.zeros(S, B, beam, dtype=torch.long),
              toks=torch.zeros(S, B, beam, dtype=torch.long), order=torch.zeros(n, dtype=torch.long),
              anc=torch.arange(n, dtype=torch.int32).unsqueeze(1).repeat(1, S).contiguous(),
              gam=torch.randn(n, 2, T_cap), psi=torch.randn(n), last=torch.randint(-1, V, (n,), generator=g).int(),
              frozen=torch.rand(n, generator=g) < 0.2)
    if B > 1:
        st["done"][B - 1] = True
    dev = {k: v.cuda() for k, v in st.items()}
    step = torch.zeros(1, dtype=torch.long, device="cuda")
    ticket = torch.zeros(1, dtype=torch.long, device="cuda")
    for t in range(S - 1):
        ids = torch.stack([torch.randperm(V, generator=g)[:K] for _ in range(n)]).int()
        if t >= 2:
            ids[0, 0] = eos                                 # the best candidate of utterance 0 -> EOS
        lp = -torch.rand(n, K, generator=g) * 5
        lp[0, 0] = 5.0 if t >= 2 else lp[0, 0]
        delta = -torch.rand(n, K, generator=g) * 3
        delta[torch.rand(n, K, generator=g) < 0.1] = float("-inf")
        cand_gam = torch.randn(n, K, 2, T_cap, generator=g)
        cand_psi = torch.randn(n, K, generator=g)
        full = dict(st, cand_gam=cand_gam, cand_psi=cand_psi)
        want = _joint_torch(full, ids, lp, delta if w > 0 else torch.zeros_like(delta), w, beam, K, eos, t)
        nv.beam_advance_joint(ids.cuda(), lp.cuda(), delta.cuda(), w, beam, step, eos, dev["scores"], dev["tokens"], dev["done"],
                              dev["lengths"], dev["hist"], dev["back"], dev["toks"], dev["order"], anc=dev["anc"], advance_step=True,
                              ticket=ticket, ctc=(cand_gam.cuda(), cand_psi.cuda(), dev["gam"], dev["psi"], dev["last"], dev["frozen"]))
        assert int(step) == t + 1 and int(ticket) == 0
        for k in ("back", "toks", "order", "tokens", "lengths", "done", "last", "frozen", "anc"):
            assert torch.equal(dev[k].cpu(), want[k].to(dev[k].dtype)), (t, k)
        for k in ("scores", "hist", "psi", "gam"):
            a, b = dev[k].cpu(), want[k].float()
            fin = torch.isfinite(b)
            assert torch.equal(torch.isfinite(a), fin) and torch.allclose(a[fin], b[fin], atol=1e-5, rtol=1e-6), (t, k)
        st = {k: dev[k].cpu() for k in st}


def _head(V, d, scale, seed, device):
    from transformer.Loss import CTCAttentionLoss
    torch.manual_seed(seed)
    head = CTCAttentionLoss(d, V)
    with torch.no_grad():
        head.ctc_proj.weight.mul_(scale)
        head.ctc_proj.bias.zero_()
        head.ctc_proj.bias[BLANK] = 2.0                 # mostly blank frames, peaky label frames
    return head.to(device)


def _ctc_lp64(p, head, x, in_len, n_head, device="cpu"):
    """fp64 CTC log-probabilities [B, T, V] from the oracle encoder and the head's weights."""
    enc, _ = orc.encoder(p, x[:, :int(in_len.max())], in_len, n_head)
    W = head.ctc_proj.weight.detach().double().to(enc.device)
    bb = head.ctc_proj.bias.detach().double().to(enc.device)
    return torch.log_softmax(enc @ W.t() + bb, -1)


def _joint_truth(lp_att_sum, ctc_lp, in_len, hyp, w):
    """(1 - w) sum log p_att + w (psi(hyp) or log p_ctc(hyp without EOS))."""
    x = ctc_lp[:int(in_len)].cpu().numpy()
    if hyp and hyp[-1] == bo.EOS:
        _, end = ref.prefix_scores(x, hyp[:-1], BLANK, bo.EOS)
        c = end
    else:
        psis, _ = ref.prefix_scores(x, hyp, BLANK, bo.EOS)
        c = psis[-1]
    return (1 - w) * lp_att_sum + w * c


def _small(device, eos_boost=3.0):
    from tests.test_decode_cpu import _params, _model
    p = _params(eos_boost)
    return p, _model(p, device)


def test_joint_weight_zero_with_head_is_bit_equal_to_attention_only():
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    p, model = _small("cuda")
    batch = orc.synthetic_batch(5, 80, 10, 80, 30, seed=2, t_min=30, l_min=5)
    src = (batch["x"], batch["in_len"])
    a = Decode(AttrDict(dict(beam_size=4, n_best=2, max_steps=16)), "cuda", model=model)
    h1, s1 = a.decode_batch(src)
    b = Decode(AttrDict(dict(beam_size=4, n_best=2, max_steps=16, ctc_weight=0.0)), "cuda", model=model,
               ctc_head=_head(30, 128, 8.0, 0, "cuda"))
    h2, s2 = b.decode_batch(src)
    assert h1 == h2
    assert all(torch.equal(x, y) for x, y in zip(s1, s2))
    att = a.score_hypotheses(src, [h[0] for h in h1])
    assert torch.equal(att, b.score_hypotheses(src, [h[0] for h in h1]))
    assert torch.equal(att, b.score_hypotheses(src, [h[0] for h in h1], ctc_weight=0.0))


def test_score_hypotheses_joint_small_model_vs_fp64():
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    p, model = _small("cuda")
    head = _head(30, 128, 8.0, 1, "cuda")
    batch = orc.synthetic_batch(5, 80, 10, 80, 30, seed=2, t_min=30, l_min=5)
    x, in_len = batch["x"], batch["in_len"]
    g = torch.Generator().manual_seed(3)
    hyps = [torch.randint(4, 30, (int(k),), generator=g).tolist() for k in (3, 5, 6, 8, 4)]
    for b in (0, 2, 3):
        hyps[b] = hyps[b] + [bo.EOS]
    hyps[1][2] = hyps[1][1]                                 # a repeated label
    w = 0.3
    dec = Decode(AttrDict(dict(beam_size=4, n_best=1, max_steps=16)), "cuda", model=model, ctc_head=head)
    got = dec.score_hypotheses((x, in_len), hyps, ctc_weight=w).double().cpu()
    ctc_lp = _ctc_lp64(p, head, x.double(), in_len, 4)
    errs = []
    for b in range(5):
        att = bo.score_hypothesis(p, x[b:b + 1].double(), in_len[b:b + 1], 4, hyps[b])
        truth = _joint_truth(att, ctc_lp[b], in_len[b], hyps[b], w)
        errs.append(float(got[b]) - truth)
        assert abs(float(got[b]) - truth) <= max(0.16, 5e-2 * abs(truth)), (b, float(got[b]), truth)
    _report("joint_score_parity.txt", ["small model, w 0.3: joint teacher-forced score - fp64 %s" % ["%+.4f" % e for e in errs]])


def test_score_hypotheses_joint_at_config5_shape_vs_fp64():
    """Joint teacher-forced scores at the benchmarked decode shape (6+6 layers, d 256, V 4337, 32 utterances of 500..1000
    frames, 25..50 tokens ending in EOS) against (1 - w) x the fp64 oracle's attention score + w x -ctc_loss over fp64 CTC
    log-probabilities of the oracle encoder; the bf16 reference (the same arithmetic under autocast) is the noise floor."""
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import synthetic
    from transformer.Decode import Decode
    cfg = C5
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(cfg))
    U.init_parameters(model)
    wts = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.eval().cuda()
    head = _head(cfg["vocab_size"], cfg["d_model"], 4.0, 2, "cuda")
    x, _, in_len, tgt_len, _ = synthetic.make_batch(32, 1000, 50, cfg["feature_dim"], cfg["vocab_size"], seed=0, t_min=500, l_min=25)
    g = torch.Generator().manual_seed(11)
    hyps = [torch.randint(4, cfg["vocab_size"], (int(n) - 1,), generator=g).tolist() + [bo.EOS] for n in tgt_len]
    w = 0.3
    xg = x.cuda()
    dec = Decode(U.AttrDict(beam_size=10, n_best=1, max_steps=50), "cuda", model=model, ctc_head=head)
    got = dec.score_hypotheses((xg, in_len), hyps, ctc_weight=w).double().cpu()
    L = max(len(h) for h in hyps)
    prefix = torch.zeros(32, L, dtype=torch.long)
    fed = torch.zeros(32, L, dtype=torch.long)
    for b, h in enumerate(hyps):
        prefix[b, :len(h)] = torch.tensor([bo.BOS] + h[:-1])
        fed[b, :len(h)] = torch.tensor(h)
    lens = torch.tensor([len(h) for h in hyps])
    live = (torch.arange(L).view(1, -1) < lens.view(-1, 1)).cuda()
    labels = torch.zeros(32, L - 1, dtype=torch.long)
    for b, h in enumerate(hyps):
        labels[b, :len(h) - 1] = torch.tensor(h[:-1])

    def score(p, xin, hw, hb):
        enc, _ = orc.encoder(p, xin, in_len, cfg["n_heads"])
        out, _, _ = orc.decoder(p, prefix.cuda(), lens, in_len, enc, cfg["n_heads"])
        lp = torch.log_softmax(torch.nn.functional.linear(out, p["tgt_word_proj.weight"]).double(), -1)
        att = (lp.gather(2, fed.cuda().unsqueeze(2)).squeeze(2) * live).sum(1).cpu()
        clp = torch.log_softmax(torch.nn.functional.linear(enc, hw, hb).double(), -1).cpu()
        nll = torch.nn.functional.ctc_loss(clp.transpose(0, 1), labels, in_len, lens - 1, blank=BLANK, reduction="none")
        return (1 - w) * att - w * nll

    hw, hb = head.ctc_proj.weight.detach(), head.ctc_proj.bias.detach()
    with torch.no_grad():
        truth = score({k: v.double().cuda() for k, v in wts.items()}, xg.double(), hw.double(), hb.double())
        with torch.autocast("cuda", dtype=torch.bfloat16):
            floor = score({k: v.float().cuda() for k, v in wts.items()}, xg.float(), hw.float(), hb.float())
    err, ferr = got - truth, floor - truth
    rms = lambda v: float((v * v).mean().sqrt())
    report = ["# joint (w 0.3) Decode.score_hypotheses at B = 32, T <= 1000, V = 4337 vs fp64",
              "scores %.1f .. %.1f   product error: rms %.4f max %.4f   reference under bf16 autocast: rms %.4f max %.4f"
              % (float(truth.min()), float(truth.max()), rms(err), float(err.abs().max()), rms(ferr), float(ferr.abs().max()))]
    _report("joint_score_parity.txt", report)
    assert torch.isfinite(got).all(), report
    assert float(err.abs().max()) < max(0.1, 3.5 * rms(ferr)), report
    assert rms(err) <= max(0.08, 2.0 * rms(ferr)), report


def _joint_search_fp64(p, head, x, in_len, beam, K, w, max_steps):
    """fp64 joint search: oracle/beam_oracle's Beam driven with the joint increments (top-K attention pre-beam, CTC prefix
    increments of the fp64 restatement, frozen after EOS)."""
    bsz = x.shape[0]
    enc, _ = orc.encoder(p, x[:, :int(in_len.max())], in_len, 4)
    ctc_lp = _ctc_lp64(p, head, x, in_len, 4)
    beams = [bo.Beam(beam) for _ in range(bsz)]
    states = [[ref.empty_state(ctc_lp[b, :int(in_len[b])].numpy(), BLANK) + (False,)] * beam for b in range(bsz)]
    for step in range(max_steps):
        active = [b for b in range(bsz) if not beams[b].done]
        if not active:
            break
        prefixes = torch.cat([beams[b].current_prefixes() for b in active], 0)
        idx = torch.tensor(active).repeat_interleave(beam)
        tgt_len = torch.full((prefixes.shape[0],), step + 1, dtype=torch.long)
        t_act = int(in_len[idx].max())
        dec, _, _ = orc.decoder(p, prefixes, tgt_len, in_len[idx], enc[idx][:, :t_act], 4)
        lp = torch.log_softmax(torch.nn.functional.linear(dec[:, -1], p["tgt_word_proj.weight"]), -1).view(len(active), beam, -1)
        for i, b in enumerate(active):
            xb = ctc_lp[b, :int(in_len[b])].numpy()
            word = torch.full_like(lp[i], float("-inf"))
            new = {}
            for s in range(beam):
                gn, gb, psi, last, fz = states[b][s]
                v, ids = lp[i, s].topk(K)
                for c, a in zip(ids.tolist(), v.tolist()):
                    if fz:
                        d, nst = 0.0, states[b][s]
                    else:
                        ph, ns = ref.extend(xb, (gn, gb, psi, last), c, BLANK, bo.EOS)
                        d = ph - psi if ph != -np.inf else -np.inf
                        nst = (ns + (False,)) if ns is not None else (gn, gb, ph, c, True)
                    word[s, c] = (1 - w) * a + w * d
                    new[(s, c)] = nst
            beams[b].advance(word)
            dead = (None, None, float("-inf"), -1, True)        # (a -inf non-candidate: only when fewer than beam are finite)
            states[b] = [new.get((int(o), int(c)), dead) for o, c in zip(beams[b].prev_ks[-1], beams[b].next_ys[-1])]
    out_h, out_s = [], []
    for b in range(bsz):
        sc, order = beams[b].sort_scores()
        out_s.append(sc)
        out_h.append([beams[b].get_hypothesis(int(k)) for k in order])
    return out_h, out_s, ctc_lp


def test_joint_search_parity_small_model():
    """Joint search (w 0.3, beam 4) on the small decode model with a peaky CTC head: every returned hypothesis's reported score
    equals its fp64 joint teacher-forced score within the noise, the best is at least as good as the fp64 joint search's best
    (oracle Beam driven with the joint increments), and graph-replayed and eager runs give identical results."""
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    p, model = _small("cuda")
    head = _head(30, 128, 8.0, 1, "cuda")
    batch = orc.synthetic_batch(5, 80, 10, 80, 30, seed=2, t_min=30, l_min=5)
    x, in_len = batch["x"], batch["in_len"]
    w, beam, steps = 0.3, 4, 16
    runs = []
    for ug in (True, False):
        dec = Decode(AttrDict(dict(beam_size=beam, n_best=2, max_steps=steps, use_graph=ug, ctc_weight=w)), "cuda", model=model,
                     ctc_head=head)
        runs.append(dec.decode_batch((x, in_len)))
        if ug:
            runs.append(dec.decode_batch((x, in_len)))     # the second call captures before its step 0
    (h, s) = runs[0]
    for hh, ss in runs[1:]:
        assert hh == h and all(torch.equal(a, b) for a, b in zip(ss, s))
    ref_h, ref_s, ctc_lp = _joint_search_fp64(p, head, x.double(), in_len, beam, 6, w, steps)
    tol = 0.16
    errs = []
    for b in range(x.shape[0]):
        for k in range(2):
            att = bo.score_hypothesis(p, x[b:b + 1].double(), in_len[b:b + 1], 4, h[b][k])
            truth = _joint_truth(att, ctc_lp[b], in_len[b], h[b][k], w)
            if h[b][k][-1] != bo.EOS and bo.EOS in h[b][k]:
                continue                                     # (extended past an EOS below the top: frozen CTC part)
            errs.append(float(s[b][k]) - truth)
            assert abs(float(s[b][k]) - truth) <= max(tol, 5e-2 * abs(truth)), (b, k, h[b][k], float(s[b][k]), truth)
        assert float(s[b][0]) >= float(ref_s[b][0]) - max(tol, 5e-2 * abs(float(ref_s[b][0]))), (b, h[b][0], ref_h[b][0])
    assert len(errs) >= 5
    _report("joint_score_parity.txt", ["joint search parity, small model, w 0.3 beam 4: reported - fp64 %s; best hyps %s vs fp64 %s"
                                       % (["%+.4f" % e for e in errs], [hh[0] for hh in h], [hh[0] for hh in ref_h])])


def test_joint_decode_at_config5_shape_graph_replay():
    """The benchmarked decode shape (seed-0 batch of st_amd.synthetic, 6+6 layers, d 256, V 4337, beam 10) joint-decoded with a
    random head under graph replay: every score finite, hypotheses of the step budget."""
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import synthetic
    from transformer.Decode import Decode
    cfg = C5
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(cfg))
    U.init_parameters(model)
    model = model.eval().cuda()
    head = _head(cfg["vocab_size"], cfg["d_model"], 1.0, 3, "cuda")
    x, _, in_len, _, _ = synthetic.make_batch(32, 1000, 50, cfg["feature_dim"], cfg["vocab_size"], seed=0, t_min=500, l_min=25)
    dec = Decode(U.AttrDict(beam_size=10, n_best=2, max_steps=20, ctc_weight=0.3), "cuda", model=model, ctc_head=head)
    assert dec.use_graph
    hyps, scores = dec.decode_batch((x.cuda(), in_len))
    assert len(hyps) == 32
    for b in range(32):
        assert torch.isfinite(scores[b]).all(), (b, scores[b])
        assert 1 <= len(hyps[b][0]) <= 20


def test_ctc_greedy_matches_host_argmax_collapse():
    from st_amd import ctc_decode
    from st_amd.arena import arena_of
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    p, model = _small("cuda")
    head = _head(30, 128, 8.0, 1, "cuda")
    batch = orc.synthetic_batch(5, 80, 10, 80, 30, seed=2, t_min=30, l_min=5)
    x, in_len = batch["x"], batch["in_len"]
    dec = Decode(AttrDict(dict(beam_size=4, n_best=1, max_steps=16)), "cuda", model=model, ctc_head=head)
    got = dec.ctc_greedy((x, in_len))
    with torch.no_grad(), arena_of(model).scope():
        enc, _ = model.encoder.forward_rows(x.cuda()[:, :int(in_len.max())], in_len)
        logits = ctc_decode.head_logits(head, enc)[:, :30].cpu()
    best = logits.argmax(-1).tolist()
    o, n_labels = 0, 0
    for b, T in enumerate(in_len.tolist()):
        want, prev = [], None
        for k in best[o:o + T]:
            if k != prev and k != BLANK:
                want.append(k)
            prev = k
        o += T
        assert got[b] == want, (b, got[b], want)
        n_labels += len(want)
    assert n_labels > 0

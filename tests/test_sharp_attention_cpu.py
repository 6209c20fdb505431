"""The checks of tests/test_sharp_attention_gpu.py, run here on the emulation (tests/_sharp_attn.py with a CPU backend): every
floor is below 1e-2, so 1.25 x floor is never looser than the tolerances the other attention tests use; the unmodified emulation
in fp32 passes every case; the fp64 reference agrees with the dense one on a padded case; and each defect the checks are there
for - an operand rounded a second time, one-term P, one wrong row, a causal mask off by one, the dQ scale of the other key form -
is reported when it is injected through a backend."""
import math
import types

import pytest
import torch

from tests import _attn_ref as ref
from tests import _emul as em
from tests import _sharp_attn as sh

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
CASES = sh.cases()
BY_ID = dict(CASES)


@pytest.mark.parametrize("kw", [kw for _, kw in CASES], ids=[i for i, _ in CASES])
def test_floor_is_below_the_bf16_bound_and_the_emulation_passes(kw):
    floor = sh.floors(kw)
    assert floor, "the case compares nothing"
    for nm, f in floor.items():
        assert 0 < f < sh.L_BF16, "%s: floor %.3e of %s is not below %.0e - choose other inputs" % (kw["name"], f, nm, sh.L_BF16)
    sh.run(kw, sh.CPU)


def test_case_list_reaches_every_family():
    """What the issue lists: each family at s = 1, 2, 3 and once with dropout; plain AND pre-scaled keys at the streams' shapes; the
    merged backward with and without its key split; lengths of at most 300."""
    fams = {}
    for cid, kw in CASES:
        fams.setdefault(kw["family"], []).append(kw)
        assert max(kw["k_lens"]) <= 300
    assert set(fams) == {"general", "psplit", "ks2", "xs", "fwd64", "bwd64", "two-launch"}
    for fam, kws in fams.items():
        assert {kw["s"] for kw in kws} == {1, 2, 3}, fam
        assert any(kw.get("p", 0) > 0 and kw["s"] == 3 for kw in kws), fam
    assert {kw.get("prescaled", False) for kw in fams["bwd64"]} == {False, True}
    assert {kw.get("prescaled", False) for kw in fams["fwd64"]} == {False, True}
    assert {kw.get("split", True) for kw in fams["ks2"]} == {False, True}
    assert {kw["dk"] for kw in fams["ks2"]} == {32, 64, 128} and {kw["dk"] for kw in fams["general"]} == {32, 64, 128}
    assert {kw.get("packed", True) for kw in fams["general"]} == {False, True} == {kw.get("packed", True) for kw in fams["bwd64"]}


@pytest.mark.parametrize("causal,p", [(False, 0.0), (True, 0.0), (False, sh.P_DROP)])
def test_packed_reference_agrees_with_the_dense_reference(causal, p):
    """A padded layout is a dense problem whose mask hides the keys past k_len (causal: and past the query) and kills the query
    rows past q_len: two references written from two headers must agree to fp64 rounding on the utterances' rows."""
    B, H, dk, q_len, k_len = 2, 3, 32, ([70, 33] if not causal else [70, 41]), [70, 41]
    Lq, Lk, d, scale = max(q_len), max(k_len), H * dk, 1 / math.sqrt(dk)
    gen = torch.Generator().manual_seed(5)
    Q, dO = ((torch.randn(B * Lq, d, generator=gen) * s).to(BF16) for s in (1.5, 0.5))
    K, V = ((torch.randn(B * Lk, d, generator=gen) * s).to(BF16) for s in (1.5, 0.7))
    mask = torch.zeros(B, Lq, Lk, dtype=torch.uint8)
    for b in range(B):
        mask[b, :, k_len[b]:] = 1
        mask[b, q_len[b]:, :] = 1
        if causal:
            mask[b] |= torch.ones(Lq, Lk, dtype=torch.uint8).triu(1)
    keep_d = keep_p = None
    ks = 1.0
    if p > 0:
        de = em.Drop(torch.tensor([99], dtype=I32), 5, p)
        keep_d = torch.stack([em.keep_qk(de, bh, Lq, Lk) for bh in range(B * H)])
        keep_p = [keep_d[b * H + h][:q_len[b], :k_len[b]] for b in range(B) for h in range(H)]
        ks = de.scale
    O, lse, _, delta, dQ, dK, dV = ref.dense_attention(Q, K, V, mask, dO, B, H, Lq, Lk, scale, keep=keep_d, keep_scale=ks)
    q_off, k_off = [b * Lq for b in range(B)], [b * Lk for b in range(B)]
    got = ref.packed_attention(Q, K, V, dO, q_off, q_len, k_off, k_len, H, causal, scale, keep=keep_p, keep_scale=ks)
    qr, kr = sh._utt_rows(q_off, q_len, B * Lq), sh._utt_rows(k_off, k_len, B * Lk)
    for nm, a, b_, rows in zip(("O", "lse", "delta", "dQ", "dK", "dV"), got, (O, lse / math.log(2.0), delta, dQ, dK, dV), (qr, qr, qr, qr, kr, kr)):
        if a.dim() == 1:
            a, b_ = a.view(H, -1)[:, rows], b_.view(H, -1)[:, rows]
        else:
            assert bool((a[~rows] == 0).all()), nm
            a, b_ = a[rows], b_[rows]
        assert float((a - b_).abs().max()) <= 1e-12 * max(1.0, float(b_.abs().max())), nm


def test_prescaled_reference_is_the_plain_one_on_the_unscaled_keys():
    """k_prescaled: K~ / (scale log2 e) is the key; K~ chosen as exact multiples, both calls see the same key up to fp64 rounding."""
    H, dk, lens = 2, 32, [40, 17]
    d, scale = H * dk, 1 / math.sqrt(dk)
    gen = torch.Generator().manual_seed(6)
    Q, V, dO = ((torch.randn(sum(lens), d, generator=gen) * s).to(BF16) for s in (2.0, 0.7, 0.5))
    Kt = (torch.randn(sum(lens), d, generator=gen) * 0.4).to(BF16)
    off = [0, lens[0]]
    a = ref.packed_attention(Q, Kt, V, dO, off, lens, off, lens, H, True, scale, k_prescaled=True)
    # the same problem without the flag: scores ln 2 (q . K~) = scale' (q . K~) with scale' = ln 2; dK of the unscaled key = dK' scale log2 e
    b = ref.packed_attention(Q, Kt, V, dO, off, lens, off, lens, H, True, math.log(2.0))
    for nm, x, y in zip(("O", "lse", "delta", "dQ", "dK", "dV"), a, b):
        y = y * (scale * math.log2(math.e)) if nm == "dK" else y
        assert float((x - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max())), nm


# ---- defects, injected through a backend -------------------------------------------------------------------------------------------------
def _fwd(Q, K, V, O, lse, q_off, q_len, k_off, k_len, n_head, max_q, causal, scale, work=None, drop=None, max_k=0, ores=None,
         k_prescaled=False, dtype=F32, diag=1):
    """A forward with the general kernels' rounding points (P to bf16 before P V, O once) whose causal mask starts ``diag`` past the
    query (1: correct)."""
    rows, dk = Q.shape[0], Q.shape[1] // n_head
    c2 = 1.0 if k_prescaled else scale * sh.K_LOG2_SCALE
    for b in range(len(q_len)):
        qs, ks = slice(int(q_off[b]), int(q_off[b]) + int(q_len[b])), slice(int(k_off[b]), int(k_off[b]) + int(k_len[b]))
        for h in range(n_head):
            cs = slice(h * dk, (h + 1) * dk)
            s2 = Q[qs, cs].to(dtype) @ K[ks, cs].to(dtype).t() * c2
            if causal:
                s2 = s2.masked_fill(torch.ones(s2.shape, dtype=torch.bool).triu(diag), float("-inf"))
            l2 = torch.logsumexp(s2 * math.log(2.0), -1) / math.log(2.0)
            O[qs, cs] = (torch.exp2(s2 - l2.unsqueeze(-1)).to(BF16).to(dtype) @ V[ks, cs].to(dtype)).to(BF16)
            lse.view(n_head, rows)[h, qs] = l2.to(lse.dtype)


def _bwd(Q, K, V, O, dO, lse, delta, dQ, dK, dV, q_off, q_len, k_off, k_len, n_head, max_q, max_k, causal, scale, parts=3, work_q=None,
         work_k=None, drop=None, k_prescaled=False, dtype=F32, reround=False, swap_dq=False, diag=1):
    """The backward as its two bodies compute it (csrc/st_attn_common.cuh, AttnArgs: c2, dq_scale): each exponentiates its own
    scores q . k c2 in the log2 domain; dS to bf16, dQ = dq_scale dS K, dK = scale dS^T Q, dV = bf16(Pd)^T dO.
    reround: the operand held in registers is multiplied by c2 and rounded to bf16 again - K in the dQ body, Q in the dK / dV body
    (what the backward streams do to plain keys).  swap_dq: dq_scale of the other key form.  diag: as _fwd."""
    rows, dk = Q.shape[0], Q.shape[1] // n_head
    c2 = 1.0 if k_prescaled else scale * sh.K_LOG2_SCALE
    dq_scale = (math.log(2.0) if k_prescaled else scale) if not swap_dq else (scale if k_prescaled else math.log(2.0))
    rr = lambda t: (t * c2).to(BF16).to(dtype) if reround and c2 != 1.0 else t * c2
    for b in range(len(q_len)):
        qs, ks = slice(int(q_off[b]), int(q_off[b]) + int(q_len[b])), slice(int(k_off[b]), int(k_off[b]) + int(k_len[b]))
        for h in range(n_head):
            cs = slice(h * dk, (h + 1) * dk)
            q, k, v, do = Q[qs, cs].to(dtype), K[ks, cs].to(dtype), V[ks, cs].to(dtype), dO[qs, cs].to(dtype)
            if O is not None:
                delta.view(n_head, rows)[h, qs] = (do * O[qs, cs].to(dtype)).sum(-1)
            dl = delta.view(n_head, rows)[h, qs].to(dtype).unsqueeze(-1)
            keep = em.keep_qk(drop, b * n_head + h, q.shape[0], k.shape[0]) * drop.scale if em._on(drop) else 1.0
            dp = do @ v.t() * keep

            def body(s2):
                if causal:
                    s2 = s2.masked_fill(torch.ones(s2.shape, dtype=torch.bool).triu(diag), float("-inf"))
                p = torch.exp2(s2 - lse.view(n_head, rows)[h, qs].to(dtype).unsqueeze(-1))
                return p, (p * (dp - dl)).to(BF16).to(dtype)

            _, ds = body(q @ rr(k).t())
            dQ[qs, cs] = (ds @ k * dq_scale).to(BF16)
            p, ds = body(rr(q) @ k.t())
            dK[ks, cs] = (ds.t() @ q * scale).to(BF16)
            dV[ks, cs] = ((p * keep).to(BF16).to(dtype).t() @ do).to(BF16)


def _backend(fwd=em.attn_fwd, bwd=em.attn_bwd, dtype=F32):
    return sh.Backend(types.SimpleNamespace(attn_fwd=fwd, attn_bwd=bwd), "cpu", em.Drop, dtype=dtype)


def _with(fn, **fixed):
    return lambda *a, **kw: fn(*a, **dict(kw, **fixed))


def _reported(cid, be, match):
    with pytest.raises(AssertionError, match=match):
        sh.run(BY_ID[cid], be)


@pytest.mark.parametrize("cid", [i for i, kw in CASES if kw.get("bwd", True)])
def test_the_two_body_backward_without_a_defect_passes(cid):
    """The harness of the injections below is itself a correct backward: with no defect switched on it passes every case."""
    sh.run(BY_ID[cid], _backend(bwd=_bwd))


@pytest.mark.parametrize("cid", ["general-dk64-causal-s3", "general-dk32-causal-s1", "psplit-dk64-causal-s2"])
def test_the_forward_of_the_injections_without_a_defect_passes(cid):
    sh.run(dict(BY_ID[cid], ores=False), _backend(fwd=_fwd, bwd=_bwd))


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", ["plain", "plain-padded"])
def test_reports_an_operand_rounded_a_second_time(name, s):
    """bf16(k c2) in the dQ pass, bf16(q c2) in the dK / dV pass - the backward streams on plain keys: beyond 1.25 x floor at
    s = 2 already, in every output."""
    _reported("bwd64-%s-s%d" % (name, s), _backend(bwd=_with(_bwd, reround=True)), "less accurate than its rounding points allow")
    c = sh.build(**BY_ID["bwd64-%s-s%d" % (name, s)])
    err = sh.errors(c, sh.outputs(c, sh.launch(c, _backend(bwd=_with(_bwd, reround=True)))))
    floor = sh.floors(BY_ID["bwd64-%s-s%d" % (name, s)])
    for nm in sh.OUT_BWD:
        assert err[nm] > 1.4 * floor[nm], (nm, err[nm] / floor[nm])


def test_an_operand_rounded_a_second_time_is_invisible_to_the_old_tolerances():
    """... and at N(0, 1)-sized scores (s = 1) it hides: why the cases at s = 2, 3 exist."""
    c = sh.build(**BY_ID["bwd64-plain-s1"])
    err = sh.errors(c, sh.outputs(c, sh.launch(c, _backend(bwd=_with(_bwd, reround=True)))))
    assert all(err[nm] < 2.5e-2 for nm in sh.OUT_BWD)


@pytest.mark.parametrize("cid", ["psplit-dk64-causal-s1", "psplit-dk64-causal-s3", "psplit-dk32-cross-s2", "xs-dk64-ores-s3"])
def test_reports_one_term_p(cid):
    """(the emulation forms P of two terms only when told at most 64 queries)"""
    one_term = lambda *a, **kw: em.attn_fwd(*a[:10], 65, *a[11:], **kw)
    _reported(cid, _backend(fwd=one_term), r"O\+Ores")


@pytest.mark.parametrize("cid,nm,row", [("general-dk128-s1", "dK", 199), ("bwd64-prescaled-s3", "dQ", 256), ("ks2-dk32-s2", "dV", 300),
                                        ("fwd64-plain-s2", "O", 257)])
def test_reports_one_wrong_row(cid, nm, row):
    def tamper(fn, pos):
        def run(*a, **kw):
            fn(*a, **kw)
            a[pos][row] = a[pos][row - 1]           # (the neighbour's values: an index off by one in a tail)
        return run
    be = _backend(fwd=tamper(em.attn_fwd, 3), bwd=em.attn_bwd) if nm == "O" else _backend(bwd=tamper(em.attn_bwd, dict(dQ=7, dK=8, dV=9)[nm]))
    _reported(cid, be, nm)


def test_reports_a_row_never_written_and_a_write_outside_the_utterances():
    def skip_row(*a, **kw):
        keep = a[9][5].clone()
        em.attn_bwd(*a, **kw)
        a[9][5] = keep
    _reported("general-dk64-s1", _backend(bwd=skip_row), "non-finite")

    def stray(*a, **kw):
        em.attn_bwd(*a, **kw)
        a[8][100] = 0                       # padded layout [128, 65]: row 100 of utterance 0 is live, row 128 + 100 belongs to nobody
        a[8][128 + 100] = 0
    _reported("general-dk64-padded-s1", _backend(bwd=stray), "must not write")


@pytest.mark.parametrize("cid", ["general-dk64-causal-s1", "general-dk32-causal-s3", "psplit-dk64-causal-s2"])
@pytest.mark.parametrize("where", ["fwd", "bwd"])
def test_reports_a_causal_mask_off_by_one(cid, where):
    kw = dict(BY_ID[cid], ores=False)
    be = _backend(fwd=_with(_fwd, diag=2), bwd=_bwd) if where == "fwd" else _backend(fwd=_fwd, bwd=_with(_bwd, diag=2))
    with pytest.raises(AssertionError):
        sh.run(kw, be)


@pytest.mark.parametrize("cid", ["bwd64-prescaled-s1", "bwd64-prescaled-padded-s3", "bwd64-plain-s2", "general-dk32-causal-s1"])
def test_reports_the_dq_scale_of_the_other_key_form(cid):
    """ln 2 belongs to sum dS K~, scale to sum dS K: swapped, dQ is off by the factor scale log2 e."""
    _reported(cid, _backend(bwd=_with(_bwd, swap_dq=True)), "dQ")


# ---- the per-GEMM path hands the streams pre-scaled keys -----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,L,grad,want_kpre", [(4, 130, True, True), (8, 130, True, False), (4, 128, True, False)])
def test_per_gemm_self_attention_prescales_keys_where_the_streams_serve_the_backward(H, L, grad, want_kpre, monkeypatch):
    """st_attn_bwd sends only pre-scaled keys to the backward streams.  MhaFn on the per-GEMM path, at row counts where the
    weight-stationary GEMM would serve the q | k | v projection (which leaves the keys plain): where a gradient is wanted, with 64-wide
    heads and more than 128 rows it takes st_gemm_kscale and tells st_attn_bwd so; otherwise st_gemm_ws and plain keys."""
    import transformer.Attention as A
    from st_amd import native as nv

    seen = dict(kscale=0, ws=0, kpre=[])
    with em.emulated_kernels():
        monkeypatch.setattr(nv, "ws_ok", lambda M, N, K: K == 256 and N % 256 == 0)          # (as if the row count were encoder-sized)

        def spy(name, key):
            f = getattr(nv, name)

            def g(*a, **kw):
                if key == "kpre":
                    seen["kpre"].append(bool(kw.get("k_prescaled", False)))
                else:
                    seen[key] += 1
                return f(*a, **kw)
            monkeypatch.setattr(nv, name, g)
        spy("gemm_kscale", "kscale"), spy("gemm_ws", "ws"), spy("attn_bwd", "kpre")
        torch.manual_seed(1)
        mha = A.MultiHeadAttention(H, 256, 256 // H, 256 // H, dropout=0.0).eval()
        x = torch.randn(2, L, 256).requires_grad_(grad)
        out, _ = mha(x, x, x)
        if grad:
            out.sum().backward()
        monkeypatch.undo()
    assert (seen["kscale"], seen["ws"]) == ((1, 0) if want_kpre else (0, 1)), seen
    assert seen["kpre"] == ([want_kpre] if grad else []), seen

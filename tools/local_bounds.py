"""Where the local bounds of tests/test_kernels_gpu.py come from (tests/LOCAL_BOUNDS.md): on the CPU, every emulation of
tests/_emul.py evaluated with fp32 and with fp64 accumulation - same bf16 rounding points - over the kernel tests' own cases;
the largest per-row / per-column / per-element ratio of tests/_local.py per family and output; likewise the slow-path attention
kernels over the cases of tests/test_slow_attention_gpu.py (families "dense" and "probs") and the fast attention kernels at sharp
scores over the cases of tests/test_sharp_attention_gpu.py (family "sharp"); the LayerNorm statistic off centre, at tiny spread and on
constant rows over the cases of tests/test_ln_stats_gpu.py (family "ln_stats"); the LayerNorm-backward kernels and backward chains
against fp64 over the cases of tests/test_lnbwd_fp64_gpu.py (family "ln_bwd": two fp32 evaluations, the common-mode strength of the
fused kernels, what leaving Ores out moves delta by); the vocabulary log-sum-exp restated in fp32 in two orders over the row families of
tests/_lse_cases.py (family "lse": the bounds L_LSE and P_REL of tests/test_lse_fp64_gpu.py).  No kernel runs here.

    python tools/local_bounds.py            # prints one line per family / output
    python tools/local_bounds.py lse        # the "lse" family alone, with its table
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-tranformer-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from st_amd import chains, native as nv          # noqa: E402
from tests import _emul as em                     # noqa: E402
from tests import _ln_stats as ls                 # noqa: E402
from tests import _lnbwd_cases as lb              # noqa: E402
from tests import _lnbwd_ref as lref              # noqa: E402
from tests import _lse_cases as lse_cases         # noqa: E402
from tests import _sharp_attn as sh               # noqa: E402
from tests import _slow_attn as sa                # noqa: E402
from tests import test_kernels_gpu as tk          # noqa: E402
from tests._local import local_figures            # noqa: E402

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
g = tk.g
worst = {}


def note(family, name, a, b, rows=None):
    if rows is not None:
        a, b = (a.view(-1, rows.numel())[:, rows].reshape(-1), b.view(-1, rows.numel())[:, rows].reshape(-1)) if a.dim() == 1 else (a[rows], b[rows])
    for axis, ratio in local_figures(a, b):
        if ratio.numel():
            key = (family, name, axis)
            worst[key] = max(worst.get(key, 0.0), float(ratio.max()))


def attention(cases, family, drop=None, prescaled=False):
    for case in cases:
        c = tk._attn_case(*case, seed=11)
        K = (c["K"].float() * (c["scale"] * nv.K_LOG2_SCALE)).to(BF16) if prescaled else c["K"]
        meta = [c[k] for k in ("q_off", "q_len", "k_off", "k_len")]
        res = {}
        for dt in (F32, F64):
            O, lse = torch.zeros(c["Mq"], c["d"], dtype=BF16), torch.zeros(c["H"] * c["Mq"], dtype=F32)
            em.attn_fwd(c["Q"], K, c["V"], O, lse, *meta, c["H"], c["max_q"], c["causal"], c["scale"], drop=drop, max_k=c["max_k"],
                        k_prescaled=prescaled, dtype=dt)
            delta = torch.zeros_like(lse)
            dQ, dK, dV = torch.zeros(c["Mq"], c["d"], dtype=BF16), torch.zeros(c["Mk"], c["d"], dtype=BF16), torch.zeros(c["Mk"], c["d"], dtype=BF16)
            em.attn_bwd(c["Q"], K, c["V"], O, c["dO"], lse, delta, dQ, dK, dV, *meta, c["H"], c["max_q"], c["max_k"], c["causal"], c["scale"],
                        drop=drop, k_prescaled=prescaled, dtype=dt)
            res[dt] = dict(O=O, lse=lse, delta=delta, dQ=dQ, dK=dK, dV=dV)
        for nm in res[F32]:
            if nm != "delta":
                note(family, nm, res[F32][nm], res[F64][nm], rows=tk._attn_rows(c, nm))
        # delta is a function of the backward's inputs dO and O: the fp32 sum against the fp64 one over the SAME O
        note(family, "delta", res[F32]["delta"], tk._delta_of(c["dO"], res[F32]["O"], c["H"]).float(), rows=tk._attn_rows(c, "delta"))


def ln_family():
    for M, N in [(100, 128), (1000, 256), (333, 512), (5000, 256)]:
        for masked in (False, True):
            dy, xhat = g(M, N, seed=1), g(M, N, seed=2)
            rstd, gamma = g(M, seed=3, dtype=F32).abs() + 0.5, 1 + 0.2 * g(N, seed=4, dtype=F32)
            mask = g(M, N, seed=5) if masked else None
            res = {}
            for dt in (F32, F64):
                dx, acc = torch.zeros(M, N, dtype=BF16), [torch.ones(N, dtype=F32) for _ in range(3)]
                em.ln_bwd(dy, xhat, rstd, gamma, dx, *acc, mask=mask, dtype=dt)
                res[dt] = [dx] + acc
            for a, b, nm in zip(res[F32], res[F64], ("dx", "dgamma", "dbeta", "dbias")):
                note("ln_bwd", nm, a, b)
    for M, N, K, with_aux in [(300, 128, 128, True), (1000, 256, 1024, True), (130, 256, 768, False), (70, 512, 512, True), (999, 256, 256, True),
                              (16500, 256, 768, True), (8250, 512, 512, True)]:
        dY, W = g(M, K, seed=1), g(K, N, seed=2, scale=K ** -0.5)
        aux = g(M, N, seed=3) if with_aux else None
        xhat, rstd, gamma = g(M, N, seed=4), g(M, seed=5, dtype=F32).abs() + 0.5, 1 + 0.2 * g(N, seed=6, dtype=F32)
        res = {}
        for dt in (F32, F64):
            dx, acc = torch.zeros(M, N, dtype=BF16), [torch.ones(N, dtype=F32) for _ in range(3)]
            em.gemm_lnbwd(dY, W, aux, xhat, rstd, gamma, dx, *acc, dtype=dt, dbias_rounded=True)
            res[dt] = [dx] + acc
        for a, b, nm in zip(res[F32], res[F64], ("dx", "dgamma", "dbeta", "dbias")):
            note("gemm_lnbwd", nm, a, b)
    for M, N, K in [(300, 128, 128), (1206, 256, 1024), (500, 256, 80), (16500, 256, 544), (8230, 512, 1024)]:
        X, W = g(M, K, seed=1), g(N, K, seed=2, scale=K ** -0.5)
        b, gamma, beta, res_ = g(N, seed=3, dtype=F32), 1 + 0.2 * g(N, seed=4, dtype=F32), 0.2 * g(N, seed=5, dtype=F32), g(M, N, seed=6)
        out = {}
        for dt in (F32, F64):
            o, xh, rs = torch.zeros(M, N, dtype=BF16), torch.zeros(M, N, dtype=BF16), torch.zeros(M, dtype=F32)
            em.gemm_ln(X, W, b, res_, gamma, beta, o, xh, rs, dtype=dt)
            out[dt] = dict(out=o, xhat=xh, rstd=rs)
        for nm in out[F32]:
            note("gemm_ln", nm, out[F32][nm], out[F64][nm])


def chain_bwd():
    d, dff, nb = 256, 1024, 3
    wp, w1, w2, wo = g(768, d, seed=1, scale=d ** -0.5), g(dff, d, seed=2, scale=d ** -0.5), g(d, dff, seed=3, scale=dff ** -0.5), g(d, d, seed=4, scale=d ** -0.5)
    blocks = chains.t_blocks(chains.blocks_of(wp)) + chains.ffn_blocks_bwd(w1, w2) + chains.t_blocks(chains.blocks_of(wo))
    for M in (5, 1206, 24700):
        dP, G = g(M, 768, seed=5, scale=0.3), g(M, d, seed=6, scale=0.3)
        xa, xb = g(M, d, seed=8), g(M, d, seed=9)
        ra, rb = g(M, seed=10, dtype=F32).abs() + 0.5, g(M, seed=11, dtype=F32).abs() + 0.5
        ga, gb = g(d, seed=12, dtype=F32) * 0.2 + 1, g(d, seed=13, dtype=F32) * 0.2 + 1
        H = torch.relu(g(M, dff, seed=14))
        O, Ores = g(M, d, seed=15), g(M, d, seed=16, scale=2.0 ** -9)
        res = {}
        for dt in (F32, F64):
            Z = lambda *s, dt_=BF16: torch.zeros(*s, dtype=dt_)
            o = dict(ds_a=Z(M, d), dga=Z(d, dt_=F32) + 1, dba=Z(d, dt_=F32) + 2, dbia=Z(d, dt_=F32) + 3, dH=Z(M, dff), ds_b=Z(M, d),
                     dgb=Z(d, dt_=F32) - 1, dbb=Z(d, dt_=F32) - 2, dbib=Z(d, dt_=F32) - 3, dctx=Z(M, d), delta=Z(4 * M, dt_=F32))
            em.row_chain_bwd(chains.Chain(None, len(blocks), blocks), M,
                             head=(nb, dP, G, xa, ra, ga, None, o["ds_a"], o["dga"], o["dba"], o["dbia"]),
                             ffn=(dff, em.relu_bits_from(H), 1.0, o["dH"], xb, rb, gb, o["ds_b"], o["dgb"], o["dbb"], o["dbib"]),
                             tail=(O, Ores, o["dctx"], o["delta"]), dtype=dt, dbias_rounded=True)
            res[dt] = o
        for nm in res[F32]:
            note("row_chain_bwd", nm, res[F32][nm], res[F64][nm])


def probs_and_ctc():
    """st_attn_probs' fp32 maps (the emulation's softmax in fp32 against fp64) and st_ctc_dlogits' bf16 gradient."""
    for case in tk.PRESCALED_CASES:
        c = tk._attn_case(*case, seed=31)
        meta = [c[k] for k in ("q_off", "q_len", "k_off", "k_len")]
        P = em.attn_probs(c["Q"], c["K"], *meta, c["H"], c["max_q"], c["max_k"], c["causal"], c["scale"])
        P64 = em.attn_probs(c["Q"], c["K"], *meta, c["H"], c["max_q"], c["max_k"], c["causal"], c["scale"], dtype=F64)
        note("attn_probs", "P", P, P64)
    from st_amd.functional import Rows
    for V, lens, C in [(23, [30, 17, 25], 8), (4337, [300, 211], 41), (1000, [64, 1, 33, 128], 12)]:
        gen = torch.Generator().manual_seed(V)
        lens_t = torch.tensor(lens)
        B, T, R = len(lens), int(max(lens)), int(sum(lens))
        v_pad = (V + 1 + 7) // 8 * 8
        logits = torch.randn(R, v_pad, generator=gen) * 3
        logits[:, V:] = -1e30
        cols = torch.randint(0, V, (B, C), generator=gen, dtype=torch.int32)
        scat = cols.clone()
        scat[:, C - 1] = -1
        rowmap = Rows.packed(lens_t, "cpu").scatter_index(T)
        roww = torch.rand(B, generator=gen) * 0.1
        gsmall = torch.randn(B, T, C, generator=gen) * 0.05
        lse, lp = torch.zeros(R), torch.zeros(B, T, C)
        em.ctc_gather(logits, rowmap, T, cols, lse, lp, V=V)
        out = {}
        for dt in (F32, F64):
            out[dt] = torch.zeros(R, v_pad, dtype=BF16)
            em.ctc_dlogits(logits, lse, rowmap, T, roww, scat, gsmall, torch.tensor([0.7]), out[dt], V=V, dtype=dt)
        note("ctc_dlogits", "dlogits", out[F32][:, :V], out[F64][:, :V])


def dense():
    """The slow-path attention kernels over the cases of tests/test_slow_attention_gpu.py (tests/_slow_attn.py).  They have no
    bf16 rounding point between their inputs and their outputs, so the fp32 outputs lse / delta / P follow the rule (the emulation
    in fp32 against fp64); the bf16 outputs are single-rounding outputs (L_BF16) - their row "(bf16 vs fp64)" is the once-rounded
    emulation against the UNROUNDED fp64 reference of tests/_attn_ref.py: the room the rounding alone takes of the bound."""
    for _, kw in sa.dense_cases() + [(n, k) for n, k, _, _ in sa.lds_cases()]:
        c = sa.build(**kw)
        drop = sa.CPU.drop(c)
        res = {}
        for dt in (F32, F64):
            n = c.H * c.B * c.Lq
            r = dict(O=torch.zeros(c.B * c.Lq, c.d, dtype=BF16), lse=torch.zeros(n, dtype=dt), delta=torch.zeros(n, dtype=dt),
                     dQ=torch.zeros(c.B * c.Lq, c.d, dtype=BF16), dK=torch.zeros(c.B * c.Lk, c.d, dtype=BF16),
                     dV=torch.zeros(c.B * c.Lk, c.d, dtype=BF16))
            r["P"] = em.attn_dense_fwd(c.Q, c.K, c.V, c.mask, r["O"], r["lse"], c.B, c.H, c.Lq, c.Lk, c.scale, drop=drop, want_probs=True, dtype=dt)
            if c.dO is not None:
                em.attn_dense_bwd(c.Q, c.K, c.V, c.mask, c.dO, r["lse"], r["delta"], r["dQ"], r["dK"], r["dV"], c.B, c.H, c.Lq, c.Lk, c.scale,
                                  drop=drop, dtype=dt)
            res[dt] = r
        live = torch.isfinite(res[F64]["lse"])                        # (a dead row's lse is +inf on both sides: compared exactly)
        note("dense", "lse", res[F32]["lse"][live], res[F64]["lse"][live])
        note("dense", "P", res[F32]["P"], res[F64]["P"])
        if c.dO is not None:
            note("dense", "delta", res[F32]["delta"], res[F64]["delta"])
        for nm in ("O", "dQ", "dK", "dV"):
            if c.ref[nm] is not None:
                note("dense (bf16 vs fp64)", nm, res[F32][nm], c.ref[nm])


def sharp():
    """The fast attention kernels over the cases of tests/test_sharp_attention_gpu.py (tests/_sharp_attn.py): the rule - the emulation
    in fp32 against fp64, same rounding points - per output, and "(bf16 vs fp64)": the fp32 emulation against the UNROUNDED fp64
    reference the test compares with, row by row - the room the kernels' own rounding points take of the bound in force."""
    for _, kw in sh.cases():
        c = sh.build(**kw)
        out = {be: sh.outputs(c, sh.launch(c, be)) for be in (sh.CPU, sh.CPU64)}
        fam = "sharp, dropout" if c.p > 0 else "sharp"
        for nm in out[sh.CPU]:
            if nm == "Ores":
                continue
            rows = c.rows[sh.side(nm)]
            a, b = out[sh.CPU][nm], out[sh.CPU64][nm]
            if nm == "delta":          # a function of the backward's inputs: the fp32 sum against the fp64 one over the same O
                b = c.delta_of_O
            note(fam, nm, a, b, rows=rows)
            if nm in c.ref and nm not in ("lse", "delta"):
                note(fam + " (bf16 vs fp64)", nm, a, c.ref[nm], rows=rows)
            elif nm == "O+Ores":
                note(fam + " (bf16 vs fp64)", nm, a, c.ref["O"], rows=rows)
            elif nm == "lse":
                note(fam + " (bf16 vs fp64)", nm, a, c.ref[nm].float(), rows=rows)


def ln_stats():
    """The LayerNorm kernels over the cases of tests/test_ln_stats_gpu.py (tests/_ln_stats.py), per row family: the fp32 emulation
    against the UNROUNDED fp64 reference of tests/_ln_ref.py - rstd as the worst |got / ref - 1| over all rows, implementations'
    shapes and both LayerNorms of a chain (the figure L_RSTD = 1e-4 leaves room above), xhat / out as the worst row: the room the
    one rounding takes of L_BF16."""
    import contextlib
    import io
    for _, kw in ls.cases():
        report = []
        with contextlib.redirect_stdout(io.StringIO()):        # (the checks print every figure)
            ls.run(kw, ls.CPU, report=report)
        for _, _, f, xh, o, _ in report:
            for nm, axis, v in (("rstd", "element", f), ("xhat", "row", xh), ("out", "row", o)):
                key = ("ln_stats %s" % kw["family"], nm, axis)
                worst[key] = max(worst.get(key, 0.0), v)


def ln_bwd_fp64():
    """The LayerNorm-backward family over the cases of tests/test_lnbwd_fp64_gpu.py (tests/_lnbwd_cases.py), against the plain fp64
    reference tests/_lnbwd_ref.py, by two fp32 evaluations: the emulation as it is (CPU) and with every column sum, delta's 64 products
    and the contraction (chunks of 32) accumulated serially (SERIAL).  Per kernel kind and output the larger figure - L_DELTA and
    L_COL are 3 x these, capped by the bounds in force; the matrices' rows are judged against their OWN norm.  Then the common-mode
    candidates of the fused kernels (worst row of any matrix output, to stay below L_BF16 / 3) and what leaving Ores out moves delta by
    (per case the worst and the median element; the smallest of each over the cases)."""
    import contextlib
    import io
    col = {"dga": "dgamma", "dgb": "dgamma", "dba": "dbeta", "dbb": "dbeta", "dbia": "dbias", "dbib": "dbias"}
    for be_name, be in (("CPU", lb.CPU), ("SERIAL", lb.SERIAL)):
        for _, kw in lb.cases():
            report = []
            with contextlib.redirect_stdout(io.StringIO()):
                lb.run(kw, be, report=report, asserted=False)
            kind = lb.IMPLS[kw["impl"]]["kind"]
            for _, nm, f, _ in report:
                for axis, v in f.items():
                    for key in (("ln_bwd fp64 %s" % kind, col.get(nm, nm), axis), ("ln_bwd fp64 %s %s %s" % (kind, kw["family"], be_name), col.get(nm, nm), axis)):
                        worst[key] = max(worst.get(key, 0.0), v)
    for cm in lb.CM_CANDIDATES:
        for be_name, be in (("CPU", lb.CPU), ("SERIAL", lb.SERIAL)):
            for _, kw in lb.cases():
                if kw["family"] != "common-mode" or lb.IMPLS[kw["impl"]]["kind"] == "ln_bwd":
                    continue
                c, report = lb.build(cm=cm, **kw), []
                with contextlib.redirect_stdout(io.StringIO()):
                    lb.verify(c, lb.launch(c, be), report=report, asserted=False)
                key = ("ln_bwd fp64 common-mode (%g, %g, %g)" % cm, "any", "row")
                worst[key] = max([worst.get(key, 0.0)] + [f["row"] for _, _, f, _ in report if "row" in f])
    lo_max, lo_med = float("inf"), float("inf")
    for _, kw in lb.cases():
        c = lb.build(**kw)
        if c.kind != "chain" or not c.has_tail:
            continue
        dctx = lb.launch(c, lb.CPU)["dctx"].view
        ratio = local_figures(lref.delta_of(dctx, c.O, None), lref.delta_of(dctx, c.O, c.Ores))[0][1]
        live = ratio[~c.dead.repeat(4)] if c.dead is not None else ratio
        lo_max, lo_med = min(lo_max, float(live.max())), min(lo_med, float(live.median()))
    worst[("ln_bwd fp64 delta without Ores (smallest over the cases)", "delta", "worst element")] = lo_max
    worst[("ln_bwd fp64 delta without Ores (smallest over the cases)", "delta", "median element")] = lo_med


def probs():
    """st_attn_probs over the cases of tests/test_slow_attention_gpu.py: the emulation's fp32 maps against the fp64 reference."""
    for kw in sa.probs_cases():
        c = sa.build_probs(**kw)
        ti = lambda v: torch.tensor(v, dtype=I32)
        P = em.attn_probs(c.Q, c.K, ti(c.q_off), ti(c.q_len), ti(c.k_off), ti(c.k_len), c.H, c.Lq, c.Lk, c.causal, c.scale,
                          k_prescaled=c.prescaled)
        note("probs", "P", P, c.ref)


def losses():
    R, V = 1206, 4337
    vp = (V + 7) // 8 * 8
    gen = torch.Generator().manual_seed(3)
    logits = torch.full((R, vp), -1e30)
    logits[:, :V] = torch.randn(R, V, generator=gen) * 3
    target = torch.randint(1, V, (R,), generator=gen)
    target[::5] = 0
    res = {}
    for dt in (F32, F64):
        lse, sums, dl = torch.zeros(R), torch.zeros(3), torch.zeros(R, vp, dtype=BF16)
        em.ce_fwd(logits, target, 0, lse, sums)
        em.ce_bwd(logits, target, 0, lse, sums, torch.ones(1), dl, dtype=dt)
        res[dt] = dl
    note("ce_bwd", "dlogits", res[F32][:, :V], res[F64][:, :V])
    n, H, d, S, t = 37, 4, 256, 128, 127
    qkv, cache = g(n, 3 * d, seed=1), g(n, S, 2 * d, seed=2)
    out = {}
    for dt in (F32, F64):
        out[dt] = torch.zeros(n, d, dtype=BF16)
        em.decode_self_attn(qkv, cache.clone(), torch.tensor([t]), out[dt], H, 0.125, dtype=dt)
    note("decode_self_attn", "ctx", out[F32], out[F64])
    M, N, K = 1206, 256, 4344
    X, W, b = g(M, K, seed=1), g(N, K, seed=2, scale=K ** -0.5), g(N, seed=3, dtype=F32)
    note("gemm (fp32 output)", "out", em.gemm(X, W, torch.zeros(M, N), bias=b, epi=nv.EPI_F32),
         em.gemm(X, W, torch.zeros(M, N), bias=b, epi=nv.EPI_F32, dtype=F64))


def lse_family():
    """The vocabulary log-sum-exp over every row family and V of tests/_lse_cases.py, restated in fp32 in two orders - the kernels'
    batched running (max, sum) with a tree merge, and a plain serial max-then-sum, both with __expf as exp2(fp32(d x log2 e)) - against
    fp64.  Per order and family: the worst |err| - ulp32(|ref|) / 2 (clipped at 0) and the worst relative error of exp(x - lse32) over
    the entries with p_ref >= 2^-100.  L_LSE and P_REL are 3 x the larger figure of each column."""
    l_lse, p_rel, rows = lse_cases.measure_bounds()
    print("%-8s %-12s %-24s %s" % ("order", "family", "|err| - ulp32(|ref|) / 2", "relative error of exp(x - lse32)"))
    for order, family, wl, wp in rows:
        print("%-8s %-12s %-24.3e %.3e" % (order, family, wl, wp))
    print("L_LSE = 3 x %.3e = %.3e (in force %.3e; condition <= log(5120 / 5119) / 4 = %.3e: %s)"
          % (l_lse / 3, l_lse, lse_cases.L_LSE, lse_cases.L_LSE_MAX, "met" if l_lse <= lse_cases.L_LSE_MAX else "BROKEN"))
    print("P_REL = 3 x %.3e = %.3e (in force %.3e; condition <= 2^-10 = %.3e: %s)"
          % (p_rel / 3, p_rel, lse_cases.P_REL, lse_cases.P_REL_MAX, "met" if p_rel <= lse_cases.P_REL_MAX else "BROKEN"))


if __name__ == "__main__":
    torch.manual_seed(0)
    if sys.argv[1:] == ["lse"]:
        lse_family()
        sys.exit(0)
    attention(tk.ATTN_CASES, "attention")
    attention(tk.DELTA_CASES, "attention")
    attention(tk.PRESCALED_CASES, "attention (prescaled keys)", prescaled=True)
    attention([(2, 2, 32, None, [7, 4], True, True), (3, 4, 64, None, [200, 131, 64], False, True), (2, 4, 64, [50, 33], [300, 257], False, True),
               (2, 4, 32, None, [129, 70], True, False), (2, 2, 128, None, [200, 131], False, True),
               (2, 2, 128, [50, 33], [300, 257], False, True)], "attention (dropout)",
              drop=em.Drop(torch.tensor([1234567], dtype=I32), 3, 0.2))
    ln_family()
    chain_bwd()
    probs_and_ctc()
    dense()
    probs()
    sharp()
    ln_stats()
    ln_bwd_fp64()
    losses()
    for (family, name, axis), v in sorted(worst.items()):
        print("%-28s %-8s %-8s worst ratio %.3e   x3 = %.3e" % (family, name, axis, v, 3 * v))
    lse_family()

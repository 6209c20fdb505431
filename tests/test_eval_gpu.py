"""-m gpu: forward-only validation on the hardware - st_ce_eval_fwd / st_eval_note (csrc/st_eval.hip) against the fp64 closed
form of tests/_emul_eval.py on the same fp32 logits, then st_amd/evaluate.py:EvalStep: consistency with the logits
forward_packed returns, the fp64 oracle, bucket graphs against eager launches bit for bit, training left alone, averaged weights.

Tolerances of the kernel tests are those tests/test_kernels_gpu.py::test_cross_entropy_rows_matches_torch holds st_ce_fwd to:
per row, L_F32 = 2e-3 of max(|reference|, a quarter of the typical row) through tests/_local.check (its lse check), and 1e-5
relative on the batch's sum (its loss check).  Hits, token counts and states are integers and must be equal.

Shapes: V crosses every boundary of the row reduction - 1 column, fewer than a wave (7, 63), exactly one / one more (64, 65), fewer
than / exactly / one more than the workgroup's 256-column stride (255, 256, 257), exactly / one more than one 2,048-column chunk
of the loop (2048, 2049), the flagship vocabulary (4233); R = 1, 3 and 300 rows (more rows than st_eval_note has threads)."""
import functools

import pytest
import torch

from tests import _emul_eval
from tests._local import Guarded, check, guarded_input
from tests.test_eval_cpu import EPS, STEP_LOSS_TOL, c1_case, d256_case, run_model_mode, run_step_consistency_and_oracle

pytestmark = pytest.mark.gpu

L_F32 = 2e-3          # tests/test_kernels_gpu.py: fp32 lse, per row
SUM_TOL = 1e-5        # ... and its loss: |got - ref| <= 1e-5 |ref|
VS = [1, 7, 63, 64, 65, 255, 256, 257, 2048, 2049, 4233]
RS = [1, 3, 300]


def _triples(V):
    """(confidence, smooth, zero_col) of the plain loss, nn.CrossEntropyLoss(label_smoothing) and LabelSmoothingLoss.  A
    vocabulary of one column has nothing to smooth over (both smoothed losses are identically 0 there): the plain loss only."""
    if V == 1:
        return [("plain", (1.0, 0.0, -1))]
    return [("plain", (1.0, 0.0, -1)), ("ce", (1 - EPS + EPS / V, EPS / V, -1)), ("ls", (1 - EPS, EPS / (V - 1), 0))]


def _run_kernel(logits, target, ignore, triple, V, index=None):
    """logits [R, ldl] on the host -> (rows from the kernel, rows of the fp64 closed form on the same fp32 logits); logits go in
    as a window of a NaN-filled buffer, rows come out inside guard bands."""
    from st_amd import native as nv
    R = logits.shape[0]
    lg = guarded_input(logits, "cuda")
    gr = Guarded(R, 4, torch.float32, "cuda", pad_rows=4, pad_cols=(0, 0))
    nv.ce_eval_fwd(lg, target.cuda(), ignore, triple[0], triple[1], triple[2], gr.view, V=V, index=None if index is None else index.cuda())
    torch.cuda.synchronize()
    gr.assert_intact("ce_eval_fwd rows (R %d, V %d)" % (R, V))
    want = torch.empty(R, 4, dtype=torch.float64)
    _emul_eval.ce_eval_fwd(logits.double(), target, ignore, triple[0], triple[1], triple[2], want, V=V, index=index)
    return gr.view.cpu(), want


def _compare(got, want, what):
    assert torch.equal(got[:, 3].double(), want[:, 3]), "%s: row states differ" % what
    bad = torch.nonzero(got[:, 2].double() != want[:, 2]).flatten()
    assert bad.numel() == 0, "%s: arg-max hit differs in rows %s" % (what, bad[:10].tolist())
    for col, name in ((0, "row_loss"), (1, "row_nll")):
        check(got[:, col], want[:, col], L_F32, "%s %s" % (what, name), tol_local=L_F32)
        s, r = float(got[:, col].double().sum()), float(want[:, col].sum())
        print("%s %s: sum %.9g, fp64 %.9g" % (what, name, s, r))
        assert abs(s - r) <= SUM_TOL * abs(r), (what, name, s, r)
    out = want[:, 3] != 1
    if bool(out.any()):
        assert float(got[out][:, :3].abs().max()) == 0.0, "%s: an ignored / stray row left something" % what


# ---- 1. the row kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VS)
def test_ce_eval_fwd_matches_fp64_on_the_same_logits(V):
    vp = (V + 7) // 8 * 8
    ignore = 0 if V > 1 else -1                 # (V = 1: the only column is the target, so PAD cannot be the ignored one)
    gen = torch.Generator().manual_seed(V)
    for R in RS:
        logits = torch.full((R, vp), -1e30)
        logits[:, :V] = torch.randn(R, V, generator=gen) * 3
        target = torch.randint(min(1, V - 1), V, (R,), generator=gen)
        target[::5] = ignore                    # ignored rows (R = 1: the only row - nothing is counted)
        if R > 1:
            target[1] = V - 1
        idx = torch.randperm(2 * R, generator=gen)[:R]
        truth = torch.full((2 * R,), ignore, dtype=torch.long)
        truth[idx] = target
        for name, triple in _triples(V):
            got, want = _run_kernel(logits, target, ignore, triple, V)
            _compare(got, want, "%s R %d V %d" % (name, R, V))
            # the indexed form (row r's target = truth[index[r]]): same rows, bit for bit
            got_i, _ = _run_kernel(logits, truth, ignore, triple, V, index=idx)
            assert torch.equal(got_i, got), "%s R %d V %d: indexed targets" % (name, R, V)
    # one counted row when R = 1
    logits = torch.full((1, vp), -1e30)
    logits[:, :V] = torch.randn(1, V, generator=gen) * 3
    got, want = _run_kernel(logits, torch.tensor([V - 1]), ignore, (1.0, 0.0, -1), V)
    _compare(got, want, "single counted row V %d" % V)


# (thread i of the 256 holds columns i, i + 256, .., i + 1792 of every 2,048-column chunk)
TIE_PAIRS = [(0, 1),          # neighbouring lanes
             (5, 261),        # one thread: two of the 8 values it holds per chunk (same lane position, one stride on)
             (63, 64),        # across two lanes and a wave boundary
             (255, 256),      # across the workgroup's stride: the last thread and the first
             (5, 2053),       # one thread, across the 2,048-column chunks of the loop
             (4232, 0),       # (V - 1, 0)
             (0, 1792), (2047, 2048), (127, 192)]      # first and last value of a chunk; across chunks and threads; waves 1 and 3


def test_argmax_ties_resolve_to_the_lowest_column():
    """Constructed rows: the maximum sits in two columns; the arg-max is the lower one wherever the two meet in the reduction -
    inside a thread, across lanes, across waves, across chunks.  Each pair twice: the target at the lower column is a hit, at the
    higher one it is not.  Padding columns hold a LARGER value than any logit: they must never be read."""
    V, vp = 4233, 4240
    gen = torch.Generator().manual_seed(7)
    rows_, targets, hits = [], [], []
    for a, b in TIE_PAIRS:
        lo, hi = min(a, b), max(a, b)
        for tgt, hit in ((lo, 1.0), (hi, 0.0)):
            x = torch.randn(V, generator=gen).clamp(-4, 4) * 3
            x[a] = x[b] = 20.0
            rows_.append(x), targets.append(tgt), hits.append(hit)
    x = torch.randn(V, generator=gen).clamp(-4, 4) * 3        # three equal maxima: thread 5's chunks 0 and 1, and a later lane
    x[5] = x[2053] = x[4000] = 20.0
    rows_.append(x), targets.append(5), hits.append(1.0)
    for tgt, hit in ((0, 1.0), (1, 0.0), (V - 1, 0.0)):       # an all-equal row: column 0
        rows_.append(torch.full((V,), 0.5)), targets.append(tgt), hits.append(hit)
    x = torch.randn(V, generator=gen).clamp(-4, 4) * 3        # the maximum in the last valid column is found
    x[V - 1] = 20.0
    rows_.append(x), targets.append(V - 1), hits.append(1.0)
    logits = torch.full((len(rows_), vp), 1e4)                # padding columns: larger than everything, never to be read
    logits[:, :V] = torch.stack(rows_)
    got, want = _run_kernel(logits, torch.tensor(targets), -1, (1.0, 0.0, -1), V)
    assert got[:, 2].tolist() == hits, (got[:, 2].tolist(), hits)
    _compare(got, want, "tie rows")
    # (V - 1, 0) wherever the last column lands: another lane, another wave, the next stride, the next chunk
    for Vs in (2, 7, 64, 65, 257, 2049):
        lg = torch.full((2, (Vs + 7) // 8 * 8), 1e4)
        lg[:, :Vs] = (torch.randn(2, Vs, generator=gen).clamp(-4, 4) * 3)
        lg[:, 0] = lg[:, Vs - 1] = 20.0
        got, want = _run_kernel(lg, torch.tensor([0, Vs - 1]), -1, (1.0, 0.0, -1), Vs)
        assert got[:, 2].tolist() == [1.0, 0.0], (Vs, got[:, 2].tolist())
        _compare(got, want, "tie (V - 1, 0) at V %d" % Vs)


def test_a_stray_label_is_counted_not_followed():
    """Targets V and -5 (neither is ignore_index): the rows leave 0 / 0 / 0, land in acc[6], and the process lives - st_ce_fwd
    traps here."""
    from st_amd import native as nv
    V, vp = 30, 32
    logits = torch.full((6, vp), -1e30)
    logits[:, :V] = torch.randn(6, V, generator=torch.Generator().manual_seed(1)) * 3
    target = torch.tensor([3, V, -5, 0, 7, 10 ** 12])
    got, want = _run_kernel(logits, target, 0, (0.9, 0.1 / 29, 0), V)
    assert got[:, 3].tolist() == [1.0, 2.0, 2.0, 0.0, 1.0, 2.0]
    _compare(got, want, "stray labels")
    acc, last = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(4, device="cuda")
    nv.eval_note(got.cuda(), acc, last)
    torch.cuda.synchronize()
    a = acc.tolist()
    assert a[3] == 2.0 and a[6] == 3.0 and a[5] == 1.0 and a[1] == 2.0
    assert a[0] == float(got[:, 0].double().sum()) and a[2] == float(got[:, 1].double().sum())


# ---- 2. the accumulator ----------------------------------------------------------------------------------------------------------
def _note_rows(R, seed):
    """Rows as the kernel leaves them.  Losses are fp32 values in [2^-10, 16): multiples of 2^-33 below 2^4, so every partial
    sum of the ~1,100 of them added here is a multiple of 2^-33 below 2^15 - 48 bits: exact in fp64, in ANY order."""
    gen = torch.Generator().manual_seed(seed)
    rows = torch.empty(R, 4)
    rows[:, :2] = torch.rand(R, 2, generator=gen) * 15.99 + 2.0 ** -10
    rows[:, 2] = (torch.rand(R, generator=gen) < 0.3).float()
    rows[:, 3] = torch.randint(0, 3, (R,), generator=gen).float()
    rows[rows[:, 3] != 1, :3] = 0.0
    return rows


def test_eval_note_accumulates_exactly_in_fp64():
    from st_amd import native as nv
    ga, gl = Guarded.vec(8, torch.float64, "cuda"), Guarded.vec(4, torch.float32, "cuda")
    ga.view.zero_()
    acc, last = ga.view, gl.view
    want = torch.zeros(8, dtype=torch.float64)
    for k, (R, denom) in enumerate(((300, None), (1, None), (513, 77.0), (257, None))):
        rows = _note_rows(R, k)
        if R == 1:
            rows[0] = torch.tensor([1.25, 0.75, 1.0, 1.0])
        r64 = rows.double()
        tok, bad = float((rows[:, 3] == 1).sum()), float((rows[:, 3] == 2).sum())
        den = tok if denom is None else denom
        s = r64[:, :3].sum(0)
        want += torch.tensor([float(s[0]), den, float(s[1]), tok, float(s[2]), 1.0, bad, 0.0], dtype=torch.float64)
        nv.eval_note(guarded_input(rows, "cuda", pad_rows=4, pad_cols=(0, 0)), acc, last,
                     denom=None if denom is None else torch.tensor([denom], device="cuda"))
        torch.cuda.synchronize()
        ga.assert_intact("acc"), gl.assert_intact("last")
        assert torch.equal(acc.cpu(), want), (k, acc.tolist(), want.tolist())              # exactly: fp64 adds of fp32 inputs
        # last is this batch's alone: the same fp64 quotients, rounded once to fp32
        per = torch.stack([s[0] / den, s[1] / tok, s[2] / tok, torch.tensor(tok, dtype=torch.float64)]).float()
        assert torch.equal(last.cpu(), per), (k, last.tolist(), per.tolist())
    # a batch without a counted token: nan means, acc[0:5] keeps its bits, the batch is counted
    before = acc.clone()
    nv.eval_note(torch.zeros(40, 4, device="cuda"), acc, last)
    torch.cuda.synchronize()
    assert torch.equal(acc[:5].view(torch.int64), before[:5].view(torch.int64)) and float(acc[5]) == float(before[5]) + 1.0
    assert bool(torch.isnan(last[:3]).all()) and float(last[3]) == 0.0
    nv.eval_note(torch.zeros(0, 4, device="cuda"), acc, last)           # ... and one without a row
    torch.cuda.synchronize()
    assert torch.equal(acc[:5].view(torch.int64), before[:5].view(torch.int64)) and float(acc[5]) == float(before[5]) + 2.0
    ga.assert_intact("acc"), gl.assert_intact("last")


# ---- 3. / 4. the step: consistent with its own logits, and against the oracle ---------------------------------------------------
def test_step_c1_consistency_and_oracle(golden_dir):
    m, batch, V, truth = c1_case(golden_dir, "cuda")
    run_step_consistency_and_oracle(m, batch, V, truth, row_tol=SUM_TOL)


def test_step_d256_row_chains_consistency_and_oracle():
    m, batch, V, truth = d256_case("cuda")
    run_step_consistency_and_oracle(m, batch, V, truth, row_tol=SUM_TOL)
    assert m.encoder._st_chains[1] is not None and m.decoder._st_chains[1] is not None, "row chains were not taken"


# ---- 5. - 8. graphs, training, averaged weights, model mode -------------------------------------------------------------------
B, T_CAP, L_CAP = 3, 160, 20


def _small(dropout=0.0, seed=0):
    from transformer.Models import Transformer
    from transformer.Utils import AttrDict, init_parameters
    cfg = AttrDict(dict(feature_dim=80, max_inputs_length=200, max_target_length=32, num_enc_layer=2, num_dec_layer=2, n_heads=4,
                        d_k=32, d_v=32, d_model=128, d_inner_hid=256, dropout=dropout, vocab_size=30))
    torch.manual_seed(seed)
    model = Transformer(cfg).cuda()
    init_parameters(model)
    return cfg, model.eval()


@functools.lru_cache(maxsize=None)
def _batches():
    """Three batches of B utterances with different lengths (and different longest utterances), in TrainStep's argument order."""
    from st_amd import synthetic
    out = []
    for seed, (t, l) in enumerate(((T_CAP, L_CAP), (120, 14), (90, 17))):
        x, tok, in_len, tgt_len, gt = synthetic.make_batch(B, t, l, 80, 30, seed=seed + 1, t_min=t // 3, l_min=l // 3)
        out.append((x.cuda(), in_len, tok.cuda(), tgt_len, gt.cuda()))
    return out


def _packed_capacity():
    rows_in = max(int(b[1].sum()) for b in _batches())
    rows_tgt = max(int(b[3].sum()) for b in _batches())
    cap = ((rows_in + 7) // 8 * 8, (rows_tgt + 7) // 8 * 8)
    assert T_CAP <= cap[0] < B * T_CAP and L_CAP <= cap[1] < B * L_CAP          # packed for real: fewer rows than the padded bucket
    return cap


def _pass(ev):
    ev.reset()
    for b in _batches():
        ev(*b)
    torch.cuda.synchronize()
    return ev.acc.clone().view(torch.int64)


@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("kind", ["plain", "ls"])
def test_bucket_graph_equals_eager_bit_for_bit(layout, kind):
    from st_amd.evaluate import EvalStep
    from transformer.Loss import LabelSmoothingLoss
    _, model = _small()
    crit = None if kind == "plain" else LabelSmoothingLoss(EPS, 30, ignore_index=0)      # ("rows": the denominator is staged per batch)
    kw = dict(criterion=crit, bucket=(T_CAP, L_CAP), bucket_rows=_packed_capacity() if layout == "packed" else None)
    eager = EvalStep(model, 30, use_graph=False, **kw)
    want = _pass(eager)
    graph = EvalStep(model, 30, use_graph=True, graph_warmup=1, **kw)
    first = _pass(graph)                     # one eager batch, the capture + its replay, one more replay
    assert len(graph._buckets) == 1 and next(iter(graph._buckets.values())).cap is not None
    second = _pass(graph)                    # after reset(): three replays
    r = graph.result()
    print("bucket %s %s: %s" % (layout, kind, r))
    assert torch.equal(first, want), (first.view(torch.float64).tolist(), want.view(torch.float64).tolist())
    assert torch.equal(second, first)
    tokens = sum(int((b[4] != 0).sum()) for b in _batches())
    assert r["tokens"] == tokens and r["batches"] == 3 and r["bad_targets"] == 0 and 0.0 <= r["accuracy"] <= 1.0
    if kind == "ls":
        assert float(graph.acc[1]) == float(sum(B * int(b[3].max()) for b in _batches()))
    # the same batches without a bucket (ragged layouts of each batch): the same tokens, and an NLL inside the bf16 band a
    # step's loss is held to
    plain = EvalStep(model, 30, criterion=crit, use_graph=False)
    _pass(plain)
    rp = plain.result()
    assert rp["tokens"] == tokens and abs(rp["nll"] - r["nll"]) <= STEP_LOSS_TOL * r["nll"]


def test_train_and_eval_bucket_captures_interleaved():
    """A TrainStep and an EvalStep on ONE model, both capturing a packed bucket, called alternately: each driver's warm-up,
    its recording call and its capture fall between the other's (what they share is the process-wide TailBuffers.active of
    stepdriver.bucket_step).  The model and the batches are those of tests/test_composition_cpu.py:run_bucket_mode, without
    its over-long batch - all six fit the one packed capacity; so are the bounds of the train step against an eager twin.
    Every eval call equals, bit for bit, a fresh eager EvalStep over the same bucket layouts on the same weights."""
    import copy
    import oracle as orc
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd.evaluate import EvalStep
    from st_amd.functional import TailBuffers
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    t_cap, l_cap, rows = 96, 12, (340, 44)
    torch.manual_seed(5)
    cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=t_cap, max_target_length=l_cap, num_enc_layer=2, num_dec_layer=2,
                          n_heads=4, d_k=64, d_v=64, d_model=256, d_inner_hid=512, dropout=0.0, vocab_size=30))
    ma = M.Transformer(cfg)
    U.init_parameters(ma)
    mb = copy.deepcopy(ma)
    ma, mb = ma.eval().cuda(), mb.eval().cuda()
    kw = dict(bucket=(t_cap, l_cap), bucket_rows=rows)
    sa = TrainStep(ma, ScheduledOptim(ma, 256, U.AttrDict(n_warmup_steps=50)), 30, 5.0, use_graph=True, graph_warmup=1, **kw)
    sb = TrainStep(mb, ScheduledOptim(mb, 256, U.AttrDict(n_warmup_steps=50)), 30, 5.0, use_graph=False)
    ev = EvalStep(ma, 30, use_graph=True, **kw)
    seen = set()
    for i in range(6):
        b = orc.synthetic_batch(4, t_cap, l_cap, 80, 30, seed=20 + i, t_min=40, l_min=4)
        assert int(b["in_len"].sum()) <= rows[0] and int(b["tgt_len"].sum()) <= rows[1]
        seen.add((tuple(b["in_len"].tolist()), tuple(b["tgt_len"].tolist())))
        T, L = int(b["in_len"].max()), int(b["tgt_len"].max())
        batch = (b["x"][:, :T].cuda(), b["in_len"], b["tokens"][:, :L].cuda(), b["tgt_len"], b["gt"][:, :L].cuda())
        la, ga = sa(*batch)
        lb, gb = sb(*batch)
        la, ga, lb, gb = float(la), float(ga), float(lb), float(gb)
        print("batch %d: train loss %.7g (eager twin %.7g), norm %.7g (%.7g)" % (i, la, lb, ga, gb))
        assert TailBuffers.active is None
        assert abs(la - lb) <= (1e-5 if i == 0 else 5e-3) * abs(lb), (i, la, lb)
        assert abs(ga - gb) <= (1e-4 if i == 0 else 3e-2) * abs(gb), (i, ga, gb)
        got = ev(*batch).clone()
        assert TailBuffers.active is None
        want = EvalStep(ma, 30, use_graph=False, **kw)(*batch)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (i, got.tolist(), want.tolist())
    assert len(seen) == 6, "the batches' lengths must not repeat"
    for drv in (sa, ev):
        assert len(drv._buckets) == 1 and next(iter(drv._buckets.values())).cap is not None
    assert TailBuffers.active is None


def _train_batches():
    """Single utterances of at most 30 frames and 6 tokens.  The training step adds its LayerNorm / bias column sums and the
    embedding gradient with fp32 atomics (include/st_hip.h: "accumulated atomically"), so with two or more workgroups per launch
    two identical runs differ in a few dozen of 681,088 parameter elements after one step (measured: 48 - 137 at the shapes of
    _batches(), 3 - 39 at 2 x 48 frames, 0 in every run at these shapes, with and without dropout).  Here every row-wise launch
    is ONE workgroup and no token occurs more than twice, so every atomic sum has at most two terms and the step is
    reproducible bit for bit - which is what a bitwise comparison of two runs needs to say anything about the validation pass."""
    from st_amd import synthetic
    out = []
    for seed, (t, l) in ((11, (30, 6)), (12, (24, 5)), (13, (20, 4))):
        x, tok, in_len, tgt_len, gt = synthetic.make_batch(1, t, l, 80, 30, seed=seed, t_min=t // 3, l_min=l // 3)
        assert int(torch.bincount(tok.view(-1)).max()) <= 2
        out.append((x.cuda(), in_len, tok.cuda(), tgt_len, gt.cuda()))
    return out


def test_eval_pass_leaves_training_alone():
    """Two runs of 4 TrainStep steps in train() mode with dropout, from the same weights and the same dropout seed; one has an
    EvalStep pass (over the three batches of _batches()) between steps 2 and 3, toggling eval() / train().  Parameters and Adam
    moments end bit for bit equal - and, looked at directly, the pass itself changes no bit of the parameters, the moments, the
    gradient buffer, the step count or the dropout seed.  The training batches: _train_batches()."""
    from st_amd import rng
    from st_amd.evaluate import EvalStep
    from st_amd.trainer import TrainStep
    from transformer.Optim import ScheduledOptim
    from transformer.Utils import AttrDict

    train = _train_batches()

    def run(with_eval):
        _, model = _small(dropout=0.1, seed=3)
        model.train()
        opt = ScheduledOptim(model, 128, AttrDict(n_warmup_steps=20))
        dev = next(model.parameters()).device
        rng.seed_tensor(dev)
        rng.manual_seed(20260928)
        step = TrainStep(model, opt, 30, 5.0, use_graph=False)
        ev = EvalStep(model, 30, use_graph=False)
        for it in range(4):
            if with_eval and it == 2:
                st = opt._flat_state()[1]
                watched = (opt.arena.flat, opt.arena.grad, st["exp_avg"], st["exp_avg_sq"], st["step"], rng.seed_tensor(dev))
                before = [t.detach().clone().view(torch.int32) for t in watched]
                model.eval()
                for b in _batches():
                    ev(*b)
                assert ev.result()["batches"] == 3
                model.train()
                for name, a, t in zip(("parameters", "gradients", "exp_avg", "exp_avg_sq", "step count", "dropout seed"), before, watched):
                    assert torch.equal(a, t.detach().view(torch.int32)), "the validation pass changed the %s" % name
            step(*train[it % 3])
        st = opt._flat_state()[1]
        torch.cuda.synchronize()
        return [t.detach().clone().view(torch.int32) for t in (opt.arena.flat, st["exp_avg"], st["exp_avg_sq"])]

    a, b = run(False), run(True)
    for name, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), a, b):
        assert torch.equal(x, y), "%s differ in %d elements" % (name, int((x != y).sum()))


def test_averaged_weights_eager_and_replay():
    """Inside optimizer.averaged() EvalStep gives, bit for bit, the accumulator of a second model loaded with the averaged
    weights - eagerly and from a captured graph; outside the context the SAME graph gives the raw weights' result again."""
    from st_amd.evaluate import EvalStep
    from st_amd.trainer import TrainStep
    from transformer.Models import Transformer
    from transformer.Optim import ScheduledOptim
    from transformer.Utils import AttrDict
    cfg, model = _small()
    opt = ScheduledOptim(model, 128, AttrDict(n_warmup_steps=20))
    opt.enable_averaging(decay=0.5, warmup=False)
    step = TrainStep(model, opt, 30, 5.0, use_graph=False)
    for _ in range(3):
        step(*_batches()[0])
    with pytest.raises(RuntimeError, match="averaged"):
        with opt.averaged():
            step(*_batches()[0])                                   # (TrainStep refuses the context; EvalStep works inside it)
    arena = opt.arena
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for name, p in model.named_parameters():
        sd[name] = arena.avg_view(p).detach().clone()
    fresh = Transformer(cfg).cuda()
    fresh.load_state_dict(sd)
    fresh.eval()
    kw = dict(bucket=(T_CAP, L_CAP))
    want_avg = _pass(EvalStep(fresh, 30, use_graph=False, **kw))
    want_raw = _pass(EvalStep(model, 30, use_graph=False, **kw))
    assert not torch.equal(want_avg, want_raw), "the averaged weights must evaluate differently"
    eager, graph = EvalStep(model, 30, use_graph=False, **kw), EvalStep(model, 30, use_graph=True, graph_warmup=1, **kw)
    with opt.averaged():
        assert torch.equal(_pass(eager), want_avg)
        assert torch.equal(_pass(graph), want_avg)                 # eager batch, capture + replay, replay
        assert torch.equal(_pass(graph), want_avg)                 # three replays
    assert torch.equal(_pass(graph), want_raw)                     # the same captured graph, the raw weights
    assert torch.equal(_pass(eager), want_raw)
    assert len(graph._buckets) == 1


def test_training_mode_raises(golden_dir):
    m, batch, V, _ = c1_case(golden_dir, "cuda")
    run_model_mode(m, batch, V)

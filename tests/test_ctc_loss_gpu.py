"""-m gpu: the HIP CTC loss (csrc/st_ctc_loss.hip: native.ctc_loss_fwd / ctc_loss_grad, functional.ctc_loss,
CTCAttentionLoss.ctc_rows(impl="hip"), JointTrainStep(ctc="hip")) on the hardware.

Accuracy is judged against the fp64 truth of tests/_ctc_loss_ref.py and RELATIVE TO torch-ROCm's own float32 ``ctc_loss`` on the
same inputs: the kernels must be no worse than 1.5 x torch's error (a different but equally long float32 summation order) plus a
small absolute floor that comes from the number format alone (see FLOOR_NLL / floor_g below).  torch is only consulted where its definition coincides with
the truth - labels >= 1; a grid point's blank-id variant is held to the bound its labels >= 1 variant (same shape, same
distribution) set.  The tables go to the report directory (REPORTS below: ST_TEST_REPORT_DIR, default test_reports/) as
ctc_loss_parity.txt and parity_c4_b32_hip_ctc.txt; a copy of both lives in profiles/ctc_loss_parity.txt."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as func

import oracle as orc
from st_amd import functional as F_
from st_amd import native as nv
from tests import _ctc_loss_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = os.environ.get("ST_TEST_REPORT_DIR") or os.path.join(ROOT, "test_reports")      # (kept out of git)
EPS = float(np.finfo(np.float32).eps)
# The absolute floor, for the cases where torch's error is (nearly) exactly zero - a few frames, values of order 1: what remains
# then is the float32 format itself.
#  - nll is stored as a float32 and comes out of a final float32 logaddexp: a few roundings -> 4 eps relative;
#  - an occupancy is a float32 exp of a float32 sum, summed over a class's states, and exp(lp) is another: a handful of
#    roundings each -> 16 eps of the OCCUPANCIES' norm.  The gradient exp(lp) - occ inherits that as an absolute error - where the
#    model is confident both terms are ~1 and the gradient is their small difference - so on the gradient's rel-L2 the floor is
#    16 eps |occ| / |g|.
# Neither grows with T or |nll|: the error of a long float32 recursion is what the 1.5 x torch term is for.
FLOOR_NLL = 4 * EPS
MARGIN = 1.5


def floor_g(truth):
    fin = np.isfinite(truth["nll"])
    gn = float(np.linalg.norm(truth["g"][fin]))
    return 16 * EPS * (float(np.linalg.norm(truth["occ"][fin])) / gn if gn > 0 else 1.0)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def make_case(B, T, L, peaked, lo, seed):
    """Ragged lengths, repeats, (lo = 0:) blank-id labels, and - where the shape allows - an infeasible utterance; frames past a
    length are NaN in the kernels' input."""
    g = torch.Generator().manual_seed(seed)
    C = L + 1 if L > 0 else 2
    lp = torch.log_softmax(torch.randn(B, T, C, generator=g) * (6.0 if peaked else 0.5), -1)
    il = torch.randint(max(1, T // 2), T + 1, (B,), generator=g)
    il[0] = T
    tl = torch.randint(L // 2, L + 1, (B,), generator=g) if L > 0 else torch.zeros(B, dtype=torch.int64)
    if L > 0:
        tl[0] = L
    cls = torch.randint(lo, C, (B, L), generator=g) if L > 0 else torch.zeros(B, 0, dtype=torch.int64)
    if L > 1:
        cls[:, 1] = cls[:, 0]                                                 # an adjacent repeat in every utterance
        if lo == 0:
            cls[:, L - 1] = 0                                                 # ... and utterances that END in the blank id
    if B > 1 and L > 1:
        il[B - 1] = min(int(il[B - 1]), max(1, int(tl[B - 1]) // 2))          # fewer frames than labels: no alignment
    poisoned = lp.clone()
    poisoned[torch.arange(T).view(1, -1) >= il.view(-1, 1)] = float("nan")
    return lp, poisoned, cls, il, tl


def run_hip(lp, cls, il, tl, coef=None, softmax_term=True):
    B, T, C = lp.shape
    dev = "cuda"
    lpg, clg = lp.to(dev), cls.to(dev)
    ilg, tlg = il.to(dev, torch.int32), tl.to(dev, torch.int32)
    ws = torch.empty(nv.ctc_loss_ws_bytes(B, T, cls.shape[1]), dtype=torch.uint8, device=dev)
    nll = torch.empty(B, device=dev)
    g, roww = torch.full((B, T, C), 7.0, device=dev), torch.full((B,), 7.0, device=dev)
    cf = torch.ones(B, device=dev) if coef is None else coef.to(dev)
    nv.ctc_loss_fwd(lpg, clg, ilg, tlg, ws, nll)
    nv.ctc_loss_grad(lpg, clg, ilg, tlg, cf, ws, nll, g, roww, softmax_term=softmax_term)
    torch.cuda.synchronize()
    return nll.cpu(), g.cpu(), roww.cpu()


def errors(nll, g, truth):
    fin = np.isfinite(truth["nll"])
    if not fin.any():
        return 0.0, 0.0
    e_n = float(np.max(np.abs(nll.double().numpy()[fin] - truth["nll"][fin]) / np.maximum(np.abs(truth["nll"][fin]), 1e-30)))
    tg = torch.from_numpy(truth["g"][fin])
    e_g = rel(g[torch.from_numpy(fin)], tg) if float(tg.abs().max()) > 0 else float(g[torch.from_numpy(fin)].abs().max())
    return e_n, e_g


LS = [0, 1, 50, 63, 64, 127, 200]


@pytest.mark.parametrize("T", [1, 7, 200, 1000])
@pytest.mark.parametrize("B", [1, 8, 32])
def test_kernels_vs_fp64_truth_relative_to_torch_float32(B, T):
    lines, failures = [], []
    for L in LS:
        for peaked in (True, False):
            for lo in (1, 0):                                                 # labels >= 1 first: it sets the bound
                lp, poisoned, cls, il, tl = make_case(B, T, L, peaked, lo, seed=1000 * B + 10 * T + L + (500 if peaked else 0))
                truth = ref.alpha_beta(lp.numpy(), cls.numpy(), il.numpy(), tl.numpy())
                nll, g, roww = run_hip(poisoned, cls, il, tl)
                fin = np.isfinite(truth["nll"])
                tag = "B %2d T %4d L %3d %s labels>=%d" % (B, T, L, "peaked" if peaked else "flat  ", lo)
                # exact properties: the infinite losses, zero_infinity, nothing read or written past a length
                assert np.array_equal(np.isinf(nll.numpy()) & (nll.numpy() > 0), ~fin), tag
                assert torch.isfinite(g).all() and torch.isfinite(nll[torch.from_numpy(fin)]).all(), tag
                assert float(g[torch.from_numpy(~fin)].abs().sum()) == 0.0, tag
                assert float(g[torch.arange(T).view(1, -1) >= il.view(-1, 1)].abs().sum()) == 0.0, tag
                assert np.array_equal(roww.numpy(), np.where(fin, 1.0, 0.0).astype(np.float32)), tag
                e_n, e_g = errors(nll, g, truth)
                nmax = float(np.abs(truth["nll"][fin]).max()) if fin.any() else 0.0
                if lo == 1:
                    leaf = lp.cuda().requires_grad_(True)
                    t_nll = func.ctc_loss(leaf.transpose(0, 1), cls.cuda() if L > 0 else torch.zeros(B, 1, dtype=torch.int64, device="cuda"),
                                          il, tl, blank=0, reduction="none", zero_infinity=True)
                    (t_g,) = torch.autograd.grad(t_nll.sum(), leaf)
                    t_nll = torch.where(torch.from_numpy(fin).cuda(), t_nll.detach(), torch.full_like(t_nll, float("inf")))
                    t_n, t_gg = errors(t_nll.cpu(), t_g.cpu(), truth)
                    lines.append("%s  nll rel: hip %.3e torch %.3e | grad rel-L2: hip %.3e torch %.3e | floor %.1e | max |nll| %.1f"
                                 % (tag, e_n, t_n, e_g, t_gg, floor_g(truth), nmax))
                else:                                                         # (torch's figures of the labels >= 1 variant stand)
                    lines.append("%s  nll rel: hip %.3e               | grad rel-L2: hip %.3e                 | floor %.1e | max |nll| %.1f"
                                 % (tag, e_n, e_g, floor_g(truth), nmax))
                bound = (MARGIN * t_n + FLOOR_NLL, MARGIN * t_gg + floor_g(truth))
                print(lines[-1])
                if e_n > bound[0] or e_g > bound[1]:
                    failures.append(lines[-1])
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, "ctc_loss_parity.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")
    assert not failures, "outside 1.5 x torch's float32 error + floor:\n" + "\n".join(failures)


def test_two_launches_are_bit_equal_and_coef_scales_the_gradient():
    lp, poisoned, cls, il, tl = make_case(32, 1000, 50, True, 0, seed=11)
    coef = torch.rand(32) + 0.5
    a = run_hip(poisoned, cls, il, tl, coef=coef)
    b = run_hip(poisoned, cls, il, tl, coef=coef)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    one = run_hip(poisoned, cls, il, tl)
    assert torch.equal(a[0], one[0])
    assert rel(a[1], one[1] * coef.view(-1, 1, 1)) < 4 * EPS
    fin = torch.isfinite(a[0])
    assert torch.equal(a[2], torch.where(fin, coef, torch.zeros(32)))
    # softmax_term = False: -coef occ, i.e. the other form minus coef exp(lp) on the live frames; every live row sums to -coef
    occ = run_hip(poisoned, cls, il, tl, coef=coef, softmax_term=False)
    live = (torch.arange(1000).view(1, -1) < il.view(-1, 1)) & fin.view(-1, 1)
    soft = torch.where(live.unsqueeze(2), torch.exp(lp), torch.zeros(()))
    assert rel(occ[1], a[1] - coef.view(-1, 1, 1) * soft) < 16 * EPS
    rows = occ[1].double().sum(2)
    # (an occupancy carries the float32 error of its exponent - three terms that reach log2(e) |nll| in the kernels' base-2
    # units, half an ulp each at best: 4 eps (1 + log2(e) max |nll|) bounds a row's relative defect)
    tol = 4 * EPS * (1.0 + 1.4427 * float(a[0][fin].abs().max()))
    assert float(((rows + coef.double().view(-1, 1)) / coef.double().view(-1, 1))[live].abs().max()) < tol, tol
    assert float(rows[~live].abs().max()) == 0.0


def test_functional_ctc_loss_under_graph_capture_follows_refilled_buffers():
    """functional.ctc_loss forward + backward captured by torch.cuda.graph: the replay equals the eager call bit for bit, and a
    replay after the label and lp buffers were refilled IN PLACE follows the new contents (lengths and labels are read on the
    device at replay time, nothing was baked in at capture)."""
    B, T, L = 8, 200, 50
    lp1, _, cls1, il, tl = make_case(B, T, L, True, 0, seed=21)
    lp2, _, cls2, _, _ = make_case(B, T, L, False, 1, seed=22)
    il[B - 1] = T                                             # (all feasible: a finite mean)
    lp_s, cls_s = lp1.cuda().requires_grad_(True), cls1.cuda()
    il_s, tl_s = il.to("cuda", torch.int32), tl.to("cuda", torch.int32)

    def eager(lp, cls):
        leaf = lp.cuda().requires_grad_(True)
        loss = F_.ctc_loss(leaf, cls.cuda(), il_s, tl_s)
        loss.backward()
        none = F_.ctc_loss(leaf.detach(), cls.cuda(), il_s, tl_s, reduction="none")
        return loss.detach().clone(), leaf.grad.clone(), none

    e1, e2 = eager(lp1, cls1), eager(lp2, cls2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F_.ctc_loss(lp_s, cls_s, il_s, tl_s).backward()
    torch.cuda.current_stream().wait_stream(side)
    lp_s.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = F_.ctc_loss(lp_s, cls_s, il_s, tl_s)
        loss_s.backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_s.detach(), e1[0]) and torch.equal(lp_s.grad, e1[1])
    with torch.no_grad():
        lp_s.copy_(lp2)
        cls_s.copy_(cls2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_s.detach(), e2[0]) and torch.equal(lp_s.grad, e2[1])
    assert not torch.equal(e1[0], e2[0])
    # the value against the truth, and the gradient is -occ / (B tl): rows of the live frames sum to -1 / (B tl)
    truth = ref.alpha_beta(lp2.numpy(), cls2.numpy(), il.numpy(), tl.numpy())
    want = float((truth["nll"] / np.maximum(tl.numpy(), 1)).mean())
    assert abs(float(e2[0]) - want) < 1e-4 * abs(want)
    assert rel(e2[2].cpu(), torch.from_numpy(truth["nll"])) < 1e-4
    assert rel(e2[1].cpu(), torch.from_numpy(-truth["occ"] / (B * np.maximum(tl.numpy(), 1))[:, None, None])) < 1e-4


C2 = dict(feature_dim=80, max_inputs_length=1000, max_target_length=50, num_enc_layer=6, num_dec_layer=6, n_heads=4,
          d_k=64, d_v=64, d_model=256, d_inner_hid=1024, dropout=0.1, vocab_size=4337)
GRAD_TOL_TENSOR = 8e-2


def test_config4_joint_trainstep_hip_ctc_b32_one_graph_vs_fp64_oracle():
    """tests/test_fullsize_gpu.py::test_config4_joint_trainstep_b32_graph_vs_fp64_oracle for JointTrainStep(ctc="hip"): the whole
    step is ONE captured graph; joint loss, CTC loss, attention CE and EVERY gradient after a replay against the fp64 oracle - whose
    CTC term is the differentiable fp64 restatement of tests/_ctc_loss_ref.py (the seed-0 ground truth ends every utterance with
    id 0 = the blank id, where torch's gradient is not the derivative).  Same bounds and the same floor column (the fp64 oracle
    with torch's ctc_loss in float32) as the original.

    Measured (profiles/ctc_loss_parity.txt): see the file's c4_b32 block; the rel-L2 between the HIP g_lp and torch-ROCm's on this
    batch is recorded there as information."""
    import transformer.Models as M
    import transformer.Utils as U
    from st_amd import synthetic
    from st_amd.arena import arena_of
    from st_amd.trainer import JointTrainStep
    from transformer.Loss import CTCAttentionLoss
    from transformer.Optim import ScheduledOptim

    cfg = C2
    torch.manual_seed(0)
    model = M.Transformer(U.AttrDict(cfg))
    U.init_parameters(model)
    w = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.eval().cuda()
    x, tokens, in_len, tgt_len, gt = synthetic.make_batch(32, 1000, 50, cfg["feature_dim"], cfg["vocab_size"], seed=0, t_min=500, l_min=25)
    L, T = int(tgt_len.max()), int(in_len.max())
    xg, tg, gg = x[:, :T].cuda(), tokens[:, :L].cuda(), gt[:, :L].cuda()
    torch.manual_seed(0)
    head = CTCAttentionLoss(cfg["d_model"], cfg["vocab_size"], ctc_weight=0.3).cuda()
    H = cfg["n_heads"]

    names = [k for k in w if not k.endswith(".pe")]
    l64 = {k: (v.double().cuda().requires_grad_(True) if k in names else v.double().cuda()) for k, v in w.items()}
    w64 = head.ctc_proj.weight.detach().double().clone().requires_grad_(True)
    b64 = head.ctc_proj.bias.detach().double().clone().requires_grad_(True)
    enc, _ = orc.encoder(l64, xg.double(), in_len, H)
    dec, _, _ = orc.decoder(l64, tg, tgt_len, in_len, enc, H)
    att64 = orc.cross_entropy(func.linear(dec, l64["tgt_word_proj.weight"]), gg)
    logp_bt = func.log_softmax(func.linear(enc, w64, b64), -1)                  # [B, T, V]: the dense alphabet, classes = ids
    nll64 = ref.nll_torch(logp_bt, gg, in_len.cuda(), tgt_len.cuda())
    assert not bool(ref.is_inf(nll64).any())
    ctc64 = (nll64 / tgt_len.cuda().clamp_min(1).double()).mean()
    truth = 0.3 * ctc64 + 0.7 * att64
    g64 = torch.autograd.grad(truth, [l64[k] for k in names] + [w64, b64], allow_unused=True, retain_graph=True)
    allnames = names + ["ctc_proj.weight", "ctc_proj.bias"]
    tgd = dict(zip(allnames, g64))
    # the floor column of the original test: torch's ctc_loss in float32 with everything else in float64
    logp = logp_bt.transpose(0, 1)
    ctc32 = func.ctc_loss(logp.float(), gg, in_len, tgt_len, blank=0, reduction="mean", zero_infinity=True)
    g32 = torch.autograd.grad(0.3 * ctc32.double() + 0.7 * att64, [l64[k] for k in names] + [w64, b64], allow_unused=True)
    floor = {k: (rel(a, t) if t is not None else 0.0) for k, a, t in zip(allnames, g32, g64)}
    del enc, dec, logp, logp_bt, g32, nll64
    torch.cuda.empty_cache()

    opt = ScheduledOptim(model, cfg["d_model"], U.AttrDict(n_warmup_steps=10 ** 9))      # lr ~ 1e-15: the weights stay put
    step = JointTrainStep(model, opt, head, max_grad_norm=1e9, use_graph=True, graph_warmup=1, ctc="hip")
    for _ in range(3):                                     # eager, capture + replay, replay
        loss, att, ctc, gnorm = step(xg, in_len, tg, tgt_len, gg)
    torch.cuda.synchronize()
    assert step._cap is not None and len(step.graphs) == 1, "ctc='hip': the whole step must be ONE captured graph"
    assert step._side is None, "no side stream on the HIP path"
    print("c4_b32 hip: loss %.5f (oracle %.5f), ctc %.5f (%.5f), att %.5f (%.5f)"
          % (float(loss), truth.item(), float(ctc), ctc64.item(), float(att), att64.item()))
    assert abs(float(loss) - truth.item()) < 2e-2 * abs(truth.item()), (float(loss), truth.item())
    assert abs(float(ctc) - ctc64.item()) < 2e-2 * abs(ctc64.item()), (float(ctc), ctc64.item())
    assert abs(float(att) - att64.item()) < 2e-2 * abs(att64.item())
    arena = arena_of(model)
    rows = []
    for nme, q in model.named_parameters():
        if "linear_k.bias" in nme or tgd[nme] is None:
            continue
        g = arena.grad_view(q).detach().double()
        assert torch.isfinite(g).all(), nme
        rows.append((rel(g, tgd[nme]), floor[nme], nme, tgd[nme].norm().item()))
    for nme, q in (("ctc_proj.weight", head.ctc_proj.weight), ("ctc_proj.bias", head.ctc_proj.bias)):
        rows.append((rel(q.grad.detach().double(), tgd[nme]), floor[nme], nme, tgd[nme].norm().item()))
    rows.sort(reverse=True)
    keep = [(nme, q) for nme, q in model.named_parameters() if "linear_k.bias" not in nme and tgd[nme] is not None]
    glob = rel(torch.cat([arena.grad_view(q).detach().double().reshape(-1) for _, q in keep]), torch.cat([tgd[nme].reshape(-1) for nme, _ in keep]))
    # information, not a gate: the HIP g_lp against torch-ROCm's float32 gradient on the same log-probabilities
    plan = step._plan
    g_hip = plan.g_lp.clone()
    _, g_torch = head.ctc_rows(plan.lp, plan, impl="torch")
    info = rel(g_hip, 0.3 * g_torch)
    last = torch.zeros_like(g_hip, dtype=torch.bool)
    last[torch.arange(32, device="cuda"), (in_len - 1).cuda()] = True
    info_body = rel(g_hip[~last], 0.3 * g_torch[~last])
    lines = ["# c4_b32: JointTrainStep(ctc='hip'), ONE graph (replay), joint 0.3 CTC + 0.7 attention, 6+6 / d256, B = 32: loss %.5f (oracle %.5f), ctc %.4f (%.4f), att %.4f (%.4f)"
             % (float(loss), truth.item(), float(ctc), ctc64.item(), float(att), att64.item()),
             "# (information) rel-L2 of the HIP g_lp against torch-ROCm's float32 ctc_loss gradient on the same lp: %.3e over all frames, %.3e without each utterance's last frame"
             % (info, info_body),
             "gradients: global rel-L2 %.3e; per-tensor rel-L2 (worst first):  HIP path | the fp64 oracle with ctc_loss in fp32 | tensor | |g|" % glob]
    lines += ["  %.3e  %.3e  %-58s %.3e" % r for r in rows]
    print("\n".join(lines[:8]))
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, "parity_c4_b32_hip_ctc.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    bad = [r for r in rows if r[0] > (2e-1 if r[2].startswith("decoder.") else max(GRAD_TOL_TENSOR, 1.5 * r[1]))]
    assert not bad, "\n".join(lines[:3] + ["outside the bound:"] + ["  %.3e  %.3e  %s" % r[:3] for r in bad])
    med, fmed = sorted(r[0] for r in rows)[len(rows) // 2], sorted(r[1] for r in rows)[len(rows) // 2]
    assert med < max(7e-2, 1.5 * fmed), "\n".join(lines[:12])


@pytest.mark.parametrize("use_graph", [False, True])
def test_joint_trainstep_hip_ctc_follows_refilled_labels_and_clips_the_head(use_graph):
    """tests/test_modules_gpu.py::test_joint_trainstep_follows_refilled_labels_and_clips_the_head for ctc="hip": (1) labels
    refilled in place under an unchanged batch signature train CTC against the new labels - through the single captured graph as
    well; (2) the clip norm covers the model's gradient AND the head's, both scaled by the same coefficient."""
    from st_amd import synthetic
    from st_amd.arena import arena_of
    from st_amd.trainer import JointTrainStep
    from transformer.Loss import CTCAttentionLoss
    from transformer.Models import Transformer
    from transformer.Optim import ScheduledOptim
    from transformer.Utils import AttrDict, init_parameters

    cfg = AttrDict(dict(feature_dim=80, max_inputs_length=200, max_target_length=32, num_enc_layer=2, num_dec_layer=2, n_heads=4,
                        d_k=64, d_v=64, d_model=256, d_inner_hid=512, dropout=0.0, vocab_size=30))
    inputs, targets, in_len, tgt_len, truth = synthetic.make_batch(4, 160, 20, 80, 30, seed=1, t_min=100, l_min=6)
    _, _, _, _, truth2 = synthetic.make_batch(4, 160, 20, 80, 30, seed=7, t_min=100, l_min=6)
    L = truth.shape[1]
    valid = torch.arange(L).view(1, -1) < tgt_len.view(-1, 1)
    labels2 = torch.where(valid, truth2[:, :L].clamp_min(1), torch.zeros_like(truth))       # other labels, the same lengths

    def build(max_norm):
        torch.manual_seed(0)
        model = Transformer(cfg).cuda()
        init_parameters(model)
        model.eval()
        head = CTCAttentionLoss(256, 30, ctc_weight=0.3).cuda()
        head._st_prepare("cuda")
        opt = ScheduledOptim(model, 256, AttrDict(n_warmup_steps=1e9))       # ~zero learning rate: the weights stay put
        hopt = torch.optim.Adam(head.parameters(), lr=1e-12, betas=(0.9, 0.98), eps=1e-9, capturable=True)
        return model, head, JointTrainStep(model, opt, head, max_grad_norm=max_norm, head_optimizer=hopt, use_graph=use_graph,
                                           graph_warmup=1, ctc="hip")

    x, t, gt = inputs.cuda(), targets.cuda(), truth.cuda()
    _, _, step = build(1e9)
    for _ in range(3):
        first = [float(v) for v in step(x, in_len, t, tgt_len, gt)]
    assert len(step.graphs) == (1 if use_graph else 0)
    gt.copy_(labels2)                                   # the loader refills the buffer in place
    for _ in range(2):
        refilled = [float(v) for v in step(x, in_len, t, tgt_len, gt)]
    torch.cuda.synchronize()
    _, _, fresh_step = build(1e9)
    for _ in range(3):
        fresh = [float(v) for v in fresh_step(x, in_len, t, tgt_len, gt)]
    torch.cuda.synchronize()
    assert abs(first[2] - fresh[2]) > 1e-2 * abs(fresh[2]), "the two label sets must differ in their CTC loss"
    assert abs(refilled[2] - fresh[2]) < 2e-3 * abs(fresh[2]), (refilled[2], fresh[2])
    assert abs(refilled[1] - fresh[1]) < 2e-3 * abs(fresh[1])
    # ... and the loss is the truth's for the new labels, on the step's own log-probabilities
    plan = fresh_step._plan
    out = ref.alpha_beta(plan.lp.cpu().numpy(), plan.classes.cpu().numpy(), in_len.numpy(), tgt_len.numpy())
    want = float((out["nll"] / tgt_len.numpy()).mean())
    assert abs(fresh[2] - want) < 1e-4 * abs(want), (fresh[2], want)

    m0, h0, s0 = build(1e9)
    m1, h1, s1 = build(0.05)
    for _ in range(3):
        r0 = s0(x, in_len, t, tgt_len, gt)
        r1 = s1(x, in_len, t, tgt_len, gt)
    torch.cuda.synchronize()
    g_model, g_head = arena_of(m0).grad.double(), torch.cat([h0._st_gw.reshape(-1), h0._st_gb]).double()
    want = float(torch.sqrt((g_model * g_model).sum() + (g_head * g_head).sum()))
    assert abs(float(r0[3]) - want) < 1e-3 * want and abs(float(r1[3]) - want) < 1e-2 * want, (float(r0[3]), float(r1[3]), want)
    coef = 0.05 / (want + 1e-6)
    assert coef < 0.5
    c_head = torch.cat([h1._st_gw.reshape(-1), h1._st_gb]).double()
    assert float((c_head - coef * g_head).norm() / (coef * g_head).norm()) < 2e-2
    assert float((arena_of(m1).grad.double() - coef * g_model).norm() / (coef * g_model).norm()) < 2e-2

"""-m gpu: the label-smoothed cross-entropy kernels (st_ce_smooth_fwd / st_ce_smooth_bwd, csrc/st_loss.hip + st_ce.cuh) against
the fp64 closed form, their plain instantiation against st_ce_fwd / st_ce_bwd bit for bit, and the bodies of
tests/test_label_smoothing_cpu.py on the hardware: TrainStep(criterion=...) eager / captured / in both bucket modes, and the
joint CTC + attention step as one graph."""
import pytest
import torch
import torch.nn as nn

from st_amd import functional as F_
from st_amd import native as nv
from tests import test_label_smoothing_cpu as body
from tests._local import Guarded
from tests.test_kernels_gpu import L_CE, check
from transformer.Loss import LabelSmoothingLoss

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
EPS = body.EPS


def _case(R, V, scale=3.0, seed=3):
    """fp32 logits [R, v_pad + 8] with every column >= V at -1e30; targets with every 5th row ignored and one target V - 1."""
    vp = (V + 7) // 8 * 8
    gen = torch.Generator().manual_seed(seed)
    logits = torch.full((R, vp + 8), -1e30)
    logits[:, :V] = torch.randn(R, V, generator=gen) * scale
    target = torch.randint(1, V, (R,), generator=gen)
    target[::5] = 0
    target[1] = V - 1
    return logits, target, vp, gen


def _closed_form(x64, t, spec, denom, go):
    """fp64: the header's definition, written out with the dense target distribution."""
    R, V = x64.shape
    valid = (t != 0)
    q = torch.full((R, V), spec.smooth, dtype=torch.float64)
    if spec.zero_col >= 0:
        q[:, spec.zero_col] = 0
    q.scatter_(1, t.clamp_min(0).view(-1, 1), spec.confidence)
    q = q * valid.view(-1, 1)
    leaf = x64.clone().requires_grad_(True)
    logp = torch.log_softmax(leaf, -1)
    D = float(valid.sum()) if denom is None else float(denom)
    loss = -(q * logp).sum() / D
    (g,) = torch.autograd.grad(loss * go, leaf)
    nll = -(logp.detach().gather(1, t.view(-1, 1)).squeeze(1) * valid).sum() / valid.sum()
    return float(loss.detach()), float(nll), g


def _run(logits, target, V, vp, spec, denom, go, index=None):
    R = logits.shape[0]
    lg = logits.cuda()
    lse, sums = torch.empty(R, device="cuda"), torch.full((4,), float("nan"), device="cuda")
    d = None if denom is None else torch.tensor([float(denom)], device="cuda")
    nv.ce_smooth_fwd(lg, target.cuda(), 0, spec.confidence, spec.smooth, spec.zero_col, lse, sums, V=V, index=index, denom=d)
    gd = Guarded(R, vp, BF16, "cuda", pad_cols=(0, 0))      # NaN rows around and in the window: every element of dl is the kernel's to write
    dl = gd.view
    nv.ce_smooth_bwd(lg, target.cuda(), 0, spec.confidence, spec.smooth, spec.zero_col, lse, sums, torch.tensor([go], device="cuda"),
                     dl, V=V, index=index, denom=d)
    torch.cuda.synchronize()
    gd.assert_intact("smoothed cross-entropy gradient")
    return lse, sums, dl


@pytest.mark.parametrize("R,V", [(7, 30), (37, 2049), (9, 4337)])
def test_smoothed_kernels_match_the_fp64_closed_form(R, V):
    """30: a partial wave with the padding columns adjacent; 2049: one column into the second 2,048-column trip of the row loop;
    4337: the shipped vocabulary.  Both smoothing specs, with and without a denominator, through target_index, and once with
    logits of magnitude 80."""
    specs = [F_.ce_spec(LabelSmoothingLoss(EPS, V, ignore_index=0), V), F_.ce_spec(nn.CrossEntropyLoss(ignore_index=0, label_smoothing=EPS), V)]
    cases = [(3.0, spec, denom) for spec in specs for denom in (None, R)] + [(None, specs[0], R)]
    for scale, spec, denom in cases:
        logits, target, vp, gen = _case(R, V, scale=3.0 if scale is None else scale)
        if scale is None:          # logits scaled to +-80
            logits[:, :V] *= 80.0 / float(logits[:, :V].abs().max())
        want, want_nll, g = _closed_form(logits[:, :V].double(), target, spec, denom, 0.7)
        lse, sums, dl = _run(logits, target, V, vp, spec, denom, 0.7)
        what = "R %d V %d spec %s denom %s scale %s" % (R, V, tuple(spec), denom, scale)
        print("%s: loss %.7f (fp64 %.7f) nll %.7f (%.7f)" % (what, float(sums[2]), want, float(sums[3]), want_nll))
        assert abs(float(sums[2]) - want) <= 1e-5 * abs(want), (what, float(sums[2]), want)
        assert abs(float(sums[3]) - want_nll) <= 1e-5 * abs(want_nll), (what, float(sums[3]), want_nll)
        assert float(sums[1]) == float((target != 0).sum())
        check(dl[:, :V], g, 6e-3, "smoothed cross-entropy gradient (%s)" % what, tol_local=L_CE)
        assert float(dl[:, V:].float().abs().max()) == 0.0 and float(dl[::5].float().abs().max()) == 0.0
        # through target_index with a permuted padded truth: same kernels, same bits
        idx = torch.randperm(2 * R, generator=gen)[:R]
        truth = torch.zeros(2 * R, dtype=torch.long)
        truth[idx] = target
        lse2, sums2, dl2 = _run(logits, truth, V, vp, spec, denom, 0.7, index=idx.cuda())
        assert torch.equal(lse, lse2) and torch.equal(sums, sums2) and torch.equal(dl, dl2), what


@pytest.mark.parametrize("R,V", [(7, 30), (37, 2049), (9, 4337)])
def test_plain_instantiation_is_the_same_body(R, V):
    """st_ce_smooth_* at (1, 0, -1, NULL) with V = v_pad == st_ce_fwd / st_ce_bwd, bit for bit: one kernel body, one reduction
    order."""
    logits, target, vp, _ = _case(R, V)
    lg, tg = logits.cuda()[:, :vp], target.cuda()          # (a column slice: ldl = v_pad + 8)
    assert lg.stride(0) == vp + 8
    go = torch.tensor([0.7], device="cuda")
    lse0, sums0 = torch.empty(R, device="cuda"), torch.empty(3, device="cuda")
    nv.ce_fwd(lg, tg, 0, lse0, sums0)
    dl0 = torch.empty(R, vp, dtype=BF16, device="cuda")
    nv.ce_bwd(lg, tg, 0, lse0, sums0, go, dl0)
    lse1, sums1 = torch.empty(R, device="cuda"), torch.empty(4, device="cuda")
    nv.ce_smooth_fwd(lg, tg, 0, 1.0, 0.0, -1, lse1, sums1, V=vp)
    dl1 = torch.empty(R, vp, dtype=BF16, device="cuda")
    nv.ce_smooth_bwd(lg, tg, 0, 1.0, 0.0, -1, lse1, sums1, go, dl1, V=vp)
    torch.cuda.synchronize()
    assert torch.equal(lse0, lse1) and torch.equal(sums0, sums1[:3]) and torch.equal(dl0, dl1)
    assert float(sums1[3]) == pytest.approx(float(sums1[2]), rel=1e-6)


def test_cross_entropy_rows_with_a_spec_backpropagates():
    """functional.cross_entropy_rows(spec=..., vocab_size=...) as an autograd node over a padded logits buffer: value and gradient
    against torch's label smoothing; the padding columns get no gradient."""
    R, V = 19, 30
    logits, target, vp, _ = _case(R, V)
    ref_in = logits[:, :V].clone().requires_grad_(True)
    ref = nn.CrossEntropyLoss(ignore_index=0, label_smoothing=EPS)(ref_in, target)
    (ref * 0.7).backward()
    x = logits[:, :vp].contiguous().cuda().requires_grad_(True)
    spec = F_.ce_spec(nn.CrossEntropyLoss(ignore_index=0, label_smoothing=EPS), V)
    loss = F_.cross_entropy_rows(x, target.cuda(), 0, spec=spec, vocab_size=V)
    (loss * 0.7).backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    check(x.grad[:, :V], ref_in.grad, 6e-3, "smoothed cross-entropy gradient through autograd", tol_local=L_CE)
    assert float(x.grad[:, V:].abs().max()) == 0.0 and float(x.grad[::5].abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["ls", "ce"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_smooth_trainstep_vs_oracle_gpu(golden_dir, kind, use_graph):
    body.run_smooth_trainstep_vs_oracle(golden_dir, "cuda", kind, use_graph=use_graph)


@pytest.mark.parametrize("bucket_rows", [None, (340, 48)])
def test_smooth_bucket_modes_one_capture_serves_changing_l_max(bucket_rows):
    body.run_smooth_bucket_mode("cuda", use_graph=True, bucket_rows=bucket_rows)


def test_joint_smooth_step_one_graph_gpu():
    body.run_joint_smooth_step("cuda", use_graph=True, d_model=256, layers=2)

"""CTC forced alignment on the device: WHEN was each token of a transcript spoken.

``align_rows(head, enc_rows, in_rows, labels, label_lengths)`` runs the CTC head over the packed encoder rows (one ``st_gemm``),
gathers the log-probabilities of every utterance's small alphabet (``functional.CtcPlan`` + ``st_ctc_gather``: equal labels
share a class, spans stay per label POSITION) and takes the Viterbi path through the CTC lattice with ONE ``st_ctc_align`` launch
for the batch (csrc/st_ctc_align.hip: one wave per utterance, back-pointers in LDS, a wave-uniform backtrace).  Forward-only.

Rows and time: the alignment is in ENCODER ROWS.  Row t of an utterance stands at raw feature frame ``t * interval`` - with 10 ms
frames at ``t * interval * 10 ms`` - ``interval`` being the frame-stacking stride of ``st_amd.features.stack_frames`` (1 when the
features are not subsampled)."""
import torch

from . import ctc_decode
from . import functional as F_
from . import native as nv

F32, I32, I64 = torch.float32, torch.int32, torch.int64


class Alignment(object):
    """Device tensors of one aligned batch: ``path`` i32 [B, T] (label position of every encoder row, -1 = blank or past the
    utterance), ``spans`` i32 [B, L, 2] ([start, end) rows of label position j; (-1, -1) past a label length), ``score`` f32 [B]
    (log-probability of the best path; -inf: the rows cannot spell the labels - then path and spans are all -1), ``token_logp``
    f32 [B, L] (sum of lp over the token's own rows: a per-token confidence; 0 past a label length, -inf where there is no
    alignment), ``blank_logp`` f32 [B] (the same sum over the blank rows: token_logp.sum(1) + blank_logp = score) and the
    ``plan`` (functional.CtcPlan) that holds lp, classes and the device lengths."""

    __slots__ = ("path", "spans", "score", "token_logp", "blank_logp", "plan")

    def __init__(self, path, spans, score, token_logp, blank_logp, plan):
        self.path, self.spans, self.score, self.token_logp, self.blank_logp, self.plan = path, spans, score, token_logp, blank_logp, plan


@torch.no_grad()
def align_plan(plan):
    """The alignment of the labels of ``plan`` through ``plan.lp`` (already gathered) -> Alignment.  One st_ctc_align launch plus
    a few small torch ops for the per-token sums; the workspace is the plan's (allocated outside any capture)."""
    dev = plan.lp.device
    B, T, L = plan.B, plan.T, plan.L
    ws = plan.align_workspace()
    path = torch.empty(B, T, dtype=I32, device=dev)
    spans = torch.empty(B, L, 2, dtype=I32, device=dev)
    score = torch.empty(B, dtype=F32, device=dev)
    nv.ctc_align(plan.lp, plan.classes, plan.in_len_dev, plan.tgt_len_dev, ws, path, spans, score)
    # per-token confidence: the emission of every row along the path, summed per label position (slot 0 collects the blank
    # rows; rows past a length hold lp = 0 and path = -1, so they add nothing)
    pos = path.to(I64)
    cls = torch.where(pos >= 0, plan.classes.gather(1, pos.clamp_min(0)), torch.zeros_like(pos))
    em = plan.lp.gather(2, cls.unsqueeze(2)).squeeze(2).double()
    sums = torch.zeros(B, L + 1, dtype=torch.float64, device=dev).scatter_add_(1, pos + 1, em)
    none = (score == float("-inf")).unsqueeze(1)
    sums = torch.where(none, torch.full_like(sums, float("-inf")), sums).float()
    return Alignment(path, spans, score, sums[:, 1:].contiguous(), sums[:, 0].contiguous(), plan)


@torch.no_grad()
def align_rows(head, enc_rows, in_rows, labels, label_lengths):
    """head: the ``transformer.Loss.CTCAttentionLoss`` of a joint model; enc_rows bf16 [sum(len), d] + in_rows: the packed encoder
    output (``Encoder.forward_rows``); labels i64 [B, L] vocabulary ids (L <= 255; padding past a length is ignored),
    label_lengths [B] -> Alignment."""
    labels = labels.to(device=enc_rows.device, dtype=I64)
    if labels.dim() != 2 or labels.shape[0] != in_rows.B:
        raise ValueError("align_rows: labels must be [B, L] with B = %d utterances, got %s" % (in_rows.B, tuple(labels.shape)))
    if labels.shape[1] > nv.CTC_LOSS_MAX_L:
        raise ValueError("align_rows: at most %d labels per utterance are supported (got L = %d)" % (nv.CTC_LOSS_MAX_L, labels.shape[1]))
    if labels.shape[1] == 0:                   # (the kernels want at least one label column besides the blank)
        labels = torch.zeros(labels.shape[0], 1, dtype=I64, device=labels.device)
    in_len = in_rows.lens_host if in_rows.lens_host is not None else in_rows.len.cpu()
    logits = ctc_decode.head_logits(head, enc_rows)
    plan = F_.CtcPlan(labels, torch.as_tensor(label_lengths).cpu(), in_len, in_rows, int(head.blank), logits.shape[1])
    lse = torch.empty(logits.shape[0], dtype=F32, device=logits.device)
    nv.ctc_gather(logits, plan.rowmap, plan.T, plan.cols, lse, plan.lp)
    return align_plan(plan)

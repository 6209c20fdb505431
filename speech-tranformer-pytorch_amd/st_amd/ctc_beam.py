"""CTC prefix beam search on the device and the glue of two-pass decoding (CTC n-best, attention rescoring).

``search_rows(head, enc_rows, in_rows, beam)`` runs the CTC head over the packed encoder rows (one ``st_gemm``), takes the
``pre_beam`` best classes of every row's log-softmax (``st_beam_pre_beam``), reads the blank's log-probability off the same
numbers (no further pass over the logits: the row's log-sum-exp is logit(best) - lp(best)) and searches all utterances with ONE
``st_ctc_beam_search`` launch (csrc/st_ctc_beam.hip: one wave per utterance; prefixes are merged by their labels).  The decoder is
never touched.  ``combine`` is the host side of ``Decode.decode_two_pass``: the joint score of every first-pass hypothesis from
its CTC and its teacher-forced attention score, re-sorted.

With ``lm`` (a ``st_amd.ngram.NGramLM`` on the device) and a weight, the search itself ranks by log p_ctc + lambda log p_lm + beta
|h| every frame (``st_ctc_beam_search_lm``: the same single launch); ``NBest.fused`` is then the LM side of the rank,
lambda log p_lm(h . EOS) + beta (|h| + 1) with ``final_eos``, and ``score`` stays the pure log p_ctc."""
import math

import torch

import transformer.Constants as Constants

from . import ctc_decode
from . import native as nv

F32, I32, I64 = torch.float32, torch.int32, torch.int64
MAX_V = 5120              # st_beam_pre_beam's vocabulary limit


class NBest(object):
    """Device tensors of one searched batch: ``tokens`` i32 [B, N, L_cap] (-1 past a length), ``lens`` i32 [B, N], ``score`` f32
    [B, N] - log p_ctc of the label prefix summed over the alignments the search kept; best first, -inf where an utterance has
    fewer than N live prefixes.  ``fused`` f32 [B, N]: None for an LM-less search, else the language-model side of the rank the
    search sorted by (score + fused), -inf in a dead slot."""

    __slots__ = ("tokens", "lens", "score", "fused")

    def __init__(self, tokens, lens, score, fused=None):
        self.tokens, self.lens, self.score, self.fused = tokens, lens, score, fused

    def head(self, N):
        """The N best of every utterance."""
        if N >= self.tokens.shape[1]:
            return self
        return NBest(self.tokens[:, :N].contiguous(), self.lens[:, :N].contiguous(), self.score[:, :N].contiguous(),
                     None if self.fused is None else self.fused[:, :N].contiguous())

    def lists(self):
        """-> (labels[b][j]: the label list of hypothesis j of utterance b, scores: f32 [B, N] on the host).  One host read."""
        B, N, L = self.tokens.shape
        host = torch.cat([self.tokens.reshape(B, N * L).double(), self.lens.double(), self.score.double()], 1).cpu()
        lens = host[:, N * L:N * L + N].long().tolist()
        toks = host[:, :N * L].long().view(B, N, L).tolist()
        return [[toks[b][j][:lens[b][j]] for j in range(N)] for b in range(B)], host[:, N * L + N:].float()


def check_widths(V, beam, pre_beam=None, n_best=None):
    """-> (beam, K, N) of a search over a vocabulary of V classes; ValueError on a bad combination."""
    beam = int(beam)
    K = beam if pre_beam is None else int(pre_beam)
    N = beam if n_best is None else int(n_best)
    if V > MAX_V:
        raise ValueError("ctc_beam: vocabularies above %d classes are not supported (got %d)" % (MAX_V, V))
    if not 1 <= beam <= nv.CTC_BEAM_MAX:
        raise ValueError("ctc_beam: beam must lie in [1, %d], got %d" % (nv.CTC_BEAM_MAX, beam))
    if not 1 <= K <= nv.CTC_BEAM_MAX:
        raise ValueError("ctc_beam: pre_beam must lie in [1, %d], got %d" % (nv.CTC_BEAM_MAX, K))
    if K > V:
        raise ValueError("ctc_beam: pre_beam %d exceeds the vocabulary %d" % (K, V))
    if not 1 <= N <= beam:
        raise ValueError("ctc_beam: n_best must lie in [1, beam] = [1, %d], got %d" % (beam, N))
    return beam, K, N


def label_capacity(t_max, max_len=None):
    """L_cap of a search: an utterance of T rows spells at most T labels; the kernel holds 255."""
    cap = nv.CTC_LOSS_MAX_L if max_len is None else int(max_len)
    if not 1 <= cap <= nv.CTC_LOSS_MAX_L:
        raise ValueError("ctc_beam: max_len must lie in [1, %d], got %d" % (nv.CTC_LOSS_MAX_L, cap))
    return max(1, min(cap, int(t_max)))


def check_lm(lm, lm_weight, lm_length_bonus, V=None, device=None, who="ctc_beam"):
    """-> (lambda, beta, fused: whether the search runs with the model); ValueError for a weight < 0 / not finite, a weight without
    ``lm``, or a model that does not fit (vocabulary, device)."""
    lam = float(lm_weight or 0.0)
    beta = float(lm_length_bonus or 0.0)
    if not lam >= 0.0 or not math.isfinite(lam) or not math.isfinite(beta):
        raise ValueError("%s: lm_weight must be a finite number >= 0 (got %r), lm_length_bonus finite (got %r)" % (who, lam, beta))
    if lam == 0.0 and beta == 0.0:
        return lam, beta, False
    if lm is None:
        raise ValueError("%s: lm_weight %r / lm_length_bonus %r need a language model (lm=...)" % (who, lam, beta))
    if lm.trie is None:
        raise ValueError("%s: the language model has no device trie - pass lm.to(device)" % who)
    if V is not None and lm.V != V:
        raise ValueError("%s: the language model's vocabulary %d differs from the head's %d" % (who, lm.V, V))
    if device is not None and torch.device(lm.trie.device).type != torch.device(device).type:
        raise ValueError("%s: the language model lives on %s, the rows on %s - pass lm.to(device)" % (who, lm.trie.device, device))
    return lam, beta, True


@torch.no_grad()
def search_logits(logits, V, in_rows, blank, beam, K, L_cap, lm=None, lm_weight=0.0, lm_length_bonus=0.0, final_eos=True):
    """The search over the head's logits f32 [R, >= V] -> NBest with N = beam.  ``lm`` + ``lm_weight`` (lambda) / ``lm_length_bonus``
    (beta): the fused search; without a model, or with both 0, the launches are the LM-less ones."""
    lam, beta, fuse = check_lm(lm, lm_weight, lm_length_bonus, V, logits.device)
    dev, R, B = logits.device, logits.shape[0], in_rows.B
    ids = torch.empty(R, K, dtype=I32, device=dev)
    lp = torch.empty(R, K, dtype=F32, device=dev)
    nv.beam_pre_beam(logits, V, ids, lp)
    best = logits.gather(1, ids[:, :1].to(I64)).squeeze(1)
    lpb = (logits[:, int(blank)] - (best - lp[:, 0])).contiguous()
    tokens = torch.empty(B, beam, L_cap, dtype=I32, device=dev)
    lens = torch.empty(B, beam, dtype=I32, device=dev)
    score = torch.empty(B, beam, dtype=F32, device=dev)
    if not fuse:
        nv.ctc_beam_search(ids, lp, lpb, in_rows.off, in_rows.len, blank, tokens, lens, score)
        return NBest(tokens, lens, score)
    fused = torch.empty(B, beam, dtype=F32, device=dev)
    nv.ctc_beam_search_lm(ids, lp, lpb, in_rows.off, in_rows.len, blank, tokens, lens, score, lm.trie, Constants.BOS, Constants.EOS,
                          lam, beta, fused, final_eos=final_eos)
    return NBest(tokens, lens, score, fused)


@torch.no_grad()
def search_rows(head, enc, in_rows, beam, pre_beam=None, n_best=None, max_len=None, lm=None, lm_weight=0.0, lm_length_bonus=0.0,
                final_eos=True):
    """head: the ``transformer.Loss.CTCAttentionLoss`` of a joint model; enc bf16 [sum(len), d] + in_rows: the packed encoder
    output (``Encoder.forward_rows``) -> NBest of the ``n_best`` (default ``beam``) best label prefixes per utterance.
    ``pre_beam`` (default ``beam``): classes considered per row; ``max_len``: label capacity (default min(255, longest utterance)).
    ``lm``, ``lm_weight``, ``lm_length_bonus``, ``final_eos``: the n-gram model fused into the search (default: off)."""
    V = head.ctc_proj.weight.shape[0]
    beam, K, N = check_widths(V, beam, pre_beam, n_best)
    L_cap = label_capacity(in_rows.max_len, max_len)
    check_lm(lm, lm_weight, lm_length_bonus, V, enc.device)                     # (before any launch)
    out = search_logits(ctc_decode.head_logits(head, enc), V, in_rows, int(head.blank), beam, K, L_cap, lm, lm_weight, lm_length_bonus,
                        final_eos)
    return out.head(N)


def combine(hyps, ctc_scores, att_scores, weight, n_best, eos, extra=None):
    """Second-pass ranking on the host.  hyps[b][j]: label lists (no EOS); ctc_scores, att_scores: [B, N] - the first pass' log
    p_ctc(h) and the teacher-forced log p_att(h . EOS); a missing hypothesis has -inf in either.  Final score
    (1 - w) att + w ctc (w = 0: the attention score alone), sorted best first (the first pass' order on ties), the ``n_best`` kept
    -> (all_hyp with EOS closing every list, scores f32 [B, n_best]); a slot without a hypothesis: ([], -inf).  ``extra``: None, or
    [B, N] added to the final score of every present hypothesis (the language-model term of shallow fusion; -inf there vetoes)."""
    w = float(weight)
    if not 0.0 <= w < 1.0:
        raise ValueError("decode_two_pass: ctc_weight must lie in [0, 1), got %r" % w)
    ctc = torch.as_tensor(ctc_scores).double().cpu()
    att = torch.as_tensor(att_scores).double().cpu()
    B, N = ctc.shape
    if tuple(att.shape) != (B, N) or len(hyps) != B or not 1 <= int(n_best) <= N:
        raise ValueError("decode_two_pass: %d x %d first-pass scores, second-pass %s, %d lists, n_best %d"
                         % (B, N, tuple(att.shape), len(hyps), n_best))
    ninf = torch.full_like(ctc, float("-inf"))
    missing = torch.isinf(ctc) | torch.isinf(att) | torch.isnan(att)
    final = (1.0 - w) * att + (w * ctc if w > 0.0 else 0.0)
    if extra is not None:
        extra = torch.as_tensor(extra).double().cpu()
        if tuple(extra.shape) != (B, N):
            raise ValueError("decode_two_pass: the extra term is %s for %d x %d hypotheses" % (tuple(extra.shape), B, N))
        final = final + torch.where(missing, torch.zeros_like(extra), extra)
    final = torch.where(missing, ninf, final)
    order = torch.sort(final, dim=1, descending=True, stable=True)[1][:, :int(n_best)]
    all_hyp = []
    for b in range(B):
        row = []
        for j in order[b].tolist():
            row.append([] if bool(missing[b, j]) else [int(k) for k in hyps[b][j]] + [int(eos)])
        all_hyp.append(row)
    return all_hyp, final.gather(1, order).float()

"""Forward-only validation: teacher-forced dev-set loss, NLL and token accuracy on the HIP path, as one callable.

What a recipe reports per epoch - and picks checkpoints, stops early and chooses between raw and averaged weights by - is the
criterion's value, the plain token-mean NLL (perplexity) and the share of positions whose arg-max is the ground truth, all
under teacher forcing.  ``EvalStep`` computes them on the path a training step takes (the shared driver pieces - bucket staging,
capture, replay - are st_amd/stepdriver.py): ``model.forward_packed`` leaves the
logits in the ragged ``[rows, v_pad]`` layout, ``st_ce_eval_fwd`` reads every row once (loss numerator, NLL, arg-max hit) and
``st_eval_note`` adds the batch into an fp64 accumulator in device memory.  Nothing is scattered to ``[B, L, V]``, nothing is
saved for a backward, the optimizer and the dropout seed are never touched, and the host reads ONE tensor per pass::

    ev = EvalStep(model, vocab_size, criterion=None, use_graph=True, bucket=(T_cap, L_cap), bucket_rows=None)
    model.eval()
    with optimizer.averaged():            # optional: TrainStep refuses this context, EvalStep works inside it
        ev.reset()
        for inputs, input_lengths, targets, target_lengths, ground_truth in dev_loader:
            ev(inputs, input_lengths, targets, target_lengths, ground_truth)     # no host read; returns ev.last
        r = ev.result()                   # dict(loss, nll, ppl, accuracy, tokens, batches, bad_targets)

Data parallelism: every rank evaluates its shard, then ``torch.distributed.all_reduce(ev.acc, op=SUM)`` before ``result()``.
"""
from __future__ import annotations

import math

import torch

from . import native as nv
from .functional import ce_spec
from .stepdriver import (LossDenom, bucket_step, capture_kwargs, no_gc_inside_capture, parse_buckets, prepare_capture,
                         stage_bucket, trim_batch, zero_tails)


class _Cap:
    __slots__ = ("graph", "keep")


class EvalStep:
    def __init__(self, model, vocab_size: int, criterion=None, use_graph: bool = True, bucket=None, bucket_rows=None,
                 graph_warmup: int = 1):
        """criterion: what ``TrainStep`` accepts - None = ``nn.CrossEntropyLoss(ignore_index=0)``, the same with
        ``label_smoothing``, or ``transformer.Loss.LabelSmoothingLoss`` (functional.ce_spec; ValueError HERE for anything else).
        ``loss`` is the criterion's value over the pass (numerators and denominators summed over the batches: token counts, the
        ``B * l_max`` rows of every trimmed batch for LabelSmoothingLoss's mean, 1 per batch for its sum); ``nll`` and
        ``accuracy`` do not depend on the criterion.

        use_graph=True needs ``bucket=(T_cap, L_cap)``: a dev set never repeats a length signature, so a capture per
        signature would never be replayed.  The bucket capture is ONE forward-only graph over static padded buffers with the
        lengths on the device; bucket_rows = (input rows, target rows) or an ascending list of them packs the layouts
        (``TrainStep`` documents both).  The first ``graph_warmup`` batches of a bucket run eagerly.

        The model must be in ``eval()`` mode - every module of it: a call with dropout or SpecAugment live raises RuntimeError.
        ``self.acc``: fp64 [8] on the device (st_eval_note lists the slots), ``self.last``: f32 [4] = the last batch's
        (loss, nll, accuracy, tokens).  A target outside the vocabulary that is not PAD does not abort anything: its row is
        left out and counted in ``bad_targets``."""
        if not hasattr(model, "forward_packed"):
            raise ValueError("EvalStep: needs a model with forward_packed (the HIP path)")
        self.model, self.vocab_size = model, int(vocab_size)
        spec = ce_spec(criterion, vocab_size)
        self.norm = "tokens" if spec is None else spec.norm
        self._triple = (1.0, 0.0, -1) if spec is None else (float(spec.confidence), float(spec.smooth), int(spec.zero_col))
        if use_graph and bucket is None:
            raise ValueError("EvalStep: use_graph=True needs bucket=(T_cap, L_cap) - the batches of a dev set do not repeat a "
                             "length signature, so only a bucket capture is ever replayed (or pass use_graph=False)")
        self.use_graph, self.graph_warmup = bool(use_graph), int(graph_warmup)
        self.bucket, self.bucket_rows = parse_buckets("EvalStep", bucket, bucket_rows)
        self._buckets = {}
        self.acc = self.last = None
        self._denom = LossDenom()       # the loss denominator of a "rows" / "sum" criterion, staged per batch

    # ---- device state -----------------------------------------------------------------------------------------------------
    def _state(self, device) -> None:
        """The accumulator and the per-batch results: created once (captured graphs hold their addresses), zeroed in place."""
        if self.acc is None:
            self.acc = torch.zeros(8, dtype=torch.float64, device=device)
            self.last = torch.zeros(4, dtype=torch.float32, device=device)
        elif self.acc.device != device:
            raise RuntimeError("EvalStep: the accumulator lives on %s, this batch on %s" % (self.acc.device, device))

    def reset(self) -> None:
        """A new pass: the accumulator back to zero, in place."""
        if self.acc is not None:
            self.acc.zero_()
            self.last.zero_()

    def result(self) -> dict:
        """The pass so far - the one host read."""
        if self.acc is None:
            a = [0.0] * 8
        else:
            a = self.acc.cpu().tolist()
        nan = float("nan")
        nll = a[2] / a[3] if a[3] else nan
        ppl = nan if nll != nll else (math.exp(nll) if nll < 700.0 else float("inf"))
        return dict(loss=a[0] / a[1] if a[1] else nan, nll=nll, ppl=ppl,
                    accuracy=a[4] / a[3] if a[3] else nan, tokens=int(a[3]), batches=int(a[5]), bad_targets=int(a[6]))

    # ---- one batch ----------------------------------------------------------------------------------------------------------
    def _forward(self, inputs, input_lengths, targets, target_lengths, ground_truth, layouts=None):
        zero_tails()
        with torch.no_grad():
            # the whole [rows, v_pad] buffer, padding columns at -1e30; the kernel reads the first vocab_size columns
            logits, t_rows = self.model.forward_packed(inputs, input_lengths, targets, target_lengths, padded_logits=True,
                                                       layouts=layouts)
            # (a 1-D ground truth is the padded [B, L_cap] one flattened, with a spare ignored element behind it for the
            # rows a packed bucket leaves unassigned: stepdriver.stage_bucket)
            L_gt = ground_truth.shape[1] if ground_truth.dim() == 2 else t_rows.max_len
            rows = torch.empty(logits.shape[0], 4, dtype=torch.float32, device=logits.device)
            c, s, z = self._triple
            nv.ce_eval_fwd(logits, ground_truth.contiguous().view(-1), 0, c, s, z, rows, V=self.vocab_size,
                           index=t_rows.scatter_index(L_gt))
            nv.eval_note(rows, self.acc, self.last, denom=self._denom.tensor)
        return self.last

    def _capture(self, batch, layouts):
        prepare_capture(batch[0].device)
        with no_gc_inside_capture():
            cap = _Cap()
            cap.graph = torch.cuda.CUDAGraph()
            # the captured kernels read the layouts and the staging buffers by address (the served tail buffers: the bucket's)
            cap.keep = (layouts, batch[0], batch[2], batch[4])
            with torch.cuda.graph(cap.graph, pool=torch.cuda.graph_pool_handle(), **capture_kwargs()):
                self._forward(*batch, layouts=layouts)
        return cap          # capture only records: the replay that follows runs the batch

    def __call__(self, inputs, input_lengths, targets, target_lengths, ground_truth):
        """inputs [B, T, F] / targets, ground_truth [B, L] on the GPU; lengths on host or GPU -> ``self.last`` (device f32 [4]:
        this batch's loss, nll, accuracy, tokens), and the batch is added into ``self.acc``."""
        if any(m.training for m in self.model.modules()):
            raise RuntimeError("EvalStep: the model (or one of its modules) is in training mode - dropout and SpecAugment would "
                               "mask the validation pass; call model.eval() first")
        batch = trim_batch(inputs, input_lengths, targets, target_lengths, ground_truth)
        self._state(inputs.device)
        self._denom.stage(self.norm, batch[4].shape[0], batch[4].shape[1], inputs.device)
        if self.bucket is None:
            return self._forward(*batch)
        st, batch, packed = stage_bucket("EvalStep", self.model, self._buckets, self.bucket, self.bucket_rows, *batch)
        if not self.use_graph:
            return self._forward(*batch, layouts=st.layouts)
        return bucket_step(st, packed, self.graph_warmup, lambda: self._forward(*batch, layouts=st.layouts),
                           lambda: self._capture(batch, st.layouts), self._replay, serve_tails=True)

    def _replay(self, cap):
        cap.graph.replay()
        return self.last

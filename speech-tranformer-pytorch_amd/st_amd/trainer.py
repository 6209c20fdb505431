"""The training step of the reference's ``train()`` loops, as one callable.

Sequence (train.py:25-46 / train_multi.py:47-68): trim the batch to its longest
utterance, zero_grad, forward, ``CrossEntropyLoss(ignore_index=0)`` over
``logits.view(-1, V)`` vs ``ground_truth.view(-1)``, backward, [gradient average
over ranks], global-norm clip, Noam-Adam update.  The per-step ``.item()`` syncs of
the reference (train.py:31-32,42) are not reproduced: lengths are taken on the host
(where the loader produced them) and the loss / grad-norm come back as device tensors.

HIP-graph mode (``use_graph=True``): the step launches ~190 kernels; the decoder half
(M ~ 1.2k rows) is launch-bound from Python (~10 us of host time per launch vs 2-4 us of
GPU time).  The step is therefore captured per batch SIGNATURE (same tensors, same length
vectors) into a HIP graph and replayed; the Noam rate is a device scalar updated before each
replay.  Up to ``max_graphs`` signatures are kept (default 4; least recently used evicted; every
signature owns a private memory pool with a full step of activations - ~5 GB at config 2 -
so the cap is a memory bound), each with its own memory pool and with references to the ragged layouts its kernels read by address,
so a loader that cycles through a set of pre-collated batches (bench.py; an epoch over a
bucketed, cached dataset) replays, and one whose length vectors never repeat runs the eager
path - whose ms/step bench.py reports next to the replay figure.  With data parallelism the
backward is cut at the encoder output: forward + loss + decoder backward | encoder backward |
clip+Adam.  The decoder's and the vocabulary projection's gradients (the tail ~2/3 of the flat
buffer) are final after the first part, so their RCCL all-reduce runs while the encoder's
backward - ~40 % of the step - is executing.  The bucket all-reduces are captured INSIDE the
step graph (``dp_in_graph``; RCCL collectives are stream-capturable), so a DP step is one graph
replay; where that capture is refused the three parts become three graphs with eager
collectives between them.

Gradient accumulation (``TrainStep(..., accumulate=K)``): K calls are K micro-batches of ONE update whose objective is what one
step on their concatenation would compute.  Every micro-batch adds the gradient of its SUM loss into the flat buffer; the
denominator (the window's token count, say) is summed on the device and applied once, inside the norm and the clip + Adam
kernels of the update (st_grad_norm, st_adam_clip with their win pointer) - no host read, and the update kernel leaves the buffer zeroed for
the next window.  In graph mode the micro-batch and the update are two captures.

What the drivers here share with each other and with the validation driver - batch trimming and signatures, the loss
denominator, the preparation of a capture, bucket staging and the bucket's warm-up / capture / replay runner - is
st_amd/stepdriver.py; this file keeps each driver's own policy (and re-exports the names tests and tools import from here).
"""
from __future__ import annotations

import collections
import os
import time
from typing import Optional

import torch
import torch.distributed
import torch.nn as nn

from .arena import arena_of
from .dp import GradReducer
from . import rng
from . import native as nv
from .functional import CeSpec, ce_spec, deferred_wgrads
from .stepdriver import (LossDenom, _Bucket, batch_signature, bucket_step, capture_kwargs,  # noqa: F401  (re-exported)
                         no_gc_inside_capture, optimizer_options, parse_buckets, prepare_capture, stage_bucket, trim_batch,
                         zero_tails)


def clip_grad_norm_flat(arena, max_norm: float) -> torch.Tensor:
    """``nn.utils.clip_grad_norm_`` (train.py:45) over the flat gradient buffer: one
    reduction + one scale instead of a pass per tensor; padding elements are zero."""
    total = torch.linalg.vector_norm(arena.grad)
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    arena.grad.mul_(coef)
    return total


class TrainStep:
    def __init__(self, model: nn.Module, optimizer, vocab_size: int, max_grad_norm: float,
                 reducer: Optional[GradReducer] = None, use_graph: bool = False, graph_warmup: int = 2,
                 max_graphs: int = 4, bucket=None, dp_in_graph: bool = True, bucket_rows=None, criterion=None,
                 accumulate: Optional[int] = None):
        """criterion: None = ``nn.CrossEntropyLoss(ignore_index=0)`` (train.py:120); or ``nn.CrossEntropyLoss(ignore_index=0,
        label_smoothing=e)`` / ``transformer.Loss.LabelSmoothingLoss(e, vocab_size, ignore_index=0)`` - label smoothing inside
        the same projection + loss node and the same captured graph (functional.ce_spec maps the object to the kernels and
        raises ValueError HERE for one the HIP path cannot honour: class weights, another reduction or ignore_index, any
        other module).  ``self.nll`` holds the plain token-mean NLL of the last step as a device scalar - the number that
        stays comparable across smoothing values (with the plain criterion: the loss itself).

        The optimizer's options (``ScheduledOptim.enable_nonfinite_guard`` / ``enable_averaging``) need no argument here: the
        step reads the optimizer.  A captured step holds the launches of the options as they were at capture - after a change
        the next call raises RuntimeError - and a call inside ``optimizer.averaged()`` raises RuntimeError (the model holds
        the averaged weights).  A SKIPPED step (non-finite gradient norm under the guard) is still a call: the Noam rate
        follows the host's ``global_step``, which counts calls, while Adam's bias corrections follow the device step count,
        which counts applied updates.  Data parallelism needs nothing: the norm is taken after the all-reduce, so every rank
        reaches the same verdict.

        accumulate: None or 1 = every call is a step (the code and the launches above).  K >= 2 = gradient accumulation: every
        call is one MICRO-BATCH (forward, loss, backward adding into the flat gradient buffer) and the K-th call of a window
        also applies the update; :meth:`flush` applies it to a partly filled window (the end of an epoch).  The window's
        objective is the criterion on the concatenation of its micro-batches: each contributes the SUM of its row losses and the
        update divides once by the summed denominators - non-ignored tokens (``nn.CrossEntropyLoss``), ``B * l_max`` of every
        trimmed micro-batch (``LabelSmoothingLoss``'s mean), 1 (its sum) - which live on the device; averaging per-micro-batch
        means instead is NOT the gradient of the large batch when token counts differ.  The call returns ``(loss, grad_norm)``:
        this micro-batch's loss in its own normalisation (comparable with a non-accumulating step's) and the norm of the most
        recent update (0 before the first).  ``self.updated``: this call applied - or, under the guard, skipped - an update;
        ``self.window_loss`` / ``self.window_nll``: device scalars written when a window closes; ``self.nll`` stays per
        micro-batch.  ``global_step`` and the Noam rate advance per UPDATE; dropout and SpecAugment masks are drawn per call.
        Under the non-finite guard a non-finite accumulated norm or a window without a single token skips the WHOLE window
        (``skipped`` counts one) and the next window starts clean.  After an update the flat gradient buffer holds ZEROS, not the
        clipped gradient (the update kernel is the next window's zero_grad).  Data parallelism: nothing is exchanged on
        non-final micro-batches; at the update the gradient sums and the window's sums are all-reduced (SUM), so the update is the
        token mean over all ranks and micro-batches - unlike the non-accumulating DP step, which averages the ranks' means as
        Horovod does.  Needs ``model.forward_packed`` and the optimizer's flat arena (ValueError otherwise)."""
        self.model, self.optimizer = model, optimizer
        self.vocab_size, self.max_grad_norm = vocab_size, max_grad_norm
        self.crit = criterion or nn.CrossEntropyLoss(ignore_index=0)          # train.py:120
        # resolved once: a model without forward_packed runs self.crit itself on the padded logits (any criterion will do)
        self.ce_spec = ce_spec(criterion, vocab_size) if hasattr(model, "forward_packed") else None
        # the denominator of a CeSpec with norm "rows" (B * l_max of the trimmed batch) / "sum" (1): a persistent device
        # scalar the kernels read at run time (stepdriver.LossDenom; read back as self._ce_denom)
        self._denom = LossDenom()
        self.nll = None
        self.reducer = reducer
        self.global_step = 0
        self.use_graph, self.graph_warmup, self.max_graphs = use_graph, graph_warmup, max_graphs
        # data parallelism in graph mode: the bucket all-reduces are CAPTURED with the step (RCCL collectives are
        # stream-capturable: ProcessGroupNCCL forks its stream off the capturing one and joins it again in wait()), so a DP
        # step is ONE graph replay with no host in the loop; False (or a capture that fails) = three graphs with eager
        # collectives in between
        self.dp_in_graph = dp_in_graph
        self.dp_mode = None                            # "in-graph" / "split" after the first DP capture (introspection)
        # bucket = (T_cap, L_cap): ONE captured step serves every batch of B utterances with at most T_cap frames and L_cap
        # target tokens - the batch is staged into static padded buffers, the lengths live on the device (Rows.bucket), so
        # a loader whose batches never repeat a length signature still replays a graph.  Costs the padding rows
        # (B * T_cap instead of sum(len) rows through the row-wise kernels): for length-bucketed loaders.
        # bucket_rows = (input rows, target rows): the bucket's layouts are PACKED into that many rows (Rows.bucket(rows=...)) -
        # offsets on the device as well - so the captured step runs over about the batch's real row count instead of
        # B * T_cap.  Several capacities may be given, [(rows, rows), ...] in ascending order: a batch takes the first one it
        # fits (one capture each); a batch with more rows than the largest takes the padded bucket.  Pick the capacities
        # from the loader's length statistics AND the kernels' tile rounds: the encoder-sized row chains run one 96-row
        # workgroup per CU, so 256 x 96 = 24,576 rows are one round and 24,577 are two (of 64-row workgroups: up to 32,768).
        self.bucket, self.bucket_rows = parse_buckets("TrainStep", bucket, bucket_rows)
        self._buckets = {}
        self._graphs = collections.OrderedDict()      # signature -> captured step (LRU)
        self._seen = collections.OrderedDict()        # signature -> eager sightings before the capture
        self._g_fb = self._g_enc = self._g_opt = None
        self._loss = self._gnorm = None
        self._cut = None
        self._seed = None
        # gradient accumulation: None = off (accumulate=None / 1 take the code above unchanged)
        if accumulate is not None and (isinstance(accumulate, bool) or int(accumulate) != accumulate or int(accumulate) < 1):
            raise ValueError("TrainStep: accumulate must be None or an int >= 1, got %r" % (accumulate,))
        self.accumulate = None if accumulate is None or int(accumulate) == 1 else int(accumulate)
        self.updated = False
        self.window_loss = self.window_nll = None
        if self.accumulate is not None:
            if not hasattr(model, "forward_packed"):
                raise ValueError("TrainStep(accumulate=%d): needs a model with forward_packed (the HIP loss path)" % self.accumulate)
            if getattr(optimizer, "arena", None) is None or not hasattr(optimizer, "_step_window"):
                raise ValueError("TrainStep(accumulate=%d): needs an optimizer with the flat arena (ScheduledOptim over a model "
                                 "on the GPU)" % self.accumulate)
            # every micro-batch runs the smoothed kernels with a device denominator of 1.0: the SUM of its row losses
            # (CeSpec(1, 0, -1) is the plain criterion: one kernel body with st_ce_fwd / st_ce_bwd)
            self._acc_norm = "tokens" if self.ce_spec is None else self.ce_spec.norm
            self._acc_spec = CeSpec(1.0, 0.0, -1, "sum") if self.ce_spec is None else self.ce_spec._replace(norm="sum")
            self._win = self._win_out = self._win_rows = None      # device state: _stage_window
            self._win_rows_host = None
            self._n_acc = 0                                          # micro-batches in the open window (the host counts calls)
            self._loads = getattr(optimizer, "_state_loads", 0)
            self._last_cap = None
            if reducer is not None:
                reducer.detach()                                     # nothing is exchanged before the update

    def _options(self):
        return optimizer_options(self.optimizer, type(self).__name__)

    @property
    def _ce_denom(self):
        return self._denom.tensor

    def _backward(self, loss):
        """loss.backward() with a resident gradient seed (autograd's own ones_like(loss) is a fill launch per step)."""
        if self._seed is None or self._seed.device != loss.device or self._seed.dtype != loss.dtype:
            self._seed = torch.ones((), dtype=loss.dtype, device=loss.device)
        torch.autograd.backward(loss, grad_tensors=self._seed)

    # ---- gradient accumulation ----------------------------------------------------------------------
    def _stage_window(self, B: int, l_max: int, device) -> None:
        """The window's device state, created on the first call (never inside a capture), and this micro-batch's share of a
        "rows" denominator.  A fresh window starts with one eager zero_grads: here, and after optimizer.load_state_dict()."""
        loads = getattr(self.optimizer, "_state_loads", 0)
        if self._win is None or self._win.device != device or loads != self._loads:
            if self._win is None or self._win.device != device:
                self._win = torch.zeros(4, dtype=torch.float32, device=device)        # denominator, loss sum, NLL sum, micro-batches
                self._win_out = torch.zeros(4, dtype=torch.float32, device=device)    # what st_window_close leaves
                self._denom.tensor = torch.ones(1, dtype=torch.float32, device=device)    # the kernels' denominator: always 1
                self._gnorm = torch.zeros((), dtype=torch.float32, device=device)
                self.window_loss, self.window_nll = self._win_out[0], self._win_out[1]
                self._win_rows, self._win_rows_host = None, None
            self._win.zero_()
            arena_of(self.model).zero_grads()
            self._n_acc, self._loads = 0, loads
        if self._acc_norm == "rows":
            d = float(B * l_max)
            if self._win_rows is None:
                self._win_rows = torch.full((1,), d, dtype=torch.float32, device=device)
            elif d != self._win_rows_host:
                self._win_rows.fill_(d)
            self._win_rows_host = d

    def _micro_batch(self, inputs, input_lengths, targets, target_lengths, ground_truth, layouts=None):
        """One micro-batch of a window: forward, SUM loss, its note in the window, backward ADDING into the flat buffer (no
        zero_grad, no update) -> this micro-batch's loss in its own normalisation."""
        zero_tails()
        rng.advance()
        loss, _ = self.model.forward_packed(inputs, input_lengths, targets, target_lengths, ce_truth=ground_truth, ignore_index=0,
                                            layouts=layouts, ce_spec=self._acc_spec, ce_denom=self._ce_denom)
        self.nll = self.model._st_ce_nll
        sums = self.model._st_ce_sums
        d = sums[1:2] if self._acc_norm == "tokens" else (self._win_rows if self._acc_norm == "rows" else None)
        out = nv.accum_note(sums, d, self._win, torch.empty(1, dtype=torch.float32, device=sums.device))
        with deferred_wgrads(True):
            self._backward(loss)
        return out[0]

    def _window_update(self):
        """Norm + clip + Adam over the window's sum divided by its denominator, then the window's results and a fresh window.
        (Across ranks the sums were all-reduced, denominator included: nothing is left to scale.)"""
        gnorm = self.optimizer.step_captured(grad_norm=True, max_norm=self.max_grad_norm, grad_scale=1.0, window=self._win)
        nv.window_close(self._win, self._win_out)
        return gnorm

    def _close_window(self):
        self.global_step += 1
        self.optimizer.update_learning_rate(self.global_step)
        red = self.reducer
        if red is not None and red.active:
            red.reduce_all(divide=False)             # the rank SUM of the gradient sums ...
            if red.world > 1:                        # ... and of (denominator, loss sum, NLL sum): the mean over all ranks' tokens.
                torch.distributed.all_reduce(self._win[:3], op=torch.distributed.ReduceOp.SUM, group=red.group)
                # (norm "sum": win[0] = 1 on every rank adds up to the world size - the rank average of the sums)
        self._apply_window()

    def _apply_window(self):
        """The update of the open window: the captured one behind a replayed micro-batch, else eager."""
        cap = self._last_cap
        if cap is not None:
            cap.g_opt.replay()
            self._gnorm = cap.gnorm
        else:
            self._gnorm = self._window_update()
        self._n_acc, self.updated = 0, True

    def flush(self):
        """Apply the update to a partly filled window (the end of an epoch); a no-op when nothing has been accumulated (and
        without ``accumulate``).  -> (window_loss, grad_norm) or None."""
        if self.accumulate is None or self._n_acc == 0:
            return None
        self._options()
        self._close_window()
        return self.window_loss, self._gnorm

    def _accumulate_call(self, batch, raw):
        self.updated = False
        loss, _ = self._dispatch(batch, raw)
        self._n_acc += 1
        if self._n_acc >= self.accumulate:
            self._close_window()
        return loss, self._gnorm

    # ---- the two halves of a step -------------------------------------------------------------
    def _single_graph(self) -> bool:
        """The whole step is captured as ONE graph (no data-parallel split into several captures that share a memory pool)."""
        split = self.reducer is not None and self.reducer.active and hasattr(self.model, "forward_packed") \
            and hasattr(self.model, "encoder")
        return not split or self.dp_in_graph or self.accumulate is not None      # (a micro-batch is always one graph)

    def _forward_backward(self, inputs, input_lengths, targets, target_lengths, ground_truth, captured=False, layouts=None):
        zero_tails()
        self.optimizer.zero_grad()
        rng.advance()                          # next step's dropout masks (an in-place device add: capturable)
        if layouts is not None:
            loss, _ = self.model.forward_packed(inputs, input_lengths, targets, target_lengths, ce_truth=ground_truth,
                                                ignore_index=0, layouts=layouts, ce_spec=self.ce_spec,
                                                ce_denom=self._ce_denom)
            self.nll = self.model._st_ce_nll
        elif hasattr(self.model, "forward_packed"):
            # loss over the valid tokens only: the kernels' ragged logits rows against the matching ground-truth
            # entries.  Identical to train.py:40 on the padded [B, L, V] tensor: its padded positions carry
            # ground truth 0 = ignore_index, and the mean is over non-ignored tokens either way.
            # (projection + cross-entropy as one autograd node: functional.VocabCeFn)
            # (ce_spec has made sure that the ignored index is 0 = PAD, with or without label smoothing)
            loss, t_rows = self.model.forward_packed(inputs, input_lengths, targets, target_lengths, ce_truth=ground_truth,
                                                     ignore_index=0, ce_spec=self.ce_spec, ce_denom=self._ce_denom)
            self.nll = self.model._st_ce_nll
        else:
            logits, _ = self.model(inputs, input_lengths, targets, target_lengths)
            loss = self.crit(logits.contiguous().view(-1, self.vocab_size), ground_truth.contiguous().view(-1))
            self.nll = loss.detach()
            if not isinstance(self.crit, nn.CrossEntropyLoss) or self.crit.label_smoothing:
                with torch.no_grad():
                    self.nll = nn.functional.cross_entropy(logits.contiguous().view(-1, self.vocab_size),
                                                           ground_truth.contiguous().view(-1), ignore_index=0)
        # the decoder's weight gradients are deferred into one grouped launch - unless eager gradient-ready hooks
        # are live (they assume a weight gradient is enqueued when its layer's backward returns)
        hooks_live = self.reducer is not None and not captured
        with deferred_wgrads(not hooks_live):
            self._backward(loss)
        return loss.detach()

    # ---- data-parallel graph mode: the backward in two captures -----------------------------------
    def _forward_decoder_backward(self, inputs, input_lengths, targets, target_lengths, ground_truth, layouts=None):
        """zero_grad, forward, loss, and the backward down to the encoder output (weight gradients of the decoder
        flushed).  Leaves (encoder output, its gradient) in ``self._cut`` for :meth:`_encoder_backward`."""
        zero_tails()
        self.optimizer.zero_grad()
        rng.advance()
        loss, t_rows, enc, enc_leaf = self.model.forward_packed(inputs, input_lengths, targets, target_lengths,
                                                                cut_encoder=True, ce_truth=ground_truth, ignore_index=0,
                                                                layouts=layouts, ce_spec=self.ce_spec,
                                                                ce_denom=self._ce_denom)
        self.nll = self.model._st_ce_nll
        with deferred_wgrads(True):
            self._backward(loss)
        self._cut = (enc, enc_leaf.grad)
        return loss.detach()

    def _encoder_backward(self, fire_layers: bool = False):
        """fire_layers (the collectives are being captured with the step): every time the backward has left an encoder layer,
        the weight gradients deferred so far are flushed and the buckets that lie wholly in the finished layers start their
        all-reduce - the exchange of the upper encoder layers runs under the backward of the lower ones instead of behind the
        whole backward (the deferred weight gradients otherwise become final in ONE launch at its end)."""
        enc, d_enc = self._cut
        self._cut = None
        chains = self._encoder_chains() if fire_layers else None
        if chains is not None:
            chains.layer_hook = self._encoder_layer_done
        try:
            with deferred_wgrads(True):
                enc.backward(d_enc)
        finally:
            if chains is not None:
                chains.layer_hook = None

    def _encoder_chains(self):
        enc = getattr(self.model, "encoder", None)
        if enc is None or not hasattr(enc, "row_chains") or self._encoder_layer_offsets() is None:
            return None
        return enc.row_chains(arena_of(self.model))

    def _encoder_layer_offsets(self):
        """First element of every encoder layer in the flat gradient buffer - None unless the layers lie in stack order with
        everything that is not the encoder behind them (the layout ParamArena builds from module order)."""
        hit = getattr(self, "_enc_layer_lo", False)
        if hit is not False:
            return hit
        arena = arena_of(self.model)
        los = [min(arena.offset[id(p)] for p in layer.parameters()) for layer in self.model.encoder.layer_stack]
        his = [max(arena.offset[id(p)] + arena.size[id(p)] for p in layer.parameters()) for layer in self.model.encoder.layer_stack]
        cut = self._decoder_grad_start()
        ok = all(his[i] <= los[i + 1] for i in range(len(los) - 1)) and cut < arena.total and his[-1] <= cut
        self._enc_layer_lo = los if ok else None
        return self._enc_layer_lo

    def _encoder_layer_done(self, first_finished: int) -> None:
        los = self._encoder_layer_offsets()
        if los is None or first_finished >= len(los):
            return
        lo = los[first_finished]
        red = self.reducer
        if any(blo >= lo and not red._fired[i] for i, (blo, _) in enumerate(red.buckets)):
            from .functional import flush_deferred_wgrads
            flush_deferred_wgrads()          # everything registered so far: the finished layers' weight (+ bias) gradients
            red.fire_from(lo)

    def _decoder_grad_start(self) -> int:
        """First element of the flat gradient buffer that the encoder's backward no longer touches."""
        arena = arena_of(self.model)
        enc = {id(p) for p in self.model.encoder.parameters()}
        cut = max(arena.offset[i] + arena.size[i] for i in enc)
        others = [arena.offset[id(p)] for p in arena.params if id(p) not in enc]
        return cut if not others or min(others) >= cut else arena.total      # interleaved layout: nothing fires early

    def _fold_scale(self) -> bool:
        """The rank average's 1 / world is folded into the norm + clip + Adam kernels (no pass of its own over the flat buffer)."""
        return getattr(self.optimizer, "arena", None) is not None

    def _clip_and_update(self, grad_scale: float = 1.0):
        if getattr(self.optimizer, "arena", None) is not None:
            # global norm (one launch over the flat buffer: st_grad_norm, which also advances the step count), then clip +
            # Adam as one pass (st_adam_clip); grad_scale: the reducer left the rank sum (GradReducer.synchronize(divide=False))
            return self.optimizer.step_captured(grad_norm=True, max_norm=self.max_grad_norm, grad_scale=grad_scale)
        if grad_scale != 1.0:
            arena_of(self.model).grad.mul_(grad_scale)
        grad_norm = clip_grad_norm_flat(arena_of(self.model), self.max_grad_norm)
        self.optimizer.step_captured()
        return grad_norm

    def _eager(self, batch, layouts=None):
        if self.accumulate is not None:
            self._last_cap = None
            return self._micro_batch(*batch, layouts=layouts), None
        loss = self._forward_backward(*batch, layouts=layouts)
        scale = self.reducer.synchronize(divide=not self._fold_scale()) if self.reducer is not None else 1.0
        self.optimizer.update_learning_rate(self.global_step)
        return loss, self._clip_and_update(scale)

    def __call__(self, inputs, input_lengths, targets, target_lengths, ground_truth):
        """inputs [B, T, F] / targets, ground_truth [B, L] on the GPU; lengths on host or GPU."""
        self._options()
        raw = (inputs, input_lengths, targets, target_lengths, ground_truth)
        batch = trim_batch(*raw)
        B, l_max = batch[4].shape
        if self.accumulate is not None:
            self._stage_window(B, l_max, inputs.device)
            return self._accumulate_call(batch, raw)
        self.global_step += 1                    # (accumulating: counted per update, in _close_window)
        self._denom.stage(getattr(self.ce_spec, "norm", None), B, l_max, inputs.device)      # (label smoothing, norm "rows": B * l_max)
        return self._dispatch(batch, raw)

    def _dispatch(self, batch, raw):
        """Eager step, bucket step, or the captured step of this batch signature (that of the untrimmed tensors ``raw``)."""
        if self.bucket is not None:
            st, batch, packed = stage_bucket("TrainStep", self.model, self._buckets, self.bucket, self.bucket_rows, *batch)
            if not self.use_graph:
                return self._eager(batch, st.layouts)
            return bucket_step(st, packed, self.graph_warmup, lambda: self._eager(batch, st.layouts),
                               lambda: self._capture(batch, st.layouts), self._replay, serve_tails=self._single_graph())
        if not self.use_graph:
            return self._eager(batch)

        sig = batch_signature(*raw)
        cap = self._graphs.get(sig)
        if cap is None:
            n = self._seen.get(sig, 0) + 1
            self._seen[sig] = n
            while len(self._seen) > 64:
                self._seen.popitem(last=False)
            if n <= self.graph_warmup:                   # lazy init (arena, layouts, allocator) happens eagerly
                return self._eager(batch)
            cap = self._capture(batch)
            self._graphs[sig] = cap
            self._seen.pop(sig, None)
            while len(self._graphs) > self.max_graphs:
                self._graphs.popitem(last=False)         # least recently used: its graphs, pool and pinned layouts go
        self._graphs.move_to_end(sig)
        return self._replay(cap)

    def _replay(self, cap):
        if cap.options != self._options():
            raise RuntimeError("TrainStep: the optimizer's options changed after this step was captured (the graph holds the "
                               "old launches): enable the guard / the average before the first capture, or build a new TrainStep")
        if self.accumulate is not None:                   # the micro-batch capture; _close_window replays the update's
            self._g_fb, self._g_enc, self._g_opt, self._last_cap = cap.g_fb, None, cap.g_opt, cap
            self.nll = cap.nll
            cap.g_fb.replay()
            return cap.loss, None
        self._g_fb, self._g_enc, self._g_opt, self._dec_lo = cap.g_fb, cap.g_enc, cap.g_opt, cap.dec_lo     # (introspection / tests)
        self.nll = cap.nll                                # a static output of the graph, like the loss
        self.optimizer.update_learning_rate(self.global_step)
        cap.g_fb.replay()
        if cap.g_enc is not None:
            self.reducer.fire_from(cap.dec_lo)           # decoder-side buckets: exchanged while the encoder's backward runs
            cap.g_enc.replay()
            self.reducer.synchronize(divide=not self._fold_scale())      # (the captured update applies 1 / world: _capture)
        elif self.reducer is not None and cap.g_opt is not None:
            self.reducer.reduce_all(divide=not self._fold_scale())
        # (cap.g_opt None with a reducer: the collectives were captured inside g_fb - nothing happens on the host)
        if cap.g_opt is not None:
            cap.g_opt.replay()
        return cap.loss, cap.gnorm

    def _capture(self, batch, layouts=None):
        with no_gc_inside_capture():
            return self._capture_graphs(batch, layouts)

    def _capture_graphs(self, batch, layouts=None):
        dev = batch[0].device
        if self._seed is None or self._seed.device != dev:       # (the backward seed: resident, like the shared scratch)
            self._seed = torch.ones((), dtype=torch.float32, device=dev)
        prepare_capture(dev, self.optimizer)
        if self.reducer is not None and self.reducer.active:
            drain_collective_watchdog()
        cap = _Captured()
        cap.options = self._options()
        # the captured kernels read the ragged layouts (offsets, lengths, positions, attention work lists, scatter
        # index) by ADDRESS: pin the layout objects of this batch for as long as its graphs live (the layout cache may
        # be flushed by other shapes meanwhile)
        if layouts is not None:
            cap.keep = layouts
        elif hasattr(self.model, "prepare_layouts"):
            cap.keep = self.model.prepare_layouts(batch[1], batch[3], batch[2].shape[1], batch[0].device)
        # ... and the batch tensors themselves: the signature matches on their addresses, so the memory must not be
        # recycled for something else while a capture that reads it is alive
        cap.keep = (cap.keep, batch[0], batch[2], batch[4])
        pool = torch.cuda.graph_pool_handle()           # one pool per signature: replays of different signatures interleave freely
        cap.g_fb, cap.g_opt = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        split = self.reducer is not None and self.reducer.active and hasattr(self.model, "forward_packed") \
            and hasattr(self.model, "encoder")
        if self.reducer is not None:
            self.reducer.detach()                       # bucket all-reduces are issued explicitly between the graphs
        mode = capture_kwargs()
        if self.accumulate is not None:
            # two captures from one pool: the micro-batch (no zero_grad, no update), and the update (norm, clip + Adam, close);
            # with data parallelism the collectives run eagerly between them (_close_window)
            with torch.cuda.graph(cap.g_fb, pool=pool, **mode):
                cap.loss = self._micro_batch(*batch, layouts=layouts)
                cap.nll = self.nll
            with torch.cuda.graph(cap.g_opt, pool=pool, **mode):
                cap.gnorm = self._window_update()
            return cap
        if split and self.dp_in_graph:
            # ONE graph: forward + loss + decoder backward | decoder-side buckets start on RCCL's stream (a forked branch
            # of the graph) | encoder backward runs beside them | remaining buckets | join | clip + Adam
            failure = None
            try:
                g_all = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_all, pool=pool, **mode):
                    cap.loss = self._forward_decoder_backward(*batch, layouts=layouts)
                    cap.nll = self.nll
                    self.reducer.fire_from(self._decoder_grad_start())
                    self._encoder_backward(fire_layers=True)
                    cap.gnorm = self._clip_and_update(self.reducer.synchronize(divide=not self._fold_scale()))
            except Exception as e:  # noqa: BLE001 - a process group / RCCL build that cannot be captured: eager collectives
                failure = e
            # every rank must take the same mode (a rank replaying captured collectives beside one that issues them from the
            # host would deadlock): the ranks agree before anything else is exchanged - capture only records, so this is
            # the next collective on every rank either way
            if self.reducer.world > 1:
                ok = torch.tensor([0.0 if failure is not None else 1.0], device=batch[0].device)
                torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN, group=self.reducer.group)
                if float(ok) == 0.0 and failure is None:
                    failure = RuntimeError("another rank could not capture its collectives")
            if failure is None:
                cap.g_fb, cap.g_enc, cap.g_opt = g_all, None, None
                self.dp_mode = "in-graph"
                return cap
            import warnings
            warnings.warn("TrainStep: capturing the gradient all-reduces failed (%s: %s); using eager collectives "
                          "between three graphs" % (type(failure).__name__, failure))
            # the failed capture may have stopped anywhere: collectives noted as fired, tail buffers handed out, the
            # encoder cut stored, weight gradients still deferred - the recapture starts from a clean slate
            from .functional import TailBuffers, _Deferred
            self.reducer._work, self.reducer._fired = [], [False] * len(self.reducer.buckets)
            self._cut = None
            _Deferred.pending.clear()
            _Deferred.active = False
            nv._fold_pending.clear()
            nv.fold_deferred = False
            if TailBuffers.active is not None:
                TailBuffers.active.i = 0
            del g_all
            torch.cuda.synchronize()
            drain_collective_watchdog()      # (the agreement all-reduce above: see the wait before the capture)
            pool = torch.cuda.graph_pool_handle()
            cap.g_fb, cap.g_opt = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        if split:
            self.dp_mode = "split"
            cap.g_enc, cap.dec_lo = torch.cuda.CUDAGraph(), self._decoder_grad_start()
            with torch.cuda.graph(cap.g_fb, pool=pool, **mode):
                cap.loss = self._forward_decoder_backward(*batch, layouts=layouts)
                cap.nll = self.nll
            with torch.cuda.graph(cap.g_enc, pool=pool, **mode):
                self._encoder_backward()
        elif self.reducer is not None and self.reducer.active:
            with torch.cuda.graph(cap.g_fb, pool=pool, **mode):
                cap.loss = self._forward_backward(*batch, captured=True, layouts=layouts)
                cap.nll = self.nll
        else:                                           # nothing happens between backward and the update: ONE graph
            cap.g_opt = None
            with torch.cuda.graph(cap.g_fb, pool=pool, **mode):
                cap.loss = self._forward_backward(*batch, captured=True, layouts=layouts)
                cap.nll = self.nll
                cap.gnorm = self._clip_and_update()
            return cap
        # (the collectives run eagerly between the graphs and leave the rank SUM: the captured update carries the 1 / world)
        left = 1.0 / self.reducer.world if (self.reducer is not None and self.reducer.active and self.reducer.world > 1
                                            and self._fold_scale()) else 1.0
        with torch.cuda.graph(cap.g_opt, pool=pool, **mode):
            cap.gnorm = self._clip_and_update(left)
        # capture only records; the step that triggered it is executed by the replay that follows
        return cap


def drain_collective_watchdog(limit_s: float = 5.0) -> str:
    """Before a capture that contains collectives: wait until ProcessGroupNCCL's watchdog thread has RETIRED every eager collective.

    The eager steps' all-reduces are finished on the GPU after torch.cuda.synchronize(), but the watchdog retires them on its own
    clock - and its hipEventQuery of an eager collective's end event fails with "operation not permitted on an event last recorded
    in a capturing stream" once RCCL's stream has joined a capture, which terminates the process from the watchdog thread (round
    5: tools/dev/dp_capture_stress.py - 6 of 16 processes of 12 captures each died).  Round 5 waited a fixed 300 ms; that is not a
    synchronisation.  Now: the process group's flight recorder says for every collective whether the watchdog thread
    has RETIRED it (the ``retired`` flag of ``_dump_nccl_trace`` entries is set by that thread, when it drops the work from its
    list - unlike ``onlyActive`` and the ``state`` strings, which the dump call fills in itself by querying the events) - poll until
    every recorded collective is retired.  The recorder must be on: whoever creates the process group sets the environment variable
    ``TORCH_NCCL_TRACE_BUFFER_SIZE`` (the ring's size in collectives; 512 everywhere here) before ``init_process_group`` -
    ``dp.init_from_env`` does, and so do bench.py ``--force-dp`` and the tests that make a one-rank group themselves; where it is
    off or absent the fixed wait remains as the fallback (``ST_DP_DRAIN_MS``, default 300).  -> which of the two happened ("recorder" / "sleep")."""
    torch.cuda.synchronize()
    fallback_s = float(os.environ.get("ST_DP_DRAIN_MS", "300")) / 1e3
    dump = getattr(torch._C._distributed_c10d, "_dump_nccl_trace", None) if torch.distributed.is_available() else None
    if dump is not None and os.environ.get("ST_DP_DRAIN", "recorder") == "recorder":
        import pickle
        try:
            t0 = time.time()
            while time.time() - t0 < limit_s:
                entries = pickle.loads(dump(includeCollectives=True, includeStackTraces=False, onlyActive=False)).get("entries")
                if not entries or "retired" not in entries[0]:
                    break                      # the recorder is off (or speaks another format): the fixed wait below
                if all(e["retired"] for e in entries):
                    return "recorder"
                time.sleep(0.005)
        except Exception:      # (an unexpected dump format: fall through to the fixed wait)
            pass
    time.sleep(fallback_s)
    return "sleep"


class _Captured:
    """One batch signature's captured step: its graph(s), static result tensors and pinned ragged layouts."""
    __slots__ = ("g_fb", "g_enc", "g_opt", "loss", "gnorm", "dec_lo", "keep", "nll", "options")

    def __init__(self):
        self.g_fb = self.g_enc = self.g_opt = self.loss = self.gnorm = self.keep = self.nll = self.options = None
        self.dec_lo = 0


class JointTrainStep:
    """One optimisation step of the joint CTC + attention objective (BASELINE config 4; the reference's
    train_attn_and_ctc.py is an empty file - the step is train.py:25-46 with transformer/Loss.py:CTCAttentionLoss as the
    criterion):  loss = w * CTC(encoder output) + (1 - w) * CE(decoder logits).

    ``ctc="torch"`` (the default; environment ST_CTC_LOSS): everything except ``ctc_loss`` itself runs as HIP kernels and, in
    graph mode, inside three captured graphs that share a memory pool:
      graph A1  zero_grad, encoder forward, the CTC head's projection over the ragged encoder rows and st_ctc_gather (the
                <= L + 1 log-probabilities per frame ctc_loss reads - the [T, B, V] log-softmax tensor of the module-level
                path is never built);
      eager     ``torch.nn.functional.ctc_loss`` on that small tensor + its gradient, ON A SIDE STREAM (torch's CTC kernels
                build their length tables from pageable host memory, which a stream capture refuses).  Its three kernels walk
                the 1,000 frames sequentially on 32 workgroups - 3.1 ms at config 2 with the chip idle beside them - so
                meanwhile the main stream replays
      graph A2  decoder forward, vocabulary projection + cross-entropy (one node), and the backward of that branch down to the
                encoder output (the decoder never sees the CTC branch);
      graph B   (after the side stream's event) backward from BOTH roots into the encoder - the encoder output with the
                decoder's gradient, the log-probabilities with w * ctc_loss's gradient (st_ctc_dlogits -> the head's backward
                GEMMs) -, the deferred weight gradients, clip + Adam over the model's arena, the head's own Adam.

    ``ctc="hip"``: the CTC loss is csrc/st_ctc_loss.hip - lengths and labels on the device, two launches (the alpha / beta
    recursions, one wave per utterance and direction; the gradient), which write ``plan.g_lp`` / ``plan.roww`` themselves.
    Nothing of the step touches host memory any more, so graph mode captures ONE graph on one stream - part A1, the two CTC
    launches, part A2, part B - with no side stream and no events; eager mode runs the same sequence.

    The attention branch honours ``head.att_criterion`` (functional.ce_spec): the default ``nn.CrossEntropyLoss(ignore_index=0)``
    runs the plain st_ce_* launches; ``nn.CrossEntropyLoss(ignore_index=0, label_smoothing=e)`` and
    ``transformer.Loss.LabelSmoothingLoss(e, V, ignore_index=0)`` run the smoothed pair inside the same node and the same
    graph.  A head whose criterion the HIP path cannot honour (class weights, another reduction or ignore_index, any other
    module) now RAISES ValueError at construction - until this criterion support existed the step silently trained every head
    with the plain cross-entropy.  ``self.nll``: the plain token-mean NLL of the last step's attention branch (a device scalar).

    The optimizer's options (``ScheduledOptim.enable_nonfinite_guard`` / ``enable_averaging``) are read from the optimizer, as
    in TrainStep, with the JOINT norm as the verdict.  The CTC head lives outside the arena under ``head_optimizer``: with the
    guard on it must be torch's fused capturable Adam (ValueError otherwise) and gets ``found_inf = optimizer.found_inf`` -
    it then skips its update and rolls its step count back on that device scalar; with averaging on the head's average is
    kept here with ``lerp_`` by the device weight ``optimizer.averaging_weight()`` and registered with the optimizer, so
    ``optimizer.averaged()`` swaps the head's tensors with the arena.

    One batch signature at a time (a new signature re-captures)."""

    def __init__(self, model: nn.Module, optimizer, head, max_grad_norm: float, head_optimizer=None, use_graph: bool = True,
                 graph_warmup: int = 2, ctc: Optional[str] = None):
        self.model, self.optimizer, self.head, self.head_optimizer = model, optimizer, head, head_optimizer
        self.ctc = os.environ.get("ST_CTC_LOSS", "torch") if ctc is None else ctc
        if self.ctc not in ("torch", "hip"):
            raise ValueError("JointTrainStep: ctc must be 'torch' or 'hip', got %r" % (self.ctc,))
        self.max_grad_norm, self.use_graph, self.graph_warmup = max_grad_norm, use_graph, graph_warmup
        self.global_step = 0
        self._sig, self._seen, self._cap, self._plan = None, 0, None, None
        self._seed = None
        self._side = None
        self.ce_spec = ce_spec(getattr(head, "att_criterion", None), model.tgt_word_proj.weight.shape[0])
        self._denom = LossDenom()             # B * l_max (norm "rows") or 1 ("sum") on the device; read back as self._ce_denom
        self.nll = None
        self._options_token, self._head_avg = None, None
        self._bind_options()

    def _bind_options(self):
        """Carry the optimizer's options over to the head's optimizer (see the class docstring)."""
        self._options_token = optimizer_options(self.optimizer, "JointTrainStep")
        self._head_avg = None
        opt, hopt = self.optimizer, self.head_optimizer
        if hopt is None or self._options_token is None:
            return
        if getattr(opt, "found_inf", None) is not None:
            if not all(g.get("fused") and g.get("capturable") for g in hopt.param_groups):
                raise ValueError("JointTrainStep: with the non-finite guard on, head_optimizer must be torch's fused capturable "
                                 "Adam (fused=True, capturable=True): only that one skips its update on a device found_inf")
            hopt.found_inf = opt.found_inf
        if getattr(opt, "_avg_opts", None) is not None:
            params = [q for g in hopt.param_groups for q in g["params"]]
            self._head_avg = (params, opt.register_averaged(params))
            self._options_token = optimizer_options(self.optimizer, "JointTrainStep")

    def _check_options(self):
        if optimizer_options(self.optimizer, "JointTrainStep") != self._options_token:
            if self._cap is not None:
                raise RuntimeError("JointTrainStep: the optimizer's options changed after this step was captured (the graph "
                                   "holds the old launches): enable them before the first capture, or build a new step")
            self._bind_options()

    @property
    def _ce_denom(self):
        return self._denom.tensor

    def _average_head(self):
        if self._head_avg is not None:
            w = self.optimizer.averaging_weight()          # device scalar, 0 on a skipped step
            with torch.no_grad():
                for q, a in zip(*self._head_avg):
                    a.lerp_(q.detach(), w)

    # ---- the parts ------------------------------------------------------------------------------------------------------
    def _part_a1(self, batch, plan, layouts):
        inputs, in_len, targets, tgt_len, gt = batch
        in_rows, t_rows = layouts
        # the plan's label-derived tensors are a derived copy of the label buffer: re-made in place at the head of every step
        # (a loader may refill the buffer with new labels of the same lengths) - inside graph A1 when the step is captured, so
        # the dozen tiny launches cost no host time (eagerly they were 0.36 ms of launch gaps per step)
        plan.refresh_labels(gt)
        self.optimizer.zero_grad()
        self.head.zero_grad_buffers()
        rng.advance()
        arena = arena_of(self.model)
        with arena.scope():
            enc, _ = self.model.encoder.forward_rows(inputs, in_len, in_rows)
        lp = self.head.project_rows(enc, plan)
        return enc, lp

    def _part_a2(self, batch, enc, layouts):
        from . import functional as F_
        inputs, in_len, targets, tgt_len, gt = batch
        in_rows, t_rows = layouts
        arena = arena_of(self.model)
        enc_in = enc.detach().requires_grad_(True)
        arena._depth += 1                     # the bf16 shadow of this step's weights exists (graph A1 refreshed it)
        try:
            dec, _ = self.model.decoder.forward_rows(targets, tgt_len, enc_in, in_rows, t_rows)
            att = F_.VocabCeFn.apply(dec, self.model.tgt_word_proj.weight, self.model, gt.contiguous().view(-1), 0,
                                     t_rows.scatter_index(gt.shape[1]), self.ce_spec, self._ce_denom)
        finally:
            arena._depth -= 1
        self.nll = self.model._st_ce_nll      # (captured: a static output of the graph, like att)
        if self._seed is None or self._seed.device != att.device:
            self._seed = torch.empty((), dtype=att.dtype, device=att.device)
        self._seed.fill_(1.0 - float(self.head.ctc_weight))
        with deferred_wgrads(True):
            torch.autograd.backward(att, self._seed)
        return att.detach(), enc_in

    def _ctc(self, lp, plan):
        w = float(self.head.ctc_weight)
        if self.ctc == "hip":           # the gradient kernel writes w * g and the per-utterance softmax weights itself
            return self.head.ctc_rows(lp, plan, impl="hip", fill_weight=w)[0]
        ctc, g = self.head.ctc_rows(lp, plan)
        plan.g_lp.copy_(g)
        plan.g_lp.mul_(w)
        torch.mul(plan.finite.to(plan.roww.dtype), w / plan.B, out=plan.roww)
        plan.roww.div_(plan.tl.to(plan.roww.dtype))
        return ctc

    def _part_b(self, enc, enc_in, lp, plan):
        with deferred_wgrads(True):
            torch.autograd.backward([enc, lp], [enc_in.grad, plan.g_lp])
        if getattr(self.optimizer, "arena", None) is None:
            if self.head_optimizer is not None:
                self.head_optimizer.step()
            return None
        if self.head_optimizer is None:
            return self.optimizer.step_captured(grad_norm=True, max_norm=self.max_grad_norm)
        # train.py:45 clips everything that is being optimised: the global norm runs over the model's flat gradient AND the
        # CTC head's (its buffers live outside the arena), and both are scaled by the same coefficient
        arena = arena_of(self.model)
        self.optimizer.norm_scratch(arena.grad.device)
        g_model = nv.grad_norm(arena.grad, self.optimizer._norm_scratch, torch.empty((), dtype=torch.float32, device=arena.grad.device))
        gw, gb = self.head._st_gw, self.head._st_gb
        gnorm = torch.sqrt(g_model * g_model + (gw * gw).sum() + (gb * gb).sum())
        coef = torch.clamp(self.max_grad_norm / (gnorm + 1e-6), max=1.0)
        gw.mul_(coef)
        gb.mul_(coef)
        self.optimizer.step_captured(grad_norm=gnorm, max_norm=self.max_grad_norm)       # (advances the step count itself)
        self.head_optimizer.step()
        self._average_head()
        return gnorm

    def _joint(self, att, ctc):
        w = float(self.head.ctc_weight)
        return w * ctc + (1.0 - w) * att

    def _side_ctc(self, lp, plan):
        """ctc_loss + its gradient on the side stream, behind everything the main stream has queued so far; -> (loss, event)"""
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream()
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            ctc = self._ctc(lp, plan)
            done = torch.cuda.Event()
            done.record(self._side)
        return ctc, done

    def __call__(self, inputs, input_lengths, targets, target_lengths, ground_truth):
        """-> (joint loss, attention CE, CTC loss, clip norm): device tensors."""
        self._check_options()
        self.global_step += 1
        batch = trim_batch(inputs, input_lengths, targets, target_lengths, ground_truth)
        self._denom.stage(getattr(self.ce_spec, "norm", None), batch[4].shape[0], batch[4].shape[1], inputs.device)
        sig = batch_signature(inputs, input_lengths, targets, target_lengths, ground_truth)
        if sig != self._sig:
            self._sig, self._seen, self._cap = sig, 0, None
            self._layouts = self.model.prepare_layouts(batch[1], batch[3], batch[4].shape[1], inputs.device)
            # the CTC labels are the ground truth of train.py:40 (label ids, PAD = blank = 0 past each length)
            self._plan = self.head.plan(batch[4], batch[3], batch[1], self._layouts[0])
            self._keep = batch
        plan, layouts = self._plan, self._layouts
        self.optimizer.update_learning_rate(self.global_step)
        if not self.use_graph or self._seen < self.graph_warmup:
            self._seen += 1
            return self._step(batch, plan, layouts)
        if self._cap is None:
            self._before_capture(inputs.device, plan)
            with no_gc_inside_capture():
                self._cap = self._capture(batch, plan, layouts)
        if self.ctc == "hip":
            graph, out = self._cap
            graph.replay()
            return out
        ga1, ga2, gb, att, lp, gnorm = self._cap
        ga1.replay()
        ctc, done = self._side_ctc(lp, plan)
        ga2.replay()
        torch.cuda.current_stream().wait_event(done)
        gb.replay()
        return self._joint(att, ctc), att, ctc, gnorm

    def _step(self, batch, plan, layouts):
        """The whole step as one sequence on the current stream - with ctc="torch", ctc_loss beside part A2 on the side stream:
        the eager step, and what the one graph of ctc="hip" records.  -> (joint loss, attention CE, CTC loss, clip norm)"""
        enc, lp = self._part_a1(batch, plan, layouts)
        ctc, done = (self._ctc(lp, plan), None) if self.ctc == "hip" else self._side_ctc(lp, plan)
        att, enc_in = self._part_a2(batch, enc, layouts)
        if done is not None:
            torch.cuda.current_stream().wait_event(done)
        gnorm = self._part_b(enc, enc_in, lp, plan)
        return self._joint(att, ctc), att, ctc, gnorm

    def _capture(self, batch, plan, layouts):
        """ctc="hip": the step as ONE graph.  ctc="torch": its three parts as three graphs from one pool - ctc_loss runs between
        them at every replay (``__call__``), so the capture itself leaves it out.  Capture only records."""
        if self.ctc == "hip":
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._step(batch, plan, layouts)
            return graph, out
        pool = torch.cuda.graph_pool_handle()
        ga1, ga2, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga1, pool=pool):
            enc, lp = self._part_a1(batch, plan, layouts)
        with torch.cuda.graph(ga2, pool=pool):
            att, enc_in = self._part_a2(batch, enc, layouts)
        with torch.cuda.graph(gb, pool=pool):
            gnorm = self._part_b(enc, enc_in, lp, plan)
        return ga1, ga2, gb, att, lp, gnorm

    def _before_capture(self, device, plan):
        """What must exist before the capture and is this driver's own - the seed, the head optimizer's state, the HIP CTC
        loss's workspace - then stepdriver.prepare_capture."""
        if self._seed is None or self._seed.device != device:
            self._seed = torch.empty((), dtype=torch.float32, device=device)
        if self.head_optimizer is not None:
            groups = self.head_optimizer.param_groups
            if not all(g.get("capturable", False) for g in groups):
                raise ValueError("JointTrainStep(use_graph=True): head_optimizer must be built with capturable=True "
                                 "(its step is captured in graph B)")
            if any(len(self.head_optimizer.state.get(q, {})) == 0 for g in groups for q in g["params"]):
                raise ValueError("JointTrainStep(use_graph=True): head_optimizer has no state yet - run at least one eager "
                                 "step first (graph_warmup >= 1): state created inside the capture would be reset by "
                                 "every replay")
        if self.ctc == "hip":
            plan.loss_workspace()                 # alpha / beta belong to the plan, not to the graph's pool
        prepare_capture(device, self.optimizer)

    @property
    def graphs(self):
        """The captured graphs of the current batch signature (three with ctc="torch", one with ctc="hip"; none before a capture)."""
        return [] if self._cap is None else [x for x in self._cap if isinstance(x, torch.cuda.CUDAGraph)]

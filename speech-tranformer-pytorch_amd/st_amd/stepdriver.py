"""What the step drivers share: trainer.TrainStep, trainer.JointTrainStep and evaluate.EvalStep.

Every driver trims the batch to its longest utterance, stages a loss denominator on the device, prepares the process for a
capture, and - in bucket mode - walks one bucket through warm-up, recording, capture and replay.  Those pieces live here,
once, with no driver's policy in them: what a driver launches eagerly, what it captures and how it replays are callables it
passes in; how many warm-up calls it wants, which captures may serve tail buffers and what happens on a device change are its
arguments and its own code.
"""
from __future__ import annotations

import contextlib
import gc

import torch
import torch.distributed

from . import native as nv
from .functional import TailBuffers


@contextlib.contextmanager
def no_gc_inside_capture():
    """Around the captures of a step: collect garbage BEFORE them and keep the collector off until they have ended.

    A generational pass that happens to fire inside ``with torch.cuda.graph(...)`` runs destructors in the middle of a stream
    capture - those of a dead TrainStep's graphs and private pool, say, left in a reference cycle by an earlier step object
    - and the process aborted there (main thread, inside the collector, inside the micro-batch capture).  torch.cuda.graph used
    to call gc.collect() on entry; it no longer does unless torch.compiler.config.force_cudagraph_gc is set, so when a pass
    fires is a matter of how many objects the process happens to have allocated."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


# ---- the batch ------------------------------------------------------------------------------------------------------------
def trim_batch(inputs, input_lengths, targets, target_lengths, ground_truth):
    """The batch cut to its longest utterance and its longest target (host ints when the lengths are CPU tensors)."""
    t_max, l_max = int(input_lengths.max()), int(target_lengths.max())
    return inputs[:, :t_max], input_lengths, targets[:, :l_max], target_lengths, ground_truth[:, :l_max]


def batch_signature(inputs, input_lengths, targets, target_lengths, ground_truth):
    """What a per-signature capture is keyed by: the addresses and shapes of the (untrimmed) tensors, the length vectors' bytes."""
    return (inputs.data_ptr(), targets.data_ptr(), ground_truth.data_ptr(), tuple(inputs.shape), tuple(targets.shape),
            input_lengths.cpu().numpy().tobytes(), target_lengths.cpu().numpy().tobytes())


def parse_buckets(who, bucket, bucket_rows):
    """-> (bucket as an int pair or None, bucket_rows as a list of int pairs or None); one pair may be given bare."""
    bucket = None if bucket is None else (int(bucket[0]), int(bucket[1]))
    if bucket_rows is not None and not isinstance(bucket_rows[0], (tuple, list)):
        bucket_rows = [bucket_rows]
    bucket_rows = None if bucket_rows is None else [(int(a), int(b)) for a, b in bucket_rows]
    if bucket_rows is not None and bucket is None:
        raise ValueError("%s: bucket_rows needs bucket=(T_cap, L_cap)" % who)
    return bucket, bucket_rows


class LossDenom:
    """The denominator of a criterion with norm "rows" (B * l_max of the trimmed batch) / "sum" (1): a persistent device
    scalar the loss kernels read at run time - staged per batch by an eager fill, never inside a capture, so one captured
    step serves batches whose l_max differ.  ``tensor`` stays None for "tokens" (the kernels count the tokens themselves)."""
    __slots__ = ("tensor", "host")

    def __init__(self):
        self.tensor, self.host = None, None

    def stage(self, norm, B: int, l_max: int, device) -> None:
        """Refresh the value for this batch: created on first use or on another device, filled only when the value changes."""
        if norm is None or norm == "tokens":
            return
        d = float(B * l_max) if norm == "rows" else 1.0
        if self.tensor is None or self.tensor.device != device:
            self.tensor = torch.full((1,), d, dtype=torch.float32, device=device)
        elif d != self.host:
            self.tensor.fill_(d)
        self.host = d


def optimizer_options(optimizer, who):
    """The optimizer's option token (None for an optimizer without options); raises inside ``optimizer.averaged()``."""
    if getattr(optimizer, "_in_averaged", False):
        raise RuntimeError("%s: called inside optimizer.averaged() - the model holds the averaged weights" % who)
    token = getattr(optimizer, "options_token", None)
    return None if token is None else token()


# ---- captures -------------------------------------------------------------------------------------------------------------
def zero_tails():
    """First launch of a captured packed-bucket step: the unassigned tail rows of every registered buffer (one launch)."""
    tb = TailBuffers.active
    if tb is not None and tb.mode == "serve" and tb.bufs:
        nv.zero_tails(tb.table, TailBuffers.N_MAX)


def prepare_capture(device, optimizer=None) -> None:
    """Everything lazily created must exist BEFORE a capture: Adam's flat state (a captured zero-fill would reset it on every
    replay) and the process-wide scratch the step's kernels share - split-K partials and tickets, the norm's block partials:
    created inside a capture they would live in that graph's private pool while later captures and eager calls keep using
    them.  Ends with a device synchronisation.  (A driver's gradient seed is its own: it makes it before calling this.)"""
    if optimizer is not None and hasattr(optimizer, "_flat_state") and getattr(optimizer, "arena", None) is not None:
        optimizer._flat_state()
    nv.splitk_scratch(device)
    if optimizer is not None and hasattr(optimizer, "norm_scratch"):
        optimizer.norm_scratch(device)
    torch.cuda.synchronize()


def capture_kwargs() -> dict:
    """Arguments of ``torch.cuda.graph``.  ProcessGroupNCCL's watchdog thread polls the events of outstanding collectives
    (hipEventQuery); under the default "global" capture mode that call from ANOTHER thread aborts the process ("operation
    not permitted when stream is capturing").  With a process group alive, only this thread's unsafe calls are policed."""
    return dict(capture_error_mode="thread_local") if torch.distributed.is_initialized() else {}


# ---- bucket mode ----------------------------------------------------------------------------------------------------------
class _Bucket:
    """Bucket mode: static staging buffers, device-length layouts and the captured step of one (B, feature) shape."""
    __slots__ = ("x", "tok", "gt", "gt_flat", "layouts", "cap", "seen", "tails")

    def __init__(self):
        self.x = self.tok = self.gt = self.gt_flat = self.layouts = self.cap = self.tails = None
        self.seen = 0


def stage_bucket(who, model, buckets, bucket, bucket_rows, inputs, input_lengths, targets, target_lengths, ground_truth):
    """The staging of one batch into a bucket, shared by the step drivers: the batch is copied
    into the bucket's static padded buffers, the lengths (packed capacities: the offsets too) are refreshed on the device, the
    encoder's work lists follow the batch.  ``buckets``: the driver's dict of _Bucket by (B, feature, dtype, device,
    capacity); a missing one is created here - buffers, Rows.bucket layouts, chain plans and work lists, all before any capture.
    -> (the _Bucket, the batch to run: static tensors + this batch's lengths, whether the layouts are packed)."""
    T_cap, L_cap = bucket
    B, T, Fd = inputs.shape
    L = targets.shape[1]
    if T > T_cap or L > L_cap or ground_truth.shape[1] > L_cap:
        raise ValueError("%s(bucket=%r): batch of %d frames / %d tokens does not fit" % (who, bucket, T, L))
    caps = None                   # the first packed capacity the batch fits (None: the padded bucket)
    if bucket_rows is not None:
        n_in, n_tgt = int(input_lengths.sum()), int(target_lengths.sum())
        caps = next((c for c in bucket_rows if n_in <= c[0] and n_tgt <= c[1]), None)
    packed = caps is not None
    key = (B, Fd, inputs.dtype, str(inputs.device), caps)
    st = buckets.get(key)
    if st is None:
        from .functional import Rows
        dev = inputs.device
        st = _Bucket()
        st.x = torch.zeros(B, T_cap, Fd, dtype=inputs.dtype, device=dev)
        st.tok = torch.zeros(B, L_cap, dtype=targets.dtype, device=dev)
        # (one spare element behind the padded ground truth: the target of the rows a packed bucket leaves unassigned;
        # it stays 0 = ignore_index)
        st.gt_flat = torch.zeros(B * L_cap + 1, dtype=ground_truth.dtype, device=dev)
        st.gt = st.gt_flat[:B * L_cap].view(B, L_cap)
        in_cap, tgt_cap = caps if packed else (None, None)
        st.layouts = (Rows.bucket(B, T_cap, dev, rows=in_cap), Rows.bucket(B, L_cap, dev, rows=tgt_cap))
        if hasattr(model, "prepare_layouts"):          # chain plans, work lists: before any capture
            from .functional import attn_work
            model.prepare_layouts(torch.full((B,), T_cap), torch.full((B,), L_cap), L_cap, dev)
            ir, tr = st.layouts
            dk, nh = getattr(model, "_d_k", 64), getattr(model, "_n_head", 0)
            attn_work(ir, ir, False, dk, nh), attn_work(tr, tr, True, dk, nh), attn_work(tr, ir, False, dk, nh)
            tr.scatter_index(L_cap)
        buckets[key] = st
    st.x[:, :T].copy_(inputs, non_blocking=True)
    if T < T_cap:
        st.x[:, T:].zero_()                                  # no frame of an earlier batch survives behind a length
    st.tok.zero_()
    st.tok[:, :L].copy_(targets, non_blocking=True)
    st.gt.zero_()                                            # padding positions: ground truth 0 = ignore_index
    st.gt[:, :ground_truth.shape[1]].copy_(ground_truth, non_blocking=True)
    st.layouts[0].set_lengths(input_lengths)
    st.layouts[1].set_lengths(target_lengths)
    if hasattr(model, "prepare_layouts"):
        # the encoder self-attention's work lists follow the batch (longest utterance first); the decoder's attentions
        # are a handful of short workgroups either way
        from .functional import refresh_attn_work
        ir = st.layouts[0]
        refresh_attn_work(ir, ir, False, getattr(model, "_d_k", 64), getattr(model, "_n_head", 0),
                          input_lengths.tolist(), input_lengths.tolist())
    batch = (st.x, input_lengths, st.tok, target_lengths, st.gt_flat if packed else st.gt)
    return st, batch, packed


def bucket_step(st, packed, warmup, eager, capture, replay, serve_tails):
    """One call of a graph-mode driver on the staged bucket ``st``: ``eager()`` for the first ``warmup`` calls, then
    ``st.cap = capture()`` once - which only records - and ``replay(st.cap)`` from that call on.

    The last eager call of a PACKED bucket notes the buffers whose unassigned tail rows must read as zeros; the capture
    serves them from persistent memory and zeroes all tails with one launch (functional.TailBuffers, :func:`zero_tails`) -
    where ``serve_tails`` holds: a step cut into several captures that share a memory pool takes its buffers the plain way.
    ``TailBuffers.active`` is set here and nowhere else, and is None again when this returns or raises."""
    if st.cap is None:
        st.seen += 1
        try:
            if st.seen <= warmup:
                if packed and st.seen == warmup:
                    st.tails = TailBuffers.active = TailBuffers()
                return eager()
            if packed and st.tails is not None and serve_tails:
                TailBuffers.active = st.tails.materialize(st.x.device)
            st.cap = capture()
        finally:
            TailBuffers.active = None
    return replay(st.cap)

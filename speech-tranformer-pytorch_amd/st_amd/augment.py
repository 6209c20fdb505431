"""SpecAugment (Park et al. 2019: time warp, time and frequency masks) inside the training step.

A policy object holds the mask counts and widths; the masks themselves are drawn ON THE DEVICE, per utterance, from the
same seed in device memory that gives dropout fresh masks on every replay of a captured step (st_amd/rng.py), by one small
plan launch (st_specaug_plan), and applied by the kernel that turns the features into bf16 rows anyway (st_pack_rows_aug
for the padded inputs of a step, st_feat_stack_aug for raw features) - no extra pass over the features and nothing on the
host.  include/st_hip.h (st_specaug_plan) spells the draw out; tests/_specaug_ref.py restates it in Python integers.

``time_warp = W > 0`` adds the paper's first step: per utterance one source frame c moves to c' (|c' - c| <= W), the time
axis is resampled piecewise linearly with both ends fixed, and the masks are applied to the warped utterance.  The pair is
drawn by the same plan launch (st_specaug_plan_warp writes both tables) and the resampling happens in the same kernel
that applies the masks (st_pack_rows_warp / st_feat_stack_warp, csrc/st_augment.hip): still two launches per step.
include/st_hip.h (st_specaug_plan_warp) holds the definition, tests/_timewarp_ref.py its restatement.  With
``time_warp = 0`` (the default) nothing of this is launched.

    enc = model.encoder
    enc.spec_augment = SpecAugment(mel_bins=80, left=3, right=0, frame_rate=30)   # how the step's inputs were stacked
    model.train()          # eval() - or spec_augment = None - takes the unmasked path
"""
from __future__ import annotations

from typing import Optional

import torch

from . import native as nv
from . import rng
from .functional import Rows, rows_buffer

_salt = 0x80000000       # next default salt: counts up from 2^31, dropout's salts (rng.site) count up from 1 - disjoint
_TABLES = {}             # (salt, device, B) -> mask table; never freed: a captured graph has its address baked into two nodes
_WARPS = {}              # (salt, device, B) -> warp table, likewise


class SpecAugment:
    """``mel_bins``: bins of one RAW frame.  ``n_time_masks`` masks of up to ``time_width`` raw frames each - and no wider
    than ``time_ratio_permille`` / 1000 of the utterance -, ``n_freq_masks`` masks of up to ``freq_width`` bins.
    ``left`` / ``right`` / ``frame_rate``: how the inputs of the training step were stacked and subsampled (reference
    Dataset.py:121-153; st_amd.features.stack_frames) - masks are drawn in raw frames and raw bins and mapped onto the
    stacked rows, so one raw frame is masked in every row that shows it.  ``salt``: fixed per instance (default: a counter
    of its own, apart from dropout's - attaching a policy changes no dropout mask).  ``time_warp``: W of the paper, in raw
    frames - 0 (the default): no warp; utterances shorter than 2 W + 3 raw frames are never warped.  ``pack`` fetches the
    warp's source frames from the stacked rows themselves, which show every raw frame only with ``right == 0`` and
    ``left >= interval - 1`` (the reference's left 3 / right 0 / frame_rate 30 does); other geometries are warped from the
    raw features: ``features.stack_frames(..., augment=aug)``.

    ``last_masks``: int32 [B, n_time_masks + n_freq_masks, 2] on the device, the (start, width) pairs of the most recent
    plan launch (time masks first); in a captured step a static tensor that every replay rewrites.  ``last_warp``: int32
    [B, 2] on the device, (c, c') of the most recent WARPING plan launch - (0, 0): not warped -, static in the same way; None
    until one ran."""

    def __init__(self, mel_bins: int, n_time_masks: int = 2, time_width: int = 40, time_ratio_permille: int = 200,
                 n_freq_masks: int = 2, freq_width: int = 27, left: int = 0, right: int = 0, frame_rate: int = 10,
                 salt: Optional[int] = None, time_warp: int = 0):
        global _salt
        values = dict(mel_bins=mel_bins, n_time_masks=n_time_masks, time_width=time_width, time_ratio_permille=time_ratio_permille,
                      n_freq_masks=n_freq_masks, freq_width=freq_width, left=left, right=right, frame_rate=frame_rate,
                      time_warp=time_warp)
        for name, v in values.items():
            try:
                ok = int(v) == v and v >= 0
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("SpecAugment: %s = %r must be a non-negative integer" % (name, v))
        if n_time_masks + n_freq_masks > 64:
            raise ValueError("SpecAugment: at most 64 masks in all (%d + %d)" % (n_time_masks, n_freq_masks))
        if right > left:
            raise ValueError("SpecAugment: right context > left context is a shape error in the reference (Dataset.py:139)")
        if mel_bins < 4 or mel_bins % 4:
            raise ValueError("SpecAugment: mel_bins = %d must be a positive multiple of 4" % mel_bins)
        if time_ratio_permille > 1000:
            raise ValueError("SpecAugment: time_ratio_permille = %d lies outside 0 .. 1000" % time_ratio_permille)
        if time_warp > nv.WARP_MAX_FRAMES:
            raise ValueError("SpecAugment: time_warp = %d exceeds the %d raw frames the warp kernels take" % (time_warp, nv.WARP_MAX_FRAMES))
        if salt is not None and salt < 0:
            raise ValueError("SpecAugment: salt = %r must be non-negative" % (salt,))
        for name, v in values.items():
            setattr(self, name, int(v))
        self.interval = 1 if self.frame_rate == 10 else int(self.frame_rate / 10)     # as features.stack_frames
        if self.interval < 1:
            raise ValueError("SpecAugment: frame_rate = %d gives no positive subsampling interval" % frame_rate)
        if salt is None:
            salt, _salt = _salt, _salt + 1
        self.salt = int(salt) & 0xFFFFFFFF
        self.last_masks = None
        self.last_warp = None

    @property
    def n_masks(self) -> int:
        return self.n_time_masks + self.n_freq_masks

    def plan(self, lengths: torch.Tensor, stacked: bool) -> torch.Tensor:
        """One plan launch -> ``last_masks`` (and, with a time warp, ``last_warp``).  lengths: int32 [B] ON THE DEVICE (read by
        the kernel: a bucket layout's current lengths, a replay's current lengths) - rows stacked with this policy's geometry if
        ``stacked``, else raw frames."""
        B, dev = lengths.numel(), lengths.device
        key = (self.salt, str(dev), B, self.n_masks)
        table = _TABLES.get(key)
        if table is None:
            table = _TABLES[key] = torch.zeros(B, self.n_masks, 2, dtype=torch.int32, device=dev)
        geometry = dict(interval=self.interval if stacked else 1, right=self.right if stacked else 0)
        if self.time_warp > 0:
            warp = _WARPS.get(key[:3])
            if warp is None:
                warp = _WARPS[key[:3]] = torch.zeros(B, 2, dtype=torch.int32, device=dev)
            nv.specaug_plan_warp(rng.seed_tensor(dev), self.salt, lengths, table, warp, self.n_time_masks, self.time_width,
                                 self.time_ratio_permille, self.n_freq_masks, self.freq_width, self.mel_bins, self.time_warp,
                                 **geometry)
            self.last_warp = warp
        else:
            nv.specaug_plan(rng.seed_tensor(dev), self.salt, lengths, table, self.n_time_masks, self.time_width,
                            self.time_ratio_permille, self.n_freq_masks, self.freq_width, self.mel_bins, **geometry)
        self.last_masks = table
        return table

    def pack(self, inputs: torch.Tensor, rows: Rows) -> torch.Tensor:
        """What functional.PackFn does for the encoder - padded fp32 [B, T, F] -> bf16 row matrix - with this step's masks
        (and, first, its time warp) applied.  No gradient flows to ``inputs``."""
        if inputs.dim() != 3 or inputs.shape[2] != self.mel_bins * (1 + self.left + self.right):
            raise ValueError("SpecAugment: inputs %s do not have mel_bins * (1 + left + right) = %d * (1 + %d + %d) columns"
                             % (tuple(inputs.shape), self.mel_bins, self.left, self.right))
        if inputs.requires_grad:
            raise ValueError("SpecAugment: the augmenting pack has no backward - inputs must not require a gradient")
        if self.time_warp > 0 and (self.right != 0 or self.left < self.interval - 1):
            raise ValueError("SpecAugment: pack cannot warp rows stacked with (left %d, right %d, interval %d) - they show every "
                             "raw frame only with right == 0 and left >= interval - 1; warp the raw features instead: "
                             "features.stack_frames(..., augment=aug)" % (self.left, self.right, self.interval))
        out = rows_buffer(rows.total, inputs.shape[2], rows, inputs.device)
        table = self.plan(rows.len, stacked=True)
        if self.time_warp > 0:
            nv.pack_rows_warp(inputs.contiguous(), rows.off, rows.len, out, table, self.last_warp, self.n_time_masks,
                              self.n_freq_masks, self.mel_bins, self.left, self.right, self.interval)
        else:
            nv.pack_rows_aug(inputs.contiguous(), rows.off, rows.len, out, table, self.n_time_masks, self.n_freq_masks,
                             self.mel_bins, self.left, self.right, self.interval)
        return out

"""Beam-search decode on the HIP path: drop-in for the reference's transformer/Decode.py (BASELINE config 5).

Semantics follow Decode.py:48-179 - encode once, at most 100 steps, every unfinished utterance's beam is advanced
with the log-softmax of the last position, an utterance leaves the batch when the top of its beam is EOS, the
``n_best`` hypotheses come from the final score order - with two structural changes that do not alter results:

* **KV cache** instead of re-running the decoder over the whole prefix every step (Decode.py:96-98): each
  layer's self-attention keys / values of the tokens decoded so far are kept per hypothesis (re-gathered by the
  beam's back-pointers each step); the decoder is causal, so position t only ever needed the new token.
* the encoder output is **not repeated per beam** (Decode.py:57-66): the encoder-decoder keys / values are
  projected once per utterance and every hypothesis's attention points its (offset, length) at its utterance's rows.

* the **beam state lives on the device** (scores, back-pointers, tokens, finished flags as [.., B, beam] tensors; the
  arithmetic of transformer/Beam.py for all utterances in one top-k) and so do the step counter and the cache length,
  so ONE decoder step - ~60 launches - is captured into a HIP graph after the first step and replayed; the host reads
  the finished flags every 8 steps.  A finished utterance keeps its rows and is frozen (the reference drops it from
  the batch, Decode.py:112-165: identical results); hypotheses inherit their parent's K|V history through
  ``st_cache_reorder`` (the back-pointers of Beam.py:65 applied to the cache).

One decode step reuses the training kernels through the C-ABI (``st_gemm``, ``st_gemm_ln``, ``st_attn_fwd``: the
hypotheses of one utterance are one ``beam``-query problem of the key-split attention kernel).  The reference's constructor
cannot run (obsolete ``Transformer(...)`` signature, undefined ``prob_projection``): pass the model."""
import math

import torch

import transformer.Constants as Constants
from st_amd import biasing
from st_amd import ctc_decode
from st_amd import functional as F_
from st_amd import native as nv
from st_amd import ngram
from st_amd.arena import arena_of
from transformer.Beam import Beam  # noqa: F401  (re-exported: the reference's Decode module exposes it)

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
LN_EPS = 1e-6


class Decode(object):
    ''' Beam search over a trained Transformer. '''

    def __init__(self, opt, device, model=None, ctc_head=None, lm=None, bias=None):
        """opt: attribute-style (beam_size, n_best, [max_steps=100], [use_graph], [ctc_weight=0.0], [ctc_pre_beam], [lm_weight=0.0],
        [lm_length_bonus=0.0], [ctc_lm_weight=0.0], [ctc_lm_length_bonus=0.0], [bias_weight=1.0]); model: a
        transformer.Models.Transformer on ``device`` (the reference loads a checkpoint here with an API that no longer exists).
        ``ctc_head``: the ``transformer.Loss.CTCAttentionLoss`` a joint model was trained with (its ``ctc_proj`` over the encoder
        output).  With a head and ``opt.ctc_weight`` = w > 0 the search is the joint CTC / attention beam search (see
        st_amd.ctc_decode): a token c of the ``ctc_pre_beam`` (default ceil(1.5 beam)) best attention tokens of hypothesis g
        scores (1 - w) log p_att(c | g) + w (psi(g.c) - psi(g)), psi = the CTC prefix log-probability; every other token -inf.
        ``lm``: a ``st_amd.ngram.NGramLM`` on ``device`` (``NGramLM....to(device)``) - shallow fusion: with ``opt.lm_weight`` =
        lambda > 0 (or ``opt.lm_length_bonus`` = beta != 0) every candidate that extends a hypothesis which has not emitted EOS
        also scores lambda log p_lm(c | g) + beta (st_ngram_score between the pre-beam and the advance).  Without a CTC head (or
        w = 0) the LM route keeps the pre-beam: it considers the ``ctc_pre_beam`` (default ceil(1.5 beam)) best ATTENTION tokens of
        every hypothesis, not the whole vocabulary - a token the attention decoder ranks below them is never proposed, whatever
        the LM thinks of it.  With ``lm=None``, or lambda = 0 and beta = 0, every method launches exactly what it does without.
        ``opt.ctc_lm_weight`` / ``opt.ctc_lm_length_bonus`` (default 0: off; they do NOT default to ``opt.lm_weight``): the model
        fused into the CTC prefix beam search itself - ``ctc_beam`` and the first pass of ``decode_two_pass``.
        ``bias``: a ``st_amd.biasing.ContextBias`` on ``device`` (``ContextBias.from_phrases(...).to(device)``) - contextual biasing:
        with ``opt.bias_weight`` = b > 0 (default 1; it multiplies every phrase weight) a hypothesis h also scores b x reward(h), the
        sum of w_p |p| over the occurrences of the phrases in it; while it grows it carries a provisional reward for the phrase in
        progress, taken back when the match falls through or EOS closes the list (st_bias_score / st_bias_advance around the
        advance, inside the captured step).  Without a CTC head (or w = 0) the search keeps the pre-beam as with a language model,
        and on EVERY route a token can only be boosted if the pre-beam proposes it: a phrase token the attention decoder ranks
        below its ``ctc_pre_beam`` best is never considered, whatever its weight.  ``ctc_beam`` and the first pass of
        ``decode_two_pass`` are not biased; its rescoring is.  With ``bias=None`` or b = 0 every method launches exactly what it
        does without.  Each ``decode_batch`` call captures its own step, so a call may follow one with another ``bias`` object."""
        if model is None:
            raise NotImplementedError("Decode(HIP): pass the Transformer instance (the reference's checkpoint loader "
                                      "calls an obsolete constructor and cannot run)")
        self.ctc_weight, self.ctc_pre_beam = ctc_decode.check_options(opt, int(opt.beam_size), ctc_head, model, device)
        self.ctc_head = ctc_head
        self.lm_weight, self.lm_length_bonus, self.lm_pre_beam = ngram.check_options(
            opt, lm, model, device, int(opt.beam_size), joint=self.ctc_pre_beam is not None)
        self.lm = lm
        self._lm_on = lm is not None and (self.lm_weight > 0.0 or self.lm_length_bonus != 0.0)
        from st_amd import ctc_beam
        self.ctc_lm_weight, self.ctc_lm_length_bonus, _ = ctc_beam.check_lm(
            lm, getattr(opt, "ctc_lm_weight", None), getattr(opt, "ctc_lm_length_bonus", None), who="Decode: ctc_lm_weight")
        self.bias_weight, self.bias_pre_beam = biasing.check_options(opt, bias, model, device, int(opt.beam_size),
                                                                     joint=self.ctc_pre_beam is not None)
        self.bias = bias
        self._bias_on = bias is not None and self.bias_weight > 0.0
        self.opt, self.device = opt, device
        self.model = model.to(device).eval()
        self.max_steps = int(getattr(opt, "max_steps", None) or 100)
        ug = getattr(opt, "use_graph", None)
        self.use_graph = torch.device(device).type == "cuda" if ug is None else bool(ug)
        self._side = None
        self.alignment = None     # align(): the device tensors of its last call
        self._warm = False       # a step has run eagerly on this object: later calls capture before their step 0

    def set_bias(self, bias):
        """Replace the context bias (None: none) for the calls that follow - the per-request phrase list.  Checked as in the
        constructor; ``decode_batch`` builds its state and captures its step per call, so nothing of the earlier one is reused."""
        self.bias_weight, self.bias_pre_beam = biasing.check_options(self.opt, bias, self.model, self.device, int(self.opt.beam_size),
                                                                     joint=self.ctc_pre_beam is not None)
        self.bias = bias
        self._bias_on = bias is not None and self.bias_weight > 0.0

    # ---- one decoder step for all n = B * beam hypotheses; everything that changes from step to step is DEVICE state ---
    @torch.no_grad()
    def _step(self, st):
        """-> vocabulary logits [n, v_pad] fp32 of the next token; writes the step's self-attention K|V into the caches.
        ``st`` (a _DecodeState) holds: tokens [n] int64, step [1] int64, c_len [n] int32 (= step + 1), caches
        [L, n, S, 2d], the per-utterance encoder keys / values ``cross[l]`` and the attention layouts."""
        dec = self.model.decoder
        n, d, S = st.n, dec.d_model, self.max_steps
        dst = dec._st
        if st.x_in is not None:    # (search: st_beam_advance left the decoder input of the tokens it chose; step 0: _init_state)
            x = st.x_in
        else:
            x = nv.embed_step(st.tokens, dst.emb, dst.pe, st.step, torch.empty(n, d, dtype=BF16, device=st.tokens.device))  # Models.py:84,87
        dc = st.chains
        layers = list(dec.layer_stack)

        def E(cols):
            return torch.empty(n, cols, dtype=BF16, device=x.device)

        qkv = None
        for l, layer in enumerate(layers):
            # -- masked self-attention over the cache (the causal mask is implicit: only the past is cached)
            s = layer.slf_attn._st
            c = layer.enc_attn._st
            f = layer.pos_ffn._st
            H = s.n_head
            scale = 1.0 / math.sqrt(d // H)
            if qkv is None:
                qkv = E(3 * d)
                nv.gemm(x, s.w_qkv, qkv, bias=s.b_qkv)
            ctx = E(d)
            if d // H == 64 and S <= 128:
                # decode-shaped kernel: one wave per (hypothesis, head); it also appends this step's K | V to the cache
                nv.decode_self_attn(qkv, st.caches[l], st.step, ctx, H, scale, anc=st.anc)
            else:
                st.caches[l].index_copy_(1, st.step, qkv[:, d:].unsqueeze(1))
                kv = st.caches[l].view(n * S, 2 * d)
                nv.attn_fwd(qkv[:, :d], kv[:, :d], kv[:, d:], ctx, st.lse, st.q_off, st.q_one, st.c_off, st.c_len, H, 1, False,
                            scale, max_k=S)
            # -- output_linear + LayerNorm, then the encoder-decoder attention's q projection: separate launches, or ONE
            #    row chain (csrc/st_rowchain.hip) when the layers fit it
            # -- encoder-decoder attention: keys / values projected once per utterance; the beam's hypotheses of one
            #    utterance are consecutive rows = ONE attention problem of `beam` queries (one pass over its keys).  With the
            #    row chains the chain stage and the attention are one launch (nv.attn_f1_fwd) where the shape allows
            y, q, ctx2 = E(d), E(d), E(d)
            if dc is not None:
                nv.attn_f1_fwd(ctx, dc.f1[l], (x, s.b_o, s.gamma, s.beta, y, None, None), (1, c.b_q, q), st.cross[l][:, :d],
                               st.cross[l][:, d:], ctx2, st.lse, st.u_off, st.u_len, st.k_off, st.k_len, H, st.beam, scale,
                               max_k=st.max_k)
            else:
                nv.gemm_ln(ctx, s.w_o, s.b_o, x, s.gamma, s.beta, y, None, None, eps=LN_EPS)
                nv.gemm(y, c.w_q, q, bias=c.b_q)
                nv.attn_fwd(q, st.cross[l][:, :d], st.cross[l][:, d:], ctx2, st.lse, st.u_off, st.u_len, st.k_off, st.k_len, H,
                            st.beam, False, scale, max_k=st.max_k)
            ctx = ctx2
            # -- its output_linear + LayerNorm, the position-wise feed-forward, the next layer's q|k|v projection
            x_next = E(d)
            z, h = (None, None) if dc is not None else (E(d), E(f.d_ff))      # (inside the chain neither leaves the chip)
            nxt = layers[l + 1].slf_attn._st if l + 1 < len(layers) else None
            qkv = E(3 * d) if nxt is not None else None
            if dc is not None:
                nv.row_chain(ctx, dc.f2[l], pre=(y, c.b_o, c.gamma, c.beta, z, None, None),
                             ffn=(f.d_ff, f.b1, f.b2, f.gamma, f.beta, h, x_next, None, None, None, None),
                             post=(3, nxt.b_qkv, qkv) if nxt is not None else None)
            else:
                nv.gemm_ln(ctx, c.w_o, c.b_o, y, c.gamma, c.beta, z, None, None, eps=LN_EPS)
                nv.gemm(z, f.w1, h, bias=f.b1, epi=nv.EPI_BF16_RELU)
                nv.gemm_ln(h, f.w2, f.b2, z, f.gamma, f.beta, x_next, None, None, eps=LN_EPS)
                if nxt is not None:
                    nv.gemm(x_next, nxt.w_qkv, qkv, bias=nxt.b_qkv)
            x = x_next
        ms = self.model._st
        logits = torch.empty(n, ms.v_pad, dtype=F32, device=x.device)
        nv.gemm(x, ms.w_vocab, logits, epi=nv.EPI_F32)
        return logits           # the log-softmax (the undefined `prob_projection`) is taken by st_beam_advance

    @torch.no_grad()
    def _advance(self, st, logits):
        """Beam.advance (Beam.py:43-74) for every utterance at once, on the device (``st_beam_advance``: the best of every
        hypothesis row, then one wave per utterance merges them):
        log-softmax of the logits, top-k over beam x vocab of score + log-probability, back-pointer = index // vocab,
        token = index % vocab; an utterance is finished once the top of its beam emits EOS - after which its state is
        frozen (the reference removes it from the batch, Decode.py:112-165; here it keeps its rows and is ignored).
        Step 0 expands slot 0 only (Beam.py:48-51): the other slots start at -inf.  Then the self-attention histories
        follow the back-pointers - through the lineage table the same launch maintains (``st.anc``: the cache rows stay
        where they were written), or, on the fall-back attention path, by permuting the caches - and the step counter
        advances."""
        embed = (self.model.decoder._st.emb, self.model.decoder._st.pe, st.x_in) if st.x_in is not None else None
        if st.ctc is not None:     # joint CTC / attention: pre-beam, CTC prefix scores, the joint advance (st_amd.ctc_decode)
            st.ctc.advance(st, logits, self.model.vocab_size, Constants.EOS, st.anc, st.anc is not None, embed, lm=st.lm, bias=st.bias)
        elif st.pre is not None:   # attention + language model and / or context bias: pre-beam, their terms, the joint advance
            # with weight 0 (st_amd.ngram.PreBeamSearch)
            st.pre.advance(st, logits, self.model.vocab_size, Constants.EOS, st.anc, st.anc is not None, embed, lm=st.lm, bias=st.bias)
        else:
            nv.beam_advance(logits, self.model.vocab_size, st.beam, st.step, Constants.EOS, st.scores, st.tokens, st.done,
                            st.lengths, st.hist_scores, st.back, st.toks, st.order, work=st.beam_work, anc=st.anc,
                            advance_step=st.anc is not None, embed=embed)
        if st.anc is None:         # (with the lineage table the cache rows stay where they were written, and the merge
            nv.cache_reorder(st.caches, st.order, st.step, st.beam)             # launch has advanced the step counter)
            st.step.add_(1)
        if st.need_c_len:          # (only the fall-back self-attention path reads the cache length vector)
            st.c_len.add_(1)

    @torch.no_grad()
    def decode_batch(self, src_batch):
        """src_batch = (inputs [B, T, F] fp32, input_lengths [B]) -> (all_hyp, all_scores) as Decode.py:168-177:
        all_hyp[b] = the n_best token lists of utterance b, all_scores[b] = their scores (tensor[n_best])."""
        if not self.use_graph:
            return self._decode_batch(src_batch)
        # the whole call runs on this object's side stream: a step can then be captured where it is (graph capture needs
        # a non-default stream) without hopping streams in the middle of the batch
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        cur = torch.cuda.current_stream()
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            out = self._decode_batch(src_batch)
        cur.wait_stream(self._side)
        return out

    def _init_state(self, src_batch, beam, arena, search=True, ctc=None, encoded=None, lm=False, bias=None):
        """Encoder pass + the device state of a search over ``beam`` hypotheses per utterance (call inside ``arena.scope()``).
        ``ctc`` = (pre-beam width K, weight): also the CTC side of a joint search (st_amd.ctc_decode.CtcSearch).
        ``encoded`` = (enc, in_rows): the encoder output of this batch, already computed in this scope (None: run the encoder).
        ``lm``: also the language-model side of the search (st_amd.ngram.LmSearch: the histories [-1, .., -1, BOS]).
        ``bias``: a ContextBias - also the biasing side of the search (st_amd.biasing.BiasSearch: every state at the root)."""
        inputs, in_len = src_batch
        model, dev = self.model, self.device
        B = inputs.shape[0]
        if encoded is None:
            inputs = inputs.to(dev)
            t_max = int(in_len.max())
            enc, in_rows = model.encoder.forward_rows(inputs[:, :t_max], in_len)    # packed [sum T, d]
        else:
            enc, in_rows = encoded
        dec = model.decoder
        d, S, n = dec.d_model, self.max_steps, B * beam
        if S > dec.position_enc.pe.shape[1]:
            raise ValueError("Decode: max_steps %d exceeds the decoder's positional-encoding table" % S)
        st = _DecodeState()
        st.B, st.beam, st.n = B, beam, n
        st.ctc = None if ctc is None else ctc_decode.CtcSearch(self.ctc_head, enc, in_rows, beam, ctc[0], ctc[1])
        st.lm = None
        if lm:
            w = st.ctc.weight if st.ctc is not None else 0.0
            st.lm = ngram.LmSearch(self.lm, B, beam, self.lm_weight / (1.0 - w), self.lm_length_bonus / (1.0 - w))
        st.bias = None
        if bias is not None:
            w = st.ctc.weight if st.ctc is not None else 0.0
            st.bias = biasing.BiasSearch(bias, B, beam, self.bias_weight / (1.0 - w))
        st.pre = None
        if st.ctc is None and (st.lm is not None or st.bias is not None):
            st.pre = ngram.PreBeamSearch(B, beam, self.lm_pre_beam if self.lm_pre_beam is not None else self.bias_pre_beam, dev)
        st.chains = dec.row_chains(arena)          # None: the layers do not fit the row-chain kernel
        st.need_c_len = not (dec.d_model // dec.layer_stack[0].slf_attn.n_head == 64 and self.max_steps <= 128)
        st.cross = []
        for layer in dec.layer_stack:                                               # once per utterance
            s = layer.enc_attn._st
            kv = torch.empty(enc.shape[0], 2 * d, dtype=BF16, device=dev)
            nv.gemm(enc, s.w_kv, kv, bias=s.b_kv)
            st.cross.append(kv)
        H = dec.layer_stack[0].slf_attn.n_head
        ar = torch.arange(n, dtype=I32, device=dev)
        st.q_off, st.q_one, st.c_off = ar, torch.ones(n, dtype=I32, device=dev), ar * S
        st.c_len = torch.ones(n, dtype=I32, device=dev)
        st.u_off = torch.arange(B, dtype=I32, device=dev) * beam
        st.u_len = torch.full((B,), beam, dtype=I32, device=dev)
        st.k_off, st.k_len, st.max_k = in_rows.off, in_rows.len, int(in_rows.max_len)
        st.lse = torch.empty(H * n, dtype=F32, device=dev)
        st.caches = torch.zeros(len(dec.layer_stack), n, S, 2 * d, dtype=BF16, device=dev)
        st.tokens = torch.full((n,), Constants.BOS, dtype=torch.long, device=dev)
        st.step = torch.zeros(1, dtype=torch.long, device=dev)
        st.scores = torch.full((B, beam), float("-inf"), dtype=F32, device=dev)
        st.scores[:, 0] = 0.0
        st.done = torch.zeros(B, dtype=torch.bool, device=dev)
        st.lengths = torch.zeros(B, dtype=torch.long, device=dev)
        st.hist_scores = torch.zeros(S, B, beam, dtype=F32, device=dev)
        st.back = torch.zeros(S, B, beam, dtype=torch.long, device=dev)
        st.toks = torch.zeros(S, B, beam, dtype=torch.long, device=dev)
        st.order = torch.zeros(n, dtype=torch.long, device=dev)
        st.beam_work = torch.zeros(nv.beam_work_words(B, beam), dtype=torch.long, device=dev)  # st_beam_advance's keys + tickets
        # the lineage table of the decode-shaped self-attention (cache row of every earlier position of every hypothesis):
        # the caches are then never permuted.  The fall-back self-attention reads its own rows: st_cache_reorder stays.
        st.anc = None if st.need_c_len or model.vocab_size > 5120 else \
            torch.arange(n, dtype=I32, device=dev).unsqueeze(1).repeat(1, S).contiguous()
        # the decoder input of the current step: written by st_beam_advance for the tokens it chose (no st_embed_step launch per
        # step); step 0's is made here.  Only a search advances that way (search=False: the caller feeds the tokens).
        st.x_in = None
        if search and st.anc is not None:
            st.x_in = nv.embed_step(st.tokens, dec._st.emb, dec._st.pe, st.step, torch.empty(n, d, dtype=BF16, device=dev))
        return st

    @torch.no_grad()
    def score_hypotheses(self, src_batch, hyps, ctc_weight=None):
        """Teacher-forced log-probability of ONE given token list per utterance, computed by the DECODE path (the step
        kernels of ``decode_batch``: KV cache, shared encoder keys, row chains) with the search switched off - the tokens
        are fed, not chosen.  -> tensor [B] fp32.  Not in the reference (its Decode has no scoring entry point): this is what
        lets the decode kernels be held to the fp64 oracle WITHOUT the selection bias of an arg-max over noisy scores
        (tests/test_decode_cpu.py::run_decode), and it rescores n-best lists.
        ``ctc_weight`` = w (needs the CTC head): the JOINT score of the search, sum over the tokens of
        (1 - w) log p_att + w (psi(prefix + token) - psi(prefix)) through the joint search's own kernels (st_ctc_prefix_score,
        st_beam_advance_joint with the token fed as the only candidate) - for a hypothesis that ends in EOS
        (1 - w) sum log p_att + w log p_ctc(hypothesis without EOS)."""
        B = src_batch[0].shape[0]
        assert len(hyps) == B and all(len(h) <= self.max_steps for h in hyps)
        V, dev = self.model.vocab_size, self.device
        joint = ctc_weight is not None
        if joint:
            w = float(ctc_weight)
            if not 0.0 <= w < 1.0:
                raise ValueError("score_hypotheses: ctc_weight must lie in [0, 1), got %r" % w)
            if self.ctc_head is None:
                raise ValueError("score_hypotheses: ctc_weight needs the CTC head (Decode(..., ctc_head=...))")
        arena = arena_of(self.model)
        total = torch.zeros(B, dtype=torch.float64, device=dev)
        ctc_total = torch.zeros(B, dtype=torch.float64, device=dev)
        with arena.scope():
            st = self._init_state(src_batch, 1, arena, search=False, ctc=(1, w) if joint else None)
            steps = max(len(h) for h in hyps)
            fed = torch.full((steps, B), Constants.PAD, dtype=torch.long)
            live = torch.zeros(steps, B, dtype=torch.float64)
            for b, h in enumerate(hyps):
                fed[:len(h), b] = torch.tensor(h, dtype=torch.long)
                live[:len(h), b] = 1.0
            fed, live = fed.to(dev), live.to(dev)
            for t in range(steps):
                lp = torch.log_softmax(self._step(st)[:, :V].double(), -1)
                total += lp.gather(1, fed[t].unsqueeze(1)).squeeze(1) * live[t]
                if joint:                               # the fed token as the only candidate of the joint kernels
                    cs = st.ctc
                    cs.ids.copy_(fed[t].unsqueeze(1))
                    cs.lp.copy_(lp.gather(1, fed[t].unsqueeze(1)))
                    cs.score(Constants.EOS, None)
                    ctc_total += torch.where(live[t] > 0, cs.delta[:, 0].double(), torch.zeros_like(ctc_total))
                    nv.beam_advance_joint(cs.ids, cs.lp, cs.delta, cs.weight, 1, st.step, Constants.EOS, st.scores, st.tokens,
                                          st.done, st.lengths, st.hist_scores, st.back, st.toks, st.order, ctc=cs.state())
                st.tokens.copy_(fed[t])                 # beam 1: no back-pointers, the cache row stays where it is
                st.step.add_(1)
                if st.need_c_len:
                    st.c_len.add_(1)
        if joint and w > 0.0:
            return ((1.0 - w) * total + w * ctc_total).float()
        return total.float()

    @torch.no_grad()
    def ctc_greedy(self, src_batch):
        """Greedy CTC decoding with the CTC head: per utterance the frame arg-max of its CTC logits (``st_ctc_best_path``),
        repeats collapsed and blanks dropped -> list of B label lists."""
        if self.ctc_head is None:
            raise ValueError("ctc_greedy: needs the CTC head (Decode(..., ctc_head=...))")
        inputs, in_len = src_batch
        model, dev = self.model, self.device
        inputs = inputs.to(dev)
        t_max = int(in_len.max())
        with arena_of(model).scope():
            enc, in_rows = model.encoder.forward_rows(inputs[:, :t_max], in_len)
            logits = ctc_decode.head_logits(self.ctc_head, enc)
            best = nv.ctc_best_path(logits, self.ctc_head.ctc_proj.weight.shape[0],
                                    torch.empty(logits.shape[0], dtype=I32, device=dev)).cpu().tolist()
        blank, out, o = int(self.ctc_head.blank), [], 0
        for T in in_len.tolist():
            labels, prev = [], None
            for k in best[o:o + int(T)]:
                if k != prev and k != blank:
                    labels.append(k)
                prev = k
            out.append(labels)
            o += int(T)
        return out

    def _encode(self, src_batch):
        """-> (enc bf16 [sum T, d], in_rows) of the batch (call inside ``arena.scope()``)."""
        inputs, in_len = src_batch
        return self.model.encoder.forward_rows(inputs.to(self.device)[:, :int(in_len.max())], in_len)

    def _ctc_widths(self, who, beam, n_best):
        from st_amd import ctc_beam
        if self.ctc_head is None:
            raise ValueError("%s: needs the CTC head (Decode(..., ctc_head=...))" % who)
        beam = int(self.opt.beam_size if beam is None else beam)
        n_best = int(self.opt.n_best if n_best is None else n_best)
        return ctc_beam.check_widths(self.model.vocab_size, beam, getattr(self.opt, "ctc_beam_pre_beam", None), n_best)

    def _first_pass_lm(self, who, lm_weight, lm_length_bonus):
        """-> (lambda, beta) of the CTC prefix beam search's own LM term: the arguments, else opt.ctc_lm_weight /
        opt.ctc_lm_length_bonus (default 0: the LM-less search); ValueError for a weight < 0 or a weight without the model."""
        from st_amd import ctc_beam
        lam, beta, _ = ctc_beam.check_lm(self.lm, self.ctc_lm_weight if lm_weight is None else lm_weight,
                                         self.ctc_lm_length_bonus if lm_length_bonus is None else lm_length_bonus, who=who)
        return lam, beta

    @torch.no_grad()
    def ctc_beam(self, src_batch, beam=None, n_best=None, lm_weight=None, lm_length_bonus=None):
        """CTC prefix beam search with the CTC head (st_amd.ctc_beam: the encoder-only first pass): per utterance the ``n_best``
        most probable label lists under the head, each summed over its alignments.  -> (all_hyp, all_scores) shaped as
        decode_batch's: all_hyp[b] = n_best label lists WITHOUT EOS (as ctc_greedy), all_scores[b] = their log-probabilities
        (tensor[n_best], best first; an utterance with fewer live prefixes: [] with -inf).  ``beam`` defaults to
        ``opt.beam_size``, ``n_best`` to ``opt.n_best``; ``opt.ctc_beam_pre_beam`` (default ``beam``): classes considered per row.
        One encoder pass, one st_ctc_beam_search launch and one host read per batch; the decoder does not run.
        ``lm_weight`` = lambda / ``lm_length_bonus`` = beta (default ``opt.ctc_lm_weight`` / ``opt.ctc_lm_length_bonus``, both 0:
        off) with a language model: the search ranks by log p_ctc(h) + lambda log p_lm(h) + beta |h| EVERY FRAME (the same single
        launch, st_ctc_beam_search_lm) and, at the end, with the EOS term; the lists come back sorted by that rank and the method
        returns a third value, ``fused`` [b] = tensor[n_best] of lambda log p_lm(h . EOS) + beta (|h| + 1): all_scores stays the pure
        log p_ctc, all_scores + fused is the rank."""
        from st_amd import ctc_beam
        beam, K, N = self._ctc_widths("ctc_beam", beam, n_best)
        lam, beta = self._first_pass_lm("ctc_beam", lm_weight, lm_length_bonus)
        with arena_of(self.model).scope():
            enc, in_rows = self._encode(src_batch)
            out = ctc_beam.search_rows(self.ctc_head, enc, in_rows, beam, K, N, lm=self.lm, lm_weight=lam, lm_length_bonus=beta)
            hyps, scores = out.lists()
        if out.fused is None:
            return hyps, list(scores.to(self.device).unbind(0))
        return hyps, list(scores.to(self.device).unbind(0)), list(out.fused.unbind(0))

    def _nbest_rows(self, src_batch, nbest, arena, encoded=None):
        """Teacher-forced log p_att(h . EOS) of nbest[b][j] -> f64 [B, N] on the device (call inside ``arena.scope()``): the decode
        path with the search off, N rows per utterance - one encoder pass (or none: ``encoded``), one cross K|V projection and one
        decoder step per position for ALL rows."""
        B, V, dev = src_batch[0].shape[0], self.model.vocab_size, self.device
        if len(nbest) != B:
            raise ValueError("score_nbest: %d n-best lists for %d utterances" % (len(nbest), B))
        N = max(1, max(len(hs) for hs in nbest))
        steps = 1 + max([len(h) for hs in nbest for h in hs] or [0])
        if steps > self.max_steps:
            raise ValueError("score_nbest: a hypothesis of %d labels plus EOS exceeds max_steps = %d" % (steps - 1, self.max_steps))
        fed = torch.full((steps, B * N), Constants.PAD, dtype=torch.long)
        live = torch.zeros(steps, B * N, dtype=torch.float64)
        have = torch.zeros(B * N, dtype=torch.bool)
        for b, hs in enumerate(nbest):
            for j, h in enumerate(hs):
                if h is None:
                    continue
                h = [int(k) for k in h]
                if any(k < 0 or k >= V for k in h):
                    raise ValueError("score_nbest: utterance %d has a token outside the vocabulary [0, %d)" % (b, V))
                fed[:len(h) + 1, b * N + j] = torch.tensor(h + [Constants.EOS], dtype=torch.long)
                live[:len(h) + 1, b * N + j] = 1.0
                have[b * N + j] = True
        fed, live, have = fed.to(dev), live.to(dev), have.to(dev)
        st = self._init_state(src_batch, N, arena, search=False, encoded=encoded)
        total = torch.zeros(B * N, dtype=torch.float64, device=dev)
        for t in range(steps):
            lp = torch.log_softmax(self._step(st)[:, :V].double(), -1)
            total += lp.gather(1, fed[t].unsqueeze(1)).squeeze(1) * live[t]
            st.tokens.copy_(fed[t])                     # rows stay where they are: no back-pointers, no cache moves
            st.step.add_(1)
            if st.need_c_len:
                st.c_len.add_(1)
        return torch.where(have, total, torch.full_like(total, float("-inf"))).view(B, N)

    @torch.no_grad()
    def score_nbest(self, src_batch, nbest):
        """Teacher-forced attention scores of an n-best list: nbest[b] = up to N label lists WITHOUT EOS (``ctc_beam``'s) ->
        f32 [B, N], log p_att(h . EOS) of each, -inf for a missing one (a shorter nbest[b], or None in it).  The decode path of
        ``score_hypotheses`` with N rows per utterance in ONE pass: the encoder, the cross-attention K|V projections and every
        decoder step are shared by all B x N hypotheses; no top-k, no cache lineage, no pre-beam."""
        arena = arena_of(self.model)
        with arena.scope():
            return self._nbest_rows(src_batch, nbest, arena).float()

    @torch.no_grad()
    def lm_score(self, nbest):
        """Language-model scores of an n-best list: nbest[b] = up to N label lists WITHOUT EOS -> f32 [B, N], log p_lm(h . EOS) of
        each (the history starts at BOS), -inf for a missing one (a shorter nbest[b], or None in it).  One st_ngram_score_seq launch
        over all lists; the positions are summed in fp64 on the device."""
        if self.lm is None:
            raise ValueError("lm_score: needs the language model (Decode(..., lm=...))")
        return ngram.score_lists(self.lm, nbest, Constants.EOS, Constants.BOS)

    @torch.no_grad()
    def bias_score(self, nbest):
        """Phrase rewards of an n-best list: nbest[b] = up to N label lists WITHOUT EOS -> f32 [B, N], reward(h) of each (the sum of
        w_p |p| over the occurrences of the context bias's phrases; NOT multiplied by ``bias_weight``), -inf for a missing one (a
        shorter nbest[b], or None in it).  One st_bias_score_seq launch over all lists; the positions are summed in fp64 on the
        device."""
        if self.bias is None:
            raise ValueError("bias_score: needs the context bias (Decode(..., bias=...))")
        return biasing.score_lists(self.bias, nbest, Constants.EOS)

    @torch.no_grad()
    def decode_two_pass(self, src_batch, ctc_weight=None, beam=None, n_best=None, lm_weight=None, first_pass_lm_weight=None,
                        first_pass_lm_length_bonus=None, bias_weight=None):
        """Two-pass decoding ("attention rescoring"): the encoder once, a CTC prefix beam search for ``beam`` hypotheses
        (``ctc_beam``), their teacher-forced attention scores in one batched pass (``score_nbest``), and the joint score
        (1 - w) log p_att(h . EOS) + w log p_ctc(h) - w = ``ctc_weight``, default ``opt.ctc_weight`` - re-sorted, the ``n_best``
        kept.  -> (all_hyp, all_scores) as decode_batch returns them, EOS closing every list (``align`` takes them as they are).
        Hypotheses are capped at max_steps - 1 labels.  With a language model and ``lm_weight`` = lambda (default
        ``opt.lm_weight``) > 0 or ``opt.lm_length_bonus`` = beta != 0 the score also has lambda log p_lm(h . EOS) + beta (len(h) + 1)
        (``lm_score``: one more launch).  ``first_pass_lm_weight`` / ``first_pass_lm_length_bonus`` (default ``opt.ctc_lm_weight`` /
        ``opt.ctc_lm_length_bonus``, both 0: off): the language model inside the first pass as in ``ctc_beam`` - it changes WHICH
        ``beam`` hypotheses are rescored, nothing else: the final score is the same three-term sum with the pure log p_ctc.
        With a context bias and ``bias_weight`` = b (default ``opt.bias_weight``) > 0 the score also has b x reward(h)
        (``bias_score``: one more launch); the first pass is not biased."""
        from st_amd import ctc_beam
        lam1, beta1 = self._first_pass_lm("decode_two_pass", first_pass_lm_weight, first_pass_lm_length_bonus)
        w = float((getattr(self.opt, "ctc_weight", None) or 0.0) if ctc_weight is None else ctc_weight)
        if not 0.0 <= w < 1.0:
            raise ValueError("decode_two_pass: ctc_weight must lie in [0, 1), got %r" % w)
        lam = float(self.lm_weight if lm_weight is None else lm_weight)
        if not lam >= 0.0:
            raise ValueError("decode_two_pass: lm_weight must be >= 0, got %r" % lam)
        if self.lm is None and lm_weight is not None and lam > 0.0:
            raise ValueError("decode_two_pass: lm_weight needs the language model (Decode(..., lm=...))")
        fuse = self.lm is not None and (lam > 0.0 or self.lm_length_bonus != 0.0)
        bw = float(self.bias_weight if bias_weight is None else bias_weight)
        if not bw >= 0.0 or not math.isfinite(bw):
            raise ValueError("decode_two_pass: bias_weight must be a finite number >= 0, got %r" % bw)
        if self.bias is None and bias_weight is not None and bw > 0.0:
            raise ValueError("decode_two_pass: bias_weight needs the context bias (Decode(..., bias=...))")
        beam, K, N = self._ctc_widths("decode_two_pass", beam, n_best)
        if self.max_steps < 2:
            raise ValueError("decode_two_pass: max_steps must allow a label and EOS")
        arena = arena_of(self.model)
        with arena.scope():
            enc, in_rows = self._encode(src_batch)
            first = ctc_beam.search_rows(self.ctc_head, enc, in_rows, beam, K, None, max_len=min(255, self.max_steps - 1), lm=self.lm,
                                         lm_weight=lam1, lm_length_bonus=beta1)
            hyps, ctc_scores = first.lists()
            fin = torch.isfinite(ctc_scores)
            nbest = [[h if bool(fin[b, j]) else None for j, h in enumerate(hs)] for b, hs in enumerate(hyps)]
            att = self._nbest_rows(src_batch, nbest, arena, encoded=(enc, in_rows)).cpu()
            extra = None
            if fuse:
                lens1 = torch.tensor([[len(h) + 1 for h in hs] for hs in hyps], dtype=torch.float64)
                extra = self.lm_length_bonus * lens1
                if lam > 0.0:
                    extra = extra + lam * self.lm_score(nbest).double().cpu()
            if self.bias is not None and bw > 0.0:
                boost = bw * self.bias_score(nbest).double().cpu()
                boost = torch.where(torch.isfinite(boost), boost, torch.zeros_like(boost))     # (a missing list: att is -inf already)
                extra = boost if extra is None else extra + boost
        all_hyp, scores = ctc_beam.combine(hyps, ctc_scores, att, w, N, Constants.EOS, extra=extra)
        return all_hyp, list(scores.to(self.device).unbind(0))

    @torch.no_grad()
    def align(self, src_batch, hyps, strip_eos=True):
        """CTC forced alignment of ONE token list per utterance (``hyps[b]``, e.g. ``decode_batch(...)[0][b][0]``) with the CTC
        head: WHEN each token was spoken.  -> a list of B pairs ``(items, score)``: ``items`` = one ``(token, start, end, logp)``
        per token - the token occupies the encoder rows [start, end) of its utterance (contiguous, at least one row, in order),
        ``logp`` = the sum of the head's log-probabilities of the token over its own rows (a per-token confidence) - and
        ``score`` = the log-probability of the whole best path (blank rows included).  An utterance whose rows cannot spell its
        tokens (fewer rows than tokens + adjacent repeats) returns ``([], -inf)``.

        Rows and time: row t stands at raw feature frame ``t * interval``, i.e. at ``t * interval * 10 ms`` for 10 ms frames,
        ``interval`` as in ``st_amd.features.stack_frames`` (1 without frame stacking).

        ``strip_eos=True`` drops one trailing EOS (the prefix scorer's convention: EOS is not a CTC label); ``strip_eos=False``
        aligns the closing token as a label (the convention of JointTrainStep's labels).  ValueError: no CTC head, a leading BOS,
        a token outside the vocabulary, more than 255 labels.  One encoder pass, one st_ctc_align launch and one host read per
        batch (st_amd.ctc_align)."""
        from st_amd import ctc_align
        if self.ctc_head is None:
            raise ValueError("align: needs the CTC head (Decode(..., ctc_head=...))")
        inputs, in_len = src_batch
        B, V = inputs.shape[0], self.model.vocab_size
        if len(hyps) != B:
            raise ValueError("align: %d token lists for %d utterances" % (len(hyps), B))
        labs = []
        for b, h in enumerate(hyps):
            h = [int(k) for k in h]
            if h and h[0] == Constants.BOS:
                raise ValueError("align: utterance %d starts with BOS - pass the tokens after it" % b)
            if strip_eos and h and h[-1] == Constants.EOS:
                h = h[:-1]
            if any(k < 0 or k >= V for k in h):
                raise ValueError("align: utterance %d has a token outside the vocabulary [0, %d)" % (b, V))
            if len(h) > nv.CTC_LOSS_MAX_L:
                raise ValueError("align: utterance %d has %d labels, at most %d are supported" % (b, len(h), nv.CTC_LOSS_MAX_L))
            labs.append(h)
        L = max(1, max(len(h) for h in labs))
        labels = torch.zeros(B, L, dtype=torch.long)
        for b, h in enumerate(labs):
            labels[b, :len(h)] = torch.tensor(h, dtype=torch.long)
        lengths = torch.tensor([len(h) for h in labs], dtype=torch.long)
        model, dev = self.model, self.device
        inputs = inputs.to(dev)
        t_max = int(in_len.max())
        with arena_of(model).scope():
            enc, in_rows = model.encoder.forward_rows(inputs[:, :t_max], in_len)
            al = ctc_align.align_rows(self.ctc_head, enc, in_rows, labels.to(dev), lengths)
            host = torch.cat([al.spans.reshape(B, 2 * L).double(), al.token_logp.double(), al.score.double().unsqueeze(1)], 1).cpu()
        self.alignment = al        # the device tensors of the last call (st_amd.ctc_align.Alignment: the per-row path, lp, classes)
        out = []
        for b, h in enumerate(labs):
            row = host[b].tolist()
            score = row[3 * L]
            if score == float("-inf"):
                out.append(([], score))
                continue
            out.append(([(k, int(row[2 * j]), int(row[2 * j + 1]), row[2 * L + j]) for j, k in enumerate(h)], score))
        return out

    def _decode_batch(self, src_batch):
        inputs, in_len = src_batch
        model, dev = self.model, self.device
        B, beam, n_best = inputs.shape[0], int(self.opt.beam_size), int(self.opt.n_best)
        arena = arena_of(model)
        with arena.scope():
            st = self._init_state(src_batch, beam, arena,
                                  ctc=(self.ctc_pre_beam, self.ctc_weight) if self.ctc_pre_beam is not None else None, lm=self._lm_on,
                                  bias=self.bias if self._bias_on else None)
            S = self.max_steps

            def one_step():
                self._advance(st, self._step(st))

            graph, steps_done = None, 0
            # the first call on this object runs step 0 eagerly (kernel modules loaded, allocator warm) and captures at step
            # 1; later calls capture before step 0 - the host records the step while the GPU is still busy with the encoder
            capture_at = 0 if self._warm else 1
            while steps_done < S:
                if self.use_graph and steps_done == capture_at and graph is None:
                    # every later step is a replay of ONE captured step: the position, the cache length, the tokens and the
                    # beams are device state
                    # (captured by hand, on decode_batch's side stream: `with torch.cuda.graph(...)` also runs gc.collect() and
                    # torch.cuda.empty_cache() - 4 ms of every decode_batch call, a tenth of a 32-utterance batch)
                    if not self._warm:
                        torch.cuda.current_stream().synchronize()      # (as torch.cuda.graph does before a capture)
                    graph = torch.cuda.CUDAGraph()
                    graph.capture_begin(**(dict(capture_error_mode="thread_local") if torch.distributed.is_initialized() else {}))
                    try:
                        one_step()
                    except BaseException:
                        # a wrapper raised mid-capture (non-zero status, out of memory in the private pool): leave
                        # capture mode before the error travels on, or every later call on this stream fails with
                        # errors that hide this one
                        try:
                            graph.capture_end()
                        except Exception:  # noqa: BLE001 - the original error is the one to report
                            pass
                        graph = None
                        raise
                    graph.capture_end()
                    self._warm = True
                if graph is not None:
                    graph.replay()
                else:
                    one_step()
                steps_done += 1
                # the EOS test of Beam.py:70 lives on the device; the host looks at it every few steps only
                if (steps_done % 8 == 0 or not self.use_graph) and bool(st.done.all()):
                    break

        # ---- read-out (Beam.sort_scores / Beam.get_hypothesis, Beam.py:76-116) from the device trellis ------------------
        # The trellis crosses to the host ONCE and is walked as plain lists: per utterance the scores are sorted as
        # Beam.sort_scores does and each of the n_best slots is followed back through the back-pointers.  (Building a Beam
        # object per utterance - three lists of per-step tensor views, a stack + tolist per hypothesis - was 3.0 of the
        # 28.6 ms of a 32-utterance call; before that the read-out ran on the device: a sort, two stacks and three
        # synchronising .tolist() per utterance.)
        lengths = st.lengths.tolist()
        back_h, toks_h, scores_h = st.back.cpu().tolist(), st.toks.cpu().tolist(), st.scores.cpu()
        all_hyp, best = [], []
        for b in range(B):
            scores, slots = torch.sort(scores_h[b], 0, True)
            best.append(scores[:n_best])
            hyps = []
            for slot in slots[:n_best].tolist():
                out = []
                for step in range(lengths[b] - 1, -1, -1):
                    out.append(toks_h[step][b][slot])
                    slot = back_h[step][b][slot]
                out.reverse()
                hyps.append(out)
            all_hyp.append(hyps)
        all_scores = list(torch.stack(best).to(dev).unbind(0)) if best else []
        self.beams = None
        return all_hyp, all_scores


class _DecodeState(object):
    """Device-resident state of one decode_batch call (attribute bag)."""
    pass

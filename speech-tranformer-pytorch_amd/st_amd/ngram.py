"""Back-off n-gram language model over the model's own token ids, for shallow fusion in beam search and rescoring
(``transformer.Decode`` with ``lm=...``: the third term of (1 - w) log p_att + w log p_ctc + lambda log p_lm).

Host side, fp64: ``NGramLM`` holds the table ``{(w_1 .. w_m): (logp, backoff)}`` in natural log (ARPA's content), read from an
ARPA file (``from_arpa``), given directly (``from_table``) or estimated from token lists (``estimate``: interpolated absolute
discounting, stored in back-off form).  ``logp(history, token)`` is the definition itself:

    logp(h, c) = table[h . c].logp                       if h . c is stored
               = backoff(h) + logp(h without its oldest token, c)      otherwise (backoff 0 for a context that is not stored)
    logp((), c) = oov_logp                               for a token without a unigram

Device side: ``lm.to(device)`` builds the trie the kernels of csrc/st_ngram.hip walk (``DeviceTrie``).  Contexts are keyed in
REVERSE: the node of the n-gram (w_1 .. w_m) is reached by w_m, w_{m-1}, .., w_1, so ONE walk c, h_1, h_2, .. (h_1 the most
recent token) finds the longest stored n-gram that ends in c, and one walk h_1, h_2, .. the back-off weights of every context
length.  Depth 1 is dense (node id = token id); below it the children of a node are consecutive nodes sorted by token (CSR:
``child_lo`` i32 [nodes + 1]).  Before building, the table is COMPLETED: a stored n-gram whose suffix (oldest token dropped) is
missing gets that suffix inserted with the log-probability the back-off rule gives it and back-off 0 - no probability changes,
and "walk until a child is missing" becomes correct.  Values are rounded to fp32 once, there.

Score of candidate c after the history h_k .. h_1 (k <= N - 1 valid tokens), as the kernels compute it: m = the depth the walk
c, h_1, .. reaches (no unigram: the value is oov_logp and m counts as 1), bo_j = the back-off of the context of length j on
the walk h_1, .. (0 from the first missing child on); score = logp_m + bo_m + bo_(m+1) + .. + bo_k, in fp32, in that order."""
import math

import numpy as np
import torch

import transformer.Constants as Constants

from . import native as nv

F32, I32, I64 = torch.float32, torch.int32, torch.int64
LN10 = math.log(10.0)
OOV_LOGP = -99.0 * LN10          # ARPA's customary zero
MAX_ORDER, MAX_V = 5, 5120       # the kernels' history registers; st_beam_pre_beam's vocabulary limit
NO_UNIGRAM = float("inf")        # the dense depth-1 slot of a token without a unigram (a log-probability is never +inf)


def _check_shape(order, V):
    if not 2 <= int(order) <= MAX_ORDER:
        raise ValueError("NGramLM: order must lie in [2, %d], got %r" % (MAX_ORDER, order))
    if not 1 <= int(V) <= MAX_V:
        raise ValueError("NGramLM: the vocabulary must lie in [1, %d], got %r" % (MAX_V, V))


def complete(table, oov_logp=OOV_LOGP):
    """-> a copy of ``table`` closed under "drop the oldest token": every missing suffix is inserted with the back-off rule's
    log-probability and back-off 0 (longest n-grams first, so an inserted suffix is itself completed)."""
    lm = NGramLM.__new__(NGramLM)
    lm.table, lm.oov_logp = dict(table), float(oov_logp)
    lm.order = 1 + max([len(g) for g in table] or [1])
    out = lm.table
    for g in sorted(table, key=len, reverse=True):
        s = g[1:]
        while len(s) >= 1 and s not in out:
            out[s] = (lm.logp(s[:-1], s[-1]), 0.0)
            s = s[1:]
    return out


class NGramLM(object):
    """Back-off n-gram model of order N (2..5) over token ids [0, V), V <= 5120.  ``table``: {tuple of m token ids (oldest first):
    (logp, backoff)}, natural log.  ``oov_logp``: the unigram slot of a token without a unigram (-inf: the token is vetoed)."""

    def __init__(self, table, order, V, oov_logp=OOV_LOGP):
        _check_shape(order, V)
        self.order, self.V, self.oov_logp = int(order), int(V), float(oov_logp)
        if math.isnan(self.oov_logp) or self.oov_logp > 0.0:
            raise ValueError("NGramLM: oov_logp must be a log-probability (<= 0, -inf allowed), got %r" % oov_logp)
        self.table = {}
        for g, val in table.items():
            g = tuple(int(k) for k in g)
            if not 1 <= len(g) <= self.order or any(k < 0 or k >= self.V for k in g):
                raise ValueError("NGramLM: n-gram %r does not fit order %d over [0, %d)" % (g, self.order, self.V))
            lp, bo = (float(val[0]), float(val[1]))
            if math.isnan(lp) or lp == float("inf") or not math.isfinite(bo):
                raise ValueError("NGramLM: n-gram %r has logp %r / backoff %r (logp < +inf, backoff finite)" % (g, lp, bo))
            self.table[g] = (lp, bo)
        self.dropped = 0
        self.device = torch.device("cpu")
        self.trie = None

    # ---- constructors -----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_table(cls, table, order, V, oov_logp=OOV_LOGP):
        return cls(table, order, V, oov_logp)

    @classmethod
    def from_arpa(cls, path_or_lines, symbols, bos=Constants.BOS, eos=Constants.EOS, V=None, oov_logp=OOV_LOGP):
        """An ARPA file (a path, or its lines).  ``symbols``: ARPA word -> token id; ``<s>`` / ``</s>`` map to ``bos`` / ``eos``.
        log10 -> natural log; an n-gram with a word that is not in ``symbols`` is dropped and counted in ``.dropped``; a malformed
        file raises ValueError naming the line.  ``V``: the vocabulary (default: 1 + the largest id of ``symbols``, bos, eos)."""
        if isinstance(path_or_lines, (str, bytes)) or hasattr(path_or_lines, "__fspath__"):
            with open(path_or_lines) as f:
                lines = f.read().splitlines()
        else:
            lines = [str(x).rstrip("\n") for x in path_or_lines]
        sym = dict(symbols)
        sym["<s>"], sym["</s>"] = int(bos), int(eos)

        def bad(no, why):
            return ValueError("ARPA line %d: %s: %r" % (no, why, lines[no - 1] if 0 < no <= len(lines) else ""))

        counts, table, dropped, seen = {}, {}, 0, {}
        section, state, ended = 0, "head", False
        for no, raw in enumerate(lines, 1):
            line = raw.strip()
            if not line:
                continue
            if ended:
                raise bad(no, "text after \\end\\")
            if line == "\\data\\":
                if state != "head":
                    raise bad(no, "a second \\data\\")
                state = "counts"
                continue
            if line == "\\end\\":
                if state == "head":
                    raise bad(no, "\\end\\ before \\data\\")
                ended = True
                continue
            if line.startswith("\\") and line.endswith("-grams:"):
                try:
                    k = int(line[1:-len("-grams:")])
                except ValueError:
                    raise bad(no, "bad section header") from None
                if state == "head" or k != section + 1 or k not in counts:
                    raise bad(no, "section out of order or without a count line")
                section, state = k, "grams"
                seen[k] = 0
                continue
            if state == "head":
                continue                                   # (free text before \data\)
            if state == "counts":
                ok = line.startswith("ngram ") and "=" in line
                if ok:
                    left, right = line[len("ngram "):].split("=", 1)
                    ok = left.strip().isdigit() and right.strip().isdigit()
                if not ok or int(left) != len(counts) + 1:
                    raise bad(no, "bad count line (want 'ngram %d=<count>')" % (len(counts) + 1))
                counts[int(left)] = int(right)
                continue
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise bad(no, "a %d-gram line has %d or %d fields, found %d" % (section, section + 1, section + 2, len(f)))
            try:
                lp10 = float(f[0])
                bo10 = float(f[section + 1]) if len(f) == section + 2 else 0.0
            except ValueError:
                raise bad(no, "a number does not parse") from None
            seen[section] += 1
            if any(w not in sym for w in f[1:section + 1]):
                dropped += 1
                continue
            table[tuple(sym[w] for w in f[1:section + 1])] = (min(lp10 * LN10, 0.0), bo10 * LN10)
        if not ended:
            raise bad(len(lines), "no \\end\\ (the file is cut short)")
        if not counts:
            raise bad(len(lines), "no count lines")
        for k, c in counts.items():
            if seen.get(k) != c:
                raise ValueError("ARPA: 'ngram %d=%d' but the %d-grams section holds %s lines" % (k, c, k, seen.get(k, "no")))
        order = max(counts)
        if V is None:
            V = 1 + max(sym.values())
        lm = cls(table, max(order, 2), V, oov_logp)
        lm.dropped = dropped
        return lm

    @classmethod
    def estimate(cls, token_lists, order, V, discount=0.75, exclude=(Constants.PAD, Constants.BOS), bos=Constants.BOS,
                 eos=Constants.EOS, oov_logp=OOV_LOGP):
        """Interpolated absolute discounting in back-off form, fp64, from token lists (each scored as BOS . list . EOS):
        p(c | h) = max(n(h, c) - D, 0) / n(h) + gamma(h) p(c | h'), gamma(h) = D |{c: n(h, c) > 0}| / n(h), backoff(h) = log gamma(h);
        the unigrams interpolate with the uniform distribution over the tokens not in ``exclude``, so each of those has one.
        (BOS, when excluded, is stored with ``oov_logp`` only to carry the back-off of the context (BOS).)"""
        _check_shape(order, V)
        D = float(discount)
        if not 0.0 < D < 1.0:
            raise ValueError("NGramLM.estimate: the discount must lie in (0, 1), got %r" % discount)
        excl = set(int(k) for k in exclude)
        if eos in excl:
            raise ValueError("NGramLM.estimate: EOS cannot be excluded - every list ends in it")
        U = [k for k in range(V) if k not in excl]
        cnt = [dict() for _ in range(order + 1)]           # cnt[m][h][c]: counts of the m-grams h . c, per context
        for toks in token_lists:
            toks = [int(k) for k in toks]
            if any(k < 0 or k >= V or k in excl for k in toks):
                raise ValueError("NGramLM.estimate: a list holds a token outside [0, %d) or an excluded one" % V)
            seq = [int(bos)] + toks + [int(eos)]
            for i in range(1, len(seq)):
                for j in range(0, min(order - 1, i) + 1):
                    ctx = cnt[j + 1].setdefault(tuple(seq[i - j:i]), {})
                    ctx[seq[i]] = ctx.get(seq[i], 0) + 1
        table, prob = {}, {}
        uni = cnt[1].get((), {})
        n0 = float(sum(uni.values()))
        g0 = D * len(uni) / n0 if n0 > 0 else 1.0
        for c in U:
            prob[(c,)] = (max(uni.get(c, 0) - D, 0.0) / n0 if n0 > 0 else 0.0) + g0 / len(U)

        def p_backoff(h, c):                               # p(c | h) of the model built so far (orders below len(h) + 1)
            if h + (c,) in prob:
                return prob[h + (c,)]
            return gamma.get(h, 1.0) * p_backoff(h[1:], c) if h else 0.0

        gamma = {}
        for m in range(2, order + 1):
            for h, ctx in cnt[m].items():
                n_h = float(sum(ctx.values()))
                gamma[h] = D * len(ctx) / n_h
            for h, ctx in cnt[m].items():
                n_h = float(sum(ctx.values()))
                for c, k in ctx.items():
                    prob[h + (c,)] = max(k - D, 0.0) / n_h + gamma[h] * p_backoff(h[1:], c)
        for g, p in prob.items():
            table[g] = (math.log(p), math.log(gamma[g]) if g in gamma else 0.0)
        for h in gamma:                                    # a context that is no stored n-gram: (BOS) when BOS is excluded
            if h not in table:
                assert len(h) == 1, h
                table[h] = (float(oov_logp), math.log(gamma[h]))
        return cls(table, order, V, oov_logp)

    # ---- the fp64 reference -----------------------------------------------------------------------------------------------------
    def logp(self, history, token):
        """log p(token | history) by the definition; ``history`` oldest first (only its last N - 1 tokens count)."""
        h = tuple(int(k) for k in history)[-(self.order - 1):] if self.order > 1 else ()
        c = int(token)
        total = 0.0
        while True:
            hit = self.table.get(h + (c,))
            if hit is not None:
                return total + hit[0]
            if not h:
                return total + self.oov_logp
            ctx = self.table.get(h)
            total += ctx[1] if ctx is not None else 0.0
            h = h[1:]

    def score_list(self, tokens, bos=Constants.BOS):
        """Sum of logp over ``tokens`` (close the list with EOS yourself), starting from the history (BOS)."""
        hist, total = [int(bos)], 0.0
        for c in tokens:
            total += self.logp(hist, c)
            hist.append(int(c))
        return total

    def completed(self):
        """The suffix-closed table (see ``complete``)."""
        return complete(self.table, self.oov_logp)

    # ---- the device trie --------------------------------------------------------------------------------------------------------
    def to(self, device):
        """-> a model over the same table whose ``trie`` lives on ``device`` (what ``Decode(..., lm=...)`` takes)."""
        out = NGramLM.__new__(NGramLM)
        out.__dict__.update(self.__dict__)
        out.device = torch.device(device)
        out.trie = DeviceTrie(self, device)
        return out


class DeviceTrie(object):
    """The reverse-keyed trie of a completed table.  ``host``: the numpy arrays (child_lo i32 [nodes + 1], tok i32, logp f32, bo
    f32 [nodes]) - node v < V is the unigram of token v (logp +inf: no unigram), the children of a node are the consecutive
    nodes child_lo[node] .. child_lo[node + 1] - 1 sorted by token.  The same arrays as device tensors: child_lo, tok, logp, bo."""

    def __init__(self, lm, device):
        V, N = lm.V, lm.order
        table = lm.completed()
        # a node's key: its n-gram reversed; level d + 1 is ordered by (parent's node id, token)
        levels = [[] for _ in range(N + 1)]
        for g in table:
            levels[len(g)].append(tuple(reversed(g)))
        node_of = {(v,): v for v in range(V)}
        keys = [(v,) for v in range(V)]
        for d in range(2, N + 1):
            level = sorted(levels[d], key=lambda k: (node_of[k[:-1]], k[-1]))
            for k in level:
                node_of[k] = len(keys)
                keys.append(k)
        nodes = len(keys)
        tok = np.array([k[-1] for k in keys], dtype=np.int32)
        logp = np.full(nodes, NO_UNIGRAM, dtype=np.float32)
        bo = np.zeros(nodes, dtype=np.float32)
        n_child = np.zeros(nodes, dtype=np.int64)
        with np.errstate(over="ignore"):
            for i, k in enumerate(keys):
                hit = table.get(tuple(reversed(k)))
                if hit is not None:
                    logp[i], bo[i] = np.float32(hit[0]), np.float32(hit[1])
                if len(k) > 1:
                    n_child[node_of[k[:-1]]] += 1
        child_lo = np.empty(nodes + 1, dtype=np.int32)
        child_lo[0] = V
        child_lo[1:] = V + np.cumsum(n_child)
        assert int(child_lo[-1]) == nodes
        self.V, self.order, self.nodes = V, N, nodes
        self.oov_logp = float(np.float32(lm.oov_logp))
        self.host = dict(child_lo=child_lo, tok=tok, logp=logp, bo=bo)
        self.device = torch.device(device)
        self.child_lo, self.tok, self.logp, self.bo = (torch.from_numpy(self.host[k]).to(device)
                                                       for k in ("child_lo", "tok", "logp", "bo"))

    def rounded_model(self):
        """The host model of the ROUNDED values (what an fp64 reference of the kernels reads): the completed table with every
        logp / backoff as the fp32 the trie holds, and the fp32 oov_logp."""
        h, V = self.host, self.V
        table = {}

        def down(node, rev):
            if h["logp"][node] != NO_UNIGRAM:
                table[tuple(reversed(rev))] = (float(h["logp"][node]), float(h["bo"][node]))
            for ch in range(int(h["child_lo"][node]), int(h["child_lo"][node + 1])):
                down(ch, rev + (int(h["tok"][ch]),))

        for v in range(V):
            down(v, (v,))
        return NGramLM(table, self.order, V, self.oov_logp)


def initial_history(n, order, device, bos=Constants.BOS):
    """hist i32 [n, order - 1] of n fresh hypotheses: [-1, .., -1, BOS] (oldest first, -1 = no token)."""
    hist = torch.full((n, order - 1), -1, dtype=I32, device=device)
    hist[:, -1] = int(bos)
    return hist


def check_options(opt, lm, model, device, beam, joint):
    """-> (lambda, beta, K of the LM-only route or None); ValueError on a bad combination (Decode's constructor)."""
    from . import ctc_decode
    lam = float(getattr(opt, "lm_weight", None) or 0.0)
    beta = float(getattr(opt, "lm_length_bonus", None) or 0.0)
    if not lam >= 0.0 or not math.isfinite(lam) or not math.isfinite(beta):
        raise ValueError("Decode: lm_weight must be a finite number >= 0 (got %r), lm_length_bonus finite (got %r)" % (lam, beta))
    if lm is None:
        return lam, beta, None
    _check_shape(lm.order, lm.V)
    if lm.V != model.vocab_size:
        raise ValueError("Decode: the language model's vocabulary %d differs from the decoder's %d" % (lm.V, model.vocab_size))
    if lm.trie is None or not ctc_decode._same_device(lm.device, device):
        raise ValueError("Decode: the language model lives on %s, the decoder on %s - pass lm.to(device)" % (lm.device, device))
    K = None
    if not joint and (lam > 0.0 or beta != 0.0):
        K = ctc_decode.pre_beam_width(opt, beam)
        if beam > 16 or K < beam or K > 64 or K > model.vocab_size:
            raise ValueError("Decode: a search with a language model needs beam_size <= 16 and ctc_pre_beam in [beam_size, "
                             "min(64, vocabulary)], got beam_size %d, ctc_pre_beam %d" % (beam, K))
    return lam, beta, K


class LmSearch(object):
    """The language-model side of one search over B utterances x ``beam`` hypotheses: the history of every hypothesis (device
    state of the captured step) and the two launches around the joint advance.  ``scale`` / ``bias``: what st_ngram_score adds
    to the pre-beam's ``lp``, lp += scale lm + bias - lambda / (1 - w) and beta / (1 - w), because st_beam_advance_joint weighs
    ``lp`` by (1 - w)."""

    def __init__(self, lm, B, beam, scale, bias):
        self.lm, self.trie, self.B, self.beam = lm, lm.trie, B, beam
        self.scale, self.bias = float(scale), float(bias)
        self.hist = initial_history(B * beam, lm.order, lm.trie.device)

    def score(self, ids, lp, done, eos):
        nv.ngram_score(self.trie, self.hist, ids, done, eos, self.scale, self.bias, lp=lp)

    def follow(self, order, tokens, done, eos):
        nv.ngram_advance(self.hist, order, tokens, done, eos, self.beam)


class PreBeamSearch(object):
    """The search without a CTC head whose candidates carry extra terms - a language model (LmSearch), a context bias
    (st_amd.biasing.BiasSearch), or both: it owns the pre-beam buffers (the joint route uses CtcSearch's)."""

    def __init__(self, B, beam, K, device):
        n = B * beam
        self.ids = torch.zeros(n, K, dtype=I32, device=device)
        self.lp = torch.zeros(n, K, dtype=F32, device=device)
        self.zero = torch.zeros(n, K, dtype=F32, device=device)
        self.ticket = torch.zeros(1, dtype=I64, device=device)

    def advance(self, st, logits, V, eos, anc, advance_step, embed, lm=None, bias=None):
        """One Beam.advance of the head-less route: the K best attention tokens of every hypothesis (NOT the whole vocabulary),
        their LM scores and / or phrase rewards, st_beam_advance_joint with weight 0 and no CTC state, the histories / states."""
        nv.beam_pre_beam(logits, V, self.ids, self.lp)
        if lm is not None:
            lm.score(self.ids, self.lp, st.done, eos)
        if bias is not None:
            bias.score(self.ids, self.lp, st.done, eos)
        nv.beam_advance_joint(self.ids, self.lp, self.zero, 0.0, st.beam, st.step, eos, st.scores, st.tokens, st.done, st.lengths,
                              st.hist_scores, st.back, st.toks, st.order, anc=anc, advance_step=advance_step, ticket=self.ticket,
                              embed=embed, ctc=None)
        if lm is not None:
            lm.follow(st.order, st.tokens, st.done, eos)
        if bias is not None:
            bias.follow(st.order, st.tokens, st.done, eos)


@torch.no_grad()
def score_lists(lm, nbest, eos=Constants.EOS, bos=Constants.BOS):
    """log p_lm(h . EOS) of nbest[b][j] (label lists without EOS; None or a shorter row: missing) -> f32 [B, N] on the LM's
    device, -inf for a missing one: ONE st_ngram_score_seq launch, the positions summed in fp64 on the device."""
    B = len(nbest)
    N = max(1, max((len(hs) for hs in nbest), default=1))
    L = 1 + max([len(h) for hs in nbest for h in hs if h is not None] or [0])
    toks = torch.full((B * N, L), -1, dtype=I32)
    lens = torch.zeros(B * N, dtype=I32)
    have = torch.zeros(B * N, dtype=torch.bool)
    for b, hs in enumerate(nbest):
        for j, h in enumerate(hs):
            if h is None:
                continue
            row = [int(k) for k in h] + [int(eos)]
            toks[b * N + j, :len(row)] = torch.tensor(row, dtype=I32)
            lens[b * N + j] = len(row)
            have[b * N + j] = True
    dev = lm.trie.device
    out = torch.empty(B * N, L, dtype=F32, device=dev)
    nv.ngram_score_seq(lm.trie, toks.to(dev), lens.to(dev), bos, out)
    total = out.double().sum(1)
    return torch.where(have.to(dev), total, torch.full_like(total, float("-inf"))).view(B, N).float()

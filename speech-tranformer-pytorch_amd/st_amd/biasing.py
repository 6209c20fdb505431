"""Contextual biasing ("hot words"): per-request phrases over the model's own token ids that the beam search and the rescoring
reward (``transformer.Decode`` with ``bias=...``: one more term, bias_weight x reward(h), next to the attention, CTC and LM ones).

Host side, fp64 - the definition.  ``ContextBias.from_phrases`` holds {phrase: per-token weight w_p > 0}.  For a label list h

    reward(h) = sum of w_p |p| over every occurrence of every phrase p as a contiguous sub-list of h

(overlapping and nested occurrences all count; ``reward`` counts them by brute force).  A search cannot wait for a phrase to
complete - the partial match would be pruned first - so a growing hypothesis also carries a PROVISIONAL reward for the match in
progress.  With s(h) the Aho-Corasick state of h (the longest suffix of h that is a prefix of some phrase):

    Phi(s)      = depth(s) x max{w_p : p continues beyond s}           (0 when no phrase does)
    B(h)        = reward(h) + Phi(s(h))                                the running bias
    Delta(s, c) = cash[s'] + (Phi[s'] - Phi[s]),  s' = delta(s, c)      the increment of appending c
    Delta(s, EOS) = -Phi[s]                                            EOS revokes what is provisional

cash[s] = the sum of w_p |p| over the phrases that are suffixes of the path to s (accumulated along the fail links here, on the
host).  The increments telescope: a hypothesis closed by EOS carries exactly reward(h); one that has emitted EOS is frozen
(increment 0).  delta(s, c): while s has no child c and s is not the root, s = fail[s]; then the child if there is one, else the
root.

Device side: ``bias.to(device)`` builds the ``DeviceAutomaton`` the kernels of csrc/st_bias.hip walk - nodes numbered
breadth-first, so the children of a node are the consecutive nodes child_lo[node] .. child_lo[node + 1] - 1 sorted by token (the
layout of st_amd.ngram.DeviceTrie), node 0 the root; fail i32, cash / phi f32 [S], rounded to fp32 once, there."""
import math

import numpy as np
import torch

import transformer.Constants as Constants

from . import native as nv

F32, I32, I64 = torch.float32, torch.int32, torch.int64
MAX_PHRASE, MAX_STATES = 32, 65536       # the kernels' fail-loop bound (= the deepest state); the table limit


class Automaton(object):
    """The Aho-Corasick automaton of a phrase set as arrays (numpy; ``cash`` / ``phi`` f64) and the fp64 definition over them:
    child_lo [S + 1], tok / fail / depth [S].  ``ContextBias.automaton`` holds the exact values, ``DeviceAutomaton.rounded_model()``
    the fp32-rounded ones."""

    def __init__(self, child_lo, tok, fail, depth, cash, phi):
        self.child_lo, self.tok, self.fail, self.depth = child_lo, tok, fail, depth
        self.cash, self.phi = np.asarray(cash, dtype=np.float64), np.asarray(phi, dtype=np.float64)
        self.S = int(tok.shape[0])

    def child(self, s, c):
        lo, hi = int(self.child_lo[s]), int(self.child_lo[s + 1])
        i = lo + int(np.searchsorted(self.tok[lo:hi], c))
        return i if i < hi and int(self.tok[i]) == c else -1

    def next(self, s, c):
        """delta(s, c)."""
        c = int(c)
        ch = self.child(s, c)
        while ch < 0 and s != 0:
            s = int(self.fail[s])
            ch = self.child(s, c)
        return ch if ch >= 0 else 0

    def state(self, tokens):
        s = 0
        for c in tokens:
            s = self.next(s, c)
        return s

    def increments(self, tokens, eos=Constants.EOS):
        """Delta of every position of ``tokens`` from the root: a token equal to ``eos`` revokes Phi and freezes the list (0
        from then on)."""
        out, s = [], 0
        for c in tokens:
            if s < 0:
                out.append(0.0)
            elif int(c) == int(eos):
                out.append(-float(self.phi[s]))
                s = -1
            else:
                s2 = self.next(s, c)
                out.append(float(self.cash[s2]) + (float(self.phi[s2]) - float(self.phi[s])))
                s = s2
        return out

    def reward(self, tokens):
        """reward(tokens) through the automaton: the sum of cash over the states it passes (fp64)."""
        total, s = 0.0, 0
        for c in tokens:
            s = self.next(s, c)
            total += float(self.cash[s])
        return total


def _build(phrases):
    """{phrase: w} -> Automaton with exact fp64 cash / phi, nodes in breadth-first order, children sorted by token."""
    kids = [{}]                                # the trie, in insertion order
    own = [0.0]                                # w_p |p| of the phrase that ends here
    below = [0.0]                              # max w_p over the phrases that pass through this node and go on
    for p, w in phrases.items():
        s = 0
        for c in p:
            below[s] = max(below[s], w)
            if c not in kids[s]:
                kids[s][c] = len(kids)
                kids.append({})
                own.append(0.0)
                below.append(0.0)
            s = kids[s][c]
        own[s] = w * len(p)
    S = len(kids)
    if S > MAX_STATES:
        raise ValueError("ContextBias: %d automaton states exceed the limit of %d" % (S, MAX_STATES))
    # breadth-first renumbering: new id = position in the queue
    queue, new_of = [0], {0: 0}
    parent, tok, depth = [0], [-1], [0]
    child_lo = np.zeros(S + 1, dtype=np.int32)
    head = 0
    while head < len(queue):
        u = queue[head]
        child_lo[head] = len(queue)
        for c in sorted(kids[u]):
            v = kids[u][c]
            new_of[v] = len(queue)
            queue.append(v)
            parent.append(head)
            tok.append(c)
            depth.append(depth[head] + 1)
        head += 1
    child_lo[S] = S
    tok = np.array(tok, dtype=np.int32)
    depth = np.array(depth, dtype=np.int32)
    fail = np.zeros(S, dtype=np.int32)
    cash, phi = np.zeros(S), np.zeros(S)
    auto = Automaton(child_lo, tok, fail, depth, cash, phi)
    for i in range(1, S):                      # (breadth-first: the fail link of a shallower node is final)
        if depth[i] > 1:
            fail[i] = _fail_of(auto, int(fail[parent[i]]), int(tok[i]))
        cash[i] = own[queue[i]] + cash[fail[i]]
        phi[i] = float(depth[i]) * below[queue[i]]
    auto.cash, auto.phi = cash, phi
    return auto


def _fail_of(auto, f, c):
    """The fail link of the child by ``c`` of a node whose own fail link is ``f``."""
    while True:
        ch = auto.child(f, c)
        if ch >= 0:
            return ch
        if f == 0:
            return 0
        f = int(auto.fail[f])


def check_tables(child_lo, tok, fail, depth, cash, phi):
    """ValueError unless the arrays are an automaton the kernels may walk: child ranges inside [0, S] and non-decreasing, every
    fail link pointing to a strictly shallower node (the root's to itself), finite values."""
    S = int(tok.shape[0])
    if not 1 <= S <= MAX_STATES or child_lo.shape[0] != S + 1:
        raise ValueError("ContextBias: %d states (limit %d), child_lo of %d entries" % (S, MAX_STATES, child_lo.shape[0]))
    lo = child_lo.astype(np.int64)
    if lo[0] < 0 or lo[-1] > S or (np.diff(lo) < 0).any():
        raise ValueError("ContextBias: child ranges leave [0, %d] or decrease" % S)
    f = fail.astype(np.int64)
    if f[0] != 0 or (f < 0).any() or (f >= S).any() or (depth[f[1:]] >= depth[1:]).any():
        raise ValueError("ContextBias: a fail link does not point to a strictly shallower node")
    if int(depth.max()) > MAX_PHRASE:
        raise ValueError("ContextBias: a state deeper than %d" % MAX_PHRASE)
    if not (np.isfinite(cash).all() and np.isfinite(phi).all()):
        raise ValueError("ContextBias: a non-finite cash / phi value")


class ContextBias(object):
    """A set of phrases to boost: {tuple of 1..32 token ids >= 0: per-token weight w_p, finite and > 0}."""

    def __init__(self, phrases):
        self.phrases = {}
        for p, w in phrases.items():
            p, w = tuple(int(k) for k in p), float(w)
            if not 1 <= len(p) <= MAX_PHRASE:
                raise ValueError("ContextBias: a phrase has 1..%d tokens, got %d" % (MAX_PHRASE, len(p)))
            if any(k < 0 for k in p):
                raise ValueError("ContextBias: token ids are >= 0, got %r" % (p,))
            if not (math.isfinite(w) and w > 0.0):
                raise ValueError("ContextBias: a phrase weight must be finite and > 0, got %r" % w)
            self.phrases[p] = max(w, self.phrases.get(p, 0.0))      # a duplicate phrase keeps the larger weight
        self.automaton = _build(self.phrases)
        a = self.automaton
        check_tables(a.child_lo, a.tok, a.fail, a.depth, a.cash, a.phi)
        self.device = torch.device("cpu")
        self.tables = None

    @classmethod
    def from_phrases(cls, token_lists, weight=1.0, weights=None):
        """``token_lists``: the phrases as lists of token ids; ``weights``: one per-token weight per phrase (default: ``weight``
        for all).  ValueError: an empty phrase, one over 32 tokens, a negative id, a weight that is not finite and > 0, more
        than 65,536 automaton states."""
        token_lists = [list(p) for p in token_lists]
        if weights is None:
            weights = [weight] * len(token_lists)
        weights = list(weights)
        if len(weights) != len(token_lists):
            raise ValueError("ContextBias: %d weights for %d phrases" % (len(weights), len(token_lists)))
        merged = {}
        for p, w in zip(token_lists, weights):
            p, w = tuple(int(k) for k in p), float(w)
            if not (math.isfinite(w) and w > 0.0):
                raise ValueError("ContextBias: a phrase weight must be finite and > 0, got %r" % w)
            merged[p] = max(w, merged.get(p, 0.0))
        return cls(merged)

    def reward(self, tokens):
        """The definition, by brute force: sum of w_p |p| over every occurrence of every phrase in ``tokens`` (fp64)."""
        h = tuple(int(k) for k in tokens)
        total = 0.0
        for p, w in self.phrases.items():
            n = len(p)
            for i in range(len(h) - n + 1):
                if h[i:i + n] == p:
                    total += w * n
        return total

    def to(self, device):
        """-> the same phrases with ``tables`` (a DeviceAutomaton) on ``device``: what ``Decode(..., bias=...)`` takes."""
        out = ContextBias.__new__(ContextBias)
        out.__dict__.update(self.__dict__)
        out.device = torch.device(device)
        out.tables = DeviceAutomaton(self.automaton, device)
        return out


class DeviceAutomaton(object):
    """The automaton as the kernels read it.  ``host``: child_lo i32 [S + 1], tok i32, fail i32, cash f32, phi f32 [S] (and depth,
    which only the host uses); the same arrays as device tensors: child_lo, tok, fail, cash, phi."""

    def __init__(self, automaton, device):
        a = automaton
        with np.errstate(over="ignore"):
            cash, phi = a.cash.astype(np.float32), a.phi.astype(np.float32)
        check_tables(a.child_lo, a.tok, a.fail, a.depth, cash, phi)
        self.S = a.S
        self.host = dict(child_lo=a.child_lo.astype(np.int32), tok=a.tok.astype(np.int32), fail=a.fail.astype(np.int32), cash=cash,
                         phi=phi, depth=a.depth)
        self.device = torch.device(device)
        self.child_lo, self.tok, self.fail, self.cash, self.phi = (torch.from_numpy(self.host[k]).to(device)
                                                                   for k in ("child_lo", "tok", "fail", "cash", "phi"))

    def rounded_model(self):
        """The fp64 definition over the ROUNDED tables (what an fp64 reference of the kernels reads)."""
        h = self.host
        return Automaton(h["child_lo"], h["tok"], h["fail"], h["depth"], h["cash"].astype(np.float64), h["phi"].astype(np.float64))


def check_options(opt, bias, model, device, beam, joint):
    """-> (bias_weight, K of the head-less pre-beam route or None); ValueError on a bad combination (Decode's constructor)."""
    from . import ctc_decode
    bw = getattr(opt, "bias_weight", None)
    bw = 1.0 if bw is None else float(bw)
    if not bw >= 0.0 or not math.isfinite(bw):
        raise ValueError("Decode: bias_weight must be a finite number >= 0, got %r" % bw)
    if bias is None:
        return bw, None
    if bias.tables is None or not ctc_decode._same_device(bias.device, device):
        raise ValueError("Decode: the context bias lives on %s, the decoder on %s - pass bias.to(device)" % (bias.device, device))
    K = None
    if not joint and bw > 0.0:
        K = ctc_decode.pre_beam_width(opt, beam)
        if beam > 16 or K < beam or K > 64 or K > model.vocab_size:
            raise ValueError("Decode: a search with a context bias needs beam_size <= 16 and ctc_pre_beam in [beam_size, "
                             "min(64, vocabulary)], got beam_size %d, ctc_pre_beam %d" % (beam, K))
    return bw, K


class BiasSearch(object):
    """The biasing side of one search over B utterances x ``beam`` hypotheses: the automaton state of every hypothesis (device
    state of the captured step; -1 = frozen after EOS) and the two launches around the joint advance.  ``scale``: what
    st_bias_score multiplies Delta by before adding it to the pre-beam's ``lp`` - bias_weight / (1 - w), because
    st_beam_advance_joint weighs ``lp`` by (1 - w)."""

    def __init__(self, bias, B, beam, scale):
        self.bias, self.tables, self.B, self.beam, self.scale = bias, bias.tables, B, beam, float(scale)
        self.state = torch.zeros(B * beam, dtype=I32, device=bias.tables.device)

    def score(self, ids, lp, done, eos):
        nv.bias_score(self.tables, self.state, ids, done, eos, self.scale, lp=lp)

    def follow(self, order, tokens, done, eos):
        nv.bias_advance(self.tables, self.state, order, tokens, done, eos, self.beam)


@torch.no_grad()
def score_lists(bias, nbest, eos=Constants.EOS):
    """reward(h) of nbest[b][j] (label lists without EOS; None or a shorter row: missing) -> f32 [B, N] on the tables' device,
    -inf for a missing one: ONE st_bias_score_seq launch over h . EOS (the closing EOS revokes the provisional part), the
    positions summed in fp64 on the device."""
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
    dev = bias.tables.device
    out = torch.empty(B * N, L, dtype=F32, device=dev)
    nv.bias_score_seq(bias.tables, toks.to(dev), lens.to(dev), eos, out)
    total = out.double().sum(1)
    return torch.where(have.to(dev), total, torch.full_like(total, float("-inf"))).view(B, N).float()

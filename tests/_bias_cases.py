"""Shared cases of tests/test_bias_cpu.py and tests/test_bias_gpu.py: the small automaton with nested / prefix / repeated-token
phrases, the rows of a st_bias_score / st_bias_advance call, and the torch / NumPy formulation of one search step with a context
bias (pre-beam -> bias -> joint advance -> follow)."""
import math

import numpy as np
import torch

from st_amd.biasing import ContextBias
from tests import _emul_bias as emul

BOS, EOS = 2, 3
A, B_, C, D, E, F_, G = 4, 5, 6, 7, 8, 9, 10               # the 7 tokens of the small automaton
# nested (a b c d / b c), prefix (a b / a b c d), repeated tokens (a a a), a duplicate with another weight, overlapping tails
SEVEN = [([A, B_, C, D], 1.0), ([B_, C], 0.5), ([A, B_], 0.25), ([A, A, A], 2.0), ([C, D, E], 1.5), ([B_, C], 0.75), ([G], 0.5),
         ([D, E, F_, G, A], 0.125), ([E], 1.0)]


def seven():
    return ContextBias.from_phrases([p for p, _ in SEVEN], weights=[w for _, w in SEVEN])


def score_case(tables, Bn, beam, K, seed):
    """state i32 [n], cand i32 [n, K], done bool [B]: every automaton state appears, frozen rows (-1), one finished utterance,
    candidates over the 7 tokens, a stranger (20), EOS and -1."""
    rng = np.random.default_rng(seed)
    n = Bn * beam
    state = rng.integers(0, tables.S, n).astype(np.int32)
    state[:min(n, tables.S)] = np.arange(min(n, tables.S))
    pool = [A, B_, C, D, E, F_, G, 20, EOS, -1]
    cand = np.array([[pool[(i * K + j + int(rng.integers(3))) % len(pool)] for j in range(K)] for i in range(n)], dtype=np.int32)
    if n > 2:
        state[rng.choice(np.arange(1, n), size=max(1, n // 6), replace=False)] = -1
    done = np.zeros(Bn, dtype=bool)
    if Bn > 1:
        done[1] = True
    return state, cand, done


def advance_case(tables, Bn, beam, seed):
    """state, order, tokens, done: cycles (every parent overwritten), two children per parent, random parents with duplicates
    and self-overwrites, frozen parents, chosen EOS, one done utterance."""
    rng = np.random.default_rng(seed)
    n = Bn * beam
    state = rng.integers(0, tables.S, n).astype(np.int32)
    order = np.zeros(n, dtype=np.int64)
    for b in range(Bn):
        base = b * beam
        if b % 3 == 0:
            order[base:base + beam] = base + (np.arange(beam) + 1) % beam
        elif b % 3 == 1:
            order[base:base + beam] = base + np.arange(beam) // 2
        else:
            order[base:base + beam] = base + rng.integers(0, beam, beam)
    frozen = rng.random(n) < 0.25
    frozen[0] = n > 1 and beam > 1
    state[frozen] = -1
    tokens = rng.choice([A, B_, C, D, E, F_, G, 20], size=n).astype(np.int64)
    tokens[rng.random(n) < 0.15] = EOS
    if n > 1:
        tokens[n // 2] = EOS
    done = np.zeros(Bn, dtype=bool)
    if Bn > 1:
        done[Bn - 1] = True
    return state, order, tokens, done


def chain_reference(st, state, ids, lp, delta, tables, scale, w, beam, K, t):
    """One step of the torch side: the joint formulation (tests/test_joint_decode_gpu.py::_joint_torch) over lp + scale x the
    emulated increments.  -> (state dict after, automaton states after, the smallest gap at a selection boundary relative to its
    tolerance)."""
    from tests.test_joint_decode_gpu import _joint_torch
    Bn = st["scores"].shape[0]
    done = st["done"].numpy()
    raw = emul.score_rows(tables, state, ids.numpy(), EOS, done, beam)
    raw = np.where(np.isnan(raw), 0.0, raw)
    fused = lp.double() + torch.from_numpy(np.float64(np.float32(scale)) * raw.astype(np.float64))
    want = _joint_torch(st, ids, fused, delta.double(), w, beam, K, EOS, t)
    margin = float("inf")
    for b in range(Bn):
        if done[b]:
            continue
        rows = slice(b * beam, (b + 1) * beam)
        val = (st["scores"][b].double().unsqueeze(1) + (1 - w) * fused[rows] + (w * delta[rows].double() if w > 0 else 0.0)).reshape(-1)
        top = torch.sort(val, descending=True)[0][:beam + 1]
        for a, c in zip(top[:-1].tolist(), top[1:].tolist()):
            if math.isinf(a) or math.isinf(c):
                continue
            margin = min(margin, (a - c) / (1e-5 + 1e-6 * max(abs(a), abs(c))))
    state2 = emul.advance(tables, state, want["order"].numpy(), want["tokens"].numpy(), EOS, beam, want["done"].numpy())
    return want, state2, margin


def chain_bias(V, seed):
    """Phrases dense enough over [4, V) that five random steps meet them: every third token alone, 40 random phrases of 2-3."""
    rng = np.random.default_rng(seed)
    phrases = [[int(k)] for k in range(4, V, 3)] + [[int(k) for k in rng.integers(4, V, rng.integers(2, 4))] for _ in range(40)]
    weights = [float(rng.choice([0.25, 0.5, 1.0, 1.5])) for _ in phrases]
    return ContextBias.from_phrases(phrases, weights=weights)


def hypothesis_of(st, b, s, t):
    """The tokens of slot s of utterance b after step t, from the trellis (back / toks)."""
    out = []
    for step in range(t, -1, -1):
        out.append(int(st["toks"][step, b, s]))
        s = int(st["back"][step, b, s])
    return out[::-1]

"""-m "not gpu": the definition the CTC forced alignment (csrc/st_ctc_align.hip) is held to, and the host side around it.

The fp64 Viterbi of tests/_ctc_align_ref.py - score, path AND tie rule - is pinned by brute-force enumeration of every valid
alignment; then the exports, the binding's argument checks and, under the kernel emulations, the wiring of
st_amd.ctc_align.align_rows and transformer.Decode.align on a tiny model."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from st_amd import native
from tests import _ctc_align_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(lp, classes, T_in):
    """Every state sequence of the lattice: start in state 0 or 1, move by 0, +1 or (where l'(s) != l'(s-2)) +2, end in S-1 or
    S-2.  -> (best score, the best sequence that is lexicographically largest read from the last frame backwards) or None."""
    ext, skip = ref.extended(classes)
    S = len(ext)
    best = None
    for seq in itertools.product(range(S), repeat=T_in):
        if seq[0] > 1 or seq[-1] < S - 2:
            continue
        ok = True
        for a, b in zip(seq, seq[1:]):
            if not (b == a or b == a + 1 or (b == a + 2 and skip[b])):
                ok = False
                break
        if not ok:
            continue
        key = (sum(float(lp[t, ext[s]]) for t, s in enumerate(seq)), tuple(reversed(seq)))
        if best is None or key > best:
            best = key
    return None if best is None else (best[0], list(reversed(best[1])))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_reference_equals_enumeration_of_all_alignments(T):
    """Integer emissions in [-3, -1] (ties in almost every case; sums exact): score, path and the tie rule agree with the
    enumeration - labels with adjacent repeats, labels equal to class 0, tl 0 .. 3, infeasible lengths included."""
    rng = np.random.default_rng(100 + T)
    label_sets = [[], [1], [0], [1, 2], [1, 1], [0, 0], [2, 0], [0, 1], [1, 2, 1], [1, 1, 2], [2, 2, 2], [0, 1, 0], [1, 0, 0], [3, 1, 2]]
    ties = feasible = infeasible = 0
    for classes in label_sets:
        for rep in range(4):
            lp = rng.integers(-3, 0, size=(T + 1, 4)).astype(np.float64)          # (one frame past the length: never read)
            lp[T] = 1000.0
            want = _brute(lp, classes, T)
            path, spans, score, best = ref.align_one(lp, classes, T)
            if want is None:
                infeasible += 1
                assert score == -np.inf and (path == -1).all() and (spans == -1).all()
                continue
            feasible += 1
            assert score == want[0] == best, (classes, score, want)
            assert ref.states_of(path, T) == want[1], (classes, lp, path, want)
            assert path[T] == -1
            for j in range(len(classes)):
                frames = [t for t in range(T) if want[1][t] == 2 * j + 1]
                assert list(spans[j]) == [frames[0], frames[-1] + 1] and frames == list(range(frames[0], frames[-1] + 1))
            ext, _ = ref.extended(classes)
            n_best = sum(1 for seq in itertools.product(range(len(ext)), repeat=T)
                         if _valid(seq, classes) and sum(float(lp[t, ext[s]]) for t, s in enumerate(seq)) == want[0])
            ties += n_best > 1
    assert feasible > 10 and (T >= 3 or infeasible > 0) and (T < 3 or ties > 5), (feasible, infeasible, ties)


def _valid(seq, classes):
    ext, skip = ref.extended(classes)
    S = len(ext)
    if seq[0] > 1 or seq[-1] < S - 2:
        return False
    return all(b == a or b == a + 1 or (b == a + 2 and skip[b]) for a, b in zip(seq, seq[1:]))


def test_reference_tie_rule_by_hand():
    """All-equal emissions: every alignment is optimal.  Stay first, then s-1, then s-2, and the last blank wins the end: the
    labels are pushed to the EARLIEST frames and the tail is blank."""
    lp = np.zeros((5, 3))
    path, spans, score, _ = ref.align_one(lp, [1, 2], 5)
    assert path.tolist() == [0, 1, -1, -1, -1] and spans.tolist() == [[0, 1], [1, 2]] and score == 0.0
    path, spans, _, _ = ref.align_one(lp, [1, 1], 5)                  # the repeat forces one blank between
    assert path.tolist() == [0, -1, 1, -1, -1] and spans.tolist() == [[0, 1], [2, 3]]
    path, _, _, _ = ref.align_one(lp, [1, 1], 3)                      # unique
    assert path.tolist() == [0, -1, 1, -1, -1]                         # (frames past the length: -1)
    assert ref.align_one(lp, [1, 1], 2)[2] == -np.inf and ref.align_one(lp, [1], 0)[2] == -np.inf
    path, _, score, _ = ref.align_one(lp, [], 4)
    assert path.tolist() == [-1, -1, -1, -1, -1] and score == 0.0


def test_new_exports_in_header_binding_and_library():
    names = ["st_ctc_align_ws_kib", "st_ctc_align"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "st_hip.h")).read(), flags=re.S)
    assert native.ABI_VERSION == int(re.search(r"#define\s+ST_ABI_VERSION\s+(\d+)", text).group(1)) == native.abi_fingerprint(text)
    decl = dict(re.findall(r"\bint\s+(st_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S))
    lib = native.load()
    assert lib.st_version() == native.ABI_VERSION
    syms = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT\s+(st_[a-z0-9_]+)", syms))
    for n in names:
        assert n in decl and n in native.SIGNATURES and n in exported, n
        assert decl[n].count(",") + 1 == len(native.SIGNATURES[n]), n
    # `long long ws_bytes` sits between the workspace pointer and the three outputs
    params = [p.strip() for p in decl["st_ctc_align"].split(",")]
    assert params[10] == "long long ws_bytes" and params[9] == "void* ws" and len(params) == 14
    import ctypes
    assert native.SIGNATURES["st_ctc_align"][10] is ctypes.c_longlong and native.SIGNATURES["st_ctc_align"][9] is ctypes.c_void_p
    assert "st_ctc_align.hip" in __import__("st_amd.build", fromlist=["SOURCES"]).SOURCES
    # the host-only workspace query: nothing while every frame count fits LDS (2,048 frames up to 127 labels, 1,024 above), else
    # one back-pointer word (1 byte; 2 bytes above 127 labels) per lane, frame and utterance
    raw = lib._cdll.st_ctc_align_ws_kib
    assert raw(32, 750, 50) == 0 and raw(32, 2048, 127) == 0 and raw(32, 1024, 255) == 0
    assert raw(32, 2049, 50) == (32 * 2049 * 64 + 1023) // 1024 and raw(3, 2048, 255) == 3 * 2048 * 128 // 1024
    assert raw(8, 2048, 256) == -1 and raw(-1, 10, 3) == -1
    assert native.ctc_align_ws_bytes(3, 2048, 255) == 3 * 2048 * 128
    with pytest.raises(ValueError):
        native.ctc_align_ws_bytes(4, 100, 256)


def test_binding_argument_checks_raise_before_any_launch():
    B, T, C, L = 3, 9, 5, 4
    ok = dict(lp=torch.zeros(B, T, C), classes=torch.zeros(B, L, dtype=torch.int64), in_len=torch.full((B,), T, dtype=torch.int32),
              tgt_len=torch.full((B,), L, dtype=torch.int32), ws=torch.zeros(0, dtype=torch.uint8),
              path=torch.zeros(B, T, dtype=torch.int32), spans=torch.zeros(B, L, 2, dtype=torch.int32), score=torch.zeros(B))
    bad = [dict(lp=torch.zeros(B, T, C, dtype=torch.float64)), dict(lp=torch.zeros(B, T, 2 * C)[:, :, ::2]), dict(lp=torch.zeros(B, T, 1)),
           dict(lp=torch.zeros(B * T, C)), dict(classes=torch.zeros(B, L, dtype=torch.int32)),
           dict(classes=torch.zeros(B, 256, dtype=torch.int64), spans=torch.zeros(B, 256, 2, dtype=torch.int32)),
           dict(classes=torch.zeros(B + 1, L, dtype=torch.int64)), dict(in_len=torch.full((B,), T, dtype=torch.int64)),
           dict(tgt_len=torch.full((B + 1,), L, dtype=torch.int32)), dict(path=torch.zeros(B, T, dtype=torch.int64)),
           dict(path=torch.zeros(B, T + 1, dtype=torch.int32)), dict(path=torch.zeros(T, B, dtype=torch.int32).t()),
           dict(spans=torch.zeros(B, L, dtype=torch.int32)), dict(spans=torch.zeros(B, 2, L, dtype=torch.int32).transpose(1, 2)),
           dict(score=torch.zeros(B, dtype=torch.float64)), dict(score=torch.zeros(B + 1)),
           dict(ws=torch.zeros(16, dtype=torch.float32)), dict(ws=torch.zeros(4, 4, dtype=torch.uint8))]
    for change in bad:
        with pytest.raises(ValueError):
            native.ctc_align(**{**ok, **change})
    # a workspace that is too short for a shape that needs one (2,048 frames, 255 labels: 128 bytes per frame and utterance)
    T2, L2 = 2048, 255
    big = dict(lp=torch.zeros(1, T2, 4), classes=torch.zeros(1, L2, dtype=torch.int64), in_len=torch.full((1,), T2, dtype=torch.int32),
               tgt_len=torch.full((1,), L2, dtype=torch.int32), ws=torch.zeros(T2 * 128 - 1, dtype=torch.uint8),
               path=torch.zeros(1, T2, dtype=torch.int32), spans=torch.zeros(1, L2, 2, dtype=torch.int32), score=torch.zeros(1))
    with pytest.raises(ValueError, match="ws holds"):
        native.ctc_align(**big)
    # well-formed arguments that are not on the GPU: refused as everywhere in the binding (no CPU fallback)
    with pytest.raises(RuntimeError):
        native.ctc_align(**ok)
    with pytest.raises(RuntimeError):
        native.ctc_align(**dict(big, ws=torch.zeros(T2 * 128, dtype=torch.uint8)))


def _small_model():
    import oracle as orc
    import transformer.Models as M
    import transformer.Utils as U
    p = orc.xavier_init_(orc.make_params(80, 30, 128, 256, 1, 1, 100, 20, dtype=torch.float64), seed=1)
    cfg = U.AttrDict(dict(feature_dim=80, max_inputs_length=100, max_target_length=20, num_enc_layer=1, num_dec_layer=1, n_heads=4,
                          d_k=32, d_v=32, d_model=128, d_inner_hid=256, dropout=0.0, vocab_size=30))
    m = M.Transformer(cfg)
    m.load_state_dict({k: v.float() for k, v in p.items()})
    return m.eval()


def _batch():
    g = torch.Generator().manual_seed(5)
    in_len = torch.tensor([30, 21, 12, 4])
    x = torch.randn(4, 30, 80, generator=g)
    for b, n in enumerate(in_len.tolist()):
        x[b, n:] = 0
    return x, in_len


def _decoder(model, head):
    from transformer.Decode import Decode
    from transformer.Utils import AttrDict
    return Decode(AttrDict(dict(beam_size=2, n_best=1, max_steps=10, use_graph=False)), "cpu", model=model, ctc_head=head)


def test_align_rows_composition_under_the_emulations():
    """align_rows on a tiny model: the plan's classes / lengths reach the launch, path / spans / score are what the reference
    says of the plan's lp, token_logp + blank_logp decompose the score, and an utterance that cannot be aligned is all -1."""
    from st_amd import ctc_align
    from tests._emul import emulated_kernels
    from tests._emul_ctc_align import emulated_ctc_align
    from transformer.Loss import CTCAttentionLoss
    torch.manual_seed(0)
    model, head = _small_model(), CTCAttentionLoss(128, 30).eval()
    x, in_len = _batch()
    labels = torch.tensor([[5, 6, 6, 7, 0], [8, 0, 0, 0, 0], [9, 9, 9, 9, 9], [4, 5, 6, 7, 8]])
    lengths = torch.tensor([5, 1, 0, 5])                       # (utterance 2: no labels; utterance 3: 4 rows for 5 labels)
    with emulated_kernels(), emulated_ctc_align():
        enc, in_rows = model.encoder.forward_rows(x, in_len)
        al = ctc_align.align_rows(head, enc, in_rows, labels, lengths)
    plan = al.plan
    assert plan.classes[0].tolist() == [1, 2, 2, 4, 0]          # equal labels share a class; a label equal to the blank id is class 0
    path, spans, score, _ = ref.align_batch(plan.lp.numpy(), plan.classes.numpy(), in_len.tolist(), lengths.tolist())
    assert np.array_equal(al.path.numpy(), path) and np.array_equal(al.spans.numpy(), spans) and np.array_equal(al.score.numpy(), score)
    assert al.path.dtype == torch.int32 and al.spans.shape == (4, 5, 2) and al.token_logp.shape == (4, 5)
    assert score[3] == -np.inf and (path[3] == -1).all() and (spans[3] == -1).all() and np.isfinite(score[:3]).all()
    assert (al.token_logp[3] == float("-inf")).all() and (al.path[2] == -1).all() and (al.token_logp[2] == 0).all()
    lp = plan.lp.double().numpy()
    for b in range(3):
        for j in range(int(lengths[b])):
            s, e = spans[b, j]
            want = sum(lp[b, t, int(plan.classes[b, j])] for t in range(s, e))
            assert abs(float(al.token_logp[b, j]) - want) <= 1e-5 * max(1.0, abs(want))
        total = float(al.token_logp[b].double().sum() + al.blank_logp[b].double())
        assert abs(total - float(score[b])) <= 1e-5 * abs(float(score[b]))


def test_decode_align_composition_and_argument_checks():
    """Decode.align under the emulations: EOS stripping, the tokens of the items, ordered contiguous spans inside the utterance,
    ([], -inf) for an utterance without an alignment, and the ValueErrors."""
    from tests._emul import emulated_kernels
    from tests._emul_ctc_align import emulated_ctc_align
    from transformer.Loss import CTCAttentionLoss
    import transformer.Constants as Constants
    torch.manual_seed(0)
    model, head = _small_model(), CTCAttentionLoss(128, 30).eval()
    x, in_len = _batch()
    EOS, BOS = Constants.EOS, Constants.BOS
    hyps = [[5, 6, 6, 7, EOS], [8], [EOS], [4, 5, 6, 7, 8, EOS]]
    dec = _decoder(model, head)
    with emulated_kernels(), emulated_ctc_align():
        out = dec.align((x, in_len), hyps)
        out_eos = dec.align((x, in_len), hyps, strip_eos=False)
    assert len(out) == 4
    for b, (items, score) in enumerate(out[:3]):
        want = hyps[b][:-1] if hyps[b][-1] == EOS else hyps[b]
        assert [it[0] for it in items] == want and np.isfinite(score)
        end = 0
        for tok, s, e, logp in items:
            assert end <= s < e <= int(in_len[b]) and logp <= 0.0 and isinstance(s, int)
            end = e
    assert out[2] == ([], out[2][1]) and np.isfinite(out[2][1])            # no labels: the all-blank path
    assert out[3] == ([], float("-inf"))                                     # 4 rows cannot spell 5 labels
    assert [it[0] for it in out_eos[0][0]] == hyps[0] and [it[0] for it in out_eos[2][0]] == [EOS]
    assert out_eos[0][1] != out[0][1]
    with emulated_kernels(), emulated_ctc_align():
        for bad in ([[BOS, 5], [8], [], []], [[5, 30], [8], [], []], [[5, -1], [8], [], []], [[5] * 256, [8], [], []], [[5], [8], []]):
            with pytest.raises(ValueError):
                dec.align((x, in_len), bad)
        with pytest.raises(ValueError):
            _decoder(model, None).align((x, in_len), hyps)

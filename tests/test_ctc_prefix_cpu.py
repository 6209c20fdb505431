"""-m "not gpu": the fp64 restatement of the CTC prefix scorer (tests/_ctc_ref.py - what st_ctc_prefix_score is held to in
tests/test_joint_decode_gpu.py) pinned by brute-force path enumeration and by torch's ctc_loss, and the argument checks of the
joint CTC / attention decode options."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import _ctc_ref as ref

BLANK = 0


def _collapse(path):
    out, prev = [], None
    for k in path:
        if k != prev and k != BLANK:
            out.append(k)
        prev = k
    return out


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_prefix_scores_equal_path_enumeration(T):
    """Two labels plus blank (and an EOS id outside the path alphabet): psi(g) of every prefix up to length 3 equals the summed
    probability of all 3^T paths whose collapse starts with g; psi(g.EOS) the probability of those that collapse to g exactly."""
    rng = np.random.default_rng(T)
    V, eos = 4, 3
    z = rng.normal(size=(T, 3)) * 2.0
    x = np.full((T, V), -np.inf)
    x[:, :3] = z - np.log(np.exp(z).sum(1, keepdims=True))          # no probability on EOS in any frame
    starts, exact = {}, {}
    for path in itertools.product(range(3), repeat=T):
        p = math.exp(sum(x[t, k] for t, k in enumerate(path)))
        col = tuple(_collapse(path))
        exact[col] = exact.get(col, 0.0) + p
        for n in range(len(col) + 1):
            starts[col[:n]] = starts.get(col[:n], 0.0) + p
    checked = 0
    for n in range(4):
        for g in itertools.product((1, 2), repeat=n):
            psis, end = ref.prefix_scores(x, list(g), BLANK, eos)
            want = starts.get(g, 0.0)
            got = math.exp(psis[-1])
            assert abs(got - want) <= 1e-12 + 1e-9 * want, (g, got, want)
            want_end = exact.get(g, 0.0)
            assert abs(math.exp(end) - want_end) <= 1e-12 + 1e-9 * want_end, (g, math.exp(end), want_end)
            checked += 1
    assert checked == 15
    # blank as a label: -inf
    assert ref.extend(x, ref.empty_state(x, BLANK), BLANK, BLANK, eos)[0] == -np.inf


@pytest.mark.parametrize("T,L,seed", [(7, 3, 0), (50, 12, 1), (128, 30, 2), (400, 60, 3), (1000, 80, 4), (1000, 25, 5)])
def test_telescoped_increments_equal_ctc_loss(T, L, seed):
    """The increments Delta(c | g) along a label sequence plus EOS sum to log p_ctc(y | x) = -ctc_loss(y) (fp64, torch's
    implementation); label sequences with repeats (c == last(g): the blank-separated branch of the recursion)."""
    g = torch.Generator().manual_seed(seed)
    V, eos = 12, 11
    logits = torch.randn(T, V, generator=g, dtype=torch.float64) * 2.0
    lp = torch.log_softmax(logits, -1)
    labels = torch.randint(1, eos, (L,), generator=g)
    labels[1::4] = labels[0::4][:labels[1::4].numel()]           # immediate repeats
    inc = ref.increments(lp.numpy(), labels.tolist(), BLANK, eos)
    nll = torch.nn.functional.ctc_loss(lp.unsqueeze(1), labels.unsqueeze(0), torch.tensor([T]), torch.tensor([L]), blank=BLANK,
                                       reduction="none")
    assert math.isfinite(sum(inc))
    assert abs(sum(inc) + float(nll[0])) <= 1e-8 * max(1.0, float(nll[0])), (sum(inc), -float(nll[0]))


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


def test_joint_decode_argument_checks():
    """Decode(opt, device, model, ctc_head): ValueError for a weight outside [0, 1), a pre-beam outside [beam, 64], a head of
    another width or on another device; no head or weight 0 keeps the attention-only search."""
    from transformer.Decode import Decode
    from transformer.Loss import CTCAttentionLoss
    from transformer.Utils import AttrDict
    model = _small_model()
    head = CTCAttentionLoss(128, 30)

    def opt(**kw):
        return AttrDict(dict(beam_size=4, n_best=1, max_steps=10, use_graph=False, **kw))

    for bad in (opt(ctc_weight=1.0), opt(ctc_weight=-0.1), opt(ctc_weight=0.3, ctc_pre_beam=3), opt(ctc_weight=0.3, ctc_pre_beam=65)):
        with pytest.raises(ValueError):
            Decode(bad, "cpu", model=model, ctc_head=head)
    with pytest.raises(ValueError):
        Decode(opt(ctc_weight=0.3), "cpu", model=model, ctc_head=CTCAttentionLoss(64, 30))
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            Decode(opt(ctc_weight=0.3), "cpu", model=model, ctc_head=CTCAttentionLoss(128, 30).cuda())
    else:
        with pytest.raises(ValueError):
            Decode(opt(ctc_weight=0.3), "cuda", model=model, ctc_head=head)
    d = Decode(opt(ctc_weight=0.3), "cpu", model=model, ctc_head=head)
    assert d.ctc_weight == 0.3 and d.ctc_pre_beam == 6
    assert Decode(opt(ctc_weight=0.3, ctc_pre_beam=4), "cpu", model=model, ctc_head=head).ctc_pre_beam == 4
    for off in (Decode(opt(), "cpu", model=model, ctc_head=head), Decode(opt(ctc_weight=0.3), "cpu", model=model)):
        assert off.ctc_weight == 0.0 and off.ctc_pre_beam is None

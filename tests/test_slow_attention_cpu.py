"""The checks of tests/test_slow_attention_gpu.py can see the defects they are there for.  Everything here runs the EMULATION
(tests/_emul.py; no kernel involved) through the very code the GPU tests run (tests/_slow_attn.py): undamaged it passes - which
also checks the fp64 references of tests/_attn_ref.py against em.attn_dense_* / em.attn_probs within the bounds, and against the
reference-import goldens -; with one defect injected into its output, or into the mask / keep set it works from, the checks fail
and name the place.  The first four defects pass the whole-tensor metric of test_general_attention_* at its fixture shapes: the
gap these tests close.  Last: DenseMhaFn refuses, before any launch, a forward whose backward the LDS limits would refuse."""
import os

import numpy as np
import pytest
import torch

from tests import _attn_ref as ref
from tests import _emul as em
from tests import _slow_attn as sa
from tests import test_composition_cpu as comp
from tests._emul import emulated_kernels
from tests._local import check_local, rel

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CPU = sa.CPU


def _fails(fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    for n in needles:
        assert n in str(e.value), "%r not in: %s" % (n, e.value)
    return str(e.value)


def _view(o, nm):
    return o.g[nm].view


# ---- undamaged: the references agree with the goldens and with the emulation ---------------------------------------------------------
@pytest.mark.parametrize("name", ["mha_dense_mask", "mha_dense_mask_kv"])
def test_reference_probabilities_equal_the_goldens(name, golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    H = int(fx["n_head"])
    q, k = torch.from_numpy(fx["q"]).double(), torch.from_numpy(fx["k"]).double()
    B, Lq, d = q.shape
    Lk = k.shape[1]
    W = {n[2:]: torch.from_numpy(v).double() for n, v in fx.items() if n.startswith("w/")}
    Q = (q @ W["linear_q.weight"].t() + W["linear_q.bias"]).view(B * Lq, d)
    K = (k @ W["linear_k.weight"].t() + W["linear_k.bias"]).view(B * Lk, d)
    mask = torch.from_numpy(fx["mask"])
    P = ref.dense_attention(Q, K, K, mask, None, B, H, Lq, Lk, (d // H) ** -0.5)[2]
    gold = torch.from_numpy(fx["f64/attn"])
    assert gold.shape == P.shape
    assert rel(P, gold) < 1e-6
    if Lq == Lk:        # the same map through attention_probs is a different function: only an unmasked problem compares
        return
    P2 = ref.attention_probs(Q, K, [Lq] * B, [Lk] * B, ([b * Lq for b in range(B)], [b * Lk for b in range(B)]), H, Lq, Lk, False,
                             (d // H) ** -0.5)
    P0 = ref.dense_attention(Q, K, K, None, None, B, H, Lq, Lk, (d // H) ** -0.5)[2]
    assert rel(P2, P0) < 1e-12


DENSE = sa.dense_cases()


@pytest.mark.parametrize("part", range(4))
def test_emulation_passes_every_dense_case(part):
    for i, kw in DENSE[part::4]:
        sa.run(sa.build(**kw), CPU, what=i)


def test_emulation_passes_the_lds_limit_cases():
    for name, kw, _, _ in sa.lds_cases():
        sa.run(sa.build(**kw), CPU, what=name, backward=kw.get("backward", True))


def test_emulation_passes_every_probs_case():
    for kw in sa.probs_cases():
        sa.run_probs(sa.build_probs(**kw), CPU)


def test_bf16_rounding_alone_stays_well_inside_the_bound():
    """The room between 'correct' and L_BF16: the emulation's once-rounded outputs against the unrounded fp64 reference."""
    from tests._local import local_figures
    worst = 0.0
    for i, kw in DENSE[::9]:
        c = sa.build(**kw)
        o = sa.launch(c, CPU)
        for nm in ("O", "dQ", "dK", "dV"):
            worst = max([worst] + [float(r.max()) for _, r in local_figures(_view(o, nm), c.ref[nm])])
    print("worst row / column ratio of a once-rounded bf16 output: %.3e" % worst)
    assert worst < 4e-3


# ---- injected defects ------------------------------------------------------------------------------------------------------------------
def _with_mask(c, m):
    """What the kernels compute when they see mask m instead of the case's."""
    return sa.launch(sa.variant(c, mask=m.to(torch.uint8)), CPU)


def _base_mask(c):
    return torch.zeros(c.B, c.Lq, c.Lk, dtype=torch.uint8) if c.mask is None else c.mask.clone()


def test_keys_from_256_on_ignored():
    c = sa.build(2, 2, 64, 7, 300, gseed=80)
    sa.run(c, CPU)
    m = _base_mask(c)
    m[:, :, 256:] = 1
    o = _with_mask(c, m)
    _fails(lambda: sa.verify(c, o), " O:")
    c = sa.build(2, 2, 64, 7, 600, needle=True, gseed=80)          # the needle at key 256: a whole wrong row
    m = _base_mask(c)
    m[:, :, 256:] = 1
    msg = _fails(lambda: sa.verify(c, _with_mask(c, m)), " O:")
    assert "rel-L2" in msg or "worst row" in msg


def test_the_last_key_ignored():
    for kw in (dict(Lk=257), dict(Lk=600), dict(Lk=65, B=3, H=3, dk=32, Lq=5)):
        c = sa.build(**dict(dict(B=2, H=2, dk=64, Lq=7, needle=True, gseed=81), **kw))
        sa.run(c, CPU)
        m = _base_mask(c)
        m[:, :, c.Lk - 1] = 1
        o = _with_mask(c, m)
        _fails(lambda: sa.verify(c, o), " O:")
        o.g["O"].view.copy_(sa.launch(c, CPU).g["O"].view)       # O repaired: the next output tells
        _fails(lambda: sa.verify(c, o), " P:")
    c = sa.build(2, 2, 64, 7, 257, gseed=81)                      # without a needle: a 1 / Lk perturbation, still seen row by row
    m = _base_mask(c)
    m[:, :, 256] = 1
    _fails(lambda: sa.verify(c, _with_mask(c, m)), " O:")


def test_queries_from_256_on_ignored_by_the_key_side():
    c = sa.build(2, 2, 64, 300, 9, gseed=82)
    o = sa.run(c, CPU)
    m = _base_mask(c)
    m[:, 256:, :] = 1
    bad = _with_mask(c, m)
    for nm in ("dK", "dV"):
        o2 = sa.launch(c, CPU)
        _view(o2, nm).copy_(_view(bad, nm))
        _fails(lambda: sa.verify(c, o2), " %s:" % nm)


def test_columns_64_to_127_of_a_128_wide_head_zero():
    c = sa.build(2, 1, 128, 7, 300, gseed=83)
    for nm in ("O", "dQ", "dK", "dV"):
        o = sa.launch(c, CPU)
        _view(o, nm)[:, 64:128] = 0
        _fails(lambda: sa.verify(c, o), " %s:" % nm)
        _fails(lambda: check_local(_view(o, nm), c.ref[nm], sa.L_BF16, nm), "64 of 128 columns fail")
    c = sa.build(2, 3, 96, 300, 9, gseed=83)                      # the partial second pass: columns 64 .. 95 of head 1
    o = sa.launch(c, CPU)
    _view(o, "dK")[:, 96 + 64:96 + 96] = 0
    _fails(lambda: sa.verify(c, o), " dK:")
    _fails(lambda: check_local(_view(o, "dK"), c.ref["dK"], sa.L_BF16, "dK"), "32 of 288 columns fail")


class _flipped_keep:
    """em.keep_qk with the decision of one (bh, q, k) flipped, while the emulation runs."""

    def __init__(self, bh, q, k):
        self.at, self.orig = (bh, q, k), em.keep_qk

    def __enter__(self):
        def keep_qk(d, bh, nq, nk):
            m = self.orig(d, bh, nq, nk)
            if bh == self.at[0]:
                m = m.clone()
                m[self.at[1], self.at[2]] ^= True
            return m
        em.keep_qk = keep_qk

    def __exit__(self, *a):
        em.keep_qk = self.orig


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_one_keep_decision_flipped_at_eight_keys(which):
    """One disagreeing pair moves its row by far more than the bound, in whichever kernel it happens."""
    c = sa.build(2, 3, 16, 5, 8, p=0.5, gseed=50)
    good = sa.run(c, CPU)
    with _flipped_keep(4, 3, 5):
        bad = sa.launch(c, CPU)
    if which == "fwd":                                            # only the forward disagrees
        for nm in ("delta", "dQ", "dK", "dV"):
            _view(bad, nm).copy_(_view(good, nm))
        _fails(lambda: sa.verify(c, bad), " O:")
    else:                                                         # only the backward does
        _view(bad, "O").copy_(_view(good, "O"))
        msg = _fails(lambda: sa.verify(c, bad))
        assert " dQ:" in msg or " dK:" in msg or " dV:" in msg or " delta:" in msg


def test_one_keep_decision_flipped_in_the_read_out():
    c = sa.build_readout(2, 3, 64, 9, 300, 0.5)
    sa.assert_keep_equal(sa.read_keep_fwd(c, CPU), c.keep, "forward")
    with _flipped_keep(3, 6, 257):
        got = sa.read_keep_fwd(c, CPU)
    _fails(lambda: sa.assert_keep_equal(got, c.keep, "forward"), "1 of %d pairs" % c.keep.numel(), "(bh, q, k) = (3, 6, 257)")
    c = sa.build_readout(2, 3, 64, 300, 9, 0.1)
    sa.assert_keep_equal(sa.read_keep_bwd(c, CPU), c.keep, "key side")
    with _flipped_keep(5, 299, 8):
        got = sa.read_keep_bwd(c, CPU)
    _fails(lambda: sa.assert_keep_equal(got, c.keep, "key side"), "1 of %d pairs" % c.keep.numel(), "(bh, q, k) = (5, 299, 8)")


def test_a_dead_row_given_a_uniform_distribution():
    c = sa.build(2, 2, 64, 7, 300, mask="dead", gseed=84)
    b, q = 1, 4
    assert bool(c.dead_q[b, q])
    o = sa.run(c, CPU)
    V = c.V.float().view(c.B, c.Lk, c.H, c.dk)
    _view(o, "P")[b, :, q, :] = 1.0 / c.Lk
    _fails(lambda: sa.verify(c, o), " P: masked entry not exactly zero", "dead row: True")
    o = sa.launch(c, CPU)
    _view(o, "O")[b * c.Lq + q] = V[b].mean(0).reshape(-1).to(BF16)
    _fails(lambda: sa.verify(c, o), " O: dead row", "row %d" % (b * c.Lq + q))
    o = sa.launch(c, CPU)
    _view(o, "lse").view(c.H, -1)[:, b * c.Lq + q] = 3.0
    _fails(lambda: sa.verify(c, o), "lse: dead row without lse = +inf")
    o = sa.launch(c, CPU)
    kd = int(torch.nonzero(c.dead_k[0])[0])
    _view(o, "dV")[kd] = 1e-3
    _fails(lambda: sa.verify(c, o), " dV: dead key", "row %d" % kd)


def test_probabilities_returned_after_dropout():
    c = sa.build(2, 3, 32, 20, 300, mask="dead", p=0.5, gseed=70)
    o = sa.run(c, CPU)
    plain = sa.launch(sa.variant(c, p=0.0), CPU, backward=False)
    sa.assert_same_bits(_view(o, "P"), _view(plain, "P"), "P")
    _view(o, "P").mul_((c.keep.view(c.B, c.H, c.Lq, c.Lk) * c.keep_scale).float())
    _fails(lambda: sa.assert_same_bits(_view(o, "P"), _view(plain, "P"), "P with dropout"), "not bit-identical")
    _fails(lambda: sa.verify(c, o), " P:")


def test_head_and_utterance_swapped_in_the_block_index():
    """H = 3, B = 2: slot n = b H + h taken apart as (b, h) = (n % B, n / B).  With B = H the swap is a transposition that the
    same check sees as well; with H and B powers of two and equal lengths nothing distinguishes the decompositions less."""
    c = sa.build(2, 3, 32, 20, 70, mask="rand30", gseed=85)
    for nm, L in (("O", c.Lq), ("dQ", c.Lq), ("dK", c.Lk), ("dV", c.Lk)):
        o = sa.launch(c, CPU)
        good = _view(o, nm).clone().view(c.B, L, c.H, c.dk)
        bad = good.clone()
        for n in range(c.B * c.H):
            bad[n // c.H, :, n % c.H] = good[n % c.B, :, n // c.B]
        _view(o, nm).copy_(bad.view(c.B * L, c.d))
        _fails(lambda: sa.verify(c, o), " %s:" % nm)
    o = sa.launch(c, CPU)
    good = _view(o, "lse").clone().view(c.H, c.B, c.Lq)
    bad = good.clone()
    for n in range(c.B * c.H):
        bad[n % c.H, n // c.H] = good[n // c.B, n % c.B]
    _view(o, "lse").copy_(bad.view(-1))
    _fails(lambda: sa.verify(c, o), " lse")


def test_attn_probs_defects():
    c = sa.build_probs(2, 2, 64, 600, False, True, False)

    def past_the_diagonal(P):
        P[0, 1, 300, 301] = 1e-9
    _fails(lambda: sa.run_probs(c, CPU, tamper=past_the_diagonal), "not exactly zero", "[0, 1, 300, 301]")

    def keys_from_256_on(P):
        P[..., 256:] = 0
        P.div_(P.sum(-1, keepdim=True).clamp_min(1e-30))
    _fails(lambda: sa.run_probs(c, CPU, tamper=keys_from_256_on), "attn_probs")
    c = sa.build_probs(3, 3, 32, 257, True, False, True)

    def last_key(P):
        P[0, :, :, 256] = 0
    _fails(lambda: sa.run_probs(c, CPU, tamper=last_key), "attn_probs")


# ---- the gap: the first four defects pass the old whole-tensor metric at the old fixture shapes ------------------------------------------
@pytest.mark.parametrize("defect", ["keys_from_256", "last_key", "queries_from_256", "columns_64_127"])
def test_old_metric_at_the_old_fixture_shapes_against_the_defect(defect, golden_dir):
    """run_general_attention (Lq = Lk = 9 and Lq = 11, Lk = 23, d_k = 32, one relative L2 norm per tensor after a projection and a
    LayerNorm) with the defect in the dense kernels' emulation.  Three of the four pass it untouched: there are no 256 keys or
    queries and no column 64 to lose.  The fourth does NOT: one key of 9 ignored moves the module's output by 0.29 of its norm
    against the 2e-2 it is held to - the old fixtures do see a last key that is dropped at every length; what they cannot see is a
    last key dropped only once the keys pass the 256-key stride (Lk = 257: test_the_last_key_ignored), which at 9 and 23 keys is
    the first case over again."""
    from st_amd import native as nv
    fwd, bwd = em.attn_dense_fwd, em.attn_dense_bwd

    def defective(mask, B, Lq, Lk):
        m = torch.zeros(B, Lq, Lk, dtype=torch.uint8) if mask is None else mask.clone()
        if defect == "keys_from_256":
            m[:, :, 256:] = 1
        elif defect == "last_key":
            m[:, :, Lk - 1] = 1
        return m

    def fwd_d(Q, K, V, mask, O, lse, B, H, Lq, Lk, scale, **kw):
        P = fwd(Q, K, V, defective(mask, B, Lq, Lk), O, lse, B, H, Lq, Lk, scale, **kw)
        if defect == "columns_64_127":
            O.view(B * Lq, H, -1)[:, :, 64:128] = 0
        return P

    def bwd_d(Q, K, V, mask, dO, lse, delta, dQ, dK, dV, B, H, Lq, Lk, scale, **kw):
        bwd(Q, K, V, defective(mask, B, Lq, Lk), dO, lse, delta, dQ, dK, dV, B, H, Lq, Lk, scale, **kw)
        if defect == "queries_from_256":
            m = defective(mask, B, Lq, Lk)
            m[:, 256:, :] = 1
            bwd(Q, K, V, m, dO, lse, delta.clone(), dQ.clone(), dK, dV, B, H, Lq, Lk, scale, **kw)
        if defect == "columns_64_127":
            for t in (dQ, dK, dV):
                t.view(t.shape[0], H, -1)[:, :, 64:128] = 0

    with emulated_kernels():
        nv.attn_dense_fwd, nv.attn_dense_bwd = torch.no_grad()(fwd_d), torch.no_grad()(bwd_d)
        if defect == "last_key":
            with pytest.raises(AssertionError, match="mha_dense_mask"):
                comp.run_general_attention(golden_dir, "cpu")
        else:
            comp.run_general_attention(golden_dir, "cpu")


# ---- the module boundary ---------------------------------------------------------------------------------------------------------------
def test_module_training_dropout_through_the_dense_path_composition():
    with emulated_kernels():
        sa.run_module_dropout("cpu")


def _mha_call(Lq, Lk, grad, calls=None):
    import transformer.Attention as A
    calls = [] if calls is None else calls
    with emulated_kernels():
        from st_amd import native as nv
        for n in ("gemm", "attn_dense_fwd"):
            setattr(nv, n, (lambda f, n=n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(nv, n)))
        mha = A.MultiHeadAttention(4, 128, 32, 32).eval()
        q, k, v = torch.zeros(1, Lq, 128), torch.zeros(1, Lk, 128), torch.zeros(1, Lk, 128)
        if grad:
            out, _ = mha(q, k, v)
        else:
            with torch.no_grad():
                out, _ = mha(q, k, v)
    return out, calls


def test_a_forward_the_backward_would_refuse_is_refused_before_any_launch():
    """d_k = 32: the forward takes Lk <= 16220, the backward's query side Lk <= 8094, its key side Lq <= 8032."""
    from st_amd import native as nv
    assert nv.attn_dense_lds_floats(32, 8032, 8094) == (8094 + 164, 16384, 16384)
    nv.attn_dense_check(32, 8032, 8094)
    nv.attn_dense_check(32, 9000, 16220, backward=False)
    for Lq, Lk, side in ((3, 8095, "2 Lk + 6 d_k + 4 = 16386"), (8033, 3, "2 Lq + 10 d_k = 16386")):
        launched = []
        with pytest.raises(ValueError) as e:
            _mha_call(Lq, Lk, grad=True, calls=launched)
        assert launched == []                                      # refused before anything ran
        for needle in ("Lq = %d" % Lq, "Lk = %d" % Lk, "d_k = 32", "16384", side):
            assert needle in str(e.value), (needle, str(e.value))
    with pytest.raises(ValueError) as e:
        nv.attn_dense_check(32, 3, 16221, backward=False)
    assert "Lk + 5 d_k + 4 = 16385" in str(e.value)
    # the same extents without a gradient run (the forward's range)
    calls = []
    orig = nv.attn_dense_check
    try:
        nv.attn_dense_check = lambda *a, **k: (calls.append(k.get("backward")), orig(*a, **k))[1]
        with pytest.raises(ValueError):
            _mha_call(3, 8095, grad=True)
        out, ran = _mha_call(3, 8095, grad=False)
    finally:
        nv.attn_dense_check = orig
    assert calls == [True, False] and "attn_dense_fwd" in ran and out.shape == (1, 3, 128) and bool(torch.isfinite(out).all())
    out, ran = _mha_call(3, 8094, grad=True)
    assert "attn_dense_fwd" in ran and out.requires_grad

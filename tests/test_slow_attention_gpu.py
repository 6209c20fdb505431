"""The slow-path attention kernels - st_attn_dense_fwd / st_attn_dense_bwd (csrc/st_attn_dense.hip) and st_attn_probs
(csrc/st_misc.hip) - called directly and compared with plain fp64 references (tests/_attn_ref.py) at the shapes where their code
paths change: more than 256 keys / queries (the k += 256 strides, all four waves in the block reductions), head widths that take
a second or a partial pass of the head-column loop, leading dimensions other than H d_k, dropout (the three kernels recompute the
keep decision and must agree), P requested with dropout, dead rows and dead keys, the 64 KiB LDS limits.  Every output sits in a
guard, every bf16 operand in NaN surroundings; cases, checks and bounds: tests/_slow_attn.py, tests/LOCAL_BOUNDS.md.  The same
checks are shown to see injected defects in tests/test_slow_attention_cpu.py."""
import pytest
import torch

from tests import _slow_attn as sa

pytestmark = pytest.mark.gpu

DENSE = sa.dense_cases()


@pytest.fixture(scope="module")
def be():
    return sa.gpu_backend()


@pytest.mark.parametrize("kw", [kw for _, kw in DENSE], ids=[i for i, _ in DENSE])
def test_dense_fwd_bwd_against_fp64(kw, be):
    """Shape grid x masks, operand layouts, sharp inputs and needles, dropout (with P requested): O, lse, P, delta, dQ, dK, dV."""
    sa.run(sa.build(**kw), be, what="dense %s" % sa.case_id(kw))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dense_forward_kept_set_is_keep_qk_exactly(p, be):
    """V one-hot over a block of d_k keys, the blocks walked across Lk = 300: O == 0 exactly where keep_qk says dropped.  Pins
    the counter indexing past k = 255 and both parities of q and k (a 2 x 2 block of pairs shares one counter)."""
    c = sa.build_readout(2, 3, 64, 9, 300, p)
    sa.assert_keep_equal(sa.read_keep_fwd(c, be), c.keep, "forward, p = %g" % p)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dense_key_side_kept_set_is_keep_qk_exactly(p, be):
    """dO one-hot over a block of d_k queries, the blocks walked across Lq = 300: dV == 0 exactly where keep_qk says dropped."""
    c = sa.build_readout(2, 3, 64, 300, 9, p)
    sa.assert_keep_equal(sa.read_keep_bwd(c, be), c.keep, "key side of the backward, p = %g" % p)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dense_probabilities_are_returned_before_dropout(p, be):
    """P requested together with dropout == P without dropout, bit for bit (the header: the probabilities BEFORE dropout)."""
    c = sa.build(2, 3, 32, 20, 300, mask="dead", p=p, gseed=70)
    with_drop = sa.run(c, be, what="P with dropout")
    plain = sa.launch(sa.variant(c, p=0.0), be, backward=False, what="P without dropout")
    sa.assert_same_bits(with_drop.g["P"].view, plain.g["P"].view, "P with dropout against P without")
    assert not torch.equal(with_drop.g["O"].view, plain.g["O"].view)               # (dropout did act on O)


@pytest.mark.parametrize("name,kw,Lq_no,Lk_no", sa.lds_cases(), ids=[c[0] for c in sa.lds_cases()])
def test_dense_lds_limits(name, kw, Lq_no, Lk_no, be):
    """The largest extent each kernel's 64 KiB of LDS takes runs and matches the reference; one more is refused with a Python
    exception and nothing is written (accepted and rejected arguments of the contract in include/st_hip.h)."""
    c = sa.build(**kw)
    sa.run(c, be, what="LDS limit %s" % name, backward=kw.get("backward", True))
    n = sa.build(**dict(kw, Lq=Lq_no, Lk=Lk_no))
    Q, K, V, dO, mask = sa.place(n, be.device)
    if name == "fwd":
        g = sa.fwd_guards(n, be.device)
        with pytest.raises(ValueError):
            be.k.attn_dense_fwd(Q, K, V, mask, g["O"].view, g["lse"].view, n.B, n.H, n.Lq, n.Lk, n.scale, probs=g["P"].view)
    else:
        g = sa.bwd_guards(n, be.device)
        lse = torch.zeros(n.H * n.B * n.Lq, dtype=torch.float32, device=be.device)
        with pytest.raises(ValueError):
            be.k.attn_dense_bwd(Q, K, V, mask, dO, lse, g["delta"].view, g["dQ"].view, g["dK"].view, g["dV"].view, n.B, n.H, n.Lq, n.Lk,
                                n.scale)
    torch.cuda.synchronize()
    sa.unwritten(g, "refused %s" % name)


@pytest.mark.parametrize("B,H,dk", sa.PROBS_SHAPES)
@pytest.mark.parametrize("Lk", sa.PROBS_LK)
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_attn_probs_against_fp64(B, H, dk, Lk, packed, be):
    """Ragged q_len / k_len (1 included), causal on and off, pre-scaled keys on and off: P in a guard, structural zeros exact."""
    for causal in (False, True):
        for prescaled in (False, True):
            c = sa.build_probs(B, H, dk, Lk, packed, causal, prescaled)
            sa.run_probs(c, be, what="attn_probs %dx%dx%d Lk %d %s causal %d prescaled %d" % (B, H, dk, Lk, "packed" if packed else "padded",
                                                                                           causal, prescaled))


def test_module_training_dropout_through_the_dense_path():
    sa.run_module_dropout("cuda")

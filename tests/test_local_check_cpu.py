"""The local metric and the guard bands of tests/_local.py have teeth: every defect below - injected into an otherwise
correct EMULATION output (tests/_emul.py; no kernel involved) - (a) passes the whole-tensor relative L2 norm at the tolerance
the kernel tests hold it to, (b) fails check_local / Guarded with a message that names the right row or region, while (c) the
undamaged output passes everything.  The reference is the same emulation evaluated in fp64 (same bf16 rounding points), so the
undamaged comparison also IS the calibration of tests/LOCAL_BOUNDS.md: the reference-only noise figures are asserted here."""
import math

import pytest
import torch

from tests import _emul as em
from tests._local import Guarded, check, check_local, guarded_input, local_figures, rel

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32


def g(*shape, seed=0, scale=1.0, dtype=BF16):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(dtype)


def _gemm_pair(M, N, K):
    """bf16 GEMM output with the kernel tests' input distribution: fp32 accumulation (what is under test) and fp64."""
    X, W, b = g(M, K, seed=1), g(N, K, seed=2, scale=K ** -0.5), g(N, seed=3, dtype=F32)
    return (em.gemm(X, W, torch.zeros(M, N, dtype=BF16), bias=b),
            em.gemm(X, W, torch.zeros(M, N, dtype=BF16), bias=b, dtype=F64))


@pytest.fixture(scope="module")
def big():
    return _gemm_pair(24700, 256, 256)


def _fails(fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    for n in needles:
        assert n in str(e.value), "%r not in: %s" % (n, e.value)
    return str(e.value)


@pytest.mark.parametrize("M,N,K", [(24700, 256, 256), (3000, 256, 1024)])
def test_reference_only_noise_of_a_single_rounding_output(M, N, K, big):
    """Two correct evaluations (fp32 and fp64 accumulation, each rounded to bf16 once) differ by at most 1e-3 in any single
    row and 5e-4 in any single column: the room between 'correct' and the 1e-2 local bound."""
    got, ref = big if (M, N, K) == (24700, 256, 256) else _gemm_pair(M, N, K)
    (_, rows), (_, cols) = local_figures(got, ref)
    print("K = %d: worst row %.3e, worst column %.3e, whole tensor %.3e" % (K, float(rows.max()), float(cols.max()), rel(got, ref)))
    assert float(rows.max()) <= 1e-3 and float(cols.max()) <= 5e-4
    check(got, ref, 1e-2, "undamaged", tol_local=1e-2)


@pytest.mark.parametrize("defect", ["zeroed", "noise"])
def test_last_row_of_24700_missing_or_garbage(defect, big):
    got, ref = big[0].clone(), big[1]
    M = got.shape[0]
    got[M - 1] = 0 if defect == "zeroed" else g(1, 256, seed=9, scale=float(ref.float().pow(2).mean().sqrt()))[0]
    assert 4e-3 < rel(got, ref) < 1e-2
    check(got, ref, 1e-2, "old metric")                                        # (a) the hole
    msg = _fails(lambda: check_local(got, ref, 1e-2, "last row"), "worst row %d" % (M - 1), "1 of %d rows fail" % M)
    assert "index mod 32 / 64 / 96 / 128 = %d / %d / %d / %d" % ((M - 1) % 32, (M - 1) % 64, (M - 1) % 96, (M - 1) % 128) in msg
    _fails(lambda: check(got, ref, 1e-2, "through check", tol_local=1e-2), "local bound violated")
    check(big[0], ref, 1e-2, "undamaged", tol_local=1e-2)                      # (c)


def test_one_chunk_of_eight_columns_wrong_in_a_padded_vocabulary():
    M, N, K, row, c0 = 1000, 4344, 256, 777, 4336
    got, ref = _gemm_pair(M, N, K)
    check(got, ref, 1e-2, "undamaged", tol_local=1e-2)
    got = got.clone()
    got[row, c0:c0 + 8] = -got[row, c0:c0 + 8] + 1.0
    check(got, ref, 1e-2, "old metric")
    _fails(lambda: check_local(got, ref, 1e-2, "chunk"), "worst row %d" % row, "1 of %d rows fail" % M, "8 of %d columns fail" % N)


def test_one_entry_of_an_fp32_vector_ten_percent_off():
    """rstd of the GEMM + LayerNorm emulation and lse of the attention emulation (6,560 entries each)."""
    M, N, K = 6560, 256, 256
    X, W = g(M, K, seed=1), g(N, K, seed=2, scale=K ** -0.5)
    b, gamma, beta = g(N, seed=3, dtype=F32), 1 + 0.2 * g(N, seed=4, dtype=F32), 0.2 * g(N, seed=5, dtype=F32)
    rstd = {}
    for dt in (F32, F64):
        rstd[dt] = torch.zeros(M, dtype=F32)
        em.gemm_ln(X, W, b, None, gamma, beta, torch.zeros(M, N, dtype=BF16), None, rstd[dt], dtype=dt)
    H, lens, dk = 4, [1000, 640], 64
    qkv = g(sum(lens), 3 * H * dk, seed=11)
    ti = lambda v: torch.tensor(v, dtype=I32)
    lse = {}
    for dt in (F32, F64):
        lse[dt] = torch.zeros(H * sum(lens), dtype=F32)
        em.attn_fwd(qkv[:, :256], qkv[:, 256:512], qkv[:, 512:], torch.zeros(sum(lens), 256, dtype=BF16), lse[dt], ti([0, 1000]), ti(lens),
                    ti([0, 1000]), ti(lens), H, 1000, False, 1 / math.sqrt(dk), dtype=dt)
    for name, v, at in (("rstd", rstd, 6559), ("lse", lse, 4321)):
        assert v[F64].numel() == 6560
        check(v[F32], v[F64], 2e-3, name + " undamaged", tol_local=2e-3)
        got = v[F32].clone()
        got[at] *= 1.1
        assert rel(got, v[F64]) < 2e-3
        check(got, v[F64], 2e-3, name + " old metric")
        _fails(lambda: check_local(got, v[F64], 2e-3, name), "worst element %d" % at, "1 of 6560 elements fail")


@pytest.mark.parametrize("dtype", [BF16, F32, I32])
def test_guard_bands_see_one_value_in_each_region(dtype):
    R, C = 37, 40
    ref = (torch.arange(R * C).view(R, C) % 97).to(dtype)

    def fresh():
        gd = Guarded(R, C, dtype, "cpu")
        assert gd.buf.shape == (R + 6, C + 128) and gd.view.shape == (R, C) and gd.view.stride() == (C + 128, 1)
        assert gd.view.data_ptr() % 16 == 0
        if dtype.is_floating_point:
            assert bool(torch.isnan(gd.view).all())                      # an unwritten row trips check's isfinite assertion
        gd.view.copy_(ref)
        return gd

    gd = fresh()
    gd.assert_intact("undamaged")
    check(gd.view, ref, 1e-2, "undamaged", tol_local=1e-2)
    for name, (r, c), where in (("rows above", (2, 64 + 5), "row -1 column 5"), ("rows below", (3 + R, 64 + C - 1), "row %d column %d" % (R, C - 1)),
                                ("columns left", (3 + 10, 63), "row 10 column -1"), ("columns right", (3 + R - 1, 64 + C), "row %d column %d" % (R - 1, C))):
        gd = fresh()
        gd.buf[r, c] = 1
        check(gd.view, ref, 1e-2, "old metric", tol_local=1e-2)           # the window itself is fine: nothing else looked
        _fails(lambda: gd.assert_intact("guard"), name, where, "1 elements")
    vec = Guarded.vec(100, dtype, "cpu")
    assert vec.view.shape == (100,) and vec.view.is_contiguous()
    vec.view.zero_()
    vec.assert_intact("vector")
    vec.buf[0, 64 + 100] = 0                                             # (a ZERO written one element past the end counts too)
    _fails(lambda: vec.assert_intact("vector"), "columns right", "column 100")
    cache = Guarded(2 * 3 * 4, 16, dtype, "cpu", pad_cols=(0, 0), shape=(2, 3, 4, 16))
    assert cache.view.shape == (2, 3, 4, 16) and cache.view.is_contiguous()
    cache.view.zero_()
    cache.assert_intact("contiguous window")


def test_a_row_of_no_utterance_written_in_a_padded_layout():
    """Padded attention layout [B, T] with lengths below T: the rows between the utterances belong to nobody and the kernels
    never write them.  The tests compare utterance rows only, so a write there is invisible to the old metric."""
    H, dk, lens, T = 2, 32, [20, 33], 33
    d = H * dk
    q = g(2 * T, 3 * d, seed=3)
    ti = lambda v: torch.tensor(v, dtype=I32)
    meta = (ti([0, T]), ti(lens), ti([0, T]), ti(lens))
    ref = torch.zeros(2 * T, d, dtype=BF16)
    em.attn_fwd(q[:, :d], q[:, d:2 * d], q[:, 2 * d:], ref, torch.zeros(H * 2 * T, dtype=F32), *meta, H, T, False, dk ** -0.5, dtype=F64)
    gd = Guarded(2 * T, d, BF16, "cpu")
    em.attn_fwd(q[:, :d], q[:, d:2 * d], q[:, 2 * d:], gd.view, torch.zeros(H * 2 * T, dtype=F32), *meta, H, T, False, dk ** -0.5)
    rows = torch.zeros(2 * T, dtype=torch.bool)
    for o, n in zip((0, T), lens):
        rows[o:o + n] = True
    gd.assert_intact("undamaged"), gd.assert_untouched(~rows, "undamaged")
    check(gd.view[rows], ref[rows], 1.5e-2, "undamaged", tol_local=1.5e-2)
    gd.view[25, 8:16] = 0                                                # zeros: what a zero-filled output would have hidden
    check(gd.view[rows], ref[rows], 1.5e-2, "old metric", tol_local=1.5e-2)
    gd.assert_intact("the guards around the window do not see it either")
    _fails(lambda: gd.assert_untouched(~rows, "gap"), "first at row 25 column 8", "8 elements in 1 rows")


def test_an_operand_read_outside_its_window_turns_the_output_non_finite():
    x = g(50, 72, seed=1)
    xin = guarded_input(x, "cpu")
    assert torch.equal(xin, x) and xin.stride() == (72 + 128, 1)
    wide = torch.as_strided(xin, (50, 80), xin.stride(), xin.storage_offset())      # a kernel that reads one chunk too many
    _fails(lambda: check(wide.float().sum(1), x.float().sum(1), 2e-3, "read past K"), "non-finite")

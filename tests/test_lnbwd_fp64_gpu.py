"""The LayerNorm-backward family (through st_amd.native) against the plain fp64 reference tests/_lnbwd_ref.py: st_ln_bwd at N = 128,
256, 512 with a ragged last row group and with the grid-stride loop taken twice, with and without mask, with output dropout;
st_gemm_lnbwd as the 4-wave kernels and the 8-wave 64- / 128-row tile variants at N = 256 and 512, with and without aux, with dropout;
st_row_chain_bwd as the 32-row, the split and the pipelined 64- / 96-row kernels (column sums through the workspace and
st_colsum_fold, folded at once and deferred), head0, ffn + tail and tail alone - on the families of tests/_lnbwd_cases.py: today's
benign inputs, rstd over six orders of magnitude, a gradient that lies almost wholly in the LayerNorm's null space, a hard gamma, dead
rows and st_ln_bwd's mask at its edge.  A chain is referenced stage by stage from the tensors the kernel itself wrote for the stage
before; delta from the kernel's own dctx as stored, dbias of the fused kernels from their own stored dx.  Every matrix row is judged
against its OWN reference norm.  Families, checks and where the bounds come from: tests/_lnbwd_cases.py, tests/LOCAL_BOUNDS.md; the
same checks are shown to see injected defects in tests/test_lnbwd_fp64_cpu.py.  Every case's figures go to the report directory
(ST_TEST_REPORT_DIR, default test_reports/) as lnbwd_accuracy.txt; a copy lives in profiles/lnbwd_accuracy.txt."""
import os

import pytest

from tests import _lnbwd_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = os.environ.get("ST_TEST_REPORT_DIR") or os.path.join(ROOT, "test_reports")      # (kept out of git)
CASES = lc.cases()


@pytest.fixture(scope="module")
def be():
    return lc.gpu_backend()


@pytest.fixture(scope="module")
def report():
    rows = []
    yield rows
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, "lnbwd_accuracy.txt"), "w") as f:
        f.write(lc.table(rows))


@pytest.mark.parametrize("kw", [kw for _, kw in CASES], ids=[i for i, _ in CASES])
def test_layernorm_backward_against_fp64(kw, be, report):
    lc.run(kw, be, report=report)


def test_the_chain_cases_reach_the_kernels_they_name():
    """What the host-side dispatch says about the chains' shapes (csrc/st_rowchain.hip): no column-sum workspace at 70 rows (the 32-row
    and split kernels add atomically), one workspace row per 64-row workgroup past 8,192 rows and per 96-row workgroup past 16,384 -
    and only for HEAD + FFN + TAIL."""
    from st_amd import native as nv
    rows = nv.load()._cdll.st_row_chain_bwd_colsum_rows
    assert rows(70, 1, lc.D_FF, 1) == 0
    assert rows(8200, 1, lc.D_FF, 1) == -(-8200 // 64) and rows(16400, 1, lc.D_FF, 1) == -(-16400 // 96)
    assert rows(8200, 0, lc.D_FF, 1) == 0 and rows(8200, 1, lc.D_FF, 0) == 0

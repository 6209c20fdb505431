"""Every kernel that forms a LayerNorm behind a GEMM (through st_amd.native) against a plain fp64 reference on rows that are not
N(0, 1): st_gemm_ln (plain, 8-wave K split, the 64- and 128-row 8-wave tile variants at N = 256 and 512, ReLU + positional encoding),
st_row_chain as the 32-row, the split (d_ff 512: two workgroups per row block) and the pipelined 64- / 96-row kernels,
st_row_chain512, and the PRE stage of st_attn_f1_fwd (st_attn_sf1_fwd's PRE stage is the same code and is not run here) - on centred rows, rows
whose mean is 8 .. 512 row standard deviations away (through the fp32 bias, and 64.0 through the residual), rows whose variance is
comparable to eps and far below it (also with eps = 1e-5), and constant rows.  rstd element by element within L_RSTD = 1e-4 of fp64,
out / xhat / pre within the single-rounding bound row by row, the constant rows exact, all outputs in guards and all bf16 operands in NaN
surroundings.  Families, checks and where the bounds come from: tests/_ln_stats.py, tests/LOCAL_BOUNDS.md; the same checks are shown to
see injected defects in tests/test_ln_stats_cpu.py.  Every case's worst rstd figure goes to the report directory (ST_TEST_REPORT_DIR,
default test_reports/) as ln_stats_accuracy.txt; a copy lives in profiles/ln_stats_accuracy.txt."""
import os

import pytest
import torch

from tests import _ln_stats as ls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = os.environ.get("ST_TEST_REPORT_DIR") or os.path.join(ROOT, "test_reports")      # (kept out of git)
CASES = ls.cases()


@pytest.fixture(scope="module")
def be():
    return ls.gpu_backend()


@pytest.fixture(scope="module")
def report():
    rows = []
    yield rows
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, "ln_stats_accuracy.txt"), "w") as f:
        f.write(ls.table(rows))


@pytest.mark.parametrize("kw", [kw for _, kw in CASES], ids=[i for i, _ in CASES])
def test_layernorm_statistic_against_fp64(kw, be, report):
    ls.run(kw, be, report=report)


def test_the_split_case_takes_the_split_kernel(be):
    """st_row_chain ignores the scratch unless the chain has two or more hidden chunks: with d_ff 512 the second LayerNorm runs on
    partial sums that went through the scratch and were added in chunk order - a result that differs in rounding from the
    one-workgroup chain's (include/st_hip.h), which itself is reproducible (asserted first); with d_ff 256 the scratch changes nothing."""
    def outputs(iid, split):
        c = ls.build(iid, "centred")
        gd = ls.launch(c, be, split=split)
        return {nm: gd[nm].view.detach().cpu() for nm in ("rstd0", "H", "rstd1", "xhat1", "out1")}

    one, again, split = outputs("chain-split-dff512", False), outputs("chain-split-dff512", False), outputs("chain-split-dff512", True)
    for nm in one:
        assert torch.equal(one[nm], again[nm]), "the one-workgroup chain is not reproducible: %s" % nm
    assert not torch.equal(one["rstd1"], split["rstd1"]), "d_ff 512 with the scratch did not take the split kernel: rstd1 is bit for bit the one-workgroup chain's"
    a, b = outputs("chain-split", False), outputs("chain-split", True)
    assert all(torch.equal(a[nm], b[nm]) for nm in a), "one hidden chunk: the scratch must change nothing"

"""The eight kernels that carry their own log-sum-exp over the vocabulary (through st_amd.native) against the plain fp64 reference
tests/_lse_ref.py: st_ce_fwd / st_ce_bwd, st_ce_smooth_fwd / _bwd (smoothed with a denominator, and at (1, 0, -1)), st_ce_eval_fwd
(both targets), st_ctc_gather / st_ctc_dlogits with 16-byte and with scalar loads, st_ctc_vocab_lp (also at a row count that is no multiple
of 4 with one utterance shorter), st_beam_advance without and with `work`, st_beam_pre_beam - and st_ctc_best_path's arg-max on the
one-hot and masked rows - over the row families of tests/_lse_cases.py at V = 2, 5, 257, 513, 2,049, 4,337, 5,120: today's random-normal
rows, uniform rows (every candidate ties), one-hot@j at the pass boundaries, ramps, peaked rows, offsets up to +-1,000, rows with
-inf (masked) logits, -1e30 padding counted as valid.  Columns >= V and the surroundings of every logits buffer are NaN; every output
sits in a Guarded buffer.  lse is held to L_LSE + ulp32(|ref|) element by element, derived log-probabilities to L_LSE + ulp32(|lse|) +
ulp32(|ref|), gradients element by element in probability units to 2^-8 |ref| + P_REL p + 2^-126 (next to the whole-tensor and per-row
bounds in force); choices equal the reference's list, adjacent near ties excepted and counted.  Families, checks and where L_LSE and
P_REL come from: tests/_lse_cases.py, tests/LOCAL_BOUNDS.md; the same checks are shown to see injected defects in
tests/test_lse_fp64_cpu.py.  The figures go to the report directory (ST_TEST_REPORT_DIR, default test_reports/) as lse_accuracy.txt; a
copy lives in profiles/lse_accuracy.txt."""
import os

import pytest

from tests import _lse_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = os.environ.get("ST_TEST_REPORT_DIR") or os.path.join(ROOT, "test_reports")      # (kept out of git)
CASES = lc.cases()


@pytest.fixture(scope="module")
def be():
    return lc.gpu_backend()


@pytest.fixture(scope="module")
def report():
    rep = lc.Report()
    yield rep
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, "lse_accuracy.txt"), "w") as f:
        f.write(rep.table())


@pytest.mark.parametrize("kernel,family", [kw for _, kw in CASES], ids=[i for i, _ in CASES])
def test_vocabulary_lse_against_fp64(kernel, family, be, report):
    lc.run(kernel, family, be, rep=report)


def test_near_tie_exemptions_stay_rare(be):
    """Over every kernel that chooses (both st_beam_advance forms, st_beam_pre_beam) and every family: the share of rows whose choice
    used the near-tie exemption is capped, and it is zero on the families whose seeds were picked to show no near tie."""
    rep = lc.Report()
    for kernel in ("beam_advance", "beam_advance_work", "beam_pre_beam"):
        for family in lc.RUNNERS[kernel][2]:
            lc.run(kernel, family, be, rep=rep)
    assert rep.choices and rep.exempt_share() <= lc.EXEMPT_SHARE, rep.table()
    assert all(used == 0 for (_, fam), (_, used) in rep.choices.items() if fam in lc.NO_EXEMPTION), rep.table()

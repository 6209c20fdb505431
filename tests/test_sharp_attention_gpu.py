"""The fast attention kernels (st_attn_fwd / st_attn_bwd through st_amd.native) against a plain fp64 reference at the scores of a
trained model, family by family: the general kernels (causal, 32- / 64- / 128-wide heads), their two-term-P forward, the
few-queries / many-keys kernels (KS = 2, the forward of csrc/st_attn_xs.hip, the merged backward launch with and without its
cross-workgroup key split), the long-sequence forward of csrc/st_attn64.hip, the backward streams of csrc/st_attn_bwd64.hip, the
two-launch backward, and each with dropout.  Every output within 1.25 x of what the kernels' own bf16 rounding points cost
(the emulation with exact arithmetic in between, computed here on the CPU), row by row within the attention bounds, in guards.
Cases, checks and where the bounds come from: tests/_sharp_attn.py, tests/LOCAL_BOUNDS.md; the same checks are shown to see
injected defects in tests/test_sharp_attention_cpu.py; the measured margins: profiles/attn_sharp_accuracy.txt."""
import os

import pytest
import torch

from tests import _sharp_attn as sh

pytestmark = pytest.mark.gpu

CASES = sh.cases()


@pytest.fixture(scope="module")
def be():
    return sh.gpu_backend()


@pytest.mark.parametrize("kw", [kw for _, kw in CASES], ids=[i for i, _ in CASES])
def test_attention_family_against_fp64_at_sharp_scores(kw, be):
    sh.run(kw, be)


def test_plain_keys_at_a_streams_shape_take_the_general_kernels(be):
    """The backward streams re-round their register-resident operand when the keys are not pre-scaled (csrc/st_attn.hip,
    bwd_long64): st_attn_bwd must not send plain keys there.  With the default environment dQ / dK / dV of a streams-shaped
    problem are bit for bit those of ST_ATTN_BWD64=0 (the general kernels, which are reproducible: asserted first); with
    pre-scaled keys the switch still changes the kernel - the streams remain in use where they are accurate."""
    kw = dict(dict(CASES)["bwd64-plain-s3"])
    c, ck = sh.build(**kw), sh.build(**dict(dict(CASES)["bwd64-prescaled-s3"]))

    def run(case, mode):
        with be.switches({} if mode is None else {"ST_ATTN_BWD64": mode}):
            g = sh.launch(case, be)
        return [g[n].view.detach().cpu()[case.rows[sh.side(n)]] for n in sh.OUT_BWD]

    assert os.environ.get("ST_ATTN_BWD64") is None
    general, again, default = run(c, "0"), run(c, "0"), run(c, None)
    for a, b, d, nm in zip(general, again, default, sh.OUT_BWD):
        assert torch.equal(a, b), "the general kernels' backward is not reproducible: %s" % nm
        assert torch.equal(a, d), "plain keys at a streams shape did not take the general kernels: %s differs from ST_ATTN_BWD64=0" % nm
    assert any(not torch.equal(a, b) for a, b in zip(run(ck, "0"), run(ck, None))), "pre-scaled keys no longer reach the streams"

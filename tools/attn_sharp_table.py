"""The kernel-level accuracy table of the fast attention kernels at sharp scores: every case of tests/_sharp_attn.py (the cases of
tests/test_sharp_attention_gpu.py) through st_amd.native on the GPU, against the fp64 reference.  Per family, s (q, k = 0.7 s
N(0, 1)) and output: the floor (the emulation with exact arithmetic between the kernels' bf16 rounding points), the kernel's
error and their ratio - the test holds the ratio to 1.25.  Nothing is asserted here.

    python tools/attn_sharp_table.py [output file, default profiles/attn_sharp_accuracy.txt]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-tranformer-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import _sharp_attn as sh          # noqa: E402


def main(path):
    be = sh.gpu_backend()
    lines = ["# relL2 against fp64 (tests/_attn_ref.packed_attention) over the utterances' rows; floor: tests/_emul.py with dtype=float64;",
             "# O+Ores: held to %.0e instead of a ratio (tests/_sharp_attn.py, L_OSUM)" % sh.L_OSUM,
             "%-12s %-18s %-2s %-5s %-7s %10s %10s %7s" % ("family", "case", "s", "drop", "output", "floor", "kernel", "ratio")]
    worst = {}
    for _, kw in sh.cases():
        c = sh.build(**kw)
        err, floor = sh.errors(c, sh.outputs(c, sh.launch(c, be))), sh.floors(kw)
        for nm, e in err.items():
            lines.append("%-12s %-18s %-2d %-5s %-7s %10.3e %10.3e %7.3f" % (c.family, c.name, c.s, "yes" if c.p > 0 else "no", nm, floor[nm], e,
                                                                            e / floor[nm]))
            if nm != "O+Ores":
                worst[c.family] = max(worst.get(c.family, 0.0), e / floor[nm])
    lines.append("# worst ratio per family: " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "attn_sharp_accuracy.txt"))

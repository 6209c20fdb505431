"""Build libst_hip.so (the C-ABI HIP library) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build
container; the resulting .so travels to the GPU box with the source tree.
Staleness is decided by a content hash of csrc/ and include/st_hip.h stored next to the library
(file mtimes do not survive the copy to the GPU box).  Every source is compiled
to its own object (in parallel; objects are cached by content hash under
lib/obj/), then linked.
"""
import hashlib
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include")
ABI_HEADER = os.path.join(INCLUDE, "st_hip.h")       # the one copy of the C ABI: the sources are compiled against it, native.py parses it
LIBDIR = os.path.join(os.path.dirname(HERE), "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIB = os.path.join(LIBDIR, "libst_hip.so")
STAMP = LIB + ".srchash"
SOURCES = ["st_gemm_sym.hip", "st_wgrad.hip", "st_gemm_ws.hip", "st_gemm_ln.hip", "st_gemm_lnbwd.hip", "st_rowchain.hip", "st_attn.hip",
           "st_attn64.hip", "st_attn_bwd64.hip", "st_attn_xs.hip", "st_attn_dense.hip", "st_misc.hip",
           "st_ctc_decode.hip", "st_ctc_loss.hip", "st_ctc_align.hip", "st_ctc_beam.hip", "st_ngram.hip", "st_bias.hip", "st_loss.hip", "st_augment.hip", "st_optim.hip", "st_eval.hip"]
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-fPIC", "-Wno-unused-result",
         "-I" + os.path.relpath(INCLUDE, CSRC)]      # (relative: hipcc runs in csrc/, and the flags are part of the source hash, which must not depend on where the checkout lies)
# per-file additions (none today; a kernel that owns all 512 registers per lane would want "-mllvm -amdgpu-mfma-vgpr-form":
# left to its heuristics the compiler then puts score accumulators into AGPRs and pays a v_accvgpr_read per score)
EXTRA = {}
if os.environ.get("ST_MERGE_FENCE") == "1":
    # the last-arriver merges with language-level agent-scope release / acquire fences (csrc/st_common.cuh): the documented
    # conservative build; the flag is part of the source hash, so the library is rebuilt when the switch changes
    FLAGS = FLAGS + ["-DST_MERGE_FENCE=1"]
if os.environ.get("ST_DEV_DEFS"):
    # development: extra -D switches for same-box A/Bs of kernel variants (tools/dev/ab_defs.sh); part of the source hash, so
    # every setting is its own library build.  The shipped library is built without.
    FLAGS = FLAGS + os.environ["ST_DEV_DEFS"].split()
if os.environ.get("ST_DEV_TRACE") == "1":
    # development: the per-workgroup clock-stamp hook of the attention backward streams (tools/dev/attn_bwd64_trace.py); the
    # shipped library has no code that writes through an address taken from the environment
    FLAGS = FLAGS + ["-DST_DEV_TRACE=1"]


def _headers() -> bytes:
    with open(ABI_HEADER, "rb") as f:
        h = b"st_hip.h" + f.read()
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".cuh", ".h", ".inc")):
            with open(os.path.join(CSRC, name), "rb") as f:
                h += name.encode() + f.read()
    return h


def source_hash() -> str:
    h = hashlib.sha256(" ".join(FLAGS + sorted(sum(([k] + v for k, v in EXTRA.items()), []))).encode())
    with open(ABI_HEADER, "rb") as f:
        h.update(f.read())
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), "rb") as f:
            h.update(name.encode())
            h.update(f.read())
    return h.hexdigest()


def _stale() -> bool:
    if not (os.path.exists(LIB) and os.path.exists(STAMP)):
        return True
    with open(STAMP) as f:
        return f.read().strip() != source_hash()


def _compile(hipcc: str, src: str, headers: bytes, verbose: bool) -> str:
    flags = FLAGS + EXTRA.get(src, [])
    with open(os.path.join(CSRC, src), "rb") as f:
        key = hashlib.sha256(" ".join(flags).encode() + headers + f.read()).hexdigest()[:24]
    obj = os.path.join(OBJDIR, "%s.%s.o" % (os.path.splitext(src)[0], key))
    if not os.path.exists(obj):
        for old in os.listdir(OBJDIR):
            if old.startswith(os.path.splitext(src)[0] + "."):
                os.remove(os.path.join(OBJDIR, old))
        cmd = [hipcc] + flags + ["-c", os.path.join(CSRC, src), "-o", obj + ".tmp"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=CSRC)
        os.replace(obj + ".tmp", obj)
    return obj


def build_lib(force: bool = False, verbose: bool = False) -> str:
    """Compile the library if it is missing or was built from different sources."""
    if not force and not _stale():
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libst_hip.so")
    os.makedirs(OBJDIR, exist_ok=True)
    headers = _headers()
    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 4)) as ex:
        objs = list(ex.map(lambda s: _compile(hipcc, s, headers, verbose), SOURCES))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(LIB + ".tmp", LIB)
    with open(STAMP, "w") as f:
        f.write(source_hash())
    return LIB


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))

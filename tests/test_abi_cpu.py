"""-m "not gpu": the C-ABI library builds, loads, and exports exactly the entry
points include/st_hip.h declares (no compute calls - there is no GPU here); the header is the one copy of the ABI - the
sources are compiled against it and the binding is parsed from it."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from st_amd import build, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st_hip.h")
DEV_HOOKS = {"st_dev_chain_trace"}        # development entry points: defined in csrc/, deliberately not in the header or the binding


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_declarations():
    """name -> parameter text of every `int st_*(...);` of the header, in header order."""
    return dict(re.findall(r"\bint\s+(st_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", _header_text(), flags=re.S))


def _source(name):
    with open(os.path.join(build.CSRC, name)) as f:
        return f.read()


def test_library_exports_header_symbols():
    """ONE list: what the header declares == what the binding binds == what the library exports == what the sources define
    (development hooks aside) - for every entry point, whichever feature brought it."""
    lib = native.load()
    declared = _header_declarations()
    assert list(declared) == list(native.SIGNATURES), (set(declared) ^ set(native.SIGNATURES))
    syms = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT\s+(st[a-z0-9]*_[a-z0-9_]+)$", syms, flags=re.M))
    assert exported - DEV_HOOKS == set(declared), exported ^ set(declared)
    for name, args in declared.items():
        params = [] if args.strip() == "void" else args.split(",")
        assert len(params) == len(native.SIGNATURES[name]), name
        want = [ctypes.c_void_p if "*" in a or a.split()[0] == "st_stream_t" else native._CTYPES[" ".join(a.replace("const", " ").split()[:-1])]
                for a in params]
        assert want == native.SIGNATURES[name], name
        assert isinstance(getattr(lib, name), native._Timed), name          # bound through the per-launch timing bracket
    assert lib.st_version() == native.ABI_VERSION


def test_sources_define_exactly_the_declared_entry_points():
    """Every `extern "C" int st*_*` of the library's sources is a declaration of the header or a development hook - and nothing
    the header declares is left undefined."""
    found = set()
    for src in build.SOURCES:
        found |= set(re.findall(r'extern\s+"C"\s+int\s+(st[a-z0-9]*_\w+)\s*\(', _source(src)))
    declared = set(_header_declarations())
    assert found == declared | DEV_HOOKS, (found ^ (declared | DEV_HOOKS))


def test_every_source_is_compiled_against_the_header():
    """st_hip.h reaches every translation unit - directly, or through a header the file demonstrably includes - so a definition
    that disagrees with its declaration stops the build."""
    def includes(name, seen):
        if name in seen:
            return False
        seen.add(name)
        local = re.findall(r'^\s*#\s*include\s+"([^"]+)"', _source(name), flags=re.M)
        return "st_hip.h" in local or any(os.path.exists(os.path.join(build.CSRC, h)) and includes(h, seen) for h in local)
    for src in build.SOURCES:
        assert includes(src, set()), "%s does not include st_hip.h" % src
    assert any(f == "-I" + os.path.relpath(os.path.dirname(HEADER), build.CSRC) for f in build.FLAGS)
    assert os.path.samefile(build.ABI_HEADER, HEADER)


def test_header_edits_rebuild(monkeypatch, tmp_path):
    """The header's bytes are part of the library's source hash and of every object's cache key."""
    other = tmp_path / "st_hip.h"
    other.write_bytes(open(HEADER, "rb").read() + b"/* edited */\n")
    before = build.source_hash(), build._headers()
    monkeypatch.setattr(build, "ABI_HEADER", str(other))
    assert build.source_hash() != before[0] and build._headers() != before[1]


def test_width_sensitive_slots_of_the_parsed_binding():
    """Pinned literally, so a parser bug cannot hide behind "derived from the header": an int where a long long belongs shifts or
    truncates the arguments of kernels that see raw pointers."""
    S = native.SIGNATURES
    for name, args in _header_declarations().items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert n == len(S[name]), (name, n, len(S[name]))
    assert S["st_gemm_splitk"][-1] is ctypes.c_longlong and S["st_gemm_splitk"][-2] is ctypes.c_void_p
    assert S["st_gemm_stacked"][-2:] == [ctypes.c_long, ctypes.c_long] and S["st_gemm_stacked"][-3] is ctypes.c_int
    assert S["st_gemm_ws"][-2:] == [ctypes.c_long, ctypes.c_long]
    assert S["st_gemm"][18] is ctypes.c_uint and S["st_gemm"][20] is ctypes.c_float and S["st_gemm"][19] is ctypes.c_int
    assert S["st_gemm"][0] is ctypes.c_void_p and S["st_gemm"][17] is ctypes.c_void_p and len(S["st_gemm"]) == 22
    assert S["st_zero"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    assert S["st_version"] == [] and len(S["st_version"]) == 0 and S["st_wfrag_depth"] == []
    assert len(S["st_adam_clip"]) == 19 and S["st_adam_clip"][1] is ctypes.c_longlong
    assert S["st_adam_clip"][9:14] == [ctypes.c_float] * 5          # max_norm, beta1, beta2, eps, grad_scale
    assert S["st_adam_clip"][-5:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    assert len(S["st_grad_norm"]) == 9 and S["st_grad_norm"][-2:] == [ctypes.c_void_p, ctypes.c_void_p]
    assert S["st_grad_norm"][2] is ctypes.c_longlong and S["st_grad_norm"][6] is ctypes.c_float
    assert S["st_row_chain"][-2] is ctypes.c_longlong and S["st_row_chain"][-1] is ctypes.c_float
    assert S["st_row_chain"][22] is ctypes.c_void_p          # unsigned long long* relu_bits: a pointer, not a scalar
    assert S["st_attn_bwd"][-1] is ctypes.c_longlong and S["st_ctc_loss_fwd"][-2] is ctypes.c_longlong
    assert S["st_beam_advance_joint"][5] is ctypes.c_float


@pytest.mark.parametrize("decl,param", [("int st_a(st_stream_t stream, double x);", "double x"),
                                        ("int st_b(const void* p, size_t n);", "size_t n"),
                                        ("int st_c(int k, struct st_opts opts);", "struct st_opts opts"),
                                        ("int st_d(unsigned long long words);", "unsigned long long words")])
def test_parser_refuses_a_type_it_does_not_know(decl, param):
    text = "#define ST_ABI_VERSION 6\nenum { %s };\n%s\n" % (", ".join("ST_EPI_%d = %d" % (i, i) for i in range(8)), decl)
    with pytest.raises(RuntimeError) as e:
        native.parse_header(text)
    assert param in str(e.value) and decl[4:8] in str(e.value)
    ok = text.replace(param, "long long n")
    sigs, version, epi = native.parse_header(ok)
    assert sigs[decl[4:8]][-1] is ctypes.c_longlong and version == 6 and len(epi) == 8


def test_version_and_epilogues_come_from_the_header():
    text = _header_text()
    assert native.ABI_VERSION == int(re.search(r"#define\s+ST_ABI_VERSION\s+(\d+)", text).group(1)) == native.load().st_version()
    assert len(re.findall(r"#define\s+\w*VERSION\b", text)) == 1 and not [n for n in native.SIGNATURES if n.endswith("_version") and n != "st_version"]
    enum = dict(re.findall(r"\bST_(EPI_\w+)\s*=\s*(\d+)", text))
    assert len(enum) == 8 and sorted(map(int, enum.values())) == list(range(8))
    for name, value in enum.items():
        assert getattr(native, name) == int(value), name
    # only the header carries the number
    assert not re.search(r"return\s+\d+\s*;", re.search(r"int st_version\(void\)[^\n]*", _source("st_misc.hip")).group(0))
    assert not re.search(r"^ABI_VERSION\s*=\s*\d", open(native.__file__).read(), flags=re.M)


# ---- the version is a fingerprint of the declarations: derived, so no test (this one included) spells the number out -------------
def _macro(text):
    return int(re.search(r"#define\s+ST_ABI_VERSION\s+(\d+)", text).group(1))


def test_the_version_is_the_fingerprint_of_the_header():
    text = open(HEADER).read()
    assert _macro(text) == native.abi_fingerprint(text) == native.ABI_VERSION == native.load().st_version()
    assert native.check_fingerprint(text) == native.ABI_VERSION


SYNTHETIC = """/* a synthetic header */
#define ST_ABI_VERSION 0
enum { %s };
int st_a(st_stream_t stream, const float* p, long long n);
int st_b(int k, float x, const void* const* X);
int st_c(void);
""" % ", ".join("ST_EPI_%d = %d" % (i, i) for i in range(8))


@pytest.mark.parametrize("old,new", [
    ("int k, float x", "long long k, float x"),                                    # a parameter's type: int -> long long
    ("const float* p", "const float p"),                                           # ... float* -> float
    ("long long n);", "long long n, int flag);"),                                  # a parameter added
    ("int k, float x,", "int k,"),                                                 # ... removed
    ("int st_c(void);", "int st_c(void);\nint st_d(int k);"),                      # a declaration added
    ("int st_b(", "int st_bb("),                                                   # ... renamed
    ("int st_b(int k, float x, const void* const* X);\nint st_c(void);",
     "int st_c(void);\nint st_b(int k, float x, const void* const* X);"),          # two declarations swapped
    ("ST_EPI_3 = 3", "ST_EPI_3 = 9"),                                              # an epilogue selector's value
])
def test_fingerprint_changes_with_the_abi(old, new):
    assert SYNTHETIC.count(old) == 1
    assert native.abi_fingerprint(SYNTHETIC.replace(old, new)) != native.abi_fingerprint(SYNTHETIC)


@pytest.mark.parametrize("old,new", [
    ("/* a synthetic header */", "/* another comment */"),                         # a comment edited
    ("int k, float x", "int k, /* the count */ float x"),                          # ... added inside a parameter list
    (", const float* p, ", ",\n         const float *p ,\n  "),                    # whitespace and line breaks
    ("int st_c(void);", "int   st_c ( void ) ;"),
    ("float x", "float scale"),                                                    # a parameter renamed
    ("const float* p", "float* p"),                                                # const removed
    ("int k", "const int k"),                                                      # ... added
    ("const void* const* X", "void** Y"),
])
def test_fingerprint_ignores_what_is_not_the_abi(old, new):
    assert SYNTHETIC.count(old) == 1
    assert native.abi_fingerprint(SYNTHETIC.replace(old, new)) == native.abi_fingerprint(SYNTHETIC)


def test_an_edited_declaration_fails_the_import_and_names_the_number(tmp_path):
    """A signature edited without touching ST_ABI_VERSION: check_fingerprint, and with it `import st_amd.native` (a fresh
    interpreter whose build.ABI_HEADER points at the edited copy), raises and prints the value to write."""
    import sys
    text = open(HEADER).read()
    edited = text.replace("int st_zero(st_stream_t stream, void* ptr, long long bytes);", "int st_zero(st_stream_t stream, void* ptr, int bytes);")
    assert edited != text
    want = native.abi_fingerprint(edited)
    assert want != native.ABI_VERSION
    with pytest.raises(RuntimeError, match=r"ST_ABI_VERSION %d\b" % want):
        native.check_fingerprint(edited)
    assert native.check_fingerprint(re.sub(r"(#define\s+ST_ABI_VERSION\s+)\d+", r"\g<1>%d" % want, edited)) == want
    (tmp_path / "st_hip.h").write_text(edited)
    code = "from st_amd import build; build.ABI_HEADER = %r; import st_amd.native" % str(tmp_path / "st_hip.h")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path)))
    assert r.returncode != 0 and "RuntimeError" in r.stderr and "#define ST_ABI_VERSION %d" % want in r.stderr, r.stderr[-2000:]


def test_a_missing_header_is_a_broken_checkout(monkeypatch, tmp_path):
    monkeypatch.setattr(build, "ABI_HEADER", str(tmp_path / "nowhere" / "st_hip.h"))
    with pytest.raises(RuntimeError, match="broken checkout"):
        native._read_header()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc is not installed")
def test_a_definition_that_disagrees_with_the_header_does_not_compile(tmp_path):
    """One host-only syntax pass of st_gemm_sym.hip against a copy of the header whose st_gemm takes `long long ldx`."""
    text = open(HEADER).read()
    changed = text.replace("int st_gemm(st_stream_t stream, int x_cmajor, int y_cmajor, const void* X, int ldx,",
                           "int st_gemm(st_stream_t stream, int x_cmajor, int y_cmajor, const void* X, long long ldx,")
    assert changed != text
    (tmp_path / "st_hip.h").write_text(changed)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = ["-I" + str(tmp_path) if f.startswith("-I") else f for f in build.FLAGS]      # the copy instead of include/
    r = subprocess.run([hipcc] + flags + ["--cuda-host-only", "-fsyntax-only", os.path.join(build.CSRC, "st_gemm_sym.hip")],
                       cwd=build.CSRC, capture_output=True, text=True)
    assert r.returncode != 0 and "conflicting types for 'st_gemm'" in r.stderr, r.stderr[-2000:]


def test_no_cpu_fallback():
    """The product path refuses CPU tensors instead of silently emulating."""
    import torch
    import transformer.SubLayers as S
    ff = S.PositionwiseFeedForward(128, 256, dropout=0.0).eval()
    with pytest.raises(RuntimeError):
        ff(torch.randn(2, 3, 128))
    with pytest.raises(RuntimeError):
        native.gemm(torch.zeros(8, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16),
                    torch.zeros(8, 8, dtype=torch.bfloat16))


def test_generated_instruction_streams_are_the_generators_output(tmp_path):
    """csrc/st_attn_bwd64_*.inc are GENERATED (tools/gen_attn_bwd64.py): the committed files must be what the committed
    generator writes, byte for byte (no hand edit of either side goes unnoticed)."""
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith("BWD64_")}      # the development knobs change the output
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_attn_bwd64.py"), str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    csrc = os.path.join(ROOT, "speech-tranformer-pytorch_amd", "csrc")
    made = sorted(os.listdir(tmp_path))
    assert made == sorted(n for n in os.listdir(csrc) if n.startswith("st_attn_bwd64_") and n.endswith(".inc")), made
    for name in made:
        with open(os.path.join(tmp_path, name), "rb") as a, open(os.path.join(csrc, name), "rb") as b:
            assert a.read() == b.read(), name


def test_host_side_plans_of_the_round6_scratch_buffers():
    """The pure host queries of ABI 4 (no launch, no GPU): which backward-chain launches write their column sums to a workspace and
    how many rows it has; which attention backward launches split their dQ items over workgroups and how much scratch they want."""
    lib = native.load()._cdll
    # encoder-sized HEAD + FFN + TAIL launches: 96-row workgroups above 16,384 rows, 64-row above 8,192; everything else: atomics
    assert lib.st_row_chain_bwd_colsum_rows(24060, 1, 1024, 1) == 251
    assert lib.st_row_chain_bwd_colsum_rows(9000, 1, 1024, 1) == 141
    assert lib.st_row_chain_bwd_colsum_rows(1206, 1, 1024, 1) == 0
    assert lib.st_row_chain_bwd_colsum_rows(24060, 0, 1024, 1) == 0 and lib.st_row_chain_bwd_colsum_rows(24060, 1, 0, 1) == 0
    assert lib.st_row_chain_bwd_colsum_rows(24060, 1, 1024, 0) == 0 and lib.st_row_chain_bwd_colsum_rows(0, 1, 1024, 1) == 0
    # few queries against many keys, not causal: up to four parts of whole 128-key tiles; 16 KiB of tickets + parts x 64 x d_k fp32 per item
    assert lib.st_attn_bwd_split_kib(32, 4, 64, 50, 1000, 0) == 16 + 32 * 4 * 4 * 16
    assert lib.st_attn_bwd_split_kib(4, 4, 64, 50, 300, 0) == 16 + 4 * 4 * 3 * 16            # three key tiles: three parts
    assert lib.st_attn_bwd_split_kib(32, 4, 64, 50, 1000, 1) == 0                              # causal
    assert lib.st_attn_bwd_split_kib(32, 4, 64, 1000, 1000, 0) == 0                            # self-attention shapes
    assert lib.st_attn_bwd_split_kib(32, 4, 64, 50, 200, 0) == 0                               # too few keys for the key-split kernels
    assert lib.st_attn_bwd_split_kib(2000, 4, 64, 50, 1000, 0) == 0                            # more items than tickets

"""ctypes binding of libst_hip.so - the C-ABI declared in include/st_hip.h.

Each Python wrapper validates tensor dtype / layout on the host (the kernels
themselves only see raw pointers), passes ``torch.cuda.current_stream()`` and
raises on a non-zero status.  There is deliberately NO fallback: if the library
is missing, or a tensor is not on a GPU, the call raises.

Tensor conventions: activations are 2-D row matrices with ``stride(1) == 1``;
column slices of a wider matrix (``qkv[:, :d]``) are fine - the leading
dimension is taken from ``stride(0)``.
"""
from __future__ import annotations

import ctypes
import os
import re
import zlib
from typing import Optional

import torch

from . import build as _build

_CTYPES = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "long": ctypes.c_long,
           "long long": ctypes.c_longlong}


def _argtypes(name: str, params: str):
    """The ctypes of one declaration's parameter list - the header's C subset is tiny: a parameter with a ``*`` or of type
    st_stream_t is a pointer, the five scalar types above are themselves, and ANY other type raises - a new type in the
    header is a decision, not a default."""
    argtypes = []
    for param in ([] if params.strip() == "void" else params.split(",")):
        words = param.replace("const", " ").split()
        ctype = ctypes.c_void_p if "*" in param or words[0] == "st_stream_t" else _CTYPES.get(" ".join(words[:-1]))
        if ctype is None:
            raise RuntimeError("include/st_hip.h: %s: parameter '%s' has a type the binding does not know" % (name, param.strip()))
        argtypes.append(ctype)
    return argtypes


def _declarations(text: str):
    """(name, parameter list) of every ``int st_*(...);`` declaration of the header text, in header order, comments removed."""
    return re.findall(r"\bint\s+(st_\w+)\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def parse_header(text: str):
    """-> (SIGNATURES: name -> argtypes of every ``int st_*(...);`` declaration, ABI version, the ST_EPI_* enum) of the text
    of include/st_hip.h.  The header's C subset is tiny: a parameter with a ``*`` or of type st_stream_t is a pointer, the five
    scalar types above are themselves, and ANY other type raises - a new type in the header is a decision, not a default."""
    sigs = {name: _argtypes(name, params) for name, params in _declarations(text)}
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    version = re.search(r"#define\s+ST_ABI_VERSION\s+(\d+)", text)
    epi = {k: int(v) for k, v in re.findall(r"\b(ST_EPI_\w+)\s*=\s*(\d+)", text)}
    if not sigs or version is None or len(epi) != 8:
        raise RuntimeError("include/st_hip.h: no declarations / ST_ABI_VERSION / ST_EPI_* found: broken checkout")
    return sigs, int(version.group(1)), epi


def abi_fingerprint(text: str) -> int:
    """What ST_ABI_VERSION must be for this header text: a CRC of the ABI itself.  One line ``NAME(T1,...,Tn)`` per declaration
    in header order - Ti the parameter without ``const``, its name and all whitespace (``const void* const* X`` -> ``void**``,
    ``long long n`` -> ``longlong``, ``(void)`` -> no parameter) - then one line ``NAME=VALUE`` per ST_EPI_* enumerator.
    Comments, layout, parameter names and const-ness do not count; a type, a parameter, a declaration, their order do."""
    lines = []
    for name, params in _declarations(text):
        types = [re.sub(r"\s+", "", re.sub(r"\w+\s*$", "", re.sub(r"\bconst\b", " ", p)))
                 for p in ([] if params.strip() == "void" else params.split(","))]
        lines.append("%s(%s)" % (name, ",".join(types)))
    lines += ["%s=%s" % kv for kv in re.findall(r"\b(ST_EPI_\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", text, flags=re.S))]
    return zlib.crc32("\n".join(lines).encode("utf-8")) & 0x7fffffff


def check_fingerprint(text: str) -> int:
    """The header's ST_ABI_VERSION literal, which must BE the fingerprint of its declarations - or the RuntimeError that names
    the number to write (a declaration was edited; the literal is what st_version() and a C consumer see)."""
    literal, want = parse_header(text)[1], abi_fingerprint(text)
    if literal != want:
        raise RuntimeError("include/st_hip.h: ST_ABI_VERSION is %d but its declarations have the fingerprint %d: a declaration "
                           "changed - write `#define ST_ABI_VERSION %d` and rebuild (python __graft_entry__.py)" % (literal, want, want))
    return literal


def _read_header() -> str:
    try:
        with open(_build.ABI_HEADER) as f:
            return f.read()
    except OSError as e:
        raise RuntimeError("%s is missing (%s): broken checkout - restore it and rebuild (python __graft_entry__.py)"
                           % (_build.ABI_HEADER, e)) from None


# name -> argtypes (restype is int everywhere), the library's ABI version and st_gemm's epilogue selectors: all read from
# include/st_hip.h, the one place they are written down
SIGNATURES, ABI_VERSION, _EPI = parse_header(_read_header())
check_fingerprint(_read_header())      # ... where the version is a fingerprint of the declarations, so an edited one cannot keep it
(EPI_BF16, EPI_BF16_RELU, EPI_F32, EPI_BF16_MASK, EPI_BF16_ADD, EPI_F32_ATOMIC, EPI_F32_ATOMIC_T, EPI_BF16_DELTA) = (
    _EPI["ST_" + k] for k in ("EPI_BF16", "EPI_BF16_RELU", "EPI_F32", "EPI_BF16_MASK", "EPI_BF16_ADD", "EPI_F32_ATOMIC",
                              "EPI_F32_ATOMIC_T", "EPI_BF16_DELTA"))
_c_int = ctypes.c_int

_LIB = None
_TIMING = None   # list of (kernel name, tag, algorithmic bytes, start event, end event) while bench.py profiles a step
_TAG = None
_TAG_BYTES = None


class _Timed:
    """Per-launch HIP-event bracket on torch's current stream (the stream the kernels are
    launched on); off unless ``timing_start()`` was called - bench.py's roofline pass."""

    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __call__(self, *args):
        global _TAG, _TAG_BYTES
        if _TIMING is None:
            return self.fn(*args)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rc = self.fn(*args)
        e.record()
        _TIMING.append((self.name, _TAG, _TAG_BYTES, s, e))
        _TAG = _TAG_BYTES = None
        return rc


class _Lib:
    pass


def timing_start() -> None:
    global _TIMING
    _TIMING = []


def timing_stop():
    """-> list of (name, tag, milliseconds, algorithmic HBM bytes of the launch or None); synchronises the device."""
    global _TIMING
    torch.cuda.synchronize()
    out = [(n, t, s.elapsed_time(e), nb) for n, t, nb, s, e in (_TIMING or [])]
    _TIMING = None
    return out


def _io_bytes(io) -> float:
    """Bytes of a launch's operands, each counted once: items are tensors (whole), (tensor, rows) (the first ``rows`` rows
    of a row matrix / elements of a vector), plain byte counts, or None."""
    n = 0.0
    for item in io:
        if item is None:
            continue
        if isinstance(item, (int, float)):
            n += item
            continue
        t, rows = item if isinstance(item, tuple) else (item, None)
        if t is None:
            continue
        if t.dim() == 2:
            n += (t.shape[0] if rows is None else min(int(rows), t.shape[0])) * t.shape[1] * t.element_size()
        else:
            n += (t.numel() if rows is None else min(int(rows), t.numel())) * t.element_size()
    return n


def _tag(*info, io=None) -> None:
    """Label the next launch for bench.py's per-launch timing pass: ``info`` = (class, shape numbers ...), ``io`` = the
    operands the launch must move through HBM once (its ALGORITHMIC traffic - see _io_bytes)."""
    global _TAG, _TAG_BYTES
    if _TIMING is not None:
        _TAG = info
        _TAG_BYTES = _io_bytes(io) if io is not None else None


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = True):
    """dlopen libst_hip.so (building it first if hipcc is available)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("ST_HIP_LIB") or lib_path()      # (development: A/B a library built from variant sources)
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError("libst_hip.so not built: run `python __graft_entry__.py` (build())")
        _build.build_lib()
    cdll = ctypes.CDLL(path)
    # the ABI version first: a library built from other sources would be called with shifted arguments
    try:
        cdll.st_version.restype = _c_int
        ver = int(cdll.st_version())
    except AttributeError:
        ver = -1
    if ver != ABI_VERSION:
        raise RuntimeError("libst_hip.so at %s has ABI version %d, this binding needs %d: rebuild it (python __graft_entry__.py)"
                           % (path, ver, ABI_VERSION))
    missing = [name for name in SIGNATURES if not hasattr(cdll, name)]
    if missing:
        raise RuntimeError("libst_hip.so at %s lacks %s: rebuild it (python __graft_entry__.py)" % (path, ", ".join(missing)))
    lib = _Lib()
    for name, argtypes in SIGNATURES.items():
        fn = getattr(cdll, name)
        fn.argtypes = argtypes
        fn.restype = _c_int
        setattr(lib, name, _Timed(name, fn))
    lib._cdll = cdll
    _LIB = lib
    return lib


def _stream() -> int:
    """Raw handle of torch's current stream on the current device (torch.cuda.current_stream() builds a Stream object
    per call: ~8 us of host time, measurable in the eager decode loop's ~100 launches per step)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def sustained_clock_mhz(device=None, iters: int = 30000) -> float:
    """The shader clock (MHz) the device holds under ~2 ms of chip-wide dense MFMA work (st_clock_probe): median over the
    compute units' own s_memtime / s_memrealtime ratios.  bench.py records it next to its roofline - the same commit measures
    4-8 % apart on different boxes, and most of that is this number."""
    dev = torch.device("cuda" if device is None else device)
    n_wg = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    out = torch.zeros(2 * n_wg, dtype=torch.int64, device=dev)
    for _ in range(2):       # (the first launch also pays the clock's ramp)
        _check(load().st_clock_probe(_stream(), out.data_ptr(), n_wg, int(iters)), "st_clock_probe")
    torch.cuda.synchronize(dev)
    t = out.view(n_wg, 2).double().cpu()
    return float((100.0 * t[:, 0] / t[:, 1].clamp_min(1)).median())


def env_refresh() -> None:
    """After changing ST_ATTN_FWD64 / ST_ATTN_XS / ST_ATTN_BWD64 in os.environ: make the library re-read them (it caches the
    switches at its first attention call; the production dispatch never calls getenv)."""
    load().st_env_refresh()


def _check(rc: int, what: str) -> None:
    if rc == 0:
        return
    if rc < 0:
        raise ValueError("%s: unsupported argument (code %d) - see include/st_hip.h" % (what, rc))
    raise RuntimeError("%s: HIP launch failed (hipError_t %d)" % (what, rc))


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# The kernels index these buffers by raw pointer: every property they rely on is checked here, by one of three helpers that
# RAISE (never `assert`: python -O must not remove them) - RuntimeError for a tensor that is not on the GPU, TypeError /
# ValueError for a wrong dtype / shape / layout.  Nothing is allocated or formatted on the success path.
_NO_GPU = "%s must live on the GPU: the HIP path has no CPU fallback"


def _mat(t: torch.Tensor, dtype, name: str, rows=None, cols=None, ld=None, min_rows=0) -> None:
    """A 2-D row matrix with unit column stride; optionally with exactly ``rows`` / at least ``min_rows`` rows, exactly
    ``cols`` columns and the leading dimension ``ld``."""
    if not t.is_cuda:
        raise RuntimeError(_NO_GPU % name)
    if t.dtype != dtype:
        raise TypeError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("%s: expected a 2-D row matrix with unit column stride, got shape %s stride %s"
                         % (name, tuple(t.shape), t.stride()))
    if ((rows is not None and t.shape[0] != rows) or t.shape[0] < min_rows or (cols is not None and t.shape[1] != cols)
            or (ld is not None and t.stride(0) != ld)):
        raise ValueError("%s: shape %s stride %s, expected rows %s (at least %d), columns %s, leading dimension %s (None = any)"
                         % (name, tuple(t.shape), t.stride(), rows, min_rows, cols, ld))


def _vec(t: Optional[torch.Tensor], dtype, n: int, name: str) -> None:
    """None, or a contiguous buffer of at least ``n`` elements read as a flat vector."""
    if t is None or (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() >= n):
        return
    if not t.is_cuda:
        raise RuntimeError(_NO_GPU % name)
    raise ValueError("%s: expected contiguous %s[>= %d], got %s %s stride %s" % (name, dtype, n, t.dtype, tuple(t.shape), t.stride()))


def _dev(t: torch.Tensor, dtype, shape, name: str) -> int:
    """A contiguous tensor of exactly ``shape`` (an extent of None: any) -> its address."""
    if t is not None and t.is_cuda and t.dtype == dtype and t.is_contiguous() and (
            t.shape == shape or (t.dim() == len(shape) and all(w is None or w == n for w, n in zip(shape, t.shape)))):
        return t.data_ptr()
    if t is not None and not t.is_cuda:
        raise RuntimeError(_NO_GPU % name)
    raise ValueError("%s: expected a contiguous %s %s tensor (None = any extent), got %s" % (
        name, dtype, list(shape), None if t is None else (t.dtype, tuple(t.shape), t.stride())))


# ---- groups of checks that several wrappers share ---------------------------------------------------------------------------------
def _offsets(q_off, q_len, k_off, k_len) -> int:
    """The four int32 [B] offset / length vectors of a ragged attention problem -> B."""
    B = q_off.numel()
    _vec(q_off, I32, B, "q_off"), _vec(q_len, I32, B, "q_len"), _vec(k_off, I32, B, "k_off"), _vec(k_len, I32, B, "k_len")
    return B


def _ores(ores, O, name="ores") -> None:
    """``ores`` (optional: what rounding O to bf16 dropped) has its output's shape and stride."""
    if ores is not None:
        _mat(ores, BF16, name, rows=O.shape[0], cols=O.shape[1], ld=O.stride(0))


def _chain_pre_q(M, d, pre, bq, Qout) -> None:
    """The PRE stage + query projection that attn_f1_fwd / attn_sf1_fwd run in front of the attention (row_chain's ``pre``)."""
    R, bo, g0, be0, out0, xhat0, rstd0 = pre
    _mat(R, BF16, "R", min_rows=M), _mat(out0, BF16, "out0", ld=d), _mat(Qout, BF16, "Qout", rows=M, cols=d)
    if xhat0 is not None:
        _mat(xhat0, BF16, "xhat0", ld=d)
    _vec(bo, F32, d, "bo"), _vec(g0, F32, d, "g0"), _vec(be0, F32, d, "be0"), _vec(bq, F32, d, "bq"), _vec(rstd0, F32, M, "rstd0")


def _two_block_stream(chain, who) -> None:
    if chain.stream.numel() != 8 * (2 * 16 + wfrag_depth()) * 512 or chain.stream.dtype != BF16:
        raise ValueError("%s: the fragment stream does not match a two-block chain" % who)


def _embed_next(embed, n):
    """beam_advance's ``embed`` = (emb f32 [V', D], pe f32 [P, D], x_next bf16 [n, D]), all contiguous -> the six arguments
    (emb, V', pe, P, x_next, D) of the C entry points; None -> the launch writes no decoder input."""
    if embed is None:
        return None, 0, None, 0, None, 0
    emb, pe, x_next = embed
    D = emb.shape[-1]
    return (_dev(emb, F32, (emb.shape[0], D), "embed: emb"), emb.shape[0], _dev(pe, F32, (pe.shape[0], D), "embed: pe"), pe.shape[0],
            _dev(x_next, BF16, (n, D), "embed: x_next"), D)


BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64


class Drop:
    """One dropout call site (nn.Dropout in training mode): ``seed`` is a 1-element int32 DEVICE tensor (the
    kernels read it, so a captured HIP graph draws new masks once it is advanced), ``salt`` a per-site
    constant, ``p`` the drop probability - quantised to 8 bits: keep iff draw >= round(256 p), survivors scaled
    by 256 / (256 - thresh).  The backward of an op takes the same Drop object as its forward."""
    __slots__ = ("seed", "salt", "thresh", "scale")

    def __init__(self, seed: torch.Tensor, salt: int, p: float):
        if not (seed.is_cuda and seed.dtype == torch.int32 and seed.numel() == 1):
            raise ValueError("Drop: seed must be a 1-element int32 tensor on the GPU")
        if not 0.0 <= p < 1.0:
            raise ValueError("Drop: p must be in [0, 1)")
        self.seed, self.salt = seed, int(salt) & 0xFFFFFFFF
        self.thresh = min(255, int(round(256.0 * p)))
        self.scale = 256.0 / (256 - self.thresh)

    @property
    def p_effective(self) -> float:
        return self.thresh / 256.0


def _drop(d: Optional["Drop"]):
    if d is None or d.thresh == 0:
        return None, 0, 0, 1.0
    return d.seed.data_ptr(), d.salt, d.thresh, d.scale


# ------------------------------------------------------------------------------------------------
def gemm(X, Y, out, bias=None, aux=None, epi=EPI_BF16, x_cmajor=False, y_cmajor=False, splits=1,
         m=None, n=None, kc=None, drop=None, delta=None, head_dim=0, stack=None, aux2=None):
    """out[i][j] (+)= sum_c X(i,c) Y(j,c).  ``*_cmajor``: that tensor is stored [c, rows].
    ``stack = (blocks, stride, bias_stride)``: Y (and bias) is the FIRST of ``blocks`` equally shaped blocks lying
    ``stride`` (``bias_stride``) elements apart - the same weight of consecutive identical layers in the parameter
    arena; the operand is their vertical stack (more output columns forward, a longer contraction for dgrad).
    EPI_BF16_DELTA: additionally delta[h][i] = sum over head h's ``head_dim`` columns of out(i, .) * (aux + aux2)(i, .)
    (fp32 [N / head_dim, M]) - the attention backward's rowsum(dO * O), produced by the GEMM that produces dO;
    ``aux2`` (optional) = attn_fwd's ``ores``, the part of O its bf16 rounding dropped."""
    _mat(X, BF16, "X"), _mat(Y, BF16, "Y")
    _mat(out, F32 if epi in (EPI_F32, EPI_F32_ATOMIC, EPI_F32_ATOMIC_T) else BF16, "out")
    M = m if m is not None else (X.shape[1] if x_cmajor else X.shape[0])
    N = n if n is not None else (Y.shape[1] if y_cmajor else Y.shape[0])
    Kc = kc if kc is not None else (X.shape[0] if x_cmajor else X.shape[1])
    blocks, block_rows, y_stride, b_stride = 1, 0, 0, 0
    if stack is not None:
        blocks, y_stride, b_stride = stack
        block_rows = Y.shape[0]
        if y_cmajor:
            Kc = blocks * block_rows
        else:
            N = blocks * block_rows
    need = (N, M) if epi == EPI_F32_ATOMIC_T else (M, N)
    if out.shape[0] < need[0] or out.shape[1] < need[1]:
        raise ValueError("gemm: out %s too small for %dx%d" % (tuple(out.shape), need[0], need[1]))
    _vec(bias, F32, N // blocks if not y_cmajor else N, "bias")
    if epi == EPI_BF16_DELTA:
        if head_dim not in (32, 64, 128) or N % head_dim:
            raise ValueError("gemm: EPI_BF16_DELTA needs head_dim in {32, 64, 128} dividing N")
        _vec(delta, F32, (N // head_dim) * M, "delta")
        bias, splits = delta, head_dim          # the C-ABI passes them in the bias / splits slots of this epilogue
    ldaux = 0
    if epi in (EPI_BF16_MASK, EPI_BF16_ADD, EPI_BF16_DELTA):
        _mat(aux, BF16, "aux")
        ldaux = aux.stride(0)
        if aux2 is not None:
            _mat(aux2, BF16, "aux2")
            if epi != EPI_BF16_DELTA or aux2.stride(0) != ldaux or aux2.shape != aux.shape:
                raise ValueError("gemm: aux2 goes with EPI_BF16_DELTA and must have aux's shape and stride")
    esz = 4 if epi in (EPI_F32, EPI_F32_ATOMIC, EPI_F32_ATOMIC_T) else 2
    _tag("gemm", int(x_cmajor), int(y_cmajor), M, N, Kc, epi,
         io=(2.0 * M * Kc, 2.0 * N * Kc, float(esz) * M * N, 2.0 * M * N if aux is not None else 0, 2.0 * M * N if aux2 is not None else 0))
    dropargs = _drop(drop) if epi in (EPI_BF16_RELU, EPI_BF16_MASK) else _drop(None)
    if stack is None:
        rc = load().st_gemm(_stream(), int(x_cmajor), int(y_cmajor), X.data_ptr(), X.stride(0), Y.data_ptr(),
                            Y.stride(0), out.data_ptr(), out.stride(0), M, N, Kc, _p(bias), _p(aux), ldaux, epi, splits,
                            *dropargs, _p(aux2))
    else:
        rc = load().st_gemm_stacked(_stream(), int(x_cmajor), int(y_cmajor), X.data_ptr(), X.stride(0), Y.data_ptr(),
                                    Y.stride(0), out.data_ptr(), out.stride(0), M, N, Kc, _p(bias), _p(aux), ldaux,
                                    epi, splits, *dropargs, block_rows, y_stride, b_stride)
    _check(rc, "st_gemm")
    return out


def gemm_ws(X, W, out, bias=None, relu=False, drop=None, stack=None):
    """out = act(X W^T + bias) through the weight-stationary streaming kernel (K = 256, N % 256 == 0); stack as in gemm()."""
    _mat(X, BF16, "X"), _mat(W, BF16, "W"), _mat(out, BF16, "out")
    M, K = X.shape
    N = W.shape[0]
    blocks, block_rows, w_stride, b_stride = 1, 0, 0, 0
    if stack is not None:
        blocks, w_stride, b_stride = stack
        block_rows = W.shape[0]
        N = blocks * block_rows
    if out.shape[0] < M or out.shape[1] < N:
        raise ValueError("gemm_ws: out %s too small for %dx%d" % (tuple(out.shape), M, N))
    _vec(bias, F32, N // blocks, "bias")
    _tag("gemm", 0, 0, M, N, K, EPI_BF16_RELU if relu else EPI_BF16, io=(2.0 * M * K, 2.0 * N * K, 2.0 * M * N))
    rc = load().st_gemm_ws(_stream(), X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(), out.stride(0),
                           M, N, K, _p(bias), int(relu), *(_drop(drop) if relu else _drop(None)), block_rows, w_stride, b_stride)
    _check(rc, "st_gemm_ws")
    return out


def gemm_kscale(X, W, out, bias, col_lo, col_hi, scale):
    """out = X W^T + bias with columns [col_lo, col_hi) scaled by `scale` in fp32 before the rounding (st_gemm_kscale): a
    q | k | v projection whose key block leaves pre-scaled (attn_fwd's k_prescaled)."""
    _mat(X, BF16, "X"), _mat(W, BF16, "W"), _mat(out, BF16, "out")
    M, K = X.shape
    N = W.shape[0]
    _vec(bias, F32, N, "bias")
    _tag("gemm", 0, 0, M, N, K, EPI_BF16, io=(2.0 * M * K, 2.0 * N * K, 2.0 * M * N, 0, 0))
    _check(load().st_gemm_kscale(_stream(), X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(), out.stride(0),
                                 M, N, K, _p(bias), int(col_lo), int(col_hi), float(scale)), "st_gemm_kscale")
    return out


def ws_ok(M, N, K):
    """Shapes the weight-stationary kernel takes, and where it pays (measured on MI355X, tools/dev/ws_bench.py: 1.2-1.4x
    over the tiled kernel from ~16 k rows up, on par at 7 k, so only encoder-sized row counts are routed to it)."""
    return K == 256 and N % 256 == 0 and M >= 12288


def wgrad_group(problems, wide=False):
    """One launch for several weight gradients.  problems: iterable of (X [tokens, K_in] bf16, dY [tokens, N_out]
    bf16, gW f32 [>= N_out, K_in], gB f32 [N_out] or None, splits, N_out) - the argument tuple of
    ``functional.wgrad``; each is gW[n][k] += sum_m dY[m][n] X[m][k] (and gB[n] += sum_m dY[m][n]).
    wide: the 256 x 256-tile kernel for encoder-sized token counts (st_wgrad_wide) instead of the 128 x 128 one."""
    problems = list(problems)
    n = len(problems)
    if n == 0:
        return
    PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
    X, dY, dW, dB = PA(), PA(), PA(), PA()
    ldx, lddy, lddw, tokens, k_in, n_out, splits = IA(), IA(), IA(), IA(), IA(), IA(), IA()
    for q, (x, dy, gw, gb, sp, rows) in enumerate(problems):
        _mat(x, BF16, "X"), _mat(dy, BF16, "dY"), _mat(gw, F32, "gW")
        if x.shape[0] != dy.shape[0] or gw.shape[0] < rows or gw.shape[1] < x.shape[1]:
            raise ValueError("wgrad_group: problem %d has inconsistent shapes" % q)
        _vec(gb, F32, rows, "gB")
        X[q], dY[q], dW[q], dB[q] = x.data_ptr(), dy.data_ptr(), gw.data_ptr(), _p(gb)
        ldx[q], lddy[q], lddw[q] = x.stride(0), dy.stride(0), gw.stride(0)
        tokens[q], k_in[q], n_out[q], splits[q] = x.shape[0], x.shape[1], rows, sp
    name = "st_wgrad_wide" if wide else "st_wgrad_group"
    _tag(name[3:], n, sum(2.0 * pr[0].shape[0] * pr[0].shape[1] * pr[5] for pr in problems),
         io=[2.0 * pr[0].shape[0] * (pr[0].shape[1] + pr[5]) + 8.0 * pr[5] * pr[0].shape[1] for pr in problems])   # X, dY in; gW read + written (fp32)
    rc = getattr(load(), name)(_stream(), n, X, ldx, dY, lddy, dW, lddw, dB, tokens, k_in, n_out, splits)
    _check(rc, name)


def gemm_ln(X, W, bias, res, gamma, beta, out, xhat, rstd, eps=1e-6, relu=False, pe=None, pos=None, pre=None,
            drop=None, drop_where=0):
    """drop_where: 1 = dropout before the LayerNorm (after bias / ReLU), 2 = on the LayerNorm output."""
    _mat(X, BF16, "X"), _mat(W, BF16, "W"), _mat(out, BF16, "out")
    M, K = X.shape
    N = W.shape[0]
    if W.stride(0) != K or W.shape[1] != K:
        raise ValueError("gemm_ln: W must be a contiguous [N, K] matrix")
    _vec(bias, F32, N, "bias"), _vec(gamma, F32, N, "gamma"), _vec(beta, F32, N, "beta")
    if res is not None:
        _mat(res, BF16, "res")
    if xhat is not None:
        _mat(xhat, BF16, "xhat", ld=N)
    if pre is not None:
        _mat(pre, BF16, "pre", ld=N)
    _vec(rstd, F32, M, "rstd")
    if pe is not None:
        _mat(pe, F32, "pe", ld=N)
        _vec(pos, I32, M, "pos")
    _tag("gemm_ln", M, N, K, io=((X, M), W, (res, M), (out, M), (xhat, M), (pre, M), (rstd, M)))
    rc = load().st_gemm_ln(_stream(), X.data_ptr(), X.stride(0), W.data_ptr(), M, N, K, bias.data_ptr(), _p(res),
                           0 if res is None else res.stride(0), gamma.data_ptr(), beta.data_ptr(), float(eps),
                           int(relu), _p(pe), _p(pos), out.data_ptr(), out.stride(0), _p(xhat), _p(rstd), _p(pre),
                           *_drop(drop if drop_where in (1, 2) else None), int(drop_where))
    _check(rc, "st_gemm_ln")
    return out


_WFRAG_DEPTH = None


def wfrag_depth() -> int:
    """Padding fragments at the end of every wave stream (the chain kernel prefetches this far ahead)."""
    global _WFRAG_DEPTH
    if _WFRAG_DEPTH is None:
        _WFRAG_DEPTH = load().st_wfrag_depth()
    return _WFRAG_DEPTH


def wfrag_build(table):
    """(Re)build weight-fragment streams (csrc/st_rowchain.hip): ``table`` int64 [n_blocks, 4] on the device, one row per
    256 x 256 weight block: (address of its first element, leading dimension | transposed << 32, fragment index inside a
    wave stream | wave stride in fragments << 32, address of the chain's buffer) - see st_amd/chains.py."""
    _dev(table, I64, (None, 4), "wfrag_build: table")
    _tag("wfrag_build", table.shape[0], 0, 0, io=(4.0 * 256 * 256 * table.shape[0],))
    _check(load().st_wfrag_build(_stream(), table.data_ptr(), table.shape[0]), "st_wfrag_build")


K_LOG2_SCALE = 1.4426950408889634      # log2(e): a pre-scaled key projection holds scale * K_LOG2_SCALE * k (attn_fwd's k_prescaled)


def row_chain(A, chain, pre=None, ffn=None, post=None, eps=1e-6, post_kscale=0.0):
    """One launch for a chain of row-wise layers over decoder-sized row counts (csrc/st_rowchain.hip).
    ``chain``: st_amd.chains.Chain (the fragment streams of this chain's weight blocks); A [M, 256] bf16.
    pre  = (R, bo, gamma, beta, out, xhat, rstd):                 cur = LN(A Wo^T + bo + R)
    ffn  = (d_ff, b1, b2, gamma, beta, H, out, xhat, rstd, drop1, drop2[, relu_bits]): cur = drop2(LN(drop1(relu(cur W1^T + b1)) W2^T + b2 + cur));
           H (the hidden activation, the weight gradient's operand) may be None when no backward follows
           relu_bits (int64 [chain_mask_words(M, d_ff)]) receives the H > 0 mask row_chain_bwd reads
    post = (n_blocks_out, bias, P):                               P = cur Wp^T + bias, Wp [256 n_blocks_out, 256]
    post_kscale (n_blocks_out == 3 only; 0 = plain): the KEY block of a q | k | v projection leaves multiplied by it (in fp32,
    before its one rounding) - scale * K_LOG2_SCALE for attention kernels called with k_prescaled=True.
    xhat / rstd may be None when no backward follows."""
    _mat(A, BF16, "A")
    M, d = A.shape
    if d not in (256, 512):
        raise ValueError("row_chain: d_model 256 or 512")
    wfrag, n_blocks = chain.stream, chain.n_blocks
    if d == 512:      # csrc/st_rowchain_pipe512.cuh: PRE + FFN [+ a q | k | v projection], 256 x 256 blocks of 512-wide matrices
        if not (pre and ffn) or (post and post[0] != 6):
            raise ValueError("row_chain (d_model 512): PRE and FFN are required, POST is a 1,536-column projection (6 blocks)")
        nb = 4 + 4 * (ffn[0] // 256) + (12 if post else 0)
    else:
        nb = (1 if pre else 0) + (2 * (ffn[0] // 256) if ffn else 0) + (post[0] if post else 0)
    if nb != n_blocks or wfrag.numel() != 8 * (n_blocks * 16 + wfrag_depth()) * 512 or wfrag.dtype != BF16:
        raise ValueError("row_chain: the fragment stream does not match the chain")
    z = (None,) * 11
    R, bo, g0, be0, out0, xhat0, rstd0 = pre if pre else z[:7]
    relu_bits = None
    if ffn and len(ffn) == 12:        # (.., relu_bits): int64 [chain_mask_words(M, d_ff)] for row_chain_bwd
        relu_bits, ffn = ffn[11], ffn[:11]
    d_ff, b1, b2, g1, be1, H, out1, xhat1, rstd1, drop1, drop2 = ffn if ffn else (0,) + z[:10]
    pb, bp, P = post if post else (0, None, None)
    if pre:
        _mat(R, BF16, "R", min_rows=M), _vec(bo, F32, d, "bo"), _vec(g0, F32, d, "g0"), _vec(be0, F32, d, "be0")
        if out0 is not None:       # (None: the sublayer's output is only the chain's own running activation - inference)
            _mat(out0, BF16, "out0", ld=d)
        if xhat0 is not None:
            _mat(xhat0, BF16, "xhat0", ld=d)
        _vec(rstd0, F32, M, "rstd0")
    if ffn:
        _mat(out1, BF16, "out1", ld=d), _vec(b1, F32, d_ff, "b1"), _vec(b2, F32, d, "b2")
        _vec(g1, F32, d, "g1"), _vec(be1, F32, d, "be1")
        if H is not None:          # (None: inference - the hidden activation stays on the chip)
            _mat(H, BF16, "H", rows=M, cols=d_ff, ld=d_ff)
        if xhat1 is not None:
            _mat(xhat1, BF16, "xhat1", ld=d)
        _vec(rstd1, F32, M, "rstd1")
        if relu_bits is not None:
            _vec(relu_bits, I64, chain_mask_words(M, d_ff, d), "relu_bits")
    if post:
        _mat(P, BF16, "P", rows=M, cols=256 * pb), _vec(bp, F32, 256 * pb, "bp")
    seed = None
    for dr in (drop1, drop2):
        if dr is not None and dr.thresh:
            if seed is not None and seed.data_ptr() != dr.seed.data_ptr():
                raise ValueError("row_chain: both dropout sites must read the same device seed")
            seed = dr.seed
    s1, s2 = _drop(drop1), _drop(drop2)
    work = getattr(chain, "split_work", None) if ffn else None
    _vec(work, I32, 0, "chain.split_work")
    _tag("row_chain", M, n_blocks, d_ff, io=((A, M), (R, M), (out0, M), (xhat0, M), (H, M), relu_bits, (out1, M), (xhat1, M), (P, M),
                                             (rstd0, M), (rstd1, M), 2.0 * 256 * 256 * n_blocks))
    if d == 512:
        rc = load().st_row_chain512(_stream(), M, wfrag.data_ptr(), n_blocks, int(chain.next_blocks), float(eps), A.data_ptr(), A.stride(0),
                                    _p(R), R.stride(0), _p(bo), _p(g0), _p(be0), _p(out0), _p(xhat0), _p(rstd0), int(d_ff), _p(b1), _p(b2),
                                    _p(g1), _p(be1), _p(H), _p(relu_bits), _p(out1), _p(xhat1), _p(rstd1), _p(seed), s1[1], s1[2], s1[3],
                                    s2[1], s2[2], s2[3], int(pb), _p(bp), _p(P), 0 if P is None else P.stride(0), float(post_kscale))
        _check(rc, "st_row_chain512")
        return
    rc = load().st_row_chain(_stream(), M, wfrag.data_ptr(), n_blocks, int(chain.next_blocks), float(eps), A.data_ptr(), A.stride(0), _p(R),
                             0 if R is None else R.stride(0), _p(bo), _p(g0), _p(be0), _p(out0), _p(xhat0), _p(rstd0),
                             int(d_ff), _p(b1), _p(b2), _p(g1), _p(be1), _p(H), _p(relu_bits), _p(out1), _p(xhat1), _p(rstd1), _p(seed),
                             s1[1], s1[2], s1[3], s2[1], s2[2], s2[3], int(pb), _p(bp), _p(P), 0 if P is None else P.stride(0),
                             _p(work), 0 if work is None else work.numel() * work.element_size(), float(post_kscale))
    _check(rc, "st_row_chain")


def split_work_words() -> int:
    """int32 elements of the scratch a Chain may carry as ``split_work`` (zero-initialised; the kernel leaves it zeroed where
    it matters): the 32 x 256 fp32 partial sums of up to 256 workgroups, and one ticket per row block."""
    return 256 * 512 * 16 + 256          # 256 workgroups' partials (the launch never uses more) + tickets


_splitk_work = {}          # device -> the split-K scratch in use
_ATTN_SPLIT_WORK = {}      # device index -> the attention backward's key-split scratch in use
_SUPERSEDED = []           # every buffer a larger one has replaced: referenced for the life of the process (see _scratch)
_SPLITK_BYTES = 4096 + 256 * 65536


def _scratch(in_use: dict, key, device, nbytes: int):
    """Process-wide zero-initialised int32 scratch (tickets + fp32 partials of a last-arriver merge; the kernels leave the
    tickets zero, launches are stream-ordered, so every launch of one purpose on a device may share it).  -> ``in_use[key]`` if
    it is large enough; else a larger one takes its place and the old one moves to _SUPERSEDED - it is never freed, because a
    captured graph may have its address baked into a node.  -> None when the buffer would have to be created inside a
    stream capture: a tensor born there belongs to that graph's private pool and must never become the process-wide one -
    the caller decides (splitk_scratch raises, attn_bwd takes a buffer for that one call)."""
    work = in_use.get(key)
    if work is None or work.numel() * 4 < nbytes:
        if torch.cuda.is_current_stream_capturing():
            return None
        if work is not None:
            _SUPERSEDED.append(work)
        work = in_use[key] = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)
    return work


def splitk_scratch(device):
    """The per-device scratch of st_gemm_splitk (tickets + 256 fp32 tile partials), zeroed once; the kernel restores its
    tickets.  TrainStep creates it before a capture."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    work = _scratch(_splitk_work, device, device, _SPLITK_BYTES)
    if work is None:
        raise RuntimeError("splitk_scratch: first use inside a stream capture; call st_amd.native.splitk_scratch(device) before it")
    return work


def gemm_splitk(X, Y, out, splits, y_cmajor=False):
    """out (bf16 [M, N]) = X Y^T with the contraction cut ``splits`` ways over workgroups and merged by the last one to finish
    each output tile (st_gemm_splitk: few output tiles, long contraction).  Y: [N, Kc], or [Kc, N] with y_cmajor."""
    _mat(X, BF16, "X"), _mat(Y, BF16, "Y"), _mat(out, BF16, "out")
    M, Kc = X.shape
    N = Y.shape[1] if y_cmajor else Y.shape[0]
    if (Y.shape[0] if y_cmajor else Y.shape[1]) != Kc or tuple(out.shape) != (M, N):
        raise ValueError("gemm_splitk: shapes")
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles * int(splits) > 256:
        raise ValueError("gemm_splitk: at most 256 (output tile, split) pairs")
    # ONE scratch per device, sized for the largest launch (16.8 MB): a size that followed the shape would be allocated anew -
    # possibly inside a graph capture, from the graph's private pool - whenever a batch brings another row count
    need = _SPLITK_BYTES
    work = splitk_scratch(X.device)
    _tag("gemm", 0, int(y_cmajor), M, N, Kc, 0, io=(X, Y, out, 2.0 * tiles * int(splits) * 65536))
    _check(load().st_gemm_splitk(_stream(), int(y_cmajor), X.data_ptr(), X.stride(0), Y.data_ptr(), Y.stride(0), out.data_ptr(),
                                 out.stride(0), M, N, Kc, int(splits), work.data_ptr(), need), "st_gemm_splitk")
    return out


def chain_mask_words(M: int, d_ff: int, d_model: int = 256) -> int:
    """int64 words of the ReLU-mask buffer a feed-forward row chain over M rows writes (row_chain) and reads (row_chain_bwd)."""
    if d_model == 512:
        return int(load()._cdll.st_row_chain512_mask_words(int(M), int(d_ff)))
    return int(load()._cdll.st_row_chain_mask_words(int(M), int(d_ff)))     # host-only: not a launch (bypasses the per-launch timer)


def relu_bits_from(H, d_model: int = 256):
    """The relu_bits buffer of a hidden activation H [M, d_ff] that did NOT come out of row_chain (a separate forward, a
    test): word ((workgroup * d_ff/256 + chunk) * 8 + wave) * 64 + lane, bit 16 mt + 4 g + e  <->  row
    workgroup * 32 MT + 32 mt + (lane & 31), column 256 chunk + 32 wave + 8 g + 4 (lane >> 5) + e - the accumulator layout
    of csrc/st_rowchain.hip (MT row tiles per workgroup as st_row_chain picks them for M)."""
    M, d_ff = H.shape
    words = chain_mask_words(M, d_ff, d_model)
    nc = d_ff // 256
    n_wg = words // (nc * 512)
    mt_n = -(-M // (32 * n_wg))                       # rows per workgroup / 32
    rows = n_wg * 32 * mt_n
    pos = torch.zeros(rows, d_ff, dtype=torch.int64, device=H.device)
    pos[:M] = (H.float() > 0).to(torch.int64)
    # [wg, mt, r, ch, wave, g, hi, e] -> [wg, ch, wave, hi, r, mt, g, e]
    v = pos.view(n_wg, mt_n, 32, nc, 8, 4, 2, 4).permute(0, 3, 4, 6, 2, 1, 5, 7).reshape(n_wg * nc * 8 * 64, mt_n * 16)
    shifts = torch.arange(mt_n * 16, device=H.device, dtype=torch.int64)
    return (v << shifts).sum(1).contiguous()


def row_chain_bwd(chain, M, head=None, ds_in=None, ffn=None, tail=None):
    """One launch for the backward of a row chain (csrc/st_rowchain.hip; ``chain`` holds the TRANSPOSED weight blocks in
    the order HEAD | FFN | TAIL).
    head = (n_blocks, dP, G, xhat, rstd, gamma, drop, ds_out, dgamma, dbeta, dbias):
           dy = dP Wp + G;  ds_out = LayerNorm-backward(dropout-backward(dy)); column sums accumulated atomically
           (n_blocks = 0, dP = None: dy = G - the bare LayerNorm backward of a gradient arriving from outside the stack)
    ds_in: without head, the running gradient [M, 256] the chain starts from
    ffn  = (d_ff, relu_bits, mask_scale, dH, xhat, rstd, gamma, ds_out, dgamma, dbeta, dbias):
           dH = (ds W2) masked by H > 0 (the bits the forward chain wrote), scaled;  ds_out = LayerNorm-backward(dH W1 + ds)
    tail = (O, Ores, dctx, delta): dctx = ds Wo, delta[h][i] = sum over head h (64 columns) of dctx (O + Ores)"""
    z = (None,) * 11
    nb, dP, G, xa, ra, ga, drop, dsa, dga, dba, dbia = head if head else (0,) + z[:10]
    d_ff, bits, msc, dH, xb, rb, gb, dsb, dgb, dbb, dbib = ffn if ffn else (0, None, 1.0) + z[:8]
    O, Ores, dctx, delta = tail if tail else z[:4]
    if any(t is not None and t.dim() == 2 and t.shape[1] == 512 for t in (G, xa, ds_in, xb, O)):
        raise ValueError("row_chain_bwd: the backward chain exists at width 256 only (d_model 512 takes the per-GEMM kernels)")
    n_blocks = nb + (2 * (d_ff // 256) if ffn else 0) + (1 if tail else 0)
    if n_blocks != chain.n_blocks or chain.stream.numel() != 8 * (n_blocks * 16 + wfrag_depth()) * 512:
        raise ValueError("row_chain_bwd: the fragment stream does not match the chain")
    for t, cols, ld, name in ((dP, 256 * nb, None, "dP"), (G, 256, None, "G"), (xa, 256, 256, "xhat_a"), (dsa, 256, 256, "ds_a"),
                              (ds_in, 256, 256, "ds_in"), (dH, d_ff, d_ff, "dH"), (xb, 256, 256, "xhat_b"), (dsb, 256, 256, "ds_b"),
                              (O, 256, None, "O"), (Ores, 256, None if O is None else O.stride(0), "Ores"), (dctx, 256, None, "dctx")):
        if t is not None:
            _mat(t, BF16, name, min_rows=M, cols=cols, ld=ld)
    if ffn:
        if bits is None:
            raise ValueError("row_chain_bwd: relu_bits must be the int64 buffer the forward chain wrote (chain_mask_words(M, d_ff) words)")
        _vec(bits, I64, chain_mask_words(M, d_ff), "relu_bits")
    for v, n, name in ((ra, M, "rstd_a"), (ga, 256, "gamma_a"), (dga, 256, "dgamma_a"), (dba, 256, "dbeta_a"), (dbia, 256, "dbias_a"),
                       (rb, M, "rstd_b"), (gb, 256, "gamma_b"), (dgb, 256, "dgamma_b"), (dbb, 256, "dbeta_b"), (dbib, 256, "dbias_b"),
                       (delta, 4 * M, "delta")):
        _vec(v, F32, n, name)
    if head is None and ds_in is None:
        raise ValueError("row_chain_bwd: without head the chain needs ds_in")
    sd = _drop(drop)
    work = getattr(chain, "split_work", None) if ffn else None
    _vec(work, I32, 0, "chain.split_work")
    _tag("row_chain_bwd", M, n_blocks, d_ff, io=((dP, M), (G, M), (xa, M), (dsa, M), (ds_in, M), bits, (dH, M), (xb, M), (dsb, M), (O, M),
                                                 (Ores, M), (dctx, M), (delta, 4 * M), (ra, M), (rb, M), 2.0 * 256 * 256 * n_blocks))
    # encoder-sized HEAD + FFN + TAIL launches leave their LayerNorm column sums in a per-workgroup workspace (no atomics: 251 workgroups
    # adding to the same 768 floats queue for ~8 us per launch); st_colsum_fold adds it to the gradients - at once, or with the deferred
    # weight gradients (flush_colsum_folds)
    ws_rows = load()._cdll.st_row_chain_bwd_colsum_rows(int(M), int(head is not None), int(d_ff), int(tail is not None))
    cws = torch.empty(ws_rows * 1536, dtype=F32, device=chain.stream.device) if ws_rows > 0 else None
    rc = load().st_row_chain_bwd(
        _stream(), M, chain.stream.data_ptr(), n_blocks, int(chain.next_blocks), int(nb), _p(dP), 0 if dP is None else dP.stride(0),
        _p(G), 0 if G is None else G.stride(0), _p(xa), _p(ra), _p(ga), sd[0], sd[1], sd[2], sd[3], _p(dsa), _p(dga), _p(dba),
        _p(dbia), _p(ds_in), int(d_ff), _p(bits), float(msc), _p(dH), _p(xb), _p(rb), _p(gb), _p(dsb), _p(dgb), _p(dbb), _p(dbib),
        _p(O), _p(Ores), 0 if O is None else O.stride(0), _p(dctx), 0 if dctx is None else dctx.stride(0), _p(delta),
        _p(work), 0 if work is None else work.numel() * work.element_size(), _p(cws), 0 if cws is None else cws.numel() * 4)
    _check(rc, "st_row_chain_bwd")
    if cws is not None:
        _fold_pending.append((cws, ws_rows, (dga, dba, dbia, dgb, dbb, dbib)))
        if not fold_deferred:
            flush_colsum_folds()


_fold_pending = []        # (workspace, rows, six destination vectors) of row_chain_bwd launches whose column sums are not folded yet
fold_deferred = False     # functional.deferred_wgrads: folds wait for flush_deferred_wgrads (they feed nothing but parameter gradients)


def colsum_fold(items):
    """dst[v] += column sums over the workspace rows, for every (workspace [rows, 6, 256] fp32, rows, (6 fp32 [256] vectors or None))."""
    n = len(items)
    if n == 0:
        return
    ws = (ctypes.c_void_p * n)(*[it[0].data_ptr() for it in items])
    rows = (ctypes.c_int * n)(*[int(it[1]) for it in items])
    for it in items:
        for v in it[2]:
            _vec(v, F32, 256, "colsum_fold dst")
    dst = (ctypes.c_void_p * (6 * n))(*[_p(v) for it in items for v in it[2]])
    _tag("colsum_fold", n, 0, 0, io=tuple((it[0], it[1] * 1536) for it in items))
    _check(load().st_colsum_fold(_stream(), n, ws, rows, dst), "st_colsum_fold")


def flush_colsum_folds():
    if _fold_pending:
        items = list(_fold_pending)
        _fold_pending.clear()
        colsum_fold(items)


def gemm_lnbwd(dY, W, aux, xhat, rstd, gamma, dx, dgamma=None, dbeta=None, dbias=None, drop=None):
    """dx = LayerNorm-backward(bf16(dY W (+ aux)); xhat, rstd, gamma) in one launch; W is the nn.Linear weight
    [Kc, N] as stored (contraction-major for this product).  == gemm(dY, W, tmp, y_cmajor=True[, ADD aux]) + ln_bwd.
    drop: the forward dropped the LayerNorm output (gemm_ln drop_where = 2)."""
    _mat(dY, BF16, "dY"), _mat(W, BF16, "W"), _mat(xhat, BF16, "xhat"), _mat(dx, BF16, "dx")
    M, Kc = dY.shape
    N = W.shape[1]
    if W.shape[0] != Kc or xhat.stride(0) != N or xhat.shape[0] < M:
        raise ValueError("gemm_lnbwd: inconsistent shapes")
    if aux is not None:
        _mat(aux, BF16, "aux")
    _vec(rstd, F32, M, "rstd"), _vec(gamma, F32, N, "gamma")
    _vec(dgamma, F32, N, "dgamma"), _vec(dbeta, F32, N, "dbeta"), _vec(dbias, F32, N, "dbias")
    _tag("gemm_lnbwd", M, N, Kc, io=((dY, M), 2.0 * N * Kc, (aux, M), (xhat, M), (dx, M), (rstd, M)))
    rc = load().st_gemm_lnbwd(_stream(), dY.data_ptr(), dY.stride(0), W.data_ptr(), W.stride(0), M, N, Kc, _p(aux),
                              0 if aux is None else aux.stride(0), xhat.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                              dx.data_ptr(), dx.stride(0), _p(dgamma), _p(dbeta), _p(dbias), *_drop(drop))
    _check(rc, "st_gemm_lnbwd")
    return dx


def ln_bwd(dy, xhat, rstd, gamma, dx, dgamma=None, dbeta=None, dbias=None, mask=None, drop=None, mask_scale=1.0):
    """drop: the forward dropped the LayerNorm output; mask_scale: 1/(1-p) of a dropout between `mask`'s ReLU and the LN."""
    _mat(dy, BF16, "dy"), _mat(dx, BF16, "dx")
    M, N = dy.shape
    _mat(xhat, BF16, "xhat", ld=N)
    if mask is not None:
        _mat(mask, BF16, "mask", ld=N)
    _vec(rstd, F32, M, "rstd"), _vec(gamma, F32, N, "gamma")
    _vec(dgamma, F32, N, "dgamma"), _vec(dbeta, F32, N, "dbeta"), _vec(dbias, F32, N, "dbias")
    _tag("ln_bwd", M, N, io=((dy, M), (xhat, M), (dx, M), (mask, M), (rstd, M)))
    rc = load().st_ln_bwd(_stream(), dy.data_ptr(), dy.stride(0), xhat.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                          _p(mask), dx.data_ptr(), dx.stride(0), _p(dgamma), _p(dbeta), _p(dbias), M, N, *_drop(drop),
                          float(mask_scale))
    _check(rc, "st_ln_bwd")
    return dx


def _work(w):
    if w is None:
        return None, 0
    _vec(w, I32, w.numel(), "work")
    return w.data_ptr(), w.numel()


def attn_tile_rows(which: int, d_k: int, max_q: int, max_k: int, causal: bool) -> int:
    """Rows per work-list tile of the kernel st_attn_fwd (which = 0) / st_attn_bwd's dQ (1) and dK/dV (2) parts will
    run for a problem of this shape (host-side query, no launch)."""
    return int(load().st_attn_tile_rows(int(which), int(d_k), int(max_q), int(max_k), int(bool(causal))))


def attn_fwd(Q, K, V, O, lse, q_off, q_len, k_off, k_len, n_head, max_q, causal, scale, work=None, drop=None,
             max_k=0, ores=None, k_prescaled=False):
    """max_k (longest key sequence) only selects the kernel variant: <= 64 queries against >= 256 keys take
    the key-split path."""
    """work: optional int32 device list of (b << 16) | q_tile, heaviest first (functional.attn_work).
    ores (optional, bf16, O's shape and stride): receives bf16(O_fp32 - bf16(O_fp32)).
    k_prescaled: K holds scale * log2(e) * (key projection) (st_attn_fwd; row_chain's post_kscale) - the backward and
    attn_probs of the same sublayer must be told the same."""
    for t, nm in ((Q, "Q"), (K, "K"), (V, "V"), (O, "O")):
        _mat(t, BF16, nm)
    _ores(ores, O)
    B = _offsets(q_off, q_len, k_off, k_len)
    d_k = Q.shape[1] // n_head
    rows = Q.shape[0]
    _vec(lse, F32, n_head * rows, "lse")
    _tag("attn_fwd", n_head, d_k, int(causal), q_len, k_len, io=(Q, K, V, O, ores, lse))
    rc = load().st_attn_fwd(_stream(), Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0),
                            O.data_ptr(), O.stride(0), _p(ores), lse.data_ptr(), q_off.data_ptr(), q_len.data_ptr(),
                            k_off.data_ptr(), k_len.data_ptr(), B, n_head, d_k, int(max_q), int(max_k), rows, int(causal),
                            float(scale), *_work(work), *_drop(drop), int(bool(k_prescaled)))
    _check(rc, "st_attn_fwd")
    return O


_F1_OK = {}


def _f1_applicable(d, d_k, max_q, max_k):
    """Host-only query (not a launch: bypasses the per-launch timer), cached per shape."""
    key = (d, d_k, max_q, max_k)
    if key not in _F1_OK:
        _F1_OK[key] = bool(load()._cdll.st_attn_f1_applicable(d, d_k, max_q, max_k))
    return _F1_OK[key]


def attn_f1_fwd(A, chain, pre, post, K, V, O, lse, q_off, q_len, k_off, k_len, n_head, max_q, scale, work=None, drop=None,
                max_k=0, ores=None, eps=1e-6):
    """The decoder-encoder attention together with the chain stage in front of it, as ONE launch where the few-queries
    kernel serves the shape (d_model 256, 64-wide heads, <= 64 queries, >= 256 keys; csrc/st_attn_xs.hip), else as the two
    launches it stands for:
        row_chain(A, chain, pre=pre, post=post)        cur = LN(A Wo^T + bo + R) -> out / xhat / rstd;  q = cur Wq^T + bq -> post[2]
        attn_fwd(post[2], K, V, O, lse, ..., causal=False)
    pre = (R, bo, gamma, beta, out, xhat, rstd), post = (1, bq, Qout) exactly as row_chain takes them."""
    R, bo, g0, be0, out0, xhat0, rstd0 = pre
    pb, bq, Qout = post
    M, d = A.shape
    d_k = d // n_head
    if pb != 1 or chain.n_blocks != 2 or not _f1_applicable(int(d), int(d_k), int(max_q), int(max_k)):
        row_chain(A, chain, pre=pre, post=post, eps=eps)
        return attn_fwd(Qout, K, V, O, lse, q_off, q_len, k_off, k_len, n_head, max_q, False, scale, work=work, drop=drop,
                        max_k=max_k, ores=ores)
    for t, nm in ((A, "A"), (K, "K"), (V, "V"), (O, "O")):
        _mat(t, BF16, nm)
    _chain_pre_q(M, d, pre, bq, Qout)
    _two_block_stream(chain, "attn_f1_fwd")
    _ores(ores, O)
    B = _offsets(q_off, q_len, k_off, k_len)
    _vec(lse, F32, n_head * M, "lse")
    _tag("attn_fwd", n_head, d_k, 0, q_len, k_len, io=(A, R, out0, xhat0, rstd0, Qout, K, V, O, ores, lse))
    rc = load().st_attn_f1_fwd(_stream(), A.data_ptr(), A.stride(0), R.data_ptr(), R.stride(0), chain.stream.data_ptr(), 2,
                               int(chain.next_blocks), float(eps), bo.data_ptr(), g0.data_ptr(), be0.data_ptr(), out0.data_ptr(),
                               _p(xhat0), _p(rstd0), bq.data_ptr(), Qout.data_ptr(), Qout.stride(0), K.data_ptr(), K.stride(0),
                               V.data_ptr(), V.stride(0), O.data_ptr(), O.stride(0), _p(ores), lse.data_ptr(), q_off.data_ptr(),
                               q_len.data_ptr(), k_off.data_ptr(), k_len.data_ptr(), B, n_head, d_k, int(max_q), int(max_k), M,
                               float(scale), *_work(work), *_drop(drop))
    _check(rc, "st_attn_f1_fwd")
    return O


def attn_sf1_fwd(qkv, Os, lses, pre, post, chain, K, V, O, lse, q_off, q_len, k_off, k_len, n_head, max_q, scale, work_self=None,
                 work=None, drop_self=None, drop=None, max_k=0, ores_self=None, ores=None, eps=1e-6):
    """A decoder layer's causal self-attention, the chain stage behind it and its decoder-encoder attention as ONE launch where the
    few-queries kernel serves the shape (st_attn_sf1_fwd), else as the three launches it stands for:
        attn_fwd(q, k, v of qkv, Os, lses, ..., causal=True)                          (keys = the utterance's own target positions)
        row_chain(Os, chain, pre=pre, post=post)
        attn_fwd(post[2], K, V, O, lse, ..., causal=False)
    qkv [M, 3 d]: the layer's q | k | v projection; pre / post as attn_f1_fwd."""
    R, bo, g0, be0, out0, xhat0, rstd0 = pre
    pb, bq, Qout = post
    M, d3 = qkv.shape
    d = d3 // 3
    d_k = d // n_head
    if (pb != 1 or chain.n_blocks != 2 or n_head > 8 or not _f1_applicable(int(d), int(d_k), int(max_q), int(max_k))
            or (drop_self is not None and drop is not None and drop_self.thresh and drop.thresh
                and drop_self.seed.data_ptr() != drop.seed.data_ptr())):
        attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], Os, lses, q_off, q_len, q_off, q_len, n_head, max_q, True, scale,
                 work=work_self, drop=drop_self, max_k=max_q, ores=ores_self)
        return attn_f1_fwd(Os, chain, pre, post, K, V, O, lse, q_off, q_len, k_off, k_len, n_head, max_q, scale, work=work, drop=drop,
                           max_k=max_k, ores=ores, eps=eps)
    for t, nm in ((qkv, "qkv"), (K, "K"), (V, "V"), (O, "O")):
        _mat(t, BF16, nm)
    _mat(Os, BF16, "Os", rows=M, cols=d)
    _chain_pre_q(M, d, pre, bq, Qout)
    _two_block_stream(chain, "attn_sf1_fwd")
    _ores(ores, O), _ores(ores_self, Os, "ores_self")
    B = _offsets(q_off, q_len, k_off, k_len)
    _vec(lse, F32, n_head * M, "lse"), _vec(lses, F32, n_head * M, "lses")
    sd, cd = _drop(drop_self), _drop(drop)
    seed = sd[0] if sd[0] is not None else cd[0]
    _tag("attn_fwd", n_head, d_k, 0, q_len, k_len, io=(qkv, Os, ores_self, lses, R, out0, xhat0, rstd0, Qout, K, V, O, ores, lse))
    q_, k_, v_ = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    rc = load().st_attn_sf1_fwd(_stream(), q_.data_ptr(), k_.data_ptr(), v_.data_ptr(), qkv.stride(0), Os.data_ptr(), _p(ores_self),
                                Os.stride(0), lses.data_ptr(), sd[1], sd[2], sd[3], R.data_ptr(), R.stride(0), chain.stream.data_ptr(), 2,
                                int(chain.next_blocks), float(eps), bo.data_ptr(), g0.data_ptr(), be0.data_ptr(), out0.data_ptr(),
                                _p(xhat0), _p(rstd0), bq.data_ptr(), Qout.data_ptr(), Qout.stride(0), K.data_ptr(), K.stride(0),
                                V.data_ptr(), V.stride(0), O.data_ptr(), O.stride(0), _p(ores), lse.data_ptr(), q_off.data_ptr(),
                                q_len.data_ptr(), k_off.data_ptr(), k_len.data_ptr(), B, n_head, d_k, int(max_q), int(max_k), M,
                                float(scale), *_work(work), seed, cd[1], cd[2], cd[3])
    _check(rc, "st_attn_sf1_fwd")
    return O


def attn_bwd(Q, K, V, O, dO, lse, delta, dQ, dK, dV, q_off, q_len, k_off, k_len, n_head, max_q, max_k, causal, scale,
             parts=3, work_q=None, work_k=None, drop=None, k_prescaled=False):
    """parts: 1 = dQ (+delta) kernel, 2 = dK/dV kernel (needs delta from part 1), 3 = both.
    k_prescaled: as attn_fwd; dK is the gradient of the UNSCALED key projection either way."""
    for t, nm in ((Q, "Q"), (K, "K"), (V, "V"), (dO, "dO"), (dQ, "dQ"), (dK, "dK"), (dV, "dV")):
        _mat(t, BF16, nm)
    if O is not None:      # O = None: delta is an INPUT (produced with dO by gemm(..., epi=EPI_BF16_DELTA)); one launch
        _mat(O, BF16, "O")
    B = _offsets(q_off, q_len, k_off, k_len)
    d_k = Q.shape[1] // n_head
    rows = Q.shape[0]
    _vec(lse, F32, n_head * rows, "lse"), _vec(delta, F32, n_head * rows, "delta")
    if _TIMING is not None and parts == 3 and O is not None:   # profile the two kernels of the call separately
        for part in (1, 2):
            attn_bwd(Q, K, V, O, dO, lse, delta, dQ, dK, dV, q_off, q_len, k_off, k_len, n_head, max_q, max_k, causal,
                     scale, parts=part, work_q=work_q, work_k=work_k, drop=drop, k_prescaled=k_prescaled)
        return
    # few queries against many keys (the decoder-encoder attention): scratch for the dQ items' key split across workgroups
    kib = load()._cdll.st_attn_bwd_split_kib(B, n_head, d_k, int(max_q), int(max_k), int(causal)) if (parts == 3 and O is None) else 0
    swork = _scratch(_ATTN_SPLIT_WORK, Q.device.index, Q.device, kib * 1024) if kib > 0 else None
    if kib > 0 and swork is None:      # first use of this size inside a capture: the call's own buffer, from the capturing graph's
        swork = torch.zeros(kib * 256, dtype=torch.int32, device=Q.device)      # pool, its zero-fill a node of the graph; NOT kept
    _tag("attn_bwd", n_head, d_k, int(causal), q_len, k_len, parts, io=(Q, K, V, O, dO, dQ, dK, dV, lse, delta))
    rc = load().st_attn_bwd(_stream(), Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0),
                            _p(O), 0 if O is None else O.stride(0), dO.data_ptr(), dO.stride(0), lse.data_ptr(),
                            delta.data_ptr(),
                            dQ.data_ptr(), dQ.stride(0), dK.data_ptr(), dK.stride(0), dV.data_ptr(), dV.stride(0),
                            q_off.data_ptr(), q_len.data_ptr(), k_off.data_ptr(), k_len.data_ptr(), B, n_head, d_k,
                            int(max_q), int(max_k), rows, int(causal), float(scale), int(parts), *_work(work_q),
                            *_work(work_k), *_drop(drop), int(bool(k_prescaled)), _p(swork),
                            0 if swork is None else swork.numel() * 4)
    _check(rc, "st_attn_bwd")


def ctc_gather(logits, rowmap, T, cols, lse, lp, V=None):
    """lse[r] = logsumexp(logits[r, :V]); lp[b][t][k] = logits[row(b, t)][cols[b][k]] - lse - see st_ctc_gather."""
    _mat(logits, F32, "logits")
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    B, C = cols.shape
    _dev(rowmap, I64, (R,), "ctc_gather: rowmap"), _dev(cols, I32, (B, C), "ctc_gather: cols"), _dev(lp, F32, (B, int(T), C), "ctc_gather: lp")
    _vec(lse, F32, R, "lse")
    _tag("ctc_gather", R, V, C, io=(4.0 * R * V, 4.0 * R * C))
    _check(load().st_ctc_gather(_stream(), logits.data_ptr(), logits.stride(0), R, V, rowmap.data_ptr(), int(T), cols.data_ptr(), C,
                                lse.data_ptr(), lp.data_ptr()), "st_ctc_gather")


def ctc_dlogits(logits, lse, rowmap, T, roww, scat, gsmall, grad_out, dlogits, V=None):
    """dlogits (bf16) = grad_out * (roww[b] * softmax(logits), label columns overwritten with gsmall) - see st_ctc_dlogits."""
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    B, C = scat.shape
    _mat(dlogits, BF16, "dlogits", rows=R, ld=dlogits.shape[-1])
    if dlogits.shape[1] < V or dlogits.stride(0) % 8:
        raise ValueError("ctc_dlogits: dlogits must be a contiguous bf16 [R, >= V] matrix with a row length that is a multiple of 8")
    _dev(scat, I32, (B, C), "ctc_dlogits: scat"), _dev(gsmall, F32, (B, int(T), C), "ctc_dlogits: gsmall"), _dev(roww, F32, (B,), "ctc_dlogits: roww")
    _vec(grad_out, F32, 1, "grad_out")
    _tag("ctc_dlogits", R, V, C, io=(4.0 * R * V, 2.0 * R * dlogits.shape[1]))
    _check(load().st_ctc_dlogits(_stream(), logits.data_ptr(), logits.stride(0), R, V, lse.data_ptr(), rowmap.data_ptr(), int(T),
                                 roww.data_ptr(), scat.data_ptr(), C, gsmall.data_ptr(), grad_out.data_ptr(), dlogits.data_ptr(),
                                 dlogits.stride(0)), "st_ctc_dlogits")


# ---- CTC loss with device-resident lengths (csrc/st_ctc_loss.hip) ---------------------------------------------------------------
CTC_LOSS_MAX_L = 255      # four state pairs per lane of one wave


def ctc_loss_ws_bytes(B, T, L) -> int:
    """Bytes of the alpha / beta workspace st_ctc_loss_fwd / _grad want for lp [B, T, *] and classes [B, L] (a host-only query:
    no launch, no GPU)."""
    if L > CTC_LOSS_MAX_L or min(B, T, L) < 0:
        raise ValueError("ctc_loss: at most %d labels per utterance are supported (got L = %d)" % (CTC_LOSS_MAX_L, L))
    kib = int(load()._cdll.st_ctc_loss_ws_kib(int(B), int(T), int(L)))
    if kib < 0:
        raise ValueError("st_ctc_loss_ws_kib: unsupported shape B = %d, T = %d, L = %d" % (B, T, L))
    return kib * 1024


def _ctc_loss_args(who, lp, classes, in_len, tgt_len, ws, extra):
    """The checks of ctc_loss_fwd / ctc_loss_grad, all BEFORE any launch (and before the library is loaded): ValueError for a
    wrong dtype / shape / layout / size, RuntimeError for a tensor that is not on the GPU.  -> (B, T, C, L)"""
    if lp.dim() != 3 or lp.dtype != F32 or not lp.is_contiguous():
        raise ValueError("%s: lp must be a contiguous f32 [B, T, C] tensor, got %s %s" % (who, lp.dtype, tuple(lp.shape)))
    B, T, C = lp.shape
    if C < 2:
        raise ValueError("%s: lp needs at least two classes (blank + one label), got C = %d" % (who, C))
    if T < 1:
        raise ValueError("%s: lp has no frames" % who)
    if classes.dim() != 2 or classes.shape[0] != B or classes.dtype != I64 or not classes.is_contiguous():
        raise ValueError("%s: classes must be a contiguous i64 [B, L] tensor, got %s %s" % (who, classes.dtype, tuple(classes.shape)))
    L = classes.shape[1]
    if L > CTC_LOSS_MAX_L:
        raise ValueError("%s: at most %d labels per utterance are supported (got L = %d)" % (who, CTC_LOSS_MAX_L, L))
    for name, t in (("in_len", in_len), ("tgt_len", tgt_len)):
        if t.dtype != I32 or tuple(t.shape) != (B,) or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous i32 [B] tensor, got %s %s" % (who, name, t.dtype, tuple(t.shape)))
    for name, t, shape in extra:
        if t.dtype != F32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous f32 %s tensor, got %s %s" % (who, name, list(shape), t.dtype, tuple(t.shape)))
    if ws.dtype != torch.uint8 or ws.dim() != 1 or not ws.is_contiguous():
        raise ValueError("%s: ws must be a flat uint8 buffer (native.ctc_loss_ws_bytes)" % who)
    for name, t in [("lp", lp), ("classes", classes), ("in_len", in_len), ("tgt_len", tgt_len), ("ws", ws)] + [(n, t) for n, t, _ in extra]:
        if not t.is_cuda:
            raise RuntimeError("%s: %s must live on the GPU: the HIP path has no CPU fallback" % (who, name))
    if ws.numel() < ctc_loss_ws_bytes(B, T, L):
        raise ValueError("%s: ws holds %d bytes, %d are needed" % (who, ws.numel(), ctc_loss_ws_bytes(B, T, L)))
    return B, T, C, L


def ctc_loss_fwd(lp, classes, in_len, tgt_len, ws, nll):
    """nll f32 [B] = -log p(classes | lp), +inf where no alignment exists; alpha and beta are left in ``ws`` for ctc_loss_grad -
    see st_ctc_loss_fwd.  Lengths are DEVICE i32 tensors: nothing is read on the host (capturable)."""
    B, T, C, L = _ctc_loss_args("ctc_loss_fwd", lp, classes, in_len, tgt_len, ws, [("nll", nll, (lp.shape[0],))])
    _tag("ctc_loss_fwd", B, T, L, io=(lp, 16.0 * B * T * (L + 1)))
    _check(load().st_ctc_loss_fwd(_stream(), lp.data_ptr(), B, T, C, classes.data_ptr(), L, in_len.data_ptr(), tgt_len.data_ptr(),
                                  ws.data_ptr(), ws.numel(), nll.data_ptr()), "st_ctc_loss_fwd")
    return nll


def ctc_loss_grad(lp, classes, in_len, tgt_len, coef, ws, nll, g, roww, softmax_term=True):
    """g f32 [B, T, C] = coef[b] (exp(lp) - occ) on the frames below in_len[b], 0 past them; roww[b] = coef[b]; both 0 where
    nll[b] is infinite - see st_ctc_loss_grad (after ctc_loss_fwd on the same lp / ws).  ``softmax_term=False``: g = -coef occ, the
    derivative of coef * nll with respect to lp itself."""
    Bn = lp.shape[0] if lp.dim() == 3 else 0
    B, T, C, L = _ctc_loss_args("ctc_loss_grad", lp, classes, in_len, tgt_len, ws,
                                [("coef", coef, (Bn,)), ("nll", nll, (Bn,)), ("g", g, tuple(lp.shape)), ("roww", roww, (Bn,))])
    _tag("ctc_loss_grad", B, T, L, io=(lp, g, 16.0 * B * T * (L + 1)))
    _check(load().st_ctc_loss_grad(_stream(), lp.data_ptr(), B, T, C, classes.data_ptr(), L, in_len.data_ptr(), tgt_len.data_ptr(),
                                   coef.data_ptr(), ws.data_ptr(), ws.numel(), nll.data_ptr(), g.data_ptr(), roww.data_ptr(),
                                   1 if softmax_term else 0), "st_ctc_loss_grad")
    return g


# ---- CTC forced alignment (csrc/st_ctc_align.hip) ---------------------------------------------------------------------------------
def ctc_align_ws_bytes(B, T, L) -> int:
    """Bytes of the back-pointer workspace st_ctc_align wants for lp [B, T, *] and classes [B, L] (a host-only query: no launch,
    no GPU) - 0 while every frame count fits the kernel's LDS copy (2,048 frames for L <= 127, 1,024 above)."""
    if L > CTC_LOSS_MAX_L or min(B, T, L) < 0:
        raise ValueError("ctc_align: at most %d labels per utterance are supported (got L = %d)" % (CTC_LOSS_MAX_L, L))
    kib = int(load()._cdll.st_ctc_align_ws_kib(int(B), int(T), int(L)))
    if kib < 0:
        raise ValueError("st_ctc_align_ws_kib: unsupported shape B = %d, T = %d, L = %d" % (B, T, L))
    return kib * 1024


def ctc_align(lp, classes, in_len, tgt_len, ws, path, spans, score):
    """The Viterbi alignment of ``classes`` through lp (the inputs of ctc_loss_fwd; lengths are DEVICE i32 tensors: capturable):
    path i32 [B, T] (label position per frame, -1 = blank or past the length), spans i32 [B, L, 2] ([start, end) frames of every
    label position, (-1, -1) past tgt_len), score f32 [B] (sum of lp along the path; -inf and all -1 where no alignment exists)
    - see st_ctc_align for the recursion and its tie rule.  ws: a flat uint8 buffer of ctc_align_ws_bytes(B, T, L)."""
    who = "ctc_align"
    if lp.dim() != 3 or lp.dtype != F32 or not lp.is_contiguous():
        raise ValueError("%s: lp must be a contiguous f32 [B, T, C] tensor, got %s %s" % (who, lp.dtype, tuple(lp.shape)))
    B, T, C = lp.shape
    if C < 2:
        raise ValueError("%s: lp needs at least two classes (blank + one label), got C = %d" % (who, C))
    if T < 1:
        raise ValueError("%s: lp has no frames" % who)
    if classes.dim() != 2 or classes.shape[0] != B or classes.dtype != I64 or not classes.is_contiguous():
        raise ValueError("%s: classes must be a contiguous i64 [B, L] tensor, got %s %s" % (who, classes.dtype, tuple(classes.shape)))
    L = classes.shape[1]
    if L > CTC_LOSS_MAX_L:
        raise ValueError("%s: at most %d labels per utterance are supported (got L = %d)" % (who, CTC_LOSS_MAX_L, L))
    for name, t, dtype, shape in (("in_len", in_len, I32, (B,)), ("tgt_len", tgt_len, I32, (B,)), ("path", path, I32, (B, T)),
                                  ("spans", spans, I32, (B, L, 2)), ("score", score, F32, (B,))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s %s tensor, got %s %s" % (who, name, dtype, list(shape), t.dtype, tuple(t.shape)))
    if ws.dtype != torch.uint8 or ws.dim() != 1 or not ws.is_contiguous():
        raise ValueError("%s: ws must be a flat uint8 buffer (native.ctc_align_ws_bytes)" % who)
    need = ctc_align_ws_bytes(B, T, L)         # (a host-only query)
    if ws.numel() < need:
        raise ValueError("%s: ws holds %d bytes, %d are needed" % (who, ws.numel(), need))
    for name, t in (("lp", lp), ("classes", classes), ("in_len", in_len), ("tgt_len", tgt_len), ("ws", ws), ("path", path),
                    ("spans", spans), ("score", score)):
        if not t.is_cuda:
            raise RuntimeError("%s: %s must live on the GPU: the HIP path has no CPU fallback" % (who, name))
    if need and ws.data_ptr() % 16:
        raise ValueError("%s: ws must be 16-byte aligned" % who)
    _tag("ctc_align", B, T, L, io=(lp, path, spans))
    _check(load().st_ctc_align(_stream(), lp.data_ptr(), B, T, C, classes.data_ptr(), L, in_len.data_ptr(), tgt_len.data_ptr(),
                               ws.data_ptr(), ws.numel(), path.data_ptr(), spans.data_ptr(), score.data_ptr()), "st_ctc_align")
    return path, spans, score


# ---- CTC prefix beam search (csrc/st_ctc_beam.hip) ---------------------------------------------------------------------------------
CTC_BEAM_MAX = 16         # beam slots and classes per row of st_ctc_beam_search
TRACE_REC_BYTES = 16      # {i32 prev_slot, i32 token, f32 pb_rel, f32 pnb_rel}


def _ctc_beam_range(who, beam, L_cap, K=1):
    if not (1 <= int(beam) <= CTC_BEAM_MAX and 1 <= int(K) <= CTC_BEAM_MAX):
        raise ValueError("%s: beam and K must lie in [1, %d], got beam = %d, K = %d" % (who, CTC_BEAM_MAX, beam, K))
    if not 1 <= int(L_cap) <= CTC_LOSS_MAX_L:
        raise ValueError("%s: the label capacity must lie in [1, %d], got L_cap = %d" % (who, CTC_LOSS_MAX_L, L_cap))


def ctc_beam_ws_bytes(B, T_max, beam, L_cap) -> int:
    """Bytes of workspace st_ctc_beam_search wants (a host-only query: no launch, no GPU).  0 for every supported shape - the
    beam's label sequences live in LDS and nothing grows with the frame count; ValueError for an unsupported one."""
    if min(int(B), int(T_max)) < 0:
        raise ValueError("ctc_beam: negative B or T_max")
    _ctc_beam_range("ctc_beam", beam, L_cap)
    kib = int(load()._cdll.st_ctc_beam_ws_kib(int(B), int(T_max), int(beam), int(L_cap)))
    if kib < 0:
        raise ValueError("st_ctc_beam_ws_kib: unsupported shape B = %d, T = %d, beam = %d, L_cap = %d" % (B, T_max, beam, L_cap))
    return kib * 1024


def _ctc_beam_args(who, ids, lp, lpb, off, length, blank, tokens, lens, score, trace, trace_norm):
    """The argument checks st_ctc_beam_search and st_ctc_beam_search_lm share -> (B, R, K, beam, L_cap, T_trace)."""
    if ids.dim() != 2 or ids.dtype != I32 or not ids.is_contiguous():
        raise ValueError("%s: ids must be a contiguous i32 [R, K] tensor, got %s %s" % (who, ids.dtype, tuple(ids.shape)))
    R, K = ids.shape
    if tokens.dim() != 3 or tokens.dtype != I32 or not tokens.is_contiguous():
        raise ValueError("%s: tokens must be a contiguous i32 [B, beam, L_cap] tensor, got %s %s" % (who, tokens.dtype, tuple(tokens.shape)))
    B, beam, L_cap = tokens.shape
    _ctc_beam_range(who, beam, L_cap, K)
    if off.dim() != 1 or off.shape[0] != B:
        raise ValueError("%s: off must hold one row offset per utterance (B = %d), got %s" % (who, B, tuple(off.shape)))
    for name, t, dtype, shape in (("lp", lp, F32, (R, K)), ("lpb", lpb, F32, (R,)), ("off", off, I32, (B,)), ("length", length, I32, (B,)),
                                  ("lens", lens, I32, (B, beam)), ("score", score, F32, (B, beam))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s %s tensor, got %s %s" % (who, name, dtype, list(shape), t.dtype, tuple(t.shape)))
    if (trace is None) != (trace_norm is None):
        raise ValueError("%s: trace and trace_norm go together" % who)
    T_trace = 0
    if trace is not None:
        if trace.dim() != 4 or trace.dtype != torch.uint8 or not trace.is_contiguous() or trace.shape[0] != B or trace.shape[1] < 1 \
                or tuple(trace.shape[2:]) != (beam, TRACE_REC_BYTES):
            raise ValueError("%s: trace must be a contiguous u8 [B, T_trace >= 1, beam, %d] tensor, got %s %s"
                             % (who, TRACE_REC_BYTES, trace.dtype, tuple(trace.shape)))
        T_trace = trace.shape[1]
        if trace_norm.dtype != torch.float64 or tuple(trace_norm.shape) != (B, T_trace) or not trace_norm.is_contiguous():
            raise ValueError("%s: trace_norm must be a contiguous f64 [B, T_trace] tensor, got %s %s"
                             % (who, trace_norm.dtype, tuple(trace_norm.shape)))
    if not 0 <= int(blank):
        raise ValueError("%s: blank must be a class id, got %d" % (who, blank))
    for name, t in (("ids", ids), ("lp", lp), ("lpb", lpb), ("off", off), ("length", length), ("tokens", tokens), ("lens", lens),
                    ("score", score), ("trace", trace), ("trace_norm", trace_norm)):
        if t is not None and not t.is_cuda:
            raise RuntimeError("%s: %s must live on the GPU: the HIP path has no CPU fallback" % (who, name))
    if trace is not None and trace.data_ptr() % 16:
        raise ValueError("%s: trace must be 16-byte aligned" % who)
    return B, R, K, beam, L_cap, T_trace


def ctc_beam_search(ids, lp, lpb, off, length, blank, tokens, lens, score, trace=None, trace_norm=None):
    """CTC prefix beam search of B utterances in one launch - see st_ctc_beam_search.  ids i32 / lp f32 [R, K] (st_beam_pre_beam
    over the CTC head's logits), lpb f32 [R], off / length i32 [B] (device: capturable) -> tokens i32 [B, beam, L_cap] (-1 past a
    length), lens i32 [B, beam], score f32 [B, beam] (best first; -inf in the slots past the live prefixes).  ``trace`` u8
    [B, T_trace, beam, 16] + ``trace_norm`` f64 [B, T_trace]: the per-frame records of the beam (both or neither)."""
    B, R, K, beam, L_cap, T_trace = _ctc_beam_args("ctc_beam_search", ids, lp, lpb, off, length, blank, tokens, lens, score, trace,
                                                   trace_norm)
    _tag("ctc_beam_search", B, R, K, beam, io=(ids, lp, lpb, tokens))
    _check(load().st_ctc_beam_search(_stream(), ids.data_ptr(), lp.data_ptr(), lpb.data_ptr(), off.data_ptr(), length.data_ptr(), B, K,
                                     beam, int(blank), L_cap, tokens.data_ptr(), lens.data_ptr(), score.data_ptr(), _p(trace),
                                     _p(trace_norm), T_trace), "st_ctc_beam_search")
    return tokens, lens, score


def ctc_beam_search_lm(ids, lp, lpb, off, length, blank, tokens, lens, score, trie, bos, eos, scale, bias, fused, final_eos=True,
                       trace=None, trace_norm=None, trace_g=None):
    """``ctc_beam_search`` with the n-gram model ``trie`` (a st_amd.ngram.DeviceTrie) fused into the search - see
    st_ctc_beam_search_lm: prefixes are ranked by log p_ctc + sum over their labels of (scale lm + bias); ``final_eos``: the EOS
    term closes the rank.  fused f32 [B, beam]: the LM side of the rank (score stays the pure log p_ctc; score + fused is what the
    n-best is sorted by).  ``trace_g`` f32 [B, T_trace, beam] (only with ``trace``): g of every slot after every frame."""
    who = "ctc_beam_search_lm"
    B, R, K, beam, L_cap, T_trace = _ctc_beam_args(who, ids, lp, lpb, off, length, blank, tokens, lens, score, trace, trace_norm)
    args = _ngram_trie(trie, who)
    _dev(fused, F32, (B, beam), who + ": fused")
    if trace_g is not None:
        if trace is None:
            raise ValueError("%s: trace_g goes with trace and trace_norm" % who)
        _dev(trace_g, F32, (B, T_trace, beam), who + ": trace_g")
    scale, bias = float(scale), float(bias)
    if not 0.0 <= scale < float("inf") or not abs(bias) < float("inf"):
        raise ValueError("%s: scale must be a finite number >= 0 and bias finite, got %r, %r" % (who, scale, bias))
    _tag("ctc_beam_search_lm", B, R, K, beam, trie.order, io=(ids, lp, lpb, tokens))
    _check(load().st_ctc_beam_search_lm(_stream(), ids.data_ptr(), lp.data_ptr(), lpb.data_ptr(), off.data_ptr(), length.data_ptr(), B,
                                        K, beam, int(blank), L_cap, tokens.data_ptr(), lens.data_ptr(), score.data_ptr(), _p(trace),
                                        _p(trace_norm), T_trace, *args, int(trie.V), int(trie.order), float(trie.oov_logp), int(bos),
                                        int(eos), scale, bias, 1 if final_eos else 0, fused.data_ptr(), _p(trace_g)),
           "st_ctc_beam_search_lm")
    return tokens, lens, score, fused


# ---- n-gram language model (csrc/st_ngram.hip; st_amd/ngram.py) ----------------------------------------------------------------------
NGRAM_MAX_ORDER, NGRAM_MAX_V = 5, 5120


def _ngram_trie(trie, who):
    """The five leading arguments of the st_ngram_* entries from a st_amd.ngram.DeviceTrie: (child_lo, tok, logp, bo, nodes)."""
    V, N, nodes = int(trie.V), int(trie.order), int(trie.nodes)
    if not (2 <= N <= NGRAM_MAX_ORDER and 1 <= V <= NGRAM_MAX_V and nodes >= V):
        raise ValueError("%s: order %d / vocabulary %d / %d nodes outside order 2..%d, V <= %d, nodes >= V"
                         % (who, N, V, nodes, NGRAM_MAX_ORDER, NGRAM_MAX_V))
    return (_dev(trie.child_lo, I32, (nodes + 1,), who + ": child_lo"), _dev(trie.tok, I32, (nodes,), who + ": tok"),
            _dev(trie.logp, F32, (nodes,), who + ": logp"), _dev(trie.bo, F32, (nodes,), who + ": bo"), nodes)


def ngram_score(trie, hist, cand, done, eos, scale=1.0, bias=0.0, lm_out=None, lp=None):
    """Language-model scores of every hypothesis's K candidates - see st_ngram_score.  hist i32 [n, order - 1] (oldest first, -1 =
    no token), cand i32 [n, K], done bool [B] or None (n = B x beam), lm_out f32 [n, K] or None (the raw scores), lp f32 [n, K] or
    None (updated in place: lp += scale lm + bias)."""
    who = "ngram_score"
    if cand.dim() != 2 or not 1 <= cand.shape[1] <= 64:
        raise ValueError("%s: cand must be an i32 [n, K <= 64] tensor, got %s" % (who, tuple(cand.shape)))
    args = _ngram_trie(trie, who)
    n, K = cand.shape
    _dev(cand, I32, (n, K), who + ": cand"), _dev(hist, I32, (n, trie.order - 1), who + ": hist")
    beam = n
    if done is not None:
        B = done.numel()
        if B <= 0 or n % B:
            raise ValueError("%s: %d rows do not divide into the %d utterances of done" % (who, n, B))
        _dev(done, torch.bool, (B,), who + ": done")
        beam = n // B
    if lm_out is not None:
        _dev(lm_out, F32, (n, K), who + ": lm_out")
    if lp is not None:
        _dev(lp, F32, (n, K), who + ": lp")
    if not float(scale) >= 0.0 or float(bias) != float(bias):
        raise ValueError("%s: scale must be >= 0 and bias a number, got %r, %r" % (who, scale, bias))
    _tag("ngram_score", n, K, trie.order)
    _check(load().st_ngram_score(_stream(), *args, int(trie.V), int(trie.order), float(trie.oov_logp), hist.data_ptr(), cand.data_ptr(),
                                 n, K, max(beam, 1), _p(done), int(eos), float(scale), float(bias), _p(lm_out), _p(lp)), "st_ngram_score")


def ngram_advance(hist, order, tokens, done, eos, beam):
    """The histories of the hypotheses a beam step chose, in place: hist[i] <- shift(hist[order[i]]) . tokens[i] - see
    st_ngram_advance.  hist i32 [n, N - 1]; order / tokens i64 [n] (st_beam_advance_joint's); done bool [B] or None."""
    who = "ngram_advance"
    if hist.dim() != 2 or not 1 <= hist.shape[1] <= NGRAM_MAX_ORDER - 1:
        raise ValueError("%s: hist must be an i32 [n, order - 1] tensor with order in 2..%d, got %s" % (who, NGRAM_MAX_ORDER, tuple(hist.shape)))
    n, H = hist.shape
    beam = int(beam)
    if beam <= 0 or n % beam or beam * H > 256:
        raise ValueError("%s: %d rows, beam %d, %d history tokens: beam must divide the rows and beam x tokens <= 256" % (who, n, beam, H))
    _dev(hist, I32, (n, H), who + ": hist"), _dev(order, I64, (n,), who + ": order"), _dev(tokens, I64, (n,), who + ": tokens")
    if done is not None:
        _dev(done, torch.bool, (n // beam,), who + ": done")
    _check(load().st_ngram_advance(_stream(), hist.data_ptr(), H + 1, order.data_ptr(), tokens.data_ptr(), _p(done), int(eos), n // beam,
                                   beam), "st_ngram_advance")


def ngram_score_seq(trie, tokens, lens, bos, out):
    """Teacher-forced language-model scores: tokens i32 [M, L_cap], lens i32 [M] -> out f32 [M, L_cap] = log p(tokens[m][t] | bos,
    tokens[m][:t]) for t < lens[m], 0 elsewhere - see st_ngram_score_seq."""
    who = "ngram_score_seq"
    args = _ngram_trie(trie, who)
    if tokens.dim() != 2:
        raise ValueError("%s: tokens must be an i32 [M, L_cap] tensor, got %s" % (who, tuple(tokens.shape)))
    M, L = tokens.shape
    _dev(tokens, I32, (M, L), who + ": tokens"), _dev(lens, I32, (M,), who + ": lens"), _dev(out, F32, (M, L), who + ": out")
    _tag("ngram_score_seq", M, L, trie.order)
    _check(load().st_ngram_score_seq(_stream(), *args, int(trie.V), int(trie.order), float(trie.oov_logp), tokens.data_ptr(),
                                     lens.data_ptr(), M, L, int(bos), out.data_ptr()), "st_ngram_score_seq")
    return out


# ---- contextual biasing (csrc/st_bias.hip; st_amd/biasing.py) --------------------------------------------------------------------------
BIAS_MAX_STATES = 65536


def _bias_tables(tables, who, values=True):
    """The leading arguments of the st_bias_* entries from a st_amd.biasing.DeviceAutomaton: (child_lo, tok, fail, [cash, phi,] S)."""
    S = int(tables.S)
    if not 1 <= S <= BIAS_MAX_STATES:
        raise ValueError("%s: %d automaton states outside 1..%d" % (who, S, BIAS_MAX_STATES))
    args = (_dev(tables.child_lo, I32, (S + 1,), who + ": child_lo"), _dev(tables.tok, I32, (S,), who + ": tok"),
            _dev(tables.fail, I32, (S,), who + ": fail"))
    if values:
        args += (_dev(tables.cash, F32, (S,), who + ": cash"), _dev(tables.phi, F32, (S,), who + ": phi"))
    return args + (S,)


def bias_score(tables, state, cand, done, eos, scale=1.0, raw=None, lp=None):
    """Phrase-reward increments of every hypothesis's K candidates - see st_bias_score.  state i32 [n] (-1 = frozen), cand i32
    [n, K], done bool [B] or None (n = B x beam), raw f32 [n, K] or None (the increments), lp f32 [n, K] or None (updated in place:
    lp = fma(scale, increment, lp))."""
    who = "bias_score"
    if cand.dim() != 2 or not 1 <= cand.shape[1] <= 64:
        raise ValueError("%s: cand must be an i32 [n, K <= 64] tensor, got %s" % (who, tuple(cand.shape)))
    args = _bias_tables(tables, who)
    n, K = cand.shape
    _dev(cand, I32, (n, K), who + ": cand"), _dev(state, I32, (n,), who + ": state")
    beam = n
    if done is not None:
        B = done.numel()
        if B <= 0 or n % B:
            raise ValueError("%s: %d rows do not divide into the %d utterances of done" % (who, n, B))
        _dev(done, torch.bool, (B,), who + ": done")
        beam = n // B
    if raw is not None:
        _dev(raw, F32, (n, K), who + ": raw")
    if lp is not None:
        _dev(lp, F32, (n, K), who + ": lp")
    if not 0.0 <= float(scale) < float("inf"):
        raise ValueError("%s: scale must be a finite number >= 0, got %r" % (who, scale))
    _tag("bias_score", n, K, args[-1])
    _check(load().st_bias_score(_stream(), *args, state.data_ptr(), cand.data_ptr(), n, K, max(beam, 1), _p(done), int(eos),
                                float(scale), _p(raw), _p(lp)), "st_bias_score")


def bias_advance(tables, state, order, tokens, done, eos, beam):
    """The automaton states of the hypotheses a beam step chose, in place: state[i] <- delta(state[order[i]], tokens[i]), -1 after
    EOS - see st_bias_advance.  state i32 [n]; order / tokens i64 [n] (st_beam_advance_joint's); done bool [B] or None."""
    who = "bias_advance"
    if state.dim() != 1:
        raise ValueError("%s: state must be an i32 [n] tensor, got %s" % (who, tuple(state.shape)))
    n, beam = state.shape[0], int(beam)
    if beam <= 0 or n % beam or beam > 256:
        raise ValueError("%s: %d rows, beam %d: beam must divide the rows and be <= 256" % (who, n, beam))
    args = _bias_tables(tables, who, values=False)
    _dev(state, I32, (n,), who + ": state"), _dev(order, I64, (n,), who + ": order"), _dev(tokens, I64, (n,), who + ": tokens")
    if done is not None:
        _dev(done, torch.bool, (n // beam,), who + ": done")
    _check(load().st_bias_advance(_stream(), *args, state.data_ptr(), order.data_ptr(), tokens.data_ptr(), _p(done), int(eos), n // beam,
                                  beam), "st_bias_advance")


def bias_score_seq(tables, tokens, lens, eos, out):
    """Teacher-forced phrase-reward increments: tokens i32 [M, L_cap], lens i32 [M] -> out f32 [M, L_cap] = the increment of
    position t for t < lens[m], 0 elsewhere and after an EOS - see st_bias_score_seq."""
    who = "bias_score_seq"
    args = _bias_tables(tables, who)
    if tokens.dim() != 2:
        raise ValueError("%s: tokens must be an i32 [M, L_cap] tensor, got %s" % (who, tuple(tokens.shape)))
    M, L = tokens.shape
    _dev(tokens, I32, (M, L), who + ": tokens"), _dev(lens, I32, (M,), who + ": lens"), _dev(out, F32, (M, L), who + ": out")
    _tag("bias_score_seq", M, L, args[-1])
    _check(load().st_bias_score_seq(_stream(), *args, tokens.data_ptr(), lens.data_ptr(), M, L, int(eos), out.data_ptr()),
           "st_bias_score_seq")
    return out


def attn_probs(Q, K, q_off, q_len, k_off, k_len, n_head, Lq, Lk, causal, scale, k_prescaled=False, out=None):
    """The attention probabilities of one sublayer, materialised: f32 [B, n_head, Lq, Lk] (zeros at masked keys and in the
    rows of padding positions).  Q, K: bf16 row matrices (column slices of the q | k | v projection are fine).  out: the
    caller's contiguous f32 [B, n_head, Lq, Lk] buffer (None: a new one).  One workgroup per query holds its scores in LDS:
    Lk + d_k + 8 <= 16384 floats (64 KiB), else ValueError (code -3)."""
    for t, nm in ((Q, "Q"), (K, "K")):
        _mat(t, BF16, nm)
    B = q_off.numel()
    d_k = Q.shape[1] // n_head
    if out is None:
        P = torch.empty(B, n_head, int(Lq), int(Lk), dtype=F32, device=Q.device)
    else:
        P = out
        _dev(P, F32, (B, n_head, int(Lq), int(Lk)), "attn_probs: out")
    _tag("attn_probs", B, n_head, d_k, int(Lq), int(Lk))
    rc = load().st_attn_probs(_stream(), Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), P.data_ptr(), q_off.data_ptr(),
                              q_len.data_ptr(), k_off.data_ptr(), k_len.data_ptr(), B, n_head, d_k, int(Lq), int(Lk), int(causal),
                              float(scale), int(bool(k_prescaled)))
    _check(rc, "st_attn_probs")
    return P


# The dense kernels keep one query's scores (forward, query side of the backward) or one key's (key side) in LDS, 64 KiB = 16384
# floats per workgroup (include/st_hip.h, st_attn_dense_*):
ATTN_DENSE_LDS_FLOATS = 16384


def attn_dense_lds_floats(d_k, Lq, Lk):
    """The floats of LDS per workgroup of (the forward, the backward's query side, the backward's key side)."""
    return Lk + 5 * d_k + 4, 2 * Lk + 6 * d_k + 4, 2 * Lq + 10 * d_k


def attn_dense_check(d_k, Lq, Lk, backward=True):
    """ValueError unless attn_dense_fwd - and, with ``backward``, attn_dense_bwd - accepts these extents:
        forward                Lk + 5 d_k + 4      <= 16384
        backward, query side   2 Lk + 6 d_k + 4    <= 16384
        backward, key side     2 Lq + 10 d_k       <= 16384
    A forward that will be differentiated is checked against all three BEFORE anything is launched (functional.DenseMhaFn), so
    that the refusal does not surface inside autograd.backward; an inference call keeps the forward's larger range."""
    fwd, bq, bk = attn_dense_lds_floats(int(d_k), int(Lq), int(Lk))
    lim = ATTN_DENSE_LDS_FLOATS
    bad = []
    if fwd > lim:
        bad.append("the forward needs Lk + 5 d_k + 4 = %d" % fwd)
    if backward and bq > lim:
        bad.append("the backward's query side needs 2 Lk + 6 d_k + 4 = %d" % bq)
    if backward and bk > lim:
        bad.append("the backward's key side needs 2 Lq + 10 d_k = %d" % bk)
    if bad:
        raise ValueError("dense attention: Lq = %d, Lk = %d, d_k = %d exceed the limit of %d floats (64 KiB) of LDS per workgroup: %s"
                         % (Lq, Lk, d_k, lim, "; ".join(bad)))


def attn_dense_fwd(Q, K, V, mask, O, lse, B, n_head, Lq, Lk, scale, drop=None, want_probs=False, probs=None):
    """Attention under an arbitrary dense mask (uint8 [B, Lq, Lk], nonzero = masked; None = no mask) over padded row matrices
    Q [B Lq, H d_k], K / V [B Lk, H d_k] (see st_attn_dense_fwd: the slow general path).  -> P (f32 [B, H, Lq, Lk], the
    probabilities BEFORE dropout; ``probs``: the caller's contiguous buffer for them, which implies want_probs) or None.
    Limit: Lk + 5 d_k + 4 <= 16384 floats of LDS, else ValueError (code -3); attn_dense_bwd's limits are tighter -
    attn_dense_check(d_k, Lq, Lk) tells before the forward runs."""
    for t, nm in ((Q, "Q"), (K, "K"), (V, "V"), (O, "O")):
        _mat(t, BF16, nm)
    d_k = Q.shape[1] // n_head
    if mask is not None:
        _dev(mask, torch.uint8, (B, Lq, Lk), "attn_dense_fwd: mask")
    if Q.shape[0] != B * Lq or K.shape[0] != B * Lk or V.shape[0] != B * Lk:
        raise ValueError("attn_dense_fwd: padded layouts expected (B Lq query rows, B Lk key rows)")
    _vec(lse, F32, n_head * B * Lq, "lse")
    if probs is not None:
        P = probs
        _dev(P, F32, (B, n_head, Lq, Lk), "attn_dense_fwd: probs")
    else:
        P = torch.empty(B, n_head, Lq, Lk, dtype=F32, device=Q.device) if want_probs else None
    _tag("attn_dense", B, n_head, d_k, Lq, Lk)
    rc = load().st_attn_dense_fwd(_stream(), Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0), _p(mask),
                                  O.data_ptr(), O.stride(0), lse.data_ptr(), _p(P), B, n_head, d_k, int(Lq), int(Lk), float(scale),
                                  *_drop(drop))
    _check(rc, "st_attn_dense_fwd")
    return P


def attn_dense_bwd(Q, K, V, mask, dO, lse, delta, dQ, dK, dV, B, n_head, Lq, Lk, scale, drop=None):
    """The backward of attn_dense_fwd (same Q, K, V, mask, drop; lse from the forward): writes delta (f32 [H, B Lq]), dQ, dK, dV.
    Limits: 2 Lk + 6 d_k + 4 <= 16384 (query side) and 2 Lq + 10 d_k <= 16384 (key side) floats of LDS, else ValueError (code -3)
    with nothing launched."""
    for t, nm in ((Q, "Q"), (K, "K"), (V, "V"), (dO, "dO"), (dQ, "dQ"), (dK, "dK"), (dV, "dV")):
        _mat(t, BF16, nm)
    d_k = Q.shape[1] // n_head
    _vec(lse, F32, n_head * B * Lq, "lse"), _vec(delta, F32, n_head * B * Lq, "delta")
    _tag("attn_dense_bwd", B, n_head, d_k, Lq, Lk)
    rc = load().st_attn_dense_bwd(_stream(), Q.data_ptr(), Q.stride(0), K.data_ptr(), K.stride(0), V.data_ptr(), V.stride(0), _p(mask),
                                  dO.data_ptr(), dO.stride(0), lse.data_ptr(), delta.data_ptr(), dQ.data_ptr(), dQ.stride(0),
                                  dK.data_ptr(), dK.stride(0), dV.data_ptr(), dV.stride(0), B, n_head, d_k, int(Lq), int(Lk),
                                  float(scale), *_drop(drop))
    _check(rc, "st_attn_dense_bwd")


# ---- the feature kernel family (csrc/st_augment.hip): one private function per family, the public wrappers pass their name as
# ``who``; table None = the variant without masks, warp None = the variant without the time warp ----------------------------------
WARP_MAX_FRAMES = 32767      # raw frames of an utterance up to which the warp kernels' 32-bit map is the definition (include/st_hip.h)


def _specaug_args(who, n_time, n_freq, left, right, interval):
    """The integer checks the SpecAugment wrappers share (before any tensor is looked at): mask counts and stacking geometry."""
    n_time, n_freq, left, right, interval = int(n_time), int(n_freq), int(left), int(right), int(interval)
    if n_time < 0 or n_freq < 0 or n_time + n_freq > 64:
        raise ValueError("%s: %d time + %d frequency masks - both counts >= 0 and at most 64 masks in all" % (who, n_time, n_freq))
    if left < 0 or right < 0 or right > left or interval < 1:
        raise ValueError("%s: left %d / right %d / interval %d - contexts >= 0, right <= left, interval >= 1" % (who, left, right, interval))
    return n_time, n_freq, left, right, interval


def _given(who, name, t):
    """A table a public wrapper requires: passed on as None it would select the variant without.  Evaluated as the wrapper's
    argument, so a missing table is reported before any other bad argument - ValueError, as _dev(None) raised it before."""
    if t is None:
        raise ValueError("%s: %s: expected an int32 tensor on the GPU, got None" % (who, name))
    return t


def _tables(who, B, n_masks, table, warp):
    """The mask table and (warp None: no time warp) the warp table -> the pointers the entry point takes after its other arguments."""
    _dev(table, I32, (B, n_masks, 2), who + ": table")
    if warp is None:
        return (table.data_ptr(),)
    _dev(warp, I32, (B, 2), who + ": warp")
    return table.data_ptr(), warp.data_ptr()


def _specaug_plan(who, seed, salt, length, table, warp, n_time, time_width, time_ratio_permille, n_freq, freq_width, mel_bins, time_warp,
                  interval, right):
    B = length.numel()
    if min(int(time_width), int(freq_width)) < 0 or int(mel_bins) < 1 or not 0 <= int(time_ratio_permille) <= 1000:
        raise ValueError("%s: time_width %d / freq_width %d >= 0, mel_bins %d >= 1, time_ratio_permille %d in 0 .. 1000"
                         % (who, time_width, freq_width, mel_bins, time_ratio_permille))
    if warp is not None and (int(time_warp) != time_warp or not 0 <= int(time_warp) <= WARP_MAX_FRAMES):
        raise ValueError("%s: time_warp = %r must be an integer in 0 .. %d" % (who, time_warp, WARP_MAX_FRAMES))
    if B > 1 << 24:
        raise ValueError("%s: at most 2^24 utterances (the draw's counter is 32 bits wide)" % who)
    n_time, n_freq, _, right, interval = _specaug_args(who, n_time, n_freq, right, right, interval)
    tables = _tables(who, B, n_time + n_freq, table, warp)
    _dev(seed, I32, (1,), who + ": seed"), _vec(length, I32, B, who + ": length")
    _tag(who, B, n_time + n_freq, io=(length, table) if warp is None else (length, table, warp))
    _check(getattr(load(), "st_" + who)(_stream(), seed.data_ptr(), int(salt) & 0xFFFFFFFF, length.data_ptr(), B, interval, right, n_time,
                                        int(time_width), int(time_ratio_permille), n_freq, int(freq_width), int(mel_bins),
                                        *((int(time_warp),) if warp is not None else ()), *tables), "st_" + who)


def _pack_rows_aug(who, x, off, length, out, table, warp, n_time, n_freq, mel_bins, left, right, interval):
    if x.dim() != 3:
        raise ValueError("%s: x must be [B, T, F], got %s" % (who, tuple(x.shape)))
    B, T, Fd = x.shape
    mel_bins = int(mel_bins)
    if mel_bins < 4 or mel_bins % 4:
        raise ValueError("%s: mel_bins = %d must be a positive multiple of 4 (a 16-byte chunk lies in one context slot)" % (who, mel_bins))
    n_time, n_freq, left, right, interval = _specaug_args(who, n_time, n_freq, left, right, interval)
    if warp is not None and (right != 0 or left < interval - 1):
        raise ValueError("%s: left %d / right %d / interval %d - the warp reads raw frames from the stacked rows, which "
                         "show every one of them only with right == 0 and left >= interval - 1" % (who, left, right, interval))
    if Fd != mel_bins * (1 + left + right):
        raise ValueError("%s: %d columns are not %d bins x (1 + %d + %d) context slots" % (who, Fd, mel_bins, left, right))
    if warp is not None and T * interval > WARP_MAX_FRAMES:
        raise ValueError("%s: T %d x interval %d > %d raw frames: beyond the kernel's 32-bit map" % (who, T, interval, WARP_MAX_FRAMES))
    tables = _tables(who, B, n_time + n_freq, table, warp)
    _dev(x, F32, (B, T, Fd), who + ": x")
    _vec(off, I32, B, "off"), _vec(length, I32, B, "len")
    if off.numel() != B or length.numel() != B:
        raise ValueError("%s: off / len must have one entry per utterance (%d)" % (who, B))
    _mat(out, BF16, "out", ld=Fd)
    _tag(who, out.shape[0], Fd, io=(float(out.shape[0]) * Fd * x.element_size(), out, table) + (() if warp is None else (warp,)))
    _check(getattr(load(), "st_" + who)(_stream(), x.data_ptr(), B, T, Fd, off.data_ptr(), length.data_ptr(), out.data_ptr(), *tables,
                                        n_time, n_freq, mel_bins, left, right, interval), "st_" + who)
    return out


def _feat_stack(who, x, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out, table=None, warp=None, n_time=0,
                n_freq=0):
    if table is None:          # the plain front-end: its geometry is the entry point's to refuse
        _dev(x, F32, (None, None, None), who + ": x")
        B, T, F = x.shape
        left, right, interval = int(left), int(right), int(interval)
        extra = ()
    else:
        if x.dim() != 3:
            raise ValueError("%s: x must be [B, T, F], got %s" % (who, tuple(x.shape)))
        B, T, F = x.shape
        n_time, n_freq, left, right, interval = _specaug_args(who, n_time, n_freq, left, right, interval)
        if warp is not None and T > WARP_MAX_FRAMES:
            raise ValueError("%s: T %d > %d raw frames: beyond the kernel's 32-bit map" % (who, T, WARP_MAX_FRAMES))
        extra = _tables(who, B, n_time + n_freq, table, warp) + (n_time, n_freq)      # what the entry point takes after ld
        _dev(x, F32, (B, T, F), who + ": x")
    _vec(in_len, I32, B, "in_len"), _vec(out_off, I32, B, "out_off"), _vec(out_len, I32, B, "out_len")
    _mat(out, BF16, "out")
    if table is not None and out.stride(0) < F * (1 + left + right):
        raise ValueError("%s: out has a leading dimension of %d for %d stacked columns" % (who, out.stride(0), F * (1 + left + right)))
    if stats is not None:
        _dev(stats, F32, (B, 2, F + 1), who + ": stats")
    _tag(who, B, T, F)
    _check(getattr(load(), "st_" + who)(_stream(), x.data_ptr(), B, T, F, in_len.data_ptr(), _p(stats), left, right, interval,
                                        out_off.data_ptr(), out_len.data_ptr(), int(max_out_len), out.data_ptr(), out.stride(0),
                                        *extra), "st_" + who)
    return out


def feat_stack(x, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out):
    """Raw padded features x fp32 [B, T, F] -> stacked / subsampled / normalised bf16 rows (Dataset.py front-end)."""
    return _feat_stack("feat_stack", x, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out)


def specaug_plan(seed, salt, length, table, n_time, time_width, time_ratio_permille, n_freq, freq_width, mel_bins, interval=1,
                 right=0):
    """SpecAugment's masks of one step (st_specaug_plan): table int32 [B, n_time + n_freq, 2] <- (start, width) of every
    mask, drawn from the device seed (the 1-element int32 tensor of st_amd.rng) and ``salt``.  length: int32 [B] on the device
    - raw frames with (interval 1, right 0), else rows already stacked with that geometry."""
    _specaug_plan("specaug_plan", seed, salt, length, table, None, n_time, time_width, time_ratio_permille, n_freq, freq_width, mel_bins,
                  0, interval, right)
    return table


def pack_rows_aug(x, off, length, out, table, n_time, n_freq, mel_bins, left=0, right=0, interval=1):
    """pack_rows with the masks of ``table`` applied (st_pack_rows_aug): x fp32 [B, T, mel_bins * (1 + left + right)], rows
    already stacked / subsampled with that geometry."""
    return _pack_rows_aug("pack_rows_aug", x, off, length, out, table, None, n_time, n_freq, mel_bins, left, right, interval)


def feat_stack_aug(x, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out, table, n_time, n_freq):
    """feat_stack with the masks of ``table`` (planned with the raw lengths) applied after CMVN, before stacking
    (st_feat_stack_aug)."""
    return _feat_stack("feat_stack_aug", x, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out,
                       _given("feat_stack_aug", "table", table), None, n_time, n_freq)


def specaug_plan_warp(seed, salt, length, table, warp, n_time, time_width, time_ratio_permille, n_freq, freq_width, mel_bins,
                      time_warp, interval=1, right=0):
    """specaug_plan and the time warp's draw in one launch (st_specaug_plan_warp): ``table`` as specaug_plan writes it, bit for
    bit, and warp int32 [B, 2] <- (c, c') of every utterance ((0, 0): not warped)."""
    _specaug_plan("specaug_plan_warp", seed, salt, length, table, _given("specaug_plan_warp", "warp", warp), n_time, time_width,
                  time_ratio_permille, n_freq, freq_width, mel_bins, time_warp, interval, right)
    return table, warp


def pack_rows_warp(x, off, length, out, table, warp, n_time, n_freq, mel_bins, left=0, right=0, interval=1):
    """pack_rows_aug with the time warp of ``warp`` applied before the masks (st_pack_rows_warp): the source frames are read
    from the stacked rows themselves, so right == 0 and left >= interval - 1."""
    return _pack_rows_aug("pack_rows_warp", x, off, length, out, table, _given("pack_rows_warp", "warp", warp), n_time, n_freq, mel_bins, left,
                          right, interval)


def feat_stack_warp(x, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out, table, warp, n_time, n_freq):
    """feat_stack_aug with the time warp of ``warp`` applied after CMVN, before the masks and the stacking (st_feat_stack_warp)."""
    return _feat_stack("feat_stack_warp", x, in_len, stats, left, right, interval, out_off, out_len, max_out_len, out,
                       _given("feat_stack_warp", "table", table), _given("feat_stack_warp", "warp", warp), n_time, n_freq)


def row_index(off, length, max_len, row_pos, row_seq=None):
    B = off.numel()
    _vec(off, I32, B, "off"), _vec(length, I32, B, "len")
    _check(load().st_row_index(_stream(), off.data_ptr(), length.data_ptr(), B, int(max_len), row_pos.data_ptr(),
                               _p(row_seq)), "st_row_index")
    return row_pos


def pack_rows(x, off, length, out):
    _dev(x, F32, (None, None, None), "pack_rows: x")
    B, T, Fd = x.shape
    _mat(out, BF16, "out", ld=Fd)
    _tag("pack_rows", out.shape[0], Fd, io=(float(out.shape[0]) * Fd * x.element_size(), out))
    _check(load().st_pack_rows(_stream(), x.data_ptr(), B, T, Fd, off.data_ptr(), length.data_ptr(), out.data_ptr()),
           "st_pack_rows")
    return out


def unpack_rows(x, off, length, out):
    _mat(x, BF16, "x")
    _dev(out, F32, (None, None, None), "unpack_rows: out")
    B, T, D = out.shape
    _check(load().st_unpack_rows(_stream(), x.data_ptr(), x.stride(0), B, T, D, off.data_ptr(), length.data_ptr(),
                                 out.data_ptr()), "st_unpack_rows")
    return out


def pack_grad(g, off, length, out):
    _dev(g, F32, (None, None, None), "pack_grad: g")
    B, T, D = g.shape
    _mat(out, BF16, "out")
    _check(load().st_pack_grad(_stream(), g.data_ptr(), B, T, D, off.data_ptr(), length.data_ptr(), out.data_ptr(),
                               out.stride(0)), "st_pack_grad")
    return out


def embed_pe_fwd(tok, emb, pe, off, length, out):
    _dev(tok, I64, (None, None), "embed_pe_fwd: tok")
    B, L = tok.shape
    D = emb.shape[-1]
    _mat(emb, F32, "emb", ld=D), _mat(pe, F32, "pe", ld=D, min_rows=L), _mat(out, BF16, "out", ld=D)
    _tag("embed_pe_fwd", out.shape[0], D, io=(8.0 * out.shape[0] * D, out))
    _check(load().st_embed_pe_fwd(_stream(), tok.data_ptr(), B, L, emb.data_ptr(), emb.shape[0], pe.data_ptr(), D,
                                  off.data_ptr(), length.data_ptr(), out.data_ptr()), "st_embed_pe_fwd")
    return out


def embed_bwd(tok, dy, off, length, pad_idx, demb):
    _dev(tok, I64, (None, None), "embed_bwd: tok")
    B, L = tok.shape
    _mat(dy, BF16, "dy"), _mat(demb, F32, "demb", ld=demb.shape[-1])
    D = demb.shape[1]
    _tag("embed_bwd", dy.shape[0], D, io=(dy, 8.0 * dy.shape[0] * D))
    _check(load().st_embed_bwd(_stream(), tok.data_ptr(), B, L, dy.data_ptr(), dy.stride(0), D, off.data_ptr(),
                               length.data_ptr(), int(pad_idx), demb.data_ptr(), demb.shape[0]), "st_embed_bwd")
    return demb


def embed_step(tokens, emb, pe, step, out):
    """out bf16 [n, D] = emb[tokens] + pe[step] (step: i64 [1] on the device) - one beam-search step's decoder input."""
    n, D = out.shape
    _mat(out, BF16, "out", ld=D), _vec(tokens, I64, n, "tokens"), _vec(step, I64, 1, "step")
    _dev(emb, F32, (emb.shape[0], D), "embed_step: emb"), _dev(pe, F32, (pe.shape[0], D), "embed_step: pe")
    _check(load().st_embed_step(_stream(), tokens.data_ptr(), emb.data_ptr(), emb.shape[0], pe.data_ptr(), step.data_ptr(),
                                out.data_ptr(), n, D), "st_embed_step")
    return out


def decode_self_attn(qkv, cache, step, ctx, n_head, scale, anc=None):
    """One beam-search step's self-attention (one query per hypothesis): appends this step's k | v (columns [d, 3d) of qkv
    [n, 3d]) to ``cache`` [n, S, 2d] (one layer, contiguous) at position ``step`` (i64 [1], device) and writes the context
    [n, d] over positions 0 .. step.  d / n_head = 64, S <= 128.  ``anc``: optional lineage table i32 [n, S] (see
    st_decode_self_attn): earlier positions are read from the cache rows it names."""
    _mat(qkv, BF16, "qkv"), _mat(ctx, BF16, "ctx")
    n, S, w = cache.shape
    d = w // 2
    _dev(cache, BF16, (n, S, w), "decode_self_attn: cache")
    if qkv.shape != (n, 3 * d) or ctx.shape != (n, d):
        raise ValueError("decode_self_attn: qkv [n, 3d], cache [n, S, 2d] (contiguous bf16), ctx [n, d]")
    if d % n_head or d // n_head != 64 or S > 128:
        raise ValueError("decode_self_attn: head width 64 and at most 128 cached positions")
    _vec(step, I64, 1, "step")
    _tag("decode_self_attn", n, n_head, S)
    _check(load().st_decode_self_attn(_stream(), qkv.data_ptr(), qkv.stride(0), cache.data_ptr(), step.data_ptr(),
                                      None if anc is None else _dev(anc, I32, (n, S), "decode_self_attn: anc"), ctx.data_ptr(), ctx.stride(0), n, S, int(n_head),
                                      d // n_head, float(scale)), "st_decode_self_attn")


def beam_advance(logits, V, beam, step, eos, scores, tokens, done, lengths, hist_scores, back, toks, order, work=None, anc=None,
                 advance_step=False, embed=None):
    """Beam.advance for all utterances on the device (see st_beam_advance): logits f32 [B * beam, >= V]; the state tensors
    are updated in place (scores f32 [B, beam], tokens i64 [B * beam], done bool [B], lengths i64 [B], hist_scores f32 /
    back i64 / toks i64 [S, B, beam] at row ``step`` (i64 [1], device)); order i64 [B * beam] receives the cache rows.
    ``work``: optional zeroed i64 [>= beam_work_words(B, beam)] scratch - with it the step runs over B * beam workgroups.
    ``anc``: optional lineage table i32 [B * beam, S'] of decode_self_attn, updated for the new hypotheses (needs ``work``).
    ``advance_step``: the launch also does ``step += 1`` (needs ``work``).
    ``embed`` = (emb f32 [V', D], pe f32 [P, D], x_next bf16 [B * beam, D]): the launch also writes the next step's decoder
    input for the chosen tokens (embed_step's arithmetic at position step + 1; needs ``work``)."""
    B = scores.shape[0]
    _mat(logits, F32, "logits", rows=B * beam)
    for t, dt, n, name in ((scores, F32, B * beam, "scores"), (tokens, I64, B * beam, "tokens"), (lengths, I64, B, "lengths"),
                           (order, I64, B * beam, "order"), (step, I64, 1, "step")):
        _vec(t, dt, n, name)
    _dev(done, torch.bool, (B,), "done")
    S = hist_scores.shape[0]
    for t, dt, name in ((hist_scores, F32, "hist_scores"), (back, I64, "back"), (toks, I64, "toks")):
        _dev(t, dt, (S, B, beam), name)
    _vec(work, I64, beam_work_words(B, beam), "work")
    if (advance_step or embed is not None) and work is None:
        raise ValueError("beam_advance: advance_step / embed need the work buffer")
    _tag("beam_advance", B, beam, V)
    _check(load().st_beam_advance(_stream(), logits.data_ptr(), logits.stride(0), int(V), int(beam), B, step.data_ptr(), int(eos),
                                  scores.data_ptr(), tokens.data_ptr(), done.data_ptr(), lengths.data_ptr(),
                                  hist_scores.data_ptr(), back.data_ptr(), toks.data_ptr(), order.data_ptr(),
                                  _p(work), None if anc is None else _dev(anc, I32, (B * beam, anc.shape[-1]), "anc"),
                                  0 if anc is None else anc.shape[1], step.data_ptr() if advance_step else None,
                                  *_embed_next(embed, B * beam)), "st_beam_advance")


def beam_work_words(B: int, beam: int) -> int:
    """int64 elements of beam_advance's ``work`` scratch (zero-initialised): beam keys per hypothesis row, the step ticket, a
    ticket per utterance."""
    return B * beam * beam + 1 + B


# ---- joint CTC / attention beam search (csrc/st_ctc_decode.hip) ---------------------------------------------------------------
def ctc_vocab_lp(logits, V, off, length, T_cap, lse, lpT):
    """CTC logits f32 [R, >= V] (packed encoder rows, utterance b at off[b] .. off[b] + len[b]) -> lse f32 [R] and the
    vocabulary-major log-probabilities lpT f32 [B, V, T_cap] (frames past len[b]: 0) - see st_ctc_vocab_lp."""
    _mat(logits, F32, "logits")
    R, B = logits.shape[0], off.numel()
    _vec(off, I32, B, "off"), _vec(length, I32, B, "len")
    _dev(lse, F32, (R,), "ctc_vocab_lp: lse"), _dev(lpT, F32, (B, V, T_cap), "ctc_vocab_lp: lpT")
    _tag("ctc_vocab_lp", R, V, T_cap, io=(2 * 4.0 * R * V, lpT))
    _check(load().st_ctc_vocab_lp(_stream(), logits.data_ptr(), logits.stride(0), R, int(V), off.data_ptr(), length.data_ptr(), B,
                                  int(T_cap), lse.data_ptr(), lpT.data_ptr()), "st_ctc_vocab_lp")


def ctc_prefix_init(lpT, length, beam, blank, gam, psi, last, frozen):
    """The empty prefix's CTC state in every beam slot (see st_ctc_prefix_init): gam f32 [B * beam, 2, T_cap], psi f32, last
    i32, frozen bool [B * beam]."""
    B, V, T_cap = lpT.shape
    n = B * beam
    _dev(lpT, F32, (B, V, T_cap), "lpT"), _vec(length, I32, B, "len"), _dev(gam, F32, (n, 2, T_cap), "gam")
    _dev(psi, F32, (n,), "psi"), _dev(last, I32, (n,), "last"), _dev(frozen, torch.bool, (n,), "frozen")
    _check(load().st_ctc_prefix_init(_stream(), lpT.data_ptr(), V, T_cap, length.data_ptr(), B, int(beam), int(blank), gam.data_ptr(),
                                     psi.data_ptr(), last.data_ptr(), frozen.data_ptr()), "st_ctc_prefix_init")


def ctc_prefix_score(lpT, length, beam, blank, eos, cand, gam, psi, last, frozen, done, cand_gam, cand_psi, delta):
    """CTC prefix scores of every hypothesis's K candidates (i32 [n, K]): cand_psi / delta f32 [n, K], the candidates' states
    cand_gam f32 [n, K, 2, T_cap] - see st_ctc_prefix_score.  ``done``: bool [B] or None (no utterance skipped)."""
    B, V, T_cap = lpT.shape
    n = B * beam
    K = cand.shape[1]
    _dev(lpT, F32, (B, V, T_cap), "lpT"), _vec(length, I32, B, "len"), _dev(cand, I32, (n, K), "cand")
    _dev(gam, F32, (n, 2, T_cap), "gam"), _dev(psi, F32, (n,), "psi"), _dev(last, I32, (n,), "last")
    _dev(frozen, torch.bool, (n,), "frozen"), _dev(cand_gam, F32, (n, K, 2, T_cap), "cand_gam")
    _dev(cand_psi, F32, (n, K), "cand_psi"), _dev(delta, F32, (n, K), "delta")
    if done is not None:
        _dev(done, torch.bool, (B,), "done")
    _tag("ctc_prefix_score", n, K, T_cap, io=(4.0 * n * K * T_cap, 8.0 * n * T_cap, 8.0 * n * K * T_cap))
    _check(load().st_ctc_prefix_score(_stream(), lpT.data_ptr(), V, T_cap, length.data_ptr(), B, int(beam), int(blank), int(eos),
                                      cand.data_ptr(), K, gam.data_ptr(), psi.data_ptr(), last.data_ptr(), frozen.data_ptr(),
                                      _p(done), cand_gam.data_ptr(), cand_psi.data_ptr(), delta.data_ptr()), "st_ctc_prefix_score")


def beam_pre_beam(logits, V, ids, lp):
    """Log-softmax of every decoder logits row (f32 [n, >= V]) and its K best -> ids i32 [n, K], lp f32 [n, K] (best first) -
    see st_beam_pre_beam."""
    _mat(logits, F32, "logits")
    n, K = ids.shape
    _dev(ids, I32, (n, K), "ids"), _dev(lp, F32, (n, K), "lp")
    if logits.shape[0] != n:
        raise ValueError("beam_pre_beam: logits rows %d != ids rows %d" % (logits.shape[0], n))
    _tag("beam_pre_beam", n, V, K, io=((logits, n),))
    _check(load().st_beam_pre_beam(_stream(), logits.data_ptr(), logits.stride(0), int(V), n, K, ids.data_ptr(), lp.data_ptr()),
           "st_beam_pre_beam")


def beam_advance_joint(ids, lp, delta, ctc_weight, beam, step, eos, scores, tokens, done, lengths, hist_scores, back, toks, order,
                       anc=None, advance_step=False, ticket=None, embed=None, ctc=None):
    """st_beam_advance over beam x K joint candidates (ids i32 / lp / delta f32 [B * beam, K]; score increment
    (1 - w) lp + w delta).  State tensors as beam_advance.  ``advance_step`` needs ``ticket`` (zeroed i64 [1]).  ``embed`` as
    beam_advance.  ``ctc`` = (cand_gam, cand_psi, gam, psi, last, frozen): the CTC state of the new hypotheses is moved in the
    same launch - see st_beam_advance_joint."""
    B = scores.shape[0]
    n, K = ids.shape
    _dev(ids, I32, (B * beam, K), "ids"), _dev(lp, F32, (n, K), "lp"), _dev(delta, F32, (n, K), "delta")
    for t, dt, m, name in ((scores, F32, B * beam, "scores"), (tokens, I64, B * beam, "tokens"), (lengths, I64, B, "lengths"),
                           (order, I64, B * beam, "order"), (step, I64, 1, "step")):
        _vec(t, dt, m, name)
    _dev(done, torch.bool, (B,), "done")
    S = hist_scores.shape[0]
    for t, dt, name in ((hist_scores, F32, "hist_scores"), (back, I64, "back"), (toks, I64, "toks")):
        _dev(t, dt, (S, B, beam), name)
    if advance_step and ticket is None:
        raise ValueError("beam_advance_joint: advance_step needs the ticket word")
    if ticket is not None:
        _vec(ticket, I64, 1, "ticket")
    T_cap, cp = 0, [None] * 6
    if ctc is not None:
        cand_gam, cand_psi, gam, psi, last, frozen = ctc
        T_cap = gam.shape[2]
        _dev(cand_gam, F32, (n, K, 2, T_cap), "cand_gam"), _dev(cand_psi, F32, (n, K), "cand_psi")
        _dev(gam, F32, (n, 2, T_cap), "gam"), _dev(psi, F32, (n,), "psi"), _dev(last, I32, (n,), "last")
        _dev(frozen, torch.bool, (n,), "frozen")
        cp = [t.data_ptr() for t in ctc]
    _tag("beam_advance_joint", B, beam, K)
    _check(load().st_beam_advance_joint(_stream(), ids.data_ptr(), lp.data_ptr(), delta.data_ptr(), K, float(ctc_weight), int(beam), B,
                                        step.data_ptr(), int(eos), scores.data_ptr(), tokens.data_ptr(), done.data_ptr(),
                                        lengths.data_ptr(), hist_scores.data_ptr(), back.data_ptr(), toks.data_ptr(), order.data_ptr(),
                                        None if anc is None else _dev(anc, I32, (B * beam, anc.shape[-1]), "anc"),
                                        0 if anc is None else anc.shape[1], step.data_ptr() if advance_step else None,
                                        _p(ticket), *_embed_next(embed, B * beam), int(T_cap), *cp), "st_beam_advance_joint")


def ctc_best_path(logits, V, out):
    """out i32 [R] = the arg-max of every CTC logits row (f32 [R, >= V]) - see st_ctc_best_path."""
    _mat(logits, F32, "logits")
    _dev(out, I32, (logits.shape[0],), "ctc_best_path: out")
    _check(load().st_ctc_best_path(_stream(), logits.data_ptr(), logits.stride(0), logits.shape[0], int(V), out.data_ptr()),
           "st_ctc_best_path")
    return out


def cache_reorder(cache, order, step, beam):
    """cache bf16 [L, n, S, W] (contiguous): rows of every utterance re-gathered by ``order`` (int64 [n], device) for the
    positions <= step (int64 [1], device) - see st_cache_reorder."""
    _dev(cache, BF16, (None, None, None, None), "cache_reorder: cache")
    L, n, S, W = cache.shape
    _vec(order, I64, n, "order"), _vec(step, I64, 1, "step")
    _check(load().st_cache_reorder(_stream(), cache.data_ptr(), order.data_ptr(), step.data_ptr(), L, n, S, W, int(beam)),
           "st_cache_reorder")
    return cache


def ce_fwd(logits, target, ignore_index, lse, sums, V=None, index=None):
    """lse[r] = logsumexp(logits[r, :V]); sums = (sum of the non-ignored rows' losses, their count, the mean = the loss)
    - see st_ce_fwd.  index: row r's target is target.view(-1)[index[r]]."""
    _mat(logits, F32, "logits")
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    _vec(target, I64, R if index is None else 0, "target"), _vec(index, I64, R, "target_index")      # (with index: any i64 vector)
    _vec(lse, F32, R, "lse"), _vec(sums, F32, 3, "sums")
    row_loss = torch.empty(R, dtype=F32, device=logits.device)       # scratch: summed by the call's second launch
    _tag("ce_fwd", R, V, 0, io=(2.0 * R * V, 8.0 * R))
    _check(load().st_ce_fwd(_stream(), logits.data_ptr(), logits.stride(0), R, V, target.data_ptr(), _p(index), int(ignore_index),
                            lse.data_ptr(), row_loss.data_ptr(), sums.data_ptr()), "st_ce_fwd")


def ce_bwd(logits, target, ignore_index, lse, sums, grad_out, dlogits, V=None, index=None):
    """dlogits (bf16, same shape as logits) = d(mean loss) / d(logits) * grad_out - see st_ce_bwd."""
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    _mat(dlogits, BF16, "dlogits", rows=R, ld=dlogits.shape[-1])
    if dlogits.shape[1] < V or dlogits.stride(0) % 8:
        raise ValueError("ce_bwd: dlogits must be a contiguous bf16 [R, >= V] matrix with a row length that is a multiple of 8")
    _vec(target, I64, R if index is None else 0, "target"), _vec(index, I64, R, "target_index")
    _vec(grad_out, F32, 1, "grad_out")
    _tag("ce_bwd", R, V, 0, io=(4.0 * R * V, 8.0 * R))
    _check(load().st_ce_bwd(_stream(), logits.data_ptr(), logits.stride(0), R, V, target.data_ptr(), _p(index), int(ignore_index),
                            lse.data_ptr(), sums.data_ptr(), grad_out.data_ptr(), dlogits.data_ptr(), dlogits.stride(0)),
           "st_ce_bwd")


def _ce_smooth_args(who, logits, target, V, index, zero_col, denom, lse, sums):
    """The checks ce_smooth_fwd / ce_smooth_bwd share -> (R, V)."""
    V = logits.shape[-1] if V is None else int(V)
    if not 0 < V <= logits.shape[-1] or int(zero_col) >= V:
        raise ValueError("%s: V = %d must lie in [1, %d] (the TRUE vocabulary: no padding column) and zero_col = %d below it"
                         % (who, V, logits.shape[-1], int(zero_col)))
    _mat(logits, F32, "logits")
    R = logits.shape[0]
    _vec(target, I64, R if index is None else 0, "target"), _vec(index, I64, R, "target_index")
    _vec(lse, F32, R, "lse"), _vec(sums, F32, 4, "sums"), _vec(denom, F32, 1, "denom")
    return R, V


def ce_smooth_fwd(logits, target, ignore_index, confidence, smooth, zero_col, lse, sums, V=None, index=None, denom=None):
    """Cross-entropy against the smoothed target (confidence at the target, 0 at zero_col, smooth elsewhere) - see
    st_ce_smooth_fwd.  V: the TRUE vocabulary size (padding columns of ``logits`` are not read); sums f32 [4] = (sum of the row
    losses, non-ignored rows, the loss = sum / (*denom, or the row count when denom is None), the plain token-mean NLL)."""
    R, V = _ce_smooth_args("ce_smooth_fwd", logits, target, V, index, zero_col, denom, lse, sums)
    row_loss = torch.empty(R, dtype=F32, device=logits.device)       # scratch: summed by the call's second launch
    _tag("ce_smooth_fwd", R, V, 0, io=(2.0 * R * V, 8.0 * R))
    _check(load().st_ce_smooth_fwd(_stream(), logits.data_ptr(), logits.stride(0), R, V, target.data_ptr(), _p(index),
                                   int(ignore_index), float(confidence), float(smooth), int(zero_col), _p(denom), lse.data_ptr(),
                                   row_loss.data_ptr(), sums.data_ptr()), "st_ce_smooth_fwd")


def ce_smooth_bwd(logits, target, ignore_index, confidence, smooth, zero_col, lse, sums, grad_out, dlogits, V=None, index=None,
                  denom=None):
    """dlogits (bf16, same rows as logits) = d(loss) / d(logits) * grad_out for ce_smooth_fwd's loss - see st_ce_smooth_bwd."""
    R, V = _ce_smooth_args("ce_smooth_bwd", logits, target, V, index, zero_col, denom, lse, sums)
    _mat(dlogits, BF16, "dlogits", rows=R, ld=dlogits.shape[-1])
    if dlogits.shape[1] < V or dlogits.stride(0) % 8:
        raise ValueError("ce_smooth_bwd: dlogits must be a contiguous bf16 [R, >= V] matrix with a row length that is a multiple of 8")
    _vec(grad_out, F32, 1, "grad_out")
    _tag("ce_smooth_bwd", R, V, 0, io=(4.0 * R * V, 8.0 * R))
    _check(load().st_ce_smooth_bwd(_stream(), logits.data_ptr(), logits.stride(0), R, V, target.data_ptr(), _p(index),
                                   int(ignore_index), float(confidence), float(smooth), int(zero_col), _p(denom), lse.data_ptr(),
                                   sums.data_ptr(), grad_out.data_ptr(), dlogits.data_ptr(), dlogits.stride(0)),
           "st_ce_smooth_bwd")


def zero_tails(table, n_max):
    """table: int64 device tensor [n_max * 4] of (address, bytes per row, capacity rows, address of the valid-row count) - see
    st_zero_tails."""
    _vec(table, I64, 4 * n_max, "zero_tails: table")
    _tag("zero_tails", n_max)
    _check(load().st_zero_tails(_stream(), table.data_ptr(), int(n_max)), "st_zero_tails")


def zero_(t):
    """t.zero_() for a contiguous fp32 / bf16 GPU buffer whose byte count and address are multiples of 16 (the flat gradient buffer);
    anything else goes to torch."""
    nbytes = t.numel() * t.element_size()
    if not (t.is_cuda and t.is_contiguous()) or nbytes % 16 or t.data_ptr() % 16:
        return t.zero_()
    _tag("zero", nbytes, io=(float(nbytes),))
    _check(load().st_zero(_stream(), t.data_ptr(), nbytes), "st_zero")
    return t


_NORM_BLOCKS = None


def _norm_blocks() -> int:
    global _NORM_BLOCKS
    if _NORM_BLOCKS is None:      # (a host-side query: asked once, through the untimed handle)
        _NORM_BLOCKS = int(load()._cdll.st_grad_norm_blocks())
    return _NORM_BLOCKS


def grad_norm_scratch(device):
    """Zeroed scratch of st_grad_norm (block partials + the ticket): allocate once per gradient buffer."""
    return torch.zeros(_norm_blocks() + 1, dtype=F32, device=device)


def _scalars(who, *pairs):
    for t, nm in pairs:
        if t is not None and not (t.is_cuda and t.dtype == F32 and t.numel() == 1):
            raise ValueError("%s: %s must be an fp32 scalar on the GPU" % (who, nm))


def _grad_norm(who, g, scratch, out, step, guard, win, grad_scale):
    """st_grad_norm for the three wrappers below: ``who`` names the wrapper in messages and labels the launch for bench.py."""
    _vec(g, F32, 0, who + ": g")
    if g.numel() % 4:
        raise ValueError("%s: g must hold a multiple of 4 elements" % who)
    _vec(scratch, F32, _norm_blocks() + 1, "scratch")
    _scalars(who, (out, "out"), (step, "step"))
    if guard is not None:
        _dev(guard, F32, (2,), who + ": guard")
    if win is not None:
        _dev(win, F32, (4,), who + ": win")
    _tag(who, g.numel(), io=(4.0 * g.numel(),))
    _check(load().st_grad_norm(_stream(), g.data_ptr(), g.numel(), scratch.data_ptr(), out.data_ptr(), _p(step), float(grad_scale),
                               _p(guard), _p(win)), "st_grad_norm")
    return out


def grad_norm(g, scratch, out, step=None, grad_scale=1.0):
    """out (fp32 scalar tensor) = grad_scale * ||g||_2 over the flat fp32 buffer g; step (fp32 scalar tensor, optional) += 1 -
    see st_grad_norm."""
    return _grad_norm("grad_norm", g, scratch, out, step, None, None, grad_scale)


def grad_norm_guard(g, scratch, out, step, guard, grad_scale=1.0):
    """grad_norm with a verdict (st_grad_norm's guard): out = grad_scale * ||g||_2; a finite norm advances ``step`` and clears
    guard[0], a non-finite one leaves ``step`` alone, sets guard[0] = 1 and counts up guard[1].  guard: fp32 [2] on the GPU."""
    if step is None or guard is None:
        raise ValueError("grad_norm_guard: step and guard are required")
    return _grad_norm("grad_norm_guard", g, scratch, out, step, guard, None, grad_scale)


def grad_norm_win(g, scratch, out, step, guard, win, grad_scale=1.0):
    """grad_norm_guard over a window (st_grad_norm's win): out = grad_scale * ||g||_2 / win[0]; guard (fp32 [2]) may be None -
    then ``step`` always advances; with a guard a denominator win[0] <= 0 is a bad verdict as well."""
    if step is None or win is None:
        raise ValueError("grad_norm_win: step and win are required")
    return _grad_norm("grad_norm_win", g, scratch, out, step, guard, win, grad_scale)


def cast_bf16(src, dst):
    _vec(src, F32, 0, "cast_bf16: src"), _vec(dst, BF16, src.numel(), "cast_bf16: dst")
    if dst.numel() != src.numel():
        raise ValueError("cast_bf16: dst holds %d elements, src %d" % (dst.numel(), src.numel()))
    _tag("cast_bf16", src.numel(), io=(src, dst))
    _check(load().st_cast_bf16(_stream(), src.data_ptr(), dst.data_ptr(), src.numel()), "st_cast_bf16")
    return dst


def _adam_clip(who, p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale, found_inf, avg, decay, decay_warmup, win):
    """st_adam_clip for the three wrappers below: ``who`` names the wrapper in messages and labels the launch for bench.py."""
    n = p.numel()
    for t, k, nm in ((p, n, "p"), (g, n, "g"), (m, n, "m"), (v, n, "v"), (lr, 1, "lr"), (step, 1, "step"), (gnorm, 1, "gnorm"),
                     (found_inf, 1, "found_inf"), (avg, n, "avg")):
        _vec(t, F32, k, nm)
        if t is not None and t.numel() != k:
            raise ValueError("%s: %s holds %d elements, expected %d" % (who, nm, t.numel(), k))
    if win is not None:
        _dev(win, F32, (4,), who + ": win")
    if n % 4:
        raise ValueError("%s: the buffers must hold a multiple of 4 elements" % who)
    if avg is not None and not 0.0 <= float(decay) <= 1.0:
        raise ValueError("%s: decay must lie in [0, 1], got %r" % (who, decay))
    _tag(who, n, io=((32.0 if avg is None else 40.0) * n,))      # p, g, m, v read; p, m, v, g written (fp32); + avg read and written
    _check(load().st_adam_clip(_stream(), n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr.data_ptr(),
                               step.data_ptr(), _p(gnorm), float(max_norm), float(beta1), float(beta2), float(eps),
                               float(grad_scale), _p(found_inf), _p(avg), float(decay), int(bool(decay_warmup)), _p(win)),
           "st_adam_clip")


def adam_clip(p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale=1.0):
    """In place: g *= grad_scale * min(1, max_norm / (gnorm + 1e-6)); (p, m, v) <- Adam(p, g, m, v; lr, step).  lr / step /
    gnorm are 0-dim fp32 device tensors (gnorm None: no clipping); grad_scale: see st_adam_clip (1 / world behind a summing
    all-reduce)."""
    _adam_clip("adam_clip", p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale, None, None, 0.0, False, None)


def adam_clip_avg(p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale=1.0, found_inf=None, avg=None,
                  decay=0.999, decay_warmup=True):
    """adam_clip plus (st_adam_clip's found_inf / avg): found_inf (fp32 device scalar or None) - non-zero: nothing is written; avg
    (fp32 [n] or None) - avg += w * (p_new - avg), w = 1 - decay, or with decay_warmup 1 - min(decay, (1 + step) / (10 + step))."""
    _adam_clip("adam_clip_avg", p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale, found_inf, avg, decay,
               decay_warmup, None)


def adam_clip_win(p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, win, grad_scale=1.0, found_inf=None, avg=None,
                  decay=0.999, decay_warmup=True):
    """adam_clip_avg over a window (st_adam_clip's win): the gradient is also divided by win[0] (win: fp32 [4]) and g is left
    holding ZEROS; under a non-zero found_inf the zeros are all that is written."""
    if win is None:
        raise ValueError("adam_clip_win: win is required")
    _adam_clip("adam_clip_win", p, g, m, v, lr, step, gnorm, max_norm, beta1, beta2, eps, grad_scale, found_inf, avg, decay,
               decay_warmup, win)


def swap_(a, b):
    """Exchange the contents of two fp32 buffers of equal size in place (st_swap_f32), one launch."""
    _vec(a, F32, 0, "swap_: a"), _vec(b, F32, a.numel(), "swap_: b")
    if a.numel() != b.numel() or a.numel() % 4:
        raise ValueError("swap_: the buffers must hold the same multiple of 4 elements, got %d and %d" % (a.numel(), b.numel()))
    if a.data_ptr() % 16 or b.data_ptr() % 16:
        raise ValueError("swap_: the buffers must be 16-byte aligned")
    lo, hi = sorted((a.data_ptr(), b.data_ptr()))
    if a.numel() and lo + 4 * a.numel() > hi:
        raise ValueError("swap_: the buffers overlap")
    _tag("swap", a.numel(), io=(16.0 * a.numel(),))
    _check(load().st_swap_f32(_stream(), a.data_ptr(), b.data_ptr(), a.numel()), "st_swap_f32")


# ---- gradient accumulation over micro-batches: the window's state in device memory ----------------------------------------------
def accum_note(sums, d, win, out):
    """One micro-batch joins the window (st_accum_note): win[1] += sums[0], win[2] += sums[3] * sums[1], win[3] += 1,
    win[0] += d (d None: win[0] = 1); out[0] = sums[0] / d, the micro-batch's own loss.  sums: the fp32 [4] of ce_smooth_fwd run
    with a denominator of 1; d: a 1-element fp32 device tensor (a view into sums is fine) or None; win: fp32 [4]."""
    _dev(sums, F32, (4,), "accum_note: sums"), _dev(win, F32, (4,), "accum_note: win")
    _scalars("accum_note", (d, "d"), (out, "out"))
    if out is None:
        raise ValueError("accum_note: out is required")
    if d is not None and not d.is_contiguous():
        raise ValueError("accum_note: d must be contiguous")
    _tag("accum_note", 1)
    _check(load().st_accum_note(_stream(), sums.data_ptr(), _p(d), win.data_ptr(), out.data_ptr()), "st_accum_note")
    return out


def window_close(win, out):
    """out (fp32 [4]) = (win[1] / win[0], win[2] / win[0], win[0], win[3]): the window's loss, plain NLL, denominator and
    micro-batch count; then win = 0 (st_window_close)."""
    _dev(win, F32, (4,), "window_close: win"), _dev(out, F32, (4,), "window_close: out")
    if win.data_ptr() == out.data_ptr():
        raise ValueError("window_close: win and out must be different buffers")
    _tag("window_close", 1)
    _check(load().st_window_close(_stream(), win.data_ptr(), out.data_ptr()), "st_window_close")
    return out


# ---- forward-only validation: per-row loss / NLL / arg-max hit and the epoch accumulator ----------------------------------------
F64 = torch.float64


def _eval_arg(who, t, dtype, shape, name, optional=False):
    """The FORM of an argument: a contiguous tensor of ``dtype`` and exactly ``shape`` (an extent of None: any), or None for an
    optional one - ValueError naming the argument, whatever device it lives on (the device comes after every form: _eval_gpu)."""
    if t is None:
        if optional:
            return
        raise ValueError("%s: %s is required" % (who, name))
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.dim() != len(shape)
            or any(w is not None and w != n for w, n in zip(shape, t.shape))):
        raise ValueError("%s: %s must be a contiguous %s tensor of shape %s (None = any extent), got %s" % (
            who, name, dtype, list(shape), (t.dtype, tuple(t.shape), t.stride()) if isinstance(t, torch.Tensor) else type(t).__name__))


def _eval_gpu(who, **tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise RuntimeError(_NO_GPU % ("%s: %s" % (who, name)))


def ce_eval_fwd(logits, target, ignore_index, confidence, smooth, zero_col, rows, V=None, index=None):
    """rows (f32 [R, 4]) = per logits row {criterion numerator, plain NLL, 1 if the arg-max over the first V columns is the
    target, state} - see st_ce_eval_fwd.  logits f32 [R, ldl] with ldl >= V (unit column stride); V: the TRUE vocabulary
    (None: every column); index: row r's target is target.view(-1)[index[r]].  (confidence, smooth, zero_col) as
    ce_smooth_fwd; (1, 0, -1) is the plain loss.  A target outside [0, V) that is not ignore_index is counted, never followed."""
    who = "ce_eval_fwd"
    if not isinstance(logits, torch.Tensor) or logits.dtype != F32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("%s: logits must be an f32 row matrix with unit column stride" % who)
    R, ldl = logits.shape[0], logits.stride(0)
    V = logits.shape[1] if V is None else int(V)
    if not 0 < V <= logits.shape[1] or (R > 1 and ldl < V):
        raise ValueError("%s: V = %d must lie in [1, %d]: ldl >= V (logits has %d columns, leading dimension %d)"
                         % (who, V, logits.shape[1], logits.shape[1], ldl))
    if int(zero_col) >= V:
        raise ValueError("%s: zero_col = %d must be below V = %d (negative: none)" % (who, int(zero_col), V))
    if not isinstance(target, torch.Tensor) or target.dtype != I64 or not target.is_contiguous() or (index is None and target.numel() < R):
        raise ValueError("%s: target must be a contiguous int64 tensor%s" % (who, "" if index is not None else " of at least R = %d elements" % R))
    _eval_arg(who, rows, F32, (R, 4), "rows")
    _eval_arg(who, index, I64, (R,), "index", optional=True)
    _eval_gpu(who, logits=logits, target=target, rows=rows, index=index)
    _tag("ce_eval_fwd", R, V, 0, io=(4.0 * R * V, 24.0 * R))
    _check(load().st_ce_eval_fwd(_stream(), logits.data_ptr(), ldl, R, V, target.data_ptr(), _p(index), int(ignore_index),
                                 float(confidence), float(smooth), int(zero_col), rows.data_ptr()), "st_ce_eval_fwd")
    return rows


def eval_note(rows, acc, last, denom=None):
    """One batch joins the epoch (st_eval_note): the rows of ce_eval_fwd are summed in a fixed order in fp64 and ADDED into
    acc (f64 [8]: loss numerator, loss denominator, NLL sum, tokens, hits, batches, stray labels, spare); last (f32 [4]) = this
    batch's (loss, nll, accuracy, tokens).  denom (1-element f32 device tensor or None): the batch's loss denominator instead
    of its token count."""
    who = "eval_note"
    _eval_arg(who, rows, F32, (None, 4), "rows")
    _eval_arg(who, acc, F64, (8,), "acc")
    _eval_arg(who, last, F32, (4,), "last")
    _eval_arg(who, denom, F32, (1,), "denom", optional=True)
    _eval_gpu(who, rows=rows, acc=acc, last=last, denom=denom)
    _tag("eval_note", rows.shape[0], io=(16.0 * rows.shape[0],))
    _check(load().st_eval_note(_stream(), rows.data_ptr(), rows.shape[0], _p(denom), acc.data_ptr(), last.data_ptr()), "st_eval_note")
    return last


def probe_tr16(inp, out):
    _check(load().st_probe_tr16(_stream(), inp.data_ptr(), out.data_ptr()), "st_probe_tr16")
    return out


def probe_mfma(A, Bt, D):
    _check(load().st_probe_mfma(_stream(), A.data_ptr(), Bt.data_ptr(), D.data_ptr()), "st_probe_mfma")
    return D

"""Helpers of the kernel tests: a metric that can see ONE wrong row, and guard bands around outputs (and operands).

The whole-tensor relative L2 norm of ``check`` cannot see a localised error at the shapes where the kernels change code path: the
last of 24,700 rows never written moves it by 6.4e-3, below the 1e-2 it is held to (tests/test_local_check_cpu.py keeps these
figures as assertions).  ``check_local`` applies the same kind of bound to every row and every column on its own;
``Guarded`` puts an output inside a larger buffer filled with a pattern no result can equal - the view included - and
checks, bit for bit, that everything the kernel must not write still holds it.  Where the bounds come from:
tests/LOCAL_BOUNDS.md.
"""
import torch

FLOOR = 0.25


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def local_figures(got, ref, floor=FLOOR, own_rows=False):
    """The per-row / per-column (2-D and up: flattened to [-1, last]) or per-element (1-D) error ratios, fp64 on the CPU:
    ``e / max(n, floor * s)`` with e the norm of the difference over the row, n the reference's norm over it and s the
    root-mean-square of those norms.  A row whose reference is small (or zero) is judged against a quarter of the typical
    row.  own_rows: every ROW of a matrix against its own reference norm alone, without the floor (a row whose reference is zero
    must then be zero; columns keep the floor) - for outputs whose rows span orders of magnitude, where a wrong small row is
    invisible to the floor.  Returns a list of (axis name, ratios)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, "shapes differ: got %s, reference %s" % (tuple(got.shape), tuple(ref.shape))
    if got.dim() <= 1:
        got, ref = got.reshape(-1), ref.reshape(-1)
        s = ref.pow(2).mean().sqrt() if ref.numel() else ref.sum()
        return [("element", (got - ref).abs() / torch.maximum(ref.abs(), floor * s).clamp_min(1e-300))]
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    out = []
    for name, dim in (("row", 1), ("column", 0)):
        e, n = (got - ref).norm(dim=dim), ref.norm(dim=dim)
        s = n.pow(2).mean().sqrt() if n.numel() else n.sum()
        out.append((name, e / torch.maximum(n, (0.0 if own_rows and name == "row" else floor) * s).clamp_min(1e-300)))
    return out


def check_local(got, ref, tol_local, what, floor=FLOOR, own_rows=False):
    """Every row and every column (1-D: every element) of ``got`` within ``tol_local`` of the reference, relative to
    max(its own reference norm, floor * the typical one); own_rows: rows relative to their own norm alone.  The failure message names the worst row / column, the row's index
    modulo the tile heights, how many fail and the worst ratio.  The figures are printed either way (pytest -s shows them)."""
    figs = local_figures(got, ref, floor, own_rows)
    bad = []
    for name, ratio in figs:
        if not ratio.numel():
            continue
        fails = ~(ratio <= tol_local)                       # (a NaN ratio fails)
        worst = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
        print("local %s: worst %s %d ratio %.3e (bound %.1e)" % (what, name, worst, float(ratio[worst]), tol_local))
        if bool(fails.any()):
            idx = torch.nonzero(fails).flatten()
            msg = "%d of %d %ss fail, worst %s %d: ratio %.3e > %.1e" % (idx.numel(), ratio.numel(), name, name, worst,
                                                                          float(ratio[worst]), tol_local)
            if name != "column":
                msg += " (index mod 32 / 64 / 96 / 128 = %d / %d / %d / %d; first failing %d, last %d)" % (
                    worst % 32, worst % 64, worst % 96, worst % 128, int(idx[0]), int(idx[-1]))
            bad.append(msg)
    if bad:
        raise AssertionError("%s: local bound violated: %s" % (what, "; ".join(bad)))
    return figs


def check(got, ref, tol, what, tol_local=None):
    """Whole-tensor relative L2 norm within ``tol`` and no non-finite value; with ``tol_local`` also check_local."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert torch.isfinite(got).all(), "%s: non-finite output" % what
    r = rel(got, ref)
    if r > tol:
        err = (got - ref).abs()
        idx = torch.nonzero(err == err.max())[0].tolist()
        raise AssertionError("%s: rel-L2 %.3e > %.1e; max |err| %.4g at %s (got %.5g, ref %.5g)"
                             % (what, r, tol, err.max().item(), idx, got[tuple(idx)].item(), ref[tuple(idx)].item()))
    if tol_local is not None:
        check_local(got, ref, tol_local, what)


_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_INT_FILL = {torch.uint8: 0xA5, torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}


class Guarded:
    """A [rows, cols] output window inside a (rows + 2 pad_rows) x (pad_lo + cols + pad_hi) buffer that is filled
    completely - the window too - with NaN (floating types) or a fixed bit pattern (integer types).  ``view`` is the strided
    window; with ``pad_cols=(0, 0)`` it is contiguous (for wrappers that demand that) and only row guards remain.  The column
    pads must be multiples of 8 elements: the kernels require ld % 8 == 0 and 16-byte aligned rows.  ``shape``: the window
    seen under another shape (contiguous windows only: a [L, n, S, W] cache is L n S rows of W)."""

    def __init__(self, rows, cols, dtype, device, pad_rows=3, pad_cols=(64, 64), fill=None, shape=None):
        lo, hi = pad_cols
        assert lo % 8 == 0 and hi % 8 == 0, "column pads must be multiples of 8 elements"
        assert (pad_rows * (lo + cols + hi)) % 8 == 0, "the window must start 16-byte aligned"
        self.rows, self.cols, self.pad_rows, self.lo = rows, cols, pad_rows, lo
        if fill is None:
            fill = float("nan") if dtype.is_floating_point else _INT_FILL[dtype]
        self.buf = torch.full((rows + 2 * pad_rows, lo + cols + hi), fill, dtype=dtype, device=device)
        self.window = self.buf[pad_rows:pad_rows + rows, lo:lo + cols]
        self.view = self.window
        if shape is not None:
            assert (lo, hi) == (0, 0), "only a contiguous window can be reshaped"
            self.view = self.window.view(*shape)
        self._fill_bits = self._bits(torch.full((1, 1), fill, dtype=dtype))[0, 0].item()

    @classmethod
    def vec(cls, n, dtype, device, pad=64, fill=None):
        """A contiguous [n] vector with ``pad`` guard elements on either side."""
        gd = cls(1, n, dtype, device, pad_rows=0, pad_cols=(pad, pad), fill=fill)
        gd.view = gd.window[0]
        return gd

    @staticmethod
    def _bits(t):
        return t.view(_BITS[t.element_size()])

    def _dirty(self):
        return self._bits(self.buf) != self._fill_bits

    def assert_intact(self, what):
        """Everything outside the window still holds the fill, bit for bit."""
        dirty = self._dirty()
        r0, r1, c0, c1 = self.pad_rows, self.pad_rows + self.rows, self.lo, self.lo + self.cols
        dirty[r0:r1, c0:c1] = False
        if not bool(dirty.any()):
            return
        dirty = dirty.cpu()
        regions = (("rows above", dirty[:r0]), ("rows below", dirty[r1:]), ("columns left", dirty[r0:r1, :c0]),
                   ("columns right", dirty[r0:r1, c1:]))
        hits = []
        for name, reg in regions:
            if bool(reg.any()):
                r, c = torch.nonzero(reg)[0].tolist()
                base_r = {"rows above": -r0, "rows below": self.rows}.get(name, 0)
                base_c = {"columns left": -c0, "columns right": self.cols}.get(name, -c0)
                hits.append("%s: %d elements, first at row %d column %d of the window" % (name, int(reg.sum()), r + base_r, c + base_c))
        raise AssertionError("%s: written outside the output window - %s" % (what, "; ".join(hits)))

    def assert_untouched(self, rows_mask, what):
        """The window rows selected by ``rows_mask`` (bool [rows]: rows that belong to no utterance, which the kernel's contract
        says it never writes) still hold the fill, bit for bit."""
        rows_mask = torch.as_tensor(rows_mask, dtype=torch.bool).cpu()
        assert rows_mask.numel() == self.rows
        dirty = self._dirty()[self.pad_rows:self.pad_rows + self.rows, self.lo:self.lo + self.cols].cpu()[rows_mask]
        if bool(dirty.any()):
            r, c = torch.nonzero(dirty)[0].tolist()
            row = int(torch.nonzero(rows_mask).flatten()[r])
            raise AssertionError("%s: a row the kernel must not write was written - %d elements in %d rows, first at row %d column %d"
                                 % (what, int(dirty.sum()), int(dirty.any(1).sum()), row, c))


def guarded_like(t, device, pad_rows=3, pad_cols=(64, 64)):
    """Guarded window of t's shape and dtype (1-D: Guarded.vec; 3-D and up: contiguous, row guards only)."""
    if t.dim() == 1:
        return Guarded.vec(t.numel(), t.dtype, device)
    if t.dim() == 2:
        return Guarded(t.shape[0], t.shape[1], t.dtype, device, pad_rows=pad_rows, pad_cols=pad_cols)
    rows = t.numel() // t.shape[-1]
    return Guarded(rows, t.shape[-1], t.dtype, device, pad_rows=pad_rows, pad_cols=(0, 0), shape=tuple(t.shape))


def guarded_input(t, device, pad_rows=3, pad_cols=(64, 64)):
    """The mirror for operands: a strided view holding ``t`` inside a wider buffer whose surroundings are NaN - a read outside
    the window that reaches the arithmetic shows up as a non-finite output."""
    gd = guarded_like(t, device, pad_rows, pad_cols)
    gd.view.copy_(t)
    return gd.view

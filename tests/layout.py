"""Operand layouts for the layout tests (tests/test_operand_layouts.py): a plain helper module.

Every parity test of the suite hands the library freshly allocated, contiguous, 256-byte aligned tensors.  `window` builds the
other layouts the C ABI accepts - a row stride wider than the columns, a column offset, a pointer one float into an aligned
buffer - inside a buffer whose every other float is one fixed NaN bit pattern:

  - a kernel that READS a float outside its logical operand into a result produces a NaN (tests/util.py:assert_close fails on NaN;
    `no_nan` says so directly);
  - a kernel that WRITES a float outside its logical output changes the pattern, and `check()` compares bit for bit.
"""
import dataclasses

import torch

SENTINEL = 0x7FC0BEEF          # a quiet NaN with a recognisable payload (int32 view: 2143338223)


def _fill(buf_i32, sentinel):
    buf_i32.fill_(sentinel - (1 << 32) if sentinel >= (1 << 31) else sentinel)


def window(t, *, ld_extra=0, col_off=0, guard_rows=1, sentinel=SENTINEL, device=None):
    """Copies the 2-D row operand `t` (rows, C) - or, for an output, takes its shape `(rows, C)` and leaves the interior at the
    sentinel too, so an element the kernel never wrote reads back as NaN - into a buffer of (rows + 2 * guard_rows) rows of
    C + ld_extra floats: col_off columns to the left of the operand, ld_extra - col_off to the right, guard_rows rows before and after.
    Returns (view, check): view.stride(0) == C + ld_extra, view.stride(1) == 1; check() asserts that every float outside `view`
    still holds the sentinel, bit for bit.  The buffer base is at least 64-byte aligned (torch), so the view's pointer is 16-byte
    aligned iff (guard_rows * (C + ld_extra) + col_off) % 4 == 0."""
    if torch.is_tensor(t):
        rows, c = t.shape
        device = t.device if device is None else device
    else:
        rows, c = t
    assert 0 <= col_off <= ld_extra and guard_rows >= 0
    ld = c + ld_extra
    raw = torch.empty((rows + 2 * guard_rows, ld), dtype=torch.int32, device=device)
    _fill(raw, sentinel)
    view = raw.view(torch.float32)[guard_rows:guard_rows + rows, col_off:col_off + c]
    if torch.is_tensor(t):
        view.copy_(t)
    assert view.stride(0) == ld and view.stride(1) == 1
    inside = torch.zeros(raw.shape, dtype=torch.bool, device=raw.device)
    inside[guard_rows:guard_rows + rows, col_off:col_off + c] = True
    want = raw.new_empty(())
    _fill(want, sentinel)

    def check(what=""):
        bad = (raw != want) & ~inside
        n = int(bad.sum())
        if n:
            r, col = (int(v) for v in bad.nonzero()[0])
            raise AssertionError("%s: %d float(s) outside the %dx%d window were overwritten; first at buffer row %d (window rows %d..%d), "
                                 "column %d (window columns %d..%d)" % (what, n, rows, c, r, guard_rows, guard_rows + rows - 1, col,
                                                                       col_off, col_off + c - 1))

    check.raw = raw
    return view, check


def window_batched(t, *, batch_extra=4, lead=0, guard=1, sentinel=SENTINEL, device=None):
    """The batch-stride form for planar / 4-D / 5-D operands: every batch item of `t` (or of the shape `t`) stays dense, item b starts
    at b * (item floats + batch_extra) + lead floats into its slab, with `guard` slabs before and after.  Returns (view, check)."""
    shape = tuple(t.shape) if torch.is_tensor(t) else tuple(t)
    item = 1
    for s in shape[1:]:
        item *= s
    flat = t.reshape(shape[0], item) if torch.is_tensor(t) else (shape[0], item)
    v2, check = window(flat, ld_extra=batch_extra, col_off=lead, guard_rows=guard, sentinel=sentinel, device=device)
    strides, acc = [], 1
    for s in reversed(shape[1:]):
        strides.append(acc)
        acc *= s
    view = v2.as_strided(shape, (v2.stride(0),) + tuple(reversed(strides)), v2.storage_offset())
    return view, check


def no_nan(t, what=""):
    assert not bool(torch.isnan(t).any()), "%s: NaN in the result - a float outside an operand's window was read into it" % what


def aligned16(t):
    return t.data_ptr() % 16 == 0


@dataclasses.dataclass(frozen=True)
class LayoutCase:
    """One row of the case table: which entry point, which layout class (L1 wide / L2 alias / L3 ragged / refusal), the (ld_extra, col_off)
    of every windowed operand, and which variant the library is expected to run (a schedule number, "scalar epilogue", "refused", ...)."""
    entry: str
    layout: str
    operands: dict
    expect: str
    test: str = ""

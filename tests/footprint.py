"""Footprint harness: every tensor argument of a kernel call is a *window* into a larger allocation ("slab").

The model calls the C ABI (include/lkgd_hip.h) on views - column thirds of a QKV matrix, a frame slice of a token matrix - that
lkgd_amd/replay.py packs side by side in one arena, so the bytes before a tensor, after its last row and in the ``ld - width``
gap of every row belong to another live tensor.  A window reproduces that:

    slab rows   [0, guard)                  guard rows before        |
                [guard, guard + rows)       [col0 gap | logical window [rows, width] | gap]      row stride ld
                [guard + rows, + guard)     guard rows after         |

* output windows: the slab holds a fixed, non-repeating byte pattern, the logical window NaN.  After the call every byte outside
  the logical window must still be the pattern (:meth:`Windows.check_guards`), and no NaN may be left inside.
* input windows: guards and gaps hold NaN (int32 tables: an index far out of range).  The result must be finite, meet the
  tolerance of the op's own parity test against the fp32 reference, and equal the result of the same call on compact,
  exactly-sized copies (:func:`run_case`) - bit for bit wherever the program that runs does not depend on ``ld``.
* in-place windows: the data sits between pattern guards.

Every byte a kernel is handed, and every byte a whole tile of overrun could reach, is ordinary mapped memory of the same
allocation: nothing here can fault a device.  The harness runs on any torch device; tests/test_footprint_gpu.py checks on CPU
tensors, with deliberately misbehaving stand-in "kernels", that each of the assertions bites.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import torch

#: guard rows before and after every window.  At least the tallest tile any program uses for an operand: the GEMM programs tile
#: rows by 128 (TM in gemm_common.h), 192 / 256 (gemm_wide.hip, gemm_rowpanel.hip, gemm_resw.hip, gemm_stream.hip), the attention
#: programs by 64 / 128 query rows and 64-key stages (attn_spatial.hip, attn_spatial_pipe.hip), the fused blocks by 128-token
#: panels (ff_fused.hip, qkv_fused.hip) - 256 covers them all, so a full-tile overrun past either end lands inside the slab.
GUARD = 256

INT_POISON = 0x3fffff00    # an "index" no table of these tests reaches (and no entry point would accept as a row)


def pattern_bytes(n: int, device) -> torch.Tensor:
    """the slab fill: a counter pattern with period 251 (prime: no row stride of these tests is a multiple of it, so neither
    a shifted copy of a row nor of a column run reproduces it), never constant, rarely zero"""
    return ((torch.arange(n, dtype=torch.int64, device=device) * 37 + 11) % 251).to(torch.uint8)


class _Win:
    __slots__ = ("name", "slab", "view", "rows", "width", "col0", "guard", "pattern", "kind")


def _bytes2d(slab: torch.Tensor) -> torch.Tensor:
    return slab.view(torch.uint8)            # [slab rows, ld * itemsize]


class Windows:
    """factory of the tensor arguments of one call.  ``windowed=False`` hands out compact, exactly-sized tensors with the same
    contents instead (the second run of check (c))."""

    def __init__(self, device, windowed: bool = True, guard: int = GUARD):
        self.device = torch.device(device)
        self.windowed = windowed
        self.guard = guard
        self.wins: List[_Win] = []

    # ------------------------------------------------------------------------------------------------------------ builders
    def _slab(self, rows: int, width: int, dtype, pad: int, col0: int, guard: Optional[int], name: str, kind: str):
        assert pad > 0 or kind == "nogap", "a window needs a gap (pad > 0)"
        g = self.guard if guard is None else guard
        ld = col0 + width + pad
        slab = torch.empty(rows + 2 * g, ld, dtype=dtype, device=self.device)
        w = _Win()
        w.name, w.slab, w.rows, w.width, w.col0, w.guard, w.kind = name, slab, rows, width, col0, g, kind
        w.view = slab[g:g + rows, col0:col0 + width]
        w.pattern = None
        self.wins.append(w)
        return w

    def _poison(self, slab: torch.Tensor):
        if slab.dtype.is_floating_point:
            slab.fill_(float("nan"))
        else:
            slab.fill_(INT_POISON)

    def inp(self, data: torch.Tensor, pad: int = 8, col0: int = 0, guard: Optional[int] = None, name: str = "in",
            gap: bool = True) -> torch.Tensor:
        """input window holding ``data`` ([rows, width], any dtype); guards and gaps NaN / INT_POISON.  ``gap=False`` (with
        pad = 0): guard rows only, for operands whose row stride the entry point fixes."""
        assert data.dim() == 2
        if not self.windowed:
            return data.to(self.device).contiguous()
        w = self._slab(data.shape[0], data.shape[1], data.dtype, pad, col0, guard, name, "in" if gap else "nogap")
        self._poison(w.slab)
        w.view.copy_(data)
        w.kind = "in"
        return w.view

    def inp_cols(self, parts: Sequence[torch.Tensor], pad: int = 8, guard: Optional[int] = None, name: str = "cols"):
        """operands that share a matrix in the model (q | k | v, the GEGLU halves): the parts are column blocks of ONE window, so
        the neighbour of each part is another operand's real data.  Compact mode: separate contiguous tensors."""
        if not self.windowed:
            return [p.to(self.device).contiguous() for p in parts]
        whole = self.inp(torch.cat(list(parts), dim=1), pad=pad, guard=guard, name=name)
        out, c = [], 0
        for p in parts:
            out.append(whole[:, c:c + p.shape[1]])
            c += p.shape[1]
        return out

    def out(self, rows: int, width: int, dtype=torch.float16, pad: int = 8, col0: int = 0, guard: Optional[int] = None,
            name: str = "out", gap: bool = True) -> torch.Tensor:
        """output window: pattern everywhere, NaN (integers: INT_POISON) in the logical [rows, width]"""
        if not self.windowed:
            t = torch.empty(rows, width, dtype=dtype, device=self.device)
            self._poison(t)
            return t
        w = self._slab(rows, width, dtype, pad, col0, guard, name, "out" if gap else "nogap")
        b = _bytes2d(w.slab)
        w.pattern = pattern_bytes(b.numel(), self.device).reshape(b.shape)
        b.copy_(w.pattern)
        self._poison(w.view)
        w.kind = "out"
        return w.view

    def inout(self, data: torch.Tensor, pad: int = 8, col0: int = 0, guard: Optional[int] = None, name: str = "inout",
              gap: bool = True) -> torch.Tensor:
        """in-place operand: the data between pattern guards"""
        if not self.windowed:
            return data.to(self.device).clone().contiguous()
        v = self.out(data.shape[0], data.shape[1], data.dtype, pad, col0, guard, name, gap)
        v.copy_(data)
        return v

    def slab_of(self, view: torch.Tensor) -> torch.Tensor:
        for w in self.wins:
            if w.view is view:
                return w.slab
        raise KeyError("not a window of this factory")

    # -------------------------------------------------------------------------------------------------------------- checks
    def check_guards(self) -> None:
        """every byte of every output / in-place slab outside its logical window is still the pattern"""
        for w in self.wins:
            if w.pattern is None:
                continue
            b = _bytes2d(w.slab)
            isz = w.slab.element_size()
            keep = torch.ones(b.shape, dtype=torch.bool, device=b.device)
            keep[w.guard:w.guard + w.rows, w.col0 * isz:(w.col0 + w.width) * isz] = False
            bad = (b != w.pattern) & keep
            if bool(bad.any()):
                idx = bad.nonzero().cpu()
                rows = sorted(set((idx[:, 0] - w.guard).tolist()))
                cols = sorted(set((idx[:, 1] // isz - w.col0).tolist()))
                first = idx[0].tolist()
                raise AssertionError(
                    f"{w.name}: {idx.shape[0]} guard bytes written outside the [{w.rows}, {w.width}] window - rows (relative to "
                    f"the window) {rows[:12]}{'...' if len(rows) > 12 else ''}, columns {cols[:12]}"
                    f"{'...' if len(cols) > 12 else ''}; first at slab row {first[0]} byte {first[1]}: "
                    f"{int(b[first[0], first[1]])} instead of {int(w.pattern[first[0], first[1]])}")


def _finite(name: str, t: torch.Tensor) -> None:
    if t.dtype.is_floating_point:
        ok = torch.isfinite(t.float())
        assert bool(ok.all()), f"{name}: {int((~ok).sum())} non-finite elements (unwritten output or a leaked guard value)"
    else:
        assert bool((t != INT_POISON).all()), f"{name}: unwritten elements"


def run_case(case: Callable[[Windows], Dict[str, torch.Tensor]], device,
             refs: Optional[Callable[[], Dict[str, torch.Tensor]]] = None,
             close: Optional[Callable[[torch.Tensor, torch.Tensor, str], None]] = None, bitwise: bool = True,
             sync: Optional[Callable[[], None]] = None, guard: int = GUARD) -> Dict[str, torch.Tensor]:
    """``case(W)`` builds its arguments from the factory ``W``, makes the call and returns {name: output view}.  It runs twice,
    on windows and on compact copies.  Checks: guards intact; outputs finite; (b) ``close(out, refs()[name], name)``; (c) windowed
    == compact, bit for bit (``bitwise``) or through ``close``."""
    W = Windows(device, True, guard)
    got = case(W)
    if sync is not None:
        sync()
    W.check_guards()
    for name, t in got.items():
        _finite(name, t)
    if refs is not None:
        for name, r in refs().items():
            close(got[name], r, name)
    C = Windows(device, False, guard)
    compact = case(C)
    if sync is not None:
        sync()
    for name, t in got.items():
        c = compact[name]
        _finite(name + " (compact)", c)
        if bitwise:
            same = torch.equal(t.contiguous().view(torch.uint8), c.contiguous().view(torch.uint8))
            if not same:
                d = (t.double() - c.double()).abs()
                raise AssertionError(f"{name}: windowed and compact runs differ in {int((d > 0).sum())} elements "
                                     f"(max {float(d.max()):.4g}): bytes outside a logical window reached the result")
        else:
            close(t, c.cpu(), name + " windowed vs compact")
    return got

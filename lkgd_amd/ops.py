"""Torch-tensor front end of the C-ABI (device pointers + current HIP stream).  PyTorch is plumbing here: it owns
device memory and streams; all arithmetic happens in lkgd_amd/csrc kernels.  Every function raises if a tensor is not
a CUDA(HIP) tensor of the expected dtype - there is no CPU path."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import GemmDesc, check

A_PLAIN, A_CONV3X3, A_TCONV3, A_CONV3X3_C8, A_CCONV3 = 0, 1, 2, 3, 4
# the tile programs of lkgd_gemm_f16 (include/lkgd_hip.h: LKGD_GEMM_*), as lkgd_gemm_plan reports and lkgd_debug_set_gemm_variant forces them
GEMM_TILE128, GEMM_TILE256, GEMM_STREAM, GEMM_WIDE, GEMM_ROWPANEL, GEMM_RESW, GEMM_MID = 1, 2, 3, 4, 5, 6, 7
GEMM_PROGRAMS = {"tile128": GEMM_TILE128, "tile256": GEMM_TILE256, "stream": GEMM_STREAM, "wide": GEMM_WIDE,
                 "rowpanel": GEMM_ROWPANEL, "resw": GEMM_RESW, "mid": GEMM_MID}

_zeros = {}

#: when a list, every GEMM launch is bracketed by HIP events on the launch stream and (start, end, algorithmic_flop)
#: is appended (bench.py's live roofline measurement); None = off
GEMM_EVENTS = None

#: lkgd_amd.replay.Plan while THIS host thread records a kernel sequence (every launch below is then also appended to it).
#: Thread-local: `pipeline.denoise` records by default since round 5, and two threads that drive two pipelines must not write
#: into each other's launch lists.  Read it as ``ops.PLAN`` (module __getattr__) or ``current_plan()``; set it with ``set_plan``.
import threading as _threading

_tls = _threading.local()


def current_plan():
    return getattr(_tls, "plan", None)


def set_plan(plan) -> None:
    _tls.plan = plan


def __getattr__(name):
    if name == "PLAN":
        return current_plan()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _L():
    """the C-ABI library, or its recording stand-in while this thread records a plan"""
    plan = getattr(_tls, "plan", None)
    return plan.lib if plan is not None else _lib.lib()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def zeros_page(device) -> torch.Tensor:
    key = (device.type, device.index)
    z = _zeros.get(key)
    if z is None:
        z = torch.zeros(256, dtype=torch.float16, device=device)
        _zeros[key] = z
    return z


SPLITK_WORKSPACE_BYTES = 256 << 20


def splitk_workspace(device) -> torch.Tensor:
    """fp32 scratch for the split-K partial sums of few-row GEMMs; one per device and HOST THREAD: a GEMM and its reduce pass
    are two launches of one C call, stream-ordered against everything this thread enqueues - but a second host thread
    launching on the same stream could slip its own split GEMM between them (tests/thread_world.py runs ranks as threads).
    Kept in thread-local storage: a thread's 256 MB go back to the allocator when the thread ends."""
    ws = getattr(_tls, "splitk_ws", None)
    if ws is None:
        ws = _tls.splitk_ws = {}
    key = (device.type, device.index)
    w = ws.get(key)
    if w is None:
        w = torch.empty(SPLITK_WORKSPACE_BYTES // 4, dtype=torch.float32, device=device)
        ws[key] = w
    return w


def _req(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _lib.LkgdHipError(f"{name}: expected a GPU tensor (lkgd_amd has no CPU path)")
    if t.dtype != dtype:
        raise _lib.LkgdHipError(f"{name}: expected {dtype}, got {t.dtype}")


def _req_latents(t: torch.Tensor, name: str = "latents") -> None:
    """the loop glue's in-place operand: a contiguous GPU tensor of fp16 or fp32 (the kernels take its bare pointer)"""
    if not t.is_cuda or t.dtype not in (torch.float16, torch.float32):
        raise _lib.LkgdHipError(f"{name} must be a GPU fp16/fp32 tensor")
    if not t.is_contiguous():
        raise _lib.LkgdHipError(f"{name} must be contiguous, got strides {tuple(t.stride())}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _ld(t: torch.Tensor) -> int:
    """row stride of a 2-D (possibly column-sliced) token matrix"""
    assert t.dim() == 2 and t.stride(1) == 1, "token matrices must be [T, C] with contiguous channels"
    return t.stride(0)


RowMap = Tuple[int, ...]   # (d1, m1, d2, md[, c0]): idx(row) = ((row // d1) * m1 + row % d2 + c0) % md


def rowmap_div(div: int) -> RowMap:
    """idx = row // div"""
    return (div, 1, 1, 1 << 30)


def rowmap_div_mod(div: int, mod: int) -> RowMap:
    """idx = (row // div) % mod"""
    return (div, 1, 1, mod)


def _gemm_family(name: str, args: tuple, flop: float) -> None:
    """one launch of the GEMM family (the GEMM and the fused kernels built on its skeleton): entry point ``name`` with ``args``
    and the current stream, ``flop`` its algorithmic FLOP.  Bracketed by events when GEMM_EVENTS is a list; while this thread
    records, the plan entry of the call carries the same ``flop`` (Plan.run(gemm_events) brackets it on replay)."""
    plan = current_plan()
    fn = getattr(plan.lib if plan is not None else _lib.lib(), name)
    ev = GEMM_EVENTS
    if ev is None:
        rc = fn(*args, _stream())
    else:
        s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_ev.record()
        rc = fn(*args, _stream())
        e_ev.record()
        ev.append((s_ev, e_ev, float(flop)))
    if plan is not None:
        plan.gemm_family(flop)
    check(rc, name)


_FAKE_PTR = 1 << 12     # gemm_plan off the device: a non-NULL, 16-byte aligned stand-in for buffers the query never dereferences


def _gemm_desc(a0, w, out, *, M, N, K, bias=None, a1=None, csplit=None, mode=A_PLAIN, Cin=0, conv=None, tconv=None,
               rowbias=None, rowmap=None, res1=None, r1=1.0, res2=None, r2=1.0, s_acc=1.0, geglu=0, colstats=0, ln=None,
               cconv=None, plan_cus=None):
    """the lkgd_gemm_desc of a :func:`gemm` call.  ``plan_cus`` None: for launching (device tensors, the workspace and the column
    sum buffer are allocated); an int: for :func:`gemm_plan` - the same fields and pointer classes, nothing allocated."""
    launch = plan_cus is None
    req = _req if launch or a0.is_cuda else (lambda t, dtype, name: None)
    req(a0, torch.float16, "a0"); req(w, torch.float16, "w"); req(out, torch.float16, "out")
    d = GemmDesc()
    d.a0, d.w, d.out = a0.data_ptr(), w.data_ptr(), out.data_ptr()
    d.a1 = _ptr(a1)
    d.bias = _ptr(bias)
    d.zeros = zeros_page(a0.device).data_ptr() if a0.is_cuda else _FAKE_PTR
    d.M, d.N, d.K = M, N, K
    d.lda0 = _ld(a0)
    d.lda1 = _ld(a1) if a1 is not None else 0
    d.mode, d.Cin = mode, Cin
    if mode == A_PLAIN:
        d.csplit = csplit if csplit is not None else K
    else:
        d.csplit = csplit if csplit is not None else Cin
    if conv is not None:          # (Hout, Wout, Hin, Win, stride, ups[, pad_off])
        d.Hout, d.Wout, d.Hin, d.Win, d.stride, d.ups = conv[:6]
        d.pad_off = conv[6] if len(conv) > 6 else 0
    if tconv is not None:      # (F, HW) or (F, HW, Floc, f_off) under frame sharding
        d.F, d.HW = tconv[0], tconv[1]
        d.Floc, d.f_off = (tconv[2], tconv[3]) if len(tconv) == 4 else (tconv[0], 0)
    if cconv is not None:      # (Floc, H, W): A_CCONV3 - a0 holds Floc + 2 frames per batch entry, two context frames first
        d.Floc, d.F, d.f_off = cconv[0], cconv[0] + 2, 0
        d.Hout = d.Hin = cconv[1]
        d.Wout = d.Win = cconv[2]
        d.stride, d.ups, d.pad_off, d.HW = 1, 0, 0, cconv[1] * cconv[2]
    if rowbias is not None:
        req(rowbias, torch.float16, "rowbias")
        d.rowbias, d.ldrb = rowbias.data_ptr(), _ld(rowbias)
        d.rb_d1, d.rb_m1, d.rb_d2, d.rb_md = rowmap[:4]
        d.rb_c0 = rowmap[4] if len(rowmap) > 4 else 0
    if res1 is not None:
        req(res1, torch.float16, "res1")
        d.res1, d.ldr1 = res1.data_ptr(), _ld(res1)
    if res2 is not None:
        req(res2, torch.float16, "res2")
        d.res2, d.ldr2 = res2.data_ptr(), _ld(res2)
    d.ldc = _ld(out)
    d.s_acc, d.r1, d.r2 = s_acc, r1, r2
    d.geglu = int(geglu)        # 0 off, 32 / 80 = interleave width the weights were packed with
    if M < 12288:               # few-row problems may cut K into slices (lkgd_hip.h: lkgd_gemm_desc.workspace)
        if launch or out.is_cuda:
            ws = splitk_workspace(out.device)
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        else:
            d.workspace, d.workspace_bytes = _FAKE_PTR, SPLITK_WORKSPACE_BYTES
    if ln is not None:           # LayerNorm of the A rows folded into the GEMM (lkgd_gemm_desc.ln_colsum)
        req(ln[0], torch.float32, "ln colsum")
        d.ln_colsum, d.ln_eps = ln[0].data_ptr(), float(ln[1])
    if colstats and COLSTATS and out.shape[0] == M and out.shape[1] == N:
        d.cs_rows = int(colstats)        # the tile-form choice keeps to tile rows that divide a sample
        if launch:
            blk = _lib.lib().lkgd_gemm_colstats_block(C.byref(d))      # (a host query: nothing to record)
        else:
            info = _lib.GemmPlanInfo()
            blk = info.colstats_block if _lib.lib().lkgd_gemm_plan(C.byref(d), int(plan_cus), C.byref(info)) == 0 else 0
        if blk > 0 and int(colstats) % blk == 0:
            if launch:
                buf = torch.empty((M + blk - 1) // blk, N // 2, 2, dtype=torch.float32, device=out.device)   # channel pairs
                d.colstats = buf.data_ptr()
                out._lkgd_colstats = (buf, blk, out._version)      # see _stats_from_cols: void once `out` is written again
            else:
                d.colstats = _FAKE_PTR
        else:
            d.cs_rows = 0                # no sums attached: the tile-form choice is not restricted either
    return d


def gemm(a0: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, M: int, N: int, K: int,
         bias: Optional[torch.Tensor] = None, a1: Optional[torch.Tensor] = None, csplit: Optional[int] = None,
         mode: int = A_PLAIN, Cin: int = 0, conv: Optional[Tuple[int, int, int, int, int, int]] = None,
         tconv: Optional[Tuple[int, int]] = None, rowbias: Optional[torch.Tensor] = None,
         rowmap: Optional[RowMap] = None, res1: Optional[torch.Tensor] = None, r1: float = 1.0,
         res2: Optional[torch.Tensor] = None, r2: float = 1.0, s_acc: float = 1.0, geglu: int = 0,
         colstats: int = 0, ln: Optional[Tuple[torch.Tensor, float]] = None,
         cconv: Optional[Tuple[int, int, int]] = None) -> torch.Tensor:
    """out = epilogue(A(.) @ w.T) - see include/lkgd_hip.h section 1.  ``conv`` = (Hout, Wout, Hin, Win, stride, ups);
    ``tconv`` = (F, HW); ``cconv`` = (Floc, H, W) of A_CCONV3 (``a0`` = the [B * (Floc + 2) * H * W, Cin] context-prefixed rows).
    ``colstats`` = rows per GroupNorm sample (0 = off): ``out`` feeds a GroupNorm next - where the
    tile program that will run supports it and its row blocks tile the samples, the GEMM leaves the per-(row block, channel
    pair) sums of its rounded outputs and ``out`` carries them (``out._lkgd_colstats``) to :func:`groupnorm_stats`, which
    then skips its read pass over the tensor."""
    d = _gemm_desc(a0, w, out, M=M, N=N, K=K, bias=bias, a1=a1, csplit=csplit, mode=mode, Cin=Cin, conv=conv, tconv=tconv,
                   rowbias=rowbias, rowmap=rowmap, res1=res1, r1=r1, res2=res2, r2=r2, s_acc=s_acc, geglu=geglu,
                   colstats=colstats, ln=ln, cconv=cconv)
    _gemm_family("lkgd_gemm_f16", (C.byref(d),), 2.0 * M * N * (72 if mode == A_CONV3X3_C8 else K))
    return out


def gemm_plan(a0: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, cus: int = 0, **kwargs):
    """what :func:`gemm` would run for the same arguments (lkgd_gemm_plan): a ``_lib.GemmPlanInfo`` - tile program 1..7, K slices,
    tile rows x columns, colstats block, rows-through-LDS.  Nothing is launched or allocated.  ``cus`` = compute units to plan for
    (0 = the current device's); with ``cus`` given the tensors may live anywhere - on the CPU too, only their strides and the
    alignment of their addresses matter - and no GPU is needed.  The calling thread's debug knobs apply as they do to a launch."""
    if cus == 0 and not a0.is_cuda:
        raise _lib.LkgdHipError("gemm_plan: cus=0 asks the device, which needs GPU tensors (pass cus=... to plan without one)")
    d = _gemm_desc(a0, w, out, plan_cus=int(cus), **kwargs)
    info = _lib.GemmPlanInfo()
    check(_lib.lib().lkgd_gemm_plan(C.byref(d), int(cus), C.byref(info)), "lkgd_gemm_plan")
    return info


#: A/B switch of the GroupNorm statistics from the producing GEMM's epilogue (False = always the separate read pass)
COLSTATS = os.environ.get("LKGD_NO_COLSTATS", "0") != "1"


def _stats_from_cols(x0: torch.Tensor, x1: Optional[torch.Tensor], nsamples: int, rows_per_sample: int, eps: float,
                     as_sums: bool) -> Optional[torch.Tensor]:
    """(mean, rstd) - or raw sums - from the column sums the tensors' producing GEMMs attached (ops.gemm(colstats=True));
    None when a tensor carries none or its row blocks do not tile the samples"""
    if not COLSTATS:
        return None
    cs0 = getattr(x0, "_lkgd_colstats", None)
    cs1 = getattr(x1, "_lkgd_colstats", None) if x1 is not None else None
    if cs0 is None or (x1 is not None and cs1 is None):
        return None
    # the sums describe the tensor as its producing GEMM wrote it: any in-place torch op since then (the version counter
    # moves) voids them - the caller falls back to the read pass instead of normalising with stale statistics
    if cs0[2] != x0._version or (cs1 is not None and cs1[2] != x1._version):
        return None
    (b0, k0), (b1, k1) = cs0[:2], (cs1[:2] if cs1 is not None else (None, 1))
    if (rows_per_sample % k0 or rows_per_sample % k1 or 2 * b0.shape[1] != x0.shape[1] or
            (b1 is not None and 2 * b1.shape[1] != x1.shape[1]) or ((x0.shape[1] + (x1.shape[1] if x1 is not None else 0)) // 32) % 2):
        return None
    if b0.shape[0] * k0 < nsamples * rows_per_sample or (b1 is not None and b1.shape[0] * k1 < nsamples * rows_per_sample):
        return None
    out = torch.empty(nsamples, 32, 2, dtype=torch.float32, device=x0.device)
    check(_L().lkgd_groupnorm_stats_cols(b0.data_ptr(), k0, 2 * b0.shape[1], x0.shape[1], _ptr(b1), k1,
                                         2 * b1.shape[1] if b1 is not None else 0, x1.shape[1] if x1 is not None else 0,
                                         nsamples, rows_per_sample, eps, 1 if as_sums else 0, out.data_ptr(), _stream()),
          "lkgd_groupnorm_stats_cols")
    return out


def groupnorm_stats(x0: torch.Tensor, x1: Optional[torch.Tensor], nsamples: int, rows_per_sample: int,
                    eps: float) -> torch.Tensor:
    _req(x0, torch.float16, "x0")
    st = _stats_from_cols(x0, x1, nsamples, rows_per_sample, eps, False)
    if st is not None:
        return st
    c0 = x0.shape[1]
    c1 = x1.shape[1] if x1 is not None else 0
    L = _L()
    nchunks = _lib.lib().lkgd_groupnorm_chunks(rows_per_sample, c0 + c1)      # (a host query: nothing to record)
    partial = torch.empty(nsamples * nchunks * 64, dtype=torch.float32, device=x0.device)
    stats = torch.empty(nsamples, 32, 2, dtype=torch.float32, device=x0.device)
    check(L.lkgd_groupnorm_stats(x0.data_ptr(), c0, _ld(x0), _ptr(x1), c1, _ld(x1) if x1 is not None else 0,
                                 nsamples, rows_per_sample, eps, partial.data_ptr(), stats.data_ptr(), _stream()),
          "lkgd_groupnorm_stats")
    return stats


def groupnorm_sums(x0: torch.Tensor, x1: Optional[torch.Tensor], nsamples: int, rows_per_sample: int) -> torch.Tensor:
    """raw fp32 (sum, sumsq) per (sample, group) of the local rows (frame-sharded GroupNorm)"""
    _req(x0, torch.float16, "x0")
    st = _stats_from_cols(x0, x1, nsamples, rows_per_sample, 0.0, True)
    if st is not None:
        return st
    c0 = x0.shape[1]
    c1 = x1.shape[1] if x1 is not None else 0
    L = _L()
    nchunks = _lib.lib().lkgd_groupnorm_chunks(rows_per_sample, c0 + c1)      # (a host query: nothing to record)
    partial = torch.empty(nsamples * nchunks * 64, dtype=torch.float32, device=x0.device)
    sums = torch.empty(nsamples, 32, 2, dtype=torch.float32, device=x0.device)
    check(L.lkgd_groupnorm_sums(x0.data_ptr(), c0, _ld(x0), _ptr(x1), c1, _ld(x1) if x1 is not None else 0,
                                nsamples, rows_per_sample, partial.data_ptr(), sums.data_ptr(), _stream()),
          "lkgd_groupnorm_sums")
    return sums


def groupnorm_finalize(sums: torch.Tensor, count_per_group: float, eps: float) -> torch.Tensor:
    _req(sums, torch.float32, "sums")
    stats = torch.empty_like(sums)
    check(_L().lkgd_groupnorm_finalize(sums.data_ptr(), sums.shape[0], float(count_per_group), eps,
                                             stats.data_ptr(), _stream()), "lkgd_groupnorm_finalize")
    return stats


def groupnorm_finalize_parts(parts: torch.Tensor, nparts: int, part_stride: int, nsamples: int, sample_stride: int,
                              count_per_group: float, eps: float) -> torch.Tensor:
    """(mean, rstd) [nsamples, 32, 2] from the raw sums of ``nparts`` ranks inside one gathered buffer (``parts``: a float32
    view whose element r * part_stride + s * sample_stride starts rank r's sums of sample s), added in rank order"""
    _req(parts, torch.float32, "parts")
    stats = torch.empty(nsamples, 32, 2, dtype=torch.float32, device=parts.device)
    check(_L().lkgd_groupnorm_finalize_parts(parts.data_ptr(), nparts, part_stride, nsamples, sample_stride,
                                              float(count_per_group), eps, stats.data_ptr(), _stream()),
          "lkgd_groupnorm_finalize_parts")
    return stats


def groupnorm_apply(x0: torch.Tensor, x1: Optional[torch.Tensor], nsamples: int, rows_per_sample: int,
                    stats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, silu: bool,
                    out: torch.Tensor) -> torch.Tensor:
    _req(x0, torch.float16, "x0"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta")
    c0 = x0.shape[1]
    c1 = x1.shape[1] if x1 is not None else 0
    check(_L().lkgd_groupnorm_apply(x0.data_ptr(), c0, _ld(x0), _ptr(x1), c1,
                                          _ld(x1) if x1 is not None else 0, nsamples, rows_per_sample,
                                          stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1 if silu else 0,
                                          out.data_ptr(), _ld(out), _stream()), "lkgd_groupnorm_apply")
    return out


def groupnorm_apply_segments(segments, stats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, silu: bool = True) -> None:
    """GroupNorm apply (+ SiLU) over a list of row segments in ONE launch: ``segments`` = [(src [rows, C], dst [rows, C], sample)],
    each normalised with ``stats[sample]``; src / dst are row-contiguous fp16 views of equal row stride (lkgd_hip.h section 2)"""
    src0 = segments[0][0]
    C_, ld = src0.shape[1], _ld(src0)
    tab = []
    for src, dst, sample in segments:
        _req(src, torch.float16, "segment src"); _req(dst, torch.float16, "segment dst")
        if src.shape != dst.shape or src.shape[1] != C_ or _ld(src) != ld or _ld(dst) != ld:
            raise _lib.LkgdHipError("groupnorm_apply_segments: segments must be [rows, C] views of one row stride")
        tab += [src.data_ptr(), dst.data_ptr(), src.shape[0], int(sample)]
    table = torch.tensor(tab, dtype=torch.int64).to(src0.device)        # (kept alive by the caller's recording, if any)
    check(_L().lkgd_groupnorm_apply_segments(table.data_ptr(), len(segments), max(s[0].shape[0] for s in segments), C_, ld,
                                             stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1 if silu else 0, _stream()),
          "lkgd_groupnorm_apply_segments")
    return table


def groupnorm_silu(x0, x1, nsamples, rows_per_sample, gamma, beta, eps, silu=True, out=None):
    C_ = x0.shape[1] + (x1.shape[1] if x1 is not None else 0)
    if out is None:
        out = torch.empty(x0.shape[0], C_, dtype=torch.float16, device=x0.device)
    _req(x0, torch.float16, "x0"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta")
    stats = _stats_from_cols(x0, x1, nsamples, rows_per_sample, eps, False)
    if stats is not None:            # the producing GEMMs left column sums: no read pass
        return groupnorm_apply(x0, x1, nsamples, rows_per_sample, stats, gamma, beta, silu, out)
    c0 = x0.shape[1]
    c1 = x1.shape[1] if x1 is not None else 0
    L = _L()
    nchunks = _lib.lib().lkgd_groupnorm_chunks(rows_per_sample, c0 + c1)      # (a host query: nothing to record)
    partial = torch.empty(nsamples * nchunks * 64, dtype=torch.float32, device=x0.device)
    stats = torch.empty(nsamples, 32, 2, dtype=torch.float32, device=x0.device)
    check(L.lkgd_groupnorm_silu(x0.data_ptr(), c0, _ld(x0), _ptr(x1), c1, _ld(x1) if x1 is not None else 0, nsamples,
                                rows_per_sample, eps, partial.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                1 if silu else 0, out.data_ptr(), _ld(out), _stream()), "lkgd_groupnorm_silu")
    return out


def spatial_norm3d(f: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, yb: torch.Tensor,
                   tmap: torch.Tensor, out: torch.Tensor, B: int, T: int, H: int, W: int, Tz: int, sh: int, silu: bool,
                   out_batch_rows: Optional[int] = None) -> torch.Tensor:
    """CogVideoXSpatialNorm3D (+ SiLU) in one pass (include/lkgd_hip_cogvae.h): ``f`` [B*T*H*W, C] rows, ``stats`` [B, 32, 2] from
    :func:`groupnorm_stats` over T*H*W rows per sample, ``yb`` [B*Tz*(H>>sh)*(W>>sh), 2C] = conv_y | conv_b on the latent grid,
    ``tmap`` int32 [T].  ``out`` = the first output row (a [rows, C] view: of a compact matrix, or of a context-prefixed buffer
    behind its two context frames with ``out_batch_rows`` = (T + 2)*H*W)."""
    _req(f, torch.float16, "f"); _req(yb, torch.float16, "yb"); _req(out, torch.float16, "out")
    _req(stats, torch.float32, "stats"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta")
    _req(tmap, torch.int32, "tmap")
    C_ = f.shape[1]
    if tmap.numel() != T or not tmap.is_contiguous() or not stats.is_contiguous() or stats.numel() != B * 64:
        raise _lib.LkgdHipError("spatial_norm3d: tmap must be int32 [T], stats fp32 [B, 32, 2]")
    if f.shape[0] != B * T * H * W or yb.shape[1] != 2 * C_ or yb.shape[0] != B * Tz * (H >> sh) * (W >> sh) or out.shape[1] != C_:
        raise _lib.LkgdHipError("spatial_norm3d: f / yb / out shapes do not match (B, T, H, W, Tz, sh)")
    obr = T * H * W if out_batch_rows is None else int(out_batch_rows)
    check(_L().lkgd_spatial_norm3d(f.data_ptr(), _ld(f), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), yb.data_ptr(), _ld(yb),
                                   tmap.data_ptr(), out.data_ptr(), _ld(out), obr, B, T, H, W, C_, Tz, sh, 1 if silu else 0, _stream()),
          "lkgd_spatial_norm3d")
    return out


def layernorm(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
              out: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None,
              rowmap: Optional[RowMap] = None) -> torch.Tensor:
    """gamma = beta = None: normalise only (affine folded into the consuming Linear)"""
    _req(x, torch.float16, "x")
    if gamma is not None:
        _req(gamma, torch.float32, "gamma")
    T, C_ = x.shape
    if out is None:
        out = torch.empty(T, C_, dtype=torch.float16, device=x.device)
    d1, m1, d2, md = rowmap if rowmap is not None else (1, 0, 1, 1)
    check(_L().lkgd_layernorm(x.data_ptr(), _ld(x), T, C_, _ptr(gamma), _ptr(beta), eps,
                                    _ptr(rowbias), _ld(rowbias) if rowbias is not None else 0, d1, m1, d2, md,
                                    out.data_ptr(), _ld(out), _stream()), "lkgd_layernorm")
    return out


#: A/B switch of the one-launch feed-forward of the 72x128 level (False = LayerNorm + GEGLU GEMM + FF-out GEMM)
FF_FUSED = os.environ.get("LKGD_NO_FF_FUSED", "0") != "1"


#: A/B switch of the one-launch LayerNorm + QKV projection of the 72x128 level (False = LayerNorm kernel + GEMM)
LN_QKV = os.environ.get("LKGD_NO_LN_QKV", "0") != "1"


def ln_qkv_ok(T: int, N: int, C_: int) -> bool:
    """the fused kernel exists for 320 -> 960 and 640 -> 1920 and pays where its 128-token panels fill the CUs: from one full
    round at C = 640 (a CFG-parallel rank's 32 256 rows: 83 us against 109 for LayerNorm + GEMM; 16 128 rows tie), from two
    at C = 320, measured against the row-panel GEMM with the LayerNorm folded in (profiles/r05_ln_qkv_rows.txt)"""
    return LN_QKV and C_ in (320, 640) and N == 3 * C_ and T >= (30000 if C_ == 640 else 60000)


def ln_qkv(x: torch.Tensor, wstream: torch.Tensor, out: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """out[T, 3C] = W . LN(x) + b in one launch (lkgd_ln_qkv_c320 / _c640 by x's width)"""
    _req(x, torch.float16, "x"); _req(wstream, torch.float16, "wstream"); _req(out, torch.float16, "out")
    T, C_ = x.shape
    if C_ not in (320, 640):
        raise _lib.LkgdHipError("ln_qkv: 320 or 640 channels")
    _gemm_family("lkgd_ln_qkv_c320" if C_ == 320 else "lkgd_ln_qkv_c640",
                 (x.data_ptr(), _ld(x), T, wstream.data_ptr(), eps, out.data_ptr(), _ld(out)), 2.0 * T * 3 * C_ * C_)
    return out


def ff_fused_ok(C_: int, inner: int) -> bool:
    return FF_FUSED and C_ == 320 and inner == 1280


def ff_fused(x: torch.Tensor, wstream: torch.Tensor, b2: torch.Tensor, out: torch.Tensor, eps: float = 1e-5,
             rowbias: Optional[torch.Tensor] = None, rowmap: Optional[RowMap] = None, s_acc: float = 1.0,
             res2: Optional[torch.Tensor] = None, r2: float = 0.0) -> torch.Tensor:
    """out = s_acc * (FF(LN(x')) + x') + r2 * res2 with x' = x + rowbias[(row // d1) % md]  (lkgd_ff_fused_c320)"""
    _req(x, torch.float16, "x"); _req(wstream, torch.float16, "wstream"); _req(b2, torch.float32, "b2")
    _req(out, torch.float16, "out")
    if x.shape[1] != 320 or out.shape != x.shape:
        raise _lib.LkgdHipError("ff_fused: x / out must be [T, 320] token matrices of the same row count")
    if res2 is not None:
        _req(res2, torch.float16, "res2")
        if res2.shape[0] != x.shape[0]:
            raise _lib.LkgdHipError("ff_fused: res2 must hold one row per token")
    if rowbias is not None:
        _req(rowbias, torch.float16, "rowbias")
    d1, m1, d2, md = (rowmap if rowmap is not None else (1, 1, 1, 1))[:4]
    if rowbias is not None and (m1 != 1 or d2 != 1 or (len(rowmap) > 4 and rowmap[4] != 0)):
        raise _lib.LkgdHipError("ff_fused: only (row // d1) % md row maps (no c0 term)")
    # a GEMM-family launch for bench.py's roofline line: 2 T (2560 x 320 + 320 x 1280) algorithmic FLOP
    _gemm_family("lkgd_ff_fused_c320",
                 (x.data_ptr(), _ld(x), x.shape[0], _ptr(rowbias), _ld(rowbias) if rowbias is not None else 0, d1,
                  min(md, 1 << 30), wstream.data_ptr(), b2.data_ptr(), eps, s_acc, _ptr(res2),
                  _ld(res2) if res2 is not None else 0, r2, out.data_ptr(), _ld(out)),
                 2.0 * x.shape[0] * (2560 * 320 + 320 * 1280))
    return out


def attn_spatial(q, k, v, out, nbatch: int, S: int, heads: int, kv_batch_map: Optional[torch.Tensor] = None,
                 scale: float = 0.125, Sq: Optional[int] = None):
    """S = key / value rows per batch entry; Sq = query rows (defaults to S; smaller on a frame-sharded DiT rank)"""
    _req(q, torch.float16, "q"); _req(k, torch.float16, "k"); _req(v, torch.float16, "v")
    if Sq is None or Sq == S:
        check(_L().lkgd_attn_spatial(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v),
                                     out.data_ptr(), _ld(out), nbatch, S, heads, _ptr(kv_batch_map), scale,
                                     _stream()), "lkgd_attn_spatial")
    else:
        check(_L().lkgd_attn_spatial_qk(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v),
                                        out.data_ptr(), _ld(out), nbatch, Sq, S, heads, _ptr(kv_batch_map), scale,
                                        _stream()), "lkgd_attn_spatial_qk")
    return out


def attn_temporal(q, k, v, out, B: int, F: int, S: int, heads: int, kv_b_map: Optional[torch.Tensor] = None,
                  scale: float = 0.125, Fq: Optional[int] = None):
    """F = key/value frames; Fq = query frames (defaults to F; smaller under frame sharding)"""
    _req(q, torch.float16, "q"); _req(k, torch.float16, "k"); _req(v, torch.float16, "v")
    check(_L().lkgd_attn_temporal(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v),
                                        out.data_ptr(), _ld(out), B, Fq if Fq is not None else F, F, S, heads,
                                        _ptr(kv_b_map), scale, _stream()),
          "lkgd_attn_temporal")
    return out


def tattn_front(x: torch.Tensor, wpack: torch.Tensor, bqkv: Optional[torch.Tensor], out: torch.Tensor, B: int, F: int, HW: int,
                heads: int, eps: float = 1e-5, scale: float = 0.125) -> torch.Tensor:
    """out = attn1(LayerNorm(x)) without the out-projection, fused (include/lkgd_hip.h section 5b); x / out: [B*F*HW, 320]"""
    _req(x, torch.float16, "x"); _req(wpack, torch.float16, "wpack"); _req(out, torch.float16, "out")
    check(_L().lkgd_tattn_front(x.data_ptr(), _ld(x), wpack.data_ptr(), _ptr(bqkv), out.data_ptr(), _ld(out), B, F, HW, heads,
                                eps, scale, _stream()), "lkgd_tattn_front")
    return out


def tattn_block(x: torch.Tensor, wstream: torch.Tensor, bo: torch.Tensor, out: torch.Tensor, B: int, F: int, HW: int,
                rowbias: Optional[torch.Tensor] = None, rowmap: Optional[RowMap] = None, eps: float = 1e-5) -> torch.Tensor:
    """out = to_out(attn1(LayerNorm(x))) + b_o + x (+ rowbias[rowmap(row)]): LayerNorm, Q|K|V, the attention over the F frames
    of every pixel, the out-projection and the residual in one launch (lkgd_tattn_block_c320); x / out: [B*F*HW, 320]"""
    _req(x, torch.float16, "x"); _req(wstream, torch.float16, "wstream"); _req(out, torch.float16, "out")
    _req(bo, torch.float32, "bo")
    if x.shape[0] != B * F * HW or out.shape[0] != x.shape[0] or x.shape[1] != 320 or out.shape[1] != 320:
        raise _lib.LkgdHipError("tattn_block: x / out must be [B * F * HW, 320] token matrices")
    d1, m1, d2, md = rowmap[:4] if rowmap is not None else (1, 0, 1, 1)
    c0 = rowmap[4] if rowmap is not None and len(rowmap) > 4 else 0
    if rowbias is not None:
        _req(rowbias, torch.float16, "rowbias")
    # a GEMM-family launch for bench.py's roofline line (projections, out-projection, 16 x 16 attention)
    _gemm_family("lkgd_tattn_block_c320",
                 (x.data_ptr(), _ld(x), wstream.data_ptr(), bo.data_ptr(), _ptr(rowbias),
                  _ld(rowbias) if rowbias is not None else 0, d1, m1, d2, min(md, 0x7fffffff), c0, out.data_ptr(), _ld(out),
                  B, F, HW, eps),
                 2 * x.shape[0] * (960 * 320 + 320 * 320) + 4 * x.shape[0] * 16 * 320)
    return out


def tattn_block_ok(C_: int, heads: int, F: int, HW: int) -> bool:
    return TBLOCK and C_ == 320 and heads == 5 and 1 <= F <= 16


#: A/B switch of the one-launch temporal attention (False = fused front + out-projection GEMM)
TBLOCK = os.environ.get("LKGD_NO_TBLOCK", "0") != "1"


def tattn_front_ok(C_: int, heads: int, F: int, HW: int) -> bool:
    return TFRONT and C_ == 320 and heads * 64 == C_ and 1 <= F <= 16 and HW % 16 == 0


#: A/B switch of the fused temporal-attention front (False = LayerNorm, QKV GEMM and attention kernel as three launches)
TFRONT = os.environ.get("LKGD_NO_TFRONT", "0") != "1"


def attn_cross(q, k, v, out, heads: int, ncontexts: int, Lk: int, rowmap: RowMap, scale: float = 0.125):
    """rows of q against the Lk keys of context rowmap(row); k / v: [ncontexts * Lk, heads * 64] (lkgd_hip.h section 15)"""
    _req(q, torch.float16, "q"); _req(k, torch.float16, "k"); _req(v, torch.float16, "v"); _req(out, torch.float16, "out")
    d1, m1, d2, md = rowmap[:4]
    c0 = rowmap[4] if len(rowmap) > 4 else 0
    check(_L().lkgd_attn_cross(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(), _ld(out),
                               q.shape[0], heads, ncontexts, Lk, d1, m1, d2, md, c0, scale, _stream()), "lkgd_attn_cross")
    return out


def attn_dense(q, k, v, out, nbatch: int, S: int, heads: int, head_dim: int, scale: Optional[float] = None):
    """short-sequence attention with any head_dim <= 128 (lkgd_hip.h section 16): q, k, v, out [nbatch*S, heads*head_dim]"""
    _req(q, torch.float16, "q"); _req(k, torch.float16, "k"); _req(v, torch.float16, "v"); _req(out, torch.float16, "out")
    if scale is None:
        scale = head_dim ** -0.5
    check(_L().lkgd_attn_dense(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(), _ld(out),
                               nbatch, S, heads, head_dim, scale, _stream()), "lkgd_attn_dense")
    return out


def prepare_unet_input(latents: torch.Tensor, image_latents: torch.Tensor, cfg: int, sigma: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,F,4,H,W] latents (+ [cfg*B,F,4,H,W] image latents) -> channels-last tokens [cfg*B*F*H*W, 8]"""
    B, F, _, H, W = latents.shape
    _req_latents(latents)
    _req(image_latents, torch.float16, "image_latents")
    assert image_latents.is_contiguous()
    assert image_latents.shape == (cfg * B, F, 4, H, W), image_latents.shape
    if out is None:
        out = torch.empty(cfg * B * F * H * W, 8, dtype=torch.float16, device=latents.device)
    check(_L().lkgd_prepare_unet_input(latents.data_ptr(), int(latents.dtype == torch.float32),
                                             image_latents.data_ptr(), B, F, H, W, cfg, sigma, out.data_ptr(),
                                             _stream()), "lkgd_prepare_unet_input")
    return out


def cfg_euler_step(noise_tokens: torch.Tensor, latents: torch.Tensor, guidance: Optional[torch.Tensor], cfg: int,
                   sigma: float, sigma_next: float, v_prediction: bool = True) -> torch.Tensor:
    """in-place Euler update of ``latents`` [B,F,4,H,W] from channels-last noise tokens [cfg*B*F*H*W, 4]"""
    B, F, _, H, W = latents.shape
    _req_latents(latents)
    _req(noise_tokens, torch.float16, "noise_tokens")
    assert noise_tokens.is_contiguous()
    check(_L().lkgd_cfg_euler_step(noise_tokens.data_ptr(), latents.data_ptr(),
                                         int(latents.dtype == torch.float32), _ptr(guidance), B, F, H, W, cfg, sigma,
                                         sigma_next, 1 if v_prediction else 0, _stream()), "lkgd_cfg_euler_step")
    return latents


def cfg_fusion_euler_step(noise_tokens: torch.Tensor, latents: torch.Tensor, guidance: Optional[torch.Tensor],
                          weight: torch.Tensor, cfg: int, sigma: float, sigma_next: float,
                          v_prediction: bool = True) -> torch.Tensor:
    """direct-fusion Euler step (lkgd_cfg_fusion_euler_step): in-place update of ``latents`` [B,F,4,H,W] (B = 2P clips, clip
    b + P the backward partner of clip b) from channels-last noise tokens [cfg*B*F*H*W, 4]; ``weight`` fp32 [F] on the device
    (torch.linspace(1, 0, F)), ``guidance`` fp32 [F] on the device (or None when cfg == 1)"""
    B, F, _, H, W = latents.shape
    _req_latents(latents)
    _req(noise_tokens, torch.float16, "noise_tokens")
    _req(weight, torch.float32, "weight")
    if guidance is not None:
        _req(guidance, torch.float32, "guidance")
    assert noise_tokens.is_contiguous() and weight.is_contiguous()
    assert weight.numel() == F and (guidance is None or guidance.numel() == F)
    check(_L().lkgd_cfg_fusion_euler_step(noise_tokens.data_ptr(), latents.data_ptr(),
                                          int(latents.dtype == torch.float32), _ptr(guidance), weight.data_ptr(), B, F,
                                          H, W, cfg, sigma, sigma_next, 1 if v_prediction else 0, _stream()),
          "lkgd_cfg_fusion_euler_step")
    return latents


def _window(latents: torch.Tensor, f0: int, L: int):
    _req_latents(latents)
    if latents.dim() == 5 and latents.shape[0] == 1:
        latents = latents[0]
    if latents.dim() != 4 or latents.shape[1] != 4:
        raise _lib.LkgdHipError(f"latents must be contiguous [T,4,H,W] (or [1,T,4,H,W]), got {tuple(latents.shape)}")
    T, _, H, W = latents.shape
    if not (0 <= f0 and 0 < L and f0 + L <= T):
        raise _lib.LkgdHipError(f"window of {L} frames at {f0} does not lie inside the {T} frames")
    return T, H, W


def window_prepare_input(latents: torch.Tensor, image_latents: torch.Tensor, f0: int, L: int, cfg: int, sigma: float,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames f0 .. f0+L-1 of ``latents`` [T,4,H,W] (or [1,T,4,H,W]) + per-frame conditional ``image_latents`` [T,4,H,W] ->
    channels-last tokens [2*cfg*L*H*W, 8] of the UNet batch [window, reversed window] x [uncond, cond]
    (lkgd_window_prepare_input); ``out`` may be the leading rows of a larger token buffer"""
    T, H, W = _window(latents, f0, L)
    _req(image_latents, torch.float16, "image_latents")
    if tuple(image_latents.shape) != (T, 4, H, W) or not image_latents.is_contiguous():
        raise _lib.LkgdHipError(f"image_latents must be contiguous [T,4,H,W] = {(T, 4, H, W)}, got {tuple(image_latents.shape)}")
    rows = 2 * cfg * L * H * W
    if out is None:
        out = torch.empty(rows, 8, dtype=torch.float16, device=latents.device)
    else:
        _req(out, torch.float16, "out")
        if out.dim() != 2 or out.shape[1] != 8 or not out.is_contiguous() or out.shape[0] < rows:
            raise _lib.LkgdHipError(f"out must be a contiguous [>= {rows}, 8] token buffer, got {tuple(out.shape)}")
        out = out[:rows]
    check(_L().lkgd_window_prepare_input(latents.data_ptr(), int(latents.dtype == torch.float32), image_latents.data_ptr(),
                                         T, f0, L, H, W, cfg, sigma, out.data_ptr(), _stream()), "lkgd_window_prepare_input")
    return out


def window_cfg_euler_step(noise_tokens: torch.Tensor, latents: torch.Tensor, guidance: Optional[torch.Tensor], f0: int, L: int,
                          cfg: int, sigma: float, sigma_next: float, v_prediction: bool = True) -> torch.Tensor:
    """in-place Euler update of frames f0 .. f0+L-1 of ``latents`` [T,4,H,W] (or [1,T,4,H,W]) from the forward clip's entries of
    the window's noise tokens [2*cfg*L*H*W, 4]; ``guidance`` fp32 [L] on the device, or None when cfg == 1
    (lkgd_window_cfg_euler_step)"""
    T, H, W = _window(latents, f0, L)
    _req(noise_tokens, torch.float16, "noise_tokens")
    if tuple(noise_tokens.shape) != (2 * cfg * L * H * W, 4) or not noise_tokens.is_contiguous():
        raise _lib.LkgdHipError(f"noise_tokens must be contiguous [{2 * cfg * L * H * W}, 4], got {tuple(noise_tokens.shape)}")
    if guidance is not None:
        _req(guidance, torch.float32, "guidance")
        if guidance.numel() != L or not guidance.is_contiguous():
            raise _lib.LkgdHipError(f"guidance must hold one contiguous fp32 value per window frame ({L})")
    check(_L().lkgd_window_cfg_euler_step(noise_tokens.data_ptr(), latents.data_ptr(), int(latents.dtype == torch.float32),
                                          _ptr(guidance), T, f0, L, H, W, cfg, sigma, sigma_next, 1 if v_prediction else 0,
                                          _stream()), "lkgd_window_cfg_euler_step")
    return latents


def shard_rows(src: torch.Tensor, dst: torch.Tensor, fl: int, HW: int, C_: int, px, pack: bool) -> torch.Tensor:
    """pack: src [fl, HW, C] -> dst rows grouped by destination pixel shard (px = pixels per shard); not pack: the inverse
    (lkgd_shard_rows).  Both contiguous fp16."""
    _req(src, torch.float16, "src"); _req(dst, torch.float16, "dst")
    if not (src.is_contiguous() and dst.is_contiguous()) or src.numel() != fl * HW * C_ or dst.numel() != src.numel():
        raise _lib.LkgdHipError("shard_rows: contiguous [fl * HW, C] buffers expected")
    import ctypes
    tab = (ctypes.c_int32 * len(px))(*px)
    # (always the real library: this runs inside the host-side exchange steps, which a recorded plan re-runs as a whole -
    # recording the launch as well would run it twice per replay)
    check(_lib.lib().lkgd_shard_rows(src.data_ptr(), dst.data_ptr(), fl, HW, C_, len(px), ctypes.cast(tab, ctypes.c_void_p),
                                     int(pack), _stream()), "lkgd_shard_rows")
    return dst


def tokens_to_nchw(tokens: torch.Tensor, N: int, C_: int, H: int, W: int) -> torch.Tensor:
    _req(tokens, torch.float16, "tokens")
    out = torch.empty(N, C_, H, W, dtype=torch.float16, device=tokens.device)
    check(_L().lkgd_tokens_to_nchw(tokens.data_ptr(), _ld(tokens), N, C_, H * W, out.data_ptr(), _stream()),
          "lkgd_tokens_to_nchw")
    return out


def nchw_to_tokens(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(x, torch.float16, "x")
    N, C_, H, W = x.shape
    assert x.is_contiguous()
    if out is None:
        out = torch.empty(N * H * W, C_, dtype=torch.float16, device=x.device)
    check(_L().lkgd_nchw_to_tokens(x.data_ptr(), N, C_, H * W, out.data_ptr(), _ld(out), _stream()),
          "lkgd_nchw_to_tokens")
    return out


def timestep_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    _req(t, torch.float32, "t")
    out = torch.empty(t.numel(), dim, dtype=torch.float16, device=t.device)
    check(_L().lkgd_timestep_embedding(t.data_ptr(), t.numel(), dim, out.data_ptr(), dim, _stream()),
          "lkgd_timestep_embedding")
    return out


def silu(x: torch.Tensor) -> torch.Tensor:
    _req(x, torch.float16, "x")
    y = torch.empty_like(x)
    check(_L().lkgd_silu(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "lkgd_silu")
    return y


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _req(a, torch.float16, "a"); _req(b, torch.float16, "b")
    y = torch.empty_like(a)
    check(_L().lkgd_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), _stream()), "lkgd_add")
    return y


def fsm_rows(a: torch.Tensor, out: torch.Tensor, *, pairs: int, HW: int, C_: int, a_rows: Tuple[int, int],
             o_rows: Tuple[int, int], res: Optional[torch.Tensor] = None, r_rows: Tuple[int, int] = (0, 0),
             bias: Optional[torch.Tensor] = None, bias_map: Tuple[int, int, int] = (1, 0, 1),
             csr: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """FSM hook row kernel (include/lkgd_hip.h section 9).  ``x_rows`` = (rows per pair, row offset); ``csr`` =
    (csr_off int32 [pairs*HW+1], csr_pt int32 [pairs*P], gather_idx int32 [pairs*P], vis fp32 [pairs*P])."""
    _req(a, torch.float16, "a"); _req(out, torch.float16, "out")
    d = _lib.FsmDesc()
    d.a, d.out, d.lda, d.ldo = a.data_ptr(), out.data_ptr(), _ld(a), _ld(out)
    d.a_pair_rows, d.a_off = a_rows
    d.o_pair_rows, d.o_off = o_rows
    d.pairs, d.HW, d.C = pairs, HW, C_
    if res is not None:
        _req(res, torch.float16, "res")
        d.res, d.ldr = res.data_ptr(), _ld(res)
        d.r_pair_rows, d.r_off = r_rows
    if bias is not None:
        _req(bias, torch.float16, "bias")
        d.bias, d.ldb = bias.data_ptr(), _ld(bias)
        d.bias_mul, d.bias_add, d.bias_div = bias_map
    if csr is not None:
        off, pt, gi, vis = csr
        for t, dt, n in ((off, torch.int32, "csr_off"), (pt, torch.int32, "csr_pt"), (gi, torch.int32, "gather_idx"),
                         (vis, torch.float32, "vis")):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise _lib.LkgdHipError(f"{n} must be a contiguous GPU {dt} tensor")
        if off.numel() != pairs * HW + 1 or pt.numel() != gi.numel() or pt.numel() != vis.numel():
            raise _lib.LkgdHipError("fsm_rows: CSR table sizes do not match pairs*HW / pairs*P")
        d.csr_off, d.csr_pt, d.gather_idx, d.vis = off.data_ptr(), pt.data_ptr(), gi.data_ptr(), vis.data_ptr()
        d.P = pt.numel() // pairs
    check(_L().lkgd_fsm_rows(C.byref(d), _stream()), "lkgd_fsm_rows")
    return out


def conv3x3_small(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], nimg: int, Hin: int, Win: int,
                  stride: int = 1, silu: bool = True) -> torch.Tensor:
    """direct 3x3 convolution for small channel counts (include/lkgd_hip.h section 10); x [nimg*Hin*Win, Cin] tokens,
    w [Cout, 3, 3, Cin] fp16 -> [nimg*Hout*Wout, Cout]"""
    _req(x, torch.float16, "x"); _req(w, torch.float16, "w")
    cout, cin = w.shape[0], w.shape[3]
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    out = torch.empty(nimg * Hout * Wout, cout, dtype=torch.float16, device=x.device)
    check(_L().lkgd_conv3x3_small(x.data_ptr(), cin, _ld(x), w.data_ptr(), _ptr(bias), out.data_ptr(), cout,
                                        _ld(out), nimg, Hin, Win, stride, int(silu), _stream()), "lkgd_conv3x3_small")
    return out


def softmax_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """row softmax of an fp16 score matrix (include/lkgd_hip.h section 12); in place when out is None"""
    _req(x, torch.float16, "x")
    out = x if out is None else out
    check(_L().lkgd_softmax_rows(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out), x.shape[0], x.shape[1], _stream()),
          "lkgd_softmax_rows")
    return out


def time_conv_out(tokens: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, nbatch: int, F: int, H: int, W: int,
                  dtype=torch.float32) -> torch.Tensor:
    """Conv3d (3,1,1) over the frames on 3 channels + channels-last -> NCHW (section 12); w fp32 [3, 3, 3] = (co, ci, kt)"""
    _req(tokens, torch.float16, "tokens"); _req(w, torch.float32, "w"); _req(bias, torch.float32, "bias")
    out = torch.empty(nbatch * F, 3, H, W, dtype=dtype, device=tokens.device)
    check(_L().lkgd_time_conv_out(tokens.data_ptr(), _ld(tokens), w.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                  int(dtype == torch.float32), nbatch, F, H * W, _stream()), "lkgd_time_conv_out")
    return out


def vit_patchify(x: torch.Tensor, size: int, patch: int) -> torch.Tensor:
    """bilinear resize to size x size (align_corners=False) + patch unfold (include/lkgd_hip.h section 13):
    fp32 [N, C, H, W] -> fp16 [N*(size/patch)^2, C*patch*patch]"""
    _req(x, torch.float32, "x")
    x = x.contiguous()
    N, C_, H, W = x.shape
    g = size // patch
    out = torch.empty(N * g * g, C_ * patch * patch, dtype=torch.float16, device=x.device)
    check(_L().lkgd_vit_patchify(x.data_ptr(), N, C_, H, W, out.data_ptr(), size, patch, _stream()), "lkgd_vit_patchify")
    return out


def gelu_tanh_(x: torch.Tensor) -> torch.Tensor:
    """F.gelu(x, approximate="tanh") in place (include/lkgd_hip.h section 14)"""
    _req(x, torch.float16, "x")
    if not x.is_contiguous():
        raise _lib.LkgdHipError("gelu_tanh_ needs a contiguous tensor")
    check(_L().lkgd_gelu_tanh(x.data_ptr(), x.data_ptr(), x.numel(), _stream()), "lkgd_gelu_tanh")
    return x


def gated_add(x: torch.Tensor, gate: torch.Tensor, res: torch.Tensor, rows_per_batch: int, split: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = res + gate[(row // rows_per_batch) * 2 + (row % rows_per_batch >= split)] * x  (section 14); gate fp32 [2*B, C]"""
    _req(x, torch.float16, "x"); _req(res, torch.float16, "res"); _req(gate, torch.float32, "gate")
    if out is None:
        out = torch.empty_like(res)
    check(_L().lkgd_gated_add(x.data_ptr(), _ld(x), gate.data_ptr(), res.data_ptr(), _ld(res), out.data_ptr(), _ld(out),
                              x.shape[0], x.shape[1], rows_per_batch, split, _stream()), "lkgd_gated_add")
    return out


def _dit_latents(latents: torch.Tensor, p: int, p_t: Optional[int] = None):
    _req_latents(latents)
    if latents.dim() != 5:
        raise _lib.LkgdHipError(f"latents must be [B, F, C, H, W], got {tuple(latents.shape)}")
    B, F, C_, H, W = latents.shape
    if p != 2 or H % p or W % p or (C_ * p * p) % 8:
        raise _lib.LkgdHipError(f"DiT loop glue: patch_size 2, even H and W, C * 4 a multiple of 8; got p = {p}, latents "
                                f"{tuple(latents.shape)}")
    if p_t is not None and (p_t != 2 or F % p_t):
        raise _lib.LkgdHipError(f"DiT loop glue with temporal patches: patch_size_t 2 and a frame count it divides (pad_for_temporal_"
                                f"patches); got patch_size_t = {p_t}, latents {tuple(latents.shape)}")
    return B, F, C_, H, W


def dit_patch_rows(latents: torch.Tensor, image_latents: Optional[torch.Tensor], p: int = 2,
                   out: Optional[torch.Tensor] = None, p_t: Optional[int] = None) -> torch.Tensor:
    """[B,F,C,H,W] latents (fp16 / fp32) + fp16 image latents of the same shape (or None) -> the patch-embedding GEMM's rows
    [B*F*(H/p)*(W/p), 2C*p*p] (C*p*p without image latents), column (c*p + py)*p + px (lkgd_dit_patch_rows): one copy for
    every CFG entry.  ``out``: an fp16 [rows, >= width] matrix or column window (row stride a multiple of 8).
    ``p_t`` (the CogVideoX 1.5 models): rows [B*(F/p_t)*(H/p)*(W/p), 2C*p_t*p*p], column ((c*p_t + pt)*p + py)*p + px
    (lkgd_dit_patch_rows_t, include/lkgd_hip_dit_tpatch.h)."""
    B, F, C_, H, W = _dit_latents(latents, p, p_t)
    if image_latents is not None:
        _req(image_latents, torch.float16, "image_latents")
        if tuple(image_latents.shape) != tuple(latents.shape) or not image_latents.is_contiguous():
            raise _lib.LkgdHipError(f"image_latents must be contiguous {tuple(latents.shape)}, got {tuple(image_latents.shape)}")
    rows, width = B * F * (H // p) * (W // p), (1 if image_latents is None else 2) * C_ * p * p
    if p_t is not None:
        rows, width = rows // p_t, width * p_t
    if out is None:
        out = torch.empty(rows, width, dtype=torch.float16, device=latents.device)
    else:
        _req(out, torch.float16, "out")
        if out.dim() != 2 or tuple(out.shape) != (rows, width) or out.stride(1) != 1:
            raise _lib.LkgdHipError(f"out must be an fp16 [{rows}, {width}] matrix, got {tuple(out.shape)}")
    name, pt = ("lkgd_dit_patch_rows", ()) if p_t is None else ("lkgd_dit_patch_rows_t", (p_t,))
    check(getattr(_L(), name)(latents.data_ptr(), int(latents.dtype == torch.float32), _ptr(image_latents), B, F, C_, H, W, p, *pt,
                              out.data_ptr(), _ld(out), _stream()), name)
    return out


def dit_cfg_ddim_step(noise_rows: torch.Tensor, latents: torch.Tensor, p: int, cfg: int, guidance: float, a: float, b: float,
                      sqrt_alpha: float, sqrt_beta: float, p_t: Optional[int] = None) -> torch.Tensor:
    """in-place CFG combine + DDIM update of ``latents`` [B,F,C,H,W] from proj_out's token rows [cfg*B*Tv, C*p*p] (unconditional
    entries first; lkgd_dit_cfg_ddim_step); the scalars are ``dynamic_guidance`` / ``CogVideoXDDIMScheduler.coefficients``.
    ``p_t``: rows [cfg*B*Tv/p_t, C*p_t*p*p] of a temporal-patch model (lkgd_dit_cfg_ddim_step_t)"""
    B, F, C_, H, W = _dit_latents(latents, p, p_t)
    _req(noise_rows, torch.float16, "noise_rows")
    rows, width = cfg * B * F * (H // p) * (W // p), C_ * p * p
    if p_t is not None:
        rows, width = rows // p_t, width * p_t
    if cfg not in (1, 2) or noise_rows.dim() != 2 or tuple(noise_rows.shape) != (rows, width) or noise_rows.stride(1) != 1:
        raise _lib.LkgdHipError(f"noise_rows must be an fp16 [{rows}, {width}] matrix (cfg 1 or 2), got "
                                f"{tuple(noise_rows.shape)}, cfg = {cfg}")
    name, pt = ("lkgd_dit_cfg_ddim_step", ()) if p_t is None else ("lkgd_dit_cfg_ddim_step_t", (p_t,))
    check(getattr(_L(), name)(noise_rows.data_ptr(), _ld(noise_rows), latents.data_ptr(), int(latents.dtype == torch.float32),
                              B, F, C_, H, W, p, *pt, cfg, guidance, a, b, sqrt_alpha, sqrt_beta, _stream()), name)
    return latents


def dit_cfg_dpm_step(noise_rows: torch.Tensor, latents: torch.Tensor, x0_state: torch.Tensor, eps: Optional[torch.Tensor], p: int,
                     cfg: int, order: int, g: float, coef, p_t: Optional[int] = None) -> torch.Tensor:
    """in-place CFG combine + DPM-Solver++ update of ``latents`` [B,F,C,H,W] from proj_out's token rows, as ``dit_cfg_ddim_step`` takes
    them (lkgd_dit_cfg_dpm_step / _t with ``p_t``, include/lkgd_hip_dit_dpm.h).  ``x0_state`` fp32, the latents' shape: read when
    ``order`` is 2 (the previous step's x0), always rewritten with this step's.  ``eps``: the step's noise in the latents' shape and
    dtype; None only when ``coef.mn`` is 0.  ``coef`` = ``CogVideoXDPMScheduler.coefficients(t, t_back)`` (its own ``order`` field is
    not read: the caller passes ``order``)"""
    B, F, C_, H, W = _dit_latents(latents, p, p_t)
    _req(noise_rows, torch.float16, "noise_rows")
    _req(x0_state, torch.float32, "x0_state")
    rows, width = cfg * B * F * (H // p) * (W // p), C_ * p * p
    if p_t is not None:
        rows, width = rows // p_t, width * p_t
    if cfg not in (1, 2) or noise_rows.dim() != 2 or tuple(noise_rows.shape) != (rows, width) or noise_rows.stride(1) != 1:
        raise _lib.LkgdHipError(f"noise_rows must be an fp16 [{rows}, {width}] matrix (cfg 1 or 2), got "
                                f"{tuple(noise_rows.shape)}, cfg = {cfg}")
    if order not in (1, 2):
        raise _lib.LkgdHipError(f"dit_cfg_dpm_step: order must be 1 or 2, got {order!r}")
    if tuple(x0_state.shape) != tuple(latents.shape) or not x0_state.is_contiguous():
        raise _lib.LkgdHipError(f"x0_state must be contiguous fp32 {tuple(latents.shape)}, got {tuple(x0_state.shape)}")
    mn = float(coef.mn)
    if eps is None:
        if mn != 0.0:
            raise _lib.LkgdHipError(f"dit_cfg_dpm_step: the step has a noise term (mn = {mn}) and needs eps")
    else:
        _req(eps, latents.dtype, "eps")
        if tuple(eps.shape) != tuple(latents.shape) or not eps.is_contiguous():
            raise _lib.LkgdHipError(f"eps must be contiguous {tuple(latents.shape)} in the latents' dtype, got {tuple(eps.shape)}")
    name, pt = ("lkgd_dit_cfg_dpm_step", ()) if p_t is None else ("lkgd_dit_cfg_dpm_step_t", (p_t,))
    check(getattr(_L(), name)(noise_rows.data_ptr(), _ld(noise_rows), latents.data_ptr(), int(latents.dtype == torch.float32),
                              x0_state.data_ptr(), _ptr(eps), B, F, C_, H, W, p, *pt, cfg, order, g, float(coef.sqrt_alpha),
                              float(coef.sqrt_beta), float(coef.m1), float(coef.m2), float(coef.m3), float(coef.m4), mn, _stream()), name)
    return latents


def qk_norm_rope(q: torch.Tensor, k: torch.Tensor, heads: int, nq, nk, eps: float, rope, rows_per_batch: int,
                 split: int) -> None:
    """per-head LayerNorm of q and k, then the rotary embedding of their video rows, in place and in one launch
    (include/lkgd_hip_dit.h).  q, k fp16 [rows, >= heads * 64] (column windows allowed); nq / nk = (gamma, beta) fp32 [64];
    rope = (cos, sin) fp32 [rows_per_batch - split, 64], or None for the norm alone; rows r with r % rows_per_batch < split
    are text rows (never rotated)"""
    _req(q, torch.float16, "q"); _req(k, torch.float16, "k")
    for name, t in (("gamma_q", nq[0]), ("beta_q", nq[1]), ("gamma_k", nk[0]), ("beta_k", nk[1])):
        _req(t, torch.float32, name)
        if t.numel() != 64 or not t.is_contiguous():
            raise _lib.LkgdHipError(f"qk_norm_rope: {name} must be a contiguous fp32 [64] vector")
    if q.dim() != 2 or k.dim() != 2 or q.shape[0] != k.shape[0] or q.shape[1] != heads * 64 or k.shape[1] != heads * 64:
        raise _lib.LkgdHipError(f"qk_norm_rope: q and k must both be [rows, heads * 64], got {tuple(q.shape)} / {tuple(k.shape)}")
    cos = sin = None
    ldt = 0
    if rope is not None:
        cos, sin = rope
        _req(cos, torch.float32, "cos"); _req(sin, torch.float32, "sin")
        if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != 64 or cos.shape[0] != rows_per_batch - split:
            raise _lib.LkgdHipError(f"qk_norm_rope: cos / sin must both be [rows_per_batch - split, 64], got {tuple(cos.shape)} / "
                                    f"{tuple(sin.shape)}")
        if _ld(cos) != _ld(sin):
            raise _lib.LkgdHipError("qk_norm_rope: cos and sin must share one row stride")
        ldt = _ld(cos)
    check(_L().lkgd_qk_norm_rope(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), q.shape[0], heads, nq[0].data_ptr(), nq[1].data_ptr(),
                                 nk[0].data_ptr(), nk[1].data_ptr(), eps, _ptr(cos), _ptr(sin), ldt, rows_per_batch, split,
                                 _stream()), "lkgd_qk_norm_rope")


def scale(x: torch.Tensor, s: float) -> torch.Tensor:
    _req(x, torch.float16, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_L().lkgd_scale(x.data_ptr(), y.data_ptr(), x.numel(), s, _stream()), "lkgd_scale")
    return y


def euler_step(model_output: torch.Tensor, sample: torch.Tensor, sigma: float, sigma_next: float,
               v_prediction: bool = True, noise: torch.Tensor = None, sigma_hat: float = None, s_noise: float = 1.0,
               churn: float = 0.0) -> torch.Tensor:
    """one Euler step; with `noise` (fp16, same shape) the stochastic form: sample += fp16(fp16(noise * s_noise) * churn),
    then the step from sigma_hat to sigma_next (lkgd_hip.h section 8)"""
    _req(model_output, torch.float16, "model_output")
    if not sample.is_cuda or sample.dtype not in (torch.float16, torch.float32):
        raise _lib.LkgdHipError("sample must be a GPU fp16/fp32 tensor")
    mo, sm = model_output.contiguous(), sample.contiguous()
    prev = torch.empty_like(mo)
    if noise is None:
        check(_L().lkgd_euler_step(mo.data_ptr(), sm.data_ptr(), int(sm.dtype == torch.float32), prev.data_ptr(),
                                   mo.numel(), sigma, sigma_next, 1 if v_prediction else 0, _stream()),
              "lkgd_euler_step")
        return prev
    _req(noise, torch.float16, "noise")
    if noise.numel() != mo.numel():
        raise _lib.LkgdHipError("noise must have model_output's shape")
    nz = noise.contiguous()
    check(_L().lkgd_euler_step_churn(mo.data_ptr(), sm.data_ptr(), int(sm.dtype == torch.float32), nz.data_ptr(),
                                     prev.data_ptr(), mo.numel(), sigma, sigma_hat, s_noise, churn, sigma_next,
                                     1 if v_prediction else 0, _stream()), "lkgd_euler_step_churn")
    return prev


def conv1d_reflect(x: torch.Tensor, taps: torch.Tensor, axis: int) -> torch.Tensor:
    """fp32 [B,C,H,W]: 1-D filter along W (axis 1) or H (axis 0) with reflect padding (lkgd_hip.h section 11)"""
    _req(x, torch.float32, "x"); _req(taps, torch.float32, "taps")
    assert x.is_contiguous() and taps.is_contiguous() and x.dim() == 4
    b, c, h, w = x.shape
    out = torch.empty_like(x)
    check(_L().lkgd_conv1d_reflect(x.data_ptr(), out.data_ptr(), b * c, h, w, taps.data_ptr(), taps.numel(), axis,
                                   _stream()), "lkgd_conv1d_reflect")
    return out


def resize_bicubic_ac(x: torch.Tensor, ho: int, wo: int) -> torch.Tensor:
    """fp32 [B,C,H,W] -> [B,C,ho,wo], bicubic (A = -0.75), align_corners=True"""
    _req(x, torch.float32, "x")
    assert x.is_contiguous() and x.dim() == 4
    b, c, h, w = x.shape
    out = torch.empty(b, c, ho, wo, dtype=torch.float32, device=x.device)
    check(_L().lkgd_resize_bicubic_ac(x.data_ptr(), b * c, h, w, out.data_ptr(), ho, wo, _stream()),
          "lkgd_resize_bicubic_ac")
    return out


# ---- FP8 (e4m3fn) block linears of the DiT: include/lkgd_hip_fp8.h ----------------------------------------------------------------
def _fp8_rows(x: torch.Tensor, q: Optional[torch.Tensor], scale: Optional[torch.Tensor], what: str):
    """(q, scale) of a quantiser call on fp16 ``x`` [T, K]: uint8 [T, K] (row stride a multiple of 16) and fp32 [T], allocated
    when not given"""
    _req(x, torch.float16, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise _lib.LkgdHipError(f"{what}: x must be [T, K] with contiguous channels, got {tuple(x.shape)}")
    T, K = x.shape
    if q is None:
        q = torch.empty(T, K, dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty(T, dtype=torch.float32, device=x.device)
    _req(q, torch.uint8, "q"); _req(scale, torch.float32, "scale")
    if q.dim() != 2 or tuple(q.shape) != (T, K) or q.stride(1) != 1 or tuple(scale.shape) != (T,) or not scale.is_contiguous():
        raise _lib.LkgdHipError(f"{what}: q must be uint8 [{T}, {K}] and scale contiguous fp32 [{T}], got {tuple(q.shape)} / "
                                f"{tuple(scale.shape)}")
    return q, scale


def quant_rows_fp8(x: torch.Tensor, q: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """fp16 [T, K] -> (e4m3fn bytes uint8 [T, K], fp32 scale [T]): the per-row statement Q of include/lkgd_hip_fp8.h, one launch"""
    q, scale = _fp8_rows(x, q, scale, "quant_rows_fp8")
    check(_L().lkgd_quant_rows_fp8(x.data_ptr(), _ld(x), q.data_ptr(), _ld(q), scale.data_ptr(), x.shape[0], x.shape[1], _stream()),
          "lkgd_quant_rows_fp8")
    return q, scale


def gelu_tanh_quant_fp8(x: torch.Tensor, q: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """``quant_rows_fp8(gelu_tanh(x))`` exactly, in one launch and without the fp16 round trip (x is left as it is)"""
    q, scale = _fp8_rows(x, q, scale, "gelu_tanh_quant_fp8")
    check(_L().lkgd_gelu_tanh_quant_fp8(x.data_ptr(), _ld(x), q.data_ptr(), _ld(q), scale.data_ptr(), x.shape[0], x.shape[1],
                                        _stream()), "lkgd_gelu_tanh_quant_fp8")
    return q, scale


def layernorm_quant_fp8(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
                        q: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """``quant_rows_fp8(layernorm(x, gamma, beta, eps))`` exactly, in one launch; gamma / beta fp32 [C] or both None"""
    q, scale = _fp8_rows(x, q, scale, "layernorm_quant_fp8")
    if (gamma is None) != (beta is None):
        raise _lib.LkgdHipError("layernorm_quant_fp8: gamma and beta are given together or not at all")
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is not None:
            _req(t, torch.float32, name)
            if tuple(t.shape) != (x.shape[1],) or not t.is_contiguous():
                raise _lib.LkgdHipError(f"layernorm_quant_fp8: {name} must be a contiguous fp32 [{x.shape[1]}] vector")
    check(_L().lkgd_layernorm_quant_fp8(x.data_ptr(), _ld(x), x.shape[0], x.shape[1], _ptr(gamma), _ptr(beta), eps, q.data_ptr(),
                                        _ld(q), scale.data_ptr(), _stream()), "lkgd_layernorm_quant_fp8")
    return q, scale


def gemm_fp8(a: torch.Tensor, a_scale: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor],
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m, n] = fp16((sum_k a[m, k] w[n, k]) a_scale[m] w_scale[n] + bias[n]): a uint8 [M, K] and w uint8 [N, K] hold e4m3fn
    bytes (K contiguous), the scales and the bias are fp32; N and K multiples of 128 (lkgd_gemm_fp8)"""
    _req(a, torch.uint8, "a"); _req(w, torch.uint8, "w"); _req(a_scale, torch.float32, "a_scale"); _req(w_scale, torch.float32, "w_scale")
    if a.dim() != 2 or w.dim() != 2 or a.shape[1] != w.shape[1] or a.stride(1) != 1 or w.stride(1) != 1:
        raise _lib.LkgdHipError(f"gemm_fp8: a [M, K] and w [N, K] must share K and be K-contiguous, got {tuple(a.shape)} / "
                                f"{tuple(w.shape)}")
    (M, K), N = a.shape, w.shape[0]
    if tuple(a_scale.shape) != (M,) or tuple(w_scale.shape) != (N,) or not a_scale.is_contiguous() or not w_scale.is_contiguous():
        raise _lib.LkgdHipError(f"gemm_fp8: a_scale must be contiguous fp32 [{M}] and w_scale [{N}]")
    if bias is not None:
        _req(bias, torch.float32, "bias")
        if tuple(bias.shape) != (N,) or not bias.is_contiguous():
            raise _lib.LkgdHipError(f"gemm_fp8: bias must be a contiguous fp32 [{N}] vector")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=a.device)
    _req(out, torch.float16, "out")
    if out.dim() != 2 or tuple(out.shape) != (M, N) or out.stride(1) != 1:
        raise _lib.LkgdHipError(f"gemm_fp8: out must be fp16 [{M}, {N}], got {tuple(out.shape)}")
    # a member of the GEMM family for the live roofline and the replay plan: the same events and FLOP accounting as ``gemm``
    _gemm_family("lkgd_gemm_fp8", (a.data_ptr(), _ld(a), a_scale.data_ptr(), w.data_ptr(), _ld(w), w_scale.data_ptr(), _ptr(bias),
                                   out.data_ptr(), _ld(out), M, N, K), 2.0 * M * N * K)
    return out


# ---- the T5 text encoder's operators: include/lkgd_hip_t5.h -----------------------------------------------------------------------
def _t5_rows(t: torch.Tensor, dtype, name: str, like: Optional[torch.Tensor] = None, width: Optional[int] = None) -> None:
    """a [T, C] matrix with contiguous channels; with ``like`` / ``width``: of that row count and width"""
    _req(t, dtype, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise _lib.LkgdHipError(f"{name} must be [T, C] with contiguous channels, got {tuple(t.shape)} strides {tuple(t.stride())}")
    if like is not None and (t.shape[0] != like.shape[0] or t.shape[1] != (like.shape[1] if width is None else width)):
        raise _lib.LkgdHipError(f"{name} must be [{like.shape[0]}, {like.shape[1] if width is None else width}], got {tuple(t.shape)}")


def t5_embed_rows(ids: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t, :] = float(table[ids[t], :]): int64 ids [T], fp16 table [V, D] -> fp32 [T, D] (lkgd_t5_embed_rows).  The ids are the
    caller's to validate (a host check costs a sync); the kernel clamps them into the table"""
    _req(ids, torch.int64, "ids"); _t5_rows(table, torch.float16, "table")
    if ids.dim() != 1 or not ids.is_contiguous():
        raise _lib.LkgdHipError(f"ids must be a contiguous int64 [T] vector, got {tuple(ids.shape)}")
    if out is None:
        out = torch.empty(ids.shape[0], table.shape[1], dtype=torch.float32, device=table.device)
    _t5_rows(out, torch.float32, "out")
    if tuple(out.shape) != (ids.shape[0], table.shape[1]):
        raise _lib.LkgdHipError(f"out must be [{ids.shape[0]}, {table.shape[1]}], got {tuple(out.shape)}")
    check(_L().lkgd_t5_embed_rows(ids.data_ptr(), table.data_ptr(), _ld(table), table.shape[0], table.shape[1], out.data_ptr(), _ld(out),
                                  ids.shape[0], _stream()), "lkgd_t5_embed_rows")
    return out


def t5_rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """T5LayerNorm: fp32 [T, C] rows -> fp16(weight * (x * rsqrt(mean(x^2) + eps))), C <= 4096 (lkgd_t5_rmsnorm)"""
    _t5_rows(x, torch.float32, "x"); _req(weight, torch.float32, "weight")
    if tuple(weight.shape) != (x.shape[1],) or not weight.is_contiguous():
        raise _lib.LkgdHipError(f"weight must be a contiguous fp32 [{x.shape[1]}] vector")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _t5_rows(out, torch.float16, "out", like=x)
    check(_L().lkgd_t5_rmsnorm(x.data_ptr(), _ld(x), x.shape[0], x.shape[1], weight.data_ptr(), eps, out.data_ptr(), _ld(out), _stream()),
          "lkgd_t5_rmsnorm")
    return out


def attn_dense_relbias(q, k, v, out, nbatch: int, S: int, heads: int, head_dim: int, relbias: torch.Tensor,
                       scale: Optional[float] = None):
    """:func:`attn_dense` with ``relbias[h, j - i + S - 1]`` added to the scaled score of query i and key j before the softmax;
    relbias fp32 [heads, 2S - 1] (lkgd_attn_dense_relbias).  ``scale`` None = head_dim ** -0.5; T5 passes 1.0"""
    _req(q, torch.float16, "q"); _req(k, torch.float16, "k"); _req(v, torch.float16, "v"); _req(out, torch.float16, "out")
    _req(relbias, torch.float32, "relbias")
    if tuple(relbias.shape) != (heads, 2 * S - 1) or not relbias.is_contiguous():
        raise _lib.LkgdHipError(f"relbias must be a contiguous fp32 [{heads}, {2 * S - 1}] table, got {tuple(relbias.shape)}")
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if t.dim() != 2 or t.shape[0] != nbatch * S or t.shape[1] != heads * head_dim:
            raise _lib.LkgdHipError(f"{name} must be [{nbatch * S}, {heads * head_dim}], got {tuple(t.shape)}")
    if scale is None:
        scale = head_dim ** -0.5
    check(_L().lkgd_attn_dense_relbias(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(), _ld(out),
                                       nbatch, S, heads, head_dim, relbias.data_ptr(), scale, _stream()), "lkgd_attn_dense_relbias")
    return out


def t5_gated_gelu(h: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16 [T, 2F] -> fp16 [T, F]: gelu_tanh(h[:, :F]) * h[:, F:], fp32 arithmetic, one rounding (lkgd_t5_gated_gelu)"""
    _t5_rows(h, torch.float16, "h")
    if h.shape[1] % 2:
        raise _lib.LkgdHipError(f"h must hold the two halves side by side, got width {h.shape[1]}")
    F_ = h.shape[1] // 2
    if out is None:
        out = torch.empty(h.shape[0], F_, dtype=torch.float16, device=h.device)
    _t5_rows(out, torch.float16, "out", like=h, width=F_)
    check(_L().lkgd_t5_gated_gelu(h.data_ptr(), _ld(h), h.shape[0], F_, out.data_ptr(), _ld(out), _stream()), "lkgd_t5_gated_gelu")
    return out


def t5_residual_add_(x: torch.Tensor, y: torch.Tensor, s: float = 1.0) -> torch.Tensor:
    """x += s * float(y) in place: x fp32 [T, C] (the encoder's residual stream), y fp16 [T, C] (lkgd_t5_residual_add)"""
    _t5_rows(x, torch.float32, "x"); _t5_rows(y, torch.float16, "y", like=x)
    check(_L().lkgd_t5_residual_add(x.data_ptr(), _ld(x), y.data_ptr(), _ld(y), x.shape[0], x.shape[1], s, _stream()),
          "lkgd_t5_residual_add")
    return x


# ---- the encoder of the CogVideoX 3-D causal VAE (include/lkgd_hip_cogvae_enc.h) --------------------------------------------------------
def pooled_frames(T: int) -> int:
    """frames the temporal pool of CogVideoXDownsample3D leaves of T: T/2, or with the first frame apart 1 + (T - 1)/2 for odd T"""
    return 1 + (T - 1) // 2 if T % 2 else T // 2


def cogvae_pixel_taps(x: torch.Tensor, t0: int, Tc: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the A operand of the encoder's conv_in (lkgd_cogvae_pixel_taps): ``x`` fp16 [B, Cin <= 4, T, H, W] contiguous -> fp16
    [B*Tc*H*W, 128] rows of the 27*Cin causal taps of frames [t0, t0 + Tc), k = ((kt*3 + ky)*3 + kx)*Cin + c, zeros behind them"""
    _req(x, torch.float16, "x")
    if x.dim() != 5 or not x.is_contiguous():
        raise _lib.LkgdHipError(f"x must be a contiguous [B, Cin, T, H, W] clip, got {tuple(x.shape)} strides {tuple(x.stride())}")
    B, Cin, T, H, W = x.shape
    rows = B * Tc * H * W
    if out is None:
        out = torch.empty(rows, 128, dtype=torch.float16, device=x.device)
    _req(out, torch.float16, "out")
    if out.dim() != 2 or tuple(out.shape) != (rows, 128):
        raise _lib.LkgdHipError(f"out must be [{rows}, 128], got {tuple(out.shape)}")
    check(_L().lkgd_cogvae_pixel_taps(x.data_ptr(), out.data_ptr(), _ld(out), B, Cin, T, H, W, int(t0), int(Tc), _stream()),
          "lkgd_cogvae_pixel_taps")
    return out


def cogvae_time_pool(x: torch.Tensor, B: int, T: int, HW: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the temporal average pool of CogVideoXDownsample3D (lkgd_cogvae_time_pool): fp16 rows [B*T*HW, C] -> [B*pooled_frames(T)*HW, C]"""
    _req(x, torch.float16, "x")
    if x.dim() != 2 or x.shape[0] != B * T * HW:
        raise _lib.LkgdHipError(f"x must be [{B * T * HW}, C] rows, got {tuple(x.shape)}")
    C_ = x.shape[1]
    orows = B * pooled_frames(T) * HW
    if out is None:
        out = torch.empty(orows, C_, dtype=torch.float16, device=x.device)
    _req(out, torch.float16, "out")
    if out.dim() != 2 or tuple(out.shape) != (orows, C_):
        raise _lib.LkgdHipError(f"out must be [{orows}, {C_}], got {tuple(out.shape)}")
    check(_L().lkgd_cogvae_time_pool(x.data_ptr(), _ld(x), out.data_ptr(), _ld(out), B, T, HW, C_, _stream()), "lkgd_cogvae_time_pool")
    return out


def cogvae_posterior(mom: torch.Tensor, B: int, lc: int, T: int, h: int, w: int, noise: Optional[torch.Tensor] = None,
                     scale: float = 1.0):
    """the posterior of the encoder's moment rows (lkgd_cogvae_posterior): ``mom`` fp16 [B*T*h*w, >= 2*lc] -> ``mean`` fp16
    [B, lc, T, h, w] and, with ``noise`` (same layout), ``sample`` = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise);
    returns (mean, sample or None)"""
    _req(mom, torch.float16, "mom")
    if mom.dim() != 2 or mom.shape[0] != B * T * h * w or mom.shape[1] < 2 * lc:
        raise _lib.LkgdHipError(f"mom must be [{B * T * h * w}, >= {2 * lc}] rows, got {tuple(mom.shape)}")
    mean = torch.empty(B, lc, T, h, w, dtype=torch.float16, device=mom.device)
    sample = None
    if noise is not None:
        _req(noise, torch.float16, "noise")
        if tuple(noise.shape) != tuple(mean.shape) or not noise.is_contiguous():
            raise _lib.LkgdHipError(f"noise must be a contiguous {tuple(mean.shape)} tensor, got {tuple(noise.shape)}")
        sample = torch.empty_like(mean)
    check(_L().lkgd_cogvae_posterior(mom.data_ptr(), _ld(mom), _ptr(noise), mean.data_ptr(), _ptr(sample), float(scale), B, lc, T, h, w,
                                     _stream()), "lkgd_cogvae_posterior")
    return mean, sample


# ---- the seam operator of the tiled CogVideoX VAE (include/lkgd_hip_cogvae_tile.h) ------------------------------------------------------
def _planes(t: torch.Tensor, name: str) -> Tuple[int, int, int]:
    """(P, Y, X) of a contiguous fp16 [..., Y, X] tensor of planes"""
    _req(t, torch.float16, name)
    if t.dim() < 3 or not t.is_contiguous():
        raise _lib.LkgdHipError(f"{name} must be contiguous [..., Y, X] planes, got {tuple(t.shape)} strides {tuple(t.stride())}")
    return t.numel() // (t.shape[-2] * t.shape[-1]), t.shape[-2], t.shape[-1]


def cogvae_tile_blend_planar(tile: torch.Tensor, up: Optional[torch.Tensor], left: Optional[torch.Tensor], out: torch.Tensor,
                             y0: int, x0: int, e_y: int, e_x: int, c_y: int, c_x: int) -> torch.Tensor:
    """one tile of a tiled decode (lkgd_cogvae_tile_blend_planar): ``tile`` fp16 [..., Yt, Xt] is cross-faded IN PLACE over its first
    ``e_y`` rows with the last rows of ``up`` [..., Yu, Xt] and then over its first ``e_x`` columns with the last columns of ``left``
    [..., Yt, Xl] (the neighbours' blended tiles, or None), and its first ``c_y`` x ``c_x`` elements go to ``out`` [..., Y, X] at
    (y0, x0); returns ``tile``"""
    P, Yt, Xt = _planes(tile, "tile")
    Po, Y, X = _planes(out, "out")
    Yu = Xl = 0
    if up is not None:
        Pu, Yu, Xu = _planes(up, "up")
        if (Pu, Xu) != (P, Xt):
            raise _lib.LkgdHipError(f"up must hold {P} planes {Xt} wide, got {tuple(up.shape)}")
    if left is not None:
        Pl, Yl, Xl = _planes(left, "left")
        if (Pl, Yl) != (P, Yt):
            raise _lib.LkgdHipError(f"left must hold {P} planes {Yt} high, got {tuple(left.shape)}")
    if Po != P:
        raise _lib.LkgdHipError(f"out must hold {P} planes, got {tuple(out.shape)}")
    check(_L().lkgd_cogvae_tile_blend_planar(tile.data_ptr(), _ptr(up), _ptr(left), out.data_ptr(), P, Yt, Xt, Yu, Xl, Y, X, int(y0),
                                             int(x0), int(e_y), int(e_x), int(c_y), int(c_x), _stream()),
          "lkgd_cogvae_tile_blend_planar")
    return tile


def _image_rows(t: torch.Tensor, name: str) -> Tuple[int, int, int, int, int]:
    """(P, Y, X, C, row stride) of fp16 channels-last images [P, Y, X, C] whose rows (p, y, x) lie one row stride apart"""
    _req(t, torch.float16, name)
    if t.dim() != 4:
        raise _lib.LkgdHipError(f"{name} must be [P, Y, X, C] rows, got {tuple(t.shape)}")
    P, Y, X, C_ = t.shape
    ld = t.stride(2)
    if t.stride(3) != 1 or (Y > 1 and t.stride(1) != X * ld) or (P > 1 and t.stride(0) != Y * X * ld):
        raise _lib.LkgdHipError(f"{name}: the rows (p, y, x) of {tuple(t.shape)} must lie one row stride apart, got strides "
                                f"{tuple(t.stride())}")
    return P, Y, X, C_, ld


def cogvae_tile_blend_rows(tile: torch.Tensor, up: Optional[torch.Tensor], left: Optional[torch.Tensor], out: torch.Tensor,
                           y0: int, x0: int, e_y: int, e_x: int, c_y: int, c_x: int) -> torch.Tensor:
    """one tile of a tiled encode (lkgd_cogvae_tile_blend_rows): as ``cogvae_tile_blend_planar`` on channels-last token rows -
    ``tile`` [P, Yt, Xt, C], ``up`` [P, Yu, Xt, C], ``left`` [P, Yt, Xl, C], ``out`` [P, Y, X, C], each with its own row stride"""
    P, Yt, Xt, C_, ldt = _image_rows(tile, "tile")
    Po, Y, X, Co, ldo = _image_rows(out, "out")
    Yu = Xl = ldu = ldl = 0
    if up is not None:
        Pu, Yu, Xu, Cu, ldu = _image_rows(up, "up")
        if (Pu, Xu, Cu) != (P, Xt, C_):
            raise _lib.LkgdHipError(f"up must be [{P}, Yu, {Xt}, {C_}], got {tuple(up.shape)}")
    if left is not None:
        Pl, Yl, Xl, Cl, ldl = _image_rows(left, "left")
        if (Pl, Yl, Cl) != (P, Yt, C_):
            raise _lib.LkgdHipError(f"left must be [{P}, {Yt}, Xl, {C_}], got {tuple(left.shape)}")
    if (Po, Co) != (P, C_):
        raise _lib.LkgdHipError(f"out must be [{P}, Y, X, {C_}], got {tuple(out.shape)}")
    check(_L().lkgd_cogvae_tile_blend_rows(tile.data_ptr(), ldt, _ptr(up), ldu, _ptr(left), ldl, out.data_ptr(), ldo, P, C_, Yt, Xt, Yu,
                                           Xl, Y, X, int(y0), int(x0), int(e_y), int(e_x), int(c_y), int(c_x), _stream()),
          "lkgd_cogvae_tile_blend_rows")
    return tile


# ---- frames out and image in of the CogVideoX image-to-video pipeline (include/lkgd_hip_video.h) -----------------------------------------
VIDEO_U8, VIDEO_F32, VIDEO_F16 = 0, 1, 2
_VIDEO_OUT = {VIDEO_U8: torch.uint8, VIDEO_F32: torch.float32, VIDEO_F16: torch.float16}


def video_postprocess(video: torch.Tensor, mode: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the frames of a decoded clip (lkgd_video_postprocess): ``video`` fp16 [B, C <= 4, T, H, W] contiguous, denormalised and
    clamped to [0, 1] -> ``VIDEO_U8`` uint8 [B, T, H, W, C] (x 255, rounded half to even), ``VIDEO_F32`` fp32 [B, T, H, W, C] or
    ``VIDEO_F16`` fp16 [B, T, C, H, W]; one launch"""
    _req(video, torch.float16, "video")
    if video.dim() != 5 or not video.is_contiguous():
        raise _lib.LkgdHipError(f"video must be a contiguous [B, C, T, H, W] clip, got {tuple(video.shape)} strides "
                                f"{tuple(video.stride())}")
    if mode not in _VIDEO_OUT:
        raise _lib.LkgdHipError(f"video_postprocess: mode {mode!r}; built: VIDEO_U8, VIDEO_F32, VIDEO_F16")
    B, C_, T, H, W = video.shape
    shape = (B, T, C_, H, W) if mode == VIDEO_F16 else (B, T, H, W, C_)
    if out is None:
        out = torch.empty(shape, dtype=_VIDEO_OUT[mode], device=video.device)
    _req(out, _VIDEO_OUT[mode], "out")
    if tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.LkgdHipError(f"out must be a contiguous {shape} tensor, got {tuple(out.shape)} strides {tuple(out.stride())}")
    check(_L().lkgd_video_postprocess(video.data_ptr(), out.data_ptr(), int(mode), B, C_, T, H, W, _stream()), "lkgd_video_postprocess")
    return out


def image_preprocess(images: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the pipeline's image input (lkgd_image_preprocess): ``images`` uint8 [N, H, W, C <= 4] contiguous -> fp16 [N, C, H, W] =
    2 * (u / 255) - 1, the fp32 statements of the host chain rounded once to fp16; one launch"""
    _req(images, torch.uint8, "images")
    if images.dim() != 4 or not images.is_contiguous():
        raise _lib.LkgdHipError(f"images must be contiguous [N, H, W, C], got {tuple(images.shape)} strides {tuple(images.stride())}")
    N, H, W, C_ = images.shape
    if out is None:
        out = torch.empty(N, C_, H, W, dtype=torch.float16, device=images.device)
    _req(out, torch.float16, "out")
    if tuple(out.shape) != (N, C_, H, W) or not out.is_contiguous():
        raise _lib.LkgdHipError(f"out must be a contiguous {(N, C_, H, W)} tensor, got {tuple(out.shape)} strides {tuple(out.stride())}")
    check(_L().lkgd_image_preprocess(images.data_ptr(), out.data_ptr(), N, H, W, C_, _stream()), "lkgd_image_preprocess")
    return out

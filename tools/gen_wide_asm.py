#!/usr/bin/env python3
r"""Generates the inline-asm K-tile body of lkgd_amd/csrc/gemm_wide.hip (macros WIDE_KTILE_ASM_FIRST / _NEXT in
lkgd_amd/csrc/gemm_wide_ktile.inc): 80 x v_mfma_f32_16x16x32_f16 with the fragment reads software-pipelined one weight
fragment ahead and the next K-tile's nine LDS-DMA loads issued one per weight-fragment step of K-step 0.
Run from the repo root:  python tools/gen_wide_asm.py

Operands of the asm statement (see gemm_wide.hip::wide_ktile):
  %0-%3   x0[j]  token fragments of K-step 0          %4-%7  x1[j]  token fragments of K-step 1
  %8,%9   wf[2]  weight fragment double buffer
  %10 xa0, %11 xa1   LDS address of token fragment 0 for K-step 0 / 1;  fragment j at + j*2048
  %12 wa0, %13 wa1   LDS address of weight fragment 0 for K-step 0 / 1; fragment i at + i*2048
  %14-%17 pA[4]  global sources of this thread's four A rows of the NEXT K-tile (64-bit VGPR pairs)
  %18-%22 oB[5]  byte offsets of its five weight rows from %23 = weights + K offset of the next K-tile (SGPR pair)
  %24     m_a    LDS destination (other stage, A part) + this wave's 1 KiB slice
acc[i][j] (weight fragment i < 10, token fragment j < 4) = a[(4i+j)*4 .. +3].
"""
import asmgen
from asmgen import q


def rd(text):
    # WIDE_RD / WIDE_MM / WIDE_BAR / WIDE_LD are identity macros in the product build (timing knobs: tools/micro/wide_knobs.sh)
    return "WIDE_RD(" + q(text) + ")"


def acc(i, j):
    b = (4 * i + j) * 4
    return "a[%d:%d]" % (b, b + 3)


def body(first, part, nf=10, mf=4):
    # operand numbers: statement A uses the full list of the module docstring; statement B has its own short list
    #   B: %0 wf[1] (scratch), %1 wf[0] (in: K-step 1's first weight fragment), %2-%5 x1[j], %6 wa1
    X = (lambda j: j) if part == 0 else None
    if part == 1:
        xop, wop, waop = (lambda j: 2 + j), (lambda b: 1 - b), 6
    else:
        xop, wop, waop = None, (lambda b: 8 + b), None
    """part 0: barrier, K-step 0 (fragment reads, the nine DMA loads, 40 MFMAs) + the reads of K-step 1's first fragments;
    part 1: K-step 1 (40 MFMAs).  The C++ between the two statements prepares the next K-tile's sources while K-step 0's
    MFMAs drain."""
    lines = ["WIDE_WAIT_TOP", "WIDE_BAR(" + q("s_barrier") + ")"] if part == 0 else [q("s_waitcnt lgkmcnt(0)")]
    # K-step 0 fragments first: they are in flight while the DMA loads below issue
    if part == 0:
        for j in range(mf):
            lines.append(rd("ds_read_b128 %%%d, %%10 offset:%d" % (j, j * 2048)))
        lines.append(rd("ds_read_b128 %8, %12"))
    # the next K-tile's 9 LDS-DMA loads (4 A rows, 5 weight rows), one per weight-fragment step of K-step 0
    stage = []
    for i in range(mf):                 # 64 token rows per load: 64 * mf rows in all
        m0 = q("s_mov_b32 m0, %24") if i == 0 else q("s_add_u32 m0, m0, 8192")
        stage.append(m0 + " " + q("s_nop 0") + " WIDE_LD(" + q("global_load_lds_dwordx4 %%%d, off" % (14 + i)) + ")")
    for i in range(nf // 2):            # 64 weight rows per load: 32 * nf rows in all
        m0 = q("s_add_u32 m0, %24, 32768") if i == 0 else q("s_add_u32 m0, m0, 8192")
        stage.append(m0 + " " + q("s_nop 0") + " WIDE_LD(" + q("global_load_lds_dwordx4 %%%d, %%23" % (18 + i)) + ")")
    # load l goes out in weight-fragment step l * (nf - 1) // len(stage) of K-step 0 (nf = 10: one per step)
    slots = [[] for _ in range(nf - 1)]
    for l, text in enumerate(stage):
        slots[l * (nf - 1) // len(stage)].append(text)
    for ks in (part,):
        xbase = 0 if part == 0 else 2
        wa = 12 if part == 0 else waop
        for i in range(nf):
            cur = wop((ks * nf + i) & 1)
            nxt = wop((ks * nf + i + 1) & 1)
            if i < nf - 1:
                lines.append(rd("ds_read_b128 %%%d, %%%d offset:%d" % (nxt, wa, (i + 1) * 2048)))
                if ks == 0:
                    lines.extend(slots[i])
                lines.append(q("s_waitcnt lgkmcnt(1)"))
            elif ks == 0:
                for j in range(mf):
                    lines.append(rd("ds_read_b128 %%%d, %%11 offset:%d" % (4 + j, j * 2048)))
                lines.append(rd("ds_read_b128 %%%d, %%13" % nxt))
                lines.append(q("s_waitcnt lgkmcnt(%d)" % (mf + 1)))
            else:
                lines.append(q("s_waitcnt lgkmcnt(0)"))
            for j in range(mf):
                c = "0" if (first and ks == 0) else acc(i, j)
                lines.append("WIDE_MM(" + q("v_mfma_f32_16x16x32_f16 %s, %%%d, %%%d, %s" % (acc(i, j), cur, xbase + j, c)) + ")")
    return " \\\n  ".join(lines)


def main():
    # WIDE: wave tile 64 x 160.  WIDE8: the 256x256 form (wave tile 64 x 128: eight weight fragments, accumulators a[0:127], four
    # weight loads per thread).  _M3: the 192-row forms (wave tile 48 x 160 / 48 x 128: three token fragments, accumulators
    # (4i+j)*4 with j < 3, three token loads)
    macros = []
    for pre, nf, mf in (("WIDE", 10, 4), ("WIDE8", 8, 4), ("WIDE_M3", 10, 3), ("WIDE8_M3", 8, 3)):
        macros += [(pre + "_KTILE_ASM_FIRST_A", body(True, 0, nf, mf)), (pre + "_KTILE_ASM_NEXT_A", body(False, 0, nf, mf)),
                   (pre + "_KTILE_ASM_B", body(False, 1, nf, mf))]
    asmgen.write_inc("gen_wide_asm.py", "gemm_wide_ktile.inc", "K-tile body of gemm_wide.hip (see that script for operands).",
                     macros=macros, clobber=("WIDE_AGPR_CLOBBERS", ['"a%d"' % i for i in range(160)]))


if __name__ == "__main__":
    main()

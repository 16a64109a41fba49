#!/usr/bin/env python3
r"""Generates the inline-asm K-loop of lkgd_amd/csrc/gemm_resw.hip (lkgd_amd/csrc/gemm_resw_kloop.inc).
Run from the repo root:  python tools/gen_resw_asm.py

One statement = the whole K-loop of one 32-token block against the LDS-resident 160-channel weight slab:
NKS * 10 weight fragments (ds_read_b128, software-pipelined D fragments ahead through a ring of R buffers), two
v_mfma_f32_16x16x32_f16 per fragment (both token fragments), and the NEXT block's token fragments loaded into the
registers of K-steps already consumed.

Register plan (the compiler sees none of the AGPRs; arch VGPRs are capped at 96 by the kernel attribute):
  a[0:79]    accumulators: acc[i][j] (channel fragment i < 10, token fragment j < 2) = a[(2i+j)*4 .. +3]
  a[80:159]  token fragments (MFMA B operands): x[j][ks] = a[80 + (j*NKS + ks)*4 .. +3]; written by global_load only
Operands of the K-loop statement:
  %0-%9   wf[10] weight-fragment ring (scratch): a fragment is read nine fragments (18 MFMAs) ahead of its use
  %10 wl0, %11 wl1 LDS byte address of this lane's 16 bytes of fragment 0 / fragment 5*NKS (offsets are 16-bit)
  %12 pn0, %13 pn1 global address of the NEXT block's token row for j = 0 / 1 (+ this lane's 16-byte column)
  %14, %15         vmcnt immediates: how many vector-memory operations younger than the token fragments of K-step 0
                   (K-steps >= 1) are certainly in flight - see gemm_resw.hip
"""
import asmgen
from asmgen import q

R, D = 10, 9


# RESW_RD / RESW_MM / RESW_LX are identity macros in the product build (timing knobs: tools/micro/resw_knobs.sh)
def rdw(text):
    return "RESW_RD(" + q(text) + ")"


def mm(text):
    return "RESW_MM(" + q(text) + ")"


def lx(text):
    return "RESW_LX(" + q(text) + ")"


def kloop(nks):
    nfrag = 10 * nks
    half = 5 * nks

    def rd(n):
        ks, i = divmod(n, 10)
        f = i * nks + ks
        base, off = (R, f * 1024) if f < half else (R + 1, (f - half) * 1024)
        return rdw("ds_read_b128 %%%d, %%%d offset:%d" % (n % R, base, off))

    def xreg(j, ks):
        b = 80 + (j * nks + ks) * 4
        return "a[%d:%d]" % (b, b + 3)

    def ldx(ks):
        return [lx("global_load_dwordx4 %s, %%%d, off offset:%d" % (xreg(j, ks), R + 2 + j, ks * 64)) for j in range(2)]

    lines = [q("s_waitcnt lgkmcnt(0)")]
    for n in range(min(D, nfrag)):
        lines.append(rd(n))
    for n in range(nfrag):
        ks, i = divmod(n, 10)
        if n + D < nfrag:
            lines.append(rd(n + D))
        lg = min(D, nfrag - 1 - n)
        if i == 0:
            lines.append(q("s_waitcnt vmcnt(%%%d) lgkmcnt(%d)" % (R + 4 if ks == 0 else R + 5, lg)))
        else:
            lines.append(q("s_waitcnt lgkmcnt(%d)" % lg))
        for j in range(2):
            c = (2 * i + j) * 4
            acc = "a[%d:%d]" % (c, c + 3)
            lines.append(mm("v_mfma_f32_16x16x32_f16 %s, %%%d, %s, %s" % (acc, n % R, xreg(j, ks), "0" if ks == 0 else acc)))
        if i == 2 and ks >= 1:
            lines += ldx(ks - 1)       # K-step ks-1 was consumed six MFMAs ago: its registers take the next block's rows
    lines += ldx(nks - 1)
    lines.append(q("s_nop 15"))        # the last MFMAs have left the pipe before the epilogue reads the accumulators
    lines.append(q("s_nop 15"))
    return " \\\n  ".join(lines)


def loadx(nks):
    lines = []
    for ks in range(nks):
        for j in range(2):
            b = 80 + (j * nks + ks) * 4
            lines.append(q("global_load_dwordx4 a[%d:%d], %%%d, off offset:%d" % (b, b + 3, j, ks * 64)))
    return " \\\n  ".join(lines)


def main():
    macros = []
    for nk in (1, 2, 3, 4, 5):
        macros += [("RESW_KLOOP_ASM_%d" % nk, kloop(2 * nk)), ("RESW_LOADX_ASM_%d" % nk, loadx(2 * nk))]
    asmgen.write_inc("gen_resw_asm.py", "gemm_resw_kloop.inc", "K-loop of gemm_resw.hip (see that script for operands).",
                     macros=macros, clobber=("RESW_AGPR_CLOBBERS", ['"a%d"' % i for i in range(160)]))


if __name__ == "__main__":
    main()

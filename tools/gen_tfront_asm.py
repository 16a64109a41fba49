#!/usr/bin/env python3
r"""Generates the inline-asm chunk loop of lkgd_amd/csrc/attn_tfront.hip (lkgd_amd/csrc/attn_tfront_kloop.inc).
Run from the repo root:  python tools/gen_tfront_asm.py

One statement = one 64-row weight chunk (q, k or v of one head: 4 fragments of 16 rows x K = 320) against the wave's 32
token rows: 40 weight fragments (ds_read_b128 from the chunk's LDS stage, D fragments ahead through a ring of R registers),
two v_mfma_f32_16x16x32_f16 per fragment.  SWAPPED (q, k):  acc[d][token] += W[d][k] . x[k][token]  (weights = A operand);
DIRECT (v):  acc[token][d] += x[token][k] . W[k][d]  (tokens = A operand) - the same registers, operand order exchanged.

Register plan (AGPRs, invisible to the compiler):
  a[0:31]    acc[i][j] (weight fragment i < 4, token fragment j < 2) = a[(2i+j)*4 .. +3]
  a[32:111]  token fragments x[j][ks] (LayerNorm-ed fp16, MFMA operands) = a[32 + (j*10 + ks)*4 .. +3]
Operands: %0-%5 weight-fragment ring (scratch), %6 LDS byte address of this lane's 16 bytes of fragment 0 of the chunk's stage.
"""
import asmgen
from asmgen import q

R, D = 6, 5
NKS = 10


def chunk(direct):
    nfrag = 4 * NKS
    lines = [q("s_waitcnt lgkmcnt(0)")]

    def rd(n):
        ks, i = divmod(n, 4)
        # TF_RD / TF_MM are identity macros in the product build (timing knobs: tools/micro/tfront_knobs.sh)
        return "TF_RD(" + q("ds_read_b128 %%%d, %%6 offset:%d" % (n % R, (i * NKS + ks) * 1024)) + ")"

    for n in range(D):
        lines.append(rd(n))
    for n in range(nfrag):
        ks, i = divmod(n, 4)
        if n + D < nfrag:
            lines.append(rd(n + D))
        lines.append(q("s_waitcnt lgkmcnt(%d)" % min(D, nfrag - 1 - n)))
        for j in range(2):
            c = (2 * i + j) * 4
            acc = "a[%d:%d]" % (c, c + 3)
            xb = 32 + (j * NKS + ks) * 4
            x = "a[%d:%d]" % (xb, xb + 3)
            w = "%%%d" % (n % R)
            a_op, b_op = (x, w) if direct else (w, x)
            lines.append("TF_MM(" + q("v_mfma_f32_16x16x32_f16 %s, %s, %s, %s" % (acc, a_op, b_op, "0" if ks == 0 else acc)) + ")")
    lines.append(q("s_nop 15"))
    lines.append(q("s_nop 15"))
    return " \\\n  ".join(lines)


def loadx():
    lines = []
    for ks in range(NKS):
        for j in range(2):
            b = 32 + (j * NKS + ks) * 4
            lines.append(q("global_load_dwordx4 a[%d:%d], %%%d, off offset:%d" % (b, b + 3, j, ks * 64)))
    return " \\\n  ".join(lines)


def main():
    asmgen.write_inc("gen_tfront_asm.py", "attn_tfront_kloop.inc", "Chunk loop of attn_tfront.hip (see that script for operands).",
                     macros=[("TFRONT_CHUNK_ASM_SWAPPED", chunk(False)), ("TFRONT_CHUNK_ASM_DIRECT", chunk(True)),
                             ("TFRONT_LOADX_ASM", loadx())],
                     clobber=("TFRONT_AGPR_CLOBBERS", ['"a%d"' % i for i in range(112)]))


if __name__ == "__main__":
    main()

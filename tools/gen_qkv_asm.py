#!/usr/bin/env python3
r"""Generates lkgd_amd/csrc/qkv_fused_loop.inc: the panel statement of qkv_fused.hip - LayerNorm + a 320 -> 960 projection
(to_q | to_k | to_v of the spatial transformer block at the 72x128 level, patch/patch.py:416,440-445) in ONE kernel, the
rows read once and the normalised copy never written.
Run from the repo root:  python tools/gen_qkv_asm.py   (--stats for the per-chunk issue-cost table)

The skeleton of the fused feed-forward / one-launch temporal attention (tools/gen_ff_asm.py, gen_tblock_asm.py): one wave = 32
token rows, LayerNorm-ed in registers and parked as MFMA B operands in a[0:79]; one workgroup = 4 waves (one per SIMD) = a
128-token panel; the 960 x 320 weights stream L2 -> LDS as 30 chunks of 21 KiB (a bias fragment + 20 k-step fragments = one
32-row output tile) through a ring of five slots, three chunks ahead (LDS-DMA, counted vmcnt), one barrier per chunk, fragment
reads eight MFMAs ahead across chunk borders.  There is no second product here: tile n's accumulators (H^T = W . z^T: a lane owns
a token, registers run over the tile's 32 output channels) are converted and STORED - two 16-byte global stores per lane after a half-wave exchange - in the
MFMA gaps of tile n + 1, from the other of two accumulator sets.  The stores count in vmcnt like the DMA pieces: every counted
wait is computed from the statement's own issue log (the statement is straight-line), not from a fixed formula.

Register plan (named, clobbered): v[24:55] two accumulator tiles, v[56:71] two packed tiles (8 registers each), v[72:103]
fragment ring; a[0:79] z^T, a[80:83] the ones operand of the bias k-step.  Checks: the rule table of tools/asmgen.py.
"""
import os

import asmgen
from asmgen import Ins, R, ar, v, vr

VB = 24
ACC = [VB, VB + 16]
PK = [VB + 32, VB + 40]
NRING = 8
RING = VB + 48
TMP = RING + 4 * NRING
VEND = TMP + 2
C_IN = int(os.environ.get("QKV_GEN_C", "320"))      # 320 (30 tiles, the 72x128 level) or 640 (60 tiles, the 36x64 level)
assert C_IN in (320, 640)
NKS = C_IN // 16
PARTS = NKS // 20         # chunks per tile: a chunk is the bias fragment + 20 k-steps, or 20 further k-steps (<= 21 KiB)
ZF, ONESB, AEND = 0, 4 * NKS, 4 * NKS + 4
W1_FR = 21
W1_BYTES = W1_FR * 1024
W2_BYTES = 20 * 1024
SLOT = 24576
AHEAD = int(os.environ.get("QKV_GEN_AHEAD", "3"))      # chunks in flight ahead of the one that becomes visible
NSLOT = AHEAD + 2
WAITN = 4
NTILE = 3 * C_IN // 32    # 3 C output channels
NCH = NTILE * PARTS
RATE = 2
SP = 68                   # s[68:69]: the weight stream pointer


class Gen(asmgen.ChunkRing):
    SLOT, SP, RING, NRING = SLOT, SP, RING, NRING
    PRESET = R(ZF, 4 * NKS, "a")
    KNOB_ENV, KNOB_DROPS = "QKV_GEN_KNOB", {"nomfma": ("mfma",)}      # (and "nostore", "norows")

    def __init__(self):
        asmgen.ChunkRing.__init__(self)
        self.queue = []          # Ins or ("GATE", ring-MFMA position)
        self.mpos = 0
        self.vmlog = []          # issue order of vector-memory operations: ("dma", chunk) / ("st", tile) / ("row", k-step)

    def e(self, text, kind, rd=(), wr=(), **meta):
        self.append(Ins(text, kind, rd, wr, **meta))

    def append(self, i):
        self.ins.append(i)
        if i.kind == "vmem":
            self.vmlog.append(i.meta["vm"])

    def vm_after(self, chunk):
        """vector-memory operations issued behind the last DMA piece of `chunk` (all of them, if its pieces are older than this
        statement): what a counted wait for that chunk may leave in flight"""
        last = max((k for k, t in enumerate(self.vmlog) if t == ("dma", chunk)), default=-1)
        return len(self.vmlog) - 1 - last

    # ---- the queued work of a finished tile: conversions and stores ------------------------------------------------------
    def q_store(self, n):
        a, p = ACC[n & 1], PK[n & 1]
        for r in range(0, 16, 2):
            self.queue.append(Ins("v_cvt_pk_f16_f32 %s, %s, %s" % (v(p + r // 2), v(a + r), v(a + r + 1)), "valu",
                                  rd=[("v", a + r), ("v", a + r + 1)], wr=[("v", p + r // 2)], tile=n))
        # accumulator registers 4 g .. 4 g + 3 of lane (token, hh) are channels 32 n + 8 g + 4 hh + 0..3: packed, group g is the
        # register pair p + 2 g.  One half-wave exchange per dword of a group PAIR (v_permlane32_swap: lanes 32..63 of the first
        # operand <-> lanes 0..31 of the second) leaves lanes 0..31 with channels 16 j + 0..7 and lanes 32..63 with 16 j + 8..15
        # in four consecutive registers: one 16-byte store per pair (cdna_hip_programming.md T21; the row pointer of the upper
        # half-wave is 16 bytes further).  Its operands must have been written >= 2 wait states before (checked below).
        for j in range(2):
            for d in range(2):
                a, b = p + 4 * j + d, p + 4 * j + 2 + d
                self.queue.append(Ins("v_permlane32_swap_b32 %s, %s" % (v(a), v(b)), "swap", rd=[("v", a), ("v", b)],
                                      wr=[("v", a), ("v", b)], tile=n))
        for j in range(2):
            self.queue.append(Ins("global_store_dwordx4 %%[orow], %s, off offset:%d" % (vr(p + 4 * j, 4), 64 * n + 32 * j), "vmem",
                                  rd=R(p + 4 * j, 4), vm=("st", n), tile=n))

    def dispense(self):
        k = 0
        while self.queue and k < RATE:
            it = self.queue[0]
            if isinstance(it, tuple):
                if self.mpos < it[1]:
                    break
                self.queue.pop(0)
                continue
            self.append(self.queue.pop(0))
            k += 1

    def dma_items(self, chunk, wrap):
        first = chunk % PARTS == 0           # the chunk that opens a tile carries the bias fragment (a 21st KiB)
        self.dma_tag = ("dma", chunk)
        return self.dma_pairs(chunk % NSLOT, first, None if wrap else (W1_BYTES if first else W2_BYTES))

    # ---- one chunk = (part of) one 32-channel output tile ---------------------------------------------------------------------
    def chunk(self, c):
        n, part = divmod(c, PARTS)
        self.e("; ---- tile %d part %d" % (n, part), "comment")
        nfr, slot = (W1_FR if part == 0 else 20), c % NSLOT
        last = c == NCH - 1
        tags = [(c, i) for i in range(nfr)]
        d = ACC[n & 1]
        if part == 0:
            for it in self.queue:       # the accumulator set of tile n - 2 must have been converted
                if isinstance(it, Ins):
                    assert not (set(R(d, 16)) & set(it.rd)), ("tile %d overwrites accumulators still to be converted" % n, it.text)
        for i in range(nfr):
            if i == nfr - NRING and not last:
                assert not self.pending_dma, "the previous chunk's DMA is still being issued"
                # chunk c + 1 becomes visible: own pieces landed (whatever was issued behind them may stay in flight)
                wait_n = self.vm_after(c + 1)
                assert wait_n <= 63, wait_n
                self.e("s_waitcnt vmcnt(%d)" % wait_n, "waitvm")
                self.e("s_barrier", "barrier")
                pre = c + 1 + AHEAD              # the next panel's first chunks from the last chunks on
                self.pending_dma = self.dma_items(pre, wrap=(pre % NCH == NCH - 1))
            self.dma_first()
            if i % WAITN == 0:
                self.e("WAITFRAG", "waitfrag", frag=tags[min(i + WAITN - 1, nfr - 1)])
            rs = self.ringpos % NRING
            self.ringpos += 1
            reg = RING + 4 * rs
            if part == 0 and i == 0:
                self.e("v_mfma_f32_32x32x16_f16 %s, %s, %s, 0" % (vr(d, 16), vr(reg, 4), ar(ONESB, 4)), "mfma",
                       rd=R(reg, 4) + R(ONESB, 4, "a"), wr=R(d, 16), frag=tags[i], acc=False)
            else:
                ks = 20 * part + (i - 1 if part == 0 else i)
                self.e("v_mfma_f32_32x32x16_f16 %s, %s, %s, %s" % (vr(d, 16), vr(reg, 4), ar(ZF + 4 * ks, 4), vr(d, 16)), "mfma",
                       rd=R(reg, 4) + R(ZF + 4 * ks, 4, "a") + R(d, 16), wr=R(d, 16), frag=tags[i], acc=True)
            self.mpos += 1
            j = i + NRING
            if j < nfr:
                self.read_frag(slot, j, rs, tags[j])
            elif not last:
                self.read_frag((c + 1) % NSLOT, j - nfr, rs, (c + 1, j - nfr))
            self.dma_second()
            self.dispense()
        if part == PARTS - 1:
            self.queue.append(("GATE", self.mpos + 3))
            self.q_store(n)

    # ---- the statement of one panel ---------------------------------------------------------------------------------------
    def build(self):
        e = self.e
        assert NCH % NSLOT == 0, (NCH, NSLOT)
        e("s_mov_b32 s%d, %%[splo]" % SP, "salu")
        e("s_mov_b32 s%d, %%[sphi]" % (SP + 1), "salu")
        e("v_and_b32_e32 %s, 0x3c003c00, %%[hmask]" % v(TMP), "valu", wr=[("v", TMP)])
        e("v_accvgpr_write_b32 a%d, %s" % (ONESB, v(TMP)), "valu", rd=[("v", TMP)], wr=[("a", ONESB)])
        for i in range(1, 4):
            e("v_accvgpr_write_b32 a%d, 0" % (ONESB + i), "valu", wr=[("a", ONESB + i)])
        # chunks 0..AHEAD-1 of this panel were issued a panel ago (or by the kernel, which then waits for everything itself); the
        # previous statement's LAST stores, issued behind them, may still be in flight (vmcnt retires in order): START_VM
        e("START_WAIT", "startwait")
        e("s_barrier", "barrier")
        self.pending_dma = self.dma_items(AHEAD, wrap=False)
        self.emit_dma_all()
        # the NEXT panel's token rows (this lane: 20 x 16 bytes of its row) into the statement's output registers: issued behind
        # the first MFMAs, in registers long before the statement ends (every later counted wait retires them first)
        if C_IN == 320 and "norows" not in os.environ.get("QKV_GEN_KNOB", "").split("+"):   # (640: 160 row registers do not fit)
            for ks in range(20):
                self.queue.append(Ins("global_load_dwordx4 %%[r%d], %%[xrow], off offset:%d" % (ks, 32 * ks), "vmem", vm=("row", ks)))
        for j in range(NRING):
            self.read_frag(0, j, j, (0, j))
        for c in range(NCH):
            self.chunk(c)
        # the last tile's conversions and stores have no MFMAs left to hide behind
        self.emit_dma_all()
        self.nop(7)
        self.nop(7)
        self.nop(7)
        for it in self.queue:
            if isinstance(it, Ins):
                self.append(it)
        self.queue = []
        self.nop(1)
        start_vm = self.vm_after(NCH + AHEAD - 1)            # this statement's tail = the next statement's head
        for i in self.ins:
            if i.kind == "startwait":
                i.text, i.kind = "s_waitcnt vmcnt(%d)" % start_vm, "waitvm"
        self.start_vm = start_vm
        e("s_mov_b32 %%[splo], s%d" % SP, "salu")
        e("s_mov_b32 %%[sphi], s%d" % (SP + 1), "salu")

    def check_own(self):
        # the token rows are retired by a counted wait: some DMA piece issued behind them is waited for
        rows = [k for k, t in enumerate(self.vmlog) if t[0] == "row"]
        if rows:
            assert any(t[0] == "dma" and t[1] < NCH and k > rows[-1] for k, t in enumerate(self.vmlog)), "row loads never retired"
        # every tile stored exactly once, four pieces
        st = [t for t in self.vmlog if t[0] == "st"]
        assert sorted(st) == sorted([("st", n) for n in range(NTILE) for _ in range(2)]), "stores"

    def keep(self, i, knob):
        if "nostore" in knob and i.kind == "vmem" and i.meta["vm"][0] == "st":
            return []
        return asmgen.ChunkRing.keep(self, i, knob)

    def stats(self):
        print("instructions:", sum(1 for i in self.ins if i.kind not in ("comment", "label")),
              " MFMAs:", sum(1 for i in self.ins if i.kind == "mfma"), " stores:", sum(1 for t in self.vmlog if t[0] == "st"),
              " max counted vmcnt:", max(int(i.text.split("(")[1][:-1]) for i in self.ins if i.kind == "waitvm"))


    def inc(self):
        P = "QK" if C_IN == 320 else "QK%d" % (C_IN // 100)
        D = dict(VB=VB, VEND=VEND, AEND=AEND, ZF=ZF, PARTS=PARTS, W1_BYTES=W1_BYTES, W2_BYTES=W2_BYTES, SLOT=SLOT, NSLOT=NSLOT,
                 NTILE=NTILE, AHEAD=AHEAD)
        return dict(script="gen_qkv_asm.py", name="qkv_fused_loop.inc" if C_IN == 320 else "qkv%d_fused_loop.inc" % C_IN,
                    blurb="Panel statement of qkv_fused.hip (plan: see that script).",
                    defines=[("%s_%s" % (P, k), D[k]) for k in D], macros=[(P + "_PANEL_ASM", self.text())],
                    clobber=(P + "_CLOBBERS", asmgen.clobbers(VB, VEND, AEND, range(SP, SP + 2))))


if __name__ == "__main__":
    asmgen.main(Gen)

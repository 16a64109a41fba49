r"""What the inline-asm generators (tools/gen_*_asm.py) share: the instruction model, the counted lgkmcnt waits, the checks
every generated statement must pass before a file is written, the knob filter, the issue-cost table and the .inc writer.
Imported as `asmgen` by a generator run by path (tools/ is then sys.path[0]) and as `tools.asmgen` from the repository root.

A program is a list of Ins: text, kind, the registers it reads and writes as (file, number) tuples ("v" / "a" are checked;
anything else, e.g. ("vcc", 0) or ("op", name), only takes part in the distance rules) and free meta data.  Kinds:
    mfma valu trans swap (v_permlane32_swap) lds vmem salu nop (n) barrier branch (target) label (name) comment
    waitfrag (frag: a marker, turned into a counted wait by resolve_waits)  waitlgkm (n)  waitall  waitvm
An lds instruction carries frag = the tag of what it reads; an MFMA that consumes a ring fragment carries the same tag (frag
= None or absent: its operands are not ring fragments).  Tags that start with "X" are exchanges (ds_bpermute, out-of-line
reads), not ring fragments: their result registers are ordinary registers that must be waited for before a VALU reads them.
"""
import os
import sys

NL = r"\n\t"


def q(text):
    return '"' + text + NL + '"'


def v(n):
    return "v%d" % n


def vr(a, n):
    return "v[%d:%d]" % (a, a + n - 1)


def ar(a, n):
    return "a[%d:%d]" % (a, a + n - 1)


def R(base, n, f="v"):
    return [(f, base + i) for i in range(n)]


class Ins:
    __slots__ = ("text", "kind", "rd", "wr", "meta")

    def __init__(self, text, kind, rd=(), wr=(), **meta):
        self.text, self.kind, self.rd, self.wr, self.meta = text, kind, tuple(rd), tuple(wr), meta


class Program:
    # ---- what differs between programs in fact
    MFMA_WS = 8              # issue slots an MFMA counts for in the distance rules (32x32x16: 8 passes of 4 cycles)
    LOOP = None              # name of the loop label: check() walks its body twice, resolve_waits() checks the back edge
    LOOP_ENTRY = None        # outstanding fragments declared for every entry of the loop (None: what the first entry brings)
    INHERIT = ()             # labels that are reached only by a branch: they inherit the FIFO of that branch
    PRESET = ()              # registers the kernel has written before the statement
    RING, NRING = 0, 0       # first register and slot count of the fragment ring (4 registers per slot)
    KNOB_ENV = None          # environment variable of the timing knobs ("a+b"); results of a knob build are WRONG
    KNOB_DROPS = {}          # knob -> instruction kinds it removes
    STATS_COST = {"mfma": 8, "trans": 8, "valu": 4, "salu": 4, "lds": 4, "vmem": 4, "waitlgkm": 4, "waitvm": 4, "barrier": 4}

    def __init__(self):
        self.ins = []

    def e(self, text, kind, rd=(), wr=(), **meta):
        self.ins.append(Ins(text, kind, rd, wr, **meta))

    def label(self, name):
        self.e(name + "_%=:", "label", name=name)

    def nop(self, n):
        self.e("s_nop %d" % n, "nop", n=n)

    # ---- counted lgkmcnt waits ------------------------------------------------------------------------------------------
    def resolve_waits(self):
        """Turns every WAITFRAG marker into s_waitcnt lgkmcnt(n), n = LDS operations issued behind the fragment's (they
        return in order).  Walks the list in emission order = the fall-through path.  A marker whose fragment an earlier wait
        has retired since it was read is dropped; one whose fragment was never read is an error.  The back edge of LOOP must
        bring the FIFO the loop was entered with (LOOP_ENTRY: the declared one, which every entry's FIFO must be part of - a
        wait for N outstanding is still correct when fewer are); an INHERIT label takes over the FIFO of the branch to it."""
        out, fifo, retired, entry, saved = [], [], set(), None, {}
        for i in self.ins:
            if i.kind == "lds":
                fifo.append(i.meta["frag"])
                retired.discard(i.meta["frag"])
            elif i.kind == "waitall":
                retired.update(fifo)
                fifo = []
            elif i.kind == "waitfrag":
                fr = i.meta["frag"]
                idx = [k for k, f in enumerate(fifo) if f == fr]
                if not idx:
                    assert fr in retired, ("fragment never read", fr)
                    continue
                keep = len(fifo) - 1 - idx[-1]
                assert keep <= 15, ("lgkmcnt is a 4-bit counter", keep)
                i = Ins("s_waitcnt lgkmcnt(%d)" % keep, "waitlgkm", n=keep)
                retired.update(fifo[:idx[-1] + 1])
                fifo = fifo[idx[-1] + 1:]
            elif i.kind == "label" and i.meta["name"] == self.LOOP:
                if self.LOOP_ENTRY is not None:
                    assert all(f in self.LOOP_ENTRY for f in fifo), (fifo, self.LOOP_ENTRY)
                    fifo = list(self.LOOP_ENTRY)
                entry = list(fifo)
            elif i.kind == "branch" and i.meta["target"] == self.LOOP:
                assert fifo == entry, (fifo, entry)
            elif i.kind == "branch" and i.meta["target"] in self.INHERIT:
                saved[i.meta["target"]] = list(fifo)
            elif i.kind == "label" and i.meta["name"] in self.INHERIT:
                fifo = saved[i.meta["name"]]
            out.append(i)
        self.ins = out

    # ---- checks ---------------------------------------------------------------------------------------------------------
    def walk(self):
        """the straight-line order, the body of LOOP twice (the second walk starts from the state the first leaves)"""
        if self.LOOP is None:
            return self.ins
        a = next(k for k, i in enumerate(self.ins) if i.kind == "label" and i.meta["name"] == self.LOOP)
        b = next(k for k, i in enumerate(self.ins) if i.kind == "branch" and i.meta["target"] == self.LOOP)
        return self.ins[:b] + self.ins[a:b] + self.ins[b:]

    def problems(self):
        """Every rule below holds for every program.  Distances are issue slots between the two instructions: s_nop n counts
        n + 1, an MFMA counts MFMA_WS, labels and comments 0, everything else 1.  A report is made when the distance is
        SMALLER than the figure.

            rule                                                                    distance   from
            MFMA write -> any read or write of the register                         20         the generators (gen_attn_asm.py first)
              (but the next MFMA of the same accumulation chain: acc=True and the register both its C and its D)
            VALU / transcendental / swap write -> MFMA read                         3          "
            VALU / transcendental / swap write -> v_permlane32_swap read            3          LLVM gfx950 hazard rule, 2 wait states
                                                                                               (cdna_hip_programming.md T21)
            transcendental write -> VALU / transcendental / LDS / store read        2          the generators (1 wait state)
            VALU write -> data register of a vector-memory store                    2          gen_qkv_asm.py
            data register of a vector-memory store -> rewritten                     3          gen_qkv_asm.py (2 wait states)
            v / a register read, never written and not in PRESET
            ring MFMA: its four ring registers hold the fragment it names (a register written since holds nothing)
            ring MFMA: that fragment is not behind the last counted wait
            VALU read of an exchange ("X") result not yet waited for
        The distances are those the generators carried before they shared this module; they were not derived again.
        Returns the reports."""
        out = []
        walk = [i for i in self.walk() if i.kind not in ("label", "comment")]
        mfma_wr, valu_wr, trans_wr, store_rd = {}, {}, {}, {}
        pos = 0
        for i in walk:
            for r in i.rd + i.wr:
                chain = i.kind == "mfma" and i.meta.get("acc") and r in i.wr and r in i.rd
                if r in mfma_wr and not chain and pos - mfma_wr[r] < 20:
                    out.append("HAZARD mfma->use %s dist %d: %s" % (r, pos - mfma_wr[r], i.text))
            for r in i.rd:
                if i.kind == "mfma" and r in valu_wr and pos - valu_wr[r] < 3:
                    out.append("HAZARD valu->mfma %s: %s" % (r, i.text))
                if i.kind == "swap" and r in valu_wr and pos - valu_wr[r] < 3:
                    out.append("HAZARD valu->permlane swap %s: %s" % (r, i.text))
                if i.kind in ("valu", "trans", "lds", "vmem") and r in trans_wr and pos - trans_wr[r] < 2:
                    out.append("HAZARD trans->use %s: %s" % (r, i.text))
                if i.kind == "vmem":
                    if r in valu_wr and pos - valu_wr[r] < 2:
                        out.append("HAZARD valu->store data %s: %s" % (r, i.text))
                    store_rd[r] = pos
            for r in i.wr:
                if r in store_rd and pos - store_rd[r] < 3:
                    out.append("HAZARD store data rewritten %s: %s" % (r, i.text))
                for d in (mfma_wr, valu_wr, trans_wr):
                    d.pop(r, None)
                if i.kind == "mfma":
                    mfma_wr[r] = pos
                elif i.kind in ("valu", "trans", "swap"):
                    valu_wr[r] = pos
                    if i.kind == "trans":
                        trans_wr[r] = pos
            pos += i.meta["n"] + 1 if i.kind == "nop" else (self.MFMA_WS if i.kind == "mfma" else 1)
        written = set(self.PRESET)
        for i in walk:
            for r in i.rd:
                if r[0] in ("v", "a") and r not in written:
                    out.append("UNINITIALISED %s read by: %s" % (r, i.text))
                    written.add(r)
            written.update(i.wr)
        holds, pending = {}, []          # register -> tag of the LDS read that wrote it last; tags behind the last wait
        for i in walk:
            if i.kind == "waitlgkm":
                pending = pending[len(pending) - i.meta["n"]:] if i.meta["n"] else []
            elif i.kind == "waitall":
                pending = []
            elif i.kind == "mfma" and i.meta.get("frag") is not None:
                want = i.meta["frag"]
                regs = [r for r in i.rd if r[0] == "v" and self.RING <= r[1] < self.RING + 4 * self.NRING]
                assert len(regs) == 4, i.text
                for r in regs:
                    if holds.get(r) != want:
                        out.append("RING slot %s holds %s, MFMA expects %s" % (r, holds.get(r), want))
                if want in pending:
                    out.append("RING fragment not waited for: %s" % (want,))
            elif i.kind in ("valu", "trans"):
                for r in i.rd:
                    if r in holds and holds[r][0] == "X" and holds[r] in pending:
                        out.append("exchange result not waited for: %s" % i.text)
            for r in i.wr:
                holds.pop(r, None)
            if i.kind == "lds":
                for r in i.wr:
                    holds[r] = i.meta["frag"]
                pending.append(i.meta["frag"])
        return out

    def check_own(self):
        """the assertions only this program has (run after the shared rules)"""

    def check(self):
        out = self.problems()
        print("".join(t + "\n" for t in out), end="")
        assert not out, "%d problems" % len(out)
        self.check_own()

    # ---- text -----------------------------------------------------------------------------------------------------------
    def keep(self, i, knob):
        """what instruction i becomes in the written text under the knobs `knob`: a list of Ins (empty: removed)"""
        return [] if any(i.kind in self.KNOB_DROPS.get(k, ()) for k in knob) else [i]

    def text(self):
        knob = os.environ.get(self.KNOB_ENV, "").split("+") if self.KNOB_ENV else [""]
        return " \\\n  ".join(q(j.text) for i in self.ins if i.kind != "comment" for j in self.keep(i, knob))

    def stats(self):
        """issue cost and instruction counts of every section (a section starts at a comment)"""
        tot, n = {}, {}
        cur = None
        for i in self.ins:
            if i.kind == "comment":
                cur = i.text
                tot[cur], n[cur] = 0, {}
            elif cur is not None:
                tot[cur] += self.STATS_COST.get(i.kind, 0)
                n[cur][i.kind] = n[cur].get(i.kind, 0) + 1
        for k in tot:
            print("%-*s issue cycles %5d (matrix pipe %4d)  %s" % (max(map(len, tot)), k, tot[k], 32 * n[k].get("mfma", 0), n[k]))
        print("instructions:", sum(1 for i in self.ins if i.kind not in ("comment", "label")),
              " MFMAs:", sum(1 for i in self.ins if i.kind == "mfma"))


class ChunkRing(Program):
    """A weight stream that arrives in LDS in chunks of 1-KiB fragments: a ring of SLOT-byte slots filled by LDS-DMA from the
    pointer s[SP:SP+1], fragments read into the register ring ahead of the MFMAs that consume them."""
    SLOT = SP = 0

    def __init__(self):
        Program.__init__(self)
        self.ringpos = 0         # ring MFMAs emitted so far: ring slots rotate over all of them
        self.pending_dma = []    # pairs (M0 write, LDS-DMA) / (pointer low word, high word) still to be issued
        self.dma_half = False
        self.dma_tag = None      # meta "vm" of the LDS-DMA instructions being issued

    def slot_addr(self, slot):
        """(address operand, immediate) of byte 0 of an LDS ring slot: one base register per two slots (16-bit offset field)"""
        return "%%[fa%d]" % (slot // 2), (slot % 2) * self.SLOT

    def read_frag(self, slot, frag_i, ring_slot, tag):
        reg = self.RING + 4 * ring_slot
        base, imm = self.slot_addr(slot)
        self.e("ds_read_b128 %s, %s offset:%d" % (vr(reg, 4), base, imm + frag_i * 1024), "lds", wr=R(reg, 4), frag=tag)

    def dma_pairs(self, slot, bias, adv):
        """this wave's part of a 20-KiB chunk into ring slot `slot` (pieces w + 4 j through the five offset registers; with
        `bias`, a 21st KiB by every wave: same bytes, same place), then the pointer moved by adv bytes (None: back to the
        stream start).  Pairs: the halves go in front of and behind an MFMA, the wait state an M0 write needs."""
        it = [("s_add_u32 m0, %%[ldsw], %d" % (slot * self.SLOT + j * 4096),
               "global_load_lds_dwordx4 %%[vo%d], s[%d:%d]" % (j, self.SP, self.SP + 1)) for j in range(5)]
        if bias:
            it.append(("s_add_u32 m0, %%[lds0], %d" % (slot * self.SLOT + 20480),
                       "global_load_lds_dwordx4 %%[vob], s[%d:%d]" % (self.SP, self.SP + 1)))
        if adv is None:
            it.append(("s_mov_b32 s%d, %%[sp0lo]" % self.SP, "s_mov_b32 s%d, %%[sp0hi]" % (self.SP + 1)))
        else:
            it.append(("s_add_u32 s%d, s%d, %d" % (self.SP, self.SP, adv), "s_addc_u32 s%d, s%d, 0" % (self.SP + 1, self.SP + 1)))
        return it

    def dma_first(self):
        """first half of the next pending pair: goes in FRONT of an MFMA"""
        if self.pending_dma:
            self.e(self.pending_dma[0][0], "salu")
            self.dma_half = True

    def dma_second(self):
        """second half: behind that MFMA"""
        if self.dma_half:
            t = self.pending_dma.pop(0)[1]
            if t.startswith("global_load"):
                self.e(t, "vmem", vm=self.dma_tag)
            else:
                self.e(t, "salu")
            self.dma_half = False

    def emit_dma_all(self):
        while self.pending_dma:
            self.dma_first()
            self.nop(0)
            self.dma_second()


# ---- the .inc file ------------------------------------------------------------------------------------------------------
def clobbers(vb, vend, aend, s):
    """clobber list of a statement with named registers v[vb:vend-1], a[0:aend-1] and the SGPRs `s`"""
    return ['"v%d"' % i for i in range(vb, vend)] + ['"a%d"' % i for i in range(aend)] + ['"s%d"' % i for i in s] + \
        ['"vcc"', '"scc"', '"m0"', '"memory"']


def write_inc(script, name, blurb, defines=(), macros=(), clobber=None):
    """Writes csrc/<name> for tools/<script>, or the path behind -o (then nothing inside the repository is written):
    the header, `#define NAME value` lines, the asm macros (name, text) and the clobber list (name, registers)."""
    tools = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(os.path.dirname(tools), "lkgd_amd", "csrc", name)
    if "-o" in sys.argv:
        out = sys.argv[sys.argv.index("-o") + 1]
    with open(out, "w") as f:
        f.write("// GENERATED by tools/%s - do not edit.  %s\n" % (script, blurb))
        f.write("".join("#define %s %d\n" % d for d in defines))
        f.write("".join("#define %s \\\n  %s\n\n" % m for m in macros))
        f.write("#define %s " % clobber[0] + ", ".join(clobber[1]) + "\n")
    print("wrote", out)


def main(gen):
    """build -> counted waits -> checks -> (--stats) -> file.  gen.inc() returns the arguments of write_inc."""
    g = gen()
    g.build()
    g.resolve_waits()
    g.check()
    if "--stats" in sys.argv:
        g.stats()
    write_inc(**g.inc())

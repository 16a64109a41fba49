"""The inline-asm generators (tools/gen_*_asm.py, tools/asmgen.py): every committed csrc/*.inc is what its generator writes, the
checks the generators rely on report what they are there to report, and the timing knobs still change the text."""
import os
import subprocess
import sys

import pytest

from tools import asmgen
from tools.asmgen import Ins, R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "lkgd_amd", "csrc")

# the recipes of lkgd_amd/csrc/Makefile: (file, script, environment)
RECIPES = [
    ("gemm_wide_ktile.inc", "gen_wide_asm.py", {}),
    ("gemm_resw_kloop.inc", "gen_resw_asm.py", {}),
    ("attn_tfront_kloop.inc", "gen_tfront_asm.py", {}),
    ("attn_spatial_pipe.inc", "gen_attn_asm.py", {}),
    ("attn_spatial_pipe_masked.inc", "gen_attn_asm.py", {"ATTN_GEN_OPT": "w2+mask"}),
    ("attn_tblock_loop.inc", "gen_tblock_asm.py", {}),
    ("qkv_fused_loop.inc", "gen_qkv_asm.py", {}),
    ("qkv640_fused_loop.inc", "gen_qkv_asm.py", {"QKV_GEN_C": "640"}),
    ("ff_fused_loop.inc", "gen_ff_asm.py", {}),
]


def generate(script, env, out):
    base = {k: val for k, val in os.environ.items() if "_GEN_" not in k}
    subprocess.run([sys.executable, "../../tools/" + script, "-o", str(out)], cwd=CSRC, env=dict(base, **env), check=True,
                   stdout=subprocess.DEVNULL)
    with open(out, "rb") as f:
        return f.read()


def tree_state():
    return {n: (os.stat(os.path.join(CSRC, n)).st_mtime_ns, open(os.path.join(CSRC, n), "rb").read())
            for n in sorted(os.listdir(CSRC)) if n.endswith(".inc")}


def test_recipes_cover_every_generated_file():
    assert sorted(r[0] for r in RECIPES) == sorted(n for n in os.listdir(CSRC) if n.endswith(".inc"))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for name, script, env in RECIPES:
        rule = mk[mk.index("\n" + name + ":"):].split("\n")[1:3]
        assert "../../tools/" + script in rule[0] and "../../tools/asmgen.py" in rule[0], rule
        assert rule[1].split() == ["%s=%s" % kv for kv in env.items()] + ["python3", "../../tools/" + script], rule


@pytest.mark.parametrize("name,script,env", RECIPES, ids=[r[0] for r in RECIPES])
def test_committed_inc_is_what_its_generator_writes(name, script, env, tmp_path):
    before = tree_state()
    new = generate(script, env, tmp_path / name)
    assert tree_state() == before, "a run with -o wrote into the tree"
    assert new == before[name][1], "%s is stale: run the recipe of lkgd_amd/csrc/Makefile" % name


@pytest.mark.parametrize("script,name,env", [
    ("gen_ff_asm.py", "ff_fused_loop.inc", {"FF_GEN_KNOB": "valupad"}),
    ("gen_tblock_asm.py", "attn_tblock_loop.inc", {"TB_GEN_KNOB": "novalu"}),
    ("gen_qkv_asm.py", "qkv_fused_loop.inc", {"QKV_GEN_KNOB": "nostore"}),
    ("gen_attn_asm.py", "attn_spatial_pipe.inc", {"ATTN_GEN_KNOB": "noexp"}),
], ids=["ff", "tblock", "qkv", "attn"])
def test_knob_build_differs(script, name, env, tmp_path):
    knob = generate(script, env, tmp_path / name)
    with open(os.path.join(CSRC, name), "rb") as f:
        ref = f.read()
    assert knob != ref


# ---- the checker is itself checked: for every rule a few instructions that break exactly it, and the nearest legal neighbour
RING = 100


def program(ins, **attrs):
    p = asmgen.Program()
    p.RING, p.NRING = RING, 2
    for k, val in attrs.items():
        setattr(p, k, val)
    p.ins = list(ins)
    return p


def nop(n):
    return Ins("s_nop %d" % n, "nop", n=n)


def mfma(wr, rd=(), **meta):
    return Ins("v_mfma", "mfma", rd=rd, wr=wr, **meta)


def valu(wr=(), rd=(), kind="valu"):
    return Ins("v_op", kind, rd=rd, wr=wr)


ACC = R(0, 16)
V5 = [("v", 5)]
# (id, the rule's report, instructions that break it, nearest legal neighbour, program parameters)
HAZARDS = [
    # an MFMA counts 8 slots, s_nop n counts n + 1: the reader sits at distance 19 / 20
    ("mfma_use", "mfma->use", [mfma(ACC), nop(10), valu(rd=ACC[:1])], [mfma(ACC), nop(11), valu(rd=ACC[:1])], {}),
    ("mfma_rewrite", "mfma->use", [mfma(ACC), nop(10), valu(wr=ACC[3:4])], [mfma(ACC), nop(11), valu(wr=ACC[3:4])], {}),
    # the chain exemption is for C = D of an accumulating MFMA only: C = 0 onto a just-written accumulator is a report
    ("mfma_c0_onto_fresh_acc", "mfma->use", [mfma(ACC), mfma(ACC, acc=True)], [mfma(ACC), mfma(ACC, rd=ACC, acc=True)], {}),
    ("mfma_c0_not_a_chain", "mfma->use", [mfma(ACC), mfma(ACC, rd=ACC, acc=False)], [mfma(ACC), nop(11), mfma(ACC, acc=False)], {}),
    ("mfma_weight_1", "mfma->use", [mfma(ACC), nop(15), nop(1), valu(rd=ACC[:1])], [mfma(ACC), nop(15), nop(2), valu(rd=ACC[:1])],
     {"MFMA_WS": 1}),
    ("valu_mfma", "valu->mfma", [valu(V5), nop(0), mfma(ACC, rd=V5)], [valu(V5), nop(1), mfma(ACC, rd=V5)], {}),
    ("trans_mfma", "valu->mfma", [valu(V5, kind="trans"), nop(0), mfma(ACC, rd=V5)], [valu(V5, kind="trans"), nop(1), mfma(ACC, rd=V5)], {}),
    ("valu_swap", "valu->permlane swap", [valu(V5), nop(0), valu(V5, V5, "swap")], [valu(V5), nop(1), valu(V5, V5, "swap")], {}),
    ("trans_valu", "trans->use", [valu(V5, kind="trans"), valu(rd=V5)], [valu(V5, kind="trans"), nop(0), valu(rd=V5)], {}),
    ("trans_trans", "trans->use", [valu(V5, kind="trans"), valu(rd=V5, kind="trans")],
     [valu(V5, kind="trans"), valu(), valu(rd=V5, kind="trans")], {}),
    ("trans_lds", "trans->use", [valu(V5, kind="trans"), Ins("ds_bpermute", "lds", rd=V5, wr=[("v", 6)], frag=("X", 1))],
     [valu(V5, kind="trans"), nop(0), Ins("ds_bpermute", "lds", rd=V5, wr=[("v", 6)], frag=("X", 1))], {}),
    ("trans_store", "trans->use", [valu(V5, kind="trans"), Ins("global_store", "vmem", rd=V5)],
     [valu(V5, kind="trans"), nop(0), Ins("global_store", "vmem", rd=V5)], {}),
    ("valu_store", "valu->store data", [valu(V5), Ins("global_store", "vmem", rd=V5)],
     [valu(V5), nop(0), Ins("global_store", "vmem", rd=V5)], {}),
    ("store_rewritten", "store data rewritten", [Ins("global_store", "vmem", rd=V5), nop(0), valu(V5)],
     [Ins("global_store", "vmem", rd=V5), nop(1), valu(V5)], {"PRESET": V5}),
    ("uninitialised_v", "UNINITIALISED", [valu(rd=V5)], [valu(V5), valu(rd=V5)], {}),
    ("uninitialised_a", "UNINITIALISED", [mfma(ACC, rd=R(8, 4, "a"))], [mfma(ACC, rd=R(7, 4, "a"))], {"PRESET": R(0, 11, "a")}),
    # the body of a loop is walked twice: the MFMA at its end meets the reader at its start
    ("across_back_edge", "mfma->use",
     [valu(ACC[:1]), Ins("L", "label", name="L"), valu(rd=ACC[:1]), nop(15), mfma(ACC), Ins("b", "branch", target="L")],
     [valu(ACC[:1]), Ins("L", "label", name="L"), valu(rd=ACC[:1]), nop(15), mfma(ACC), nop(11), Ins("b", "branch", target="L")],
     {"LOOP": "L"}),
]


@pytest.mark.parametrize("rule,bad,good,attrs", [h[1:] for h in HAZARDS], ids=[h[0] for h in HAZARDS])
def test_hazard_rule_reports_and_neighbour_passes(rule, bad, good, attrs):
    out = program(bad, **attrs).problems()
    # (a store that reads a transcendental result one slot behind it breaks the VALU -> store data rule as well)
    assert out and all(rule in t or (rule == "trans->use" and "valu->store data" in t) for t in out), out
    assert any(rule in t for t in out), out
    assert program(good, **attrs).problems() == []
    with pytest.raises(AssertionError, match="problems"):
        program(bad, **attrs).check()
    program(good, **attrs).check()


def read(slot, tag):
    return Ins("ds_read_b128", "lds", wr=R(RING + 4 * slot, 4), frag=tag)


def wait(tag):
    return Ins("WAITFRAG", "waitfrag", frag=tag)


def use(slot, tag):
    return mfma(ACC, rd=R(RING + 4 * slot, 4) + ACC, frag=tag, acc=True)


def resolved(ins, **attrs):
    p = program(ins, PRESET=ACC, **attrs)
    p.resolve_waits()
    return p


def test_counted_waits():
    a, b = ("c", 0), ("c", 1)
    p = resolved([read(0, a), read(1, b), wait(a), use(0, a), wait(b), use(1, b), wait(b)])
    assert [i.meta["n"] for i in p.ins if i.kind == "waitlgkm"] == [1, 0]       # (the third marker: retired already, dropped)
    assert not any(i.kind == "waitfrag" for i in p.ins) and p.problems() == []


def test_ring_slot_holds_another_fragment():
    a, b = ("c", 0), ("c", 1)
    out = resolved([read(0, a), wait(a), use(0, b)]).problems()
    assert len(out) == 4 and all("RING slot" in t for t in out), out
    out = resolved([read(0, a), wait(a), valu(R(RING + 1, 1)), nop(1), use(0, a)]).problems()      # overwritten since
    assert len(out) == 1 and "RING slot" in out[0], out
    assert resolved([read(0, a), wait(a), use(0, a)]).problems() == []


def test_fragment_consumed_while_pending():
    a, b = ("c", 0), ("c", 1)
    out = resolved([read(0, a), read(1, b), wait(a), use(1, b)]).problems()
    assert len(out) == 1 and "not waited for" in out[0], out
    assert resolved([read(0, a), read(1, b), wait(b), use(1, b)]).problems() == []


def test_exchange_result_read_before_its_wait():
    x = ("X", 1)
    bp = Ins("ds_bpermute_b32", "lds", rd=ACC[:1], wr=[("v", 50)], frag=x)
    out = resolved([bp, valu(rd=[("v", 50)])]).problems()
    assert len(out) == 1 and "exchange result" in out[0], out
    assert resolved([bp, wait(x), valu(rd=[("v", 50)])]).problems() == []


def test_lgkmcnt_is_four_bits():
    reads = [Ins("ds_read_b32", "lds", wr=[("v", 200 + k)], frag=("X", k)) for k in range(17)]
    with pytest.raises(AssertionError, match="4-bit"):
        resolved(reads + [wait(("X", 0))])
    p = resolved(reads[:16] + [wait(("X", 0))])
    assert [i.text for i in p.ins if i.kind == "waitlgkm"] == ["s_waitcnt lgkmcnt(15)"]


def test_wait_for_a_fragment_never_read():
    with pytest.raises(AssertionError, match="never read"):
        resolved([read(0, ("c", 0)), wait(("c", 1))])


def test_loop_back_edge_brings_the_entry_fifo():
    a, b = ("c", 0), ("c", 1)
    loop, back = Ins("L", "label", name="L"), Ins("b", "branch", target="L")
    with pytest.raises(AssertionError):
        resolved([read(0, a), loop, wait(a), use(0, a), read(1, b), read(0, a), back], LOOP="L")
    p = resolved([read(0, a), loop, wait(a), use(0, a), read(1, b), wait(b), use(1, b), read(0, a), back], LOOP="L")
    assert [i.meta["n"] for i in p.ins if i.kind == "waitlgkm"] == [0, 0] and p.problems() == []

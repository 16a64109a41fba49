"""CPU-side checks of the product's host logic (no kernels run): the debug knobs are per thread, the scheduler host
tables equal the reference's KAT, state-dict compatibility with the diffusers names, weight packing layouts, patch API
bookkeeping, loud failure without a GPU."""
import ctypes
import json
import os
import sys
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_debug_knobs_are_per_thread():
    """include/lkgd_hip_debug.h: a knob set by one host thread does not reach another thread's launches ("no global
    state; safe to call from multiple host threads").  lkgd_gemm_wide_tile_n is a host-side introspection of the tile rule that
    honours the forced width, and lkgd_groupnorm_chunks honours the chunk-size knobs: both are read from two threads at once."""
    import threading
    from lkgd_amd import _lib
    lib = _lib.lib()
    assert lib.lkgd_gemm_wide_tile_n(1280) == 320
    base_chunks = lib.lkgd_groupnorm_chunks(14 * 9216, 320)
    seen, gate_a, gate_b = {}, threading.Event(), threading.Event()

    def thread_a():
        lib.lkgd_debug_set_wide_tile_n(256)
        lib.lkgd_debug_set_gn_apply_kb(64)
        seen["a"] = (lib.lkgd_gemm_wide_tile_n(1280), lib.lkgd_groupnorm_chunks(14 * 9216, 320))
        gate_a.set()
        gate_b.wait(10)                                   # stay alive, knob set, while thread b looks
        seen["a2"] = lib.lkgd_gemm_wide_tile_n(1280)
        lib.lkgd_debug_set_wide_tile_n(0)

    def thread_b():
        gate_a.wait(10)
        seen["b"] = (lib.lkgd_gemm_wide_tile_n(1280), lib.lkgd_groupnorm_chunks(14 * 9216, 320))
        lib.lkgd_debug_set_wide_tile_n(320)
        gate_b.set()

    ta, tb = threading.Thread(target=thread_a), threading.Thread(target=thread_b)
    ta.start(); tb.start(); ta.join(); tb.join()
    assert seen["a"][0] == 256 and seen["a2"] == 256 and seen["a"][1] != base_chunks
    assert seen["b"] == (320, base_chunks)
    assert lib.lkgd_gemm_wide_tile_n(1280) == 320 and lib.lkgd_groupnorm_chunks(14 * 9216, 320) == base_chunks   # this thread: untouched


def test_gemm_desc_validation_without_gpu():
    """argument errors are reported before anything touches the device"""
    from lkgd_amd import _lib
    d = _lib.GemmDesc()
    assert _lib.lib().lkgd_gemm_f16(ctypes.byref(d), None) == -1      # LKGD_E_NULL
    # small maps are cut down to 8-KiB chunks (12 rows of 320 channels, 8 rows of 1280); large ones keep the 32-KiB apply chunks
    assert _lib.lib().lkgd_groupnorm_chunks(129, 320) == 11 and _lib.lib().lkgd_groupnorm_chunks(576, 1280) == 72
    assert _lib.lib().lkgd_groupnorm_chunks(14 * 9216, 320) == (14 * 9216 + 50) // 51


def test_scheduler_tables_equal_reference_kat():
    from lkgd_amd.scheduler import EulerDiscreteScheduler
    with open(os.path.join(REPO, "tests", "golden", "scheduler_kat.json")) as f:
        kat = json.load(f)
    for c in kat["cases"]:
        s = EulerDiscreteScheduler(**kat["config"])
        s.set_timesteps(c["n"])
        assert torch.equal(s.sigmas, torch.tensor(c["sigmas"]))
        # timesteps = 0.25 * log(sigma), the reference's float32 expression: bit for bit as this host evaluates it, and within
        # one ulp of the table (float32 log rounds differently on different CPUs; the table's host rounded these correctly)
        kat_t = torch.tensor(c["timesteps"])
        assert torch.equal(s.timesteps, torch.stack([0.25 * x.log() for x in s.sigmas[:-1]]))
        assert torch.all((s.timesteps == kat_t) | (torch.nextafter(kat_t, s.timesteps) == s.timesteps))
        assert float(s.init_noise_sigma) == c["init_noise_sigma"]
        assert s.order == 1 and s.step_index is None
    s = EulerDiscreteScheduler.from_svd_config()
    s.set_timesteps(25)
    with pytest.raises(ValueError):
        s.step(torch.zeros(1), 3, torch.zeros(1))          # integer timestep guard (:458-469)


def test_state_dict_names_match_diffusers_tree():
    from lkgd_amd import unet as pu
    from oracle import unet as ou
    for ocls, pcls in ((ou.UNetSpatioTemporalConditionControlNetModel, pu.UNetSpatioTemporalConditionControlNetModel),
                       (ou.UNetSpatioTemporalConditionModel, pu.UNetSpatioTemporalConditionModel)):
        with torch.device("meta"):
            o, p = ocls(ou.SVD_CONFIG), pcls(pu.UNetConfig())
        so, sp = o.state_dict(), p.state_dict()
        assert set(so) == set(sp)
        assert all(so[k].shape == sp[k].shape for k in so)
    assert sum(v.numel() for v in sp.values()) == 1_524_623_082 + 726_796
    names = {type(m).__name__ for m in p.modules()}
    assert {"BasicTransformerBlock", "TemporalBasicTransformerBlock"} <= names   # what patch looks for
    assert p.config.in_channels == 8 and p.config.num_frames == 14 and p.add_embedding.linear_1.in_features == 768
    blk = p.down_blocks[0].attentions[0].transformer_blocks[0]
    for a in ("attn1", "attn2", "norm1", "norm2", "norm3", "ff", "norm_type", "pos_embed", "only_cross_attention",
              "_chunk_size", "_chunk_dim"):
        assert hasattr(blk, a), a
    assert blk.attn1.out_dim == 320


def test_packing_layouts():
    from lkgd_amd import packing as pk
    g = torch.Generator().manual_seed(0)
    w = torch.randn(6, 128, 3, 3, generator=g)
    p = pk.pack_conv3x3(w)
    assert p.shape == (6, 9 * 128) and p.dtype == torch.float16
    # k = ((ky * (Cin/64) + c // 64) * 3 + kx) * 64 + c % 64   (include/lkgd_hip.h section 1)
    for (ky, kx, c) in ((1, 2, 3), (0, 0, 64), (2, 1, 127)):
        assert torch.equal(p[2, ((ky * 2 + c // 64) * 3 + kx) * 64 + c % 64], w[2, c, ky, kx].half())
    w8 = torch.randn(5, 8, 3, 3, generator=g)
    p = pk.pack_conv3x3_c8(w8)
    assert p.shape == (5, 128) and torch.equal(p[:, 72:], torch.zeros(5, 56, dtype=torch.float16))
    assert torch.equal(p[1, 4 * 8 + 7], w8[1, 7, 1, 1].half())
    wt = torch.randn(6, 4, 3, 1, 1, generator=g)
    p = pk.pack_tconv3(wt)
    assert torch.equal(p[3, 2 * 4 + 1], wt[3, 1, 2, 0, 0].half())
    perm = pk.geglu_perm(128, 32)
    assert perm[:32].tolist() == list(range(32)) and perm[32:64].tolist() == list(range(128, 160))
    assert perm[64:96].tolist() == list(range(32, 64)) and sorted(perm.tolist()) == list(range(256))
    perm = pk.geglu_perm(1280, 80)
    assert perm[:80].tolist() == list(range(80)) and perm[80:160].tolist() == list(range(1280, 1360))
    assert pk.geglu_half(2560) == 32 and pk.geglu_half(512) == 32


def test_patch_api_bookkeeping():
    from lkgd_amd import patch
    from lkgd_amd import unet as pu
    from oracle import unet as ou
    m = pu.UNetSpatioTemporalConditionControlNetModel(pu.UNetConfig(**ou.TINY_CONFIG.__dict__))
    patch.apply_patch(m, flip=True, with_spatial_block=True, with_temporal_block=False)
    sp = [b for b in m.modules() if type(b).__name__ == "BasicTransformerBlock"]
    tp = [b for b in m.modules() if type(b).__name__ == "TemporalBasicTransformerBlock"]
    assert all(b.enable_joint_attention for b in sp) and not any(b.enable_joint_attention for b in tp)
    assert m._tome_info["args"]["flip"] is True
    patch.initialize_joint_layers(m)
    assert all(hasattr(b, "attn1n") and float(b.conv1n.weight.abs().sum()) == 0.0 for b in sp)
    assert any(k.endswith("attn1n.to_q.weight") for k in m.state_dict())      # A.10 hook names
    patch.set_joint_attention_mask(m, [0, 1, 0, 1])
    patch.set_joint_scale(m, 0.25)
    assert all(b.joint_scale == 0.25 for b in sp)
    patch.set_joint_attention(m, False, name_filter="down_blocks")
    assert not m.down_blocks[0].attentions[0].transformer_blocks[0].enable_joint_attention
    assert m.mid_block.attentions[0].transformer_blocks[0].enable_joint_attention
    patch.update_patch(m, foo=3)
    assert patch.collect_from_patch(m, "foo")
    patch.remove_patch(m)
    assert not any(b.enable_joint_attention for b in sp)
    # partner permutation for masks [0,1,0,1], B=4, F=3 (patch.py:466-475)
    patch.apply_patch(m, flip=False)
    patch.set_joint_attention_mask(m, [0, 1, 0, 1])
    ctx = pu.Ctx(4, 3, 2, 2, torch.device("cpu"))
    m._joint_maps(ctx)
    assert ctx.spatial_partner.tolist() == [3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8]
    assert ctx.temporal_partner.tolist() == [1, 0, 3, 2]
    m._tome_info["args"]["flip"] = True
    m._joint_maps(ctx)
    assert ctx.spatial_partner.tolist() == [5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6]
    # the LoRA-mask entry points work on lkgd_amd.lora.Linear wrappers (tests/test_lora.py); without wrappers they are no-ops
    assert patch.hack_lora_forward(m) is m and patch.set_patch_lora_mask(m, "xy_lora", [1, 0, 1, 0]) is m
    assert m.lora_mask["xy_lora"].tolist() == [True, False, True, False]
    from lkgd_amd import patch_FSM
    with pytest.raises(AttributeError):
        patch_FSM.initialize_joint_lora(m, "a", "b")       # commented out in the reference's ToMeBlock (patch_FSM.py:107-120)


def test_forward_fails_loudly_without_gpu():
    from lkgd_amd import LkgdHipError
    from lkgd_amd import unet as pu
    from oracle import unet as ou
    m = pu.UNetSpatioTemporalConditionControlNetModel(pu.UNetConfig(**ou.TINY_CONFIG.__dict__))
    with pytest.raises(LkgdHipError):
        m(torch.zeros(1, 2, 8, 8, 8), 1.0, torch.zeros(1, 1, 1024), added_time_ids=torch.zeros(1, 3))
    with pytest.raises(LkgdHipError):
        pu.Attention(64, None, 4, 16)          # head_dim != 64 is refused at construction


def test_product_does_not_import_the_oracle():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import lkgd_amd, lkgd_amd.unet, lkgd_amd.pipeline, lkgd_amd.patch, "
            "lkgd_amd.scheduler, lkgd_amd.lk_fuse, lkgd_amd.dist; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'" % REPO)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_fsm_track_tables_match_reference_indexing():
    """host side of the FSM hook (patch_FSM.py:381-403): CSR inversion of the tracks == what scatter_add would visit"""
    from types import SimpleNamespace
    from lkgd_amd import patch_FSM
    from lkgd_amd._lib import LkgdHipError
    g = torch.Generator().manual_seed(3)
    pairs, P, fh, fw = 3, 50, 5, 7
    src = torch.stack([torch.randint(0, 2 * fw, (pairs, P), generator=g),
                       torch.randint(0, 2 * fh, (pairs, P), generator=g)], -1).float()
    dst = torch.stack([torch.randint(-4, 2 * fw + 4, (pairs, P), generator=g),
                       torch.randint(-4, 2 * fh + 4, (pairs, P), generator=g)], -1).float()
    vis = (torch.rand(pairs, P, generator=g) > 0.3).float()
    blk = SimpleNamespace(_tome_info={"fsm_tables": {}}, track=(src, dst, vis), track_res=(2 * fh, 2 * fw))
    ctx = SimpleNamespace(H=fh, W=fw, HW=fh * fw, N=2 * pairs, B=1, F=2 * pairs, b0=0, f0=0, B_total=1, F_total=2 * pairs,
                          device=torch.device("cpu"))
    (off, pt, gi, v), (boff, bpt, bgi, _) = patch_FSM.track_tables(blk, ctx)
    # a sharded rank (round 6): entries [b0, b0 + B) x frames [f0, f0 + F) of a 2-entry x 6-frame call take their pairs' rows
    if pairs == 3:
        blk6 = SimpleNamespace(_tome_info={"fsm_tables": {}}, track=(torch.cat([src, src]), torch.cat([dst, dst]),
                                                                     torch.cat([vis, 1.0 - vis])), track_res=(2 * fh, 2 * fw))
        c2 = SimpleNamespace(H=fh, W=fw, HW=fh * fw, N=2, B=1, F=2, b0=1, f0=4, B_total=2, F_total=6, device=torch.device("cpu"))
        (_, _, gi2, v2), _ = patch_FSM.track_tables(blk6, c2)          # global pair (1 * 6 + 4) / 2 = 5 = the second copy's pair 2
        assert torch.equal(gi2, gi.reshape(pairs, -1)[2].reshape(-1)) and torch.equal(v2, 1.0 - v.reshape(pairs, -1)[2].reshape(-1))
    assert off.dtype == torch.int32 and off.numel() == pairs * fh * fw + 1 and int(off[-1]) == pairs * P
    sidx = (src / 2).long()
    sidx = sidx[..., 0] + sidx[..., 1] * fw
    didx = (dst / 2).long()
    didx = didx[..., 0].clamp(0, fw - 1) + didx[..., 1].clamp(0, fh - 1) * fw
    for table, tgt, gat, o_, p_ in ((0, sidx, didx, off, pt), (1, didx, sidx, boff, bpt)):
        g_ = gi if table == 0 else bgi
        for pair in range(pairs):
            for cell in range(fh * fw):
                want = [pair * P + k for k in range(P) if int(tgt[pair, k]) == cell]     # increasing point order
                r = pair * fh * fw + cell
                assert p_[int(o_[r]):int(o_[r + 1])].tolist() == want
        assert g_.tolist() == gat.reshape(-1).tolist()
    assert torch.equal(v, vis.reshape(-1))
    assert patch_FSM.track_tables(blk, ctx) is blk._tome_info["fsm_tables"][(fh, fw, 2 * pairs, 0, 0, 1, 2 * pairs)]   # cached
    bad = SimpleNamespace(_tome_info={"fsm_tables": {}}, track=(src - 100.0, dst, vis), track_res=(2 * fh, 2 * fw))
    with pytest.raises(LkgdHipError):
        patch_FSM.track_tables(bad, ctx)
    with pytest.raises(LkgdHipError):
        patch_FSM.track_tables(SimpleNamespace(_tome_info={}, track=None, track_res=None), ctx)


def test_lk_fuse_cache_never_serves_a_recycled_address(monkeypatch):
    """the one-entry cache of the latent-knowledge fuse owns its key tensors: 20 freshly allocated, same-shape,
    different-content embeddings (the allocator hands addresses back) all get their own result; the same objects hit.  (The
    fuse itself is a HIP launch since round 5 - tests/test_unet_gpu.py -; here a host stand-in computes a value that depends on
    every input, the cache logic is what is under test.)"""
    from lkgd_amd import lk_fuse as lf
    from lkgd_amd import unet as pu
    from oracle import unet as ou
    m = pu.UNetSpatioTemporalConditionModel(pu.UNetConfig(**ou.TINY_CONFIG.__dict__))
    with pytest.raises(lf.LkgdHipError):
        lf.lk_fuse(m, torch.zeros(2, 1, 1024), torch.zeros(1, 1, 1000), torch.zeros(1, 1, 1000))     # no CPU path
    calls = []

    def stand_in(unet, e, d, f):
        calls.append(1)
        return (e * 2.0 + d.sum() - f.sum()).half()
    monkeypatch.setattr(lf, "lk_fuse", stand_in)
    g = torch.Generator().manual_seed(5)
    d, f = torch.randn(1, 1, 1000, generator=g), torch.randn(1, 1, 1000, generator=g)
    for i in range(20):
        e = torch.randn(2, 1, 1024, generator=g)           # fresh tensor, very likely a recycled address
        got = lf.lk_fuse_cached(m, e, d, f)
        assert torch.equal(got, stand_in(m, e, d, f)), i
        n = len(calls)
        assert lf.lk_fuse_cached(m, e, d, f) is got and len(calls) == n          # same objects, unchanged: a hit
        del e, got
    e = torch.randn(2, 1, 1024, generator=g)
    a = lf.lk_fuse_cached(m, e, d, f)
    e.mul_(2.0)                                             # in-place change bumps the version: recompute
    assert not torch.equal(lf.lk_fuse_cached(m, e, d, f), a)


def test_controlnet_condition_cache_owns_its_key():
    from lkgd_amd import controlnet as pc
    from lkgd_amd import unet as pu
    from oracle import unet as ou
    c = pc.ControlNetSDVModel(pu.UNetConfig(**ou.TINY_CONFIG.__dict__))
    calls = []

    class _Emb:
        def run_until_out(self, cond):
            calls.append(float(cond.sum()))
            return torch.full((2 * 4 * 8 * 8, 4), float(cond.sum())), 8, 8
    object.__setattr__(c, "controlnet_cond_embedding", _Emb())
    c.__dict__["_modules"].pop("controlnet_cond_embedding", None)
    for i in range(6):
        cond = torch.full((2, 4, 3, 64, 64), float(i))      # fresh same-shape tensor per "call"
        t = c._cond_tokens(cond, 2, 4, 8, 8)
        assert float(t[0, 0]) == float(cond.sum())
        assert c._cond_tokens(cond, 2, 4, 8, 8) is t
        del cond, t
    assert len(calls) == 6


def test_resident_weight_kernel_has_no_register_spills():
    """lkgd_amd/csrc/gemm_resw.hip issues and awaits its epilogue loads by hand (inline asm, counted vmcnt): spill code
    between a load and its wait would save a register whose data has not arrived.  Every instantiation the launcher can
    pick must therefore be allocated without scratch spills inside its 96-register budget (hipcc cross-compiles here)."""
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    src = os.path.join(REPO, "lkgd_amd", "csrc", "gemm_resw.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-inline-asm",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = [(n, s, c) for n, s, c in zip(names, spills, scratch) if "lkgd_gemm_resw_kernel" in n]
    assert len(kernels) >= 30, len(kernels)
    bad = [k for k in kernels if k[1] or k[2]]
    assert not bad, bad


@pytest.mark.parametrize("src,kernel,agprs", [("ff_fused.hip", "ff_fused_kernel", 244), ("attn_spatial_pipe.hip", "attn_pipe_kernel", 108),
                                              ("attn_tblock.hip", "tattn_block_kernel", 244), ("qkv_fused.hip", "ln_qkv_kernel", (84, 164))])
def test_generated_loop_kernels_keep_their_accumulation_registers(src, kernel, agprs, tmp_path):
    """ff_fused.hip / attn_spatial_pipe.hip keep state in accumulation registers ACROSS their asm statements (Y^T and z^T; Q and
    O), which the compiler knows nothing about: it must never place values of its own there.  Checked on the ISA: every
    instantiation allocates exactly the accumulation registers the generated loop names, has no scratch spills, and no
    compiler-generated instruction (outside the #ASMSTART / #ASMEND blocks) touches an accumulation register."""
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path / "k.o"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-inline-asm", "-mllvm",
                        "-amdgpu-spill-vgpr-to-agpr=0", "--save-temps=obj", "-c", os.path.join(REPO, "lkgd_amd", "csrc", src),
                        "-o", str(out)], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    isa = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert len(isa) == 1
    text = open(tmp_path / isa[0]).read()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from check_agpr_isa import check          # the same check lkgd_amd/csrc/Makefile runs after compiling these objects
    problems = check(text, kernel, agprs if isinstance(agprs, tuple) else (agprs,))
    assert not problems, problems[:10]
    assert check(text.replace("#ASMEND", "#ASMEND\n\tv_accvgpr_write_b32 a3, v1", 1), kernel,
                 agprs if isinstance(agprs, tuple) else (agprs,)), "the check must notice a compiler write to an a-register"


def test_isa_identity_compares_everything_but_the_source_hash():
    """tools/isa_identity.py, the gate of a refactor that must leave every kernel alone: two device-ISA texts are the same if
    they differ in nothing but their __hip_cuid_<hash of the source text> lines; one changed instruction, or one changed
    metadata value, is a difference, and it is reported with the kernel it belongs to."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from isa_identity import compare
    def isa(cuid, op="v_add_f32_e32 v1, v2, v3", vgprs=12):
        return "\n".join([
            '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"', "\t.text",
            "\t.protected\tk_one ; -- Begin function k_one", "\t.type\tk_one,@function", "k_one:", "\ts_load_dwordx2 s[0:1], s[0:1], 0x0",
            "\ts_endpgm", "\t.amdhsa_kernel k_one", "\t\t.amdhsa_next_free_vgpr 4", "\t.end_amdhsa_kernel",
            "\t.protected\tk_two ; -- Begin function k_two", "\t.type\tk_two,@function", "k_two:", "\t" + op, "\ts_endpgm",
            "\t.amdhsa_kernel k_two", "\t\t.amdhsa_next_free_vgpr 12", "\t.end_amdhsa_kernel",
            "\t.type\t__hip_cuid_%s,@object ; @__hip_cuid_%s" % (cuid, cuid), "\t.globl\t__hip_cuid_%s" % cuid, "__hip_cuid_%s:" % cuid,
            "\t.byte\t0", "\t.size\t__hip_cuid_%s, 1" % cuid, "\t.addrsig_sym __hip_cuid_%s" % cuid,
            "\t.amdgpu_metadata", "---", "amdhsa.kernels:",
            "  - .agpr_count:     0", "    .args:", "      - .name:           x", "        .size:           8", "    .name:           k_one",
            "    .vgpr_count:     4",
            "  - .agpr_count:     0", "    .args:", "      - .name:           y", "        .size:           8", "    .name:           k_two",
            "    .vgpr_count:     %d" % vgprs, "...", "\t.end_amdgpu_metadata", ""])
    base = isa("49abf5c6b4c29cac")
    assert compare(base, isa("0123456789abcdef")) is None
    assert compare(base, base) is None
    diff = compare(base, isa("0123456789abcdef", op="v_add_f32_e32 v1, v2, v4"))
    assert diff == ("k_two", "v_add_f32_e32 v1, v2, v3", "v_add_f32_e32 v1, v2, v4"), diff
    assert compare(base, isa("49abf5c6b4c29cac", op="v_add_f32_e32 v1, v2, v4")) is not None      # with the same hash too
    diff = compare(base, isa("0123456789abcdef", vgprs=13))
    assert diff is not None and diff[0] == "k_two", diff
    assert compare(base, base + "\ts_nop 0\n") is not None                                         # a longer text


def test_clip_module_takes_transformers_state_dict_names(tmp_path):
    """lkgd_amd.clip keeps transformers' parameter names (image_encoder/ checkpoints load as they are), round-trips through
    save_pretrained / from_pretrained, ignores the persisted position_ids of older checkpoints, and refuses to run off the GPU"""
    import json
    import pytest
    import torch
    from safetensors.torch import load_file, save_file
    from lkgd_amd._lib import LkgdHipError
    from lkgd_amd.clip import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, patch_size=14,
                           image_size=28, projection_dim=64)
    m = CLIPVisionModelWithProjection(cfg)
    names = set(m.state_dict())
    want = {"vision_model.embeddings.class_embedding", "vision_model.embeddings.patch_embedding.weight",
            "vision_model.embeddings.position_embedding.weight", "vision_model.pre_layrnorm.weight", "vision_model.pre_layrnorm.bias",
            "vision_model.post_layernorm.weight", "vision_model.post_layernorm.bias", "visual_projection.weight"}
    for i in range(2):
        for lin in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2",
                    "layer_norm1", "layer_norm2"):
            want |= {f"vision_model.encoder.layers.{i}.{lin}.weight", f"vision_model.encoder.layers.{i}.{lin}.bias"}
    assert names == want
    try:
        import transformers
        c = transformers.CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                          patch_size=14, image_size=28, projection_dim=64, hidden_act="gelu")
        assert set(transformers.CLIPVisionModelWithProjection(c).state_dict()) == names
    except ImportError:
        pass
    d = tmp_path / "image_encoder"
    m.save_pretrained(str(d))
    sd = load_file(str(d / "model.safetensors"))
    sd["vision_model.embeddings.position_ids"] = torch.arange(5)[None]
    save_file(sd, str(d / "model.safetensors"))
    assert json.load(open(d / "config.json"))["hidden_size"] == 128
    m2 = CLIPVisionModelWithProjection.from_pretrained(str(d), torch_dtype=torch.float32)
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v)
    with pytest.raises(LkgdHipError):
        m2(torch.zeros(1, 3, 28, 28))
    with pytest.raises(LkgdHipError):
        CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=128, num_attention_heads=2, hidden_act="relu"))


# ---------------------------------------------------------------------------------------------------------------------------------
# lkgd_gemm_plan: the dispatcher's decision, asked without a GPU

GEMM_CLASSES = ("plain", "rowmap", "two-source", "geglu", "conv3x3 stride 1 ups 0", "conv3x3 stride 2 ups 0", "conv3x3 stride 1 ups 1",
                "tconv")
#: the operand / epilogue classes each forced variant supports (lkgd_amd/csrc/gemm_plan.cpp::gemm_pick: the row-panel and resident-weight
#: programs take a plain single-source A with K <= 320; the 80-wide GEGLU interleave exists on the 256x320 and resident-weight
#: programs only, the 32-wide one on the others)
VARIANT_CLASSES = {1: GEMM_CLASSES, 2: GEMM_CLASSES, 3: GEMM_CLASSES, 4: GEMM_CLASSES, 5: ("plain", "rowmap", "geglu"),
                   6: ("plain", "rowmap", "geglu"), 7: GEMM_CLASSES}


def test_gemm_plan_reports_what_the_front_end_would_launch():
    from lkgd_amd import _lib, ops
    e = lambda *s, dt=torch.float16: torch.empty(*s, dtype=dt)       # noqa: E731
    M, N, K = 4032, 1280, 3840
    p = ops.gemm_plan(e(M, K), e(N, K), e(M, N), M=M, N=N, K=K, bias=e(N, dt=torch.float32), cus=256)
    assert (p.program, p.k_slices, p.tile_m, p.tile_n) == (ops.GEMM_WIDE, 4, 256, 320)       # 64 tiles, deep K: four equal K slices
    # without the workspace ops.gemm hands to problems below 12288 rows there is nothing to slice into
    p = ops.gemm_plan(e(12288, K), e(N, K), e(12288, N), M=12288, N=N, K=K, cus=256)
    assert p.program == ops.GEMM_WIDE and p.k_slices == 1
    # column sums: asked for -> the tile rows divide the sample, the rows leave through LDS, the block is the tile's rows
    p = ops.gemm_plan(e(16128, 640), e(640, 640), e(16128, 640), M=16128, N=640, K=640, colstats=576, cus=256)
    assert p.program == ops.GEMM_WIDE and p.colstats_block == p.tile_m and 576 % p.tile_m == 0 and p.lds_out == 1
    # rows that are not 16-byte pieces keep the persistent programs out
    p = ops.gemm_plan(e(40000, 320), e(324, 320), e(40000, 324), M=40000, N=324, K=320, cus=256)
    assert p.program in (ops.GEMM_TILE128, ops.GEMM_TILE256, ops.GEMM_MID)
    # the CU count is an input: fewer CUs, fewer idle ones to fill with K slices
    p64 = ops.gemm_plan(e(M, K), e(N, K), e(M, N), M=M, N=N, K=K, cus=64)
    assert p64.program == ops.GEMM_WIDE and p64.k_slices == 1
    with pytest.raises(_lib.LkgdHipError):
        ops.gemm_plan(e(M, K), e(N, K), e(M, N), M=M, N=N, K=K)                 # cus = 0 asks a device
    with pytest.raises(_lib.LkgdHipError):
        ops.gemm_plan(e(M, K + 8), e(N, K + 8), e(M, N), M=M, N=N, K=K + 8, cus=256)     # K % 64: the launch's own LKGD_E_SHAPE
    info = _lib.GemmPlanInfo()
    assert _lib.lib().lkgd_gemm_plan(None, 256, ctypes.byref(info)) == -1
    assert _lib.lib().lkgd_gemm_plan(ctypes.byref(_lib.GemmDesc()), 256, None) == -1


def test_forced_variant_matrix_reaches_every_program():
    """tests/test_kernels_gpu.py runs its GEMM tests under every forced variant, and a forced variant falls back to another program
    where it does not apply.  For every variant and every operand / epilogue class it supports, at least one shape of those tests
    must really run THAT program (at 256 CUs) - otherwise the class is tested on the 128x128 program seven times."""
    import test_kernels_gpu as tk
    from lkgd_amd import _lib, ops
    lib = _lib.lib()
    cases = tk.gemm_plan_cases(ops)
    assert {c for c, _ in cases} == set(GEMM_CLASSES)
    reached = {}
    try:
        for v in sorted(tk.VARIANTS.values()):
            lib.lkgd_debug_set_gemm_variant(v)
            for cls, kw in cases:
                kw = dict(kw)
                p = ops.gemm_plan(kw.pop("a0"), kw.pop("w"), kw.pop("out"), cus=256, **kw)
                assert p.program in ops.GEMM_PROGRAMS.values()
                if p.program == v:
                    reached.setdefault(v, set()).add(cls)
    finally:
        lib.lkgd_debug_set_gemm_variant(0)
    missing = {v: sorted(set(cl) - reached.get(v, set())) for v, cl in VARIANT_CLASSES.items() if set(cl) - reached.get(v, set())}
    assert not missing, f"forced variant -> classes that only ever fall back: {missing}"
    # and nothing runs where it is documented not to apply
    for v, cl in VARIANT_CLASSES.items():
        assert reached[v] <= set(cl), (v, reached[v] - set(cl))


def test_gemm_census_plans_reproduce_from_the_stored_fields():
    """tests/golden/gemm_census.json: every lkgd_gemm_f16 signature of the real forwards with the plan at 256 CUs.  The stored
    plan must be what lkgd_gemm_plan says for the stored fields today - a dispatch change shows up as a diff of that file
    (tools/gemm_census.py --write on a GPU box), reviewed, not as a silent change of what the suite exercises."""
    from tools import gemm_census as gc
    rows = gc.load_table()
    keys = [gc.sig_key(e) for e in rows]
    assert keys == sorted(set(keys)) and len(rows) > 300
    for e in rows:
        assert gc.plan(gc.desc_from_signature(e), gc.PLAN_CUS) == e["plan"], gc.sig_key(e)
        variant, why = gc.second_program(e)
        assert variant == e["second_program"] and why == e.get("no_second_program"), gc.sig_key(e)
        assert set(e["launches"]) <= set(gc.FORWARDS) and all(n > 0 for n in e["launches"].values())
    # the real rows: the four levels of the full forward and a rank's slices
    ms = {e["fields"]["M"] for e in rows}
    assert {258048, 64512, 16128, 4032, 36864, 9216, 2304} <= ms


#: programs / 256x320 tile forms no signature of the census selects, with the reason - everything else must be selected by one
CENSUS_NOT_COVERED = {
    "program 5": "row-panel: the K <= 320 projections it was tuned for run in the fused LayerNorm + projection / feed-forward / "
                 "temporal-attention kernels or, with a residual, on the resident-weight program; no forward issues a LayerNorm-fold "
                 "descriptor at these geometries (tests/test_kernels_gpu.py::test_gemm_layernorm_fold and the forced `rowpanel` "
                 "variant cover the program)",
}
# (form 256x256 left this list with the row ladder of the DiT's block linears: ff1 of the 2B model selects it at 2048 and 4096 rows)


def test_gemm_census_covers_every_program_and_tile_form():
    from lkgd_amd import ops
    from tools import gemm_census as gc
    rows = gc.load_table()
    progs = {e["plan"]["program"] for e in rows}
    forms = {(e["plan"]["tile_m"], e["plan"]["tile_n"]) for e in rows if e["plan"]["program"] == ops.GEMM_WIDE}
    want = {f"program {p}" for p in range(1, 8)} | {f"form {m}x{n}" for m in (256, 192) for n in (320, 256)}
    have = {f"program {p}" for p in progs} | {f"form {m}x{n}" for m, n in forms}
    assert have | set(CENSUS_NOT_COVERED) == want, sorted(want - have - set(CENSUS_NOT_COVERED))
    assert not have & set(CENSUS_NOT_COVERED), f"now covered, drop from the list: {sorted(have & set(CENSUS_NOT_COVERED))}"
    # all three split-K schemes, both output paths of the 256x320 program, both colstats block sizes
    sliced = {e["plan"]["program"] for e in rows if e["plan"]["k_slices"] > 1}
    assert {ops.GEMM_WIDE, ops.GEMM_MID} <= sliced, sliced
    assert {e["plan"]["lds_out"] for e in rows if e["plan"]["program"] == ops.GEMM_WIDE} == {0, 1}
    assert {256, 192, 32} <= {e["plan"]["colstats_block"] for e in rows}


#: the launch sequence of a temporal transformer block's self-attention, written out from the path table of DESIGN.md ("Which launches a transformer block issues"), not computed:
#: (C, heads, F local, F total, HW, token rows, frame shards, masked LoRA, joint, TEMPORAL_GATHER) -> (path, normalised tokens needed)
TEMPORAL_PATHS = [
    # the headline geometries: 72x128 at C = 320 (2 x 14 frames), 36x64 at C = 640, 18x32 and 9x16 at C = 1280
    ((320, 5, 14, 14, 9216, 258048, 1, False, False, False), ("block", False)),
    ((640, 10, 14, 14, 2304, 64512, 1, False, False, False), ("ln_qkv", False)),
    ((1280, 20, 14, 14, 576, 16128, 1, False, False, False), ("chain", True)),
    ((1280, 20, 14, 14, 144, 4032, 1, False, False, False), ("chain", True)),
    # the joint branch reads the normalised tokens: the one-launch block keeps its main branch, everything else runs the chain
    ((320, 5, 14, 14, 9216, 258048, 1, False, True, False), ("block", True)),
    ((640, 10, 14, 14, 2304, 64512, 1, False, True, False), ("chain", True)),
    # masked LoRA: per-entry weights, always the chain
    ((320, 5, 14, 14, 9216, 258048, 1, True, False, False), ("chain", True)),
    ((320, 5, 14, 14, 9216, 258048, 1, True, True, False), ("chain", True)),
    ((640, 10, 14, 14, 2304, 64512, 1, True, False, False), ("chain", True)),
    # F = 16 / 17: the fused temporal kernels hold at most 16 frames
    ((320, 5, 16, 16, 9216, 294912, 1, False, False, False), ("block", False)),
    ((320, 5, 17, 17, 9216, 313344, 1, False, False, False), ("ln_qkv", False)),
    ((320, 5, 17, 17, 64, 2176, 1, False, False, False), ("chain", True)),
    # HW % 16
    ((320, 5, 14, 14, 9224, 258272, 1, False, False, False), ("ln_qkv", False)),
    ((320, 5, 14, 14, 16, 448, 1, False, False, False), ("block", False)),
    ((320, 5, 14, 14, 24, 672, 1, False, False, False), ("chain", True)),
    # heads != 5 at C = 320: no fused temporal kernel; LayerNorm + Q|K|V in one launch from 60 000 rows
    ((320, 4, 14, 14, 9216, 258048, 1, False, False, False), ("ln_qkv", False)),
    ((320, 4, 14, 14, 9216, 60000, 1, False, False, False), ("ln_qkv", False)),
    ((320, 4, 14, 14, 9216, 59999, 1, False, False, False), ("chain", True)),
    # ... and from 30 000 rows at C = 640
    ((640, 10, 14, 14, 2304, 30000, 1, False, False, False), ("ln_qkv", False)),
    ((640, 10, 14, 14, 2304, 29999, 1, False, False, False), ("chain", True)),
    # frames on several GPUs.  A rank of 8 (2 CFG halves x 4 frame shards; 4 of 14 frames): re-sharded by pixels
    ((320, 5, 4, 14, 9216, 36864, 4, False, False, False), ("pixels", False)),
    ((640, 10, 3, 14, 2304, 6912, 4, False, False, False), ("pixels", False)),
    ((320, 5, 4, 14, 9216, 36864, 4, True, True, False), ("pixels", False)),
    ((320, 5, 4, 14, 9216, 36864, 4, False, False, True), ("gather", True)),
    ((320, 5, 4, 14, 9216, 36864, 4, True, True, True), ("gather", True)),
    # HW just below / at frame_shards: a level with fewer pixels than shards keeps the gathered form
    ((64, 1, 2, 4, 3, 6, 4, False, False, False), ("gather", True)),
    ((64, 1, 2, 4, 4, 8, 4, False, False, False), ("pixels", False)),
    ((64, 1, 2, 4, 1, 4, 2, False, True, False), ("gather", True)),
    ((64, 1, 2, 4, 2, 8, 2, False, True, False), ("pixels", False)),
]

#: with LKGD_NO_TBLOCK=1 (the A/B switch tests use as a reference) the `front` path takes the one-launch block's geometries
TEMPORAL_PATHS_NO_TBLOCK = [
    ((320, 5, 14, 14, 9216, 258048, 1, False, False, False), ("front", False)),
    ((320, 5, 16, 16, 16, 512, 1, False, False, False), ("front", False)),
    ((320, 5, 14, 14, 9216, 258048, 1, False, True, False), ("chain", True)),
    ((320, 5, 14, 14, 9216, 258048, 1, True, False, False), ("chain", True)),
    ((320, 5, 17, 17, 9216, 313344, 1, False, False, False), ("ln_qkv", False)),
    ((320, 5, 4, 14, 9216, 36864, 4, False, False, False), ("pixels", False)),
]


def test_temporal_path_table(monkeypatch):
    """lkgd_amd.unet.temporal_path - which launch sequence TemporalBasicTransformerBlock.run takes - returns every row of the
    table: every path, both sides of every threshold, the headline geometries"""
    from lkgd_amd import ops
    from lkgd_amd.unet import temporal_path
    for sw in ("TBLOCK", "TFRONT", "LN_QKV"):          # the table is the shipped configuration, whatever the environment says
        monkeypatch.setattr(ops, sw, True)

    def got(row):
        C_, heads, F, Ft, HW, T, shards, lora, joint, gather = row
        return temporal_path(C_, heads, F, Ft, HW, T, shards, lora=lora, joint=joint, gather=gather)

    for row, want in TEMPORAL_PATHS:
        assert got(row) == want, row
    assert {w[0] for _, w in TEMPORAL_PATHS} == {"block", "ln_qkv", "chain", "pixels", "gather"}
    monkeypatch.setattr(ops, "TBLOCK", False)
    for row, want in TEMPORAL_PATHS_NO_TBLOCK:
        assert got(row) == want, row


# ----------------------------------------------------------------------------------------------------------------------
# loop glue: the wrappers' latents checker and the record-then-replay helper, without a GPU

def test_loop_glue_wrappers_refuse_cpu_latents_before_any_library_call(monkeypatch):
    """the five loop-glue wrappers hand the kernels the bare pointer of ``latents``: a CPU tensor is refused by name before the
    library (or a plan's recording stand-in) is reached"""
    from lkgd_amd import ops
    from lkgd_amd._lib import LkgdHipError

    def reached():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "_L", reached)
    B, F, H, W, T = 2, 3, 2, 2, 5
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)       # noqa: E731
    lat, win = h(B, F, 4, H, W), h(T, 4, H, W)
    gs = torch.ones(F)
    calls = {
        "prepare_unet_input": lambda x: ops.prepare_unet_input(x, h(2 * B, F, 4, H, W), 2, 1.0),
        "cfg_euler_step": lambda x: ops.cfg_euler_step(h(2 * B * F * H * W, 4), x, gs, 2, 1.0, 0.5),
        "cfg_fusion_euler_step": lambda x: ops.cfg_fusion_euler_step(h(2 * B * F * H * W, 4), x, gs, gs, 2, 1.0, 0.5),
        "window_prepare_input": lambda x: ops.window_prepare_input(x, h(T, 4, H, W), 1, F, 2, 1.0),
        "window_cfg_euler_step": lambda x: ops.window_cfg_euler_step(h(4 * F * H * W, 4), x, gs, 1, F, 2, 1.0, 0.5),
    }
    for name, call in calls.items():
        for x in ((win if name.startswith("window") else lat), (win if name.startswith("window") else lat).double()):
            with pytest.raises(LkgdHipError, match="latents"):
                call(x)


def test_replayed_disabled_runs_the_forward_every_call():
    """replay.Replayed(enabled=False): every call is the forward itself, and no arena is taken (so no GPU is needed)"""
    from lkgd_amd import ops, replay

    class NoArenas:
        def take(self, *a, **k):
            raise AssertionError("an arena was taken")
    runs = []

    def forward():
        runs.append(len(runs))
        return runs[-1]
    with replay.Replayed(NoArenas(), "cuda:0", lambda: ("key",), forward, enabled=False) as f:
        assert [f(None), f([]), f()] == [0, 1, 2]
        assert f.plan is None and ops.PLAN is None
    assert runs == [0, 1, 2] and f.plan is None


def test_gemm_census_hand_written_rows_are_what_the_builders_build():
    """the table's dit_mod_real_depth and dit_row_ladder rows are not recorded from a forward: they must equal what
    tools/gemm_census.py builds through the product's descriptor builder today, and the ladder must still reach the plans it is
    there for (tests/test_gemm_census_dit_gpu.py replays them)"""
    from tools import gemm_census as gc
    for fwd, descs in ((gc.MOD_FORWARD, gc.modulation_descs()), (gc.LADDER_FORWARD, gc.ladder_descs())):
        want = sorted(gc.sig_key(gc.signature(d)) for d in descs)
        have = sorted(gc.sig_key(e) for e in gc.load_table() if fwd in e["launches"])
        assert want == have and len(set(want)) == len(want), fwd
    plans = [e["plan"] for e in gc.load_table() if gc.LADDER_FORWARD in e["launches"]]
    reached = {(p["program"], p["tile_m"], p["tile_n"], p["k_slices"] > 1) for p in plans}
    assert {(7, 128, 128, True), (4, 256, 320, True), (4, 256, 256, False), (4, 192, 320, False), (1, 128, 128, False)} <= reached
    # the real-depth modulation GEMM: two live rows in 192x320 tiles, the last tile column ragged at 42 layers x 3072
    mod = {(e["fields"]["M"], e["fields"]["N"]): e["plan"] for e in gc.load_table() if gc.MOD_FORWARD in e["launches"]}
    assert set(mod) == {(b, n) for b in (1, 2) for n in (695040, 1554432)} and 1554432 % 320 == 192
    assert all((p["program"], p["tile_m"], p["tile_n"], p["k_slices"]) == (4, 192, 320, 1) for p in mod.values())

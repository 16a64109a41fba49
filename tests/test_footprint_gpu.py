"""Footprint suite: every data-moving entry point of include/lkgd_hip.h touches only the tensors it is given.

Each case hands the C ABI *windows* (tests/footprint.py): the operands sit inside larger allocations whose guard rows and
``ld - width`` gap columns are a byte pattern (outputs) or NaN (inputs), the way lkgd_amd/replay.py packs live tensors side by
side.  After the call (1) no guard byte of an output has changed, (2) the result is finite, (3) it meets the tolerance of the
entry point's own parity test against an fp32 CPU reference, and (4) it equals the same call on compact, exactly-sized
operands - bit for bit wherever the program that runs does not depend on ``ld`` (every case here unless it says otherwise).
Shapes sit on either side of the tile constants of the kernel sources (named at each case).  ``REGISTRY`` maps every exported
symbol to its cases; the CPU tests at the top check the registry and show, on stand-in "kernels", that the harness bites.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from lkgd_amd import ops
from footprint import GUARD, INT_POISON, Windows, pattern_bytes, run_case

gpu = pytest.mark.gpu
DEV = "cuda:0"

# ------------------------------------------------------------------------------------------------------------ the registry
#: every name in lkgd_amd._lib.SYMBOLS -> its footprint tests in this module, or "exempt: <reason>".  Only entry points that launch
#: no kernel may be exempt (EXEMPT_ALLOWED, enforced literally by test_registry_covers_every_export).
EXEMPT_ALLOWED = {"lkgd_gemm_colstats_block", "lkgd_gemm_plan", "lkgd_gemm_wide_tile_n", "lkgd_groupnorm_chunks", "lkgd_version"}
REGISTRY = {
    "lkgd_gemm_f16": ["test_gemm_plain_and_epilogue", "test_gemm_two_source_geglu_ln_colstats", "test_gemm_conv_modes",
                      "test_gemm_unaligned_rows_fall_back", "test_gemm_split_k_workspace", "test_gemm_wide_forms"],
    "lkgd_gemm_colstats_block": "exempt: host-side query of the dispatcher, launches nothing",
    "lkgd_gemm_plan": "exempt: host-side query of the dispatcher, launches nothing (writes its own lkgd_gemm_plan_info only)",
    "lkgd_gemm_wide_tile_n": "exempt: host-side query, launches nothing",
    "lkgd_groupnorm_chunks": "exempt: host-side size query, launches nothing",
    "lkgd_version": "exempt: returns a string",
    "lkgd_groupnorm_stats": ["test_groupnorm_stats_sums"],
    "lkgd_groupnorm_sums": ["test_groupnorm_stats_sums"],
    "lkgd_groupnorm_finalize": ["test_groupnorm_finalize_forms"],
    "lkgd_groupnorm_finalize_parts": ["test_groupnorm_finalize_forms"],
    "lkgd_groupnorm_stats_cols": ["test_groupnorm_stats_cols"],
    "lkgd_groupnorm_apply": ["test_groupnorm_apply_and_silu"],
    "lkgd_groupnorm_apply_segments": ["test_groupnorm_apply_segments"],
    "lkgd_groupnorm_silu": ["test_groupnorm_apply_and_silu"],
    "lkgd_layernorm": ["test_layernorm"],
    "lkgd_tattn_block_c320": ["test_tattn_block"],
    "lkgd_ln_qkv_c320": ["test_ln_qkv"],
    "lkgd_ln_qkv_c640": ["test_ln_qkv"],
    "lkgd_ff_fused_c320": ["test_ff_fused"],
    "lkgd_attn_spatial": ["test_attn_spatial"],
    "lkgd_attn_spatial_qk": ["test_attn_spatial"],
    "lkgd_attn_temporal": ["test_attn_temporal"],
    "lkgd_tattn_front": ["test_tattn_front"],
    "lkgd_prepare_unet_input": ["test_prepare_unet_input"],
    "lkgd_cfg_euler_step": ["test_cfg_euler_steps"],
    "lkgd_cfg_fusion_euler_step": ["test_cfg_euler_steps"],
    "lkgd_shard_rows": ["test_shard_rows"],
    "lkgd_tokens_to_nchw": ["test_layout_converters"],
    "lkgd_nchw_to_tokens": ["test_layout_converters"],
    "lkgd_timestep_embedding": ["test_timestep_embedding"],
    "lkgd_silu": ["test_flat_elementwise"],
    "lkgd_add": ["test_flat_elementwise"],
    "lkgd_scale": ["test_flat_elementwise"],
    "lkgd_euler_step": ["test_flat_elementwise"],
    "lkgd_euler_step_churn": ["test_flat_elementwise"],
    "lkgd_gelu_tanh": ["test_flat_elementwise"],
    "lkgd_attn_cross": ["test_attn_cross"],
    "lkgd_attn_dense": ["test_attn_dense"],
    "lkgd_fsm_rows": ["test_fsm_rows"],
    "lkgd_conv3x3_small": ["test_conv3x3_small"],
    "lkgd_conv1d_reflect": ["test_conv1d_reflect"],
    "lkgd_resize_bicubic_ac": ["test_resize_bicubic_and_patchify"],
    "lkgd_vit_patchify": ["test_resize_bicubic_and_patchify"],
    "lkgd_softmax_rows": ["test_softmax_rows"],
    "lkgd_time_conv_out": ["test_time_conv_out"],
    "lkgd_gated_add": ["test_gated_add"],
    "lkgd_lk_fuse": ["test_lk_fuse"],
}


def test_registry_covers_every_export():
    """a new export cannot arrive without a footprint case (tests/test_c_interface_cpu.py keeps the same rule for every header)"""
    from lkgd_amd import _lib
    assert set(REGISTRY) == set(_lib.SYMBOLS), (sorted(set(_lib.SYMBOLS) - set(REGISTRY)), sorted(set(REGISTRY) - set(_lib.SYMBOLS)))
    exempt = {n for n, v in REGISTRY.items() if isinstance(v, str)}
    assert exempt == EXEMPT_ALLOWED and all(REGISTRY[n].startswith("exempt: ") for n in exempt)
    for name, cases in REGISTRY.items():
        if name in exempt:
            continue
        assert cases, name
        for c in cases:
            fn = globals().get(c)
            assert callable(fn), f"{name}: no test {c} in this module"
            marks = [m.name for m in getattr(fn, "pytestmark", [])]
            assert "gpu" in marks and "skip" not in marks and "xfail" not in marks and "slow" not in marks, (name, c, marks)


# --------------------------------------------------------------------------------- the harness bites (CPU stand-in kernels)
def _cpu_close(got, ref, what=""):
    assert (got.float() - ref.float()).abs().max().item() <= 2e-2, what


def _fake_case(misbehave=None, dtype=torch.float16, rows=5, width=16):
    x = (torch.arange(rows * width, dtype=torch.float32).reshape(rows, width) / 16).to(dtype)

    def case(W):
        xv = W.inp(x, pad=8, name="x")
        ov = W.out(rows, width, dtype, pad=8, col0=8, name="y")
        ov.copy_(xv * 2)                                   # the well-behaved "kernel": y = 2 x
        if misbehave is not None and W.windowed:
            misbehave(W, xv, ov)
        return {"y": ov}
    return case, (lambda: {"y": x.float() * 2})


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.int32])
def test_harness_passes_a_well_behaved_kernel(dtype):
    case, refs = _fake_case(dtype=dtype)
    run_case(case, "cpu", refs, _cpu_close)


def test_harness_pattern_is_not_constant_and_covers_the_slab():
    p = pattern_bytes(4096, "cpu")
    assert len(set(p.tolist())) > 200
    for ld in (16, 24, 48, 656, 1936, 8):                  # a row copied onto its neighbour is seen for every row stride in use
        assert not torch.equal(p[:ld], p[ld:2 * ld])
    W = Windows("cpu")
    v = W.out(3, 8, torch.float16, pad=8, col0=8)
    slab = W.slab_of(v)
    assert slab.shape == (3 + 2 * GUARD, 24) and v.data_ptr() == slab.data_ptr() + (GUARD * 24 + 8) * 2
    assert torch.isnan(v).all() and not torch.isnan(slab[:GUARD].float()).all()
    W.check_guards()


@pytest.mark.parametrize("where", ["gap_right", "gap_left", "row_after", "row_before", "far_after", "far_before",
                                   "garbage_over_garbage"])
def test_harness_sees_a_store_outside_the_window(where):
    """one element written into a gap column of one row, one row past the end, one row before the start, the far ends of the
    guard, and a guard row copied over its neighbour ("garbage over garbage")"""
    def bad(W, xv, ov):
        s = W.slab_of(ov)
        g, rows = GUARD, ov.shape[0]
        if where == "gap_right":
            s[g + 2, 8 + ov.shape[1]] = 1.0
        elif where == "gap_left":
            s[g + rows - 1, 7] = 1.0
        elif where == "row_after":
            s[g + rows, 8:8 + ov.shape[1]] = ov[0]
        elif where == "row_before":
            s[g - 1, 8:8 + ov.shape[1]] = ov[0]
        elif where == "far_after":
            s[2 * g + rows - 1, 0] = 0.5
        elif where == "far_before":
            s[0, s.shape[1] - 1] = 0.5
        else:
            s[g + rows + 1] = s[g + rows + 2]
    case, refs = _fake_case(bad)
    with pytest.raises(AssertionError, match="guard bytes written"):
        run_case(case, "cpu", refs, _cpu_close)


def test_harness_sees_every_gap_and_guard_byte():
    """a flipped bit in ANY byte outside the logical window is reported: swept over a whole small slab"""
    W = Windows("cpu", guard=3)
    v = W.out(2, 4, torch.float16, pad=2, col0=2)
    b = W.slab_of(v).view(torch.uint8)
    inside = 0
    for r in range(b.shape[0]):
        for c in range(b.shape[1]):
            keep = int(b[r, c])
            b[r, c] = keep ^ 1
            logical = 3 <= r < 5 and 4 <= c < 12
            if logical:
                W.check_guards()
                inside += 1
            else:
                with pytest.raises(AssertionError):
                    W.check_guards()
            b[r, c] = keep
    assert inside == 2 * 4 * 2


@pytest.mark.parametrize("where", ["guard_row_after", "guard_row_before", "gap"])
def test_harness_sees_a_leaked_input_guard(where):
    """0 * (an element outside the input's logical window) added to one output element"""
    def bad(W, xv, ov):
        s = W.slab_of(xv)
        leak = {"guard_row_after": s[GUARD + xv.shape[0], 0], "guard_row_before": s[GUARD - 1, 3],
                "gap": s[GUARD + 1, xv.shape[1]]}[where]
        ov[1, 2] += 0 * leak
    case, refs = _fake_case(bad)
    with pytest.raises(AssertionError, match="non-finite"):
        run_case(case, "cpu", refs, _cpu_close)


def test_harness_sees_an_unwritten_element_a_wrong_value_and_a_layout_dependent_result():
    def skip(W, xv, ov):
        ov[4, 15] = float("nan")
    case, refs = _fake_case(skip)
    with pytest.raises(AssertionError, match="non-finite"):
        run_case(case, "cpu", refs, _cpu_close)

    def wrong(W, xv, ov):
        ov[0, 0] += 0.5
    case, refs = _fake_case(wrong)
    with pytest.raises(AssertionError):
        run_case(case, "cpu", refs, _cpu_close)

    def tiny(W, xv, ov):                                    # inside every tolerance: only check (c) can see it
        ov[3, 3] = (ov[3, 3].float() * (1 + 2 ** -10)).to(ov.dtype)
    case, refs = _fake_case(tiny)
    with pytest.raises(AssertionError, match="windowed and compact runs differ"):
        run_case(case, "cpu", refs, _cpu_close)
    run_case(case, "cpu", refs, _cpu_close, bitwise=False)   # (the tolerance form of (c) lets it through, as it must)


def test_harness_int_tables_and_inplace_windows():
    idx = torch.tensor([[3, 1, 2, 0]], dtype=torch.int32)
    W = Windows("cpu")
    v = W.inp(idx, pad=4)
    s = W.slab_of(v)
    assert int(s[GUARD, 4]) == INT_POISON and int(s[0, 0]) == INT_POISON and torch.equal(v, idx)
    data = torch.ones(2, 8, dtype=torch.float32)
    io = W.inout(data, pad=4)
    assert torch.equal(io, data)
    W.check_guards()
    W.slab_of(io)[GUARD + 2, 0] = 9.0
    with pytest.raises(AssertionError):
        W.check_guards()


# ================================================================================================== GPU cases: helpers
def _close(got, ref, what=""):
    from test_kernels_gpu import _close as c
    c(got, ref, what=what)


def fp(case, refs=None, close=None, bitwise=True):
    return run_case(case, DEV, refs, close or _close, bitwise, sync=torch.cuda.synchronize)


def _lib_():
    from lkgd_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what=""):
    assert rc == 0, f"{what}: rc = {rc}"


def _h(x):
    return x.to(torch.float16)


def _flatpad(n, itemsize):
    per = 16 // itemsize
    return per - n % per          # 1 .. per: the next row (and the first guard row) stay 16-byte aligned


def _flatguard(n, itemsize):
    """guard rows of a flat window: 64 Ki elements either side (the largest per-workgroup run of a flat kernel is 2048
    elements, elementwise.hip), never fewer than the 2048 that GUARD rows of the narrowest row give"""
    ld = n + _flatpad(n, itemsize)
    return min(GUARD, max(1, -(-65536 // ld)))


def flat_in(W, t, name="flat"):
    """a contiguous operand of n elements (no ld in the ABI): one window row, NaN right behind its last element"""
    t = t.reshape(1, -1)
    return W.inp(t, pad=_flatpad(t.shape[1], t.element_size()), guard=_flatguard(t.shape[1], t.element_size()), name=name)


def flat_out(W, n, dtype, name="flat out"):
    isz = torch.empty(0, dtype=dtype).element_size()
    return W.out(1, n, dtype, pad=_flatpad(n, isz), guard=_flatguard(n, isz), name=name)


def flat_inout(W, t, name="flat inout"):
    t = t.reshape(1, -1)
    return W.inout(t, pad=_flatpad(t.shape[1], t.element_size()), guard=_flatguard(t.shape[1], t.element_size()), name=name)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================== 1-D elementwise kernels
@gpu
@pytest.mark.parametrize("n", [1, 7, 8, 2047, 2048, 2049, 4103])
def test_flat_elementwise(n):
    """silu / add / gelu_tanh move 8 halfs per thread, 2048 per workgroup (elementwise.hip: `* 8`, grid_for(n, 2048)), with a
    scalar tail loop at n % 8 != 0; scale / euler_step one element per thread, 256 per workgroup.  n % 8 in {0, 1, 7} on
    16-byte aligned pointers whose successor bytes are guard; one less / equal / one more than a workgroup's 2048."""
    L = _lib_()
    g = _gen(n)
    x, y = _h(torch.randn(n, generator=g) * 2), _h(torch.randn(n, generator=g))
    sm32 = torch.randn(n, generator=g) * 3
    nz = _h(torch.randn(n, generator=g))

    def silu(W):
        xv, ov = flat_in(W, x), flat_out(W, n, torch.float16)
        _ok(L.lkgd_silu(xv.data_ptr(), ov.data_ptr(), n, _st()), "silu")
        return {"silu": ov}
    fp(silu, lambda: {"silu": F.silu(x.float()).reshape(1, -1)})

    def add(W):
        av, bv, ov = flat_in(W, x), flat_in(W, y), flat_out(W, n, torch.float16)
        _ok(L.lkgd_add(av.data_ptr(), bv.data_ptr(), ov.data_ptr(), n, _st()), "add")
        return {"add": ov}
    fp(add, lambda: {"add": (x.float() + y.float()).reshape(1, -1)})

    def scale(W):
        xv, ov = flat_in(W, x), flat_out(W, n, torch.float16)
        _ok(L.lkgd_scale(xv.data_ptr(), ov.data_ptr(), n, 0.37, _st()), "scale")
        return {"scale": ov}
    fp(scale, lambda: {"scale": (x.float() * 0.37).reshape(1, -1)})

    sigma, sigma_hat, sigma_next, s_noise = 1.7, 1.9, 0.9, 1.003
    churn = math.sqrt(sigma_hat ** 2 - sigma ** 2)
    for f32 in (0, 1):
        sm = sm32 if f32 else _h(sm32)
        for vpred in (1, 0):
            def euler_ref(noise):
                s = sm.float()
                if noise is not None:
                    s = s + ((noise.float() * s_noise).half().float() * churn).half().float()
                sh = sigma_hat if noise is not None else sigma
                c_out, c_skip = -sigma / math.sqrt(sigma * sigma + 1), sigma * sigma + 1
                x0 = ((x.float() * c_out).half().float() + s / c_skip) if vpred else (s - (x.float() * sh).half().float())
                return (s + (s - x0) / sh * (sigma_next - sh)).reshape(1, -1)

            def euler(W):
                mo, sv, ov = flat_in(W, x), flat_in(W, sm), flat_out(W, n, torch.float16)
                _ok(L.lkgd_euler_step(mo.data_ptr(), sv.data_ptr(), f32, ov.data_ptr(), n, sigma, sigma_next, vpred, _st()), "euler")
                return {"euler": ov}
            fp(euler, lambda: {"euler": euler_ref(None)})

            def churned(W):
                mo, sv, nv, ov = flat_in(W, x), flat_in(W, sm), flat_in(W, nz), flat_out(W, n, torch.float16)
                _ok(L.lkgd_euler_step_churn(mo.data_ptr(), sv.data_ptr(), f32, nv.data_ptr(), ov.data_ptr(), n, sigma, sigma_hat,
                                            s_noise, churn, sigma_next, vpred, _st()), "euler churn")
                return {"churn": ov}
            fp(churned, lambda: {"churn": euler_ref(nz)})

    if n % 8:                                               # gelu_tanh: n % 8 == 0 only, rejected on the host otherwise
        W = Windows(DEV)
        io = flat_inout(W, x)
        assert L.lkgd_gelu_tanh(io.data_ptr(), io.data_ptr(), n, _st()) == -2
        W.check_guards()
    else:
        def gelu(W):
            io = flat_inout(W, x)
            _ok(L.lkgd_gelu_tanh(io.data_ptr(), io.data_ptr(), n, _st()), "gelu_tanh")
            return {"gelu": io}
        fp(gelu, lambda: {"gelu": F.gelu(x.float(), approximate="tanh").reshape(1, -1)})


@gpu
@pytest.mark.parametrize("n,dim,pad", [(1, 2, 1), (5, 320, 3), (3, 258, 8)])
def test_timestep_embedding(n, dim, pad):
    """one thread per (row, frequency), 256 per workgroup; ldo only has to hold dim (no alignment rule: odd gaps)"""
    L = _lib_()
    t = torch.tensor([1.6378, -1.5537, 6.0, 127.0, 0.02])[:n].contiguous()

    def case(W):
        tv, ov = flat_in(W, t), W.out(n, dim, torch.float16, pad=pad)
        _ok(L.lkgd_timestep_embedding(tv.data_ptr(), n, dim, ov.data_ptr(), ov.stride(0), _st()), "timestep_embedding")
        return {"emb": ov}

    def refs():
        j = torch.arange(dim // 2, dtype=torch.float64)
        a = t.double()[:, None] * torch.exp(-math.log(1e4) * j / (dim // 2))[None]
        return {"emb": torch.cat([a.cos(), a.sin()], 1).float()}

    def close(got, ref, what):                              # the bound of test_embedding_helpers
        assert (got.float().cpu() - ref).abs().max().item() < 2e-3, what
    fp(case, refs, close)


# ================================================================================================== loop glue
def _tok(x):
    """[N, F, C, H, W] -> channels-last tokens [N*F*H*W, C]"""
    return x.permute(0, 1, 3, 4, 2).reshape(-1, x.shape[2]).contiguous()


@gpu
@pytest.mark.parametrize("B,Fr,H,W_,cfg,f32", [(1, 3, 5, 17, 2, 0), (2, 1, 16, 16, 1, 1), (1, 5, 3, 17, 2, 1), (1, 1, 1, 1, 1, 0)])
def test_prepare_unet_input(B, Fr, H, W_, cfg, f32):
    """one thread per output token, 256 per workgroup: cfg*B*F*H*W = 510, 512, 510, 1.  The token matrix has ld = 8 by
    definition (one 16-byte store per token): guard rows, no gap."""
    L = _lib_()
    g = _gen(B + Fr + H)
    lat = torch.randn(B, Fr, 4, H, W_, generator=g) * 3
    lat = lat if f32 else _h(lat)
    img = _h(torch.randn(cfg * B, Fr, 4, H, W_, generator=g))
    sigma = 2.3
    T = cfg * B * Fr * H * W_

    def case(W):
        lv, iv = flat_in(W, lat), flat_in(W, img)
        ov = W.out(T, 8, torch.float16, pad=0, gap=False)
        _ok(L.lkgd_prepare_unet_input(lv.data_ptr(), f32, iv.data_ptr(), B, Fr, H, W_, cfg, sigma, ov.data_ptr(), _st()), "prepare")
        return {"tokens": ov}

    def refs():
        x = torch.cat([lat.float()] * cfg) / math.sqrt(sigma ** 2 + 1)
        return {"tokens": _tok(torch.cat([x, img.float()], dim=2))}
    fp(case, refs)


@gpu
@pytest.mark.parametrize("B,Fr,H,W_", [(2, 3, 5, 17), (2, 1, 16, 16), (4, 5, 3, 7), (2, 2, 1, 1)])
def test_cfg_euler_steps(B, Fr, H, W_):
    """cfg_euler_step: one thread per (b, f, pixel), cfg_fusion_euler_step one per (b < B/2, f, pixel), 256 per workgroup:
    510 / 255, 512 / 256, 420 / 210, 4 / 2 threads.  Odd and even F (the fusion step mirrors frame f onto F-1-f), fp16 and fp32
    latents in place between pattern guards, cfg 1 / 2.  The noise tokens have ld = 4 by definition: guard rows, no gap."""
    from test_trans_controlnet_gpu import _restated_step
    L = _lib_()
    g = _gen(B * 7 + Fr)
    sigma, sigma_next = 3.1, 2.2
    gs, wt = torch.linspace(1.0, 3.0, Fr), torch.linspace(1, 0, Fr)

    def ulp(got, ref, what):                               # the bound of test_fusion_step_vs_fp32_restatement: one fp16 ulp
        err = (got.float().cpu().reshape(-1) - ref.float().reshape(-1)).abs().max().item()
        assert err <= 2 ** -10 * ref.float().abs().max().item() + 1e-3, (what, err)
    for cfg in (1, 2):
        for dt in (torch.float16, torch.float32):
            for vpred in (1, 0):
                lat = (torch.randn(B, Fr, 4, H, W_, generator=g) * sigma).to(dt)
                noise = _h(torch.randn(cfg * B, Fr, 4, H, W_, generator=g))
                f32 = int(dt == torch.float32)

                def plain(W):
                    nv = W.inp(_tok(noise), pad=0, gap=False, name="noise")
                    lv = flat_inout(W, lat, "latents")
                    gv = flat_in(W, gs, "guidance")
                    _ok(L.lkgd_cfg_euler_step(nv.data_ptr(), lv.data_ptr(), f32, gv.data_ptr() if cfg == 2 else None, B, Fr, H,
                                              W_, cfg, sigma, sigma_next, vpred, _st()), "cfg_euler_step")
                    return {"latents": lv}

                def plain_ref():
                    n = noise
                    if cfg == 2:
                        u, c = noise.chunk(2)
                        n = u + gs.half()[None, :, None, None, None] * (c - u)
                    s = torch.tensor(sigma, dtype=torch.float32)
                    x = lat.float()
                    x0 = ((n * (-s / (s ** 2 + 1) ** 0.5)).float() + x / (s ** 2 + 1)) if vpred else (x - (n * s).float())
                    return {"latents": (x + (x - x0) / s * (sigma_next - sigma)).to(dt)}
                fp(plain, plain_ref, ulp)

                def fusion(W):
                    nv = W.inp(_tok(noise), pad=0, gap=False, name="noise")
                    lv = flat_inout(W, lat, "latents")
                    gv, wv = flat_in(W, gs, "guidance"), flat_in(W, wt, "weight")
                    _ok(L.lkgd_cfg_fusion_euler_step(nv.data_ptr(), lv.data_ptr(), f32, gv.data_ptr() if cfg == 2 else None,
                                                     wv.data_ptr(), B, Fr, H, W_, cfg, sigma, sigma_next, vpred, _st()), "fusion step")
                    return {"latents": lv}
                fp(fusion, lambda: {"latents": _restated_step(noise, lat, gs, wt, cfg, sigma, sigma_next, bool(vpred))}, ulp)


@gpu
@pytest.mark.parametrize("fl,HW,C_,px", [(1, 7, 8, (3, 2, 2)), (4, 144, 320, (48, 32, 32, 32)), (3, 43, 40, (1, 41, 1)), (2, 64, 16, (64,))])
def test_shard_rows(fl, HW, C_, px):
    """one thread per 16-byte piece, 256 per workgroup (7, 23 040, 645 = 2.5 workgroups, 256 pieces); both buffers are
    contiguous [fl * HW, C] by contract (ld = C): guard rows, no gap; pack and unpack against the strided copies"""
    L = _lib_()
    x = _h(torch.randn(fl * HW, C_, generator=_gen(HW)))
    tab = (C.c_int32 * len(px))(*px)
    packed = torch.cat([x.reshape(fl, HW, C_)[:, sum(px[:r]):sum(px[:r + 1])].reshape(-1, C_) for r in range(len(px))])
    for pack, src, want in ((1, x, packed), (0, packed, x)):
        def case(W):
            sv = W.inp(src, pad=0, gap=False, name="src")
            dv = W.out(fl * HW, C_, torch.float16, pad=0, gap=False, name="dst")
            _ok(L.lkgd_shard_rows(sv.data_ptr(), dv.data_ptr(), fl, HW, C_, len(px), C.cast(tab, C.c_void_p), pack, _st()), "shard_rows")
            return {"dst": dv}
        got = fp(case, lambda: {"dst": want.float()})
        assert torch.equal(got["dst"].cpu(), want)


@gpu
@pytest.mark.parametrize("N,C_,HW,pad", [(2, 5, 51, 3), (1, 8, 256, 8), (3, 4, 43, 1), (1, 1, 1, 1)])
def test_layout_converters(N, C_, HW, pad):
    """tokens_to_nchw / nchw_to_tokens: one thread per element, 256 per workgroup (510, 2048, 516, 1), C < ld with odd gaps
    (neither entry point has an alignment rule: scalar accesses)"""
    L = _lib_()
    tok = _h(torch.randn(N * HW, C_, generator=_gen(HW)))
    nchw = tok.reshape(N, HW, C_).permute(0, 2, 1).contiguous()

    def to_nchw(W):
        tv = W.inp(tok, pad=pad, name="tokens")
        ov = flat_out(W, N * C_ * HW, torch.float16, "nchw")
        _ok(L.lkgd_tokens_to_nchw(tv.data_ptr(), tv.stride(0), N, C_, HW, ov.data_ptr(), _st()), "tokens_to_nchw")
        return {"nchw": ov}
    got = fp(to_nchw, lambda: {"nchw": nchw.float().reshape(1, -1)})
    assert torch.equal(got["nchw"].cpu().reshape(-1), nchw.reshape(-1))

    def to_tokens(W):
        xv = flat_in(W, nchw, "nchw")
        ov = W.out(N * HW, C_, torch.float16, pad=pad, col0=pad, name="tokens")
        _ok(L.lkgd_nchw_to_tokens(xv.data_ptr(), N, C_, HW, ov.data_ptr(), ov.stride(0), _st()), "nchw_to_tokens")
        return {"tokens": ov}
    got = fp(to_tokens, lambda: {"tokens": tok.float()})
    assert torch.equal(got["tokens"].cpu(), tok)


# ================================================================================================== VAE / DiT / CLIP helpers
@gpu
@pytest.mark.parametrize("cols", [8, 2040, 2048, 2056, 16384])
def test_softmax_rows(cols):
    """a workgroup per row, thread t owns the 16-byte chunks (i * 256 + t) * 8 < cols (vae_ops.hip: SM_NT = 256, NV = 8):
    2048 = one full round of chunks, 2040 / 2056 one chunk less / more, 8 a single live thread, 16384 the cap.  x and y on
    unequal ld; in place (out=None) between pattern guards"""
    L = _lib_()
    rows = 3
    x = _h(3.0 * torch.randn(rows, cols, generator=_gen(cols)))

    def close(got, ref, what):                              # the bounds of test_vae_kernels_vs_torch
        y = got.float().cpu()
        assert (y - ref).abs().max().item() < 2e-3 and abs(float(y.sum(1).mean()) - 1.0) < 2e-3, what
    refs = lambda: {"y": torch.softmax(x.float(), 1)}      # noqa: E731

    def two(W):
        xv, yv = W.inp(x, pad=8, name="x"), W.out(rows, cols, torch.float16, pad=24, col0=8, name="y")
        _ok(L.lkgd_softmax_rows(xv.data_ptr(), xv.stride(0), yv.data_ptr(), yv.stride(0), rows, cols, _st()), "softmax_rows")
        return {"y": yv}
    fp(two, refs, close)

    def inplace(W):
        io = W.inout(x, pad=8, name="x = y")
        _ok(L.lkgd_softmax_rows(io.data_ptr(), io.stride(0), io.data_ptr(), io.stride(0), rows, cols, _st()), "softmax_rows")
        return {"y": io}
    fp(inplace, refs, close)
    assert L.lkgd_softmax_rows(1 << 20, cols + 8, 1 << 20, cols + 8, rows, 16392, _st()) == -2      # over the cap: LKGD_E_SHAPE


@gpu
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("nb,Fr,HW", [(2, 5, 26), (2, 1, 129), (2, 2, 64), (1, 2, 1)])
def test_time_conv_out(ld, nb, Fr, HW):
    """one thread per (frame, pixel), 256 per workgroup (260, 258, 256, 2); every thread loads a half4 whose lane 3 is the pad
    channel: NaN there (ld = 4: the only gap column; ld = 8: five of them) must not reach the output.  Rule: ld % 4, tokens
    8-byte aligned.  F = 1 (no neighbour frame), 2, 5; fp32 and fp16 planes"""
    L = _lib_()
    g = _gen(ld + Fr + HW)
    tok = _h(torch.randn(nb * Fr * HW, 3, generator=g))
    w, b = torch.randn(3, 3, 3, generator=g), torch.randn(3, generator=g)

    def refs():
        x5 = tok.float().reshape(nb, Fr, HW, 1, 3).permute(0, 4, 1, 2, 3)
        y = F.conv3d(x5, w.reshape(3, 3, 3, 1, 1), b, padding=(1, 0, 0)).permute(0, 2, 1, 3, 4)
        return {"planes": y.reshape(1, -1)}
    for dt in (torch.float32, torch.float16):
        def case(W):
            # (the compact form of a 3-channel token matrix is ld = 4 with a zero pad channel: ld >= 4 is the entry point's rule)
            tv = W.inp(tok, pad=ld - 3, name="tokens") if W.windowed else torch.cat([tok, torch.zeros_like(tok[:, :1])], 1).to(DEV)
            wv, bv = flat_in(W, w, "w"), flat_in(W, b, "bias")
            ov = flat_out(W, nb * Fr * 3 * HW, dt, "planes")
            _ok(L.lkgd_time_conv_out(tv.data_ptr(), tv.stride(0), wv.data_ptr(), bv.data_ptr(), ov.data_ptr(), int(dt == torch.float32), nb,
                                     Fr, HW, _st()), "time_conv_out")
            return {"planes": ov}
        fp(case, refs)


@gpu
@pytest.mark.parametrize("B,rpb,split,C_", [(4, 13, 3, 40), (1, 1, 0, 8), (2, 16, 16, 64), (3, 7, 1, 2048)])
def test_gated_add(B, rpb, split, C_):
    """one thread per 16-byte piece, 256 per workgroup: 260 pieces (one past a workgroup), 1, 256, 5376; x / res / out on three
    different ld; split at 0, inside and at rows_per_batch"""
    L = _lib_()
    g = _gen(B + C_)
    rows = B * rpb
    x, res = _h(torch.randn(rows, C_, generator=g)), _h(torch.randn(rows, C_, generator=g))
    gate = torch.randn(2 * B, C_, generator=g)

    def case(W):
        xv, rv = W.inp(x, pad=8, name="x"), W.inp(res, pad=24, col0=8, name="res")
        gv = flat_in(W, gate, "gate")
        ov = W.out(rows, C_, torch.float16, pad=16, name="out")
        _ok(L.lkgd_gated_add(xv.data_ptr(), xv.stride(0), gv.data_ptr(), rv.data_ptr(), rv.stride(0), ov.data_ptr(), ov.stride(0),
                             rows, C_, rpb, split, _st()), "gated_add")
        return {"out": ov}

    def refs():
        r = torch.arange(rows)
        gi = (r // rpb) * 2 + ((r % rpb) >= split).long()
        return {"out": res.float() + gate[gi] * x.float()}
    fp(case, refs)


@gpu
@pytest.mark.parametrize("nb,S,heads,hd", [(2, 1, 2, 8), (1, 15, 3, 80), (2, 17, 2, 128), (1, 257, 2, 80), (2, 16, 1, 64)])
def test_attn_dense(nb, S, heads, hd):
    """a workgroup = (batch entry, head) x 16 query rows (attn_dense.hip: AD_QPB = 16), keys by lane in steps of 64: S = 1, 15,
    16, 17 around a query block, 257 = four key rounds + 1; head_dim 8 / 80 / 128.  q | k | v as thirds of one matrix; ldo need
    only be even and out 4-byte aligned (the kernel stores half2): the output window sits at an odd-pair column offset"""
    L = _lib_()
    g = _gen(S + hd)
    w = heads * hd
    q, k, v = (_h(torch.randn(nb * S, w, generator=g)) for _ in range(3))

    def case(W):
        qv, kv, vv = W.inp_cols([q, k, v], pad=8, name="qkv")
        ov = W.out(nb * S, w, torch.float16, pad=4, col0=2, name="out")
        _ok(L.lkgd_attn_dense(qv.data_ptr(), qv.stride(0), kv.data_ptr(), kv.stride(0), vv.data_ptr(), vv.stride(0), ov.data_ptr(),
                              ov.stride(0), nb, S, heads, hd, hd ** -0.5, _st()), "attn_dense")
        return {"out": ov}

    def refs():
        qf, kf, vf = (t.float().reshape(nb, S, heads, hd).transpose(1, 2) for t in (q, k, v))
        return {"out": F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(nb * S, w)}

    def close(got, ref, what):                              # the bound of test_attn_dense_matches_sdpa
        assert (got.float().cpu() - ref).abs().max().item() < 2e-3, what
    fp(case, refs, close)


@gpu
@pytest.mark.parametrize("T,heads,NC,Lk,rowmap", [(1, 1, 1, 1, (1, 0, 1, 1)), (255, 2, 3, 77, (100, 1, 1, 1 << 30)),
                                                  (257, 3, 2, 128, (1 << 20, 0, 2, 2)), (513, 1, 4, 1, (60, 7, 1, 4, 2)),
                                                  (256, 5, 2, 5, (16, 1, 1, 2))])
def test_attn_cross(T, heads, NC, Lk, rowmap):
    """one thread per query row, 256 per workgroup (attn_cross.hip: XA_NT): T = 1, 255, 256, 257, 513; Lk = 1 and 77;
    ncontexts * Lk at the cap of 256 (XA_MAXKV) and at 231.  K | V as the halves of one matrix (lkgd_amd/unet.py), four ld"""
    L = _lib_()
    g = _gen(T + Lk)
    Cw = heads * 64
    q = _h(torch.randn(T, Cw, generator=g))
    k, v = _h(torch.randn(NC * Lk, Cw, generator=g)), _h(torch.randn(NC * Lk, Cw, generator=g))
    d1, m1, d2, md = rowmap[:4]
    c0 = rowmap[4] if len(rowmap) > 4 else 0

    def case(W):
        qv = W.inp(q, pad=16, name="q")
        kv, vv = W.inp_cols([k, v], pad=8, name="kv")
        ov = W.out(T, Cw, torch.float16, pad=24, col0=8, name="out")
        _ok(L.lkgd_attn_cross(qv.data_ptr(), qv.stride(0), kv.data_ptr(), kv.stride(0), vv.data_ptr(), vv.stride(0), ov.data_ptr(),
                              ov.stride(0), T, heads, NC, Lk, d1, m1, d2, md, c0, 0.125, _st()), "attn_cross")
        return {"out": ov}

    def refs():
        rows = torch.arange(T)
        idx = ((rows // d1) * m1 + rows % d2 + c0) % md
        kk = k.float().reshape(NC, Lk, heads, 64)[idx]
        vv = v.float().reshape(NC, Lk, heads, 64)[idx]
        sc = torch.einsum("thd,tjhd->thj", q.float().reshape(T, heads, 64), kk) * 0.125
        return {"out": torch.einsum("thj,tjhd->thd", sc.softmax(-1), vv).reshape(T, Cw)}
    fp(case, refs)


@gpu
@pytest.mark.parametrize("nimg,Hin,Win,Cin,Cout,stride,silu", [(8, 5, 7, 8, 16, 1, 1), (3, 9, 11, 16, 32, 2, 1), (1, 1, 1, 8, 16, 1, 0),
                                                               (2, 16, 8, 8, 48, 1, 0), (9, 7, 9, 32, 16, 2, 1)])
def test_conv3x3_small(nimg, Hin, Win, Cin, Cout, stride, silu):
    """one thread per output pixel x 16 output channels, 256 pixels per workgroup: 280, 90, 1, 256, 180 pixels; odd grids with
    stride 2; the border taps skip their loads (the rows around the image are guard: NaN)"""
    L = _lib_()
    g = _gen(Hin * Win + Cin)
    x = _h(torch.randn(nimg, Cin, Hin, Win, generator=g))
    w = _h(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5)
    b = torch.randn(Cout, generator=g)
    Ho, Wo = (Hin - 1) // stride + 1, (Win - 1) // stride + 1

    def case(W):
        xv = W.inp(x.permute(0, 2, 3, 1).reshape(-1, Cin), pad=8, name="in")
        wv, bv = flat_in(W, w.permute(0, 2, 3, 1).contiguous(), "w"), flat_in(W, b, "bias")
        ov = W.out(nimg * Ho * Wo, Cout, torch.float16, pad=8, col0=8, name="out")
        _ok(L.lkgd_conv3x3_small(xv.data_ptr(), Cin, xv.stride(0), wv.data_ptr(), bv.data_ptr(), ov.data_ptr(), Cout, ov.stride(0),
                                 nimg, Hin, Win, stride, silu, _st()), "conv3x3_small")
        return {"out": ov}

    def refs():
        y = F.conv2d(x.float(), w.float(), b, stride=stride, padding=1)
        y = F.silu(y) if silu else y
        return {"out": y.permute(0, 2, 3, 1).reshape(-1, Cout)}
    fp(case, refs)


@gpu
@pytest.mark.parametrize("C_", [8, 320, 520])
def test_fsm_rows(C_):
    """a wave per output row, four rows per workgroup (fsm.hip: kRowsPerBlock), lane l owns channels [8 l, 8 l + 8) + 512 j:
    pairs * HW = 21 rows (a last workgroup with one live wave); C = 8 (one live lane), 320, 520 (a second, ragged round of the
    channel loop).  Copy / combine with res and bias windowed on their own ld; scatter-mean with the four tables windowed"""
    from lkgd_amd import _lib
    from lkgd_amd.patch_FSM import _csr
    L = _lib_()
    g = _gen(C_)
    pairs, HW, P = 3, 7, 20
    hA = _h(torch.randn(2 * pairs * HW, C_, generator=g))
    res = _h(torch.randn(2 * pairs * HW, C_, generator=g))
    bias = _h(torch.randn(2, C_, generator=g))
    tgt = torch.randint(0, HW // 2 + 1, (pairs, P), generator=g)
    src = torch.randint(0, HW, (pairs, P), generator=g)
    vis = (torch.rand(pairs, P, generator=g) > 0.3).float()
    off, pt = (t.cpu() for t in _csr(tgt.to(DEV), pairs, HW))

    def desc(a, out, a_rows, o_rows, resv=None, r_rows=(0, 0), biasv=None, bias_map=(1, 0, 1), csr=None):
        d = _lib.FsmDesc()
        d.a, d.out, d.lda, d.ldo = a.data_ptr(), out.data_ptr(), a.stride(0), out.stride(0)
        d.a_pair_rows, d.a_off = a_rows
        d.o_pair_rows, d.o_off = o_rows
        d.pairs, d.HW, d.C = pairs, HW, C_
        if resv is not None:
            d.res, d.ldr = resv.data_ptr(), resv.stride(0)
            d.r_pair_rows, d.r_off = r_rows
        if biasv is not None:
            d.bias, d.ldb = biasv.data_ptr(), biasv.stride(0)
            d.bias_mul, d.bias_add, d.bias_div = bias_map
        if csr is not None:
            d.csr_off, d.csr_pt, d.gather_idx, d.vis = (t.data_ptr() for t in csr)
            d.P = P
        return d

    def combine(W):                                          # out[even entries] = a[odd entries] + res[even] + bias[(2 pair) // 3]
        av, rv, bv = W.inp(hA, pad=8, name="a"), W.inp(res, pad=16, name="res"), W.inp(bias, pad=24, name="bias")
        ov = W.out(pairs * HW, C_, torch.float16, pad=8, col0=8, name="out")
        _ok(L.lkgd_fsm_rows(C.byref(desc(av, ov, (2 * HW, HW), (HW, 0), rv, (2 * HW, 0), bv, (2, 0, 3))), _st()), "fsm combine")
        return {"out": ov}
    want = (hA.float().reshape(pairs, 2, HW, C_)[:, 1] + res.float().reshape(pairs, 2, HW, C_)[:, 0]
            + bias.float()[(2 * torch.arange(pairs)) // 3][:, None]).half().reshape(-1, C_)
    got = fp(combine, lambda: {"out": want.float()})
    assert torch.equal(got["out"].cpu(), want)               # (bit-exact, as test_fsm_rows_copy_and_scatter_mean asks)

    def scatter(W):
        av = W.inp(hA, pad=8, name="a")
        tabs = [flat_in(W, off.int(), "csr_off"), flat_in(W, pt.int(), "csr_pt"), flat_in(W, src.reshape(-1).int(), "gather_idx"),
                flat_in(W, vis.reshape(-1), "vis")]
        ov = W.out(pairs * HW, C_, torch.float16, pad=16, name="out")
        _ok(L.lkgd_fsm_rows(C.byref(desc(av, ov, (2 * HW, HW), (HW, 0), csr=tabs)), _st()), "fsm scatter-mean")
        return {"out": ov}
    feats = hA.float().reshape(pairs, 2, HW, C_)[:, 1]
    canvas, cnt = torch.zeros(pairs, HW, C_), torch.zeros(pairs, HW, 1)
    for p_ in range(pairs):
        for k_ in range(P):
            if vis[p_, k_] != 0:
                canvas[p_, tgt[p_, k_]] += feats[p_, src[p_, k_]]
            cnt[p_, tgt[p_, k_]] += vis[p_, k_]
    want3 = (canvas / (cnt + 1e-6)).half().reshape(-1, C_)
    got = fp(scatter, lambda: {"out": want3.float()})
    assert torch.equal(got["out"].cpu(), want3)


# ================================================================================================== image ops, ViT, LK fuse
@gpu
@pytest.mark.parametrize("H,W_", [(5, 9), (16, 16), (1, 6), (7, 1)])
def test_conv1d_reflect(H, W_):
    """one thread per output element, 256 per workgroup (90, 512, 12, 14 elements over 2 planes); both axes, odd and even tap
    counts, the largest count the entry point accepts for the axis (ntaps / 2 == size - 1: the reflection reaches the far edge
    and no further) and one beyond it, which must come back as LKGD_E_SHAPE before any launch"""
    L = _lib_()
    g = _gen(H * 31 + W_)
    planes = 2
    x = torch.randn(planes, H, W_, generator=g)
    for axis in (1, 0):
        size = W_ if axis else H
        for ntaps in sorted({1, min(3, 2 * size - 1), min(4, 2 * size - 1), 2 * size - 2, 2 * size - 1} - {0}):
            taps = torch.rand(ntaps, generator=g) + 0.1

            def case(W):
                xv, tv = flat_in(W, x, "in"), flat_in(W, taps, "taps")
                ov = flat_out(W, planes * H * W_, torch.float32, "out")
                _ok(L.lkgd_conv1d_reflect(xv.data_ptr(), ov.data_ptr(), planes, H, W_, tv.data_ptr(), ntaps, axis, _st()),
                    f"conv1d_reflect axis {axis} ntaps {ntaps}")
                return {"out": ov}

            def refs():
                front = (ntaps - 1) // 2
                xx = x.double() if axis else x.double().transpose(1, 2)
                n = xx.shape[2]
                idx = torch.arange(n)[:, None] + torch.arange(ntaps)[None] - front
                idx = idx.abs()
                idx = torch.where(idx >= n, 2 * (n - 1) - idx, idx)
                y = (xx[:, :, idx] * taps.double()).sum(-1)
                return {"out": (y if axis else y.transpose(1, 2)).float().reshape(1, -1)}

            def close(got, ref, what):                      # the bound of tests/test_image_ops.py
                torch.testing.assert_close(got.cpu(), ref, rtol=1e-5, atol=1e-5)
            fp(case, refs, close)
        Wn = Windows(DEV)
        xv, tv = flat_in(Wn, x), flat_in(Wn, torch.ones(2 * size + 1))
        ov = flat_out(Wn, planes * H * W_, torch.float32)
        for beyond in (2 * size, 2 * size + 1):
            assert L.lkgd_conv1d_reflect(xv.data_ptr(), ov.data_ptr(), planes, H, W_, tv.data_ptr(), beyond, axis, _st()) == -2
        torch.cuda.synchronize()
        Wn.check_guards()


@gpu
def test_resize_bicubic_and_patchify():
    """resize_bicubic_ac: one thread per output element, border taps clamped to the plane (its neighbours are NaN guard rows);
    sizes around a 256-thread workgroup, up- and down-scaling, 1-pixel sources.  vit_patchify: bilinear taps clamped the same way"""
    L = _lib_()
    g = _gen(3)
    for planes, H, W_, Ho, Wo in ((2, 5, 9, 16, 16), (3, 17, 6, 5, 17), (1, 1, 1, 3, 3), (2, 8, 8, 1, 1), (1, 4, 64, 4, 65)):
        x = torch.randn(planes, H, W_, generator=g)

        def case(W):
            xv, ov = flat_in(W, x, "in"), flat_out(W, planes * Ho * Wo, torch.float32, "out")
            _ok(L.lkgd_resize_bicubic_ac(xv.data_ptr(), planes, H, W_, ov.data_ptr(), Ho, Wo, _st()), "resize_bicubic_ac")
            return {"out": ov}

        def refs():
            if Ho == 1 or Wo == 1 or H == 1 or W_ == 1:     # align_corners with one sample: the source index is 0 (lkgd_hip.h 11)
                y = x[:, :1, :1].expand(planes, Ho, Wo) if (Ho == 1 and Wo == 1) or (H == 1 and W_ == 1) else None
                return {} if y is None else {"out": y.reshape(1, -1)}
            return {"out": F.interpolate(x[None], size=(Ho, Wo), mode="bicubic", align_corners=True)[0].reshape(1, -1)}

        def close(got, ref, what):
            torch.testing.assert_close(got.cpu(), ref, rtol=1e-5, atol=1e-5)
        fp(case, refs, close)
    for N, C_, H, W_, S, P in ((2, 3, 10, 14, 8, 4), (1, 1, 3, 3, 16, 16), (1, 3, 40, 24, 10, 2)):
        x = torch.randn(N, C_, H, W_, generator=g)
        gr = S // P

        def case(W):
            xv = flat_in(W, x, "in")
            ov = W.out(N * gr * gr, C_ * P * P, torch.float16, pad=0, gap=False, name="patches")   # ld = C P P by contract
            _ok(L.lkgd_vit_patchify(xv.data_ptr(), N, C_, H, W_, ov.data_ptr(), S, P, _st()), "vit_patchify")
            return {"patches": ov}

        def refs():
            r = F.interpolate(x, size=(S, S), mode="bilinear", align_corners=False)
            r = r.reshape(N, C_, gr, P, gr, P).permute(0, 2, 4, 1, 3, 5)
            return {"patches": r.reshape(N * gr * gr, C_ * P * P)}
        fp(case, refs)


@gpu
@pytest.mark.parametrize("B,Bd", [(2, 1), (3, 3)])
def test_lk_fuse(B, Bd):
    """one workgroup per batch entry; e / d / f rows and the [B, 1024] output windowed (ldo > 1024), Bd = 1 broadcasts row 0"""
    from oracle import unet as ou
    from lkgd_amd.lk_fuse import pack_lk
    L = _lib_()
    o = ou.init_weights_(ou.UNetSpatioTemporalConditionModel(ou.TINY_CONFIG), 4242)
    with torch.no_grad():
        for p in o.parameters():
            p.copy_(p.half().float())

    class OnDevice:                                          # pack_lk reads the module's parameters and `.device`
        device = torch.device(DEV)

        def __getattr__(self, n):
            return getattr(o, n)
    ws, ptrs = pack_lk(OnDevice())
    g = _gen(B)
    e = torch.randn(B, 1024, generator=g)
    d, f = 3.0 * torch.randn(Bd, 1000, generator=g), 3.0 * torch.randn(Bd, 1000, generator=g)

    def case(W):
        ev, dv, fv = flat_in(W, e, "e"), flat_in(W, d, "d"), flat_in(W, f, "f")
        ov = W.out(B, 1024, torch.float16, pad=8, col0=8, name="out")
        _ok(L.lkgd_lk_fuse(ev.data_ptr(), dv.data_ptr(), fv.data_ptr(), B, Bd, ptrs, ov.data_ptr(), ov.stride(0), _st()), "lk_fuse")
        return {"out": ov}

    def refs():
        with torch.no_grad():
            return {"out": o.lk_fuse(e[:, None], d[:, None].expand(B, 1, 1000), f[:, None].expand(B, 1, 1000)).reshape(B, 1024)}

    def close(got, ref, what):                              # the bound of test_lk_fuse_kernel_vs_oracle
        err = (got.float().cpu() - ref).abs().max().item()
        assert err <= 2e-3 * ref.abs().max().item() + 1e-3, (what, err)
    fp(case, refs, close)
    assert ws is not None


# ================================================================================================== GroupNorm / LayerNorm
def _gn_stats_ref(x, ns, rows):
    xs = x.double().reshape(ns, rows, 32, -1)
    m = xs.mean(dim=(1, 3))
    v = xs.var(dim=(1, 3), unbiased=False)
    return torch.stack([m, 1.0 / torch.sqrt(v + 1e-5)], dim=-1).float()


def _stats_close(got, ref, what):
    """(mean, rstd) from fp32 partial sums of n = rows * C / 32 fp16 values: relative error <= n 2^-24 per sum (~5e-5 at the
    sizes here), doubled by the E[x^2] - mean^2 difference; the bound test_groupnorm_statistics_from_gemm_epilogues uses"""
    assert torch.allclose(got.float().cpu().reshape(ref.shape), ref, rtol=1e-3, atol=1e-4), (what, (got.float().cpu().reshape(ref.shape) - ref).abs().max())


@pytest.fixture(params=["chunks8k", "fixed", "fixed_kb"])
def gn_chunks(request):
    """the chunk rows of the GroupNorm passes: shrunk towards 8 KiB for small maps (default, target 1024 workgroups), the fixed
    32 KiB (apply) / 128 KiB (statistics) sizes (lkgd_debug_set_gn_target_wgs(1)), and those with the two sizes swapped round
    (lkgd_debug_set_gn_apply_kb / _gn_stats_kb): 77- and 52-row samples are ragged against all of them"""
    L = _lib_()
    L.lkgd_debug_set_gn_target_wgs(1024 if request.param == "chunks8k" else 1)
    if request.param == "fixed_kb":
        L.lkgd_debug_set_gn_apply_kb(64)
        L.lkgd_debug_set_gn_stats_kb(32)
    try:
        yield request.param
    finally:
        L.lkgd_debug_set_gn_target_wgs(1024)
        L.lkgd_debug_set_gn_apply_kb(32)
        L.lkgd_debug_set_gn_stats_kb(128)


# (C = 2560: more than 256 16-byte pieces per row, the two-slot form of the chunked passes' thread map - norm.hip gn_map)
GN_SHAPES = [(128, 192, 77, 2), (320, 0, 13, 3), (64, 0, 1, 1), (640, 320, 52, 2), (2560, 0, 9, 2)]


@gpu
@pytest.mark.parametrize("C0,C1,rows,ns", GN_SHAPES)
def test_groupnorm_stats_sums(gn_chunks, C0, C1, rows, ns):
    """x = cat(x0, x1) from two windows with different ld (norm.hip: chunks of 8 KiB .. 32 / 128 KiB of rows per workgroup: 77 and
    52 rows leave a ragged last chunk, 13 and 1 a single short one); `partial` scratch and the statistics between pattern guards"""
    L = _lib_()
    g = _gen(C0 + C1 + rows)
    Cc = C0 + C1
    x = _h(torch.randn(ns * rows, Cc, generator=g) * 2 + 0.5)
    nch = L.lkgd_groupnorm_chunks(rows, Cc)

    def operands(W):
        if C1:
            return W.inp(x[:, :C0], pad=8, name="x0"), W.inp(x[:, C0:], pad=24, col0=8, name="x1")
        return W.inp(x, pad=16, name="x0"), None

    def stats(W):
        x0, x1 = operands(W)
        part, st = flat_out(W, ns * nch * 64, torch.float32, "partial"), flat_out(W, ns * 64, torch.float32, "stats")
        _ok(L.lkgd_groupnorm_stats(x0.data_ptr(), C0, x0.stride(0), x1.data_ptr() if C1 else None, C1, x1.stride(0) if C1 else 0,
                                   ns, rows, 1e-5, part.data_ptr(), st.data_ptr(), _st()), "groupnorm_stats")
        return {"stats": st}
    fp(stats, lambda: {"stats": _gn_stats_ref(x, ns, rows)}, _stats_close)

    def sums(W):
        x0, x1 = operands(W)
        part, st = flat_out(W, ns * nch * 64, torch.float32, "partial"), flat_out(W, ns * 64, torch.float32, "sums")
        _ok(L.lkgd_groupnorm_sums(x0.data_ptr(), C0, x0.stride(0), x1.data_ptr() if C1 else None, C1, x1.stride(0) if C1 else 0,
                                  ns, rows, part.data_ptr(), st.data_ptr(), _st()), "groupnorm_sums")
        return {"sums": st}

    def sums_ref():
        xs = x.double().reshape(ns, rows, 32, -1)
        return {"sums": torch.stack([xs.sum(dim=(1, 3)), (xs * xs).sum(dim=(1, 3))], -1).float()}

    def sums_close(got, ref, what):                         # fp32 sums of n values: |err| <= n 2^-24 sum|x| (n <= 1560 here: 1e-4)
        xs = x.double().reshape(ns, rows, 32, -1)
        mag = torch.stack([xs.abs().sum(dim=(1, 3)), (xs * xs).sum(dim=(1, 3))], -1).float()
        assert bool(((got.float().cpu().reshape(ref.shape) - ref).abs() <= 1e-4 * mag + 1e-6).all()), what
    fp(sums, sums_ref, sums_close)


@gpu
def test_groupnorm_finalize_forms():
    """finalize: one thread per (sample, group), 256 per workgroup: 9 samples = 288 threads.  finalize_parts: the rank parts sit
    in one gathered buffer with part / sample strides wider than the 64 floats they hold - the holes are NaN"""
    L = _lib_()
    g = _gen(5)
    ns, cnt = 9, 770.0
    mean = torch.randn(ns, 32, generator=g)
    var = torch.rand(ns, 32, generator=g) + 0.5
    sums = torch.stack([mean * cnt, (var + mean * mean) * cnt], -1)

    def ref_of(s, n):
        m = s[..., 0].double() / n
        v = (s[..., 1].double() / n - m * m).clamp_min(0)
        return torch.stack([m, 1 / torch.sqrt(v + 1e-5)], -1).float().reshape(1, -1)

    def close(got, ref, what):                              # fp64 inside, one fp32 rounding of the inputs' quotient: 1e-5 relative
        assert torch.allclose(got.float().cpu(), ref, rtol=2e-5, atol=1e-6), what

    def fin(W):
        sv, ov = flat_in(W, sums, "sums"), flat_out(W, ns * 64, torch.float32, "stats")
        _ok(L.lkgd_groupnorm_finalize(sv.data_ptr(), ns, cnt, 1e-5, ov.data_ptr(), _st()), "groupnorm_finalize")
        return {"stats": ov}
    fp(fin, lambda: {"stats": ref_of(sums, cnt)}, close)

    nparts, sample_stride, part_stride = 3, 72, 9 * 72 + 40
    parts = [sums * f for f in (0.5, 0.25, 0.25)]
    buf = torch.full((nparts * part_stride,), float("nan"))
    for r in range(nparts):
        for s in range(ns):
            o = r * part_stride + s * sample_stride
            buf[o:o + 64] = parts[r][s].reshape(-1)

    def fin_parts(W):
        pv, ov = flat_in(W, buf, "parts"), flat_out(W, ns * 64, torch.float32, "stats")
        _ok(L.lkgd_groupnorm_finalize_parts(pv.data_ptr(), nparts, part_stride, ns, sample_stride, cnt, 1e-5, ov.data_ptr(), _st()),
            "groupnorm_finalize_parts")
        return {"stats": ov}
    fp(fin_parts, lambda: {"stats": ref_of(sum(p.double() for p in parts), cnt)}, close)


@gpu
@pytest.mark.parametrize("as_sums", [0, 1])
def test_groupnorm_stats_cols(as_sums):
    """statistics from the column sums two GEMMs left: cs0 in 256-row blocks, cs1 in 32-row blocks, both with ldcs wider than
    their channel count (the gap is NaN), groups of 30 channels that straddle the two sources; a workgroup per (group, sample)"""
    L = _lib_()
    g = _gen(9)
    ns, rows, C0, C1 = 2, 512, 640, 320
    x = _h(torch.randn(ns * rows, C0 + C1, generator=g) * 1.5 + 0.3)

    def colsums(xs, blk):
        b = xs.double().reshape(-1, blk, xs.shape[1])
        return torch.stack([b.sum(1), (b * b).sum(1)], -1).float().reshape(b.shape[0], -1)      # [blocks, C/2 pairs x 2 x 2]

    def pairs(xs, blk):
        """[blocks][C / 2][2]: (sum, sum of squares) of the column PAIR 2c, 2c + 1"""
        b = xs.double().reshape(-1, blk, xs.shape[1] // 2, 2)
        return torch.stack([b.sum(dim=(1, 3)), (b * b).sum(dim=(1, 3))], -1).float().reshape(b.shape[0], -1)
    cs0, cs1 = pairs(x[:, :C0], 256), pairs(x[:, C0:], 32)

    def case(W):
        a = W.inp(cs0, pad=8, name="cs0")
        b = W.inp(cs1, pad=4, name="cs1")
        ov = flat_out(W, ns * 64, torch.float32, "stats")
        _ok(L.lkgd_groupnorm_stats_cols(a.data_ptr(), 256, a.stride(0), C0, b.data_ptr(), 32, b.stride(0), C1, ns, rows, 1e-5,
                                        as_sums, ov.data_ptr(), _st()), "groupnorm_stats_cols")
        return {"stats": ov}

    def refs():
        if not as_sums:
            return {"stats": _gn_stats_ref(x, ns, rows)}
        xs = x.double().reshape(ns, rows, 32, -1)
        return {"stats": torch.stack([xs.sum(dim=(1, 3)), (xs * xs).sum(dim=(1, 3))], -1).float()}

    def close(got, ref, what):
        if not as_sums:
            return _stats_close(got, ref, what)
        assert torch.allclose(got.float().cpu().reshape(ref.shape), ref, rtol=1e-4, atol=1e-2), what   # fp32 sums of 15 360 values
    fp(case, refs, close)
    assert colsums is not None


def _gn_ref(x, ns, rows, gamma, beta, silu):
    Cc = x.shape[1]
    y = F.group_norm(x.float().reshape(ns, rows, Cc).permute(0, 2, 1), 32, gamma, beta, 1e-5)
    return (F.silu(y) if silu else y).permute(0, 2, 1).reshape(ns * rows, Cc)


@gpu
@pytest.mark.parametrize("form", ["apply", "three_launches", "one_launch"])
@pytest.mark.parametrize("C0,C1,rows,ns", GN_SHAPES)
def test_groupnorm_apply_and_silu(gn_chunks, form, C0, C1, rows, ns):
    """lkgd_groupnorm_apply with given statistics; lkgd_groupnorm_silu as three launches (lkgd_debug_set_gn_small(0)) and as the
    one-launch program (a workgroup per (sample, group), vector width 8 / 4 / 2 halfs by C / 32 = 10, 30: 2 - forced on by
    lkgd_debug_set_gn_small_limits; samples with fewer than 64 (sample, group) pairs stay on three launches by rule)"""
    L = _lib_()
    g = _gen(C0 + 3 * C1 + rows)
    Cc = C0 + C1
    x = _h(torch.randn(ns * rows, Cc, generator=g) * 2 + 0.5)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    nch = L.lkgd_groupnorm_chunks(rows, Cc)
    silu = 1 if rows != 13 else 0

    def case(W):
        if C1:
            x0, x1 = W.inp(x[:, :C0], pad=8, name="x0"), W.inp(x[:, C0:], pad=24, col0=8, name="x1")
        else:
            x0, x1 = W.inp(x, pad=16, name="x0"), None
        gv, bv = flat_in(W, gamma, "gamma"), flat_in(W, beta, "beta")
        ov = W.out(ns * rows, Cc, torch.float16, pad=40, col0=16, name="out")
        a1 = (x1.data_ptr() if C1 else None, C1, x1.stride(0) if C1 else 0)
        if form == "apply":
            sv = flat_in(W, _gn_stats_ref(x, ns, rows), "stats")
            _ok(L.lkgd_groupnorm_apply(x0.data_ptr(), C0, x0.stride(0), *a1, ns, rows, sv.data_ptr(), gv.data_ptr(), bv.data_ptr(),
                                       silu, ov.data_ptr(), ov.stride(0), _st()), "groupnorm_apply")
            return {"out": ov}
        part, st = flat_out(W, ns * nch * 64, torch.float32, "partial"), flat_out(W, ns * 64, torch.float32, "stats")
        _ok(L.lkgd_groupnorm_silu(x0.data_ptr(), C0, x0.stride(0), *a1, ns, rows, 1e-5, part.data_ptr(), st.data_ptr(), gv.data_ptr(),
                                  bv.data_ptr(), silu, ov.data_ptr(), ov.stride(0), _st()), "groupnorm_silu")
        return {"out": ov, "stats": st}

    def refs():
        r = {"out": _gn_ref(x, ns, rows, gamma, beta, silu)}
        if form != "apply":
            r["stats"] = _gn_stats_ref(x, ns, rows)
        return r

    def close(got, ref, what):
        if "stats" in what:
            return _stats_close(got, ref, what)
        _close(got, ref, what)
    L.lkgd_debug_set_gn_small(0 if form == "three_launches" else 1)
    if form == "one_launch":
        L.lkgd_debug_set_gn_small_limits(1 << 40)
    try:
        fp(case, refs, close)
    finally:
        L.lkgd_debug_set_gn_small(1)
        L.lkgd_debug_set_gn_small_limits(10 * 1024 * 1024 + 512 * 1024)


@gpu
def test_groupnorm_apply_segments(gn_chunks):
    """a table of row segments in one launch: segments of 77, 5 and 1 rows (max_rows sizes the grid: the shorter ones leave
    whole workgroups idle) read from one source window and written into the middle of one destination window of the same ld -
    the rows between and around the segments are guard.  The table itself is a window of int64 words"""
    L = _lib_()
    g = _gen(17)
    Cc, ns = 320, 2
    seg_rows, seg_sample, src_at, dst_at = (77, 5, 1), (0, 1, 1), (0, 80, 90), (3, 100, 84)
    x = _h(torch.randn(96, Cc, generator=g) * 1.5 + 0.2)
    stats = torch.stack([torch.randn(ns, 32, generator=g), torch.rand(ns, 32, generator=g) + 0.5], -1)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)

    def case(W):
        xv = W.inp(x, pad=8, name="src")
        sv, gv, bv = flat_in(W, stats, "stats"), flat_in(W, gamma, "gamma"), flat_in(W, beta, "beta")
        dst = W.out(110, Cc, torch.float16, pad=8, name="dst")          # (compact: both matrices contiguous, ld = C)
        cover = torch.zeros(110, dtype=torch.bool)
        for r, d0 in zip(seg_rows, dst_at):
            cover[d0:d0 + r] = True
        if W.windowed:                                       # destination rows no segment covers are guard as well: pattern, not NaN
            slab = W.slab_of(dst).view(torch.uint8)
            pat = pattern_bytes(slab.numel(), DEV).reshape(slab.shape)
            keep = (~cover).nonzero().reshape(-1).to(DEV) + GUARD
            slab[keep] = pat[keep]
        tab = []
        for r, s, s0, d0 in zip(seg_rows, seg_sample, src_at, dst_at):
            tab += [xv[s0].data_ptr(), dst[d0].data_ptr(), r, s]
        tv = flat_in(W, torch.tensor(tab, dtype=torch.int64), "segments")
        ld = xv.stride(0)
        assert dst.stride(0) == ld
        _ok(L.lkgd_groupnorm_apply_segments(tv.data_ptr(), 3, max(seg_rows), Cc, ld, sv.data_ptr(), gv.data_ptr(), bv.data_ptr(), 1,
                                            _st()), "groupnorm_apply_segments")
        torch.cuda.synchronize()
        if W.windowed:                                       # uncovered rows still hold the pattern
            assert torch.equal(slab[keep], pat[keep]), "a row between the segments was written"
        return {f"seg{i}": dst[d0:d0 + r] for i, (r, d0) in enumerate(zip(seg_rows, dst_at))}

    def refs():
        out = {}
        for i, (r, s, s0) in enumerate(zip(seg_rows, seg_sample, src_at)):
            xs = x[s0:s0 + r].float().reshape(r, 32, -1)
            y = (xs - stats[s, :, 0][None, :, None]) * stats[s, :, 1][None, :, None]
            out[f"seg{i}"] = F.silu(y.reshape(r, Cc) * gamma + beta)
        return out
    fp(case, refs)


@gpu
@pytest.mark.parametrize("C_,T", [(8, 65), (64, 33), (320, 17), (320, 16), (320, 15), (640, 9), (1280, 5), (2048, 5), (1920, 1)])
def test_layernorm(C_, T):
    """a row per group of L lanes, 4 * 64 / L rows per workgroup (norm.hip: L = 4 .. 64 by C, up to 3 - at C > 1536 four - 16-byte
    vectors per lane): C = 8 -> 64 rows per workgroup (T = 65), 64 -> 32 (33), 320 -> 16 (15 / 16 / 17), 640 -> 8 (9),
    1280 / 2048 / 1920 -> 4 (5, 5, 1).  With and without affine, with the row-indexed bias; x, rowbias, out on three ld"""
    L = _lib_()
    g = _gen(C_ + T)
    x = _h(torch.randn(T, C_, generator=g) * 3 + 1)
    gamma, beta = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    emb = _h(torch.randn(3, C_, generator=g))
    idx = (torch.arange(T) // 2) % 3
    for aff in (True, False):
        for rb in (False, True):
            def case(W):
                xv = W.inp(x, pad=8, name="x")
                ov = W.out(T, C_, torch.float16, pad=24, col0=8, name="out")
                gv, bv = (flat_in(W, gamma, "gamma"), flat_in(W, beta, "beta")) if aff else (None, None)
                ev = W.inp(emb, pad=16, name="rowbias") if rb else None
                _ok(L.lkgd_layernorm(xv.data_ptr(), xv.stride(0), T, C_, gv.data_ptr() if aff else None, bv.data_ptr() if aff else None,
                                     1e-5, ev.data_ptr() if rb else None, ev.stride(0) if rb else 0, 2, 1, 1, 3, ov.data_ptr(),
                                     ov.stride(0), _st()), "layernorm")
                return {"out": ov}

            def refs():
                xx = (x + emb[idx]).float() if rb else x.float()
                return {"out": F.layer_norm(xx, (C_,), gamma if aff else None, beta if aff else None, 1e-5)}
            fp(case, refs)


# ================================================================================================== attention
def _sdpa_tokens(q, k, v, nb, heads, kvperm=None):
    qf, kf, vf = (t.float().reshape(nb, -1, heads, 64).transpose(1, 2) for t in (q, k, v))
    if kvperm is not None:
        kf, vf = kf[kvperm], vf[kvperm]
    return F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(-1, heads * 64)


@pytest.fixture(params=["rule", "never_pipe", "pipe", "waves8", "waves8_kvb128", "waves16", "waves16_kvb64"])
def attn_mode(request):
    """the spatial-attention programs small shapes reach only through a knob: the compiler-scheduled kernel with 4 waves x 64 keys
    (by rule below S = 2304), with 8 and 16 waves at 64 and 128 keys per stage, and the software-pipelined program (S >= 128; its masked
    form at S % 128 != 0) - set as tests/test_attn_pipe_gpu.py sets them"""
    L = _lib_()
    m = request.param
    L.lkgd_debug_set_attn_pipe({"never_pipe": 1, "pipe": 2}.get(m, 0))
    L.lkgd_debug_set_attn_waves(8 if m.startswith("waves8") else 16 if m.startswith("waves16") else 0)
    L.lkgd_debug_set_attn_kvb(128 if m == "waves8_kvb128" else 64 if m == "waves16_kvb64" else 0)
    try:
        yield m
    finally:
        L.lkgd_debug_set_attn_pipe(0)
        L.lkgd_debug_set_attn_waves(0)
        L.lkgd_debug_set_attn_kvb(0)


@gpu
@pytest.mark.parametrize("S,Sq", [(16, 16), (129, 129), (200, 72), (255, 255), (577, 577), (577, 1), (128, 127), (256, 129)])
def test_attn_spatial(attn_mode, S, Sq):
    """query tiles of 32 rows per wave (128 / 256 / 512 per workgroup), key stages of 64 / 128 (attn_spatial.hip), the pipelined
    program's 512-query workgroups and 128-key stages (attn_spatial_pipe.hip): S = 16 (one short stage), 129 / 255 / 577 (a last
    stage of 1 / 63 / 1 valid keys), 200, Sq < S down to a single query row and one row short of / past a tile.  q | k | v as
    thirds of one matrix; with kv_batch_map the K / V rows of the entry no query selects are NaN.  out: ldo % 4, 8-byte aligned"""
    L = _lib_()
    nb, heads = 3, 2
    Cw = heads * 64
    g = _gen(S * 3 + Sq)
    k, v = _h(torch.randn(nb * S, Cw, generator=g)), _h(torch.randn(nb * S, Cw, generator=g))
    q = _h(torch.randn(nb * Sq, Cw, generator=g))
    for kvmap in (None, [2, 0, 0]):
        kk, vv = k.clone(), v.clone()
        if kvmap is not None:                               # entry 1 is selected by no query batch: its K / V must not be read
            kk[S:2 * S] = float("nan")
            vv[S:2 * S] = float("nan")

        def case(W):
            if Sq == S:
                qv, kv, v_ = W.inp_cols([q, kk, vv], pad=8, name="qkv")
            else:
                qv = W.inp(q, pad=8, name="q")
                kv, v_ = W.inp_cols([kk, vv], pad=16, name="kv")
            ov = W.out(nb * Sq, Cw, torch.float16, pad=12, col0=4, name="out")
            mv = flat_in(W, torch.tensor(kvmap, dtype=torch.int32), "kv_batch_map") if kvmap is not None else None
            args = (qv.data_ptr(), qv.stride(0), kv.data_ptr(), kv.stride(0), v_.data_ptr(), v_.stride(0), ov.data_ptr(), ov.stride(0), nb)
            tail = (S, heads, mv.data_ptr() if kvmap is not None else None, 0.125, _st())
            if Sq == S:
                _ok(L.lkgd_attn_spatial(*args, *tail), "attn_spatial")
            else:
                _ok(L.lkgd_attn_spatial_qk(*args, Sq, *tail), "attn_spatial_qk")
            return {"out": ov}
        fp(case, lambda: {"out": _sdpa_tokens(q, k, v, nb, heads, kvmap)})


def _temporal_ref(q, k, v, B, Fq, Fk, S, heads, kvmap):
    def split(x, Fr):
        return x.float().reshape(B, Fr, S, heads, 64).permute(0, 2, 3, 1, 4)          # [B, S, heads, F, 64]
    qq, kk, vv = split(q, Fq), split(k, Fk), split(v, Fk)
    if kvmap is not None:
        kk, vv = kk[kvmap], vv[kvmap]
    o = F.scaled_dot_product_attention(qq, kk, vv)
    return o.permute(0, 3, 1, 2, 4).reshape(B * Fq * S, heads * 64)


@gpu
@pytest.mark.parametrize("Fk", [1, 3, 14, 16, 17, 25, 32])
@pytest.mark.parametrize("S,heads", [(8, 2), (3, 3), (5, 3), (1, 1)])
def test_attn_temporal(Fk, S, heads):
    """a workgroup = 8 (pixel, head) pairs x 16 (F <= 16) or 32 query-frame slots (attn_temporal.hip: TP = 8, the <16> / <32>
    instantiations): F on both sides of 16 and at 32; S * heads % 8 = 0, 1, 7 (a last workgroup with 1 / 7 live pairs whose
    other lanes are clamped onto the last pair) and a single pair; Fq = F, 1, F - 1 (query slots >= Fq are clamped onto the last
    query frame); kv_b_map = identity, a permutation, many-to-one with the unselected entries' K / V NaN"""
    L = _lib_()
    B = 3
    Cw = heads * 64
    g = _gen(Fk * 100 + S * heads)
    for Fq in sorted({Fk, 1, max(Fk - 1, 1)}):
        q = _h(torch.randn(B * Fq * S, Cw, generator=g))
        k, v = _h(torch.randn(B * Fk * S, Cw, generator=g)), _h(torch.randn(B * Fk * S, Cw, generator=g))
        for kvmap in (None, [1, 2, 0], [2, 2, 2]):
            kk, vv = k.clone(), v.clone()
            if kvmap == [2, 2, 2]:
                kk[:2 * Fk * S] = float("nan")
                vv[:2 * Fk * S] = float("nan")

            def case(W):
                if Fq == Fk:
                    qv, kv, v_ = W.inp_cols([q, kk, vv], pad=8, name="qkv")
                else:
                    qv = W.inp(q, pad=24, col0=8, name="q")
                    kv, v_ = W.inp_cols([kk, vv], pad=8, name="kv")
                ov = W.out(B * Fq * S, Cw, torch.float16, pad=16, col0=8, name="out")
                mv = flat_in(W, torch.tensor(kvmap, dtype=torch.int32), "kv_b_map") if kvmap is not None else None
                _ok(L.lkgd_attn_temporal(qv.data_ptr(), qv.stride(0), kv.data_ptr(), kv.stride(0), v_.data_ptr(), v_.stride(0),
                                         ov.data_ptr(), ov.stride(0), B, Fq, Fk, S, heads, mv.data_ptr() if kvmap is not None else None,
                                         0.125, _st()), "attn_temporal")
                return {"out": ov}
            fp(case, lambda: {"out": _temporal_ref(q, k, v, B, Fq, Fk, S, heads, kvmap)})


# ================================================================================================== fused blocks (72x128 level)
@gpu
@pytest.mark.parametrize("B,Fr,HW", [(1, 14, 16), (2, 16, 16), (3, 1, 32), (1, 5, 48)])
def test_tattn_front(B, Fr, HW):
    """panels of 16 pixels x F frames (attn_tfront.hip: HW % 16 == 0 is the entry point's rule, 16 the smallest value
    ops.tattn_front_ok admits); F = 1, 5, 14, 16 (masked keys / padded rows below 16); x and out on different ld"""
    from lkgd_amd.packing import pack_tfront
    L = _lib_()
    g = _gen(100 * B + Fr)
    Cw, heads = 320, 5
    T = B * Fr * HW
    x = _h(torch.randn(T, Cw, generator=g) * 1.7 + 0.4)
    w = _h(torch.randn(3 * Cw, Cw, generator=g) / Cw ** 0.5)
    b = torch.randn(3 * Cw, generator=g) * 0.2
    wp = pack_tfront(w, heads)

    def case(W):
        xv = W.inp(x, pad=8, name="x")
        wv, bv = flat_in(W, wp, "wpack"), flat_in(W, b, "bqkv")
        ov = W.out(T, Cw, torch.float16, pad=24, col0=8, name="out")
        _ok(L.lkgd_tattn_front(xv.data_ptr(), xv.stride(0), wv.data_ptr(), bv.data_ptr(), ov.data_ptr(), ov.stride(0), B, Fr, HW, heads,
                               1e-5, 0.125, _st()), "tattn_front")
        return {"out": ov}

    def refs():
        qkv = F.layer_norm(x.float(), (Cw,), None, None, 1e-5) @ w.float().T + b
        q, k, v = (t.reshape(B, Fr, HW, heads, 64).permute(0, 2, 3, 1, 4) for t in qkv.chunk(3, dim=-1))
        return {"out": F.scaled_dot_product_attention(q, k, v).permute(0, 3, 1, 2, 4).reshape(T, Cw)}
    fp(case, refs)


@gpu
@pytest.mark.parametrize("B,Fr,HW", [(1, 14, 7), (1, 16, 8), (3, 5, 3), (1, 1, 1), (2, 3, 13)])
def test_tattn_block(B, Fr, HW):
    """panels of 8 pixels x F frames (attn_tblock.hip: TB_PIX = 8): B * HW = 7, 8, 9, 1, 26 pixels (a last panel with 7 / 1 / 2
    live pixels); any HW is legal (ops.tattn_block_ok).  With and without the row-bias table (windowed, its own ld)"""
    from lkgd_amd.packing import pack_tblock
    from test_tblock_gpu import _close as tb_close, _ref, _weights
    L = _lib_()
    wqkv, bqkv, wo, bo = _weights(B * 100 + Fr)
    g = _gen(HW)
    T = B * Fr * HW
    x = _h(torch.randn(T, 320, generator=g) * 1.5 + 0.3)
    table = _h(torch.randn(4, 320, generator=g))
    rmap = (Fr * HW, HW, HW, 4, 3)
    rows = torch.arange(T)
    idx = ((rows // rmap[0]) * rmap[1] + rows % rmap[2] + rmap[4]) % rmap[3]
    ws = pack_tblock(wqkv, bqkv, wo)
    for rb in (False, True):
        def case(W):
            xv = W.inp(x, pad=8, name="x")
            wv, bv = flat_in(W, ws, "wstream"), flat_in(W, bo, "bo")
            tv = W.inp(table, pad=16, name="rowbias") if rb else None
            ov = W.out(T, 320, torch.float16, pad=24, col0=8, name="out")
            _ok(L.lkgd_tattn_block_c320(xv.data_ptr(), xv.stride(0), wv.data_ptr(), bv.data_ptr(), tv.data_ptr() if rb else None,
                                        tv.stride(0) if rb else 0, *(rmap if rb else (1, 0, 1, 1, 0)), ov.data_ptr(), ov.stride(0), B, Fr,
                                        HW, 1e-5, _st()), "tattn_block")
            return {"out": ov}
        fp(case, lambda: {"out": _ref(x, wqkv, bqkv, wo, bo, B, Fr, HW, rowbias=table if rb else None, idx=idx)},
           lambda got, ref, what: tb_close(got, ref, what))


@gpu
@pytest.mark.parametrize("C_", [320, 640])
@pytest.mark.parametrize("T", [1, 127, 128, 129, 300])
def test_ln_qkv(T, C_):
    """panels of 128 tokens (qkv_fused.hip): one less / equal / one more than a panel, a single row, 300 = two panels + 44"""
    from lkgd_amd.packing import pack_ln_proj
    from test_ln_qkv_gpu import _ref, _weights
    L = _lib_()
    w, b = _weights(T, C_)
    x = _h(torch.randn(T, C_, generator=_gen(T + 1)) * 1.5 + 0.3)
    ws = pack_ln_proj(w, b)
    fn = L.lkgd_ln_qkv_c320 if C_ == 320 else L.lkgd_ln_qkv_c640

    def case(W):
        xv, wv = W.inp(x, pad=8, name="x"), flat_in(W, ws, "wstream")
        ov = W.out(T, 3 * C_, torch.float16, pad=16, col0=8, name="out")
        _ok(fn(xv.data_ptr(), xv.stride(0), T, wv.data_ptr(), 1e-5, ov.data_ptr(), ov.stride(0), _st()), "ln_qkv")
        return {"out": ov}

    def close(got, ref, what):                              # the bounds of test_ln_qkv_vs_fp32
        err = (got.float().cpu() - ref).abs().max().item()
        rel = ((got.float().cpu() - ref).norm() / ref.norm()).item()
        assert err < 2e-2 and rel < 1e-3, (what, err, rel)
    fp(case, lambda: {"out": _ref(x, w, b)}, close)


@gpu
@pytest.mark.parametrize("T", [1, 31, 127, 128, 129, 300])
def test_ff_fused(T):
    """panels of 128 tokens, 32 per wave (ff_fused.hip): T = 1, 31, 127, 128, 129, 300; plain, with the row-bias table, and in
    the AlphaBlender form with res2 - x, rowbias, res2 and out on four different ld"""
    from test_ff_fused_gpu import _ref, _weights
    from lkgd_amd.packing import pack_ff_fused
    L = _lib_()
    w1, b1, w2, b2, gamma, beta = _weights(T)
    g = _gen(T + 1)
    x = _h(torch.randn(T, 320, generator=g) * 1.5 + 0.3)
    Fr, HW = 3, 7
    pe = _h(torch.randn(Fr, 320, generator=g))
    res2 = _h(torch.randn(T, 320, generator=g))
    ws = pack_ff_fused(w1.half().float() * gamma[None, :], w1.half().float() @ beta + b1, w2)
    for form in ("plain", "rowbias", "blend"):
        rb, bl = form == "rowbias", form == "blend"

        def case(W):
            xv, wv, bv = W.inp(x, pad=8, name="x"), flat_in(W, ws, "wstream"), flat_in(W, b2, "b2")
            pv = W.inp(pe, pad=16, name="rowbias") if rb else None
            rv = W.inp(res2, pad=32, col0=8, name="res2") if bl else None
            ov = W.out(T, 320, torch.float16, pad=24, col0=8, name="out")
            _ok(L.lkgd_ff_fused_c320(xv.data_ptr(), xv.stride(0), T, pv.data_ptr() if rb else None, pv.stride(0) if rb else 0,
                                     HW if rb else 1, Fr if rb else 1, wv.data_ptr(), bv.data_ptr(), 1e-5, 0.3 if bl else 1.0,
                                     rv.data_ptr() if bl else None, rv.stride(0) if bl else 0, 0.7 if bl else 0.0, ov.data_ptr(),
                                     ov.stride(0), _st()), "ff_fused")
            return {"out": ov}

        def refs():
            kw = dict(pe=pe, frames=Fr, hw=HW) if rb else (dict(s_acc=0.3, res2=res2, r2=0.7) if bl else {})
            return {"out": _ref(x, w1, b1, w2, b2, gamma, beta, **kw)}
        fp(case, refs)


# ================================================================================================== GEMM
GEMM_VARIANTS = {"auto": 0, **ops.GEMM_PROGRAMS}


@pytest.fixture(params=list(GEMM_VARIANTS))
def variant(request):
    """the seven forced tile programs of tests/test_kernels_gpu.py's `ops` fixture and the unforced dispatcher (a forced variant
    falls back to the 128x128 program on shapes it does not cover)"""
    L = _lib_()
    L.lkgd_debug_set_gemm_variant(GEMM_VARIANTS[request.param])
    try:
        yield request.param
    finally:
        L.lkgd_debug_set_gemm_variant(0)


def _gemm(a0, w, out, M, N, K, *, bias=None, a1=None, csplit=None, mode=0, Cin=0, conv=None, tconv=None, rowbias=None, rowmap=None,
          res1=None, r1=1.0, res2=None, r2=1.0, s_acc=1.0, geglu=0, workspace=None, colstats=None, cs_rows=0, ln=None, expect=0,
          block_only=False):
    """lkgd_gemm_f16 through its descriptor (lkgd_amd/ops.py::gemm builds the same one, but owns workspace and colstats)"""
    from lkgd_amd import _lib, ops
    d = _lib.GemmDesc()
    d.a0, d.w, d.out = a0.data_ptr(), w.data_ptr(), out.data_ptr()
    d.a1 = a1.data_ptr() if a1 is not None else None
    d.bias = bias.data_ptr() if bias is not None else None
    d.zeros = ops.zeros_page(out.device).data_ptr()
    d.M, d.N, d.K = M, N, K
    d.lda0 = a0.stride(0)
    d.lda1 = a1.stride(0) if a1 is not None else 0
    d.mode, d.Cin = mode, Cin
    d.csplit = csplit if csplit is not None else (K if mode == 0 else Cin)
    if conv is not None:
        d.Hout, d.Wout, d.Hin, d.Win, d.stride, d.ups = conv[:6]
        d.pad_off = conv[6] if len(conv) > 6 else 0
    if tconv is not None:
        d.F, d.HW, d.Floc, d.f_off = tconv
    if rowbias is not None:
        d.rowbias, d.ldrb = rowbias.data_ptr(), rowbias.stride(0)
        d.rb_d1, d.rb_m1, d.rb_d2, d.rb_md = rowmap[:4]
        d.rb_c0 = rowmap[4] if len(rowmap) > 4 else 0
    if res1 is not None:
        d.res1, d.ldr1 = res1.data_ptr(), res1.stride(0)
    if res2 is not None:
        d.res2, d.ldr2 = res2.data_ptr(), res2.stride(0)
    d.ldc = out.stride(0)
    d.s_acc, d.r1, d.r2 = s_acc, r1, r2
    d.geglu = geglu
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * 4
    if ln is not None:
        d.ln_colsum, d.ln_eps = ln[0].data_ptr(), ln[1]
    d.cs_rows = cs_rows
    if block_only:
        return _lib_().lkgd_gemm_colstats_block(C.byref(d))
    if colstats is not None:
        d.colstats = colstats.data_ptr()
    rc = _lib_().lkgd_gemm_f16(C.byref(d), _st())
    assert rc == expect, f"lkgd_gemm_f16 {M}x{N}x{K}: rc = {rc}"
    return rc


def _w_in(W, w, name="w"):
    """weights are [N][K] with K contiguous by contract (no ld): NaN guard rows before row 0 and after row N - 1, no gap - a tile
    that reads weight rows past N without the zeros page shows as NaN"""
    return W.inp(w, pad=0, gap=False, name=name)


@gpu
@pytest.mark.parametrize("form", ["plain", "epilogue"])
def test_gemm_plain_and_epilogue(variant, form):
    """M around the 128-row (gemm_common.h: BM) and 256-row (BM2, the stream / 256x320 / row-panel panels) tiles - 1, 127, 129,
    255, 257, 300 (a last tile with 1, 44 or 127 valid rows) - N = 64 (half a 128-column tile), 320, 328 (one 8-column piece past
    a 320-column tile), K = 64 (one K-tile: the pipeline prologue is the whole loop) and 320.  `epilogue`: bias + row-indexed bias
    + res1 + res2, every operand on its own ld.  The A operand's guard rows are NaN: a tail read the zeros page does not replace
    shows.  pad % 8 == 0 and 16-byte aligned windows: gemm_pick's rows16 and the *_ok predicates see what the compact run sees,
    so the same program runs and check (c) is bitwise"""
    g = _gen(11)
    for M in (1, 127, 129, 255, 257, 300):
        for N in (64, 320, 328):
            for K in (64, 320):
                a, w = _h(torch.randn(M, K, generator=g)), _h(torch.randn(N, K, generator=g) / K ** 0.5)
                bias = torch.randn(N, generator=g)
                r1, r2 = _h(torch.randn(M, N, generator=g)), _h(torch.randn(M, N, generator=g))
                table = _h(torch.randn(3, N, generator=g))
                idx = (torch.arange(M) // 50) % 3

                def case(W):
                    av, wv = W.inp(a, pad=8, name="a0"), _w_in(W, w)
                    ov = W.out(M, N, torch.float16, pad=24, col0=8, name="out")
                    if form == "plain":
                        _gemm(av, wv, ov, M, N, K)
                    else:
                        _gemm(av, wv, ov, M, N, K, bias=flat_in(W, bias, "bias"), rowbias=W.inp(table, pad=8, col0=8, name="rowbias"),
                              rowmap=(50, 1, 1, 3), s_acc=0.7, res1=W.inp(r1, pad=16, name="res1"), r1=0.7,
                              res2=W.inp(r2, pad=40, col0=16, name="res2"), r2=0.3)
                    return {"out": ov}

                def refs():
                    y = a.float() @ w.float().T
                    if form == "epilogue":
                        y = 0.7 * (y + bias + table.float()[idx]) + 0.7 * r1.float() + 0.3 * r2.float()
                    return {"out": y}
                try:
                    fp(case, refs)
                except AssertionError as e:
                    raise AssertionError(f"{variant} {form} {M}x{N}x{K}: {e}") from e


@gpu
@pytest.mark.parametrize("form", ["two_source", "geglu32", "geglu80", "ln", "colstats"])
def test_gemm_two_source_geglu_ln_colstats(variant, form):
    """two-source A (a1, csplit) on two ld; GEGLU with the 32-wide interleave (128-wide tiles; out has N / 2 columns) and the
    80-wide one (256x320 / resident-weight programs only: other forced variants run the 256x320 program by rule); the LayerNorm
    fold (`ln=`: the row-panel program whatever is forced); `colstats` with the column-sum buffer guarded too (programs that
    produce none - lkgd_gemm_colstats_block == 0 - must refuse the request with LKGD_E_SHAPE before any launch)"""
    from lkgd_amd.packing import pack_geglu
    g = _gen(23)
    for M in (1, 129, 257, 300):
        if form == "two_source":
            N, K0, K1 = 192, 128, 192
            a0, a1 = _h(torch.randn(M, K0, generator=g)), _h(torch.randn(M, K1, generator=g))
            w = _h(torch.randn(N, K0 + K1, generator=g) / 18)
            bias = torch.randn(N, generator=g)

            def case(W):
                ov = W.out(M, N, torch.float16, pad=8, name="out")
                _gemm(W.inp(a0, pad=8, name="a0"), _w_in(W, w), ov, M, N, K0 + K1, a1=W.inp(a1, pad=24, col0=8, name="a1"), csplit=K0,
                      bias=flat_in(W, bias, "bias"))
                return {"out": ov}
            fp(case, lambda: {"out": torch.cat([a0, a1], 1).float() @ w.float().T + bias})
        elif form in ("geglu32", "geglu80"):
            half = 32 if form == "geglu32" else 80
            Cw = 128 if half == 32 else 320
            inner = 2 * Cw if half == 32 else 320             # packed rows N = 2 * inner: a multiple of 4 * half
            a = _h(torch.randn(M, Cw, generator=g))
            w = torch.randn(2 * inner, Cw, generator=g) / Cw ** 0.5
            b = torch.randn(2 * inner, generator=g) * 0.1
            wp, bp, hh = pack_geglu(w, b, half=half)
            assert hh == half

            def case(W):
                ov = W.out(M, inner, torch.float16, pad=16, col0=8, name="out")
                _gemm(W.inp(a, pad=8, name="a0"), _w_in(W, wp), ov, M, 2 * inner, Cw, bias=flat_in(W, bp, "bias"), geglu=half)
                return {"out": ov}

            def refs():
                hid, gate = (a.float() @ _h(w).float().T + b).chunk(2, dim=-1)
                return {"out": hid * F.gelu(gate)}
            fp(case, refs)
        elif form == "ln":
            N, K = 328, 320
            a = _h(torch.randn(M, K, generator=g) * 1.5 + 0.3)
            w = _h(torch.randn(N, K, generator=g) / K ** 0.5)
            bias = torch.randn(N, generator=g)
            cs = w.float().sum(dim=1)

            def case(W):
                ov = W.out(M, N, torch.float16, pad=8, col0=8, name="out")
                _gemm(W.inp(a, pad=8, name="a0"), _w_in(W, w), ov, M, N, K, bias=flat_in(W, bias, "bias"), ln=(flat_in(W, cs, "ln_colsum"), 1e-5))
                return {"out": ov}

            def close(got, ref, what):                      # the bounds of test_gemm_layernorm_fold
                err = (got.float().cpu() - ref).abs().max().item()
                rel = ((got.float().cpu() - ref).norm() / ref.norm()).item()
                assert rel < 2e-3 and err < 3e-2, (what, err, rel)
            fp(case, lambda: {"out": F.layer_norm(a.float(), (K,)) @ w.float().T + bias}, close)
        else:
            N, K, cs_rows = 320, 320, 256
            a, w = _h(torch.randn(M, K, generator=g)), _h(torch.randn(N, K, generator=g) / K ** 0.5)
            res = _h(torch.randn(M, N, generator=g))
            seen = {}

            def case(W):
                av, wv, rv = W.inp(a, pad=8, name="a0"), _w_in(W, w), W.inp(res, pad=16, name="res1")
                ov = W.out(M, N, torch.float16, pad=8, name="out")
                blk = _gemm(av, wv, ov, M, N, K, res1=rv, cs_rows=cs_rows, block_only=True)
                seen.setdefault("blk", blk)
                assert blk == seen["blk"], "windowed and compact operands are given different programs"
                nb = (M + max(blk, 1) - 1) // max(blk, 1)
                cv = flat_out(W, nb * N, torch.float32, "colstats")
                _gemm(av, wv, ov, M, N, K, res1=rv, cs_rows=cs_rows, colstats=cv, expect=0 if blk else -2)
                if not blk:
                    _gemm(av, wv, ov, M, N, K, res1=rv)
                    return {"out": ov}
                return {"out": ov, "colstats": cv}
            got = fp(case, lambda: {"out": a.float() @ w.float().T + res.float()})
            if "colstats" in got:                          # per (row block, column pair) sums of the ROUNDED outputs over the valid rows
                blk = seen["blk"]
                o = got["out"].double().cpu()
                o = torch.cat([o, torch.zeros((-M) % blk, N, dtype=torch.float64)]).reshape(-1, blk, N // 2, 2)
                want = torch.stack([o.sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))], -1).reshape(-1)
                mag = torch.stack([o.abs().sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))], -1).reshape(-1)
                err = (got["colstats"].double().cpu().reshape(-1) - want).abs()
                # fp32 sums of <= 512 fp16 values: |err| <= 512 * 2^-24 * sum|x| = 3e-5 sum|x|
                assert bool((err <= 1e-4 * mag + 1e-5).all()), (variant, M, float(err.max()))


def _tokens(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _untokens(t, N, H, W):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2)


@gpu
@pytest.mark.parametrize("form", ["conv_s1", "conv_s2", "conv_ups", "conv_pad_off", "conv_two_source", "tconv", "tconv_floc", "c8"])
def test_gemm_conv_modes(variant, form):
    """the implicit-convolution A operands at odd H x W: 3x3 with stride 1 / 2, folded 2x upsampling, the VAE's one-sided padding,
    two sources; the temporal conv whole and for a frame shard (Floc < F: the first and last local frame read neighbours the shard
    does not own, the clip's ends read the zeros page); conv_in's C8 form, whose lda0 == 8 is fixed (guard rows, no gap).  The
    rows around the A operand are NaN: an out-of-image tap that is not replaced by the zeros page shows"""
    from lkgd_amd.packing import pack_conv3x3, pack_conv3x3_c8, pack_tconv3
    g = _gen(31)
    if form.startswith("conv"):
        N, Cin, Cout, H, Wd = 3, 64, 72, 7, 9
        stride, ups, pad_off = {"conv_s2": (2, 0, 0), "conv_ups": (1, 1, 0), "conv_pad_off": (2, 0, 1)}.get(form, (1, 0, 0))
        x = _h(torch.randn(N, Cin, H, Wd, generator=g))
        x1 = _h(torch.randn(N, 64, H, Wd, generator=g)) if form == "conv_two_source" else None
        ci = Cin + (64 if x1 is not None else 0)
        w = _h(torch.randn(Cout, ci, 3, 3, generator=g) / (9 * ci) ** 0.5)
        b = torch.randn(Cout, generator=g)
        xin = torch.cat([x, x1], 1).float() if x1 is not None else x.float()
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest") if ups else xin
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.float(), b, stride=stride) if pad_off else F.conv2d(xin, w.float(), b, stride=stride, padding=1)
        Ho, Wo = ref.shape[-2:]
        M = N * Ho * Wo

        def case(W):
            ov = W.out(M, Cout, torch.float16, pad=8, col0=8, name="out")
            _gemm(W.inp(_tokens(x), pad=8, name="a0"), _w_in(W, pack_conv3x3(w)), ov, M, Cout, 9 * ci, bias=flat_in(W, b, "bias"), mode=1, Cin=ci,
                  a1=W.inp(_tokens(x1), pad=24, name="a1") if x1 is not None else None, csplit=Cin if x1 is not None else None,
                  conv=(Ho, Wo, H, Wd, stride, ups, pad_off))
            return {"out": ov}
        fp(case, lambda: {"out": _tokens(ref)})
    elif form.startswith("tconv"):
        B, Fr, Cc, HW = 2, 5, 64, 21
        Floc, f_off = (Fr, 0) if form == "tconv" else (2, 3)
        x5 = _h(torch.randn(B, Cc, Fr, HW, 1, generator=g))
        w = _h(torch.randn(72, Cc, 3, 1, 1, generator=g) / (3 * Cc) ** 0.5)
        b = torch.randn(72, generator=g)
        ref5 = F.conv3d(x5.float(), w.float(), b, padding=(1, 0, 0))[:, :, f_off:f_off + Floc]      # [B, 72, Floc, HW, 1]
        tok = x5.permute(0, 2, 3, 4, 1).reshape(-1, Cc).contiguous()
        M = B * Floc * HW

        def case(W):
            ov = W.out(M, 72, torch.float16, pad=16, name="out")
            _gemm(W.inp(tok, pad=8, name="a0"), _w_in(W, pack_tconv3(w)), ov, M, 72, 3 * Cc, bias=flat_in(W, b, "bias"), mode=2, Cin=Cc,
                  tconv=(Fr, HW, Floc, f_off))
            return {"out": ov}
        fp(case, lambda: {"out": ref5.permute(0, 2, 3, 4, 1).reshape(M, 72)})
    else:
        N, H, Wd = 3, 9, 5
        x = _h(torch.randn(N, 8, H, Wd, generator=g))
        w = _h(torch.randn(64, 8, 3, 3, generator=g) / 72 ** 0.5)
        b = torch.randn(64, generator=g)
        M = N * H * Wd

        def case(W):
            ov = W.out(M, 64, torch.float16, pad=8, name="out")
            _gemm(W.inp(_tokens(x), pad=0, gap=False, name="a0"), _w_in(W, pack_conv3x3_c8(w)), ov, M, 64, 128, bias=flat_in(W, b, "bias"),
                  mode=3, Cin=8, conv=(H, Wd, H, Wd, 1, 0))
            return {"out": ov}
        fp(case, lambda: {"out": _tokens(F.conv2d(x.float(), w.float(), b, padding=1))})


@gpu
def test_gemm_unaligned_rows_fall_back(variant):
    """check_desc admits N % 4, ldc % 4, ldr % 4 and an 8-byte aligned out; gemm_pick's rows16 (all of them % 8 and 16-byte
    aligned) decides whether the persistent programs may run.  N = 4, 68, 324 with ldc % 8 == 4 and out 8 bytes past a 16-byte
    boundary, res1 on ld % 8 == 4: the fall-back programs.  The compact run has ldc = N (% 8 == 4 too, but 16-byte aligned):
    rows16 is false in both, yet alignment-dependent paths inside a program may differ - (c) by tolerance here"""
    g = _gen(41)
    for M in (1, 129, 257):
        for N in (4, 68, 324):
            K = 128
            a, w = _h(torch.randn(M, K, generator=g)), _h(torch.randn(N, K, generator=g) / K ** 0.5)
            bias, res = torch.randn(N, generator=g), _h(torch.randn(M, N, generator=g))

            def case(W):
                ov = W.out(M, N, torch.float16, pad=12, col0=4, name="out")            # ldc = N + 16: % 8 == 4, as N % 8 == 4
                _gemm(W.inp(a, pad=8, name="a0"), _w_in(W, w), ov, M, N, K, bias=flat_in(W, bias, "bias"), res1=W.inp(res, pad=8, name="res1"),
                      r1=0.5)
                assert not W.windowed or (ov.stride(0) % 8 == 4 and ov.data_ptr() % 16 == 8)
                return {"out": ov}
            fp(case, lambda: {"out": a.float() @ w.float().T + bias + 0.5 * res.float()}, bitwise=False)


@gpu
@pytest.mark.parametrize("prog,M,N,K,ks", [("mid", 301, 320, 704, 5), ("mid", 130, 128, 704, 4), ("wide", 300, 320, 256, 2),
                                           ("wide", 257, 640, 384, 3), ("tile128", 129, 64, 1024, 0)])
def test_gemm_split_k_workspace(prog, M, N, K, ks):
    """the split-K paths with the workspace as a window of exactly ks * M * N fp32 partials: the reduce pass reads them, nothing
    may be written behind them.  Slice counts forced the way test_gemm_four_stage_ring_k_slices (lkgd_debug_set_mid_model) and
    test_gemm_split_k_on_256x320_tiles (lkgd_debug_set_wide_ksplit) force them; the two-stage 128x128 program picks its own
    (few-row rule: tiles * 2 <= slots), given room for 16.  Partial tiles are 128 (256) rows tall: M = 129 / 130 / 257 / 300 / 301
    leave a last tile of 1 .. 45 rows whose dead rows must not be stored"""
    L = _lib_()
    g = _gen(M + K)
    a, w = _h(torch.randn(M, K, generator=g)), _h(torch.randn(N, K, generator=g) / K ** 0.5)
    bias, res = torch.randn(N, generator=g), _h(torch.randn(M, N, generator=g))
    nws = (ks if ks else 16) * M * N
    used = {}

    def case(W):
        ws = flat_out(W, nws, torch.float32, "workspace")
        ov = W.out(M, N, torch.float16, pad=8, name="out")
        _gemm(W.inp(a, pad=8, name="a0"), _w_in(W, w), ov, M, N, K, bias=flat_in(W, bias, "bias"), res1=W.inp(res, pad=16, name="res1"), r1=0.5,
              workspace=ws[0])
        torch.cuda.synchronize()
        used[W.windowed] = int(torch.isfinite(ws).sum())
        return {"out": ov}
    L.lkgd_debug_set_gemm_variant(GEMM_VARIANTS[prog])
    L.lkgd_debug_set_gemm_splitk(1)
    if prog == "mid":
        L.lkgd_debug_set_mid_model(0.0, 0.0, 0.0, 0.0, ks)
    if prog == "wide":
        L.lkgd_debug_set_wide_ksplit(ks)
    try:
        fp(case, lambda: {"out": a.float() @ w.float().T + bias + 0.5 * res.float()})
    finally:
        L.lkgd_debug_set_mid_model(0.0, 0.0, 0.0, 0.0, 0)
        L.lkgd_debug_set_wide_ksplit(0)
        L.lkgd_debug_set_gemm_variant(0)
    assert used[True] == used[False] and used[True] >= 2 * M * N and used[True] % (M * N) == 0, f"the sliced path did not run: {used}"
    if ks:
        assert used[True] <= ks * M * N


@gpu
@pytest.mark.parametrize("wm,wn,lds_out", [(256, 0, 1), (256, 0, 0), (192, 0, 1), (192, 0, 0), (256, 256, 1), (192, 256, 0)])
def test_gemm_wide_forms(wm, wn, lds_out):
    """the tile forms of the 256x320 program only a knob reaches at small shapes: 192-row tiles (lkgd_debug_set_wide_tile_m),
    256-column tiles (_wide_tile_n, N = 512), rows through LDS or direct 8-byte stores (_wide_lds_out); M = 191, 193, 255, 257,
    449 against both tile heights"""
    L = _lib_()
    g = _gen(wm + wn + lds_out)
    N, K = (512, 128) if wn else (328, 128)
    L.lkgd_debug_set_gemm_variant(ops.GEMM_WIDE)
    L.lkgd_debug_set_wide_tile_m(wm)
    L.lkgd_debug_set_wide_tile_n(wn)
    L.lkgd_debug_set_wide_lds_out(lds_out)
    try:
        for M in (191, 193, 255, 257, 449):
            a, w = _h(torch.randn(M, K, generator=g)), _h(torch.randn(N, K, generator=g) / K ** 0.5)
            bias, res = torch.randn(N, generator=g), _h(torch.randn(M, N, generator=g))
            table = _h(torch.randn(2, N, generator=g))

            def case(W):
                ov = W.out(M, N, torch.float16, pad=24, col0=8, name="out")
                _gemm(W.inp(a, pad=8, name="a0"), _w_in(W, w), ov, M, N, K, bias=flat_in(W, bias, "bias"), res1=W.inp(res, pad=16, name="res1"),
                      rowbias=W.inp(table, pad=8, name="rowbias"), rowmap=(200, 1, 1, 2))
                return {"out": ov}
            fp(case, lambda: {"out": a.float() @ w.float().T + bias + res.float() + table.float()[(torch.arange(M) // 200) % 2]})
    finally:
        L.lkgd_debug_set_wide_lds_out(-1)
        L.lkgd_debug_set_wide_tile_n(0)
        L.lkgd_debug_set_wide_tile_m(0)
        L.lkgd_debug_set_gemm_variant(0)

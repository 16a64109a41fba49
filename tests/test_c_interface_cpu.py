"""The contract of the C interface, once for every header: the files under include/ are the rows of ``_lib.HEADERS``; every header, its
ctypes table and the built library agree name by name and type by type; the three structures and the integer constants are what the
Python side mirrors; the literal pins keep header and table from drifting together; every symbol has its footprint cases.  A new
header needs a ``HEADERS`` row, a ``PINS`` row and a ``FOOTPRINT_MODULES`` row - nothing else here."""
import ctypes
import importlib
import os
import subprocess

import pytest

import c_interface as ci
from lkgd_amd import _lib, ops

HEADERS = list(_lib.HEADERS)
MAIN, DEBUG = "lkgd_hip.h", "lkgd_hip_debug.h"

#: header -> {name: number of parameters}, literally: header and table changing together still has to change this
PINS = {
    "lkgd_hip_window.h": {"lkgd_window_prepare_input": 12, "lkgd_window_cfg_euler_step": 14},
    "lkgd_hip_dit.h": {"lkgd_qk_norm_rope": 17},
    "lkgd_hip_dit_loop.h": {"lkgd_lk_fuse_tokens": 11, "lkgd_dit_patch_rows": 12, "lkgd_dit_cfg_ddim_step": 17},
    "lkgd_hip_dit_tpatch.h": {"lkgd_dit_patch_rows_t": 13, "lkgd_dit_cfg_ddim_step_t": 18},
    "lkgd_hip_dit_dpm.h": {"lkgd_dit_cfg_dpm_step": 23, "lkgd_dit_cfg_dpm_step_t": 24},
    "lkgd_hip_fp8.h": {"lkgd_quant_rows_fp8": 8, "lkgd_gelu_tanh_quant_fp8": 8, "lkgd_layernorm_quant_fp8": 11, "lkgd_gemm_fp8": 13},
    "lkgd_hip_t5.h": {"lkgd_t5_embed_rows": 9, "lkgd_t5_rmsnorm": 9, "lkgd_attn_dense_relbias": 15, "lkgd_t5_gated_gelu": 7,
                      "lkgd_t5_residual_add": 8},
    "lkgd_hip_cogvae.h": {"lkgd_spatial_norm3d": 20},
    "lkgd_hip_cogvae_enc.h": {"lkgd_cogvae_pixel_taps": 11, "lkgd_cogvae_time_pool": 9, "lkgd_cogvae_posterior": 12},
    "lkgd_hip_cogvae_tile.h": {"lkgd_cogvae_tile_blend_planar": 18, "lkgd_cogvae_tile_blend_rows": 23},
    "lkgd_hip_video.h": {"lkgd_video_postprocess": 9, "lkgd_image_preprocess": 7},
    "lkgd_hip_debug.h": {"lkgd_debug_set_gemm_variant": 1, "lkgd_debug_set_gemm_splitk": 1, "lkgd_debug_set_mid_model": 5,
                         "lkgd_debug_set_wide_ksplit": 1, "lkgd_debug_set_wide_lds_out": 1, "lkgd_debug_set_wide_tile_n": 1,
                         "lkgd_debug_set_wide_tile_m": 1, "lkgd_debug_set_attn_waves": 1, "lkgd_debug_set_attn_kvb": 1,
                         "lkgd_debug_set_attn_pipe": 1, "lkgd_debug_set_gn_apply_kb": 1, "lkgd_debug_set_gn_stats_kb": 1,
                         "lkgd_debug_set_gn_target_wgs": 1, "lkgd_debug_set_gn_small": 1, "lkgd_debug_set_gn_small_limits": 1},
}

#: header -> (test module, name of its registry {symbol: [footprint tests of that module]}).  The debug header has none: its
#: functions set per-thread knobs on the host and launch nothing
FOOTPRINT_MODULES = {
    "lkgd_hip.h": ("test_footprint_gpu", "REGISTRY"),
    "lkgd_hip_window.h": ("test_smooth_gpu", "FOOTPRINT"),
    "lkgd_hip_dit.h": ("test_cogvideox_rope_gpu", "FOOTPRINT"),
    "lkgd_hip_dit_loop.h": ("test_cogvideox_loop_gpu", "FOOTPRINT"),
    "lkgd_hip_dit_tpatch.h": ("test_cogvideox15_gpu", "FOOTPRINT"),
    "lkgd_hip_dit_dpm.h": ("test_cogvideox_dpm_gpu", "FOOTPRINT"),
    "lkgd_hip_fp8.h": ("test_fp8_gpu", "FOOTPRINT"),
    "lkgd_hip_t5.h": ("test_t5_gpu", "FOOTPRINT"),
    "lkgd_hip_cogvae.h": ("test_cogvideox_vae_gpu", "FOOTPRINT"),
    "lkgd_hip_cogvae_enc.h": ("test_cogvideox_vae_encoder_gpu", "FOOTPRINT"),
    "lkgd_hip_cogvae_tile.h": ("test_cogvideox_vae_tiling_gpu", "FOOTPRINT"),
    "lkgd_hip_video.h": ("test_video_io_gpu", "FOOTPRINT"),
}


# ---------------------------------------------------------------------------------------------------------- headers and tables
def test_include_directory_is_the_registry():
    assert sorted(os.listdir(ci.INCLUDE)) == sorted(HEADERS) and HEADERS[0] == MAIN
    assert set(PINS) == set(HEADERS) - {MAIN} and set(FOOTPRINT_MODULES) == set(HEADERS) - {DEBUG}
    tables = {k for k, v in vars(_lib).items() if k.endswith("SYMBOLS") and isinstance(v, dict)}
    assert len(tables) == len(HEADERS) and all(any(t is getattr(_lib, k) for k in tables) for t in _lib.HEADERS.values())


def test_no_name_in_two_headers_or_two_tables():
    declared = [n for h in HEADERS for n in ci.functions(h)]
    bound = [n for t in _lib.HEADERS.values() for n in t]
    assert len(declared) == len(set(declared)) == len(ci.FUNCTIONS) and len(bound) == len(set(bound))


@pytest.mark.parametrize("header", HEADERS)
def test_header_equals_table_name_by_name_and_type_by_type(header):
    """every declaration's return type and parameter types, mapped to ctypes, are the table's row"""
    declared, table = ci.functions(header), _lib.HEADERS[header]
    assert set(declared) == set(table), set(declared) ^ set(table)
    for name, (restype, params) in declared.items():
        assert (restype, [t for _, t in params]) == (table[name][0], list(table[name][1])), name
    if header == MAIN:
        assert not any(n.startswith("lkgd_debug") for n in declared)         # the product header carries no knob
    if header == DEBUG:
        assert all(n.startswith("lkgd_debug_") and declared[n][0] is None for n in declared)


@pytest.mark.parametrize("header", HEADERS)
def test_library_exports_the_table(header):
    lib = _lib.lib()                       # loads liblkgd_hip.so (links libamdhip64; no GPU needed to load)
    for name, (restype, argtypes) in _lib.HEADERS[header].items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name


#: exported and declared by no header, on purpose: the diagnostic build (`make dbg`, tools/gemm_phase_stamps.py) defines these two
#: readers of its in-kernel phase stamps; the product library does not have them
UNDECLARED_EXPORTS = {"lkgd_debug_read_stamps", "lkgd_debug_resw_stamps"}


def test_library_exports_nothing_but_the_tables():
    """the converse of the test above: every dynamic symbol lkgd_* the library defines is a row of a header's table (a cross-file
    helper that is `extern "C"` would be an export nobody declared)"""
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("lkgd_")}
    declared = {n for t in _lib.HEADERS.values() for n in t}
    assert declared <= exported <= declared | UNDECLARED_EXPORTS, sorted(exported ^ declared)


def test_version_string_and_descriptor_size():
    assert _lib.lib().lkgd_version().decode().startswith("lkgd_hip")
    # 31 int32/float fields, padded to 8; workspace + size; colstats; ln_colsum + ln_eps + pad
    assert ctypes.sizeof(_lib.GemmDesc) == 9 * 8 + 31 * 4 + 4 + 16 + 8 + 16


# --------------------------------------------------------------------------------------------------- structures and constants
def test_structures_equal_their_fields_in_name_order_and_type():
    declared = ci.structs(MAIN)
    mirrors = {"lkgd_gemm_desc": _lib.GemmDesc, "lkgd_gemm_plan_info": _lib.GemmPlanInfo, "lkgd_fsm_desc": _lib.FsmDesc}
    assert set(declared) == set(mirrors)
    for name, cls in mirrors.items():
        assert declared[name] == list(cls._fields_), name
    assert not any(ci.structs(h) for h in HEADERS if h != MAIN)


def test_error_codes_and_mirrored_constants():
    constants = {k: v for h in HEADERS for k, v in ci.constants(h).items()}
    assert sum(len(ci.constants(h)) for h in HEADERS) == len(constants)                  # no constant in two headers
    assert constants.pop("LKGD_OK") == 0
    errors = {k: constants.pop(k) for k in list(constants) if k.startswith("LKGD_E_")}
    assert {v: k for k, v in errors.items()} == _lib.ERRORS and len(errors) == len(_lib.ERRORS)
    assert (ci.OK, ci.NULL, ci.SHAPE, ci.ALIGN, ci.MODE, ci.LAUNCH) == (0, -1, -2, -3, -4, -5)
    assert constants and ops.A_CCONV3 == constants["LKGD_A_CCONV3"] == 4
    for name, value in constants.items():                                                # every other one is mirrored in ops
        assert getattr(ops, name[len("LKGD_"):]) == value, name


# ------------------------------------------------------------------------------------------------------------------- pins
@pytest.mark.parametrize("header", sorted(PINS))
def test_pinned_names_and_parameter_counts(header):
    assert {n: len(p) for n, (_, p) in ci.functions(header).items()} == PINS[header]
    assert {n: len(a) for n, (_, a) in _lib.HEADERS[header].items()} == PINS[header]


def test_relations_between_entry_points():
    names = {n: [p for p, _ in params] for n, (_, params) in ci.FUNCTIONS.items()}
    temporal = [n for n in names if n.endswith("_t") and n[:-2] in names]
    assert sorted(temporal) == ["lkgd_dit_cfg_ddim_step_t", "lkgd_dit_cfg_dpm_step_t", "lkgd_dit_patch_rows_t"]
    for n in temporal:                                               # the 2-D entry point's parameters plus p_t, nothing else
        assert "p_t" not in names[n[:-2]] and [p for p in names[n] if p != "p_t"] == names[n[:-2]], n
        assert len(names[n]) == len(names[n[:-2]]) + 1
    # the DDIM step's arguments without a, b (- 2), plus x0_state, eps, order, m1..m4, mn (+ 8)
    for sfx in ("", "_t"):
        assert len(names["lkgd_dit_cfg_dpm_step" + sfx]) == len(names["lkgd_dit_cfg_ddim_step" + sfx]) + 6


# -------------------------------------------------------------------------------------------------------- footprint coverage
@pytest.mark.parametrize("header", sorted(FOOTPRINT_MODULES))
def test_every_symbol_has_footprint_cases(header):
    """a new export cannot arrive without a footprint case: the registry of the header's GPU module names every symbol of the table,
    and every case it lists is a test of that module that runs on the GPU, unconditionally"""
    module, attr = FOOTPRINT_MODULES[header]
    mod = importlib.import_module(module)
    registry = getattr(mod, attr)
    assert set(registry) == set(_lib.HEADERS[header]), set(registry) ^ set(_lib.HEADERS[header])
    for name, cases in registry.items():
        if isinstance(cases, str):                                   # test_footprint_gpu holds its exemptions to EXEMPT_ALLOWED
            assert header == MAIN and cases.startswith("exempt: "), name
            continue
        assert cases, name
        for c in cases:
            fn = getattr(mod, c, None)
            assert callable(fn), f"{name}: no test {c} in {module}"
            own, shared = getattr(fn, "pytestmark", []), getattr(mod, "pytestmark", [])
            marks = [m.name for m in own + (shared if isinstance(shared, list) else [shared])]
            assert "gpu" in marks and "skip" not in marks and "xfail" not in marks and "slow" not in marks, (name, c, marks)


# ----------------------------------------------------------------------------------------------------------------- entry()
def test_entry_refuses_keys_that_are_no_parameters():
    good = dict(x=None, y=None, n=4)
    assert ci.entry("lkgd_silu", **good)() == ci.NULL and ci.entry("lkgd_silu", stream=None, **good)(n=8) == ci.NULL
    with pytest.raises(TypeError, match="lack.*'n'"):
        ci.entry("lkgd_silu", x=None, y=None)
    with pytest.raises(TypeError, match="unknown.*'count'"):
        ci.entry("lkgd_silu", count=4, **good)
    with pytest.raises(TypeError, match="no parameter named.*'N'"):
        ci.entry("lkgd_silu", **good)(N=8)

#!/usr/bin/env python3
"""Census of the lkgd_gemm_f16 launches of the real forwards: every descriptor the model issues, reduced to distinct SIGNATURES
(all scalar fields; per pointer NULL-ness and address mod 16; the workspace size), with the launch count per forward and the plan
lkgd_gemm_plan reports at 256 compute units.  tests/golden/gemm_census.json is that table; tests/test_gemm_census_gpu.py replays
every signature of it in isolation against tests/gemm_oracle.py and asserts that a fresh recording gives the same table;
tests/test_host_cpu.py re-derives every stored plan from the stored fields without a GPU.

    python tools/gemm_census.py --write      regenerate the table on a GPU box (weights: the seeded real-width fixtures)
    python tools/gemm_census.py              print a summary of the stored table (no GPU needed)
    python tools/gemm_census.py --dump-plans one line per stored signature x DUMP_CUS x forced variant x DUMP_KNOBS with the plan or
                                             the error code (no GPU needed): run at two revisions, the outputs of a refactor of the
                                             dispatcher are byte-equal

Forwards (geometry of BASELINE configs[1]: CFG 2 x 14 frames x 72x128 latents):
    unet_2x14                     the full forward
    unet_1x14 / unet_1x7 / unet_1x4   one CFG entry x 14 / 7 / 4 frames: what a rank of 2 / 4 / 8 runs (tools/plan_profile.py)
    controlnet_2x14               the ControlNet encoder with a fresh control video
    vae_decode / vae_encode       the real-width VAE on 2 frames of 96x128 pixels (tests/test_vae.py)
The CogVideoX path (seeded synthetic weights as tests/test_fullsize_gpu.py makes them; every layer issues the same descriptors, so
the models are built with 2 layers, the 1.5 model and T5 with 1):
    dit2b_2x17776                 CogVideoX-2B I2V (in_channels 32): CFG batch 2 x (226 text + 13x30x45 video) tokens
    dit5b_2x17776                 the 5B rotary I2V model: 3072 channels, 48 heads, learned joint position table
    dit15_2x45106                 the 1.5 I2V model: patch_size_t 2, ofs embedding, 226 text + 11x48x85 video tokens
    t5xxl_226                     the T5 encoder at d_model 4096, d_kv 64, d_ff 10240, 64 heads on 226 tokens
    dit_mod_real_depth            hand-written: the modulation GEMM of ``_modulation`` at 30 layers x 1920 and 42 layers x 3072
                                  channels, batch 2 and 1 (a two-layer model does not issue it)
    dit_row_ladder                hand-written: the block linears of the 2B and of the 5B model (q|k|v as one launch, attention out
                                  = the width of q, k, v one by one, ff1, ff2) at M in LADDER_ROWS, the smallest row counts at
                                  which the dispatcher's choice for these widths changes
The table's "fp8_signatures" are the ``lkgd_gemm_fp8`` calls of dit2b_2x17776 after ``quantize_to_float8`` (that entry point takes
no descriptor: M, N, K, the leading dimensions, bias NULL-ness and the addresses mod 16)."""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from lkgd_amd import _lib, ops                # noqa: E402
from lkgd_amd._lib import GemmDesc, GemmPlanInfo   # noqa: E402

TABLE = os.path.join(REPO, "tests", "golden", "gemm_census.json")
UNET_FORWARDS = ("unet_2x14", "unet_1x14", "unet_1x7", "unet_1x4", "controlnet_2x14", "vae_decode", "vae_encode")
DIT_FORWARDS = ("dit2b_2x17776", "dit5b_2x17776", "dit15_2x45106")
T5_FORWARD, MOD_FORWARD, LADDER_FORWARD = "t5xxl_226", "dit_mod_real_depth", "dit_row_ladder"
FORWARDS = UNET_FORWARDS + DIT_FORWARDS + (T5_FORWARD, MOD_FORWARD, LADDER_FORWARD)
FP8_FORWARD = "dit2b_2x17776"
LADDER_ROWS = (452, 2048, 4096, 12288)
TEXT_TOKENS = 226
DIT_SEED, T5_SEED = 0, 3
H, W = 72, 128
PLAN_CUS = 256
C1_SEED, VAE_SEED = 31, 21                    # tests/conftest.py::c1_oracle_model, tests/test_vae.py

POINTERS = tuple(n for n, t in GemmDesc._fields_ if t is C.c_void_p)
SCALARS = tuple(n for n, t in GemmDesc._fields_ if t is not C.c_void_p)
PLAN_FIELDS = tuple(n for n, _ in GemmPlanInfo._fields_)


def signature(d) -> dict:
    """{"fields": non-zero scalar fields, "ptr": {pointer: address mod 16} for the non-NULL pointers}"""
    fields = {}
    for n in SCALARS:
        v = getattr(d, n)
        if v:
            fields[n] = float(v) if isinstance(v, float) else int(v)
    return {"fields": fields, "ptr": {n: int(getattr(d, n)) % 16 for n in POINTERS if getattr(d, n)}}


def sig_key(sig: dict) -> str:
    return json.dumps({"fields": sig["fields"], "ptr": sig["ptr"]}, sort_keys=True)


def desc_from_signature(sig: dict, pointers=None) -> GemmDesc:
    """the descriptor of a signature.  ``pointers``: {name: address} for the non-NULL pointers; None = fake addresses of the
    recorded alignment class that nothing may dereference (enough for lkgd_gemm_plan with cus != 0)"""
    d = GemmDesc()
    for n, v in sig["fields"].items():
        setattr(d, n, v)
    for i, n in enumerate(POINTERS):
        if n in sig["ptr"]:
            p = ((i + 1) << 24) + sig["ptr"][n] if pointers is None else pointers[n]
            assert p % 16 == sig["ptr"][n], (n, p, sig["ptr"][n])
            setattr(d, n, p)
    return d


def plan(d, cus: int = PLAN_CUS) -> dict:
    info = GemmPlanInfo()
    rc = _lib.lib().lkgd_gemm_plan(C.byref(d), cus, C.byref(info))
    if rc:
        raise _lib.LkgdHipError(f"lkgd_gemm_plan: {_lib.ERRORS.get(rc, rc)}")
    return {n: int(getattr(info, n)) for n in PLAN_FIELDS}


#: why a signature may have no second program to be compared with (tests/test_gemm_census_gpu.py)
NO_SECOND = {"ln_fold": "LayerNorm fold: only the row-panel program holds whole rows in registers",
             "geglu80": "80-wide GEGLU interleave outside the resident-weight program's shapes: the 256x320 program alone"}


def second_program(sig: dict, cus: int = PLAN_CUS):
    """the forced variant whose output the census compares with the automatic program's: (variant, None), or (None, key of
    NO_SECOND) where no other program computes this descriptor"""
    lib = _lib.lib()
    if "ln_colsum" in sig["ptr"]:
        return None, "ln_fold"
    d = desc_from_signature(dict(sig, ptr={k: v for k, v in sig["ptr"].items() if k != "colstats"}))
    auto = plan(d, cus)

    def forced(v):
        lib.lkgd_debug_set_gemm_variant(v)
        try:
            return plan(d, cus)
        finally:
            lib.lkgd_debug_set_gemm_variant(0)
    if sig["fields"].get("geglu") == 80:
        other = ops.GEMM_RESW if auto["program"] == ops.GEMM_WIDE else ops.GEMM_WIDE
        return (other, None) if forced(other)["program"] == other else (None, "geglu80")
    for v in (ops.GEMM_TILE128, ops.GEMM_MID, ops.GEMM_TILE256):      # where the first IS the automatic program, another one
        pl = forced(v)
        if (pl["program"], pl["k_slices"]) != (auto["program"], auto["k_slices"]):
            return v, None
    raise AssertionError("no second program differs from the automatic one")


def load_table(path: str = TABLE) -> list:
    with open(path) as f:
        return json.load(f)["signatures"]


# ---------------------------------------------------------------------------------------------------------------- recording (GPU)
FP8_ARGS = ("a", "lda", "a_scale", "w", "ldw", "w_scale", "bias", "out", "ldc", "M", "N", "K")      # lkgd_gemm_fp8, in order
FP8_POINTERS = ("a", "a_scale", "w", "w_scale", "bias", "out")


def fp8_signature(args) -> dict:
    """the signature of one lkgd_gemm_fp8 call (its arguments without the stream): {"fields": the six integers, "ptr": {pointer:
    address mod 16} for the non-NULL pointers} - a NULL bias is absent from "ptr" """
    a = dict(zip(FP8_ARGS, args))
    return {"fields": {n: int(a[n]) for n in FP8_ARGS if n not in FP8_POINTERS},
            "ptr": {n: int(a[n]) % 16 for n in FP8_POINTERS if a[n]}}


def record_launches(run, names=("lkgd_gemm_f16",)):
    """one eager warm-up of ``run()``, then a recorded one: {name: [arguments of every call of that entry point, in order]}; the
    descriptor of an lkgd_gemm_f16 call is copied"""
    import torch
    from lkgd_amd import replay
    run()
    torch.cuda.synchronize()
    with replay.strict(False):                 # only the launch list is of interest here: nothing is replayed
        with replay.record() as p:
            run()
    torch.cuda.synchronize()
    out = {n: [] for n in names}
    for fn, args, name, _ in p.calls:
        if name == "lkgd_gemm_f16" and name in out:
            out[name].append(GemmDesc.from_buffer_copy(args[0]._obj))
        elif name in out:
            out[name].append(tuple(args))
    p.release()
    del p
    torch.cuda.empty_cache()
    return out


def record_gemms(run):
    """one eager warm-up of ``run()``, then a recorded one: copies of the lkgd_gemm_desc of every lkgd_gemm_f16 call, in order"""
    return record_launches(run)["lkgd_gemm_f16"]


def _unet_inputs(dev, cfgb, frames, seed=12345):
    import torch
    g = torch.Generator().manual_seed(seed)
    tok = torch.randn(cfgb * frames * H * W, 8, generator=g).half().to(dev)
    emb = torch.randn(cfgb, 1, 1024, generator=g).half().to(dev)
    ids = torch.tensor([[6.0, 127.0, 0.02]] * cfgb).to(dev)
    return tok, emb, ids, torch.ones(cfgb, dtype=torch.float32, device=dev)


def record_unet(unet, cfgb, frames):
    tok, emb, ids, t = _unet_inputs(unet.device, cfgb, frames)
    return record_gemms(lambda: unet.forward_tokens(tok, cfgb, frames, H, W, t, emb, ids))


def build_controlnet(unet):
    """a real-width ControlNet whose encoder is the UNet's (reference ControlNetSDVModel.from_unet); the rest seeded"""
    import torch
    from lkgd_amd import controlnet as pc
    from lkgd_amd import unet as pu
    with torch.device("meta"):
        cn = pc.ControlNetSDVModel(pu.UNetConfig(**{k: v for k, v in unet.config.__dict__.items()
                                                    if k in pu.UNetConfig.__dataclass_fields__}))
    cn = cn.to(torch.float16).to_empty(device=unet.device)
    pu.init_synthetic_weights_(cn, seed=1)
    for name in ("conv_in", "time_embedding", "add_embedding", "down_blocks", "mid_block"):
        getattr(cn, name).load_state_dict(getattr(unet, name).state_dict())
    cn.invalidate()
    return cn


def record_controlnet(unet):
    import torch
    cn = build_controlnet(unet)
    tok, emb, ids, t = _unet_inputs(unet.device, 2, 14)
    g = torch.Generator().manual_seed(12348)
    ctrl = (2.0 * torch.rand(2, 14, 3, 8 * H, 8 * W, generator=g) - 1.0).half().to(unet.device)
    # a fresh control video per call: the step-invariant conditioning embedding is part of the recorded forward
    descs = record_gemms(lambda: cn.forward_tokens(tok, 2, 14, H, W, t, emb, ids, controlnet_cond=ctrl.clone()))
    del cn
    torch.cuda.empty_cache()
    return descs


def build_vae(dev):
    import torch
    from lkgd_amd import vae as pv
    from oracle import vae as ov
    o = ov.init_weights_(ov.AutoencoderKLTemporalDecoder(ov.SVD_VAE_CONFIG), VAE_SEED)
    with torch.no_grad():
        for p in o.parameters():
            p.copy_(p.half().float())
    m = pv.AutoencoderKLTemporalDecoder(pv.VAEConfig(**{k: v for k, v in ov.SVD_VAE_CONFIG.__dict__.items()}))
    m.load_state_dict(o.state_dict())
    return m.half().to(dev)


def record_vae(dev):
    import torch
    m = build_vae(dev)
    g = torch.Generator().manual_seed(22)
    z = torch.randn(2, 4, 12, 16, generator=g).half().to(dev)
    x = (torch.rand(1, 3, 96, 128, generator=g) * 2 - 1).half().to(dev)
    dec = record_gemms(lambda: m.decode(z, num_frames=2).sample)
    enc = record_gemms(lambda: m.encode(x).latent_dist.mode())
    del m
    torch.cuda.empty_cache()
    return dec, enc


# ------------------------------------------------------------------------------------------------------- the CogVideoX path
def dit_config(name: str):
    """the DiTConfig of a DIT_FORWARDS entry and its token grid (frames, h, w)"""
    from lkgd_amd import cogvideox as pc
    if name == "dit2b_2x17776":
        return pc.DiTConfig(in_channels=32, num_layers=2), (13, 30, 45)
    if name == "dit5b_2x17776":
        return pc.DiTConfig(num_attention_heads=48, in_channels=32, num_layers=2, use_rotary_positional_embeddings=True,
                            use_learned_positional_embeddings=True), (13, 30, 45)
    if name == "dit15_2x45106":
        return pc.DiTConfig(num_attention_heads=48, in_channels=32, num_layers=1, use_rotary_positional_embeddings=True,
                            patch_size_t=2, ofs_embed_dim=512, patch_bias=False, sample_height=300, sample_width=300,
                            sample_frames=81), (11, 48, 85)
    raise KeyError(name)


def build_dit(name: str, dev="cuda:0"):
    """the model of a DIT_FORWARDS entry with the seeded weights of test_full_size_cogvideox_forward_and_ddim_steps"""
    import torch
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import unet as pu
    cfg, _ = dit_config(name)
    with torch.device("meta"):
        m = pc.CogVideoXTransformer3DModel(cfg)
    m = m.to(torch.float16).to_empty(device=dev)
    pu.init_synthetic_weights_(m, seed=DIT_SEED)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".linear." in n and ("norm1" in n or "norm2" in n or "norm_out" in n):
                p.mul_(0.1)
        if cfg.use_learned_positional_embeddings:       # a buffer: to_empty left it unset
            m.patch_embed.pos_embedding.copy_(0.02 * torch.randn(m.patch_embed.pos_embedding.shape,
                                                                 generator=torch.Generator().manual_seed(DIT_SEED + 1)))
    m.invalidate()
    return m


def dit_run(m, name: str):
    """-> a callable running the model's own ``forward`` on a CFG batch of 2 with TEXT_TOKENS text tokens"""
    import torch
    from lkgd_amd import cogvideox as pc
    cfg, (fr, h, w) = dit_config(name)
    dev = m.device
    g = torch.Generator().manual_seed(3)
    pt, p = cfg.patch_size_t or 1, cfg.patch_size
    hid = torch.randn(2, fr * pt, cfg.in_channels, h * p, w * p, generator=g).half().to(dev)
    pe = torch.randn(2, TEXT_TOKENS, cfg.text_embed_dim, generator=g).half().to(dev)
    dom, flow = torch.randn(1, 1, 1000, generator=g).to(dev), torch.randn(1, 1, 1000, generator=g).to(dev)
    kw = {}
    if cfg.use_rotary_positional_embeddings:
        kw["image_rotary_emb"] = tuple(t.to(dev) for t in pc.rotary_tables(m.config, fr, h, w))
    if cfg.ofs_embed_dim:
        kw["ofs"] = 2.0
    t = torch.tensor([500.0])
    return lambda: m(hid, pe, t, dom, flow, return_dict=False, **kw)[0]


def record_dit(name: str, dev="cuda:0", fp8: bool = False):
    """-> ([GemmDesc] of the forward, [lkgd_gemm_fp8 argument tuples] of the same forward after quantize_to_float8 or None)"""
    import torch
    m = build_dit(name, dev)
    descs = record_gemms(dit_run(m, name))
    calls = None
    if fp8:
        from lkgd_amd import fp8 as fp8_mode
        fp8_mode.quantize_to_float8(m)
        calls = record_launches(dit_run(m, name), ("lkgd_gemm_fp8",))["lkgd_gemm_fp8"]
    del m
    torch.cuda.empty_cache()
    return descs, calls


def record_t5(dev="cuda:0"):
    """one layer of the T5-XXL encoder on TEXT_TOKENS tokens through ``T5EncoderModel.forward``"""
    import torch
    from lkgd_amd import t5
    cfg = t5.T5Config(num_layers=1)
    with torch.device("meta"):
        m = t5.T5EncoderModel(cfg)
    m = m.to(torch.float16).to_empty(device=dev)
    g = torch.Generator(device=dev).manual_seed(T5_SEED)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("layer_norm.weight"):
                std, mean = 0.1, 1.0
            elif "shared" in n or "embed_tokens" in n or "relative_attention_bias" in n:
                std, mean = 1.0, 0.0
            else:                                    # linears: outputs of about unit size at every width
                std, mean = p.shape[1] ** -0.5, 0.0
            p.copy_((torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32) * std + mean).to(p.dtype))
    m.invalidate()
    ids = torch.randint(0, cfg.vocab_size, (1, TEXT_TOKENS), generator=torch.Generator().manual_seed(T5_SEED + 1))
    descs = record_gemms(lambda: m(ids)[0])
    del m
    torch.cuda.empty_cache()
    return descs


def _plain_desc(M: int, N: int, K: int) -> GemmDesc:
    """what ``ops.gemm(a, w, out, M=, N=, K=, bias=)`` on dense operands puts into the descriptor: built by the product's own
    descriptor builder on one-row stand-ins (nothing is allocated at the real size; the replay allocates its own operands)"""
    import torch
    from lkgd_amd import ops
    a, w = torch.empty(1, K, dtype=torch.float16), torch.empty(1, K, dtype=torch.float16)
    out, bias = torch.empty(1, N, dtype=torch.float16), torch.empty(N, dtype=torch.float32)
    return ops._gemm_desc(a, w, out, M=M, N=N, K=K, bias=bias, plan_cus=PLAN_CUS)


#: (layers, channels) of the released models: 2B; 5B and 1.5
REAL_DEPTHS = ((30, 1920), (42, 3072))


def modulation_descs() -> list:
    """the descriptors ``CogVideoXTransformer3DModel._modulation`` builds at real depth: [B, 512] x [(layers * 12 + 2) * D, 512]"""
    return [_plain_desc(B, (layers * 12 + 2) * D, 512) for layers, D in REAL_DEPTHS for B in (2, 1)]


def ladder_descs() -> list:
    """the block linears at D = 1920 and 3072, M in LADDER_ROWS: four widths each - q|k|v in one launch (3D x D), attention out
    (D x D: also what the block issues for q, k and v, which it projects one by one), ff1 (4D x D) and ff2 (D x 4D)"""
    return [_plain_desc(M, N, K) for _, D in REAL_DEPTHS for N, K in ((3 * D, D), (D, D), (4 * D, D), (D, 4 * D))
            for M in LADDER_ROWS]


def record_all(unet, forwards=FORWARDS, fp8_out=None) -> dict:
    """{forward: [GemmDesc ...]} for the named forwards; ``unet`` = the real-width UNet on the GPU (None where no UNet /
    ControlNet / VAE forward is asked for); ``fp8_out`` (a list): receives FP8_FORWARD's lkgd_gemm_fp8 calls"""
    out = {}
    for name in forwards:
        if name in DIT_FORWARDS:
            out[name], calls = record_dit(name, fp8=fp8_out is not None and name == FP8_FORWARD)
            if calls is not None:
                fp8_out.extend(calls)
        elif name == T5_FORWARD:
            out[name] = record_t5()
        elif name == MOD_FORWARD:
            out[name] = modulation_descs()
        elif name == LADDER_FORWARD:
            out[name] = ladder_descs()
    for name in forwards:
        if name.startswith("unet_"):
            cfgb, frames = (int(v) for v in name[5:].split("x"))
            out[name] = record_unet(unet, cfgb, frames)
        elif name == "controlnet_2x14":
            out[name] = record_controlnet(unet)
    if "vae_decode" in forwards or "vae_encode" in forwards:
        dec, enc = record_vae(unet.device)
        if "vae_decode" in forwards:
            out["vae_decode"] = dec
        if "vae_encode" in forwards:
            out["vae_encode"] = enc
    return out


def reduce(records: dict) -> list:
    """distinct signatures of {forward: [GemmDesc]}: [{"fields", "ptr", "launches": {forward: n}, "plan"}], sorted by key"""
    table = {}
    for fwd, descs in records.items():
        for d in descs:
            sig = signature(d)
            e = table.setdefault(sig_key(sig), dict(sig, launches={}))
            e["launches"][fwd] = e["launches"].get(fwd, 0) + 1
    rows = [table[k] for k in sorted(table)]
    for e in rows:
        e["plan"] = plan(desc_from_signature(e))
        variant, why = second_program(e)
        e["second_program"] = variant
        if variant is None:
            e["no_second_program"] = why
    return rows


def reduce_fp8(calls, forward=FP8_FORWARD) -> list:
    """distinct signatures of lkgd_gemm_fp8 argument tuples: [{"fields", "ptr", "launches": {forward: n}}], sorted by key"""
    table = {}
    for args in calls:
        sig = fp8_signature(args)
        e = table.setdefault(sig_key(sig), dict(sig, launches={forward: 0}))
        e["launches"][forward] += 1
    return [table[k] for k in sorted(table)]


def load_fp8_table(path: str = TABLE) -> list:
    with open(path) as f:
        return json.load(f).get("fp8_signatures", [])


def build_c1_unet(dev="cuda:0"):
    """the real-width UNet with the seeded fixture weights (what tests/conftest.py::c1_hip_model builds)"""
    import torch
    from lkgd_amd import unet as pu
    from oracle import unet as ou
    o = ou.UNetSpatioTemporalConditionControlNetModel(ou.SVD_CONFIG)
    ou.init_weights_(o, C1_SEED)
    with torch.no_grad():
        for p in o.parameters():
            p.copy_(p.half().float())
    with torch.device("meta"):
        m = pu.UNetSpatioTemporalConditionControlNetModel(pu.UNetConfig())
    m = m.to_empty(device="cpu")
    m.load_state_dict(o.state_dict(), strict=True)
    del o
    return m.half().to(dev)


def summary(rows) -> str:
    lines = [f"{len(rows)} signatures"]
    for fwd in FORWARDS:
        sel = [e for e in rows if fwd in e["launches"]]
        lines.append(f"  {fwd:16s} {sum(e['launches'][fwd] for e in sel):4d} launches, {len(sel):3d} signatures")
    progs = {}
    for e in rows:
        p = e["plan"]
        k = (p["program"], p["tile_m"], p["tile_n"], p["k_slices"])
        progs[k] = progs.get(k, 0) + 1
    for k in sorted(progs):
        lines.append(f"  program {k[0]} tile {k[1]}x{k[2]} K slices {k[3]}: {progs[k]} signatures")
    return "\n".join(lines)


#: the compute-unit counts and the knob settings of --dump-plans: (label, setter, arguments, arguments that restore the default)
DUMP_CUS = (64, 128, 256, 304)
DUMP_KNOBS = (("auto", None, (), ()),
              ("splitk=0", "lkgd_debug_set_gemm_splitk", (0,), (1,)),
              ("wide_ksplit=2", "lkgd_debug_set_wide_ksplit", (2,), (0,)),
              ("wide_ksplit=4", "lkgd_debug_set_wide_ksplit", (4,), (0,)),
              ("wide_tile_m=192", "lkgd_debug_set_wide_tile_m", (192,), (0,)),
              ("wide_tile_n=256", "lkgd_debug_set_wide_tile_n", (256,), (0,)),
              ("wide_lds_out=0", "lkgd_debug_set_wide_lds_out", (0,), (-1,)),
              ("mid_model forced 3", "lkgd_debug_set_mid_model", (0.0, 0.0, 0.0, 0.0, 3), (0.0, 0.0, 0.0, 0.0, 0)))


def dump_plans(rows, out=sys.stdout):
    """what lkgd_gemm_plan answers for every stored signature at every DUMP_CUS x forced variant 0..7 x DUMP_KNOBS, one line each"""
    lib = _lib.lib()
    info = GemmPlanInfo()
    for i, e in enumerate(rows):
        d = desc_from_signature(e)
        for label, setter, on, off in DUMP_KNOBS:
            if setter:
                getattr(lib, setter)(*on)
            try:
                for variant in range(8):
                    lib.lkgd_debug_set_gemm_variant(variant)
                    for cus in DUMP_CUS:
                        rc = lib.lkgd_gemm_plan(C.byref(d), cus, C.byref(info))
                        got = " ".join(f"{n}={int(getattr(info, n))}" for n in PLAN_FIELDS) if rc == 0 else f"error {rc}"
                        out.write(f"{i} cus={cus} variant={variant} {label}: {got}\n")
            finally:
                lib.lkgd_debug_set_gemm_variant(0)
                if setter:
                    getattr(lib, setter)(*off)


def main(argv):
    if "--dump-plans" in argv:
        return dump_plans(load_table())
    if "--write" in argv:
        fp8_calls = []
        rows = reduce(record_all(build_c1_unet(), fp8_out=fp8_calls))
        with open(TABLE, "w") as f:
            json.dump({"plan_cus": PLAN_CUS, "forwards": list(FORWARDS), "signatures": rows, "fp8_signatures": reduce_fp8(fp8_calls)},
                      f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"wrote {TABLE}")
    else:
        rows = load_table()
    print(summary(rows))
    fp8 = load_fp8_table()
    print(f"  lkgd_gemm_fp8 ({FP8_FORWARD}): {sum(sum(e['launches'].values()) for e in fp8)} launches, {len(fp8)} signatures")


if __name__ == "__main__":
    main(sys.argv[1:])

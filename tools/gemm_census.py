#!/usr/bin/env python3
"""Census of the lkgd_gemm_f16 launches of the real forwards: every descriptor the model issues, reduced to distinct SIGNATURES
(all scalar fields; per pointer NULL-ness and address mod 16; the workspace size), with the launch count per forward and the plan
lkgd_gemm_plan reports at 256 compute units.  tests/golden/gemm_census.json is that table; tests/test_gemm_census_gpu.py replays
every signature of it in isolation against tests/gemm_oracle.py and asserts that a fresh recording gives the same table;
tests/test_host_cpu.py re-derives every stored plan from the stored fields without a GPU.

    python tools/gemm_census.py --write      regenerate the table on a GPU box (weights: the seeded real-width fixtures)
    python tools/gemm_census.py              print a summary of the stored table (no GPU needed)

Forwards (geometry of BASELINE configs[1]: CFG 2 x 14 frames x 72x128 latents):
    unet_2x14                     the full forward
    unet_1x14 / unet_1x7 / unet_1x4   one CFG entry x 14 / 7 / 4 frames: what a rank of 2 / 4 / 8 runs (tools/plan_profile.py)
    controlnet_2x14               the ControlNet encoder with a fresh control video
    vae_decode / vae_encode       the real-width VAE on 2 frames of 96x128 pixels (tests/test_vae.py)"""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from lkgd_amd import _lib                     # noqa: E402
from lkgd_amd._lib import GemmDesc, GemmPlanInfo   # noqa: E402

TABLE = os.path.join(REPO, "tests", "golden", "gemm_census.json")
FORWARDS = ("unet_2x14", "unet_1x14", "unet_1x7", "unet_1x4", "controlnet_2x14", "vae_decode", "vae_encode")
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
        other = 6 if auto["program"] == 4 else 4
        return (other, None) if forced(other)["program"] == other else (None, "geglu80")
    for v in (1, 7, 2):                                  # 128x128 two-stage; where that IS the automatic program, another one
        pl = forced(v)
        if (pl["program"], pl["k_slices"]) != (auto["program"], auto["k_slices"]):
            return v, None
    raise AssertionError("no second program differs from the automatic one")


def load_table(path: str = TABLE) -> list:
    with open(path) as f:
        return json.load(f)["signatures"]


# ---------------------------------------------------------------------------------------------------------------- recording (GPU)
def record_gemms(run):
    """one eager warm-up of ``run()``, then a recorded one: copies of the lkgd_gemm_desc of every lkgd_gemm_f16 call, in order"""
    import torch
    from lkgd_amd import replay
    run()
    torch.cuda.synchronize()
    with replay.strict(False):                 # only the launch list is of interest here: nothing is replayed
        with replay.record() as p:
            run()
    torch.cuda.synchronize()
    descs = [GemmDesc.from_buffer_copy(args[0]._obj) for fn, args, name, _ in p.calls if name == "lkgd_gemm_f16"]
    p.release()
    del p
    torch.cuda.empty_cache()
    return descs


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


def record_all(unet, forwards=FORWARDS) -> dict:
    """{forward: [GemmDesc ...]} for the named forwards; ``unet`` = the real-width UNet on the GPU"""
    out = {}
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


def main(argv):
    if "--write" in argv:
        rows = reduce(record_all(build_c1_unet()))
        with open(TABLE, "w") as f:
            json.dump({"plan_cus": PLAN_CUS, "forwards": list(FORWARDS), "signatures": rows}, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"wrote {TABLE}")
    else:
        rows = load_table()
    print(summary(rows))


if __name__ == "__main__":
    main(sys.argv[1:])

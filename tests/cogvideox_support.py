"""What the CogVideoX DiT tests share (test_cogvideox*.py, test_fp8_*.py): the inputs of make_goldens.py, the half-rounded tiny oracle and
its HIP twin, and the torch statements the loop's glue kernels replace - the patch unfold, the un-patchify, one ATen step, the ATen
loop - for 2-D (``p_t`` None) and temporal patches."""
import os

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DIT_SEED = 191                       # make_goldens.py: weights of tests/golden/cogvideox*.safetensors
P = 2


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def dit_inputs(cfg, seed=DIT_SEED + 1, batch=2):
    """make_goldens.py::dit_inputs"""
    g = torch.Generator().manual_seed(seed)
    f = (cfg.sample_frames - 1) // cfg.temporal_compression_ratio + 1
    return dict(hidden=torch.randn(batch, f, cfg.in_channels, cfg.sample_height, cfg.sample_width, generator=g).half().float(),
                text=torch.randn(batch, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g).half().float(),
                t=torch.tensor([721] * batch), domain=torch.randn(1, 1, 1000, generator=g),
                flow=torch.randn(1, 1, 1000, generator=g))


def tiny_oracle(seed=DIT_SEED, cfg=None):
    """the fp32 oracle (``oc.TINY_DIT`` unless ``cfg``) with ``init_weights_(seed)`` rounded to fp16 values"""
    from oracle import cogvideox as oc
    o = oc.init_weights_(oc.CogVideoXTransformer3DModel(oc.TINY_DIT if cfg is None else cfg), seed)
    with torch.no_grad():
        for p in o.parameters():
            p.copy_(p.half().float())
    return o


def hip_twin(o, cfg=None, dev=None):
    """the HIP model of ``cfg`` (``oc.TINY_DIT`` unless given) holding ``o``'s weights, every key checked; on the CPU in the weights'
    dtype, or fp16 on ``dev``"""
    from lkgd_amd import cogvideox as pc
    from oracle import cogvideox as oc
    m = pc.CogVideoXTransformer3DModel(pc.DiTConfig(**(oc.TINY_DIT if cfg is None else cfg).__dict__))
    missing, unexpected = m.load_state_dict(o.state_dict(), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return m if dev is None else m.half().to(dev)


def tiny_cpu_model(seed=None, **over):
    """the HIP model class at ``oc.TINY_DIT`` (+ ``over``) on the CPU: as constructed, or with the oracle's ``init_weights_(seed)``"""
    from oracle import cogvideox as oc
    cfg = oc.DiTConfig(**{**oc.TINY_DIT.__dict__, **over})
    if seed is None:
        from lkgd_amd import cogvideox as pc
        return pc.CogVideoXTransformer3DModel(pc.DiTConfig(**cfg.__dict__))
    return hip_twin(oc.init_weights_(oc.CogVideoXTransformer3DModel(cfg), seed), cfg)


def loop_inputs(c=None, seed=5, f=3, cfg=True):
    """(latents, image latents, prompt embeddings, domain, flow) of a ``denoise`` over f latent frames of ``c`` (``oc.TINY_DIT``)"""
    if c is None:
        from oracle import cogvideox as oc
        c = oc.TINY_DIT
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(1, f, 16, c.sample_height, c.sample_width, generator=g)
    img = (0.5 * torch.randn(1, f, 16, c.sample_height, c.sample_width, generator=g)).half().float()
    pe = torch.randn(2 if cfg else 1, c.max_text_seq_length, c.text_embed_dim, generator=g).half().float()
    return lat, img, pe, torch.randn(1, 1, 1000, generator=g), torch.randn(1, 1, 1000, generator=g)


# ------------------------------------------------------------------------------------------------------------- the glue
def patchify(x, p_t=None):
    """[B, F, C, H, W] -> patch rows: the 2-D statement (column (c, py, px)), or with ``p_t`` the reshape of the 1.5 patch embedding
    ([EXT] diffusers CogVideoXPatchEmbed; column (c, pt, py, px))"""
    B, F, C_, H, W = x.shape
    h, w = H // P, W // P
    if p_t is None:
        return x.reshape(B, F, C_, h, P, w, P).permute(0, 1, 3, 5, 2, 4, 6).reshape(B * F * h * w, C_ * P * P).contiguous()
    r = x.permute(0, 1, 3, 4, 2).reshape(B, F // p_t, p_t, h, P, w, P, C_).permute(0, 1, 3, 5, 7, 2, 4, 6).flatten(4, 7).flatten(1, 3)
    return r.reshape(-1, C_ * p_t * P * P).contiguous()


def unpatchify(rows, B, F, H, W, p_t=None):
    """cogvideox_transformer_3d.py:624-625, or with ``p_t`` :626-630"""
    h, w = H // P, W // P
    if p_t is None:
        return rows.reshape(B, F, h, w, -1, P, P).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4).contiguous()
    out = rows.reshape(B, (F + p_t - 1) // p_t, h, w, -1, p_t, P, P)
    return out.permute(0, 1, 5, 4, 2, 6, 3, 7).flatten(6, 7).flatten(4, 5).flatten(1, 2).contiguous()


def glue_data(shape, seed, p_t=None):
    """(fp32 latents, fp16 image latents, fp16 proj_out rows of both CFG entries) of a [B, F, C, H, W] clip"""
    g = torch.Generator().manual_seed(seed)
    B, F, C_, H, W = shape
    pt = p_t or 1
    lat = torch.randn(B, F, C_, H, W, generator=g)
    img = (0.5 * torch.randn(B, F, C_, H, W, generator=g)).half()
    noise = (2 * torch.randn(2 * B * (F // pt) * (H // P) * (W // P), C_ * pt * P * P, generator=g)).half()
    return lat, img, noise


def aten_step(noise_rows, lat, cfg, g, coef, p_t=None):
    """the loop body the step kernel replaces, on the tensors' device: the un-patchify, .float(), the CFG statements,
    CogVideoXDDIMScheduler.step, the cast back"""
    B, F, C_, H, W = lat.shape
    noise = unpatchify(noise_rows, cfg * B, F, H, W, p_t).float()
    if cfg == 2:
        u, c = noise.chunk(2)
        noise = u + g * (c - u)
    a, b, sa, sb = coef
    sample = lat.float()
    x0 = sa * sample - sb * noise
    return (a * sample + b * x0).to(lat.dtype)


def aten_denoise(pc, m, sched, latents, image_latents, prompt_embeds, dom, flow, steps, guidance_scale, callback, rope=None, ofs=None):
    """the loop of pipeline_cogvideox_image2video.py:829-885 without the glue kernels (``denoise`` as it was before them):
    ``forward_tokens`` on the CFG-duplicated, channel-concatenated batch + the ATen statements"""
    sched.set_timesteps(steps)
    cfg = guidance_scale > 1.0
    text = m.fused_text(prompt_embeds, dom, flow)
    latents = latents.to(torch.float16)
    img = image_latents.to(torch.float16)
    img2 = torch.cat([img] * 2) if cfg else img
    for i, t in enumerate(sched.timesteps.tolist()):
        x = torch.cat([latents] * 2) if cfg else latents
        x = torch.cat([x, img2], dim=2)
        noise = m.forward_tokens(x, text, float(t), image_rotary_emb=rope, ofs=ofs).float()
        g = pc.dynamic_guidance(guidance_scale, steps, t)
        if cfg:
            u, c = noise.chunk(2)
            noise = u + g * (c - u)
        latents = sched.step(noise, t, latents.float())[0].to(torch.float16)
        callback(i, t, latents)
    return latents

"""What the pipeline tests share (test_cogvideox_pipeline_gpu.py): tiny components of every stage with their fp32 oracles, the
reference's ``__call__`` (pipeline_cogvideox_image2video.py:610-919) spelled out twice independently of
``lkgd_amd.pipeline_cogvideox`` - once over the HIP stage functions (``by_hand``: what the class must equal to the bit), once over the
fp32 CPU oracles (``oracle_call``: what it must be close to) - and the wrong orders both can be told to take (``DECOYS``)."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import cogvideox15_oracle as vo
import cogvideox_vae_encoder_oracle as eo
import cogvideox_vae_oracle as dec_oracle
from cogvideox_support import DEV, DIT_SEED, hip_twin, tiny_oracle
from t5_support import StubTokenizer, hf_model
from t5_support import hip_twin as t5_twin

H, W = 48, 80                          # the VAE tests' pixel size: 6 x 10 latents, 3 x 5 tokens
SEQ = 16                               # max_text_seq_length of the tiny DiTs
#: one layer at the width the fuse kernel is built for
T5_CFG = dict(vocab_size=128, d_model=4096, d_kv=64, d_ff=128, num_layers=1, num_heads=2)

#: the wrong orders: each must miss the bit-equality with the class
DECOYS = ("positive_first", "noise_first", "keep_padding", "no_scaling", "fp32_image")


def _vit_pair(seed):
    from lkgd_amd import vit as pv
    from oracle import vit as ov
    cfg = ov.ViTConfig(img_size=64, embed_dim=128, depth=1, num_heads=2, num_classes=1000)
    o = ov.init_weights_(ov.VisionTransformer(cfg), seed)
    with torch.no_grad():
        for p in o.parameters():
            p.copy_(p.half().float())
    m = pv.VisionTransformer(pv.ViTConfig(**cfg.__dict__))
    m.load_state_dict(o.state_dict())
    return o, m.half().to(DEV)


def _vae_pair():
    """the encoder recipe's weights (eo.tiny_weights) with the decoder recipe's + 1 on every conv_y bias"""
    from lkgd_amd import cogvideox_vae as pv
    o = eo.tiny_weights()
    with torch.no_grad():
        for n, p in o.named_parameters():
            if n.startswith("decoder.") and n.endswith("conv_y.conv.bias"):
                p.copy_((p + 1.0).half().float())
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**eo.TINY.__dict__), encoder=True)
    m.load_state_dict(o.state_dict())
    d = dec_oracle.AutoencoderKLCogVideoX(eo.TINY)
    d.decoder.load_state_dict(o.decoder.state_dict())
    return o, d, m.half().to(DEV)


def _dit_pair(v15: bool):
    from oracle import cogvideox as oc
    if v15:
        cfg = vo.V15DiTConfig(**{**vo.TINY_V15_DIT.__dict__, "sample_height": 6, "sample_width": 10})
        o = vo.seeded_model(cfg, DIT_SEED)
    else:
        cfg = oc.DiTConfig(**{**oc.TINY_DIT.__dict__, "sample_height": 6, "sample_width": 10})
        o = tiny_oracle(cfg=cfg)
    return o, hip_twin(o, cfg, DEV)


def build():
    """every tiny component once: .ref the fp32 oracles, the HIP modules on the GPU, and ``pipe(kind, scheduler)``"""
    t5_ref = hf_model(T5_CFG)
    te = t5_twin(t5_ref, T5_CFG, DEV)
    vae_o, dec_o, vae = _vae_pair()
    dom_o, dom = _vit_pair(21)
    flow_o, flow = _vit_pair(22)
    dits = {"sincos": _dit_pair(False), "v15": _dit_pair(True)}
    parts = SimpleNamespace(t5_ref=t5_ref, te=te, tok=StubTokenizer(T5_CFG["vocab_size"]), vae_o=vae_o, dec_o=dec_o, vae=vae, dom_o=dom_o,
                            dom=dom, flow_o=flow_o, flow=flow, dits=dits)

    def pipe(kind="sincos", scheduler="ddim"):
        from lkgd_amd import cogvideox as pc
        from lkgd_amd.pipeline_cogvideox import CogVideoXImageToVideoPipeline
        sched = pc.CogVideoXDDIMScheduler() if scheduler == "ddim" else pc.CogVideoXDPMScheduler()
        return CogVideoXImageToVideoPipeline(parts.tok, te, vae, dits[kind][1], sched, dom, flow)
    parts.pipe = pipe
    return parts


def pil_image(seed=31, size=(96, 60)):
    """an RGB image that is not the target size: the lanczos resize takes part"""
    import PIL.Image
    g = torch.Generator().manual_seed(seed)
    px = torch.randint(0, 256, (size[1], size[0], 3), generator=g, dtype=torch.uint8)
    return PIL.Image.fromarray(px.numpy())


def host_image(image):
    """``video_processor.preprocess`` on the host: VaeImageProcessor's chain, fp32 [B, 3, H, W]"""
    from lkgd_amd.image_processor import VaeImageProcessor
    return VaeImageProcessor(vae_scale_factor=8).preprocess(image, height=H, width=W)


def torch_frames(video, output_type):
    """``postprocess_video`` as torch states it on the decoded clip's own device ([B, 3, T, H, W] fp16)"""
    d = (video / 2 + 0.5).clamp(0, 1)
    if output_type == "pt":
        return d.permute(0, 2, 1, 3, 4)
    f = d.permute(0, 2, 3, 4, 1).float()
    return f if output_type == "np" else (f * 255).round().to(torch.uint8)


def by_hand(parts, kind, scheduler, image, prompt=None, negative_prompt=None, *, num_frames, steps, guidance_scale, generator=None,
            use_dynamic_cfg=False, latents=None, prompt_embeds=None, negative_prompt_embeds=None, latent=False, decoy=None):
    """the reference's call over the HIP stage functions, in its order -> the final latents (``latent``) or the decoded clip"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd.cogvideox_vae import decode_latents
    dit, vae = parts.dits[kind][1], parts.vae
    sched = pc.CogVideoXDDIMScheduler() if scheduler == "ddim" else pc.CogVideoXDPMScheduler()
    tc = dit.config
    cfg = guidance_scale > 1.0
    if prompt is not None:
        B = 1 if isinstance(prompt, str) else len(prompt)
    else:
        B = prompt_embeds.shape[0]
    pe, ne = pc.encode_prompt(parts.te, parts.tok, prompt, negative_prompt, cfg, 1, prompt_embeds, negative_prompt_embeds, SEQ, DEV)
    if cfg:
        pe = torch.cat([pe, ne] if decoy == "positive_first" else [ne, pe], dim=0)
    latent_frames = (num_frames - 1) // 4 + 1
    add, p_t = 0, tc.patch_size_t
    if p_t is not None and latent_frames % p_t != 0:
        add = p_t - latent_frames % p_t
        num_frames += add * 4
    img = host_image(image).to(DEV) if decoy == "fp32_image" else host_image(image).to(DEV, dtype=pe.dtype)
    dom = parts.dom(img).unsqueeze(1)
    flow = parts.flow(img).unsqueeze(1)
    if decoy == "noise_first":
        assert latents is None and not isinstance(generator, list)
        shape = (B, latent_frames + add, tc.in_channels // 2, H // 8, W // 8)
        latents = torch.randn(shape, generator=generator, device=generator.device, dtype=pe.dtype)
    lat, img_lat = pc.prepare_latents(vae, sched, tc, img, B, tc.in_channels // 2, num_frames, H, W, pe.dtype, DEV, generator, latents)
    rope = None
    if tc.use_rotary_positional_embeddings:
        f = lat.size(1) if p_t is None else (lat.size(1) + p_t - 1) // p_t
        rope = pc.rotary_tables(tc, f, H // (8 * tc.patch_size), W // (8 * tc.patch_size))
    lat = pc.denoise(dit, sched, lat, img_lat, pe, dom, flow, steps, guidance_scale, use_dynamic_cfg, None, rope, None, generator)
    if latent:
        return lat
    if decoy != "keep_padding":
        lat = lat[:, add:]
    if decoy == "no_scaling":
        return vae.decode(lat.permute(0, 2, 1, 3, 4)).sample
    return decode_latents(vae, lat)


@torch.no_grad()
def oracle_call(parts, image, ids, neg_ids, image_noise, init_noise, *, steps, guidance_scale, use_dynamic_cfg=False, decoy=None):
    """the same call over the fp32 CPU oracles (sin-cos DiT, DDIM): transformers' T5, the oracle ViTs behind the bilinear resize, the
    VAE oracles, the oracle DiT with its fuse in the oracle loop, and the call's glue as torch statements.  ``image`` fp32
    [B, 3, H, W] holding the fp16 values the pipeline casts to; ``image_noise`` [B, 16, 1, h, w] the posterior's draw; ``init_noise``
    [B, F, 16, h, w].  -> (final latents, ``pt`` frames [B, T, 3, H, W])"""
    from oracle import cogvideox as oc
    dit = parts.dits["sincos"][0]
    sf = eo.TINY.scaling_factor
    pe = parts.t5_ref(input_ids=ids).last_hidden_state
    ne = parts.t5_ref(input_ids=neg_ids).last_hidden_state
    prompt = torch.cat([pe, ne] if decoy == "positive_first" else [ne, pe], dim=0)
    x = F.interpolate(image, size=[64, 64], mode="bilinear")
    dom, flow = parts.dom_o(x).unsqueeze(1), parts.flow_o(x).unsqueeze(1)
    mean, _, std = parts.vae_o.posterior(image[:, :, None])
    if decoy == "noise_first":                       # the two draws trade places (same shapes per frame: the first frame's noise)
        image_noise, init_noise = init_noise[:, :1].permute(0, 2, 1, 3, 4), torch.cat(
            [image_noise.permute(0, 2, 1, 3, 4), init_noise[:, 1:]], dim=1)
    first = (sf * (mean + std * image_noise)).permute(0, 2, 1, 3, 4)
    img_lat = torch.cat([first, torch.zeros_like(init_noise[:, 1:])], dim=1)
    lat = oc.denoise(dit, oc.CogVideoXDDIMScheduler(), init_noise.clone(), img_lat, prompt, dom, flow, steps, guidance_scale,
                     use_dynamic_cfg)
    z = lat.permute(0, 2, 1, 3, 4)
    frames = parts.dec_o.decode(z if decoy == "no_scaling" else z * (1.0 / sf))
    return lat, (frames / 2 + 0.5).clamp(0, 1).permute(0, 2, 1, 3, 4)

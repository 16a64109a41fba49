"""What the text-to-video / video-to-video pipeline tests share (test_cogvideox_t2v_v2v_*.py).  Nothing here is new oracle code: the tiny
components and their fp32 oracles are those of cogvideox_pipeline_oracle.py (T5, VAE), cogvideox_support.py / cogvideox15_oracle.py (the
DiT, here with ``in_channels`` 16: the stock transformer sees the latents alone) and dpm_oracle.py (the DPM-Solver++ restatement).
Composed from them, independently of ``lkgd_amd.pipeline_cogvideox``:

* ``by_hand_t2v`` / ``by_hand_v2v``: diffusers' two ``__call__`` orders ([EXT], parity unpinned) over the HIP stage functions - what the
  classes must equal to the bit - and ``hand_loop``, ``denoise``'s loop over the public launches with the switches the V2V decoys need;
* ``oracle_t2v`` / ``oracle_v2v``: the same calls over the fp32 CPU oracles, the DiT oracle run without its fuse line
  (``dit_no_fuse``), every random draw handed in;
* ``V2V_DECOYS``: the five wrong video-to-video calls both statements can be told to make."""
from types import SimpleNamespace

import torch

import cogvideox15_oracle as vo
import cogvideox_pipeline_oracle as po
import cogvideox_vae_encoder_oracle as eo
import dpm_oracle as do
from cogvideox_support import DEV, DIT_SEED, hip_twin, tiny_oracle
from t5_support import StubTokenizer, hf_model
from t5_support import hip_twin as t5_twin

H, W, SEQ = po.H, po.W, po.SEQ         # 48 x 80 pixels: 6 x 10 latents, 3 x 5 tokens - the size the tiny VAE and DiT fixtures are made for
CHANNELS = 16

#: each must miss the class's latents
V2V_DECOYS = ("noise_first", "start_off_by_one", "untruncated_guidance", "second_order_first", "first_timestep")


def _dit_pair(v15: bool):
    from oracle import cogvideox as oc
    over = {"in_channels": CHANNELS, "sample_height": 6, "sample_width": 10}
    if v15:                             # the 1.5 text-to-video architecture: temporal patches, rotary, no ofs embedding
        cfg = vo.V15DiTConfig(**{**vo.TINY_V15_DIT.__dict__, **over, "ofs_embed_dim": None})
        o = vo.seeded_model(cfg, DIT_SEED)
    else:
        cfg = oc.DiTConfig(**{**oc.TINY_DIT.__dict__, **over})
        o = tiny_oracle(cfg=cfg)
    return o, hip_twin(o, cfg, DEV)


def build():
    """every tiny component once: the fp32 oracles, the HIP modules on the GPU, and ``pipe(cls, kind, scheduler)``"""
    t5_ref = hf_model(po.T5_CFG)
    te = t5_twin(t5_ref, po.T5_CFG, DEV)
    vae_o, dec_o, vae = po._vae_pair()
    dits = {"sincos": _dit_pair(False), "v15": _dit_pair(True)}
    parts = SimpleNamespace(t5_ref=t5_ref, te=te, tok=StubTokenizer(po.T5_CFG["vocab_size"]), vae_o=vae_o, dec_o=dec_o, vae=vae, dits=dits)

    def pipe(cls, kind="sincos", scheduler="ddim", vae=None, snr_shift_scale=3.0):
        from lkgd_amd import pipeline_cogvideox as pp
        return getattr(pp, cls)(parts.tok, te, vae if vae is not None else parts.vae, dits[kind][1], _scheduler(scheduler, snr_shift_scale))
    parts.pipe = pipe
    return parts


def _scheduler(name, snr_shift_scale=3.0):
    """3.0: CogVideoX-2B's scheduler_config.json (the classes' default); 1.0: the 5B models'"""
    from lkgd_amd import cogvideox as pc
    return (pc.CogVideoXDDIMScheduler if name == "ddim" else pc.CogVideoXDPMScheduler)(snr_shift_scale=snr_shift_scale)


def pil_clip(T, seed=51, size=(96, 60)):
    """T RGB frames that are not the target size: the lanczos resize takes part"""
    return [po.pil_image(seed + t, size) for t in range(T)]


def host_video(video):
    """``preprocess_video`` on the host: VaeImageProcessor's chain per clip, fp32 [B, 3, T, H, W]"""
    from lkgd_amd.image_processor import VaeImageProcessor
    ip = VaeImageProcessor(vae_scale_factor=8)
    clips = video if isinstance(video[0], list) else [video]
    return torch.stack([ip.preprocess(c, height=H, width=W) for c in clips]).permute(0, 2, 1, 3, 4)


# ------------------------------------------------------------------------------------------- over the HIP stage functions
def _prompt(parts, prompt, negative_prompt, cfg, num_videos_per_prompt):
    from lkgd_amd import cogvideox as pc
    pe, ne = pc.encode_prompt(parts.te, parts.tok, prompt, negative_prompt, cfg, num_videos_per_prompt, None, None, SEQ, DEV)
    return torch.cat([ne, pe], dim=0) if cfg else pe


def _rope(tc, latent_frames):
    from lkgd_amd import cogvideox as pc
    if not tc.use_rotary_positional_embeddings:
        return None
    p_t = tc.patch_size_t
    f = latent_frames if p_t is None else (latent_frames + p_t - 1) // p_t
    return pc.rotary_tables(tc, f, H // (8 * tc.patch_size), W // (8 * tc.patch_size))


def by_hand_t2v(parts, kind, scheduler, prompt, negative_prompt=None, *, num_frames, steps, guidance_scale, generator=None,
                use_dynamic_cfg=False, latents=None, num_videos_per_prompt=1, latent=True):
    """diffusers' text-to-video call over the HIP stage functions -> the final latents (``latent``) or the decoded clip"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd.cogvideox_vae import decode_latents
    dit, sched = parts.dits[kind][1], _scheduler(scheduler)
    tc = dit.config
    B = (1 if isinstance(prompt, str) else len(prompt)) * num_videos_per_prompt
    pe = _prompt(parts, prompt, negative_prompt, guidance_scale > 1.0, num_videos_per_prompt)
    latent_frames = (num_frames - 1) // 4 + 1
    add, p_t = 0, tc.patch_size_t
    if p_t is not None and latent_frames % p_t != 0:
        add = p_t - latent_frames % p_t
        num_frames += add * 4
    lat = pc.prepare_noise_latents(sched, tc, parts.vae.config, B, tc.in_channels, num_frames, H, W, pe.dtype, DEV, generator, latents)
    lat = pc.denoise(dit, sched, lat, None, pe, None, None, steps, guidance_scale, use_dynamic_cfg, None, _rope(tc, lat.size(1)), None,
                     generator)
    return lat if latent else decode_latents(parts.vae, lat[:, add:])


def hand_loop(dit, sched, latents, prompt_embeds, *, steps, guidance_scale, use_dynamic_cfg, generator, start_step=0,
              guidance_steps=None, first_t_back=None):
    """``denoise``'s loop for a sin-cos model without image latents and without the fuse, over the public launches; ``guidance_steps``
    (default ``steps - start_step``) and ``first_t_back`` (default None: the first executed step is first order) are the decoys'"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ops
    sched.set_timesteps(steps)
    dpm = isinstance(sched, pc.CogVideoXDPMScheduler)
    cfg = guidance_scale > 1.0
    text = prompt_embeds.to(device=DEV, dtype=torch.float16).contiguous()
    lat = latents.to(device=DEV, dtype=torch.float16).clone(memory_format=torch.contiguous_format)
    p = dit.config.patch_size
    grid = (lat.shape[1], lat.shape[3] // p, lat.shape[4] // p)
    x0_state = torch.zeros(lat.shape, dtype=torch.float32, device=DEV)
    n = steps - start_step if guidance_steps is None else guidance_steps
    t_back, rows = first_t_back, None
    for t in sched.timesteps[start_step:].tolist():
        rows = ops.dit_patch_rows(lat, None, p, out=rows)
        noise_rows = dit.forward_rows(rows, grid, text, float(t))
        g = pc.dynamic_guidance(guidance_scale, n, t) if use_dynamic_cfg else guidance_scale
        if dpm:
            k = sched.coefficients(int(t), t_back)
            eps = pc.dpm_noise(lat.shape, lat.dtype, DEV, generator, k.order)
            ops.dit_cfg_dpm_step(noise_rows, lat, x0_state, eps, p, 2 if cfg else 1, k.order, g, k)
            t_back = int(t)
        else:
            ops.dit_cfg_ddim_step(noise_rows, lat, p, 2 if cfg else 1, g, *sched.coefficients(int(t)))
    return lat


def by_hand_v2v(parts, kind, scheduler, video, prompt, negative_prompt=None, *, strength, steps, guidance_scale, generator=None,
                use_dynamic_cfg=False, latents=None, latent=True, decoy=None, loop="denoise"):
    """diffusers' video-to-video call over the HIP stage functions; ``video`` PIL frames (one clip or a list of clips).  ``loop``:
    ``denoise`` itself, or ``hand_loop`` (which the decoys of the loop need)"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd.cogvideox_vae import decode_latents
    assert decoy is None or decoy in V2V_DECOYS
    dit, vae, sched = parts.dits[kind][1], parts.vae, _scheduler(scheduler)
    tc = dit.config
    B = 1 if isinstance(prompt, str) else len(prompt)
    pe = _prompt(parts, prompt, negative_prompt, guidance_scale > 1.0, 1)
    sched.set_timesteps(steps)
    times, _, t_start = pc.get_timesteps(sched, steps, strength)
    timestep = (sched.timesteps if decoy == "first_timestep" else times)[:1].repeat(B)
    if latents is not None:
        lat = latents.to(DEV) * sched.init_noise_sigma                 # given latents are taken as they are: nothing is encoded
    else:
        clip = host_video(video).to(DEV, dtype=pe.dtype)
        if decoy == "noise_first":
            assert B == 1 and not isinstance(generator, list)
            shape = (1, (clip.shape[2] - 1) // 4 + 1, tc.in_channels, H // 8, W // 8)
            noise = pc.initial_noise(shape, pe.dtype, DEV, generator)
            init = vae.encode(clip).latent_dist.sample(generator, scale=vae.config.scaling_factor).permute(0, 2, 1, 3, 4)
            lat = sched.add_noise(init, noise, timestep)
        else:
            lat = pc.prepare_video_latents(vae, sched, clip, B, tc.in_channels, H, W, pe.dtype, DEV, generator, None, timestep)
    start = t_start + 1 if decoy == "start_off_by_one" else t_start
    if loop == "denoise" and decoy not in ("untruncated_guidance", "second_order_first"):
        lat = pc.denoise(dit, sched, lat, None, pe, None, None, steps, guidance_scale, use_dynamic_cfg, None, _rope(tc, lat.size(1)),
                         None, generator, start_step=start)
    else:
        lat = hand_loop(dit, sched, lat, pe, steps=steps, guidance_scale=guidance_scale, use_dynamic_cfg=use_dynamic_cfg,
                        generator=generator, start_step=start, guidance_steps=steps if decoy == "untruncated_guidance" else None,
                        first_t_back=int(sched.timesteps[t_start - 1]) if decoy == "second_order_first" else None)
    return lat if latent else decode_latents(vae, lat)


# ------------------------------------------------------------------------------------------------ over the fp32 CPU oracles
def dit_no_fuse(m, hidden_states, text, timestep):
    """``oracle.cogvideox.CogVideoXTransformer3DModel.forward`` without its ``lk_fuse`` line: the stock transformer"""
    b, f, c, h, w = hidden_states.shape
    emb = m.time_embedding(m.time_proj(timestep).to(hidden_states.dtype))
    x = m.patch_embed(text, hidden_states)
    tl = text.shape[1]
    enc, hid = x[:, :tl], x[:, tl:]
    for blk in m.transformer_blocks:
        hid, enc = blk(hid, enc, emb)
    hid = m.proj_out(m.norm_out(m.norm_final(hid), temb=emb))
    p = m.config.patch_size
    return hid.reshape(b, f, h // p, w // p, -1, p, p).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4)


def _oracle_schedule(steps, snr_shift_scale=3.0):
    from oracle import cogvideox as oc
    s = oc.CogVideoXDDIMScheduler(snr_shift_scale=snr_shift_scale)
    s.set_timesteps(steps)
    return s


def dpm_orders(steps, start_step=0, first_t_back=None):
    """the order of every executed DPM step (dpm_oracle.coefficients): how often the step draws (the same for every snr_shift_scale)"""
    s = _oracle_schedule(steps)
    ac, orders, t_back = s.alphas_cumprod.tolist(), [], first_t_back
    for t in s.timesteps[start_step:].tolist():
        orders.append(do.coefficients(ac, t, t_back, steps).order)
        t_back = t
    return orders


def host_draws(generator, shapes, orders, lat_shape):
    """the pipeline's draws replayed on the host: one fp16 ``randn`` per shape of ``shapes`` in order, then per DPM step ``order`` draws
    of ``lat_shape`` of which the last is kept -> (the first draws, the steps' kept draws), fp32"""
    first = [torch.randn(s, generator=generator, dtype=torch.float16).float() for s in shapes]
    eps = []
    for order in orders:
        for _ in range(order):
            e = torch.randn(lat_shape, generator=generator, dtype=torch.float16)
        eps.append(e.float())
    return first, eps


@torch.no_grad()
def oracle_loop(dit, latents, prompt, *, steps, guidance_scale, use_dynamic_cfg, scheduler, eps=None, start_step=0, guidance_steps=None,
                first_t_back=None, snr_shift_scale=3.0):
    """the loop over the fp32 DiT oracle: DDIM by the oracle's scheduler, DPM by dpm_oracle's coefficients and fp64 step"""
    from oracle import cogvideox as oc
    s = _oracle_schedule(steps, snr_shift_scale)
    ac = s.alphas_cumprod.tolist()
    cfg = guidance_scale > 1.0
    n = steps - start_step if guidance_steps is None else guidance_steps
    t_back, x0_old = first_t_back, torch.zeros_like(latents)
    for i, t in enumerate(s.timesteps[start_step:].tolist()):
        x = torch.cat([latents] * 2) if cfg else latents
        noise = dit_no_fuse(dit, x, prompt, torch.full((x.shape[0],), t, dtype=torch.long)).float()
        g = oc.dynamic_guidance(guidance_scale, n, t) if use_dynamic_cfg else guidance_scale
        if cfg:
            u, c = noise.chunk(2)
            noise = u + g * (c - u)
        if scheduler == "ddim":
            latents = s.step(noise, t, latents)
        else:
            out, x0_old, _, _ = do.step_fp64(noise, x0_old, latents, eps[i], do.coefficients(ac, t, t_back, steps))
            latents, t_back = out.float(), t
    return latents


def _decoded(parts, lat):
    frames = parts.dec_o.decode(lat.permute(0, 2, 1, 3, 4) * (1.0 / eo.TINY.scaling_factor))
    return lat, (frames / 2 + 0.5).clamp(0, 1).permute(0, 2, 1, 3, 4)


def _oracle_prompt(parts, ids, neg_ids):
    return torch.cat([parts.t5_ref(input_ids=neg_ids).last_hidden_state, parts.t5_ref(input_ids=ids).last_hidden_state], dim=0)


@torch.no_grad()
def oracle_t2v(parts, ids, neg_ids, init_noise, *, steps, guidance_scale, scheduler="ddim", eps=None, use_dynamic_cfg=False):
    """-> (final latents, ``pt`` frames [B, T, 3, H, W])"""
    lat = oracle_loop(parts.dits["sincos"][0], init_noise.clone(), _oracle_prompt(parts, ids, neg_ids), steps=steps,
                      guidance_scale=guidance_scale, use_dynamic_cfg=use_dynamic_cfg, scheduler=scheduler, eps=eps)
    return _decoded(parts, lat)


@torch.no_grad()
def oracle_v2v(parts, clip, ids, neg_ids, post_noise, noise, *, steps, strength, guidance_scale, scheduler="dpm", eps=None,
               use_dynamic_cfg=False, decoy=None, snr_shift_scale=3.0):
    """``clip`` fp32 [1, 3, T, H, W] holding the fp16 values the pipeline casts to; ``post_noise`` [1, 16, F, h, w] the posterior's draw,
    ``noise`` [1, F, 16, h, w] the draw ``add_noise`` mixes in, ``eps`` the DPM steps' kept draws.  ``decoy``: one of V2V_DECOYS except
    ``noise_first`` (which is a matter of the draws handed in)"""
    s = _oracle_schedule(steps, snr_shift_scale)
    t_start = max(steps - min(int(steps * strength), steps), 0)
    mean, _, std = parts.vae_o.posterior(clip)
    init = (eo.TINY.scaling_factor * (mean + std * post_noise)).permute(0, 2, 1, 3, 4)
    a = s.alphas_cumprod[int(s.timesteps[0 if decoy == "first_timestep" else t_start])]
    lat = (float(a ** 0.5) * init + float((1 - a) ** 0.5) * noise).float()
    lat = oracle_loop(parts.dits["sincos"][0], lat, _oracle_prompt(parts, ids, neg_ids), steps=steps, guidance_scale=guidance_scale,
                      use_dynamic_cfg=use_dynamic_cfg, scheduler=scheduler, eps=eps,
                      start_step=t_start + 1 if decoy == "start_off_by_one" else t_start,
                      guidance_steps=steps if decoy == "untruncated_guidance" else None,
                      first_t_back=int(s.timesteps[t_start - 1]) if decoy == "second_order_first" else None,
                      snr_shift_scale=snr_shift_scale)
    return _decoded(parts, lat)

#!/usr/bin/env python3
"""Do the denoising loops compute the same bytes as at another revision?

    python tools/loop_identity.py > here.txt          (and the same file, unmodified, in a worktree of the other revision)

The gate of a refactor that must not change what a loop enqueues.  Only signatures both revisions have are used.  The tiny
UNet and inputs of tests/test_dist_gpu.py (8x8 latents, block_out_channels (64, 128, 128, 128)) run on cuda:0 through
``pipe.denoise`` (one process: CFG on / off, ``start_step`` + callback, ``direct_fusion``, a ControlNet condition, the eager module
walk, the HIP graph), through ``DistDenoiser`` (worlds 2 and 4 over gloo, replay on and off, one and two clips, with and without a
ControlNet) and through ``DistDiTDenoiser`` (worlds 2 and 4, 3 latent frames).  The one-process CogVideoX cases (``dit_one``: 3 to
4 steps on 3 latent frames of 8 x 12, tiny two-layer models with synthetic weights) run ``cogvideox.denoise`` (DDIM, DPM with a
seeded generator, guidance off, ``start_step`` + callback, text-to-video, a ``patch_size_t`` model with ``ofs``) and
``ddim_inversion.sample`` (inverse, guided under ``OverrideAttnProcessors``, references without the override; the whole
trajectory is hashed).  ``sample`` is handed a minimal pipeline object - ``encode_prompt`` returns seeded embeddings, no tokenizer
or T5 is involved.  One line per case and rank: the sha256 of the final latents' bytes.  Two 7-step cases also run with ``ops.GEMM_EVENTS = []`` and print how many entries were appended and whether
``ops.GEMM_EVENTS`` is the same list afterwards.  Two outputs are compared with diff(1).

Every rank is a fresh child process under its own ``timeout -k 10``; the first non-zero exit status ends the run.
"""
import hashlib
import os
import socket
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

#: (name, world, frames, CFG, clips, ControlNet) of the sharded SVD launches; each runs with replay on and off
SVD_WORLDS = [("svd_w2_f4_cfg", 2, 4, True, 1, False), ("svd_w4_f5_cfg", 4, 5, True, 1, False),
              ("svd_w2_f5_nocfg", 2, 5, False, 1, False), ("svd_w4_f6_nocfg", 4, 6, False, 1, False),
              ("svd_w4_f4_cfg_2clips_cn", 4, 4, True, 2, True)]
DIT_WORLDS = [("dit_w2_f3", 2), ("dit_w4_f3", 4)]
EVENTS_CASE = "svd_w2_f4_cfg"          # the sharded launch that also runs 7 steps with an event list


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def say(case, rank, text):
    print(f"{case:<40s} rank {rank}  {text}", flush=True)


# ---- models and inputs (tests/test_dist_gpu.py) ---------------------------------------------------------------------------------
def unet_config():
    from lkgd_amd import unet as pu
    return pu.UNetConfig(sample_size=8, block_out_channels=(64, 128, 128, 128), num_attention_heads=(1, 2, 2, 2),
                         addition_time_embed_dim=64, projection_class_embeddings_input_dim=192, num_frames=4)


def make_pipe(dev, controlnet=False):
    from lkgd_amd import controlnet as pc
    from lkgd_amd import unet as pu
    from lkgd_amd.pipeline import StableVideoDiffusionPipeline
    if not controlnet:
        m = pu.UNetSpatioTemporalConditionControlNetModel(unet_config()).half().to(dev)
        pu.init_synthetic_weights_(m, seed=5)
        return StableVideoDiffusionPipeline(unet=m)
    m = pu.UNetSpatioTemporalConditionModel(unet_config()).half().to(dev)
    pu.init_synthetic_weights_(m, seed=5)
    cn = pc.ControlNetSDVModel(unet_config()).half().to(dev)
    pu.init_synthetic_weights_(cn, seed=6)
    return StableVideoDiffusionPipeline(unet=m, controlnet=cn)


def inputs(frames, cfg, clips=1):
    import torch
    g = torch.Generator().manual_seed(77)
    lat0 = torch.randn(1, frames, 4, 8, 8, generator=g)
    img = 0.18215 * torch.randn(1, 1, 4, 8, 8, generator=g).repeat(1, frames, 1, 1, 1)
    emb = torch.randn(1, 1, 1024, generator=g)
    if clips == 2:
        lat0 = torch.cat([lat0, 0.9 * lat0.flip(1)])
        img, emb = torch.cat([img, 0.8 * img]), torch.cat([emb, 0.8 * emb])
    if cfg:
        img = torch.cat([torch.zeros_like(img), img])
        emb = torch.cat([torch.zeros_like(emb), emb])
    ids = torch.tensor([[6.0, 127.0, 0.02]] * ((2 if cfg else 1) * clips))
    return lat0, img, emb, ids


def controlnet_extras(frames, cfg, clips):
    """condition [cfg * clips, F, 3, 64, 64] and the domain / flow features of the LKGD UNet"""
    import torch
    g = torch.Generator().manual_seed(78)
    ctrl = (2.0 * torch.rand(clips, frames, 3, 64, 64, generator=g) - 1.0).half()
    dom, flow = torch.randn(clips, 1, 1000, generator=g).half(), torch.randn(clips, 1, 1000, generator=g).half()
    n = 2 if cfg else 1
    return torch.cat([ctrl] * n), torch.cat([dom] * n), torch.cat([flow] * n)


def loop_args(pipe, dev, frames, cfg, steps, clips=1, fp32=False):
    import torch
    lat0, img, emb, ids = inputs(frames, cfg, clips)
    pipe.scheduler.set_timesteps(steps)
    lat = lat0 * float(pipe.scheduler.init_noise_sigma)
    lat = (lat if fp32 else lat.half()).to(dev)
    return (lat, img.half().to(dev), emb.half().to(dev), ids.to(dev), steps, 1.0, 3.0 if cfg else 1.0)


# ---- children -------------------------------------------------------------------------------------------------------------------
def child_single():
    import torch
    from lkgd_amd import ops
    dev = torch.device("cuda", 0)

    def run(case, frames, cfg, steps=3, clips=1, fp32=False, controlnet=False, setup=None, **kw):
        pipe = make_pipe(dev, controlnet)
        if setup is not None:
            setup(pipe)
        if controlnet:
            ctrl, dom, flow = controlnet_extras(frames, cfg, clips)
            kw.update(controlnet_condition=ctrl.to(dev), controlnet_cond_scale=0.8, domain_features=dom.to(dev),
                      flow_features=flow.to(dev))
        out = pipe.denoise(*loop_args(pipe, dev, frames, cfg, steps, clips, fp32), **kw)
        say(case, 0, sha(out))

    run("one_cfg_f4", 4, True)
    run("one_nocfg_f5", 5, False)
    run("one_start_step_callback", 4, True, start_step=1,
        callback_on_step_end=lambda p, i, t, kw: {"latents": kw["latents"].clone()})
    run("one_direct_fusion_b2_fp32", 4, True, clips=2, fp32=True, direct_fusion=True)
    run("one_controlnet", 4, True, controlnet=True)
    run("one_no_replay", 4, True, setup=lambda p: setattr(p, "use_replay", False))
    events = ops.GEMM_EVENTS = []
    run("one_events_7_steps", 4, True, steps=7)
    say("one_events_7_steps", 0, f"events {len(events)} same list {ops.GEMM_EVENTS is events}")
    ops.GEMM_EVENTS = None
    run("one_hip_graph", 4, True, setup=lambda p: setattr(p, "use_hip_graph", True))


def init_world(rank, world, port):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(4)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def child_svd(case, rank, world, port):
    import torch
    import torch.distributed as dist
    from lkgd_amd import ops
    from lkgd_amd.dist_run import DistDenoiser
    _, _, frames, cfg, clips, controlnet = [c for c in SVD_WORLDS if c[0] == case][0]
    init_world(rank, world, port)
    try:
        dev = torch.device("cuda", 0)
        pipe = make_pipe(dev, controlnet)
        runner = DistDenoiser(pipe, world, rank, frames, cfg=cfg)
        kw = {}
        if controlnet:
            ctrl, dom, flow = controlnet_extras(frames, cfg, clips)
            kw = dict(controlnet_condition=ctrl.to(dev), controlnet_cond_scale=0.8, domain_features=dom.to(dev),
                      flow_features=flow.to(dev))
        for replayed in (True, False):
            runner.use_replay = replayed
            out = runner.denoise(*loop_args(pipe, dev, frames, cfg, 3, clips), **kw)
            say(f"{case}_{'replay' if replayed else 'eager'}", rank, sha(out))
        if case == EVENTS_CASE:
            runner.use_replay = True
            events = ops.GEMM_EVENTS = []
            out = runner.denoise(*loop_args(pipe, dev, frames, cfg, 7, clips), **kw)
            say(f"{case}_events_7_steps", rank, sha(out))
            say(f"{case}_events_7_steps", rank, f"events {len(events)} same list {ops.GEMM_EVENTS is events}")
            ops.GEMM_EVENTS = None
    finally:
        dist.destroy_process_group()


def child_dit(case, rank, world, port):
    import torch
    import torch.distributed as dist
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import unet as pu
    from lkgd_amd.dist_run import DistDiTDenoiser
    init_world(rank, world, port)
    try:
        dev = torch.device("cuda", 0)
        cfg = pc.DiTConfig(num_attention_heads=2, in_channels=32, time_embed_dim=64, num_layers=2, sample_width=12,
                           sample_height=8, sample_frames=9, max_text_seq_length=16)
        m = pc.CogVideoXTransformer3DModel(cfg).half().to(dev)
        pu.init_synthetic_weights_(m, seed=4)
        g = torch.Generator().manual_seed(79)
        lat = torch.randn(1, 3, 16, 8, 12, generator=g).half()
        img = (0.5 * torch.randn(1, 3, 16, 8, 12, generator=g)).half()
        pe = torch.randn(2, 16, 4096, generator=g).half()
        dom, flow = torch.randn(1, 1, 1000, generator=g), torch.randn(1, 1, 1000, generator=g)
        runner = DistDiTDenoiser(m, pc.CogVideoXDDIMScheduler(), world, rank, 3, cfg=True)
        out = runner.denoise(lat.to(dev), img.to(dev), pe.to(dev), dom.to(dev), flow.to(dev), 3, 6.0, True)
        say(case, rank, sha(out))
    finally:
        dist.destroy_process_group()


def tiny_dit(dev, **over):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import unet as pu
    cfg = pc.DiTConfig(**{**dict(num_attention_heads=2, in_channels=32, time_embed_dim=64, num_layers=2, sample_width=12,
                                 sample_height=8, sample_frames=9, max_text_seq_length=16), **over})
    m = pc.CogVideoXTransformer3DModel(cfg).half().to(dev)
    pu.init_synthetic_weights_(m, seed=4)
    return m


class SamplePipeline:
    """what ``ddim_inversion.sample`` reads of a pipeline; the prompt embeddings are seeded noise ([1, 16, 4096] per prompt)"""
    vae_scale_factor_spatial = 8
    guidance_scale = property(lambda self: self._guidance_scale)

    def __init__(self, transformer, dev):
        self.transformer, self._execution_device = transformer, dev

    def encode_prompt(self, prompt, negative_prompt, do_classifier_free_guidance, device=None):
        import torch
        g = torch.Generator().manual_seed(81 + len(prompt or ""))
        pe, ne = (torch.randn(1, 16, 4096, generator=g).half().to(device) for _ in range(2))
        return pe, (ne if do_classifier_free_guidance else None)

    def _prepare_rotary_positional_embeddings(self, height, width, num_frames, device):
        from lkgd_amd import cogvideox as pc
        return pc.rotary_tables(self.transformer.config, num_frames, height // 16, width // 16)

    def maybe_free_model_hooks(self):
        pass


def child_dit_one():
    import torch
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ddim_inversion as di
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(79)
    lat = torch.randn(1, 3, 16, 8, 12, generator=g).half().to(dev)
    img = (0.5 * torch.randn(1, 3, 16, 8, 12, generator=g)).half().to(dev)
    pe = torch.randn(2, 16, 4096, generator=g).half().to(dev)
    dom, flow = torch.randn(1, 1, 1000, generator=g).to(dev), torch.randn(1, 1, 1000, generator=g).to(dev)
    ddim = pc.CogVideoXDDIMScheduler

    m = tiny_dit(dev)
    say("dit_one_ddim", 0, sha(pc.denoise(m, ddim(), lat, img, pe, dom, flow, 3, 6.0, True)))
    say("dit_one_dpm_seeded", 0, sha(pc.denoise(m, pc.CogVideoXDPMScheduler(), lat, img, pe, dom, flow, 4, 6.0, True,
                                                generator=torch.Generator().manual_seed(5))))
    say("dit_one_nocfg", 0, sha(pc.denoise(m, ddim(), lat, img, pe[1:], dom, flow, 3, 1.0, False)))
    seen = []
    out = pc.denoise(m, ddim(), lat, img, pe, dom, flow, 4, 6.0, True, start_step=1, callback=lambda i, t, x: seen.append((i, t, x)))
    say("dit_one_start_step_callback", 0, sha(out))
    say("dit_one_start_step_callback", 0, f"callback {[(i, t) for i, t, _ in seen]} {sha(torch.stack([x for _, _, x in seen]))}")
    say("dit_one_t2v", 0, sha(pc.denoise(tiny_dit(dev, in_channels=16), ddim(), lat, None, pe, None, None, 3, 6.0, True)))
    m15 = tiny_dit(dev, patch_size_t=2, use_rotary_positional_embeddings=True, ofs_embed_dim=64, patch_bias=False, sample_frames=13)
    lat15, img15 = pc.pad_for_temporal_patches(lat, img, 2)
    say("dit_one_v15_ofs", 0, sha(pc.denoise(m15, ddim(), lat15, img15, pe, dom, flow, 3, 6.0, True, ofs=2.0)))

    pipe = SamplePipeline(tiny_dit(dev, in_channels=16, use_rotary_positional_embeddings=True), dev)
    forward = ddim(snr_shift_scale=1.0)
    inverse = di.sample(pipe, lat, di.DDIMInverseScheduler(**forward.config), prompt="", num_inference_steps=3, guidance_scale=6.0)
    say("dit_sample_inverse", 0, sha(inverse))
    kw = dict(prompt="a cat", num_inference_steps=3, guidance_scale=6.0, use_dynamic_cfg=True)
    with di.OverrideAttnProcessors(pipe.transformer):
        guided = di.sample(pipe, img, forward, reference_latents=reversed(inverse), **kw)
    say("dit_sample_guided", 0, f"{sha(guided)} guidance_scale {pipe.guidance_scale!r}")
    say("dit_sample_references_no_override", 0, sha(di.sample(pipe, img, forward, reference_latents=reversed(inverse), **kw)))


# ---- parent: no GPU work of its own ---------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(case, world, seconds):
    """the ranks of one case as fresh processes, each under its own time limit; their lines, or exit at the first failure"""
    port = free_port()
    procs = [subprocess.Popen(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), case, str(r),
                               str(world), str(port)], stdout=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate()[0] for p in procs]
    codes = [p.returncode for p in procs]
    lines = sorted(l for o in outs for l in o.splitlines() if " rank " in l)
    print("\n".join(lines), flush=True)
    if any(codes):
        sys.exit(f"{case}: exit statuses {codes}; stopping here")


def main():
    launch("single", 1, 420)
    for c in SVD_WORLDS:
        launch(c[0], c[1], 300)
    for name, world in DIT_WORLDS:
        launch(name, world, 300)
    launch("dit_one", 1, 300)


if __name__ == "__main__":
    if len(sys.argv) == 1:
        main()
    else:
        case, rank, world, port = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
        if case == "single":
            child_single()
        elif case == "dit_one":
            child_dit_one()
        elif case.startswith("dit"):
            child_dit(case, rank, world, port)
        else:
            child_svd(case, rank, world, port)

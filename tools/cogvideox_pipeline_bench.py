#!/usr/bin/env python3
"""One ``CogVideoXImageToVideoPipeline.__call__`` (lkgd_amd/pipeline_cogvideox.py) at the real CogVideoX-2B geometry on one MI355X,
stage by stage, and its frames-out step against the forms it replaces.

    python tools/cogvideox_pipeline_bench.py [--generate-type {i2v,t2v,v2v}] [--steps 2] [--rounds 5] [--out FILE]

``--generate-type t2v`` / ``v2v`` (the other two branches of inference/cli_demo.py): one ``CogVideoXPipeline`` /
``CogVideoXVideoToVideoPipeline`` call at the 2B geometry (the stock 30-layer DiT, ``in_channels`` 16; v2v: a 49-frame 480 x 720 clip of
PIL frames, ``strength`` 0.8, so ``--steps`` 5 executes 4), milliseconds per stage, and for v2v ``preprocess_video`` alone: the GPU path
(one upload of the clip's uint8 frames + one ``lkgd_image_preprocess`` launch) against the host chain + the upload of its fp32 result
and the cast, PIL's resize included on both sides.  The result is merged into ``profiles/cogvideox_t2v_v2v_bench.json`` under its
generate type.  The default ``i2v`` is what it was:

Random weights at the released configurations (there is no checkpoint on a GPU box): the T5-v1.1-XXL encoder, the 30-layer I2V DiT
with the latent-knowledge fuse, the 3-D causal VAE with its encoder, two ViT-B/16-384.  One JSON line (also written to
``profiles/cogvideox_pipeline_bench.json``):
    * ``stages``: milliseconds of every stage of ONE call (49 frames, 480 x 720, a PIL image, guidance 6, ``output_type="pil"``) after one
      warm-up call, each stage bracketed by device synchronisation on the host clock: prompt (two T5 forwards), image in (lanczos on
      the host + ``lkgd_image_preprocess``), the two ViTs, image encode (``prepare_latents``), the loop, decode, frames out.  The loop
      runs ``--steps`` steps; ``loop_ms_scaled_to_50_steps`` is that time x 50 / steps - SCALED, not measured;
    * ``frames_out``: the frames-out step alone on a random [1, 3, 49, 480, 720] fp16 clip in its three modes, median of ``--rounds``
      alternations of (hip) the kernel + the copy of its result, (a) the ATen device chain + the copy of ITS result, (b) the host
      form ``tensor2vid`` runs on a CPU copy of the clip (the clip's own device -> host copy included, as a GPU pipeline pays it).
      Kernel-only time by device events around 20 back-to-back launches into one output tensor (a single launch is shorter than the
      host's way to it), with the bytes the mode moves and the rate that gives; the ATen chain the same way.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def _event_ms(fn, n=20):
    """device time of one ``fn()``: events around ``n`` back-to-back enqueues, so the queue never waits for the host between them"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


class _Stages:
    """wraps the stage entry points of one pipeline object: wall milliseconds between device synchronisations, per stage"""

    def __init__(self, pipe, cx):
        self.pipe, self.cx, self.ms = pipe, cx, {}

    def _wrap(self, name, fn):
        def timed(*a, **k):
            ms, r = _wall_ms(lambda: fn(*a, **k))
            self.ms[name] = self.ms.get(name, 0.0) + ms
            return r
        return timed

    def __enter__(self):
        p, vp = self.pipe, self.pipe.video_processor
        i2v = hasattr(p, "domain_model")
        self.saved = (p.domain_model, p.flow_model, self.cx.denoise) if i2v else (None, None, self.cx.denoise)
        p.encode_prompt = self._wrap("prompt", type(p).encode_prompt.__get__(p))
        vp.preprocess = self._wrap("image_in", type(vp).preprocess.__get__(vp))
        vp.preprocess_video = self._wrap("video_in", type(vp).preprocess_video.__get__(vp))
        if i2v:
            p.domain_model = self._wrap("vits", self.saved[0])
            p.flow_model = self._wrap("vits", self.saved[1])
        encode = "image_encode" if i2v else "video_encode" if "VideoToVideo" in type(p).__name__ else "noise"
        p.prepare_latents = self._wrap(encode, type(p).prepare_latents.__get__(p))
        self.cx.denoise = self._wrap("loop", self.saved[2])
        p.decode_latents = self._wrap("decode", type(p).decode_latents.__get__(p))
        vp.postprocess_video = self._wrap("frames_out", type(vp).postprocess_video.__get__(vp))
        self.ms.clear()
        return self

    def __exit__(self, *exc):
        p, vp = self.pipe, self.pipe.video_processor
        for obj, names in ((p, ("encode_prompt", "prepare_latents", "decode_latents")),
                           (vp, ("preprocess", "preprocess_video", "postprocess_video"))):
            for n in names:
                obj.__dict__.pop(n, None)
        if hasattr(p, "domain_model"):
            p.domain_model, p.flow_model = self.saved[:2]
        self.cx.denoise = self.saved[2]


def _build(dev, generate_type="i2v"):
    import cogvideox_vae_encoder_oracle as eo
    from t5_bench import _random_weights_
    from lkgd_amd import cogvideox as cx
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import t5, vit
    from lkgd_amd import unet as pu
    from lkgd_amd import pipeline_cogvideox as pp
    i2v = generate_type == "i2v"
    with torch.device("meta"):
        te = t5.T5EncoderModel(t5.T5Config())
        dit = cx.CogVideoXTransformer3DModel(cx.DiTConfig(in_channels=32 if i2v else 16))
        vits = [vit.vit_base_patch16_384() for _ in range(2 if i2v else 0)]
    te = te.to(torch.float16).to_empty(device=dev)
    _random_weights_(te, dev)
    te.invalidate()
    dit = dit.to(torch.float16).to_empty(device=dev)
    pu.init_synthetic_weights_(dit, seed=0)
    with torch.no_grad():
        for n, p in dit.named_parameters():          # adaLN modulation / gates small, as bench.py --cogvideox sets them
            if ".linear." in n and ("norm1" in n or "norm2" in n or "norm_out" in n):
                p.mul_(0.1)
    vits = [pu.init_synthetic_weights_(v.to(torch.float16).to_empty(device=dev), seed=5 + i) for i, v in enumerate(vits)]
    with torch.no_grad():
        for v in vits:                               # bare parameters: no module initialiser reaches them
            v.cls_token.normal_(0.0, 0.02)
            v.pos_embed.normal_(0.0, 0.02)
    cfg = eo.CogVAEConfig()
    torch.manual_seed(0)
    o = eo.AutoencoderKLCogVideoX(cfg)
    vae = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**cfg.__dict__), encoder=True)
    vae.load_state_dict(o.state_dict())
    vae = vae.half().to(dev)
    if i2v:
        return pp.CogVideoXImageToVideoPipeline(None, te, vae, dit, cx.CogVideoXDDIMScheduler(), vits[0], vits[1]), cx
    cls = pp.CogVideoXPipeline if generate_type == "t2v" else pp.CogVideoXVideoToVideoPipeline
    return cls(None, te, vae, dit, cx.CogVideoXDDIMScheduler()), cx


def _video_in(pipe, frames, rounds, dev):
    """``preprocess_video`` of 49 PIL frames to 480 x 720: the GPU path against the host chain + the upload and cast of its result"""
    vp = pipe.video_processor
    gpu, host = [], []
    for _ in range(rounds + 1):                                          # the first alternation is the warm-up
        gpu.append(_wall_ms(lambda: vp.preprocess_video(frames, 480, 720, device=dev, dtype=torch.float16))[0])
        host.append(_wall_ms(lambda: vp.preprocess_video(frames, 480, 720).to(device=dev, dtype=torch.float16))[0])
    a = vp.preprocess_video(frames, 480, 720, device=dev, dtype=torch.float16)
    b = vp.preprocess_video(frames, 480, 720).to(device=dev, dtype=torch.float16)
    return dict(clip=list(a.shape), bit_identical_to_host_chain=bool(torch.equal(a, b)), gpu_path_ms=round(statistics.median(gpu[1:]), 2),
                host_chain_plus_upload_ms=round(statistics.median(host[1:]), 2), gpu_path_ms_all=[round(x, 2) for x in gpu[1:]],
                host_chain_plus_upload_ms_all=[round(x, 2) for x in host[1:]],
                note="both sides include PIL's lanczos resize of the 49 frames (512 x 768 -> 480 x 720) on the host")


def _stock_call(args, dev):
    """``--generate-type t2v`` / ``v2v``"""
    import PIL.Image
    kind = args.generate_type
    pipe, cx = _build(dev, kind)
    res = dict(tool="cogvideox_pipeline_bench", generate_type=kind, device=torch.cuda.get_device_name(0), rounds=args.rounds)
    ids = torch.randint(2, 32000, (1, 226), generator=torch.Generator().manual_seed(1))
    neg = torch.zeros(1, 226, dtype=torch.int64)
    neg[0, 0] = 1
    common = dict(num_inference_steps=args.steps, guidance_scale=6.0, use_dynamic_cfg=True, output_type="pil")
    if kind == "t2v":
        def call():
            return pipe(ids, neg, height=480, width=720, num_frames=49, generator=torch.Generator().manual_seed(7), **common).frames
        executed = args.steps
    else:
        rng = np.random.default_rng(4)
        video = [PIL.Image.fromarray(rng.integers(0, 256, (512, 768, 3), dtype=np.uint8)) for _ in range(49)]
        res["preprocess_video"] = _video_in(pipe, video, args.rounds, dev)
        print(json.dumps({"preprocess_video": res["preprocess_video"]}), flush=True)

        def call():
            return pipe(video, ids, neg, height=480, width=720, strength=0.8, generator=torch.Generator().manual_seed(7), **common).frames
        executed = min(int(args.steps * 0.8), args.steps)
    warm_ms, frames = _wall_ms(call)
    with _Stages(pipe, cx) as st:
        total_ms, frames = _wall_ms(call)
    stages = {k: round(v, 2) for k, v in st.ms.items()}
    res["call"] = dict(frames=[len(frames), len(frames[0]), frames[0][0].size[1], frames[0][0].size[0]], steps=args.steps,
                       executed_steps=executed, warmup_call_ms=round(warm_ms, 1), call_ms=round(total_ms, 1), stages_ms=stages,
                       stages_sum_ms=round(sum(stages.values()), 1), loop_ms_per_step=round(stages["loop"] / executed, 2))
    print(json.dumps(res))
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            merged = json.load(fh)
    merged[kind] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(merged) + "\n")


def _frames_out(rounds, dev):
    import PIL.Image
    from lkgd_amd import ops
    from lkgd_amd.image_processor import VaeImageProcessor, tensor2vid
    B, C_, T, H, W = 1, 3, 49, 480, 720
    clip = (0.7 * torch.randn(B, C_, T, H, W, generator=torch.Generator().manual_seed(2))).half().to(dev)
    n = clip.numel()
    host = VaeImageProcessor(vae_scale_factor=8)

    def aten(mode):
        d = (clip / 2 + 0.5).clamp(0, 1)
        if mode == "pt":
            return d.permute(0, 2, 1, 3, 4).contiguous()
        f = d.permute(0, 2, 3, 4, 1).float()
        return f.contiguous() if mode == "np" else (f * 255).round().to(torch.uint8)

    forms = {
        "pil": (ops.VIDEO_U8, 1, lambda t: [[PIL.Image.fromarray(f) for f in c] for c in t.cpu().numpy()]),
        "np": (ops.VIDEO_F32, 4, lambda t: t.cpu().numpy()),
        "pt": (ops.VIDEO_F16, 2, lambda t: t),                          # stays on the device, as diffusers' "pt" does
    }
    out = {"clip": [B, C_, T, H, W]}
    for mode, (code, osize, finish) in forms.items():
        dst = ops.video_postprocess(clip, code)
        same = bool(torch.equal(dst, aten(mode)))
        hip, a, b, kern, akern = [], [], [], [], []
        for _ in range(rounds + 1):                                      # the first alternation is the warm-up
            kern.append(_event_ms(lambda: ops.video_postprocess(clip, code, out=dst)))
            akern.append(_event_ms(lambda: aten(mode)))
            hip.append(_wall_ms(lambda: finish(ops.video_postprocess(clip, code)))[0])
            a.append(_wall_ms(lambda: finish(aten(mode)))[0])
            b.append(_wall_ms(lambda: tensor2vid(clip.cpu(), host, mode))[0])
        med = lambda v: round(statistics.median(v[1:]), 4)               # noqa: E731
        nbytes = n * (2 + osize)
        out[mode] = dict(bit_identical_to_aten=same, kernel_ms=med(kern), kernel_mbytes=round(nbytes / 1e6, 1),
                         kernel_gbytes_per_s=round(nbytes / med(kern) / 1e6, 1), aten_device_chain_ms=med(akern),
                         aten_device_chain_gbytes_per_s_same_bytes=round(nbytes / med(akern) / 1e6, 1),
                         hip_with_copy_ms=med(hip), aten_with_copy_ms=med(a), host_tensor2vid_ms=med(b),
                         hip_with_copy_ms_all=[round(x, 2) for x in hip[1:]], aten_with_copy_ms_all=[round(x, 2) for x in a[1:]],
                         host_tensor2vid_ms_all=[round(x, 2) for x in b[1:]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2, help="loop steps of the measured call (the 50-step figure is scaled from it)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--generate-type", choices=("i2v", "t2v", "v2v"), default="i2v",
                    help="the pipeline class, named as inference/cli_demo.py names it (default i2v: unchanged)")
    ap.add_argument("--out", default=None, help="default profiles/cogvideox_pipeline_bench.json (i2v) or "
                                                "profiles/cogvideox_t2v_v2v_bench.json (t2v / v2v, merged under the generate type)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "cogvideox_pipeline_bench.json" if args.generate_type == "i2v"
                                else "cogvideox_t2v_v2v_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("cogvideox_pipeline_bench measures on the MI355X: no GPU found")
    import PIL.Image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.generate_type != "i2v":
        return _stock_call(args, dev)
    res = dict(tool="cogvideox_pipeline_bench", device=torch.cuda.get_device_name(0), rounds=args.rounds)
    res["frames_out"] = _frames_out(args.rounds, dev)
    print(json.dumps({"frames_out": res["frames_out"]}), flush=True)

    pipe, cx = _build(dev)
    rng = np.random.default_rng(4)
    image = PIL.Image.fromarray(rng.integers(0, 256, (512, 768, 3), dtype=np.uint8))
    ids = torch.randint(2, 32000, (1, 226), generator=torch.Generator().manual_seed(1))
    neg = torch.zeros(1, 226, dtype=torch.int64)
    neg[0, 0] = 1

    def call():
        return pipe(image, ids, neg, num_frames=49, num_inference_steps=args.steps, guidance_scale=6.0, use_dynamic_cfg=True,
                    generator=torch.Generator().manual_seed(7), output_type="pil").frames
    warm_ms, frames = _wall_ms(call)
    with _Stages(pipe, cx) as st:
        total_ms, frames = _wall_ms(call)
    stages = {k: round(v, 2) for k, v in st.ms.items()}
    res["call"] = dict(frames=[len(frames), len(frames[0]), frames[0][0].size[1], frames[0][0].size[0]], steps=args.steps,
                       warmup_call_ms=round(warm_ms, 1), call_ms=round(total_ms, 1), stages_ms=stages,
                       stages_sum_ms=round(sum(stages.values()), 1), loop_ms_per_step=round(stages["loop"] / args.steps, 2),
                       loop_ms_scaled_to_50_steps=round(stages["loop"] * 50 / args.steps, 1),
                       note="loop_ms_scaled_to_50_steps is SCALED from the measured steps, not measured; the once-per-clip part "
                            "of the loop (the fuse, the ofs / rotary tables) is scaled with it")
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()

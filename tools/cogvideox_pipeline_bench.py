#!/usr/bin/env python3
"""One ``CogVideoXImageToVideoPipeline.__call__`` (lkgd_amd/pipeline_cogvideox.py) at the real CogVideoX-2B geometry on one MI355X,
stage by stage, and its frames-out step against the forms it replaces.

    python tools/cogvideox_pipeline_bench.py [--steps 2] [--rounds 5] [--out FILE]

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
        self.saved = (p.domain_model, p.flow_model, self.cx.denoise)
        p.encode_prompt = self._wrap("prompt", type(p).encode_prompt.__get__(p))
        vp.preprocess = self._wrap("image_in", type(vp).preprocess.__get__(vp))
        p.domain_model = self._wrap("vits", self.saved[0])
        p.flow_model = self._wrap("vits", self.saved[1])
        p.prepare_latents = self._wrap("image_encode", type(p).prepare_latents.__get__(p))
        self.cx.denoise = self._wrap("loop", self.saved[2])
        p.decode_latents = self._wrap("decode", type(p).decode_latents.__get__(p))
        vp.postprocess_video = self._wrap("frames_out", type(vp).postprocess_video.__get__(vp))
        self.ms.clear()
        return self

    def __exit__(self, *exc):
        p, vp = self.pipe, self.pipe.video_processor
        for obj, names in ((p, ("encode_prompt", "prepare_latents", "decode_latents")), (vp, ("preprocess", "postprocess_video"))):
            for n in names:
                obj.__dict__.pop(n, None)
        p.domain_model, p.flow_model, self.cx.denoise = self.saved


def _build(dev):
    import cogvideox_vae_encoder_oracle as eo
    from t5_bench import _random_weights_
    from lkgd_amd import cogvideox as cx
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import t5, vit
    from lkgd_amd import unet as pu
    from lkgd_amd.pipeline_cogvideox import CogVideoXImageToVideoPipeline
    with torch.device("meta"):
        te = t5.T5EncoderModel(t5.T5Config())
        dit = cx.CogVideoXTransformer3DModel(cx.DiTConfig(in_channels=32))
        vits = [vit.vit_base_patch16_384() for _ in range(2)]
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
    return CogVideoXImageToVideoPipeline(None, te, vae, dit, cx.CogVideoXDDIMScheduler(), vits[0], vits[1]), cx


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cogvideox_pipeline_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cogvideox_pipeline_bench measures on the MI355X: no GPU found")
    import PIL.Image
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
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

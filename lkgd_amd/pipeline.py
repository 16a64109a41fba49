"""StableVideoDiffusionPipeline with the reference's ``__call__`` signature; the denoising loop runs on the HIP path.

Mirrors /root/reference/pipeline/pipeline_stable_video_diffusion_trans.py: ``__call__`` :352-656 (signature :352-372,
loop :545-640), ``_encode_image`` :157-203, ``_encode_vae_image`` :205-226, ``_get_add_time_ids`` :228-254,
``decode_latents`` :256-283, ``prepare_latents`` :299-331, ``check_inputs`` :285-297.

Scope: the hot path is the loop body.  ``denoise()`` is that loop: per step ONE glue kernel
(CFG duplicate + scale_model_input + channel concat -> channels-last tokens), the UNet forward on tokens, ONE glue
kernel (per-frame CFG + v-prediction + Euler update).  No host<->device sync inside the loop (sigma tables live on the
host).  CLIP / VAE are boundary stages: any modules with the diffusers interface may be passed in and are called as the
reference calls them; they are not re-implemented here (8f rank 2).
The LKGD conditioning (domain / flow ViT logits) is passed as ``domain_features`` / ``flow_features`` (intended wiring:
CogVideo-main/finetune/models/cogvideox_i2v/pipeline_cogvideox_image2video.py:794-799,849-859) and fused ONCE per clip.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Union

import numpy as np
import torch

from . import ops
from . import replay as _replay
from . import trace as _trace
from ._lib import LkgdHipError
from .image_ops import resize_with_antialiasing
from .image_processor import VaeImageProcessor, tensor2vid
from .scheduler import EulerDiscreteScheduler


@dataclass
class StableVideoDiffusionPipelineOutput:
    frames: Union[torch.Tensor, list]


def _randn_tensor(shape, generator, device, dtype):
    """diffusers' `randn_tensor` [EXT utils/torch_utils.py]: a CPU generator serves a GPU target by sampling on the CPU (so
    seeds reproduce across devices); a list of generators samples per batch entry"""
    if isinstance(generator, (list, tuple)):
        if len(generator) == 1:
            generator = generator[0]
        else:
            per = (1,) + tuple(shape[1:])
            return torch.cat([_randn_tensor(per, g, device, dtype) for g in generator], dim=0)
    gdev = generator.device if isinstance(generator, torch.Generator) else torch.device(device)
    if gdev.type != torch.device(device).type and gdev.type == "cpu":
        return torch.randn(tuple(shape), generator=generator, device="cpu", dtype=dtype).to(device)
    return torch.randn(tuple(shape), generator=generator, device=device, dtype=dtype)


def _append_dims(x, target_dims):
    dims_to_append = target_dims - x.ndim
    if dims_to_append < 0:
        raise ValueError(f"input has {x.ndim} dims but target_dims is {target_dims}, which is less")
    return x[(...,) + (None,) * dims_to_append]


def smooth_chunks(total_frames: int, num_frames: int, rng=np.random):
    """the frame windows of one Euler step of the smoothing pipeline, as (f0, L) pairs: ``get_chunks`` of
    pipeline_stable_video_diffusion_smooth.py:526-533 restated.  The first window has a random length of 1..num_frames, the
    others ``num_frames`` frames and the last one the remainder.  One ``rng.randint(0, num_frames)`` is drawn per call, as the
    reference draws it, so seeding ``np.random`` reproduces its windows."""
    if total_frames <= 0 or num_frames <= 0:
        raise ValueError(f"smooth_chunks needs positive frame counts, got {total_frames} and {num_frames}")
    first = min(int(rng.randint(0, num_frames)) + 1, total_frames)
    chunks, f0 = [(0, first)], first
    while f0 < total_frames:
        n = min(num_frames, total_frames - f0)
        chunks.append((f0, n))
        f0 += n
    return chunks


class Placement:
    """What ``denoise`` asks about the process it runs in.  The default: one process holds every batch entry and frame; a rank of a
    sharded run (lkgd_amd/dist_run.py) answers for its CFG half and frame slice.  ``owner`` (the pipeline; there the rank's runner)
    says whether the forward is replayed and holds its arenas."""
    shard = None             # handed to ``forward_tokens``
    samples_events = None    # f(i): does Euler step i sample ops.GEMM_EVENTS; None: every step, the global is left alone

    def __init__(self, owner):
        self.arenas, self.use_replay = owner._arenas, owner.use_replay

    def slice(self, cfg: int, B: int, F: int):
        """(b_local, e0, fl, f0): batch entries [e0, e0 + b_local) of the cfg * B, frames [f0, f0 + fl) of each of them"""
        return cfg * B, 0, F, 0

    def token_rows(self, tok: torch.Tensor, F: int, HW: int, b_local: int, e0: int, fl: int, f0: int):
        """(rows, refresh): this process's rows (entry, frame, pixel) of the static token buffer - a view of ``tok`` where they are
        contiguous in it (refresh None), else a buffer of their own that ``refresh()`` fills from ``tok``"""
        if fl == F:
            return tok[e0 * F * HW:(e0 + b_local) * F * HW], None
        if b_local == 1:
            r0 = (e0 * F + f0) * HW
            return tok[r0:r0 + fl * HW], None
        rows = torch.empty(b_local * fl * HW, 8, dtype=tok.dtype, device=tok.device)
        dst, src = rows.reshape(b_local, fl, HW, 8), tok.reshape(-1, F, HW, 8)[e0:e0 + b_local, f0:f0 + fl]
        return rows, lambda: dst.copy_(src)

    def noise_gather(self, b_local: int, HW: int, device):
        """f(noise tokens of this process) -> the noise tokens [cfg*B*F*HW, 4] of the whole clip; None: they are the same"""
        return None


class StableVideoDiffusionPipeline:
    model_cpu_offload_seq = "image_encoder->unet->vae"
    _callback_tensor_inputs = ["latents"]

    def __init__(self, vae=None, image_encoder=None, unet=None, scheduler: Optional[EulerDiscreteScheduler] = None,
                 feature_extractor=None, controlnet=None):
        self.vae, self.image_encoder, self.unet = vae, image_encoder, unet
        #: optional lkgd_amd.controlnet.ControlNetSDVModel (reference pipeline_stable_video_diffusion_controlnet.py:156-178)
        self.controlnet = controlnet
        self.scheduler = scheduler if scheduler is not None else EulerDiscreteScheduler.from_svd_config()
        self.feature_extractor = feature_extractor
        self.vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1) if vae is not None else 8
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor)       # reference :150
        self._guidance_scale = None
        self._num_timesteps = 0
        #: replay the per-step UNet forward from a captured HIP graph (one launch instead of ~1000): the forward is
        #: shape-static across the Euler steps, only the timestep scalar and the input tokens change (static buffers)
        self.use_hip_graph = False   # opt-in: eager launches are already hidden behind GPU work on one GPU, and bench.py times
                                     # individual GEMM launches with events, which a graph replay cannot expose
        self._graph = None
        #: replay the step's forward from a recorded launch list (denoise(); LKGD_NO_REPLAY=1 = walk the modules every step)
        self.use_replay = __import__("os").environ.get("LKGD_NO_REPLAY", "0") != "1"
        #: private allocator pools the recorded forwards allocate from (lkgd_amd/replay.py): the plan's working set is the eager
        #: peak of one forward, and the blocks stay cached here between calls; ``release_arena()`` returns them to the driver
        self._arenas = _replay.ArenaSet()

    # ---- loading (DiffusionPipeline.from_pretrained [EXT]; call sites run_models/run_inference_svd.py:166-168,
    #      utils/util.py:536) --------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, torch_dtype=torch.float16, variant: Optional[str] = None,
                        unet=None, vae=None, image_encoder=None, feature_extractor=None, scheduler=None, controlnet=None,
                        unet_class=None, device: Optional[str] = "cuda", **_ignored):
        """a local diffusers pipeline directory (``unet/ vae/ image_encoder/ feature_extractor/ scheduler/``).  The UNet,
        the VAE, the scheduler and the CLIP image encoder (`image_encoder/` -> lkgd_amd.clip, transformers' parameter names;
        `feature_extractor/` -> its mean / std normalisation) are lkgd_amd's own classes: no diffusers, no transformers.  Components passed
        as keywords are used as given (``unet=...`` as utils/util.py:607-616 does).  hub / offload keywords are accepted
        and ignored (``low_cpu_mem_usage``, ``device_map``, ``local_files_only`` ...)."""
        import os
        from .unet import UNetSpatioTemporalConditionControlNetModel
        from .vae import AutoencoderKLTemporalDecoder
        root = pretrained_model_name_or_path
        if not os.path.isdir(root):
            raise OSError(f"{root} is not a local pipeline directory (there is no hub access)")

        def has(sub, f):
            return os.path.exists(os.path.join(root, sub, f))
        if unet is None:
            unet = (unet_class or UNetSpatioTemporalConditionControlNetModel).from_pretrained(
                root, subfolder="unet", torch_dtype=torch_dtype, variant=variant)
        if vae is None and has("vae", "config.json"):
            vae = AutoencoderKLTemporalDecoder.from_pretrained(root, subfolder="vae", torch_dtype=torch_dtype, variant=variant)
        if scheduler is None and has("scheduler", "scheduler_config.json"):
            scheduler = EulerDiscreteScheduler.from_pretrained(root, subfolder="scheduler")
        if image_encoder is None and has("image_encoder", "config.json"):
            from .clip import CLIPVisionModelWithProjection          # transformers' class name and checkpoint layout, HIP forward
            image_encoder = CLIPVisionModelWithProjection.from_pretrained(root, subfolder="image_encoder",
                                                                          torch_dtype=torch_dtype, variant=variant)
        if feature_extractor is None and has("feature_extractor", "preprocessor_config.json"):
            from .clip import CLIPImageProcessor
            feature_extractor = CLIPImageProcessor.from_pretrained(root, subfolder="feature_extractor")
        pipe = cls(vae=vae, image_encoder=image_encoder, unet=unet, scheduler=scheduler,
                   feature_extractor=feature_extractor, controlnet=controlnet)
        return pipe.to(device) if device is not None else pipe

    def to(self, device=None, dtype=None):
        """``DiffusionPipeline.to`` [EXT]: every module component to the device (the HIP models run on cuda only)"""
        for name in ("unet", "vae", "image_encoder", "controlnet"):
            m = getattr(self, name, None)
            if m is not None and hasattr(m, "to"):
                m = m.to(device=device, dtype=dtype) if dtype is not None else m.to(device)
                setattr(self, name, m)
        return self

    def save_pretrained(self, save_directory: str, **kw):
        import json
        import os
        os.makedirs(save_directory, exist_ok=True)
        index = {"_class_name": "StableVideoDiffusionPipeline", "_lkgd_amd": True}
        for name in ("unet", "vae", "image_encoder", "feature_extractor", "scheduler"):
            m = getattr(self, name, None)
            if m is not None and hasattr(m, "save_pretrained"):
                m.save_pretrained(os.path.join(save_directory, name))
                index[name] = [type(m).__module__.split(".")[0], type(m).__name__]
        with open(os.path.join(save_directory, "model_index.json"), "w") as f:
            json.dump(index, f, indent=2)

    # ---- reference helpers -------------------------------------------------------------------------------------
    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        if isinstance(self.guidance_scale, (int, float)):
            return self.guidance_scale > 1
        return self.guidance_scale.max() > 1

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def _execution_device(self):
        return self.unet.device

    def enable_model_cpu_offload(self, *a, **k):
        return None   # a memory knob of the reference (run_inference_svd.py:171); nothing to offload at 288 GB

    def check_inputs(self, image, height, width):
        import PIL.Image
        if not isinstance(image, (torch.Tensor, PIL.Image.Image, list)):
            raise ValueError("`image` has to be of type `torch.FloatTensor` or `PIL.Image.Image` or "
                             f"`List[PIL.Image.Image]` but is {type(image)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")

    def _get_add_time_ids(self, fps, motion_bucket_id, noise_aug_strength, dtype, batch_size, num_videos_per_prompt,
                          do_classifier_free_guidance):
        add_time_ids = [fps, motion_bucket_id, noise_aug_strength]
        passed = self.unet.config.addition_time_embed_dim * len(add_time_ids)
        expected = self.unet.add_embedding.linear_1.in_features
        if expected != passed:
            raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of "
                             f"{passed} was created. The model has an incorrect config.")
        ids = torch.tensor([add_time_ids], dtype=dtype).repeat(batch_size * num_videos_per_prompt, 1)
        if do_classifier_free_guidance:
            ids = torch.cat([ids, ids])
        return ids

    def prepare_latents(self, batch_size, num_frames, num_channels_latents, height, width, dtype, device, generator,
                        latents=None):
        shape = (batch_size, num_frames, num_channels_latents // 2, height // self.vae_scale_factor,
                 width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an "
                             f"effective batch size of {batch_size}.")
        if latents is None:
            latents = _randn_tensor(shape, generator, device, dtype)
        else:
            latents = latents.to(device=device, dtype=dtype)
        return ops.scale(latents, float(self.scheduler.init_noise_sigma))

    def _encode_image(self, image, device, num_videos_per_prompt, do_classifier_free_guidance):
        """boundary stage (CLIP), reference :157-203; the image encoder itself is the caller's module"""
        if self.image_encoder is None:
            raise LkgdHipError("no image_encoder given: pass `image_embeddings=` to __call__ or call denoise()")
        if not isinstance(image, torch.Tensor):
            # reference :166-175: PIL -> [0,1] tensor, normalise, anti-aliased resize to CLIP's 224x224, un-normalise
            image = self.image_processor.numpy_to_pt(self.image_processor.pil_to_numpy(image))
            image = image * 2.0 - 1.0
            image = resize_with_antialiasing(image, (224, 224))
            image = (image + 1.0) / 2.0
        dtype = next(self.image_encoder.parameters()).dtype
        image = self.feature_extractor(images=image, do_normalize=True, do_center_crop=False, do_resize=False,
                                       do_rescale=False, return_tensors="pt").pixel_values
        emb = self.image_encoder(image.to(device=device, dtype=dtype)).image_embeds.unsqueeze(1)
        bs, seq, _ = emb.shape
        emb = emb.repeat(1, num_videos_per_prompt, 1).view(bs * num_videos_per_prompt, seq, -1)
        if do_classifier_free_guidance:
            emb = torch.cat([torch.zeros_like(emb), emb])
        return emb

    def _encode_vae_image(self, image, device, num_videos_per_prompt, do_classifier_free_guidance):
        if self.vae is None:
            raise LkgdHipError("no vae given: pass `image_latents=` to __call__ or call denoise()")
        lat = self.vae.encode(image.to(device=device)).latent_dist.mode()
        if do_classifier_free_guidance:
            lat = torch.cat([torch.zeros_like(lat), lat])
        return lat.repeat(num_videos_per_prompt, 1, 1, 1)

    def _encode_vae_boundary(self, img, device, num_videos_per_prompt, do_classifier_free_guidance, dtype, chunk=None):
        """the VAE encode of ``__call__`` with what the reference wraps around it; ``chunk``: encode in slices of that many images
        (pipeline_stable_video_diffusion_smooth.py:458-464)"""
        # reference :470-484: an fp16 VAE with `force_upcast` encodes in fp32 and is cast back right after (so the
        # decode at the end runs in fp16 again, :643-645).  The HIP VAE computes fp16 activations with fp32 accumulation
        # whatever the module dtype says (lkgd_amd/vae.py), so casting it there and back would only re-pack its weights
        # twice per call: the module is left alone, and what the upcast protects against - an fp16 overflow in the
        # encoder - is checked instead (deviations)
        vae_dtype = getattr(self.vae, "dtype", None)
        from .vae import AutoencoderKLTemporalDecoder
        hip_vae = isinstance(self.vae, AutoencoderKLTemporalDecoder)
        needs_upcasting = (not hip_vae and vae_dtype == torch.float16 and
                           bool(getattr(self.vae.config, "force_upcast", False)))
        if needs_upcasting:
            self.vae.to(dtype=torch.float32)
        elif vae_dtype is not None and vae_dtype != img.dtype:
            img = img.to(vae_dtype)
        if chunk is None:
            image_latents = self._encode_vae_image(img, device, num_videos_per_prompt, do_classifier_free_guidance)
        else:
            image_latents = torch.cat([self._encode_vae_image(img[i:i + chunk], device, num_videos_per_prompt,
                                                              do_classifier_free_guidance)
                                       for i in range(0, img.shape[0], chunk)], dim=0)
        image_latents = image_latents.to(dtype)                                                   # reference :480
        if needs_upcasting:
            self.vae.to(dtype=torch.float16)
        if hip_vae and not bool(torch.isfinite(image_latents).all()):
            raise LkgdHipError("VAE encode produced non-finite latents (fp16 range exceeded in the encoder): the reference "
                               "encodes in fp32 under force_upcast; scale the input or encode outside and pass image_latents")
        return image_latents

    def decode_latents(self, latents, num_frames, decode_chunk_size=14):
        if self.vae is None:
            raise LkgdHipError("no vae given: use output_type='latent'")
        latents = latents.flatten(0, 1)
        latents = 1 / self.vae.config.scaling_factor * latents
        frames = []
        for i in range(0, latents.shape[0], decode_chunk_size):
            n_in = latents[i:i + decode_chunk_size].shape[0]
            frames.append(self.vae.decode(latents[i:i + decode_chunk_size], num_frames=n_in).sample)
        frames = torch.cat(frames, dim=0)
        frames = frames.reshape(-1, num_frames, *frames.shape[1:]).permute(0, 2, 1, 3, 4)
        return frames.float()

    # ---- the hot path ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def denoise(self, latents: torch.Tensor, image_latents: torch.Tensor, image_embeddings: torch.Tensor,
                added_time_ids: torch.Tensor, num_inference_steps: int = 25, min_guidance_scale: float = 1.0,
                max_guidance_scale: float = 3.0, domain_features: Optional[torch.Tensor] = None,
                flow_features: Optional[torch.Tensor] = None, callback_on_step_end: Optional[Callable] = None,
                callback_on_step_end_tensor_inputs: List[str] = ["latents"],
                controlnet_condition: Optional[torch.Tensor] = None, controlnet_cond_scale: float = 1.0,
                start_step: int = 0, direct_fusion: bool = False, controlnet_scale: float = 1.0,
                _placement: Optional[Placement] = None) -> torch.Tensor:
        """Reference loop :503-640.  ``latents`` [B,F,4,h,w] already scaled by init_noise_sigma (fp16 or fp32, updated
        in place and returned); ``image_latents`` [cfg*B,F,4,h,w] fp16; ``image_embeddings`` [cfg*B,1,1024].
        ``controlnet_condition`` [cfg*B,F,3,8h,8w] (already preprocessed and duplicated for CFG) runs ``self.controlnet``
        before the UNet every step and feeds its residuals in (pipeline_stable_video_diffusion_controlnet.py:582-607).
        pipeline_stable_video_diffusion_trans_controlnet.py adds (defaults = the loop above): ``start_step`` skips the first
        Euler steps and their callbacks (:571-574); ``controlnet_scale`` multiplies every residual on top of
        ``controlnet_cond_scale`` (:594-598), folded into the zero-convolution epilogue; ``direct_fusion`` switches the joint
        hooks off (:568) and fuses clip b with the frame-reversed clip b + B/2 through their x0 once per step (:637-667,
        lkgd_cfg_fusion_euler_step).
        ``_placement`` (private; lkgd_amd.dist_run.DistDenoiser passes its rank's): the loop of a sharded run is this one - the
        rank feeds the forward its batch entries and frames of the replicated token buffer, the noise prediction is gathered
        over the ranks and the update is replicated.  All tensor arguments are still those of the WHOLE clip."""
        unet, sch = self.unet, self.scheduler
        dev = unet.device
        B, F, _, H, W = latents.shape
        HW = H * W
        cfg = 2 if max_guidance_scale > 1 else 1
        place = _placement if _placement is not None else Placement(self)
        b_local, e0, fl, f0 = place.slice(cfg, B, F)
        if image_latents.shape[0] != cfg * B or image_embeddings.shape[0] != cfg * B:
            raise ValueError("image_latents / image_embeddings must carry cfg*batch entries (uncond first)")
        if direct_fusion and B % 2:
            raise ValueError(f"direct_fusion pairs clip b with clip b + B/2: the clip count must be even, got {B}")
        latents = latents.to(dev).contiguous()
        image_latents = image_latents.to(device=dev, dtype=torch.float16).contiguous()
        guidance = torch.linspace(min_guidance_scale, max_guidance_scale, F, dtype=torch.float32)
        self._guidance_scale = _append_dims(guidance.unsqueeze(0).repeat(B, 1), latents.ndim)
        guidance_dev = guidance.to(dev)
        enc = image_embeddings.to(dev)
        if domain_features is not None:
            if not hasattr(unet, "fused_embedding"):
                raise LkgdHipError("domain/flow features need the LKGD UNet (UNetSpatioTemporalConditionModel)")
            enc = unet.fused_embedding(enc, domain_features.to(dev), flow_features.to(dev))   # once per clip
        ids = added_time_ids.to(dev)
        vpred = sch.config.prediction_type == "v_prediction"
        from . import patch as _patch
        _patch.set_joint_attention(unet, enable=not direct_fusion)     # reference :555 / trans_controlnet :568 (no-op unless
                                                                       # the model is patched)
        # trans_controlnet :660: torch.linspace(1, 0, F) in fp32, made once per clip on the host and copied to the device
        fusion_w = torch.linspace(1, 0, F, dtype=torch.float32).to(dev) if direct_fusion else None
        ctrl_scale = float(controlnet_cond_scale) * float(controlnet_scale)    # both scale accumulator and bias (s_acc)
        ctrl = None
        if controlnet_condition is not None:
            if self.controlnet is None:
                raise LkgdHipError("controlnet_condition given but the pipeline has no controlnet")
            if controlnet_condition.shape[0] != cfg * B or controlnet_condition.shape[1] != F:
                raise ValueError("controlnet_condition must be [cfg * batch, frames, 3, 8h, 8w] (uncond entries first)")
            # this process's entries and frames; the whole tensor stays the caller's object, by which the ControlNet's cache knows it
            ctrl = controlnet_condition if (b_local, fl) == (cfg * B, F) else controlnet_condition[e0:e0 + b_local, f0:f0 + fl]
            ctrl = ctrl.to(device=dev, dtype=torch.float16).contiguous()
        one_process = _placement is None           # the HIP graph is a one-process path
        graph = self._graphed_forward(cfg * B, F, H, W, enc, ids) if (self.use_hip_graph and ctrl is None and one_process) else None
        forward_static = gather = sampled = None
        if graph is None:
            # step-invariant addresses for everything the forward reads, so its launch list can be replayed.  The token buffer
            # holds the whole clip (every process prepares it from its replicated latents); the forward reads this process's rows
            tok_buf = torch.empty(cfg * B * F * HW, 8, dtype=torch.float16, device=dev)
            tok_rows, refresh_rows = place.token_rows(tok_buf, F, HW, b_local, e0, fl, f0)
            t_dev = torch.zeros(b_local, dtype=torch.float32, device=dev)
            enc_r, ids_r = enc.to(torch.float16).contiguous(), ids[e0:e0 + b_local].to(torch.float32).contiguous()
            gather, sampled = place.noise_gather(b_local, HW, dev), place.samples_events
            if ctrl is not None:
                self.controlnet.prepare()
                self.controlnet._cond_tokens(ctrl, b_local, fl, H, W)      # once per clip, outside the recorded forward

            def forward_static():      # residuals stay channels-last token matrices between the two models
                down = mid = None
                if ctrl is not None:
                    down, mid, _ = self.controlnet.forward_tokens(tok_rows, b_local, fl, H, W, t_dev, enc_r, ids_r, ctrl,
                                                                  ctrl_scale, shard=place.shard)
                return unet.forward_tokens(tok_rows, b_local, fl, H, W, t_dev, enc_r, ids_r, down, mid, shard=place.shard)[0]
        # The step's forward is shape-static over the Euler steps: the first step runs for real and is RECORDED as a flat list of
        # C-ABI launches (lkgd_amd/replay.py), the other 24 replay it between in-place updates of its inputs (token buffer,
        # timestep) - bit-identical, and the Python module walk (64 ms of host time per forward against 90 ms of device time)
        # stops leaving the queue dry at the 18x32 / 9x16 levels: +1.1 % frames/s on one GPU (profiles/r05_bench_pair_replay.txt).
        # LKGD_NO_REPLAY=1 walks the modules every step, on the same static inputs.
        events_all = ops.GEMM_EVENTS
        try:
            with _replay.Replayed(place.arenas, dev, lambda: (b_local, fl, H, W, ctrl is not None, id(unet._pk)), forward_static,
                                  enabled=place.use_replay) as forward:
                def step(i, latents, t, sigma, sigma_next):
                    if graph is not None:
                        ops.prepare_unet_input(latents, image_latents, cfg, sigma, out=graph.tok)
                        noise_tok = graph.run(t)
                    else:
                        if sampled is not None:    # the module global: the eager walk and the recording step read it in ops
                            ops.GEMM_EVENTS = events_all if (events_all is not None and sampled(i)) else None
                        ops.prepare_unet_input(latents, image_latents, cfg, sigma, out=tok_buf)     # replicated
                        if refresh_rows is not None:
                            refresh_rows()
                        t_dev.fill_(float(t))
                        noise_tok = forward(ops.GEMM_EVENTS)
                        if gather is not None:     # over all ranks; the update below is replicated
                            noise_tok = gather(noise_tok)
                    if direct_fusion:
                        ops.cfg_fusion_euler_step(noise_tok, latents, guidance_dev, fusion_w, cfg, sigma, sigma_next,
                                                  v_prediction=vpred)
                    else:
                        ops.cfg_euler_step(noise_tok, latents, guidance_dev, cfg, sigma, sigma_next, v_prediction=vpred)
                return self._euler_loop(latents, step, num_inference_steps, start_step, callback_on_step_end,
                                        callback_on_step_end_tensor_inputs)
        finally:          # whatever ended the loop, the caller's event list is back
            if sampled is not None:
                ops.GEMM_EVENTS = events_all

    def _euler_loop(self, latents: torch.Tensor, step: Callable, num_inference_steps: int, start_step: int,
                    callback_on_step_end: Optional[Callable], callback_on_step_end_tensor_inputs: List[str]) -> torch.Tensor:
        """the skeleton of every denoising loop here (reference :545-640): ``step(i, latents, t, sigma, sigma_next)`` takes Euler
        step ``i`` in place; around it the timestep table, the ``start_step`` skip (trans_controlnet :571-574: skipped steps run
        nothing, not even the callback), the roctx range (LKGD_ROCTX=1), the device timers (LKGD_STEP_TIMERS=1: ms per Euler
        step) and the callback, whose returned ``latents`` replace the loop's"""
        sch = self.scheduler
        sch.set_timesteps(num_inference_steps, device=None)
        self._num_timesteps = len(sch.timesteps_host)
        timers = _trace.StepTimers() if _trace.STEP_TIMERS else None
        self.last_step_timers = timers
        for i, t in enumerate(sch.timesteps_host):
            if i < start_step:
                continue
            _trace.push(f"euler_step_{i}")
            t_ev = timers.start() if timers is not None else None
            step(i, latents, t, sch.sigmas_host[i], sch.sigmas_host[i + 1])
            if timers is not None:
                timers.stop(t_ev)
            _trace.pop()
            if callback_on_step_end is not None:
                kw = {k: {"latents": latents}[k] for k in callback_on_step_end_tensor_inputs}
                out = callback_on_step_end(self, i, t, kw)
                latents = out.pop("latents", latents) if isinstance(out, dict) else latents
        sch._step_index = num_inference_steps
        if timers is not None:
            timers.finish()
        return latents

    def release_arena(self) -> None:
        """return the recorded forwards' working-set pool(s) to the driver (they are kept between calls otherwise)"""
        self._arenas.clear()

    def arena_reserved_bytes(self) -> int:
        """device memory the recorded forward's private pool holds (the plan's working set)"""
        return self._arenas.reserved_bytes()

    def _latents_for_decode(self, latents: torch.Tensor) -> torch.Tensor:
        """hook between the loop and the VAE decode (identity here; the flow pipeline un-normalises)"""
        return latents

    def _controlnet_condition_batch(self, cc, height: int, width: int, device, cfg: bool) -> torch.Tensor:
        """reference pipeline_stable_video_diffusion_controlnet.py:546-550: VaeImageProcessor.preprocess ([0,1] -> [-1,1]), add
        the batch axis, duplicate for CFG"""
        if isinstance(cc, torch.Tensor) and cc.dim() == 5:      # already batched [1,F,3,H,W] in [0,1]
            cc = 2.0 * cc.to(device) - 1.0
        else:
            cc = self.image_processor.preprocess(cc, height=height, width=width).to(device)
        if cc.dim() == 4:
            cc = cc.unsqueeze(0)
        return torch.cat([cc] * 2) if cfg else cc

    def _graphed_forward(self, Bc: int, F: int, H: int, W: int, enc: torch.Tensor, ids: torch.Tensor):
        """HIP-graph replay of ``unet.forward_tokens`` for fixed shapes / conditioning.  Static buffers: input tokens,
        timestep scalar; the captured kernels are exactly the ones the eager path launches (same stream semantics:
        everything in lkgd_amd/csrc is capturable - no allocation or sync inside).  Re-captured when shapes, weights or
        the conditioning tensors change."""
        unet = self.unet
        # the joint hooks' on/off state is part of the captured launch sequence: a graph captured with them on never replays
        # with them off (direct_fusion switches them off)
        joint = tuple(bool(m.enable_joint_attention) for m in unet.modules() if hasattr(m, "enable_joint_attention"))
        key = (Bc, F, H, W, enc.data_ptr(), enc._version, ids.data_ptr(), ids._version, id(unet._pk),
               getattr(unet, "_joint_attn_mask", None) is not None, joint)
        g = self._graph
        if g is not None and g.key == key:
            return g
        dev = unet.device

        class _G:
            pass
        g = _G()
        g.key = key
        g.tok = torch.empty(Bc * F * H * W, 8, dtype=torch.float16, device=dev)
        g.t = torch.zeros(1, dtype=torch.float32, device=dev)
        g.tok.zero_()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                    # warm-up on a side stream (allocator pools, lazy caches)
            unet.forward_tokens(g.tok, Bc, F, H, W, g.t, enc, ids)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g.out, _ = unet.forward_tokens(g.tok, Bc, F, H, W, g.t, enc, ids)
        g.graph = graph

        def run(t_value: float, _g=g):
            _g.t.fill_(float(t_value))
            _g.graph.replay()
            return _g.out
        g.run = run
        self._graph = g
        return g

    @torch.no_grad()
    def __call__(self, image, height: int = 576, width: int = 1024, num_frames: Optional[int] = None,
                 num_inference_steps: int = 25, min_guidance_scale: float = 1.0, max_guidance_scale: float = 3.0,
                 fps: int = 7, motion_bucket_id: int = 127, noise_aug_strength: float = 0.02,
                 decode_chunk_size: Optional[int] = None, num_videos_per_prompt: Optional[int] = 1,
                 generator=None, latents: Optional[torch.Tensor] = None, output_type: Optional[str] = "pil",
                 callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], return_dict: bool = True,
                 # extensions (keyword-only in practice; defaults keep the reference call sites unchanged)
                 image_embeddings: Optional[torch.Tensor] = None, image_latents: Optional[torch.Tensor] = None,
                 domain_features: Optional[torch.Tensor] = None, flow_features: Optional[torch.Tensor] = None,
                 # pipeline_stable_video_diffusion_controlnet.py:356-380: a [F,3,H,W] (or [1,F,3,H,W]) tensor in [0,1]
                 controlnet_condition: Optional[torch.Tensor] = None, controlnet_cond_scale: float = 1.0,
                 # pipeline_stable_video_diffusion_trans_controlnet.py:354-380 (StableVideoDiffusionPipelineTransControlNet)
                 original_latents: Optional[torch.Tensor] = None, start_step: int = 0, direct_fusion: bool = False,
                 controlnet_scale: float = 1.0):
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        num_frames = num_frames if num_frames is not None else self.unet.config.num_frames
        decode_chunk_size = decode_chunk_size if decode_chunk_size is not None else num_frames
        if image is not None:
            self.check_inputs(image, height, width)
        if isinstance(image, torch.Tensor):
            batch_size = image.shape[0]
        elif isinstance(image, list):
            batch_size = len(image)
        elif image is None:
            batch_size = image_latents.shape[0] // (2 if max_guidance_scale > 1 else 1)
        else:
            batch_size = 1
        device = self._execution_device
        self._guidance_scale = max_guidance_scale
        cfg = self.do_classifier_free_guidance
        if image_embeddings is None:
            image_embeddings = self._encode_image(image, device, num_videos_per_prompt, cfg)
        fps = fps - 1
        if image_latents is None:
            img = self.image_processor.preprocess(image, height=height, width=width).to(device)      # reference :466
            noise = _randn_tensor(img.shape, generator, device, img.dtype)      # drawn for the execution device (:467)
            img = img + noise_aug_strength * noise
            image_latents = self._encode_vae_boundary(img, device, num_videos_per_prompt, cfg, image_embeddings.dtype)
        image_latents = image_latents.to(device=device, dtype=torch.float16)
        if image_latents.dim() == 4:      # [cfg*B,4,h,w] -> repeat over frames (:488)
            image_latents = image_latents.unsqueeze(1).repeat(1, num_frames, 1, 1, 1)
        added_time_ids = self._get_add_time_ids(fps, motion_bucket_id, noise_aug_strength, torch.float32, batch_size,
                                                num_videos_per_prompt, cfg).to(device)
        self.scheduler.set_timesteps(num_inference_steps, device=None)
        lat = self.prepare_latents(batch_size * num_videos_per_prompt, num_frames, self.unet.config.in_channels,
                                   height, width, torch.float16, device, generator, latents)
        if direct_fusion:
            # trans_controlnet :660-666: the fp32 linspace weight promotes the reference's latents to fp32 at the first fused
            # step; here they are carried in fp32 from the start (prepare_unet_input and the fused step both take fp32)
            lat = lat.float()
        if original_latents is not None:
            # trans_controlnet :528-529: scheduler.add_noise(original_latents, randn_like(latents), timesteps[[start_step]]) -
            # an SDEdit start; the noise comes from the global RNG of the latents' device, as the reference draws it.  Once per
            # clip, before the loop
            noise = torch.randn_like(lat)
            orig = original_latents.to(device)
            lat = (orig + noise * torch.tensor(self.scheduler.sigmas_host[start_step], dtype=orig.dtype,
                                               device=device)).to(lat.dtype).contiguous()
        if controlnet_condition is not None:
            controlnet_condition = self._controlnet_condition_batch(controlnet_condition, height, width, device, cfg)
        lat = self.denoise(lat, image_latents.contiguous(), image_embeddings, added_time_ids, num_inference_steps,
                           min_guidance_scale, max_guidance_scale, domain_features, flow_features,
                           callback_on_step_end, callback_on_step_end_tensor_inputs, controlnet_condition,
                           controlnet_cond_scale, start_step=start_step, direct_fusion=direct_fusion,
                           controlnet_scale=controlnet_scale)
        if output_type != "latent":
            frames = self.decode_latents(self._latents_for_decode(lat), num_frames, decode_chunk_size)
            frames = tensor2vid(frames, self.image_processor, output_type=output_type)               # reference :644
        else:
            frames = lat
        if not return_dict:
            return frames
        return StableVideoDiffusionPipelineOutput(frames=frames)


class StableVideoDiffusionPipelineControlNet(StableVideoDiffusionPipeline):
    """/root/reference/pipeline/pipeline_stable_video_diffusion_controlnet.py: ``controlnet_condition`` is the SECOND positional
    argument (:352-376); the loop runs the ControlNet-SVD encoder before the UNet every step (:582-607)"""

    def __call__(self, image, controlnet_condition=None, height: int = 576, width: int = 1024, num_frames=None,
                 num_inference_steps: int = 25, min_guidance_scale: float = 1.0, max_guidance_scale: float = 3.0,
                 fps: int = 7, motion_bucket_id: int = 127, noise_aug_strength: float = 0.02, decode_chunk_size=None,
                 num_videos_per_prompt=1, generator=None, latents=None, output_type="pil", callback_on_step_end=None,
                 callback_on_step_end_tensor_inputs=["latents"], return_dict: bool = True, controlnet_cond_scale=1.0,
                 batch_size=1, **extensions):
        return super().__call__(image, height, width, num_frames, num_inference_steps, min_guidance_scale,
                                max_guidance_scale, fps, motion_bucket_id, noise_aug_strength, decode_chunk_size,
                                num_videos_per_prompt, generator, latents, output_type, callback_on_step_end,
                                callback_on_step_end_tensor_inputs, return_dict,
                                controlnet_condition=self._condition(controlnet_condition),
                                controlnet_cond_scale=controlnet_cond_scale, **extensions)

    def _condition(self, controlnet_condition):
        return controlnet_condition


class StableVideoDiffusionPipelineTransControlNet(StableVideoDiffusionPipeline):
    """/root/reference/pipeline/pipeline_stable_video_diffusion_trans_controlnet.py: the joint-attention pair pipeline with the
    ControlNet (signature :354-380).  ``controlnet_condition`` is one [F,C,H,W] condition or a list with one per clip
    (:531-541); ``original_latents`` + ``start_step`` start from noised latents and skip the first steps (:528-529, :571-574);
    ``controlnet_scale`` multiplies every residual on top of ``controlnet_cond_scale`` (:594-598); ``direct_fusion`` switches
    the joint hooks off and fuses clip b with the frame-reversed clip b + B/2 through their x0 once per step (:637-667).
    Its fused branch also draws ``randn_tensor(..., generator=generator)`` every step (:648-650); that noise is never read and
    nothing downstream uses the generator, so it is not drawn here.  Single-GPU only: under frame sharding the blend pairs
    frame f with frame F-1-f, which another rank holds (lkgd_amd/dist_run.py does not take these arguments)."""

    def __call__(self, image, controlnet_condition=None, height: int = 576, width: int = 1024, num_frames=None,
                 num_inference_steps: int = 25, min_guidance_scale: float = 1.0, max_guidance_scale: float = 3.0,
                 fps: int = 7, motion_bucket_id: int = 127, noise_aug_strength: float = 0.02, decode_chunk_size=None,
                 num_videos_per_prompt=1, generator=None, latents=None, output_type="pil", callback_on_step_end=None,
                 callback_on_step_end_tensor_inputs=["latents"], return_dict: bool = True, controlnet_cond_scale=1.0,
                 original_latents=None, start_step=0, direct_fusion=False, controlnet_scale=1.0, **extensions):
        return super().__call__(image, height, width, num_frames, num_inference_steps, min_guidance_scale,
                                max_guidance_scale, fps, motion_bucket_id, noise_aug_strength, decode_chunk_size,
                                num_videos_per_prompt, generator, latents, output_type, callback_on_step_end,
                                callback_on_step_end_tensor_inputs, return_dict,
                                controlnet_condition=controlnet_condition, controlnet_cond_scale=controlnet_cond_scale,
                                original_latents=original_latents, start_step=start_step, direct_fusion=direct_fusion,
                                controlnet_scale=controlnet_scale, **extensions)

    def _controlnet_condition_batch(self, cc, height: int, width: int, device, cfg: bool) -> torch.Tensor:
        """:531-541: every entry preprocessed and given a batch axis, then ``torch.cat(conds * 2)``: under CFG that lines up with
        [uncond clips..., cond clips...].  Without CFG the reference's batch would be twice the latent batch (its call cannot
        run); one copy per clip is passed instead (deviations)"""
        if not isinstance(cc, list):
            cc = [cc]
        conds = [self.image_processor.preprocess(c, height=height, width=width).unsqueeze(0) for c in cc]
        return torch.cat(conds * 2 if cfg else conds).to(device)


class StableVideoDiffusionPipelineSmooth(StableVideoDiffusionPipeline):
    """pipeline/pipeline_stable_video_diffusion_smooth.py (driven by run_models/run_inference_svd_smooth.py): an input video of
    any length T is noised to ``start_step`` and denoised in frame windows of at most ``num_frames`` frames.  ``__call__`` has
    the reference's parameter list (:320-341); ``image`` is the list or tensor of the T frames.  Every Euler step cuts the
    frames into windows (``smooth_chunks``) and runs the UNet per window on [window, reversed window] x [uncond, cond]; the
    window's first and last frame condition the forward and the reversed clip (:549-577); only the forward clip's CFG result
    steps the window's frames (:579-594).  The run script patches the UNet with ``apply_patch(flip=True)`` and the joint mask
    [0, 1, 0, 1] (utils/util.py:408-438): the joint hooks are left as the model has them.  The loop is ``denoise_smooth``: two
    glue launches per window (lkgd_window_prepare_input, lkgd_window_cfg_euler_step) around the UNet forward.
    Refused, with the reason: ``max_guidance_scale <= 1`` (the reference's own no-CFG branch feeds the whole latents tensor to
    the UNet, :565, and cannot run with more than one window), ``num_videos_per_prompt != 1``, ``num_frames > 16`` (the fused
    temporal kernels' limit), a ``controlnet_condition`` and sharded runs."""

    SCALING_FACTOR = 0.18215       # AutoencoderKLTemporalDecoder's config value, used when the pipeline carries no VAE

    def _refuse(self, num_frames, max_guidance_scale, num_videos_per_prompt=1, controlnet_condition=None, shard=None):
        if not max_guidance_scale > 1:
            raise ValueError("the smoothing pipeline needs classifier-free guidance (max_guidance_scale > 1): the reference's "
                             "no-CFG branch feeds the whole latents tensor to the UNet and cannot run with more than one window")
        if num_videos_per_prompt != 1:
            raise ValueError(f"the smoothing pipeline denoises one video: num_videos_per_prompt must be 1, got {num_videos_per_prompt}")
        if not 1 <= num_frames <= 16:
            raise ValueError(f"window length num_frames must be 1..16 (the fused temporal kernels' limit), got {num_frames}")
        if controlnet_condition is not None:
            raise ValueError("the smoothing pipeline runs no ControlNet: controlnet_condition is not taken")
        if shard is not None:
            raise ValueError("the smoothing loop is single-GPU: sharded runs are not supported")

    def _noisy_start(self, image_latents: torch.Tensor, noise: torch.Tensor, start_step: int) -> torch.Tensor:
        """:466, :516-518: scheduler.add_noise(image_latents * scaling_factor, noise, timesteps[[start_step]]) as [1,T,4,h,w]
        fp16 (the reference's latents dtype); needs ``scheduler.set_timesteps``"""
        sf = self.vae.config.scaling_factor if self.vae is not None else self.SCALING_FACTOR
        orig = (image_latents.float() * sf).unsqueeze(0)
        noise = noise.to(device=orig.device, dtype=torch.float16).reshape(orig.shape)
        start = self.scheduler.add_noise(orig, noise, [self.scheduler.timesteps_host[start_step]])
        return start.to(torch.float16).contiguous()

    @torch.no_grad()
    def denoise_smooth(self, latents: torch.Tensor, image_latents: torch.Tensor, image_embeddings: torch.Tensor,
                       added_time_ids: torch.Tensor, num_frames: int, num_inference_steps: int = 25,
                       min_guidance_scale: float = 1.0, max_guidance_scale: float = 3.0, start_step: int = 0,
                       callback_on_step_end: Optional[Callable] = None,
                       callback_on_step_end_tensor_inputs: List[str] = ["latents"], controlnet_condition=None,
                       shard=None) -> torch.Tensor:
        """Reference loop :535-605.  ``latents`` [1,T,4,h,w] noised to ``start_step`` (fp16 or fp32, updated in place and
        returned); ``image_latents`` [T,4,h,w]: the VAE latent of every input frame (the unconditional zeros are never
        materialised); ``image_embeddings`` [T,1,1024]: the CLIP embedding of every input frame; ``added_time_ids`` [1,3] (or the
        reference's 4 equal rows).  Per window: one glue kernel (gather + flip + CFG duplicate + scale_model_input + channel
        concat -> tokens of the batch of four), the UNet forward at (4, L, h, w) with the embedding rows [0, 0, emb[f0],
        emb[f0+L-1]], one glue kernel (per-frame CFG of the forward clip + Euler update of the window's frames).  The forward is
        recorded once per call at L == num_frames and replayed for the later windows of that length (token buffer, timestep and
        embedding rows are updated in place); windows of other lengths walk the modules, so the call holds one plan's arena."""
        unet, sch = self.unet, self.scheduler
        dev = unet.device
        self._refuse(num_frames, max_guidance_scale, controlnet_condition=controlnet_condition, shard=shard)
        if latents.dim() != 5 or latents.shape[0] != 1 or latents.shape[2] != 4:
            raise ValueError(f"latents must be [1,T,4,h,w] (the smoothing pipeline denoises one video), got {tuple(latents.shape)}")
        _, T, _, H, W = latents.shape
        if tuple(image_latents.shape) != (T, 4, H, W) or image_embeddings.shape[0] != T or image_embeddings.dim() != 3:
            raise ValueError("image_latents [T,4,h,w] and image_embeddings [T,1,C] must carry one conditional entry per input frame")
        cfg, nf = 2, int(num_frames)
        latents = latents.to(dev).contiguous()
        image_latents = image_latents.to(device=dev, dtype=torch.float16).contiguous()
        emb = image_embeddings.to(device=dev, dtype=torch.float16).contiguous()
        ids = added_time_ids.to(device=dev, dtype=torch.float32).reshape(-1, added_time_ids.shape[-1])
        if 2 * cfg % ids.shape[0]:
            raise ValueError(f"added_time_ids must be built for one clip (1, 2 or 4 equal rows), got {ids.shape[0]} rows")
        ids = ids.repeat(2 * cfg // ids.shape[0], 1).contiguous()           # :539 and the CFG duplicate of _get_add_time_ids
        self._guidance_scale = max_guidance_scale
        # :581: torch.linspace(min, max, len(chunk)) per window - one device table for the call, row L-1 holds the L values
        gtab = torch.zeros(nf, nf, dtype=torch.float32)
        for n in range(1, nf + 1):
            gtab[n - 1, :n] = torch.linspace(min_guidance_scale, max_guidance_scale, n, dtype=torch.float32)
        gtab = gtab.to(dev)
        vpred = sch.config.prediction_type == "v_prediction"
        HW = H * W
        # static inputs of the window forward: the tokens of the largest window, the timestep and the embedding rows of the batch
        # [uncond fwd, uncond rev, cond fwd, cond rev] (:554-561); rows 0 / 1 stay zero
        tok_buf = torch.empty(2 * cfg * nf * HW, 8, dtype=torch.float16, device=dev)
        t_dev = torch.zeros(2 * cfg, dtype=torch.float32, device=dev)
        enc = torch.zeros(2 * cfg, emb.shape[1], emb.shape[2], dtype=torch.float16, device=dev)
        with _replay.Replayed(self._arenas, dev, lambda: ("smooth", 2 * cfg, nf, H, W, id(unet._pk)),
                              lambda: unet.forward_tokens(tok_buf, 2 * cfg, nf, H, W, t_dev, enc, ids)[0],
                              enabled=self.use_replay) as full_window:
            def step(_i, latents, t, sigma, sigma_next):
                for f0, n in smooth_chunks(T, nf):
                    tok = ops.window_prepare_input(latents, image_latents, f0, n, cfg, sigma, out=tok_buf)
                    enc[2].copy_(emb[f0])
                    enc[3].copy_(emb[f0 + n - 1])
                    if n == nf:
                        t_dev.fill_(float(t))
                        noise_tok = full_window(ops.GEMM_EVENTS)
                    else:
                        noise_tok, _ = unet.forward_tokens(tok, 2 * cfg, n, H, W, t, enc, ids)
                    ops.window_cfg_euler_step(noise_tok, latents, gtab[n - 1, :n], f0, n, cfg, sigma, sigma_next,
                                              v_prediction=vpred)
            return self._euler_loop(latents, step, num_inference_steps, start_step, callback_on_step_end,
                                    callback_on_step_end_tensor_inputs)

    @torch.no_grad()
    def __call__(self, image, height: int = 576, width: int = 1024, num_frames: Optional[int] = None,
                 num_inference_steps: int = 25, min_guidance_scale: float = 1.0, max_guidance_scale: float = 3.0,
                 fps: int = 7, motion_bucket_id: int = 127, noise_aug_strength: float = 0.02,
                 decode_chunk_size: Optional[int] = None, num_videos_per_prompt: Optional[int] = 1,
                 generator=None, latents: Optional[torch.Tensor] = None, output_type: Optional[str] = "pil",
                 callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], return_dict: bool = True, start_step=0,
                 # extensions: per-frame boundary outputs computed outside ([T,1,1024] / [T,4,h,w]) and the start noise [1,T,4,h,w]
                 image_embeddings: Optional[torch.Tensor] = None, image_latents: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None, controlnet_condition=None):
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        num_frames = num_frames if num_frames is not None else self.unet.config.num_frames
        decode_chunk_size = decode_chunk_size if decode_chunk_size is not None else num_frames
        self._refuse(num_frames, max_guidance_scale, num_videos_per_prompt, controlnet_condition)
        if image is not None:
            self.check_inputs(image, height, width)
        device = self._execution_device
        self._guidance_scale = max_guidance_scale
        if image_embeddings is None:
            # one CLIP embedding per input frame (:442); the unconditional zeros are rows 0 / 1 of every window's batch
            image_embeddings = self._encode_image(image, device, 1, False)
        if image_latents is None:
            img = self.image_processor.preprocess(image, height=height, width=width).to(device)      # :450-452
            img = img + noise_aug_strength * _randn_tensor(img.shape, generator, device, img.dtype)
            # :458-464: the T frames go through the VAE in slices of decode_chunk_size
            image_latents = self._encode_vae_boundary(img, device, 1, False, torch.float32, chunk=decode_chunk_size)
        image_latents = image_latents.to(device)
        total_frames = image_latents.shape[0]
        added_time_ids = self._get_add_time_ids(fps - 1, motion_bucket_id, noise_aug_strength, torch.float32, 1, 1,
                                                False).to(device)
        self.scheduler.set_timesteps(num_inference_steps, device=None)
        if noise is None:
            # the reference draws this noise from torch's global RNG (torch.randn_like, :518) and ignores `generator` and
            # `latents` there; here it comes from `generator` (deviations)
            noise = _randn_tensor((1, total_frames) + tuple(image_latents.shape[1:]), generator, device, torch.float16)
        lat = self._noisy_start(image_latents, noise, start_step)
        lat = self.denoise_smooth(lat, image_latents.to(torch.float16), image_embeddings, added_time_ids, num_frames,
                                  num_inference_steps, min_guidance_scale, max_guidance_scale, start_step,
                                  callback_on_step_end, callback_on_step_end_tensor_inputs)
        if output_type != "latent":
            frames = self.decode_latents(lat, total_frames, decode_chunk_size)                       # :611-612
            frames = tensor2vid(frames, self.image_processor, output_type=output_type)
        else:
            frames = lat
        if not return_dict:
            return frames
        return StableVideoDiffusionPipelineOutput(frames=frames)


class StableVideoDiffusionPipelineControlNetFlow(StableVideoDiffusionPipelineControlNet):
    """/root/reference/pipeline/pipeline_stable_video_diffusion_controlnet_flow.py (BASELINE.json configs[3]) AS THE
    REFERENCE RUNS IT: same signature, but its ControlNet call and the condition's preprocessing are commented out
    (:548-553,:590-607) - ``controlnet_condition`` is accepted and unused, the UNet runs without residuals - and the
    denoised latents are flow latents, un-normalised before the VAE decode (:641, utils/optical_flow.py:62-77)."""

    def _condition(self, controlnet_condition):
        return None

    def _latents_for_decode(self, latents: torch.Tensor) -> torch.Tensor:
        from .optical_flow import optical_flow_latent_unnormalize
        return optical_flow_latent_unnormalize(latents)

"""The three pipeline objects the reference's CogVideoX launcher constructs by ``generate_type`` (CogVideo-main/inference/cli_demo.py:118-125,
:156-194): ``CogVideoXImageToVideoPipeline`` (``i2v``), ``CogVideoXPipeline`` (``t2v``) and ``CogVideoXVideoToVideoPipeline`` (``v2v``).

``CogVideoXImageToVideoPipeline`` is the reference's own class
(CogVideo-main/finetune/models/cogvideox_i2v/pipeline_cogvideox_image2video.py:166-227 the constructor, :465-527 ``check_inputs``,
:610-919 ``__call__``; inference/cli_demo.py and the trainers' validation go through it).  The stages are the free functions of
lkgd_amd/cogvideox.py and lkgd_amd/cogvideox_vae.py - ``encode_prompt``, ``prepare_latents``, ``denoise``, ``decode_latents`` - called
in the reference's order with the reference's glue between them; nothing of them is restated here.  Frames in and frames out go
through :class:`lkgd_amd.video_processor.VideoProcessor` (include/lkgd_hip_video.h).

``CogVideoXPipeline`` and ``CogVideoXVideoToVideoPipeline`` are diffusers' classes (pipelines/cogvideo/pipeline_cogvideox.py,
pipeline_cogvideox_video2video.py), which the reference only imports: **[EXT], parity unpinned** as a whole.  They
run the stock transformer - no ``domain_model`` / ``flow_model``, no latent-knowledge fuse - over the same stages: ``encode_prompt``,
``prepare_noise_latents`` or ``preprocess_video`` + ``prepare_video_latents``, ``denoise(image_latents=None, start_step=...)``,
``decode_latents``.  Per step nothing but the loop's three launches runs.

What diffusers supplies around the classes - ``DiffusionPipeline.from_pretrained`` / ``to`` / the offload switches,
``retrieve_timesteps``, ``VideoProcessor``, ``CogVideoXPipelineOutput`` - is restated from its published behaviour **[EXT], parity
unpinned**: diffusers is not installable next to this package, so none of the classes themselves can be executed.  All of that, and
what the three classes share of the reference's class, lives once in ``_CogVideoXPipelineBase``.

Arguments of ``__call__`` the loop (``denoise``) cannot honour raise ``LkgdHipError`` naming themselves; nothing is silently ignored:
custom ``timesteps``, ``eta != 0``, ``attention_kwargs``, a ``callback_on_step_end`` that returns replaced ``latents`` /
``prompt_embeds`` / ``negative_prompt_embeds`` or sets ``interrupt``, a missing ``domain_model`` / ``flow_model`` (image-to-video), a
transformer with an ``ofs_embedding`` (text- / video-to-video: their classes pass no ``ofs``).  Not built: bf16, ``export_to_video``,
``load_video``, a sharded ``__call__``.

LoRA ([EXT] diffusers ``CogVideoXLoraLoaderMixin``, parity unpinned): ``lora_state_dict``, ``load_lora_weights``,
``save_lora_weights``, ``fuse_lora`` / ``unfuse_lora``, ``set_adapters``, ``get_active_adapters``, ``enable_lora`` / ``disable_lora``,
``unload_lora_weights`` with diffusers' names and keywords, for the ``transformer`` component (any other raises, naming itself).  They
change module state only - the adapters are folded into the weights when the DiT packs - so ``__call__`` is the same call with and
without adapters, and they work before ``to("cuda")`` (the order of inference/cli_demo.py:128-132)."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from . import cogvideox as cx
from . import lora as _lora
from ._lib import LkgdHipError
from .cogvideox_vae import AutoencoderKLCogVideoX, decode_latents
from .image_processor import PIL
from .video_processor import VideoProcessor


@dataclass
class CogVideoXPipelineOutput:
    """[EXT diffusers pipelines/cogvideo/pipeline_output.py]"""
    frames: Any


def additional_latent_frames(num_frames: int, temporal_factor: int, patch_size_t: Optional[int]):
    """:779-786: (latent frames, additional latent frames, padded pixel frame count) - the 1.5 models pad the latent frames to a
    multiple of ``patch_size_t`` and ask ``prepare_latents`` for the pixel frames that give them"""
    latent_frames = (num_frames - 1) // temporal_factor + 1
    additional = cx.temporal_padding_frames(latent_frames, patch_size_t)
    return latent_frames, additional, num_frames + additional * temporal_factor


class _CogVideoXPipelineBase:
    """what the three pipelines share: [EXT] ``DiffusionPipeline``, [EXT] ``CogVideoXLoraLoaderMixin``, and the methods the reference's
    class has in common with diffusers' two (``encode_prompt``, ``decode_latents``, the rotary helper, the properties, the prompt half
    of ``check_inputs``, the callback contract).  Messages name the concrete class"""
    _optional_components: List[str] = []
    model_cpu_offload_seq = "text_encoder->transformer->vae"
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]
    #: why ``from_pretrained`` insists on the VAE's encoder (None: a decoder-only ``vae/`` will do)
    _encoder_use: Optional[str] = None

    def __init__(self, tokenizer, text_encoder, vae, transformer, scheduler):
        self.tokenizer, self.text_encoder, self.vae, self.transformer, self.scheduler = tokenizer, text_encoder, vae, transformer, scheduler
        self.vae_scale_factor_spatial = 2 ** (len(vae.config.block_out_channels) - 1) if vae is not None else 8
        self.vae_scale_factor_temporal = vae.config.temporal_compression_ratio if vae is not None else 4
        self.vae_scaling_factor_image = vae.config.scaling_factor if vae is not None else 0.7
        self.video_processor = VideoProcessor(vae_scale_factor=self.vae_scale_factor_spatial)
        self._guidance_scale = None
        self._num_timesteps = None
        self._current_timestep = None
        self._attention_kwargs = None
        self._interrupt = False

    # ---- [EXT] DiffusionPipeline ------------------------------------------------------------------------------------------------------
    @property
    def components(self) -> Dict[str, Any]:
        return dict(tokenizer=self.tokenizer, text_encoder=self.text_encoder, vae=self.vae, transformer=self.transformer,
                    scheduler=self.scheduler)

    def to(self, device):
        """every module of the pipeline moves to ``device``; returns the pipeline"""
        for m in self.components.values():
            if isinstance(m, torch.nn.Module):
                m.to(device)
        return self

    @property
    def device(self):
        return self.transformer.device

    _execution_device = device

    def enable_model_cpu_offload(self, *args, **kwargs) -> None:
        """does nothing: in the reference it only decides where the weights wait between stages, and the launchers call it
        unconditionally.  Here every module stays where ``to(device)`` put it"""

    def enable_sequential_cpu_offload(self, *args, **kwargs) -> None:
        """does nothing, for the same reason as ``enable_model_cpu_offload``"""

    def maybe_free_model_hooks(self) -> None:
        """does nothing: there are no offload hooks"""

    @classmethod
    def _load_components(cls, path: str, torch_dtype=None, tokenizer=None):
        """``from_pretrained``'s loading: (tokenizer, text_encoder, vae, transformer, scheduler) of a local checkpoint directory"""
        from .loading import load_config
        from .t5 import T5EncoderModel
        index = load_config(path, None, name="model_index.json")
        for part in ("text_encoder", "vae", "transformer", "scheduler"):
            if part not in index:
                raise LkgdHipError(f"{cls.__name__}.from_pretrained({path!r}): model_index.json names no {part!r}")
        text_encoder = T5EncoderModel.from_pretrained(path, subfolder="text_encoder", **({} if torch_dtype is None else {"torch_dtype": torch_dtype}))
        vae = AutoencoderKLCogVideoX.from_pretrained(path, subfolder="vae", torch_dtype=torch_dtype)
        if cls._encoder_use is not None and not vae.has_encoder:
            raise LkgdHipError(f"{cls.__name__}.from_pretrained({path!r}): vae/ holds no encoder.* keys; the "
                               f"{cls._encoder_use} and needs the whole VAE")
        transformer = cx.CogVideoXTransformer3DModel.from_pretrained(path, subfolder="transformer", torch_dtype=torch_dtype)
        scheduler = cx.scheduler_from_config(path)
        if tokenizer is None and os.path.isdir(os.path.join(path, "tokenizer")):
            try:
                from transformers import T5Tokenizer
                tokenizer = T5Tokenizer.from_pretrained(os.path.join(path, "tokenizer"))
            except ImportError:     # transformers or sentencepiece absent: the tokenizer stays the caller's business
                tokenizer = None
        return tokenizer, text_encoder, vae, transformer, scheduler

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=None, tokenizer=None):
        """a local checkpoint directory in diffusers' layout: ``model_index.json`` and ``text_encoder/``, ``vae/``, ``transformer/``,
        ``scheduler/``, each read by its own loader.  ``tokenizer``: the caller's; omitted, ``tokenizer/`` is read with transformers'
        ``T5Tokenizer`` where that can be imported, else it stays None (prompts as id tensors or ``prompt_embeds`` need none)"""
        return cls(*cls._load_components(path, torch_dtype, tokenizer))

    # ---- [EXT] CogVideoXLoraLoaderMixin ----------------------------------------------------------------------------------------------
    _lora_loadable_modules = ["transformer"]

    @classmethod
    def _only_transformer(cls, components, where: str) -> None:
        if isinstance(components, str) or len(components) == 0:
            raise ValueError(f"{where}: `components` has to be a non-empty list, got {components!r}")
        for c in components:
            if c not in cls._lora_loadable_modules:
                raise LkgdHipError(f"{where}: component {c!r} - LoRA is built for {cls._lora_loadable_modules} only")

    @classmethod
    def lora_state_dict(cls, pretrained_model_name_or_path_or_dict, weight_name: str = "pytorch_lora_weights.safetensors", **_hub):
        """a directory (holding ``weight_name``), a file, or a state dict -> the transformer's LoRA state dict: the keys under
        ``transformer.`` are kept, without the prefix (a key without a component prefix counts as the transformer's).  A
        ``text_encoder.`` key raises: text-encoder LoRA is not built.  ``.alpha`` entries (kohya / ``network_alphas`` files) raise as
        well; the file's metadata is not read.  Hub / cache keywords are accepted and ignored"""
        sd, alphas = _lora.lora_state_dict(pretrained_model_name_or_path_or_dict, weight_name)
        if alphas:
            raise LkgdHipError(f"lora_state_dict: '{sorted(alphas)[0]}' - `.alpha` entries (kohya / network_alphas files) are not built")
        out = {}
        for k, v in sd.items():
            if k.startswith("text_encoder"):
                raise LkgdHipError(f"lora_state_dict: key '{k}' - text-encoder LoRA is not built")
            out[k[len("transformer."):] if k.startswith("transformer.") else k] = v
        return out

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, weight_name: str = "pytorch_lora_weights.safetensors",
                          adapter_name: Optional[str] = None, **_hub):
        """``lora_state_dict`` + the transformer's ``load_lora_adapter``; the adapter (default name ``default_0``, ``default_1``, ...)
        is the active one afterwards.  Returns the ``quaternion_lora_*`` names the file did not hold"""
        sd = self.lora_state_dict(pretrained_model_name_or_path_or_dict, weight_name)
        return self.transformer.load_lora_adapter(sd, adapter_name=adapter_name)

    @classmethod
    def save_lora_weights(cls, save_directory, transformer_lora_layers=None, is_main_process: bool = True,
                          weight_name: Optional[str] = "pytorch_lora_weights.safetensors", save_function=None,
                          safe_serialization: bool = True):
        """writes ``transformer_lora_layers`` (``lora.adapter_state_dict(transformer, name)``, plus any ``quaternion_lora_*`` tensors the
        caller adds) under the ``transformer.`` prefix: ``weight_name`` as safetensors, or with ``safe_serialization=False`` by
        ``torch.save``"""
        if not transformer_lora_layers:
            raise ValueError("You must pass `transformer_lora_layers`.")
        if save_function is not None:
            raise LkgdHipError("save_lora_weights: `save_function` is not built")
        sd = {f"transformer.{k}": v.detach().to("cpu").contiguous() for k, v in transformer_lora_layers.items()}
        if not is_main_process:
            return
        os.makedirs(save_directory, exist_ok=True)
        if weight_name is None:
            weight_name = "pytorch_lora_weights.safetensors" if safe_serialization else "pytorch_lora_weights.bin"
        path = os.path.join(save_directory, weight_name)
        if safe_serialization:
            from safetensors.torch import save_file
            save_file(sd, path, metadata={"format": "pt"})
        else:
            torch.save(sd, path)

    def fuse_lora(self, components: List[str] = ["transformer"], lora_scale: float = 1.0, safe_fusing: bool = False,
                  adapter_names: Optional[List[str]] = None):
        """the transformer's ``fuse_lora``: the base weights are not written, the pack folds the fused adapters at ``lora_scale``"""
        self._only_transformer(components, "fuse_lora")
        self.transformer.fuse_lora(lora_scale, adapter_names)

    def unfuse_lora(self, components: List[str] = ["transformer"]):
        self._only_transformer(components, "unfuse_lora")
        self.transformer.unfuse_lora()

    def set_adapters(self, adapter_names, adapter_weights=None):
        self.transformer.set_adapters(adapter_names, adapter_weights)

    def get_active_adapters(self) -> List[str]:
        return self.transformer.active_adapters()

    def enable_lora(self):
        self.transformer.enable_lora()

    def disable_lora(self):
        self.transformer.disable_lora()

    def unload_lora_weights(self):
        self.transformer.unload_lora()

    # ---- what the reference's class shares with diffusers' two ---------------------------------------------------------------------
    def encode_prompt(self, prompt, negative_prompt=None, do_classifier_free_guidance: bool = True, num_videos_per_prompt: int = 1,
                      prompt_embeds=None, negative_prompt_embeds=None, max_sequence_length: int = 226, device=None, dtype=None):
        """:273-352"""
        return cx.encode_prompt(self.text_encoder, self.tokenizer, prompt, negative_prompt, do_classifier_free_guidance,
                                num_videos_per_prompt, prompt_embeds, negative_prompt_embeds, max_sequence_length, device, dtype)

    def decode_latents(self, latents: torch.Tensor) -> torch.Tensor:
        """:430-435"""
        return decode_latents(self.vae, latents)

    def _check_prompt_inputs(self, prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds,
                             negative_prompt_embeds) -> None:
        """:472-527, the same errors (the three ``check_inputs`` share them).  A prompt may also be an int64 id tensor
        (``encode_prompt``)"""
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_on_step_end_tensor_inputs is not None and not all(
                k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found "
                             f"{[k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and not isinstance(prompt, (str, list, torch.Tensor)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None:
            if prompt_embeds.shape != negative_prompt_embeds.shape:
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                                 f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds`"
                                 f" {negative_prompt_embeds.shape}.")

    def _prepare_rotary_positional_embeddings(self, height: int, width: int, num_frames: int, device=None):
        """:544-586: ``num_frames`` are LATENT frames; ``rotary_tables`` holds both branches"""
        tc = self.transformer.config
        grid_height = height // (self.vae_scale_factor_spatial * tc.patch_size)
        grid_width = width // (self.vae_scale_factor_spatial * tc.patch_size)
        p_t = tc.patch_size_t
        frames = num_frames if p_t is None else (num_frames + p_t - 1) // p_t
        return cx.rotary_tables(tc, frames, grid_height, grid_width)

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def attention_kwargs(self):
        return self._attention_kwargs

    @property
    def current_timestep(self):
        return self._current_timestep

    @property
    def interrupt(self):
        return self._interrupt

    def _not_built(self, timesteps, eta, attention_kwargs) -> None:
        name = type(self).__name__
        if timesteps is not None:
            raise LkgdHipError(f"{name}: custom `timesteps` are not built - denoise takes the scheduler's "
                               "trailing spacing of num_inference_steps")
        if eta != 0.0:
            raise LkgdHipError(f"{name}: `eta`={eta} is not built - the DDIM and DPM steps are the eta = 0 ones")
        if attention_kwargs is not None:
            raise LkgdHipError(f"{name}: `attention_kwargs` are not built - the DiT has no attention processors "
                               "to hand them to")

    def _begin_call(self, guidance_scale, attention_kwargs) -> None:
        self._guidance_scale = guidance_scale
        self._current_timestep = None
        self._attention_kwargs = attention_kwargs
        self._interrupt = False

    @staticmethod
    def _batch_size(prompt, prompt_embeds) -> int:
        if prompt is not None and isinstance(prompt, str):
            return 1
        if prompt is not None and isinstance(prompt, (list, torch.Tensor)):
            return len(prompt)
        return prompt_embeds.shape[0]

    def _step_callback(self, callback_on_step_end, tensor_inputs, step_times, prompt_embeds, negative_prompt_embeds):
        """``denoise``'s callback around ``callback_on_step_end`` (None without one): ``step_times`` are the timesteps the loop
        executes, indexed by its step count.  Callbacks observe: a replaced tensor or a set ``interrupt`` raises"""
        if callback_on_step_end is None:
            return None
        handed = {"prompt_embeds": prompt_embeds, "negative_prompt_embeds": negative_prompt_embeds}
        name = type(self).__name__

        def callback(i, t, step_latents):
            self._current_timestep = step_times[i]
            handed["latents"] = step_latents
            outputs = callback_on_step_end(self, i, step_times[i], {k: handed[k] for k in tensor_inputs})
            for key in self._callback_tensor_inputs:
                if outputs is not None and key in outputs and outputs[key] is not handed[key]:
                    raise LkgdHipError(f"{name}: `callback_on_step_end` returned a replaced `{key}` - the "
                                       "loop updates its tensors in place and takes none back (callbacks observe)")
            if self._interrupt:
                raise LkgdHipError(f"{name}: `interrupt` was set from `callback_on_step_end` - the loop "
                                   "cannot skip its remaining steps")
        return callback

    def _frames_out(self, latents, additional_frames: int, output_type: str, return_dict: bool):
        """the tail of ``__call__``: the padding frames leave (:907), decode, frames-out, the output object"""
        if not output_type == "latent":
            latents = latents[:, additional_frames:]
            video = self.decode_latents(latents)
            video = self.video_processor.postprocess_video(video=video, output_type=output_type)
        else:
            video = latents

        self.maybe_free_model_hooks()
        if not return_dict:
            return (video,)
        return CogVideoXPipelineOutput(frames=video)


class CogVideoXImageToVideoPipeline(_CogVideoXPipelineBase):
    _encoder_use = "image-to-video pipeline encodes its image"

    def __init__(self, tokenizer, text_encoder, vae, transformer, scheduler, domain_model=None, flow_model=None):
        super().__init__(tokenizer, text_encoder, vae, transformer, scheduler)
        self.domain_model, self.flow_model = domain_model, flow_model

    @property
    def components(self) -> Dict[str, Any]:
        return dict(super().components, domain_model=self.domain_model, flow_model=self.flow_model)

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=None, tokenizer=None, domain_model=None, flow_model=None):
        """a local checkpoint directory in diffusers' layout: ``model_index.json`` and ``text_encoder/``, ``vae/``, ``transformer/``,
        ``scheduler/``, each read by its own loader.  The VAE comes with its encoder (a ``vae/`` without ``encoder.*`` keys raises: an
        image-to-video pipeline encodes its image).  ``tokenizer``: the caller's; omitted, ``tokenizer/`` is read with transformers'
        ``T5Tokenizer`` where that can be imported, else it stays None (prompts as id tensors or ``prompt_embeds`` need none).  The domain
        and flow ViTs are the trainer's (lora_trainer.py:56-84), not the checkpoint's: arguments"""
        return cls(*cls._load_components(path, torch_dtype, tokenizer), domain_model, flow_model)

    # ---- the reference's class ----------------------------------------------------------------------------------------------------
    def prepare_latents(self, image, batch_size=1, num_channels_latents=16, num_frames=13, height=60, width=90, dtype=None, device=None,
                        generator=None, latents=None):
        """:354-427"""
        return cx.prepare_latents(self.vae, self.scheduler, self.transformer.config, image, batch_size, num_channels_latents, num_frames,
                                  height, width, dtype, device, generator, latents)

    def check_inputs(self, image, prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, latents=None,
                     prompt_embeds=None, negative_prompt_embeds=None):
        """:465-527, the same errors.  A prompt may also be an int64 id tensor (``encode_prompt``)"""
        if (not isinstance(image, torch.Tensor) and not (PIL is not None and isinstance(image, PIL.Image.Image))
                and not isinstance(image, list)):
            raise ValueError("`image` has to be of type `torch.Tensor` or `PIL.Image.Image` or `List[PIL.Image.Image]` but is"
                             f" {type(image)}")
        self._check_prompt_inputs(prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds,
                                  negative_prompt_embeds)

    def _not_built(self, timesteps, eta, attention_kwargs) -> None:
        super()._not_built(timesteps, eta, attention_kwargs)
        for name in ("domain_model", "flow_model"):
            if getattr(self, name) is None:
                raise LkgdHipError(f"{type(self).__name__}: `{name}` is missing - the transformer fuses its features into the "
                                   "text tokens at every call (pass it to the constructor or to from_pretrained)")

    @torch.no_grad()
    def __call__(self, image, prompt: Optional[Union[str, List[str]]] = None, negative_prompt: Optional[Union[str, List[str]]] = None,
                 height: Optional[int] = None, width: Optional[int] = None, num_frames: int = 49, num_inference_steps: int = 50,
                 timesteps: Optional[List[int]] = None, guidance_scale: float = 6, use_dynamic_cfg: bool = False,
                 num_videos_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 output_type: str = "pil", return_dict: bool = True, attention_kwargs: Optional[Dict[str, Any]] = None,
                 callback_on_step_end: Optional[Callable] = None, callback_on_step_end_tensor_inputs: List[str] = ["latents"],
                 max_sequence_length: int = 226):
        """:610-919, in its order.  The generator is consumed as there: the image posterior's sample(s), the initial noise, then the
        DPM steps' noise; a list of generators is one per batch entry"""
        if hasattr(callback_on_step_end, "tensor_inputs"):              # [EXT] PipelineCallback / MultiPipelineCallbacks
            callback_on_step_end_tensor_inputs = callback_on_step_end.tensor_inputs
        tc = self.transformer.config
        height = height or tc.sample_height * self.vae_scale_factor_spatial
        width = width or tc.sample_width * self.vae_scale_factor_spatial
        num_frames = num_frames or tc.sample_frames
        num_videos_per_prompt = 1                                                                   # :726

        # 1. Check inputs
        self.check_inputs(image=image, prompt=prompt, height=height, width=width, negative_prompt=negative_prompt,
                          callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, latents=latents,
                          prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds)
        self._not_built(timesteps, eta, attention_kwargs)
        self._begin_call(guidance_scale, attention_kwargs)

        # 2. Default call parameters
        batch_size = self._batch_size(prompt, prompt_embeds)
        device = self._execution_device
        do_classifier_free_guidance = guidance_scale > 1.0

        # 3. Encode input prompt; negative first in the concat (:772)
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt=prompt, negative_prompt=negative_prompt, do_classifier_free_guidance=do_classifier_free_guidance,
            num_videos_per_prompt=num_videos_per_prompt, prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
            max_sequence_length=max_sequence_length, device=device)
        if do_classifier_free_guidance:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)

        # 4. Prepare timesteps ([EXT] retrieve_timesteps without custom timesteps)
        self.scheduler.set_timesteps(num_inference_steps)
        step_times = self.scheduler.timesteps
        self._num_timesteps = len(step_times)

        # 5. Prepare latents; the 1.5 models pad the latent frames (:779-786)
        _, additional_frames, num_frames = additional_latent_frames(num_frames, self.vae_scale_factor_temporal, tc.patch_size_t)
        image = self.video_processor.preprocess(image, height=height, width=width, device=device, dtype=prompt_embeds.dtype)

        # the ViTs resize bilinearly to their own input size (lkgd_vit_patchify): :797's resize to 384 is theirs
        domain_features = self.domain_model(image).unsqueeze(1)
        flow_features = self.flow_model(image).unsqueeze(1)

        latent_channels = tc.in_channels // 2
        latents, image_latents = self.prepare_latents(image, batch_size * num_videos_per_prompt, latent_channels, num_frames, height,
                                                      width, prompt_embeds.dtype, device, generator, latents)

        # 7. Create rotary embeds if required
        image_rotary_emb = (self._prepare_rotary_positional_embeddings(height, width, latents.size(1), device)
                            if tc.use_rotary_positional_embeddings else None)

        # 8. Denoising loop (ofs: denoise embeds :826's 2.0 where the config asks for it)
        callback = self._step_callback(callback_on_step_end, callback_on_step_end_tensor_inputs, step_times, prompt_embeds,
                                       negative_prompt_embeds)
        latents = cx.denoise(self.transformer, self.scheduler, latents, image_latents, prompt_embeds, domain_features, flow_features,
                             num_inference_steps, guidance_scale, use_dynamic_cfg, callback, image_rotary_emb, None, generator)
        if use_dynamic_cfg:                                             # :864 leaves the last step's value behind
            self._guidance_scale = cx.dynamic_guidance(guidance_scale, num_inference_steps, int(step_times[-1]))
        self._current_timestep = None

        return self._frames_out(latents, additional_frames, output_type, return_dict)     # :905-919


class _StockTransformerPipeline(_CogVideoXPipelineBase):
    """what diffusers' text-to-video and video-to-video classes share beyond the base: the stock transformer - every latent channel is
    the loop's own, no feature models, no ``ofs``"""

    def _not_built(self, timesteps, eta, attention_kwargs) -> None:
        super()._not_built(timesteps, eta, attention_kwargs)
        if getattr(self.transformer.config, "ofs_embed_dim", None):
            raise LkgdHipError(f"{type(self).__name__}: the transformer has an `ofs_embed_dim` - an image-to-video model; this class "
                               "passes no `ofs` (use CogVideoXImageToVideoPipeline)")

    def _encode_and_concat(self, prompt, negative_prompt, guidance, num_videos_per_prompt, prompt_embeds, negative_prompt_embeds,
                           max_sequence_length, device):
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, negative_prompt, guidance, num_videos_per_prompt=num_videos_per_prompt, prompt_embeds=prompt_embeds,
            negative_prompt_embeds=negative_prompt_embeds, max_sequence_length=max_sequence_length, device=device)
        if guidance:                                                    # negative first, as in the reference's class
            return torch.cat([negative_prompt_embeds, prompt_embeds], dim=0), negative_prompt_embeds
        return prompt_embeds, negative_prompt_embeds

    def _loop(self, latents, prompt_embeds, negative_prompt_embeds, height, width, num_inference_steps, start_step, guidance_scale,
              use_dynamic_cfg, generator, callback_on_step_end, callback_on_step_end_tensor_inputs):
        """rotary tables, the callback, ``denoise`` without image latents and without the fuse, the properties it leaves behind"""
        tc = self.transformer.config
        step_times = self.scheduler.timesteps[start_step:]
        self._num_timesteps = len(step_times)
        image_rotary_emb = (self._prepare_rotary_positional_embeddings(height, width, latents.size(1))
                            if tc.use_rotary_positional_embeddings else None)
        callback = self._step_callback(callback_on_step_end, callback_on_step_end_tensor_inputs, step_times, prompt_embeds,
                                       negative_prompt_embeds)
        latents = cx.denoise(self.transformer, self.scheduler, latents, None, prompt_embeds, None, None, num_inference_steps,
                             guidance_scale, use_dynamic_cfg, callback, image_rotary_emb, None, generator, start_step=start_step)
        if use_dynamic_cfg:                                             # the last step's value stays behind, as in the I2V class
            self._guidance_scale = cx.dynamic_guidance(guidance_scale, num_inference_steps - start_step, int(step_times[-1]))
        self._current_timestep = None
        return latents


class CogVideoXPipeline(_StockTransformerPipeline):
    """[EXT diffusers pipelines/cogvideo/pipeline_cogvideox.py], parity unpinned: text-to-video (``generate_type == "t2v"`` of
    inference/cli_demo.py).  A decoder-only ``vae/`` is enough"""

    def prepare_latents(self, batch_size, num_channels_latents, num_frames, height, width, dtype, device, generator, latents=None):
        return cx.prepare_noise_latents(self.scheduler, self.transformer.config, self.vae.config, batch_size, num_channels_latents,
                                        num_frames, height, width, dtype, device, generator, latents)

    def check_inputs(self, prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds=None,
                     negative_prompt_embeds=None):
        self._check_prompt_inputs(prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds,
                                  negative_prompt_embeds)

    @torch.no_grad()
    def __call__(self, prompt: Optional[Union[str, List[str]]] = None, negative_prompt: Optional[Union[str, List[str]]] = None,
                 height: Optional[int] = None, width: Optional[int] = None, num_frames: Optional[int] = None,
                 num_inference_steps: int = 50, timesteps: Optional[List[int]] = None, guidance_scale: float = 6,
                 use_dynamic_cfg: bool = False, num_videos_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 output_type: str = "pil", return_dict: bool = True, attention_kwargs: Optional[Dict[str, Any]] = None,
                 callback_on_step_end: Optional[Callable] = None, callback_on_step_end_tensor_inputs: List[str] = ["latents"],
                 max_sequence_length: int = 226):
        """the generator is consumed by the initial noise, then by the DPM steps' noise; a list of generators is one per batch entry
        (``len(prompt) * num_videos_per_prompt`` of them).  ``num_videos_per_prompt`` repeats every prompt's embeddings"""
        if hasattr(callback_on_step_end, "tensor_inputs"):              # [EXT] PipelineCallback / MultiPipelineCallbacks
            callback_on_step_end_tensor_inputs = callback_on_step_end.tensor_inputs
        tc = self.transformer.config
        height = height or tc.sample_height * self.vae_scale_factor_spatial
        width = width or tc.sample_width * self.vae_scale_factor_spatial
        num_frames = num_frames or tc.sample_frames

        self.check_inputs(prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds,
                          negative_prompt_embeds)
        self._not_built(timesteps, eta, attention_kwargs)
        self._begin_call(guidance_scale, attention_kwargs)
        batch_size = self._batch_size(prompt, prompt_embeds)
        device = self._execution_device

        prompt_embeds, negative_prompt_embeds = self._encode_and_concat(
            prompt, negative_prompt, guidance_scale > 1.0, num_videos_per_prompt, prompt_embeds, negative_prompt_embeds,
            max_sequence_length, device)
        self.scheduler.set_timesteps(num_inference_steps)

        # the 1.5 models pad the latent frames in front, as the I2V class does
        _, additional_frames, num_frames = additional_latent_frames(num_frames, self.vae_scale_factor_temporal, tc.patch_size_t)
        latents = self.prepare_latents(batch_size * num_videos_per_prompt, tc.in_channels, num_frames, height, width,
                                       prompt_embeds.dtype, device, generator, latents)
        latents = self._loop(latents, prompt_embeds, negative_prompt_embeds, height, width, num_inference_steps, 0, guidance_scale,
                             use_dynamic_cfg, generator, callback_on_step_end, callback_on_step_end_tensor_inputs)
        return self._frames_out(latents, additional_frames, output_type, return_dict)


class CogVideoXVideoToVideoPipeline(_StockTransformerPipeline):
    """[EXT diffusers pipelines/cogvideo/pipeline_cogvideox_video2video.py], parity unpinned: video-to-video (``generate_type ==
    "v2v"`` of inference/cli_demo.py).  The clip is encoded, noised to the timestep ``strength`` selects, and the loop runs the rest of
    the schedule (``denoise(start_step=)``)"""
    _encoder_use = "video-to-video pipeline encodes its clip with the VAE's encoder"

    def get_timesteps(self, num_inference_steps, strength, device=None):
        timesteps, steps, _ = cx.get_timesteps(self.scheduler, num_inference_steps, strength)
        return timesteps, steps

    def prepare_latents(self, video=None, batch_size=1, num_channels_latents=16, height=60, width=90, dtype=None, device=None,
                        generator=None, latents=None, timestep=None):
        return cx.prepare_video_latents(self.vae, self.scheduler, video, batch_size, num_channels_latents, height, width, dtype, device,
                                        generator, latents, timestep)

    def _clip_length(self, video) -> int:
        """pixel frames of the clip(s) as given (a tensor / ndarray clip is laid out [T, C, H, W] / [T, H, W, C])"""
        return len(self.video_processor._clips(video)[0])

    def check_inputs(self, prompt, height, width, strength, negative_prompt, callback_on_step_end_tensor_inputs, video=None,
                     latents=None, prompt_embeds=None, negative_prompt_embeds=None, num_frames=None):
        """diffusers' errors, and two of this class: a ``num_frames`` that is not the clip's length (inference/cli_demo.py:183-194
        passes one), and a ``patch_size_t`` model whose latent frame count the temporal patch does not divide (diffusers' class does not
        pad)"""
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        self._check_prompt_inputs(prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds,
                                  negative_prompt_embeds)
        if video is not None and latents is not None:
            raise ValueError("Only one of `video` or `latents` should be provided")
        if video is None and latents is None:
            raise ValueError("Provide either `video` or `latents`. Cannot leave both undefined.")
        if video is not None:
            length = self._clip_length(video)
            if num_frames is not None and num_frames != length:
                raise ValueError(f"`num_frames`={num_frames} differs from the {length} frames of `video`; the clip decides")
            latent_frames = (length - 1) // self.vae_scale_factor_temporal + 1
        else:
            latent_frames = latents.shape[1]
        p_t = self.transformer.config.patch_size_t
        if p_t is not None and latent_frames % p_t != 0:
            raise ValueError(f"`patch_size_t`={p_t} does not divide the {latent_frames} latent frames of the clip; the video-to-video "
                             "class does not pad - pass a clip whose latent frame count it divides")

    @torch.no_grad()
    def __call__(self, video=None, prompt: Optional[Union[str, List[str]]] = None,
                 negative_prompt: Optional[Union[str, List[str]]] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_frames: Optional[int] = None, num_inference_steps: int = 50, timesteps: Optional[List[int]] = None,
                 strength: float = 0.8, guidance_scale: float = 6, use_dynamic_cfg: bool = False, num_videos_per_prompt: int = 1,
                 eta: float = 0.0, generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil", return_dict: bool = True,
                 attention_kwargs: Optional[Dict[str, Any]] = None, callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 226):
        """the generator is consumed by the clips' posterior samples, the noise, then the DPM steps' noise; a list of generators is
        one per batch entry.  ``num_videos_per_prompt`` repeats every prompt's embeddings and its clip"""
        if hasattr(callback_on_step_end, "tensor_inputs"):              # [EXT] PipelineCallback / MultiPipelineCallbacks
            callback_on_step_end_tensor_inputs = callback_on_step_end.tensor_inputs
        tc = self.transformer.config
        height = height or tc.sample_height * self.vae_scale_factor_spatial
        width = width or tc.sample_width * self.vae_scale_factor_spatial

        self.check_inputs(prompt=prompt, height=height, width=width, strength=strength, negative_prompt=negative_prompt,
                          callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, video=video, latents=latents,
                          prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, num_frames=num_frames)
        self._not_built(timesteps, eta, attention_kwargs)
        self._begin_call(guidance_scale, attention_kwargs)
        batch_size = self._batch_size(prompt, prompt_embeds)
        device = self._execution_device

        prompt_embeds, negative_prompt_embeds = self._encode_and_concat(
            prompt, negative_prompt, guidance_scale > 1.0, num_videos_per_prompt, prompt_embeds, negative_prompt_embeds,
            max_sequence_length, device)
        self.scheduler.set_timesteps(num_inference_steps)
        step_times, _, t_start = cx.get_timesteps(self.scheduler, num_inference_steps, strength)
        latent_timestep = step_times[:1].repeat(batch_size * num_videos_per_prompt)

        if latents is None:
            video = self.video_processor.preprocess_video(video, height=height, width=width, device=device, dtype=prompt_embeds.dtype)
            if num_videos_per_prompt != 1:
                video = video.repeat_interleave(num_videos_per_prompt, dim=0)
        latents = self.prepare_latents(video, batch_size * num_videos_per_prompt, tc.in_channels, height, width, prompt_embeds.dtype,
                                       device, generator, latents, latent_timestep)
        latents = self._loop(latents, prompt_embeds, negative_prompt_embeds, height, width, num_inference_steps, t_start,
                             guidance_scale, use_dynamic_cfg, generator, callback_on_step_end, callback_on_step_end_tensor_inputs)
        return self._frames_out(latents, 0, output_type, return_dict)

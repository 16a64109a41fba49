"""DDIM inversion and reference-guided sampling for CogVideoX on the MI355X path: the reference's
``CogVideo-main/inference/ddim_inversion.py`` with its names and keywords.

The script encodes a clip (``get_video_frames`` :263-300, ``encode_video_frames`` :303-309), walks its latents UP the noise schedule
with diffusers' ``DDIMInverseScheduler`` (``sample`` :321-452), and samples back down with the pipeline's scheduler while every
block's attention also reads the keys and values of the recorded inversion trajectory
(``CogVideoXAttnProcessor2_0ForDDIMInversion`` :118-243, installed by ``OverrideAttnProcessors`` :246-260); ``ddim_inversion``
:455-514 strings the stages together.

Nothing here launches a kernel of its own.  The per-step hot path is the loop's three launches, in two regimes:

* the attention of a [sample, reference] PAIR is ``lkgd_attn_spatial_qk`` on row windows of the q / k / v / out buffers of the whole
  batch (``CogVideoXBlock.run``: ``nbatch`` 1, Sq = L queries against the S = 2L adjacent key rows of the pair) - K and V are never
  copied or concatenated;
* both schedulers' updates are ``lkgd_dit_cfg_ddim_step``: the inverse step as the linear form ``x' = A x + M n`` passed as
  ``(a, b, sqrt_alpha, sqrt_beta) = (A, -M, 0, 1)`` (``DDIMInverseScheduler.coefficients``).

**[EXT], parity unpinned**: ``DDIMInverseScheduler`` restates diffusers' class from its published source, and the processor's
semantics are restated from the script; neither was ever executed here (diffusers is not installable next to this package).

Not built (each raises, naming itself): bf16, decord / mp4 I/O (``export_to_video``), ``CogVideoXDPMScheduler`` in ``sample``,
``eta != 0``, ``attention_kwargs``, the 1.5 (``patch_size_t``) models, frame sharding, the FP8 mode under reference attention."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch

from . import cogvideox as cx
from . import ops
from ._lib import LkgdHipError
from .image_processor import PIL


# ------------------------------------------------------------------------------------------------ the inverse scheduler
class DDIMInverseScheduler:
    """**[EXT diffusers scheduling_ddim_inverse.py], parity unpinned.**  Constructed as the script does (:489),
    ``DDIMInverseScheduler(**pipeline.scheduler.config)``, from the config of a ``CogVideoXDDIMScheduler``.

    Tables in fp64 on the host: scaled-linear betas with the zero-terminal-SNR rescale.  ``snr_shift_scale`` is IGNORED - diffusers'
    class has no such parameter and swallows the key in ``**kwargs`` - so the table equals ``_CogVideoXSchedule(snr_shift_scale=1.0)``:
    for the 5B config (1.0) that is the forward scheduler's table, for the 2B config (3.0) it is NOT (a quirk of the script,
    reproduced; the script is documented for the 5B models only).

    ``set_timesteps(n)``: ``round(arange(N, 0, -N / n)[::-1]) - 1``, ascending (n = 50: 19, 39, ..., 999).
    ``step(model_output, timestep, sample)`` moves the sample from ``cur = min(timestep - N // n, N - 1)`` to ``timestep`` - the
    integer ``N // n`` beside the fractional spacing is diffusers', and the model is evaluated at ``timestep`` while the sample sits at
    ``cur`` (both reproduced).  ``clip_sample=True``, a ``prediction_type`` other than ``v_prediction``, a spacing other than
    ``trailing`` and ``set_alpha_to_one=False`` raise, naming the key."""
    order = 1
    init_noise_sigma = 1.0
    step_kind = "ddim"        # ``cogvideox.denoise`` runs ``lkgd_dit_cfg_ddim_step`` on ``coefficients(t)``

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", clip_sample: bool = True, set_alpha_to_one: bool = True,
                 prediction_type: str = "epsilon", timestep_spacing: str = "leading", rescale_betas_zero_snr: bool = False, **kwargs):
        built = dict(clip_sample=False, prediction_type="v_prediction", timestep_spacing="trailing", set_alpha_to_one=True,
                     beta_schedule="scaled_linear", rescale_betas_zero_snr=True)
        got = dict(clip_sample=clip_sample, prediction_type=prediction_type, timestep_spacing=timestep_spacing,
                   set_alpha_to_one=set_alpha_to_one, beta_schedule=beta_schedule, rescale_betas_zero_snr=rescale_betas_zero_snr)
        for key, want in built.items():
            if got[key] != want:
                raise LkgdHipError(f"DDIMInverseScheduler: {key}={got[key]!r}; only {key}={want!r} is built")
        # snr_shift_scale (in kwargs when the config is a CogVideoX scheduler's) takes no part
        table = cx._CogVideoXSchedule(num_train_timesteps, beta_start, beta_end, snr_shift_scale=1.0)
        self.alphas_cumprod = table.alphas_cumprod
        self.initial_alpha_cumprod = torch.tensor(1.0, dtype=torch.float64)
        self.config = cx.SchedulerConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                         _class_name=type(self).__name__, **built)
        self.timesteps = None
        self.num_inference_steps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = self.config.num_train_timesteps
        if num_inference_steps > n:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `num_train_timesteps`: {n}")
        self.num_inference_steps = num_inference_steps
        steps = np.round(np.arange(n, 0, -n / num_inference_steps)[::-1]).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(steps.copy())

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _alpha_pair(self, t: int):
        """(alphas_cumprod where the sample sits, alphas_cumprod of the step's target ``t``, the sample's timestep), fp64"""
        n = self.config.num_train_timesteps
        cur = min(t - n // self.num_inference_steps, n - 1)
        at = self.alphas_cumprod[cur] if cur >= 0 else self.initial_alpha_cumprod
        return at, self.alphas_cumprod[t], cur

    def linear_coefficients(self, t: int):
        """(A, M) of ``x' = A x + M n``, fp64: with x0 = sqrt(at) x - sqrt(1 - at) n and e = sqrt(at) n + sqrt(1 - at) x, the step
        ``x' = sqrt(ap) x0 + sqrt(1 - ap) e`` collects to A = sqrt(ap at) + sqrt((1 - ap)(1 - at)), M = sqrt((1 - ap) at) -
        sqrt(ap (1 - at)).  The forward scheduler's (a, b) form divides by 1 - at, which is 0 on the first inverse step (at = 1)"""
        at, ap, _ = self._alpha_pair(int(t))
        A = (ap * at) ** 0.5 + ((1 - ap) * (1 - at)) ** 0.5
        M = ((1 - ap) * at) ** 0.5 - (ap * (1 - at)) ** 0.5
        return float(A), float(M)

    def coefficients(self, t: int):
        """what ``ops.dit_cfg_ddim_step`` takes, (a, b, sqrt_alpha, sqrt_beta) = (A, -M, 0, 1): the kernel's x0' = 0 x - 1 n = -n
        exactly, and x' = A x + (-M)(-n)"""
        A, M = self.linear_coefficients(t)
        return A, -M, 0.0, 1.0

    def step(self, model_output, timestep, sample, return_dict: bool = False, **kwargs):
        """the fp32 statements of the kernel in ATen, ``fl(fl(A x) + fl(M n))`` -> (prev_sample,)"""
        if kwargs:
            raise LkgdHipError(f"DDIMInverseScheduler.step: {sorted(kwargs)} - the inverse scheduler accepts no extra step kwargs")
        if return_dict:
            raise LkgdHipError("DDIMInverseScheduler.step: return_dict=True is not built (the script passes False)")
        A, M = self.linear_coefficients(int(timestep))
        return (A * sample.float() + M * model_output.float(),)


# ------------------------------------------------------------------------------------------------ reference attention
class CogVideoXAttnProcessor2_0ForDDIMInversion(cx.CogVideoXAttnProcessor2_0):
    """:118-243 as a marker.  A block whose ``attn1`` holds it treats the batch as [sample entries | reference entries] (:212-215): a
    sample entry's queries attend the keys / values of its own L rows followed by its reference entry's L rows (:219-220), each group
    q/k-normalised and rotated with its own positions (:156-165); a reference entry attends itself (:228-238).  The launches are
    ``CogVideoXBlock.run``'s (lkgd_amd/cogvideox.py)"""
    reference_attention = True


class OverrideAttnProcessors:
    """:246-260: installs the marker on every block's ``attn1`` and puts the original processors back on exit (an exception
    included).  The packed weights do not change: nothing is re-packed"""

    def __init__(self, transformer):
        self.transformer = transformer
        self.original_processors = {}

    def __enter__(self):
        for block in self.transformer.transformer_blocks:
            self.original_processors[id(block)] = block.attn1.get_processor()
            block.attn1.set_processor(CogVideoXAttnProcessor2_0ForDDIMInversion())

    def __exit__(self, _0, _1, _2):
        for block in self.transformer.transformer_blocks:
            block.attn1.set_processor(self.original_processors[id(block)])


def reference_attention_installed(transformer) -> bool:
    return any(b.attn1.get_processor().reference_attention for b in transformer.transformer_blocks)


# ------------------------------------------------------------------------------------------------ frames in
def select_frame_indices(video_num_frames: int, skip_frames_start: int, skip_frames_end: int, max_num_frames: int,
                         frame_sample_step: Optional[int]) -> List[int]:
    """:274-300's selection -> the indices of the frames the clip keeps: the window, subsampled when longer than ``max_num_frames``
    (``frame_sample_step`` or ``(end - start) // max_num_frames``), cut to ``max_num_frames``, then to its first 4k + 1 frames"""
    first, stop = min(skip_frames_start, video_num_frames), max(0, video_num_frames - skip_frames_end)
    span = stop - first
    if span <= 0:
        picked = [first]                        # an empty window still asks for the frame at its start (:278-279)
    else:
        stride = 1 if span <= max_num_frames else (frame_sample_step or span // max_num_frames)
        picked = list(range(first, stop, stride))
    picked = picked[:max_num_frames]            # :287
    keep = len(picked) - (len(picked) + 3) % 4  # the first 4k + 1 of them (:289-294)
    assert keep % 4 == 1
    return picked[:keep]


def get_video_frames(video_path, width: int, height: int, skip_frames_start: int, skip_frames_end: int, max_num_frames: int,
                     frame_sample_step: Optional[int], device=None) -> torch.Tensor:
    """:263-300 -> [F, C, H, W], normalised to [-1, 1].  ``video_path``: a path (read with decord, which has to import - otherwise it
    raises, naming decord), or the clip itself in memory: uint8 [N, H, W, 3] (tensor / ndarray) or a list of PIL images, already at
    ``width`` x ``height`` (anything else raises: the resize is decord's).
    ``device`` None: the script's host statement ``x / 255.0 * 2.0 - 1.0``, fp32.  A GPU ``device``: the selected uint8 frames are
    uploaded and normalised by the frames-in launch the video-to-video pipeline uses (``lkgd_image_preprocess``) into fp16 - the same
    fp32 statements rounded once, i.e. the bits of the host result's ``.half()`` (which ``encode_video_frames`` takes next)"""
    if isinstance(video_path, (str, bytes)) or hasattr(video_path, "__fspath__"):
        try:
            import decord
        except ImportError as e:
            raise LkgdHipError(f"get_video_frames({video_path!r}): reading a video file needs decord, which is not installed; pass "
                               "the clip in memory instead (uint8 [N, H, W, 3] or a list of PIL images)") from e
        with decord.bridge.use_torch():
            reader = decord.VideoReader(uri=video_path, width=width, height=height)
            indices = select_frame_indices(len(reader), skip_frames_start, skip_frames_end, max_num_frames, frame_sample_step)
            clip = reader.get_batch(indices=indices)
        indices = list(range(len(indices)))
    else:
        clip = video_path
        if isinstance(clip, (list, tuple)) and clip and PIL is not None and all(isinstance(f, PIL.Image.Image) for f in clip):
            clip = np.stack([np.asarray(f.convert("RGB")) for f in clip], axis=0)
        if isinstance(clip, np.ndarray):
            clip = torch.from_numpy(np.ascontiguousarray(clip))
        if not torch.is_tensor(clip) or clip.dtype != torch.uint8 or clip.dim() != 4 or clip.shape[3] != 3:
            raise LkgdHipError("get_video_frames: an in-memory clip must be uint8 [N, H, W, 3] or a list of PIL images, got "
                               f"{type(video_path).__name__}"
                               + (f" {clip.dtype} {tuple(clip.shape)}" if torch.is_tensor(clip) else ""))
        if tuple(clip.shape[1:3]) != (height, width):
            raise LkgdHipError(f"get_video_frames: the in-memory clip is {clip.shape[2]} x {clip.shape[1]} (width x height), asked for "
                               f"{width} x {height}; the resize is decord's and is not built")
        indices = select_frame_indices(clip.shape[0], skip_frames_start, skip_frames_end, max_num_frames, frame_sample_step)
    frames = clip[torch.as_tensor(indices, dtype=torch.int64, device=clip.device)]
    if device is not None and torch.device(device).type == "cuda":
        return ops.image_preprocess(frames.contiguous().to(device))                       # [F, 3, H, W] fp16
    frames = frames.float() / 255.0 * 2.0 - 1.0
    return frames.permute(0, 3, 1, 2).contiguous()


@torch.no_grad()
def encode_video_frames(vae, video_frames: torch.Tensor, generator=None) -> torch.Tensor:
    """:303-309: [F, C, H, W] -> ``vae.encode(...).latent_dist.sample()`` [1, f, c, h, w] times ``scaling_factor`` (the fp16 product of
    the script, after the sample is rounded).  ``generator`` None draws from the global RNG, as the script does"""
    video_frames = video_frames.to(device=vae.device, dtype=vae.dtype)
    video_frames = video_frames.unsqueeze(0).permute(0, 2, 1, 3, 4)                        # [B, C, F, H, W]
    latent_dist = vae.encode(video_frames.contiguous()).latent_dist.sample(generator).transpose(1, 2)
    return latent_dist * vae.config.scaling_factor


def export_latents_to_video(pipeline, latents: torch.Tensor, video_path: Optional[str] = None, fps: int = 8):
    """:312-317 without the mp4: decodes and post-processes -> the clip's PIL frames.  A ``video_path`` raises: ``export_to_video``
    is not built"""
    if video_path is not None:
        raise LkgdHipError(f"export_latents_to_video({video_path!r}): `export_to_video` (mp4 output) is not built; call it without a "
                           "path and write the returned frames yourself")
    video = pipeline.decode_latents(latents)
    frames = pipeline.video_processor.postprocess_video(video=video, output_type="pil")
    return frames[0]


# ------------------------------------------------------------------------------------------------ the loop
def _check_dtype(dtype, where: str) -> None:
    if dtype in ("bf16", "bfloat16", torch.bfloat16):
        raise LkgdHipError(f"{where}: bf16 is not built - fp16 is the only dtype of the HIP path")
    if dtype not in (None, "fp16", "float16", torch.float16):
        raise LkgdHipError(f"{where}: dtype={dtype!r}; fp16 is the only dtype of the HIP path")


class _ReferencePlacement(cx.LoopPlacement):
    """``sample`` with ``reference_latents``: the batch doubles into pairs, entry 2j a sample and 2j + 1 its reference, and the text
    of a pair is the sample's (:355-356, :396-399).  ``keep_samples``: no reference attention is installed, so ``forward_rows``
    returns every entry's rows - plain attention over the doubled batch - and the reference entries' are discarded, as the script
    does"""

    def __init__(self, reference_latents, keep_samples: bool):
        self.reference_latents, self.keep_samples = reference_latents, keep_samples

    def rows(self, i, latents, img, out, p, **glue):
        reference = self.reference_latents[i].to(device=latents.device, dtype=torch.float16).contiguous()
        if tuple(reference.shape) != tuple(latents.shape):
            raise ValueError(f"sample: reference_latents[{i}] is {tuple(reference.shape)}, the latents {tuple(latents.shape)}")
        Bl, Fr, C, H, W = latents.shape
        self.Tv = Fr * (H // p) * (W // p)
        if out is None:
            out = torch.empty(2 * Bl * self.Tv, C * p * p, dtype=torch.float16, device=latents.device)
        for j in range(Bl):                 # [sample j | reference j]: the rows ``forward_rows`` embeds for both CFG entries
            ops.dit_patch_rows(latents[j:j + 1], None, p, out=out[2 * j * self.Tv:(2 * j + 1) * self.Tv])
            ops.dit_patch_rows(reference[j:j + 1], None, p, out=out[(2 * j + 1) * self.Tv:(2 * j + 2) * self.Tv])
        return out

    def text(self, text):
        return text.repeat_interleave(2, dim=0)

    def noise(self, noise_rows):
        if not self.keep_samples:
            return noise_rows
        entries = noise_rows.shape[0] // self.Tv            # [u, ref_u, c, ref_c]: keep the even ones
        return noise_rows.view(entries, self.Tv, -1)[0::2].reshape(entries // 2 * self.Tv, -1)


@torch.no_grad()
def sample(pipeline, latents: torch.Tensor, scheduler, prompt: Optional[Union[str, List[str]]] = None,
           negative_prompt: Optional[Union[str, List[str]]] = None, num_inference_steps: int = 50, guidance_scale: float = 6,
           use_dynamic_cfg: bool = False, eta: float = 0.0, generator=None, attention_kwargs: Optional[Dict[str, Any]] = None,
           reference_latents=None) -> torch.Tensor:
    """:321-452, "modified from CogVideoXPipeline.__call__" -> the trajectory [steps, B, F, C, h, w] fp16, whose last entry is the
    final latents.  The loop is ``cogvideox.denoise`` on the stock transformer (no image latents, no latent-knowledge fuse); per step:
    ``ops.dit_patch_rows`` for the latents (and for ``reference_latents[i]`` when given: ``_ReferencePlacement``), ``forward_rows``,
    ``ops.dit_cfg_ddim_step`` with ``scheduler.coefficients(t)``, one device copy into ``trajectory[i]``.  The prompt is encoded and
    the rotary tables are built once per clip; dynamic guidance is the script's ``num_inference_steps - t`` (:420-430); the update runs
    in fp32 and is cast back to fp16 every step (:414, :441).
    ``scheduler``: a ``DDIMInverseScheduler`` (its timesteps ascend) or a ``CogVideoXDDIMScheduler``.  ``reference_latents``: a tensor
    [steps, B, F, C, h, w] or anything indexable per step (``reversed(tensor)`` is read as the flipped tensor).  With
    ``reference_latents`` the batch doubles (:355-356, :396-399): under ``OverrideAttnProcessors`` the sample entries attend their
    references' keys and values; without it the script runs plain attention over the doubled batch and discards the reference half,
    which is reproduced.  ``generator`` is accepted and unused: with eta 0 neither scheduler draws.
    ``CogVideoXDPMScheduler``, ``eta != 0``, ``attention_kwargs``, bf16 latents and a ``patch_size_t`` model raise."""
    dit = pipeline.transformer
    tc = dit.config
    if isinstance(scheduler, cx.CogVideoXDPMScheduler):
        raise LkgdHipError("sample: CogVideoXDPMScheduler is not built here - the script's loop has no `old_pred_original_sample`; use "
                           "CogVideoXDDIMScheduler (or DDIMInverseScheduler)")
    if not isinstance(scheduler, (DDIMInverseScheduler, cx.CogVideoXDDIMScheduler)):
        raise LkgdHipError(f"sample: scheduler is a {type(scheduler).__qualname__}; built: DDIMInverseScheduler, CogVideoXDDIMScheduler")
    if eta != 0.0:
        raise LkgdHipError(f"sample: `eta`={eta} is not built - both steps are the eta = 0 ones")
    if attention_kwargs is not None:
        raise LkgdHipError("sample: `attention_kwargs` are not built - the attention processors are markers and take none")
    if latents.dtype == torch.bfloat16:
        _check_dtype(latents.dtype, "sample")
    if tc.patch_size_t is not None:
        raise LkgdHipError(f"sample: patch_size_t={tc.patch_size_t} (CogVideoX 1.5) is not built for DDIM inversion")
    guided = reference_attention_installed(dit)
    if guided and not tc.use_rotary_positional_embeddings:
        raise NotImplementedError("This script supports CogVideoX 5B model only.")                # :477-478
    if guided and reference_latents is None:
        raise LkgdHipError("sample: reference attention is installed (OverrideAttnProcessors) but no `reference_latents` are given: "
                           "the batch has no reference entries (an odd batch of [sample | reference] entries)")
    pipeline._guidance_scale = guidance_scale
    pipeline._attention_kwargs = attention_kwargs
    pipeline._interrupt = False
    device = pipeline._execution_device
    do_classifier_free_guidance = guidance_scale > 1.0

    # 3. Encode input prompt (:347-356)
    prompt_embeds, negative_prompt_embeds = pipeline.encode_prompt(prompt, negative_prompt, do_classifier_free_guidance, device=device)
    if do_classifier_free_guidance:
        prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
    # 4. timesteps (:359-360)
    scheduler.set_timesteps(num_inference_steps)
    timesteps = scheduler.timesteps.tolist()
    pipeline._num_timesteps = len(timesteps)
    # 5. latents (:363)
    latents = latents.to(device=device) * scheduler.init_noise_sigma
    ncfg = 2 if do_classifier_free_guidance else 1
    if prompt_embeds.shape[0] != ncfg * latents.shape[0]:
        raise ValueError(f"sample: {prompt_embeds.shape[0]} prompt embeddings for {latents.shape[0]} latents under cfg x{ncfg}")
    place = cx.LoopPlacement()
    if reference_latents is not None:
        if isinstance(reference_latents, reversed):            # the script hands ``reversed(inverse_latents)`` (:508)
            reference_latents = list(reference_latents)
        if len(reference_latents) != len(timesteps):
            raise ValueError(f"sample: {len(reference_latents)} reference latents for {len(timesteps)} steps")
        place = _ReferencePlacement(reference_latents, keep_samples=not guided)
    # 7. rotary tables, once per clip (:373-382)
    rope = None
    if tc.use_rotary_positional_embeddings:
        rope = pipeline._prepare_rotary_positional_embeddings(height=latents.size(3) * pipeline.vae_scale_factor_spatial,
                                                              width=latents.size(4) * pipeline.vae_scale_factor_spatial,
                                                              num_frames=latents.size(1), device=device)
    # 8. the loop (:387-447): ``cogvideox.denoise`` on the stock transformer, one device copy per step into the trajectory
    trajectory = torch.zeros((len(timesteps),) + tuple(latents.shape), dtype=torch.float16, device=device)
    place.after_step = lambda i, t, x: trajectory[i].copy_(x)
    cx.denoise(dit, scheduler, latents, None, prompt_embeds, None, None, num_inference_steps, guidance_scale, use_dynamic_cfg,
               image_rotary_emb=rope, _placement=place)
    if use_dynamic_cfg:                         # what the script's loop leaves in ``pipeline.guidance_scale``: the last step's
        pipeline._guidance_scale = cx.dynamic_guidance(guidance_scale, num_inference_steps, timesteps[-1])
    pipeline.maybe_free_model_hooks()
    return trajectory


@torch.no_grad()
def ddim_inversion(model_path, prompt: str, video_path, output_path: Optional[str] = None, guidance_scale: float = 6.0,
                   num_inference_steps: int = 50, skip_frames_start: int = 0, skip_frames_end: int = 0,
                   frame_sample_step: Optional[int] = None, max_num_frames: int = 81, width: int = 720, height: int = 480, fps: int = 8,
                   dtype=torch.float16, seed: int = 42, device="cuda"):
    """:455-514 with the script's keywords.  ``model_path``: a checkpoint directory, or the ``CogVideoXPipeline`` object itself;
    ``video_path``: a path (decord) or an in-memory clip (``get_video_frames``).  Returns ``(inverse_latents, recon_latents,
    inversion_frames, reconstruction_frames)``: the two trajectories and the PIL frames of their last entries - the script writes those
    as ``<name>_inversion.mp4`` / ``<name>_reconstruction.mp4``; here an ``output_path`` raises (``export_to_video`` is not built).
    ``dtype`` bf16 raises.  The seed's generator is handed to ``sample`` (which draws nothing); the reconstruction's start noise and the
    posterior sample come from the global RNG, as in the script (:502, :308)"""
    from .pipeline_cogvideox import CogVideoXPipeline
    _check_dtype(dtype, "ddim_inversion")
    if output_path is not None:
        raise LkgdHipError(f"ddim_inversion(output_path={output_path!r}): `export_to_video` (mp4 output) is not built; the frames are "
                           "returned")
    if isinstance(model_path, (str, bytes)) or hasattr(model_path, "__fspath__"):
        pipeline = CogVideoXPipeline.from_pretrained(model_path, torch_dtype=torch.float16).to(device)
    else:
        pipeline = model_path
    if not pipeline.transformer.config.use_rotary_positional_embeddings:
        raise NotImplementedError("This script supports CogVideoX 5B model only.")
    device = pipeline._execution_device
    frames = get_video_frames(video_path, width, height, skip_frames_start, skip_frames_end, max_num_frames, frame_sample_step,
                              device=device)
    video_latents = encode_video_frames(pipeline.vae, frames)
    steps = dict(num_inference_steps=num_inference_steps, guidance_scale=guidance_scale)

    def seeded():
        return torch.Generator(device=device).manual_seed(seed)
    # up the schedule with the empty prompt (:489-498) ...
    inverse_latents = sample(pipeline, video_latents, DDIMInverseScheduler(**pipeline.scheduler.config), prompt="", generator=seeded(),
                             **steps)
    # ... and back down from fresh noise, every block reading the trajectory's keys and values in reverse order (:499-509)
    with OverrideAttnProcessors(pipeline.transformer):
        recon_latents = sample(pipeline, torch.randn_like(video_latents), pipeline.scheduler, prompt=prompt, generator=seeded(),
                               reference_latents=reversed(inverse_latents), **steps)
    inversion_frames = export_latents_to_video(pipeline, inverse_latents[-1], None, fps)
    reconstruction_frames = export_latents_to_video(pipeline, recon_latents[-1], None, fps)
    return inverse_latents, recon_latents, inversion_frames, reconstruction_frames

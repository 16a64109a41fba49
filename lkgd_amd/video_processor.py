"""Frames in and frames out of the CogVideoX pipelines: diffusers' ``VideoProcessor`` **[EXT diffusers `video_processor.py`, not vendored
by the reference; parity unpinned]** as far as the reference's ``__call__`` uses it - ``preprocess(image, height, width)``
(pipeline_cogvideox_image2video.py:788) and ``postprocess_video(video, output_type)`` (:909) - on top of
:class:`lkgd_amd.image_processor.VaeImageProcessor`, whose host arithmetic stays what it is.  Where the data is, or is headed, on the
GPU the arithmetic is one launch of include/lkgd_hip_video.h:

* ``postprocess_video`` of a GPU clip: ``lkgd_video_postprocess`` writes the uint8 (``pil``), fp32 (``np``) or fp16 (``pt``) frames in
  their final layout, and one device -> host copy brings the ``pil`` / ``np`` result over - 1 or 4 bytes per value instead of the
  clip's fp32 copy and four host passes over it;
* ``preprocess`` of PIL images for a GPU pipeline in fp16: PIL's lanczos resize stays on the host, the uint8 pixels are uploaded (a
  quarter of the fp32 image) and ``lkgd_image_preprocess`` normalises them into planar fp16 - bit for bit the host chain followed by the
  pipeline's ``.to(dtype=torch.float16)``.

Everything else - CPU tensors, numpy and tensor inputs, another dtype - takes the host form."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from ._lib import LkgdHipError
from .image_processor import PIL, VaeImageProcessor, tensor2vid


class VideoProcessor(VaeImageProcessor):
    def preprocess(self, image, height: Optional[int] = None, width: Optional[int] = None, device=None, dtype=None) -> torch.Tensor:
        """``VaeImageProcessor.preprocess``; with ``device`` / ``dtype`` the result is ``.to(device, dtype)`` of it, as the pipeline
        casts it at :788-790.  PIL images (or a list of them) headed for a GPU in fp16 are normalised there, from their uint8 pixels"""
        device = torch.device(device) if device is not None else None
        images = image if isinstance(image, list) else [image]
        is_pil = PIL is not None and bool(images) and all(isinstance(i, PIL.Image.Image) for i in images)
        if is_pil and device is not None and device.type == "cuda" and dtype == torch.float16 and self.config.do_normalize:
            if self.config.do_resize:
                height, width = self.get_default_height_width(images[0], height, width)
                images = [self.resize(i, height, width) for i in images]
            pixels = [np.asarray(i) for i in images]
            if all(p.dtype == np.uint8 and p.ndim in (2, 3) for p in pixels):      # other PIL modes (I;16, F, 1): the host chain
                u = np.stack([p[..., None] if p.ndim == 2 else p for p in pixels], axis=0)
                return ops.image_preprocess(torch.from_numpy(np.ascontiguousarray(u)).to(device))
        out = super().preprocess(image, height, width)
        return out if device is None and dtype is None else out.to(device=device, dtype=dtype)

    def postprocess_video(self, video: torch.Tensor, output_type: str = "np"):
        """[B, C, T, H, W] -> ``pil``: a list of B lists of T PIL frames; ``np``: fp32 [B, T, H, W, C]; ``pt``: [B, T, C, H, W].  A
        CPU clip takes ``tensor2vid``; a GPU clip (fp16, C <= 4) is one launch and, for ``pil`` / ``np``, one copy of the result"""
        if not isinstance(video, torch.Tensor) or not video.is_cuda or not self.config.do_normalize:
            return tensor2vid(video, self, output_type)
        if output_type not in ("np", "pt", "pil"):
            raise ValueError(f"{output_type} does not exist. Please choose one of ['np', 'pt', 'pil']")
        if video.dim() != 5 or video.dtype != torch.float16:
            raise LkgdHipError(f"postprocess_video: a GPU clip must be fp16 [B, C, T, H, W] (what decode_latents returns), got "
                               f"{video.dtype} {tuple(video.shape)}")
        video = video.contiguous()
        if output_type == "pt":
            return ops.video_postprocess(video, ops.VIDEO_F16)
        if output_type == "np":
            return ops.video_postprocess(video, ops.VIDEO_F32).cpu().numpy()
        frames = ops.video_postprocess(video, ops.VIDEO_U8).cpu().numpy()
        if frames.shape[-1] == 1:
            return [[PIL.Image.fromarray(f.squeeze(-1), mode="L") for f in clip] for clip in frames]
        return [[PIL.Image.fromarray(f) for f in clip] for clip in frames]

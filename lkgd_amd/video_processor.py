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
  pipeline's ``.to(dtype=torch.float16)``;
* ``preprocess_video`` (the video-to-video pipeline's clip) of PIL frames for a GPU pipeline in fp16: the same kernel, one launch per
  clip.  The clip's uint8 frames [T, H, W, C] are the kernel's image [1, T * H, W, C], whose planar result [1, C, T * H, W] IS the clip
  [C, T, H, W]: no permute copy.  The kernel's conditions admit the view: T * H is an ``int32`` height like any other, and the wide
  path asks for (T * H) * W % 8 == 0 - otherwise, and for a batch entry whose plane is not 16 bytes aligned, the one-pixel path
  writes the same bits.

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

    def preprocess_video(self, video, height: Optional[int] = None, width: Optional[int] = None, device=None, dtype=None) -> torch.Tensor:
        """[EXT diffusers ``VideoProcessor.preprocess_video``], parity unpinned: a list of PIL frames (one clip), a list of such lists,
        a 5-D tensor / ndarray [B, T, C, H, W] (ndarray: [B, T, H, W, C]), a 4-D one (one clip) or a list of 4-D ones -> [B, C, T, H, W]
        = ``torch.stack([self.preprocess(clip, height, width) for clip in clips]).permute(0, 2, 1, 3, 4)``; with ``device`` / ``dtype``
        the ``.to(device, dtype)`` of it.  PIL clips headed for a GPU in fp16: PIL's resize per frame on the host, the clip's uint8
        frames [T, H, W, C] uploaded once, and one launch of ``lkgd_image_preprocess`` per clip on the view [1, T * H, W, C], which
        writes [1, C, T * H, W] - the planar [C, T, H, W] clip in place, without a permute copy"""
        device = torch.device(device) if device is not None else None
        clips = self._clips(video)
        is_pil = PIL is not None and all(isinstance(f, PIL.Image.Image) for clip in clips for f in clip)
        if is_pil and device is not None and device.type == "cuda" and dtype == torch.float16 and self.config.do_normalize:
            pixels = []
            for clip in clips:
                if self.config.do_resize:
                    h, w = self.get_default_height_width(clip[0], height, width)
                    clip = [self.resize(f, h, w) for f in clip]
                frames = [np.asarray(f) for f in clip]
                pixels.append([p[..., None] if p.ndim == 2 else p for p in frames])
            flat = [p for clip in pixels for p in clip]
            # other PIL modes (I;16, F, 1) and clips of unequal geometry: the host chain (whose stack raises for the latter)
            if all(p.dtype == np.uint8 and p.ndim == 3 and p.shape == flat[0].shape for p in flat) \
                    and all(len(c) == len(pixels[0]) for c in pixels):
                (H, W, C_), T = flat[0].shape, len(pixels[0])
                out = torch.empty(len(clips), C_, T, H, W, dtype=torch.float16, device=device)
                for b, clip in enumerate(pixels):
                    u = torch.from_numpy(np.ascontiguousarray(np.stack(clip, axis=0))).to(device)          # [T, H, W, C], one upload
                    ops.image_preprocess(u.view(1, T * H, W, C_), out=out[b].view(1, C_, T * H, W))
                return out
        out = torch.stack([super(VideoProcessor, self).preprocess(clip, height, width) for clip in clips], dim=0).permute(0, 2, 1, 3, 4)
        return out if device is None and dtype is None else out.to(device=device, dtype=dtype)

    @staticmethod
    def _clips(video) -> list:
        """the accepted forms of ``preprocess_video`` -> a list of clips, each what ``preprocess`` takes ([EXT] diffusers' checks)"""
        def pil(x):
            return PIL is not None and isinstance(x, PIL.Image.Image)

        def array(x, nd):
            return isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == nd
        if array(video, 5):
            return list(video)
        if array(video, 4):
            return [video]
        if isinstance(video, list) and video:
            if all(pil(f) for f in video):
                return [video]
            if all(isinstance(c, list) and c and all(pil(f) for f in c) for c in video) or all(array(c, 4) for c in video):
                return list(video)
            if all(array(c, 5) for c in video):             # diffusers concatenates a list of 5-D batches
                return [clip for batch in video for clip in batch]
        raise ValueError("Input is in incorrect format. Currently, we only support a list of PIL frames, a list of such lists, a 4-D or "
                         f"5-D tensor / ndarray, or a list of 4-D or 5-D ones; got {type(video)}")

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

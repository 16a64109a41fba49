"""``PackedModule``: the bookkeeping every model host shares - parameters in their checkpoint layout, plus kernel-layout copies
("the pack", ``_pk``) made once per weight version by ``prepare()`` and forgotten whenever the parameters change.

A host subclasses it, names the sentence it refuses a module off the GPU with (``OFF_GPU``), and writes ``_pack()``: the body that
builds the kernel-layout weights and returns the namespace ``_pk`` holds.  ``load_state_dict``, ``.to()`` / ``.half()`` / ``.float()``
(all of them ``_apply``) and ``invalidate()`` reset it; a host with further weight-derived caches clears them in ``_forget()``.  The
hosts kept in the diffusers directory layout also name their config dataclass (``config_class``) and get ``from_pretrained`` /
``save_pretrained`` from here; the transformers-layout hosts (T5, CLIP) override the pair (lkgd_amd/loading.py has both bodies).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import loading
from ._lib import LkgdHipError


class PackedModule(nn.Module):
    #: the sentence ``prepare()`` raises with when the module is not on the GPU
    OFF_GPU = "lkgd_amd runs on MI355X only: move the module to cuda first"
    #: the config dataclass of a diffusers-layout directory (None: the class has no such form)
    config_class = None

    def __init__(self):
        super().__init__()
        self._pk = None                # None: not packed

    # ---- where the module lives: its first parameter, in registration order ---------------------------------------------------
    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    # ---- the pack and what forgets it -----------------------------------------------------------------------------------------
    def invalidate(self):
        """call after changing parameters in place (``load_state_dict`` / ``.to()`` do it automatically)"""
        self._pk = None
        self._forget()

    def _forget(self):
        """further caches derived from the parameters"""

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.invalidate()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self.invalidate()
        return r

    @torch.no_grad()
    def prepare(self):
        """(re)build the kernel-layout weights; idempotent, runs once per weight version"""
        if self._pk is not None:
            return
        self._check_packable()
        if self.device.type != "cuda":
            raise LkgdHipError(self.OFF_GPU)
        self._pk = self._pack()

    def _check_packable(self):
        """refusals that come before the device check"""

    def _pack(self):
        raise NotImplementedError

    # ---- the diffusers directory layout ---------------------------------------------------------------------------------------
    @classmethod
    def _config_class(cls):
        if cls.config_class is None:
            raise LkgdHipError(f"{cls.__name__} has no diffusers-layout directory form")
        return cls.config_class

    @classmethod
    def _build_options(cls, **_ignored) -> dict:
        """further keywords of ``loading.build_from_pretrained`` (constructor keywords, ``ctor_from_state``, ``strict``)"""
        return {}

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, subfolder: Optional[str] = None, torch_dtype=None,
                        variant: Optional[str] = None, **kw):
        """``ModelMixin.from_pretrained`` [EXT] for a local diffusers directory (``config.json`` + safetensors); hub / cache /
        device-map keywords are accepted and ignored"""
        return loading.build_from_pretrained(cls, cls._config_class(), pretrained_model_name_or_path, subfolder, torch_dtype, variant,
                                             **cls._build_options(**kw))

    def _saved_config(self) -> dict:
        return dict(self.config.__dict__)

    def save_pretrained(self, save_directory: str, variant: Optional[str] = None, **_ignored):
        self._config_class()
        loading.save_pretrained(self, save_directory, self._saved_config(), type(self).__name__, variant)

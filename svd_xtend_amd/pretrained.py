"""Checkpoint-folder plumbing shared by the three models (unet.py, vae.py, clip.py): the config mapping, the `.to(dtype)` contract
(float masters stay fp32, a 16-bit request selects the activation dtype) and `from_pretrained` of a diffusers / transformers folder:
`<path>/<subfolder>/config.json` + `<weights>[.<variant>].safetensors`, loaded strictly into float masters.  Local folders only."""
from __future__ import annotations

import json
import os
from typing import Optional

import torch

CONFIG_NAME = "config.json"
WEIGHTS_NAME = "diffusion_pytorch_model{variant}.safetensors"


class FrozenConfig(dict):
    """diffusers' FrozenDict in miniature: `config.addition_time_embed_dim` (train_svd.py:887) and
    `model.register_to_config(**other.config)` (train_svd.py:723) both work."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class PretrainedMixin:
    """In front of nn.Module in the bases of the three models.  Per-class hooks: `weights_name`, `skip_keys`, `_config_args`,
    `_weights_file`."""

    weights_name = WEIGHTS_NAME
    skip_keys = ()                     # checkpoint entries that are no parameter or buffer here
    _requested_dtype = None            # activation dtype asked for by `.to(dtype=...)` / `from_pretrained(torch_dtype=...)`

    @classmethod
    def _config_args(cls, raw: dict) -> dict:
        """constructor arguments from the parsed `config.json`"""
        return {k: v for k, v in raw.items() if not k.startswith("_")}

    @classmethod
    def _weights_file(cls, folder: str, variant: Optional[str]) -> str:
        wpath = os.path.join(folder, cls.weights_name.format(variant=f".{variant}" if variant else ""))
        if not os.path.exists(wpath) and variant:                         # diffusers falls back to the un-suffixed file
            wpath = os.path.join(folder, cls.weights_name.format(variant=""))
        return wpath

    @classmethod
    def from_pretrained(cls, path, subfolder: Optional[str] = None, variant: Optional[str] = None, torch_dtype=None, **unused):
        from safetensors.torch import load_file
        folder = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(folder, CONFIG_NAME)) as f:
            model = cls(**cls._config_args(json.load(f)))
        sd = load_file(cls._weights_file(folder, variant))
        model.load_state_dict({k: v.float() for k, v in sd.items() if k not in cls.skip_keys}, strict=True)   # float masters; kernels use packed copies
        if torch_dtype is not None and torch_dtype != torch.float32:
            model._requested_dtype = torch_dtype
        return model

    def to(self, *args, **kwargs):
        """`model.to(device, dtype=weight_dtype)` (train_svd.py:738-739, train_svd_lora.py:669): the float masters stay fp32 (the
        kernels run on their packed 16-bit copies); a half / bfloat16 request only selects the activation dtype."""
        device, dtype, non_blocking, _ = torch._C._nn._parse_to(*args, **kwargs)
        if dtype is not None and dtype.is_floating_point and dtype != torch.float32:
            self._requested_dtype = dtype
            return super().to(device=device, non_blocking=non_blocking) if device is not None else self
        return super().to(*args, **kwargs)

    def half(self):
        return self.to(dtype=torch.float16)

    def bfloat16(self):
        return self.to(dtype=torch.bfloat16)

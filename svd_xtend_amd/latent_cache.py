"""Latent cache: the frozen conditioners' outputs for every frame of a dataset, computed once.

The VAE encoder and the CLIP image tower are frozen, the encoder treats every frame on its own, and the reference's dataset hands out
runs of consecutive frames of a folder without augmentation (train_svd.py:69-137).  The posterior moments of every frame and the image
embedding of every frame that may open a window therefore never change over a fine-tuning run: `LatentCache.build` computes them once,
`TrainLoop(latent_cache=...)` serves any window from them (svdx_latent_batch gathers, samples and noises in one launch).

What is NOT cached is the conditioning latent: the encoding of the first frame plus fresh pixel noise of a fresh strength
(train_svd.py:954-960) differs every iteration, so one frame still goes through the encoder per sample.

A cache is fp32, lives on one device, and every rank holds all of it (mean + std: 2 * c * h * w floats per frame, 80 KB at 512 x 320).
Sharded caches, host-resident caches with per-step uploads and reduced-precision storage are out of scope."""
from __future__ import annotations

import hashlib
import json
import os
from typing import Iterable, Optional

import torch

from .clip import encode_image

TENSORS_NAME = "latent_cache.safetensors"
META_NAME = "meta.json"
FORMAT = 1


def towers_fingerprint(vae, image_encoder) -> str:
    """SHA-256 over what the cached values depend on: the encoder-side VAE weights (encoder + quant_conv) and the CLIP weights -- names,
    dtypes, shapes and bytes, in sorted order."""
    h = hashlib.sha256()
    groups = (("vae.encoder", vae.encoder.state_dict()), ("vae.quant_conv", vae.quant_conv.state_dict()),
              ("image_encoder", image_encoder.state_dict()))
    for prefix, sd in groups:
        for name in sorted(sd):
            t = sd[name].detach().contiguous().cpu()
            h.update(f"{prefix}.{name}|{t.dtype}|{tuple(t.shape)}|".encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _tower_dtype(vae, image_encoder) -> str:
    if vae.rt is None:
        vae.prepare()
    if image_encoder.rt is None:
        image_encoder.prepare()
    if vae.rt.dt != image_encoder.rt.dt:
        raise ValueError(f"the VAE runs in {vae.rt.dt} and the image encoder in {image_encoder.rt.dt}: one cache holds one tower dtype")
    return str(vae.rt.dt).replace("torch.", "")


class LatentCache:
    """mean, std [F, c, h, w] (as `DiagonalGaussianDistribution` forms them) and embed [F, D] = encode_image(frame), fp32 on the towers'
    device; video_start int64 [V + 1] on the host: video v owns the rows video_start[v] .. video_start[v + 1] - 1."""

    def __init__(self, mean: torch.Tensor, std: torch.Tensor, embed: torch.Tensor, video_start: torch.Tensor, meta: dict):
        F = mean.shape[0]
        if mean.ndim != 4 or std.shape != mean.shape or embed.ndim != 2 or embed.shape[0] != F:
            raise ValueError(f"mean / std [F, c, h, w] and embed [F, D] expected, got {tuple(mean.shape)}, {tuple(std.shape)}, {tuple(embed.shape)}")
        if any(t.dtype != torch.float32 for t in (mean, std, embed)):
            raise ValueError("a latent cache is fp32")
        vs = video_start.to("cpu", torch.int64)
        if vs.ndim != 1 or vs.numel() < 2 or int(vs[0]) != 0 or int(vs[-1]) != F or bool((vs[1:] < vs[:-1]).any()):
            raise ValueError(f"video_start must rise from 0 to {F}, got {vs.tolist()}")
        self.mean, self.std, self.embed = mean.contiguous(), std.contiguous(), embed.contiguous()
        self.video_start = vs
        self._starts = vs.tolist()
        self.meta = dict(meta)

    # ---- shape --------------------------------------------------------------------------------------------------------------
    @property
    def n_frames(self) -> int:
        return self.mean.shape[0]

    @property
    def n_videos(self) -> int:
        return len(self._starts) - 1

    @property
    def device(self) -> torch.device:
        return self.mean.device

    def video_len(self, video: int) -> int:
        return self._starts[video + 1] - self._starts[video]

    def window(self, video: int, start: int, T: int) -> int:
        """The cache row of frame `start` of `video`, for a window of T consecutive frames.  The ONLY place an index is produced: a run
        that crosses the end of its video, or any negative value, is an IndexError here (the kernel merely clamps what it is given)."""
        video, start, T = int(video), int(start), int(T)
        if video < 0 or video >= self.n_videos:
            raise IndexError(f"video {video} outside [0, {self.n_videos})")
        if start < 0 or T < 1 or start + T > self.video_len(video):
            raise IndexError(f"frames [{start}, {start + T}) outside video {video} of {self.video_len(video)} frames")
        return self._starts[video] + start

    # ---- build --------------------------------------------------------------------------------------------------------------
    @classmethod
    @torch.no_grad()
    def build(cls, vae, image_encoder, videos: Iterable[torch.Tensor], chunk: Optional[int] = None) -> "LatentCache":
        """videos: an iterable of [N_v, 3, H, W] float clips in [-1, 1] (one resolution).  Every frame goes through `vae.encode` and
        `encode_image` once, in chunks of at most `vae.max_frames(H, W)` frames (`chunk`: a smaller limit)."""
        dtype = _tower_dtype(vae, image_encoder)
        dev = vae.rt.dev
        means, stds, embeds, starts = [], [], [], [0]
        H = W = None
        for v, clip in enumerate(videos):
            if clip.ndim != 4 or clip.shape[1] != 3 or clip.shape[0] < 1:
                raise ValueError(f"video {v}: expected [N, 3, H, W], got {tuple(clip.shape)}")
            if H is None:
                H, W = int(clip.shape[2]), int(clip.shape[3])
                step = vae.max_frames(H, W)
                if chunk is not None:
                    if chunk < 1:
                        raise ValueError("chunk must be at least 1")
                    step = min(step, int(chunk))
            elif (int(clip.shape[2]), int(clip.shape[3])) != (H, W):
                raise ValueError(f"video {v} is {clip.shape[2]}x{clip.shape[3]}, the cache {H}x{W}")
            for i in range(0, clip.shape[0], step):
                x = clip[i:i + step].to(dev, non_blocking=True).to(torch.float32)
                dist = vae.encode(x).latent_dist
                means.append(dist.mean.to(torch.float32).clone())
                stds.append(dist.std.to(torch.float32).clone())
                embeds.append(encode_image(x, image_encoder).to(torch.float32).clone())
            starts.append(starts[-1] + int(clip.shape[0]))
        if H is None:
            raise ValueError("no videos")
        mean, std, embed = torch.cat(means), torch.cat(stds), torch.cat(embeds)
        meta = dict(format=FORMAT, H=H, W=W, c=int(mean.shape[1]), h=int(mean.shape[2]), w=int(mean.shape[3]), embed_dim=int(embed.shape[1]),
                    dtype=dtype, scaling_factor=float(vae.config.scaling_factor), sha256=towers_fingerprint(vae, image_encoder))
        return cls(mean, std, embed, torch.tensor(starts, dtype=torch.int64), meta)

    # ---- disk ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def exists(folder: str) -> bool:
        return os.path.isfile(os.path.join(folder, TENSORS_NAME)) and os.path.isfile(os.path.join(folder, META_NAME))

    def save(self, folder: str) -> None:
        from safetensors.torch import save_file
        os.makedirs(folder, exist_ok=True)
        save_file(dict(mean=self.mean.cpu(), std=self.std.cpu(), embed=self.embed.cpu(), video_start=self.video_start.clone()),
                  os.path.join(folder, TENSORS_NAME))
        with open(os.path.join(folder, META_NAME), "w") as fh:
            json.dump(self.meta, fh, indent=1, sort_keys=True)

    def check(self, vae=None, image_encoder=None, height: Optional[int] = None, width: Optional[int] = None, weights: bool = True) -> None:
        """ValueError unless this cache was built by these towers (weights, dtype, scaling_factor) at this resolution: a cache from other
        weights or another resolution must never train silently.  weights=False leaves out the SHA-256 over the weights (seconds at the
        SVD sizes: `load` has done it; TrainLoop repeats only the cheap part)."""
        m = self.meta
        bad = []
        if height is not None and int(height) != m["H"]:
            bad.append(f"height {height} (cache: {m['H']})")
        if width is not None and int(width) != m["W"]:
            bad.append(f"width {width} (cache: {m['W']})")
        if (vae is None) != (image_encoder is None):
            raise ValueError("pass both towers or neither: the fingerprint covers the two")
        if vae is not None:
            down = 2 ** (len(vae.config.block_out_channels) - 1)
            if float(vae.config.scaling_factor) != m["scaling_factor"]:
                bad.append(f"scaling_factor {vae.config.scaling_factor} (cache: {m['scaling_factor']})")
            if vae.config.latent_channels != m["c"] or m["h"] * down != m["H"] or m["w"] * down != m["W"]:
                bad.append(f"latent geometry {vae.config.latent_channels} channels, 1/{down} (cache: {m['c']} x {m['h']} x {m['w']} of {m['H']} x {m['W']})")
            if image_encoder.config.projection_dim != m["embed_dim"]:
                bad.append(f"embedding width {image_encoder.config.projection_dim} (cache: {m['embed_dim']})")
            dtype = _tower_dtype(vae, image_encoder)
            if dtype != m["dtype"]:
                bad.append(f"tower dtype {dtype} (cache: {m['dtype']})")
            if weights and not bad and towers_fingerprint(vae, image_encoder) != m["sha256"]:
                bad.append("the VAE encoder / CLIP weights (SHA-256 differs)")
        if bad:
            raise ValueError("latent cache does not belong to this run: " + "; ".join(bad))

    @classmethod
    def load(cls, folder: str, device, vae=None, image_encoder=None, height: Optional[int] = None, width: Optional[int] = None) -> "LatentCache":
        from safetensors.torch import load_file
        with open(os.path.join(folder, META_NAME)) as fh:
            meta = json.load(fh)
        if meta.get("format") != FORMAT:
            raise ValueError(f"{folder}: latent cache format {meta.get('format')!r}, this revision reads {FORMAT}")
        t = load_file(os.path.join(folder, TENSORS_NAME))
        shape = (meta["c"], meta["h"], meta["w"])
        if tuple(t["mean"].shape[1:]) != shape or tuple(t["std"].shape) != tuple(t["mean"].shape) or t["embed"].shape[1] != meta["embed_dim"]:
            raise ValueError(f"{folder}: tensors do not match meta.json")
        cache = cls(t["mean"].to(device), t["std"].to(device), t["embed"].to(device), t["video_start"], meta)
        cache.check(vae, image_encoder, height, width)
        return cache

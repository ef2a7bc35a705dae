"""LoRA adapters, host side: which UNet weights get one, how they start, the adapter file, and merging into a state_dict.

An adapter of rank r on a weight W0 of shape (out, in[, 1...]) is A [r, in] and B [out, r]; the model computes with
W0 + s B A, s = alpha / r.  Training (SyncMultiviewDiffusion.enable_lora) keeps A and B on the device and merges there
(csrc/k_lora.hip); inference merges once on the host (``merge_lora``) before the weights are packed, so a merged engine launches
exactly what an unmerged one does.

Adapter file (``torch.save`` of ``lora_state_dict``): ``lora.<state_dict key>.A`` / ``.B`` per target (fp32), ``lora.rank``
(int64 scalar) and ``lora.alpha`` (fp32 scalar)."""
import collections
import fnmatch
import math

import torch

UNET_PREFIX = "model.diffusion_model."
# the SpatialTransformers' self- and cross-attention projections: 8 weights per transformer block
DEFAULT_PATTERNS = ("*.transformer_blocks.*.attn[12].to_[qkv].weight", "*.transformer_blocks.*.attn[12].to_out.0.weight")
MAX_RANK = 64


def is_target_shape(shape):
    """(out, in) followed only by 1s: Linear, 1x1 and 1x1x1 convolution weights."""
    shape = tuple(shape)
    return len(shape) >= 2 and all(int(d) == 1 for d in shape[2:])


def check_rank(rank):
    if int(rank) != rank or not 1 <= int(rank) <= MAX_RANK:
        raise ValueError(f"LoRA rank must be an integer in 1..{MAX_RANK}, not {rank!r}")
    return int(rank)


def select_targets(shapes, patterns=None):
    """Sorted state_dict keys of the UNet weights that ``patterns`` select.  shapes: {state_dict key: shape} (a manifest, or a
    training engine's param_table shapes); patterns: fnmatch patterns over the UNet's keys, with or without the
    ``model.diffusion_model.`` prefix (None: DEFAULT_PATTERNS).  A pattern that matches nothing, or matches a tensor that is not
    an (out, in[, 1...]) weight, raises ValueError."""
    patterns = list(DEFAULT_PATTERNS if patterns is None else patterns)
    if isinstance(patterns, str) or not patterns:
        raise ValueError("LoRA targets: a non-empty list of fnmatch patterns")
    unet = sorted(k for k in shapes if k.startswith(UNET_PREFIX))
    picked = set()
    for pat in patterns:
        hit = [k for k in unet if fnmatch.fnmatchcase(k, pat) or fnmatch.fnmatchcase(k[len(UNET_PREFIX):], pat)]
        if not hit:
            raise ValueError(f"LoRA target pattern {pat!r} matches no UNet parameter")
        bad = [k for k in hit if not is_target_shape(shapes[k])]
        if bad:
            raise ValueError(f"LoRA target pattern {pat!r} matches {bad[0]} of shape {tuple(shapes[bad[0]])}: only "
                             "(out, in) weights followed by 1s (Linear, 1x1 convolutions) can carry an adapter")
        picked.update(hit)
    return sorted(picked)


def init_adapters(keys, shapes, rank, seed=0):
    """{key: (A, B)} on the CPU: A ~ U(-1/sqrt(in), 1/sqrt(in)) from ONE generator seeded with ``seed``, drawn in sorted key
    order; B = 0 (the adapted model starts as the base model)."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for k in sorted(keys):
        o, i = int(shapes[k][0]), int(shapes[k][1])
        a = (torch.rand(rank, i, generator=g) * 2.0 - 1.0) / math.sqrt(i)
        out[k] = (a, torch.zeros(o, rank))
    return out


def pack_lora(adapters, rank, alpha):
    """The adapter file's dict from {key: (A, B)}."""
    sd = collections.OrderedDict()
    for k in sorted(adapters):
        a, b = adapters[k]
        sd[f"lora.{k}.A"] = a.detach().to(device="cpu", dtype=torch.float32).clone()
        sd[f"lora.{k}.B"] = b.detach().to(device="cpu", dtype=torch.float32).clone()
    sd["lora.rank"] = torch.tensor(int(rank), dtype=torch.int64)
    sd["lora.alpha"] = torch.tensor(float(alpha), dtype=torch.float32)
    return sd


def unpack_lora(lora):
    """(adapters {key: (A, B)}, rank, alpha) of an adapter file's dict (or of the path of one); checks it."""
    if isinstance(lora, (str, bytes)) or hasattr(lora, "__fspath__"):
        lora = torch.load(lora, map_location="cpu")
    if "lora.rank" not in lora or "lora.alpha" not in lora:
        raise ValueError("not a LoRA adapter file: lora.rank / lora.alpha missing")
    rank, alpha = check_rank(int(lora["lora.rank"])), float(lora["lora.alpha"])
    keys = sorted(k[len("lora."):-2] for k in lora if k.startswith("lora.") and k.endswith(".A"))
    extra = [k for k in lora if k not in ("lora.rank", "lora.alpha") and not (k.startswith("lora.") and k[-2:] in (".A", ".B"))]
    if extra or not keys:
        raise ValueError(f"not a LoRA adapter file: {'unexpected key ' + repr(extra[0]) if extra else 'no adapter'}")
    out = {}
    for k in keys:
        if f"lora.{k}.B" not in lora:
            raise ValueError(f"LoRA adapter file: lora.{k}.B missing")
        a, b = lora[f"lora.{k}.A"], lora[f"lora.{k}.B"]
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != rank or b.shape[1] != rank:
            raise ValueError(f"LoRA adapter {k}: A {tuple(a.shape)} / B {tuple(b.shape)} do not have rank {rank}")
        out[k] = (a, b)
    if len(out) * 2 + 2 != len(lora):
        raise ValueError("LoRA adapter file: a B without its A")
    return out, rank, alpha


def merge_lora(state_dict, lora, scale=1.0):
    """A copy of ``state_dict`` with W + scale (alpha / rank) B A in place of every adapted weight W (fp32 arithmetic, W's
    dtype and shape kept; every other entry is the same object).  lora: an adapter file's dict or its path.  scale = 0 returns
    the weights unchanged.  A missing weight, or A / B that do not fit it, raises ValueError."""
    adapters, rank, alpha = unpack_lora(lora)
    out = type(state_dict)(state_dict) if isinstance(state_dict, dict) else dict(state_dict)
    s = float(scale) * alpha / rank
    for k, (a, b) in adapters.items():
        w = state_dict.get(k)
        if not torch.is_tensor(w):
            raise ValueError(f"LoRA adapter for {k}: the state_dict has no such weight")
        if not is_target_shape(w.shape) or (int(w.shape[0]), int(w.shape[1])) != (b.shape[0], a.shape[1]):
            raise ValueError(f"LoRA adapter for {k}: B {tuple(b.shape)} A {tuple(a.shape)} does not fit a weight of shape {tuple(w.shape)}")
        if s == 0.0:
            continue
        w32 = w.detach().to(dtype=torch.float32)
        delta = b.to(device=w32.device, dtype=torch.float32) @ a.to(device=w32.device, dtype=torch.float32)
        out[k] = (w32 + s * delta.view(w32.shape)).to(dtype=w.dtype)
    return out

"""2-D image metrics of generated views against captured views, on the device (include/mvd.h: mvd_op_image_metrics,
csrc/k_metrics.hip): SSIM, PSNR, mean squared and mean absolute error under the reference's evaluation protocol -- 8-bit images,
skimage's ``structural_similarity`` at its uint8 defaults (7 x 7 uniform window, K1 = 0.01, K2 = 0.03, L = 255, sample covariance,
the 3-pixel border cropped, channels averaged), the prediction whitened where the ground truth is background.

  image_metrics       the metrics of any batch of views: float [-1, 1] or uint8, channels first or last, CPU or device tensors
  strip_to_views      the views of a saved image strip (batch.views_to_uint8, generate_face's PNG), the input tile dropped
  load_target_views   a folder of captured views: RGBA files composited on white, their alpha == 0 as the background mask

LPIPS, FID, key-point PCK and Re-ID need networks of their own and are not computed here; neither are Gaussian-window SSIM and
MS-SSIM.
"""
import glob
import os

import numpy as np
import torch

from . import engine as E


def _views(name, t):
    """(the tensor as [V,3,H,W] or [V,H,W,3], its leading dimensions, (H, W))."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if t.dim() < 3 or (t.shape[-3] == 3) == (t.shape[-1] == 3):
        raise ValueError(f"image_metrics: {name} must be [...,3,H,W] or [...,H,W,3], got {tuple(t.shape)}")
    if t.dtype != torch.uint8 and not t.is_floating_point():
        raise ValueError(f"image_metrics: {name} must be a float tensor or uint8, not {t.dtype}")
    hw = tuple(t.shape[-2:]) if t.shape[-3] == 3 else tuple(t.shape[-3:-1])
    return t.reshape(-1, *t.shape[-3:]), tuple(t.shape[:-3]), hw


def image_metrics(pred, target, mask=None):
    """SSIM / PSNR / MSE / MAE of each predicted view against its target view.

    pred, target: ``[..., 3, H, W]`` or ``[..., H, W, 3]`` (H, W >= 7; the two may differ in layout and dtype), with the same
    leading dimensions.  A float tensor holds values in [-1, 1] and is quantised exactly as ``batch.views_to_uint8`` does,
    q = trunc(((clamp(x, -1, 1) + 1) * 0.5) * 255) in fp32; a uint8 tensor is taken as it is.  CPU tensors are copied to the
    device of the other argument, or to the current device.
    mask: the background, where the PREDICTED pixel becomes white (255, 255, 255) before it is compared and the target stays --
    the reference's rule: its ground truth was composited on white.  ``None``: no background; a tensor ``[..., H, W]`` (bool or
    number): nonzero is background -- pass ``batch["target_mask"] < 0.5`` for the batch convention, where 1 is foreground;
    ``"white"``: a pixel is background iff all three QUANTISED target channels are >= 254.  That rule is defined on the bytes: it
    is not promised to agree with ``model.foreground_mask``'s float comparison (>= 1 - 2/255) for a value at that threshold.

    Returns a dict of float64 device tensors shaped like the leading dimensions: ``ssim``, ``psnr`` (= 10 log10(255^2 / mse),
    +inf for identical images), ``mse`` and ``mae`` (over all 3 H W 8-bit values), ``background`` (masked pixels) and
    ``nonfinite`` (NaNs and infinities in the float inputs).  A view with a non-finite value reports NaN for every metric.
    Raises ValueError on a shape or dtype mismatch before anything is launched; makes no host synchronisation beyond the entry
    point's own."""
    p, lead, hw = _views("pred", pred)
    t, tlead, thw = _views("target", target)
    if lead != tlead or hw != thw:
        raise ValueError(f"image_metrics: pred is {list(lead)} views of {hw}, target {list(tlead)} views of {thw}")
    if hw[0] < 7 or hw[1] < 7:
        raise ValueError(f"image_metrics: H and W must be at least 7 (one 7 x 7 window), got {hw}")
    if p.shape[0] < 1:
        raise ValueError("image_metrics: no views")
    m, mode = None, "none"
    if isinstance(mask, str):
        if mask != "white":
            raise ValueError(f"image_metrics: mask must be None, 'white' or a tensor, not {mask!r}")
        mode = "white"
    elif mask is not None:
        m = mask if torch.is_tensor(mask) else torch.as_tensor(mask)
        if tuple(m.shape) != lead + hw:
            raise ValueError(f"image_metrics: mask must be {list(lead + hw)}, got {tuple(m.shape)}")
        m, mode = m.reshape(-1, *hw), "explicit"
    dev = next((x.device for x in (p, t) if x.device.type == "cuda"), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    out = E.op_image_metrics(p, t, m, mode, device=dev)
    n = float(3 * hw[0] * hw[1])
    mse = out[:, 1] / n
    res = {"ssim": out[:, 0], "psnr": 10.0 * torch.log10(255.0 ** 2 / mse), "mse": mse, "mae": out[:, 2] / n,
           "background": out[:, 3], "nonfinite": out[:, 4]}
    return {k: v.reshape(lead) for k, v in res.items()}


def strip_to_views(strip, n, size):
    """The views of an image strip as ``batch.views_to_uint8`` / ``generate_face`` write it -- uint8 ``[B * size, (n + 1) * size, 3]``:
    per sample one row of the input view followed by n generated views -- as ``[B, n, size, size, 3]``, the input tile dropped."""
    a = np.asarray(strip)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[1] != (n + 1) * size or a.shape[0] % size or a.shape[0] == 0:
        raise ValueError(f"strip_to_views: expected [B*{size}, {(n + 1) * size}, 3], got {a.shape}")
    tiles = a.reshape(a.shape[0] // size, size, n + 1, size, 3).transpose(0, 2, 1, 3, 4)
    return torch.from_numpy(np.ascontiguousarray(tiles[:, 1:]))


def load_target_views(dir, n, size):
    """The captured views of a folder: its ``*.png`` files in sorted order, exactly ``n`` of them at ``size`` x ``size``.  An RGBA
    file is composited on white in fp32, rgb a + 255 (1 - a) with a = alpha / 255, truncated to uint8, and its ``alpha == 0`` is
    the background mask; any other file is read as RGB, without a mask.  Returns (uint8 ``[n, size, size, 3]``, uint8 mask
    ``[n, size, size]`` -- all zero for a view without alpha -- or ``None`` when no file has an alpha channel)."""
    from PIL import Image
    files = sorted(glob.glob(os.path.join(str(dir), "*.png")))
    if len(files) != n:
        raise ValueError(f"load_target_views: {dir} holds {len(files)} *.png files, {n} expected")
    views, masks, any_alpha = [], [], False
    for f in files:
        with Image.open(f) as im:
            if im.size != (size, size):
                raise ValueError(f"load_target_views: {f} is {im.size[0]} x {im.size[1]}, {size} x {size} expected")
            if im.mode == "RGBA":
                rgba = np.asarray(im).astype(np.float32)
                a = rgba[:, :, 3:] / np.float32(255.0)
                views.append((rgba[:, :, :3] * a + np.float32(255.0) * (np.float32(1.0) - a)).astype(np.uint8))
                masks.append((rgba[:, :, 3] == 0).astype(np.uint8))
                any_alpha = True
            else:
                views.append(np.asarray(im.convert("RGB")).copy())
                masks.append(np.zeros((size, size), np.uint8))
    return torch.from_numpy(np.stack(views)), torch.from_numpy(np.stack(masks)) if any_alpha else None


def summarise(metrics, keys=("ssim", "psnr", "mse", "mae")):
    """{key: per-view list, key + "_mean": mean over the views} of a metrics dict, as plain floats for a JSON file (one copy to
    the host).  JSON has no infinity: json.dump writes a PSNR of +inf as ``Infinity``, which json.load reads back."""
    out = {}
    for k in keys:
        v = metrics[k].detach().double().reshape(-1).cpu()
        out[k] = v.tolist()
        out[k + "_mean"] = float(v.mean()) if v.numel() else float("nan")
    return out

"""The oracle of the image metrics (include/mvd.h: mvd_op_image_metrics), numpy only, written from the protocol:

  * both images are 8-bit: a float image is quantised q = trunc(((clamp(x, -1, 1) + 1) * 0.5) * 255), every step in fp32 in that
    order (batch.views_to_uint8's bytes); a uint8 image is taken as it is;
  * where a pixel is background the PREDICTED pixel becomes 255 in all three channels; mode "none", "explicit" (mask [V,H,W],
    nonzero = background) or "white" (all three quantised target channels >= 254);
  * SSIM per channel over a 7 x 7 uniform window, K1 = 0.01, K2 = 0.03, L = 255, sample (co)variances, averaged over the centres
    whose window lies inside the image, then over the channels.  The five window sums are exact integers (int64 2-D cumulative
    sums); only the rational function S is evaluated, in float64;
  * sse / sae over all 3 H W values after the background rule, the background and non-finite counts: exact integers.
"""
import numpy as np

C1 = (0.01 * 255.0) * (0.01 * 255.0)
C2 = (0.03 * 255.0) * (0.03 * 255.0)
WIN = 7


def quantise(x):
    """float array in [-1, 1] -> uint8, the fp32 operation sequence of batch.views_to_uint8 (non-finite values: see nonfinite)."""
    x = np.asarray(x, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(-1.0), x)
    c = np.clip(x, np.float32(-1.0), np.float32(1.0))
    return (((c + np.float32(1.0)) * np.float32(0.5)) * np.float32(255.0)).astype(np.uint8)


def to_bytes(img, layout):
    """(uint8 [V,H,W,3], non-finite values per view) of an image batch, layout "nchw" or "nhwc", float or uint8."""
    a = np.asarray(img)
    if layout == "nchw":
        a = a.transpose(0, 2, 3, 1)
    if a.dtype == np.uint8:
        return a, np.zeros(a.shape[0], np.int64)
    a = a.astype(np.float32)
    return quantise(a), (~np.isfinite(a)).reshape(a.shape[0], -1).sum(1).astype(np.int64)


def window_sums(a):
    """Sums of the int64 image a [H,W] over every 7 x 7 window that lies inside it -> [H-6, W-6]."""
    H, W = a.shape
    cs = np.zeros((H + 1, W + 1), np.int64)
    cs[1:, 1:] = a.cumsum(0).cumsum(1)
    return cs[WIN:, WIN:] - cs[:-WIN, WIN:] - cs[WIN:, :-WIN] + cs[:-WIN, :-WIN]


def ssim_channel(x, y):
    """Mean of S over the interior window centres of one channel; x, y uint8 [H,W]."""
    x, y = x.astype(np.int64), y.astype(np.int64)
    X, Y, XX, YY, XY = window_sums(x), window_sums(y), window_sums(x * x), window_sums(y * y), window_sums(x * y)
    a1 = (2 * X * Y).astype(np.float64) / 2401.0 + C1
    a2 = (2 * (49 * XY - X * Y)).astype(np.float64) / 2352.0 + C2
    b1 = (X * X + Y * Y).astype(np.float64) / 2401.0 + C1
    b2 = ((49 * XX - X * X) + (49 * YY - Y * Y)).astype(np.float64) / 2352.0 + C2
    return float(((a1 * a2) / (b1 * b2)).mean())


def image_metrics_ref(pred, target, mask=None, mode="none", pred_layout="nhwc", target_layout="nhwc"):
    """{"ssim", "sse", "sae", "background", "nonfinite"}: one float64 entry per view.  A view with a non-finite input value
    reports NaN for everything but its non-finite count."""
    p, nf_p = to_bytes(pred, pred_layout)
    t, nf_t = to_bytes(target, target_layout)
    assert p.shape == t.shape and p.shape[3] == 3
    V = p.shape[0]
    if mode == "explicit":
        bg = np.asarray(mask) != 0
    elif mode == "white":
        bg = (t >= 254).all(-1)
    else:
        assert mode == "none" and mask is None
        bg = np.zeros(p.shape[:3], bool)
    p = np.where(bg[..., None], np.uint8(255), p)
    d = p.astype(np.int64) - t.astype(np.int64)
    out = {"ssim": np.array([np.mean([ssim_channel(p[v, :, :, c], t[v, :, :, c]) for c in range(3)]) for v in range(V)]),
           "sse": (d * d).reshape(V, -1).sum(1).astype(np.float64), "sae": np.abs(d).reshape(V, -1).sum(1).astype(np.float64),
           "background": bg.reshape(V, -1).sum(1).astype(np.float64), "nonfinite": (nf_p + nf_t).astype(np.float64)}
    bad = out["nonfinite"] != 0
    for k in ("ssim", "sse", "sae", "background"):
        out[k][bad] = np.nan
    return out


def derived(ref, H, W):
    """psnr / mse / mae as metrics.image_metrics derives them from the sums."""
    n = float(3 * H * W)
    mse = ref["sse"] / n
    with np.errstate(divide="ignore"):
        return {"mse": mse, "mae": ref["sae"] / n, "psnr": 10.0 * np.log10(255.0 ** 2 / mse)}


def bin_edge_values():
    """float32 [3,16,17]: every k/255 * 2 - 1 and both fp32 neighbours of each -- the values at which the quantisation changes
    its byte -- followed by values at and outside [-1, 1]."""
    k = (np.arange(256, dtype=np.float64) / 255.0 * 2.0 - 1.0).astype(np.float32)
    edges = np.stack([np.nextafter(k, np.float32(-2.0)), k, np.nextafter(k, np.float32(2.0))], 1).reshape(-1)
    extra = np.array([-1.0, 1.0, -1.5, 1.5, -100.0, 100.0, -1.0000001, 1.0000001, 0.0, -0.0, 3e38, -3e38], np.float32)
    vals = np.concatenate([edges, np.resize(extra, 3 * 16 * 17 - edges.size)]).astype(np.float32)
    return vals.reshape(3, 16, 17)


def make_views(V, H, W, seed, kind="near"):
    """Seeded uint8 views [V,H,W,3] (pred, target), every view with data of its own: smooth-ish structure plus noise, so that
    means, variances and the covariance all matter.  kind "near": pred = target +- 6; "random": independent."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    tgt = np.empty((V, H, W, 3), np.uint8)
    for v in range(V):
        for c in range(3):
            base = 127 + 90 * np.sin(xx * (0.2 + 0.1 * v) + c) * np.cos(yy * (0.15 + 0.05 * c) + v)
            tgt[v, :, :, c] = np.clip(base + r.randint(-30, 31, (H, W)), 0, 255).astype(np.uint8)
    if kind == "random":
        prd = r.randint(0, 256, (V, H, W, 3)).astype(np.uint8)
    else:
        prd = np.clip(tgt.astype(np.int64) + r.randint(-6, 7, tgt.shape), 0, 255).astype(np.uint8)
    return prd, tgt


def bytes_to_float(q):
    """A float32 image in [-1, 1] that quantises back to exactly the bytes q: the middle of each byte's bin."""
    f = ((q.astype(np.float64) + 0.5) / 255.0 * 2.0 - 1.0).astype(np.float32)
    f = np.minimum(f, np.float32(1.0))
    assert (quantise(f) == q).all()
    return f

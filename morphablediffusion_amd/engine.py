"""Thin object wrapper over the C ABI: owns one mvd_ctx on one GPU, hands torch device tensors to the
library by pointer (PyTorch is used for device memory and streams only)."""
import collections
import ctypes as C
import os
import types
from typing import Dict, Optional

import torch

from . import lib as L
from .spec import UNetConfig, VolumeConfig


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


LOSS_TYPES = ("l2", "huber")  # loss_type of mvd_train_unet_step_ex / mvd_op_train_loss, by index


def op_train_loss(pred, target, sample_weight=None, pixel_weight=None, loss_type="l2", huber_delta=1.0, loss_scale=1.0,
                  want_grad=False, device=None, lib=None):
    """Engine.op_train_loss without an engine (the hook takes no context): runs on ``device`` (default: pred's)."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"loss_type must be one of {LOSS_TYPES}, not {loss_type!r}")
    lib = lib or L.load()
    dev = pred.device if device is None else device
    p, tg = _f32(pred, dev), _f32(target, dev)
    if p.dim() != 3 or p.shape != tg.shape:
        raise ValueError(f"op_train_loss: pred and target must both be [B,HW,C], got {tuple(p.shape)} and {tuple(tg.shape)}")
    B, HW, C = p.shape
    w = None if sample_weight is None else _f32(sample_weight, dev).reshape(-1)
    m = None if pixel_weight is None else _f32(pixel_weight, dev).reshape(B, -1)
    if w is not None and w.numel() != B:
        raise ValueError(f"op_train_loss: sample_weight must have {B} elements")
    if m is not None and m.shape[1] != HW:
        raise ValueError(f"op_train_loss: pixel_weight must be [{B},{HW}]")
    nan = float("nan")
    loss = torch.full((1,), nan, device=dev, dtype=torch.float32)
    lps = torch.full((B,), nan, device=dev, dtype=torch.float32)
    mps = torch.full((B,), nan, device=dev, dtype=torch.float32)
    dpred = torch.full_like(p, nan) if want_grad else None
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_train_loss(L.ptr(p), L.ptr(tg), B, HW, C, L.ptr(w), L.ptr(m), LOSS_TYPES.index(loss_type),
                                      float(huber_delta), float(loss_scale), L.ptr(dpred), L.ptr(loss), L.ptr(lps), L.ptr(mps),
                                      _stream()))
    return (loss[0], lps, mps, dpred) if want_grad else (loss[0], lps, mps)


MASK_MODES = ("none", "explicit", "white")  # mask_mode of mvd_op_image_metrics, by index
METRIC_COLUMNS = ("ssim", "sse", "sae", "background", "nonfinite")  # the columns of its output


def _image_arg(name, t):
    """(dtype code, layout code, (V, H, W)) of one image batch [V,3,H,W] / [V,H,W,3], float or uint8."""
    if t.dim() != 4 or (t.shape[1] == 3) == (t.shape[3] == 3):
        raise ValueError(f"op_image_metrics: {name} must be [V,3,H,W] or [V,H,W,3], got {tuple(t.shape)}")
    if t.dtype != torch.uint8 and not t.is_floating_point():
        raise ValueError(f"op_image_metrics: {name} must be a float tensor or uint8, not {t.dtype}")
    layout = 0 if t.shape[1] == 3 else 1
    shape = (t.shape[0], t.shape[2], t.shape[3]) if layout == 0 else tuple(t.shape[:3])
    return int(t.dtype == torch.uint8), layout, shape


def op_image_metrics(pred, target, mask=None, mask_mode=None, device=None, lib=None):
    """mvd_op_image_metrics on ``device`` (default: pred's): pred / target [V,3,H,W] or [V,H,W,3] (the two may differ), float
    (taken as [-1, 1], quantised like batch.views_to_uint8) or uint8; mask [V,H,W], nonzero = background, with mask_mode
    "explicit" (the default with a mask); "white" derives the background from the target, "none" (the default without a mask)
    has none.  Returns [V,5] float64 on the device, columns METRIC_COLUMNS.  Shapes and dtypes are checked before anything is
    copied or launched; the one host synchronisation is the entry point's own."""
    mask_mode = mask_mode or ("none" if mask is None else "explicit")
    if mask_mode not in MASK_MODES:
        raise ValueError(f"mask_mode must be one of {MASK_MODES}, not {mask_mode!r}")
    if (mask_mode == "explicit") != (mask is not None):
        raise ValueError("op_image_metrics: mask_mode 'explicit' goes with a mask, the other modes without one")
    pd, pl, shape = _image_arg("pred", pred)
    td, tl, tshape = _image_arg("target", target)
    if shape != tshape:
        raise ValueError(f"op_image_metrics: pred is (V, H, W) = {shape}, target {tshape}")
    V, H, W = shape
    if V < 1 or H < 7 or W < 7:
        raise ValueError(f"op_image_metrics: at least one view of at least 7 x 7 pixels is needed, got (V, H, W) = {shape}")
    if mask is not None and tuple(mask.shape) != shape:
        raise ValueError(f"op_image_metrics: mask must be [V,H,W] = {list(shape)}, got {tuple(mask.shape)}")
    dev = pred.device if device is None else device
    p, tg = (t.detach().to(device=dev, dtype=torch.uint8 if d else torch.float32).contiguous() for t, d in ((pred, pd), (target, td)))
    m = None if mask is None else (mask.detach().to(dev) != 0).to(torch.uint8).contiguous()
    lib = lib or L.load()
    out = torch.full((V, len(METRIC_COLUMNS)), float("nan"), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_image_metrics(L.ptr(p), pd, pl, L.ptr(tg), td, tl, L.ptr(m), MASK_MODES.index(mask_mode), V, H, W,
                                         L.ptr(out), _stream()))
    return out


# ---- mesh texturing from views (include/mvd.h: mvd_op_mesh_project / _raster / _vertex_colors; csrc/k_mesh.hip): context-free.
MESH_SUB, MESH_KMAX, MESH_GUARD_PX = 4, (1 << 24) - 1, 4096  # 1/16-pixel coordinates, the largest depth key, the guard band


def _i32(name, t, shape, who):
    """t as it is if it is an int32 tensor of that shape (None = any size), else ValueError: integers are never converted."""
    if t.dtype != torch.int32 or t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{who}: {name} must be int32 {list(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


def _mesh_image_dims(who, N, H, W):
    if N < 1 or not (1 <= H <= 4096 and 1 <= W <= 4096) or N * H * W >= 2 ** 31:
        raise ValueError(f"{who}: needs N >= 1, H and W in 1..4096 and N H W < 2^31, got (N, H, W) = {(N, H, W)}")


def op_mesh_project(verts, K, RT, z_near, device=None, lib=None):
    """mvd_op_mesh_project on ``device`` (default: verts'): verts [Nv,3], K [N,3,3], RT [N,3,4] (world -> camera), float tensors.
    Returns (xy [N,Nv,2] int32 in 1/16 pixel, key [N,Nv] int32, 0 = invalid vertex) on the device."""
    who = "op_mesh_project"
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise ValueError(f"{who}: verts must be [Nv,3] with Nv >= 1, got {tuple(verts.shape)}")
    if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or RT.dim() != 3 or tuple(RT.shape[1:]) != (3, 4) or K.shape[0] != RT.shape[0] \
            or K.shape[0] < 1:
        raise ValueError(f"{who}: K must be [N,3,3] and RT [N,3,4] with N >= 1, got {tuple(K.shape)} and {tuple(RT.shape)}")
    if not all(t.is_floating_point() for t in (verts, K, RT)):
        raise ValueError(f"{who}: verts, K and RT must be float tensors")
    z_near = float(z_near)
    if not (z_near > 0.0 and z_near < float("inf")):
        raise ValueError(f"{who}: z_near must be positive and finite, got {z_near}")
    dev = verts.device if device is None else device
    N, Nv = K.shape[0], verts.shape[0]
    v, k, rt = _f32(verts, dev), _f32(K, dev), _f32(RT, dev)
    lib = lib or L.load()
    xy = torch.zeros((N, Nv, 2), device=dev, dtype=torch.int32)
    key = torch.zeros((N, Nv), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_mesh_project(L.ptr(v), L.ptr(k), L.ptr(rt), N, Nv, z_near, L.ptr(xy), L.ptr(key), _stream()))
    return xy, key


def op_mesh_raster(xy, key, faces, H, W, device=None, lib=None):
    """mvd_op_mesh_raster on ``device`` (default: xy's): xy [N,Nv,2], key [N,Nv], faces [Nf,3], all int32.  Returns (face_id
    [N,H,W] int32, -1 = background; pix_key [N,H,W] int32, 0 = background; bad_faces [1] int32: the faces with an index outside
    [0, Nv), which were not drawn) on the device."""
    who = "op_mesh_raster"
    _i32("xy", xy, (None, None, 2), who)
    N, Nv = xy.shape[:2]
    _i32("key", key, (N, Nv), who)
    _i32("faces", faces, (None, 3), who)
    Nf, H, W = faces.shape[0], int(H), int(W)
    if Nv < 1 or Nf < 1:
        raise ValueError(f"{who}: at least one vertex and one face are needed, got Nv = {Nv}, Nf = {Nf}")
    _mesh_image_dims(who, N, H, W)
    dev = xy.device if device is None else device
    xy, key, faces = (t.detach().to(dev).contiguous() for t in (xy, key, faces))
    lib = lib or L.load()
    face_id = torch.full((N, H, W), -1, device=dev, dtype=torch.int32)
    pix_key = torch.zeros((N, H, W), device=dev, dtype=torch.int32)
    bad = torch.zeros((1,), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_mesh_raster(L.ptr(xy), L.ptr(key), L.ptr(faces), N, Nv, Nf, H, W, L.ptr(face_id), L.ptr(pix_key), L.ptr(bad),
                                       _stream()))
    return face_id, pix_key, bad


def op_mesh_vertex_colors(images, xy, key, faces, face_id, pix_key, verts, normals, centres, power=2.0, bias=4096, two_sided=False,
                          fill=(0.5, 0.5, 0.5), device=None, lib=None):
    """mvd_op_mesh_vertex_colors on ``device`` (default: images'): images [N,3,H,W] or [N,H,W,3], float (taken as [-1, 1]) or
    uint8; xy / key / faces / face_id / pix_key int32 as op_mesh_project and op_mesh_raster return them; verts / normals [Nv,3],
    centres [N,3] (the camera centres), float.  Returns a dict of device tensors: color [Nv,3], weight_sum [Nv], spread [Nv]
    (float32), n_seen [Nv] (int32), visible [N,Nv] (bool)."""
    who = "op_mesh_vertex_colors"
    if images.dim() != 4 or (images.shape[1] == 3) == (images.shape[3] == 3):
        raise ValueError(f"{who}: images must be [N,3,H,W] or [N,H,W,3], got {tuple(images.shape)}")
    if images.dtype != torch.uint8 and not images.is_floating_point():
        raise ValueError(f"{who}: images must be a float tensor or uint8, not {images.dtype}")
    dtype, layout = int(images.dtype == torch.uint8), 0 if images.shape[1] == 3 else 1
    N, H, W = (images.shape[0], images.shape[2], images.shape[3]) if layout == 0 else tuple(images.shape[:3])
    _mesh_image_dims(who, N, H, W)
    _i32("xy", xy, (N, None, 2), who)
    Nv = xy.shape[1]
    _i32("key", key, (N, Nv), who)
    _i32("faces", faces, (None, 3), who)
    _i32("face_id", face_id, (N, H, W), who)
    _i32("pix_key", pix_key, (N, H, W), who)
    Nf = faces.shape[0]
    if Nv < 1 or Nf < 1:
        raise ValueError(f"{who}: at least one vertex and one face are needed, got Nv = {Nv}, Nf = {Nf}")
    for name, t, shape in (("verts", verts, (Nv, 3)), ("normals", normals, (Nv, 3)), ("centres", centres, (N, 3))):
        if tuple(t.shape) != shape or not t.is_floating_point():
            raise ValueError(f"{who}: {name} must be a float tensor {list(shape)}, got {t.dtype} {tuple(t.shape)}")
    power, fill = float(power), tuple(float(c) for c in fill)
    if not (power >= 1.0 and power < float("inf")):
        raise ValueError(f"{who}: power must be at least 1 and finite, got {power}")
    if len(fill) != 3:
        raise ValueError(f"{who}: fill must be three numbers")
    dev = images.device if device is None else device
    img = images.detach().to(device=dev, dtype=torch.uint8 if dtype else torch.float32).contiguous()
    xy, key, faces, face_id, pix_key = (t.detach().to(dev).contiguous() for t in (xy, key, faces, face_id, pix_key))
    v, nrm, cen = _f32(verts, dev), _f32(normals, dev), _f32(centres, dev)
    lib = lib or L.load()
    nan = float("nan")
    out = {"color": torch.full((Nv, 3), nan, device=dev), "weight_sum": torch.full((Nv,), nan, device=dev),
           "n_seen": torch.full((Nv,), -1, device=dev, dtype=torch.int32), "spread": torch.full((Nv,), nan, device=dev)}
    visible = torch.zeros((N, Nv), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_mesh_vertex_colors(L.ptr(img), dtype, layout, L.ptr(xy), L.ptr(key), L.ptr(faces), L.ptr(face_id),
                                              L.ptr(pix_key), L.ptr(v), L.ptr(nrm), L.ptr(cen), N, Nv, Nf, H, W, power, int(bias),
                                              int(bool(two_sided)), fill[0], fill[1], fill[2], L.ptr(out["color"]),
                                              L.ptr(out["weight_sum"]), L.ptr(out["n_seen"]), L.ptr(out["spread"]), L.ptr(visible),
                                              _stream()))
    out["visible"] = visible.bool()
    return out


# ---- UV texture atlases (include/mvd.h: mvd_op_mesh_vertex_normals / _texel_bake / _texture_dilate / _render_uv; csrc/k_mesh_uv.hip)
def _atlas_dims(who, Ht, Wt):
    if not (1 <= Ht <= 4096 and 1 <= Wt <= 4096):
        raise ValueError(f"{who}: the atlas needs Ht and Wt in 1..4096, got {(Ht, Wt)}")


def op_mesh_vertex_normals(verts, faces, inc_ptr, inc_face, device=None, lib=None):
    """mvd_op_mesh_vertex_normals on ``device`` (default: verts'): verts [F,Nv,3] float, faces [Nf,3], inc_ptr [Nv+1] and inc_face
    [3 Nf] int32 (the vertex -> face incidence in CSR form, mesh.face_incidence).  Returns (normals [F,Nv,3] float32, bad [1] int32:
    table entries that were not dereferenced) on the device."""
    who = "op_mesh_vertex_normals"
    if not torch.is_tensor(verts) or not verts.is_floating_point() or verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[0] < 1 \
            or verts.shape[1] < 1:
        raise ValueError(f"{who}: verts must be a float tensor [F,Nv,3], got {getattr(verts, 'dtype', type(verts))} "
                         f"{tuple(getattr(verts, 'shape', ()))}")
    F, Nv = verts.shape[:2]
    _i32("faces", faces, (None, 3), who)
    Nf = faces.shape[0]
    if Nf < 1:
        raise ValueError(f"{who}: at least one face is needed")
    _i32("inc_ptr", inc_ptr, (Nv + 1,), who)
    _i32("inc_face", inc_face, (3 * Nf,), who)
    if F > 65535 or F * Nv >= 2 ** 30:
        raise ValueError(f"{who}: needs F <= 65535 and F Nv < 2^30, got (F, Nv) = {(F, Nv)}")
    dev = verts.device if device is None else device
    v = _f32(verts, dev)
    faces, inc_ptr, inc_face = (t.detach().to(dev).contiguous() for t in (faces, inc_ptr, inc_face))
    lib = lib or L.load()
    normals = torch.full((F, Nv, 3), float("nan"), device=dev)
    bad = torch.zeros((1,), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_mesh_vertex_normals(L.ptr(v), L.ptr(faces), L.ptr(inc_ptr), L.ptr(inc_face), F, Nv, Nf, L.ptr(normals),
                                               L.ptr(bad), _stream()))
    return normals, bad


def op_mesh_texel_bake(images, face_id, pix_key, K, RT, centres, z_near, verts, normals, faces, uv_xy, face_uv, tex_face, power=2.0,
                       bias=4096, two_sided=False, fill=(0.5, 0.5, 0.5), taps=True, device=None, lib=None):
    """mvd_op_mesh_texel_bake on ``device`` (default: images'): images [N,3,H,W] or [N,H,W,3], float (taken as [-1, 1]) or uint8;
    face_id / pix_key [N,H,W] int32 as op_mesh_raster returns them; K [N,3,3], RT [N,3,4], centres [N,3], verts / normals [Nv,3]
    float; faces / face_uv [Nf,3], uv_xy [Nt,2] (mesh.uv_to_atlas), tex_face [Ht,Wt] int32.  Returns a dict of device tensors:
    texture [Ht,Wt,3], weight_sum, spread [Ht,Wt] (float32), n_seen [Ht,Wt] (int32) and, with ``taps``, visible [N,Ht,Wt] (bool),
    pos [Ht,Wt,3], txy [N,Ht,Wt,2], tkey [N,Ht,Wt]: the kernel's own surface point and per-view integers."""
    who = "op_mesh_texel_bake"
    if images.dim() != 4 or (images.shape[1] == 3) == (images.shape[3] == 3):
        raise ValueError(f"{who}: images must be [N,3,H,W] or [N,H,W,3], got {tuple(images.shape)}")
    if images.dtype != torch.uint8 and not images.is_floating_point():
        raise ValueError(f"{who}: images must be a float tensor or uint8, not {images.dtype}")
    dtype, layout = int(images.dtype == torch.uint8), 0 if images.shape[1] == 3 else 1
    N, H, W = (images.shape[0], images.shape[2], images.shape[3]) if layout == 0 else tuple(images.shape[:3])
    _mesh_image_dims(who, N, H, W)
    _i32("face_id", face_id, (N, H, W), who)
    _i32("pix_key", pix_key, (N, H, W), who)
    _i32("faces", faces, (None, 3), who)
    Nf = faces.shape[0]
    _i32("face_uv", face_uv, (Nf, 3), who)
    _i32("uv_xy", uv_xy, (None, 2), who)
    _i32("tex_face", tex_face, (None, None), who)
    Nt, (Ht, Wt) = uv_xy.shape[0], tex_face.shape
    _atlas_dims(who, Ht, Wt)
    if not torch.is_tensor(verts) or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"{who}: verts must be [Nv,3]")
    Nv = verts.shape[0]
    if Nv < 1 or Nf < 1 or Nt < 1 or N * Ht * Wt >= 2 ** 31:
        raise ValueError(f"{who}: needs Nv, Nf, Nt >= 1 and N Ht Wt < 2^31, got Nv = {Nv}, Nf = {Nf}, Nt = {Nt}, atlas {(Ht, Wt)}")
    for name, t, shape in (("verts", verts, (Nv, 3)), ("normals", normals, (Nv, 3)), ("centres", centres, (N, 3)), ("K", K, (N, 3, 3)),
                           ("RT", RT, (N, 3, 4))):
        if not torch.is_tensor(t) or tuple(t.shape) != shape or not t.is_floating_point():
            raise ValueError(f"{who}: {name} must be a float tensor {list(shape)}, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    power, fill, z_near = float(power), tuple(float(c) for c in fill), float(z_near)
    if not (power >= 1.0 and power < float("inf")):
        raise ValueError(f"{who}: power must be at least 1 and finite, got {power}")
    if not (z_near > 0.0 and z_near < float("inf")):
        raise ValueError(f"{who}: z_near must be positive and finite, got {z_near}")
    if len(fill) != 3:
        raise ValueError(f"{who}: fill must be three numbers")
    dev = images.device if device is None else device
    img = images.detach().to(device=dev, dtype=torch.uint8 if dtype else torch.float32).contiguous()
    face_id, pix_key, faces, uv_xy, face_uv, tex_face = (t.detach().to(dev).contiguous()
                                                         for t in (face_id, pix_key, faces, uv_xy, face_uv, tex_face))
    k, rt, cen, v, nrm = (_f32(t, dev) for t in (K, RT, centres, verts, normals))
    lib = lib or L.load()
    nan = float("nan")
    out = {"texture": torch.full((Ht, Wt, 3), nan, device=dev), "weight_sum": torch.full((Ht, Wt), nan, device=dev),
           "n_seen": torch.full((Ht, Wt), -1, device=dev, dtype=torch.int32), "spread": torch.full((Ht, Wt), nan, device=dev)}
    tap = {}
    if taps:
        tap = {"visible": torch.zeros((N, Ht, Wt), device=dev, dtype=torch.uint8), "pos": torch.full((Ht, Wt, 3), nan, device=dev),
               "txy": torch.zeros((N, Ht, Wt, 2), device=dev, dtype=torch.int32),
               "tkey": torch.zeros((N, Ht, Wt), device=dev, dtype=torch.int32)}
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_mesh_texel_bake(L.ptr(img), dtype, layout, L.ptr(face_id), L.ptr(pix_key), L.ptr(k), L.ptr(rt), L.ptr(cen), z_near,
                                           L.ptr(v), L.ptr(nrm), L.ptr(faces), L.ptr(uv_xy), L.ptr(face_uv), L.ptr(tex_face), N, Nv, Nf, Nt,
                                           H, W, Ht, Wt, power, int(bias), int(bool(two_sided)), fill[0], fill[1], fill[2],
                                           L.ptr(out["texture"]), L.ptr(out["weight_sum"]), L.ptr(out["n_seen"]), L.ptr(out["spread"]),
                                           L.ptr(tap.get("visible")), L.ptr(tap.get("pos")), L.ptr(tap.get("txy")), L.ptr(tap.get("tkey")),
                                           _stream()))
    if taps:
        tap["visible"] = tap["visible"].bool()
    out.update(tap)
    return out


def op_mesh_texture_dilate(texture, valid, passes, device=None, lib=None):
    """mvd_op_mesh_texture_dilate on ``device`` (default: texture's): texture [Ht,Wt,3] float, valid [Ht,Wt] (bool or uint8, nonzero =
    valid), passes in 0..64.  Returns (texture [Ht,Wt,3] float32, valid [Ht,Wt] bool) after ``passes`` rounds; the inputs stay."""
    who = "op_mesh_texture_dilate"
    if not torch.is_tensor(texture) or not texture.is_floating_point() or texture.dim() != 3 or texture.shape[2] != 3:
        raise ValueError(f"{who}: texture must be a float tensor [Ht,Wt,3], got {tuple(getattr(texture, 'shape', ()))}")
    Ht, Wt = texture.shape[:2]
    _atlas_dims(who, Ht, Wt)
    if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (Ht, Wt):
        raise ValueError(f"{who}: valid must be bool or uint8 {[Ht, Wt]}, got {getattr(valid, 'dtype', type(valid))} "
                         f"{tuple(getattr(valid, 'shape', ()))}")
    passes = int(passes)
    if not 0 <= passes <= 64:
        raise ValueError(f"{who}: passes must be in 0..64, got {passes}")
    dev = texture.device if device is None else device
    tex = _f32(texture, dev)
    val = (valid.detach().to(dev) != 0).to(torch.uint8).contiguous()
    lib = lib or L.load()
    tex_out = torch.full((Ht, Wt, 3), float("nan"), device=dev)
    val_out = torch.zeros((Ht, Wt), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_mesh_texture_dilate(L.ptr(tex), L.ptr(val), Ht, Wt, passes, L.ptr(tex_out), L.ptr(val_out), _stream()))
    return tex_out, val_out.bool()


def op_mesh_render_uv(xy, key, face_id, faces, face_uv, uv, texture, background=(1.0, 1.0, 1.0), layout="nchw", device=None, lib=None):
    """mvd_op_mesh_render_uv on ``device`` (default: xy's): xy [N,Nv,2], key [N,Nv], face_id [N,H,W] int32 as op_mesh_project and
    op_mesh_raster return them; faces / face_uv [Nf,3] int32; uv [Nt,2] float; texture [Ht,Wt,3] float in [0, 1].  Returns the
    images, float32 in [-1, 1]: [N,3,H,W] (``layout`` "nchw") or [N,H,W,3] ("nhwc"); uncovered pixels take ``background``."""
    who = "op_mesh_render_uv"
    _i32("xy", xy, (None, None, 2), who)
    N, Nv = xy.shape[:2]
    _i32("key", key, (N, Nv), who)
    _i32("face_id", face_id, (N, None, None), who)
    H, W = face_id.shape[1:]
    _i32("faces", faces, (None, 3), who)
    Nf = faces.shape[0]
    _i32("face_uv", face_uv, (Nf, 3), who)
    if Nv < 1 or Nf < 1:
        raise ValueError(f"{who}: at least one vertex and one face are needed, got Nv = {Nv}, Nf = {Nf}")
    _mesh_image_dims(who, N, H, W)
    if 3 * N * H * W >= 2 ** 31:
        raise ValueError(f"{who}: needs 3 N H W < 2^31, got (N, H, W) = {(N, H, W)}")
    if not torch.is_tensor(uv) or not uv.is_floating_point() or uv.dim() != 2 or uv.shape[1] != 2 or uv.shape[0] < 1:
        raise ValueError(f"{who}: uv must be a float tensor [Nt,2], got {tuple(getattr(uv, 'shape', ()))}")
    if not torch.is_tensor(texture) or not texture.is_floating_point() or texture.dim() != 3 or texture.shape[2] != 3:
        raise ValueError(f"{who}: texture must be a float tensor [Ht,Wt,3], got {tuple(getattr(texture, 'shape', ()))}")
    Nt, (Ht, Wt) = uv.shape[0], texture.shape[:2]
    _atlas_dims(who, Ht, Wt)
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"{who}: layout must be 'nchw' or 'nhwc', not {layout!r}")
    bg = tuple(float(c) for c in background)
    if len(bg) != 3:
        raise ValueError(f"{who}: background must be three numbers")
    dev = xy.device if device is None else device
    xy, key, face_id, faces, face_uv = (t.detach().to(dev).contiguous() for t in (xy, key, face_id, faces, face_uv))
    uvd, tex = _f32(uv, dev), _f32(texture, dev)
    lib = lib or L.load()
    images = torch.full((N, 3, H, W) if layout == "nchw" else (N, H, W, 3), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_mesh_render_uv(L.ptr(xy), L.ptr(key), L.ptr(face_id), L.ptr(faces), L.ptr(face_uv), L.ptr(uvd), L.ptr(tex), N, Nv,
                                          Nf, Nt, H, W, Ht, Wt, int(layout == "nhwc"), bg[0], bg[1], bg[2], L.ptr(images), _stream()))
    return images


# ---- closest point on a mesh (include/mvd.h: mvd_op_mesh_closest_point; csrc/k_closest.hip): context-free.
def mesh_closest_slabs(Q, Nf, lib=None):
    """mvd_mesh_closest_slabs: the slab count op_mesh_closest_point plans for Q queries against Nf faces (a host function)."""
    return int((lib or L.load()).mvd_mesh_closest_slabs(int(Q), int(Nf)))


def op_mesh_closest_point(queries, verts, faces, query_normals=None, cos_min=0.0, max_dist2=float("inf"), slabs=0, device=None, lib=None):
    """mvd_op_mesh_closest_point on ``device`` (default: queries'): queries [Q,3], verts [Nv,3] float, faces [Nf,3] int32 (a point
    cloud: faces (i, i, i)), query_normals [Q,3] float or None (no normal gate), max_dist2 = +inf for no distance gate, slabs = 0 for
    the planned count.  Returns a dict of device tensors: key [Q] int64 (the bits of the uint64 key), face [Q] int32 (-1: no
    match), bary [Q,3], point [Q,3], dist2 [Q] float32 (+inf: no match)."""
    who = "op_mesh_closest_point"
    for name, t in (("queries", queries), ("verts", verts)) + ((("query_normals", query_normals),) if query_normals is not None else ()):
        if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"{who}: {name} must be a float tensor [n,3] with n >= 1, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    _i32("faces", faces, (None, 3), who)
    Q, Nv, Nf = queries.shape[0], verts.shape[0], faces.shape[0]
    if Nf < 1:
        raise ValueError(f"{who}: at least one face is needed")
    if query_normals is not None and query_normals.shape[0] != Q:
        raise ValueError(f"{who}: query_normals must be [{Q},3], got {tuple(query_normals.shape)}")
    if 3 * max(Q, Nv, Nf) >= 2 ** 31:
        raise ValueError(f"{who}: needs 3 Q, 3 Nv and 3 Nf below 2^31, got (Q, Nv, Nf) = {(Q, Nv, Nf)}")
    cos_min, max_dist2, slabs = float(cos_min), float(max_dist2), int(slabs)
    if not max_dist2 > 0.0:
        raise ValueError(f"{who}: max_dist2 must be positive (inf: no gate), got {max_dist2}")
    if not -1.0 <= cos_min <= 1.0:
        raise ValueError(f"{who}: cos_min must be in [-1, 1], got {cos_min}")
    if slabs < 0:
        raise ValueError(f"{who}: slabs must be 0 (planned) or a positive count, got {slabs}")
    dev = queries.device if device is None else device
    q, v = _f32(queries, dev), _f32(verts, dev)
    qn = None if query_normals is None else _f32(query_normals, dev)
    faces = faces.detach().to(dev).contiguous()
    lib = lib or L.load()
    nan = float("nan")
    out = {"key": torch.zeros((Q,), device=dev, dtype=torch.int64), "face": torch.full((Q,), -2, device=dev, dtype=torch.int32),
           "bary": torch.full((Q, 3), nan, device=dev), "point": torch.full((Q, 3), nan, device=dev), "dist2": torch.full((Q,), nan, device=dev)}
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_mesh_closest_point(L.ptr(q), L.ptr(qn), L.ptr(v), L.ptr(faces), Q, Nv, Nf, cos_min, max_dist2, slabs,
                                              L.ptr(out["key"]), L.ptr(out["face"]), L.ptr(out["bary"]), L.ptr(out["point"]),
                                              L.ptr(out["dist2"]), _stream()))
    return out


# ---- the morphable-model forward (include/mvd.h: mvd_op_morph_pose / _skin / _landmarks; csrc/k_morph.hip): context-free.
MORPH_MAX_JOINTS = 64


def _float_arg(who, name, t, shape):
    """ValueError unless t is a float tensor of that shape (None = any size >= 1)."""
    if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != len(shape) or \
            any((d < 1) if s is None else (s != d) for s, d in zip(shape, t.shape)):
        raise ValueError(f"{who}: {name} must be a float tensor {list(shape)}, got {getattr(t, 'dtype', type(t))} "
                         f"{tuple(getattr(t, 'shape', ()))}")


def morph_parents(who, parents, J=None):
    """parents as a list of ints after the C entry point's own rule: parents[0] == -1 and 0 <= parents[j] < j, at most 64 joints."""
    p = [int(v) for v in (parents.tolist() if hasattr(parents, "tolist") else parents)]
    if len(p) < 1 or len(p) > MORPH_MAX_JOINTS or (J is not None and len(p) != J):
        raise ValueError(f"{who}: parents must have J = {J if J is not None else '1..64'} entries (at most {MORPH_MAX_JOINTS}), got {len(p)}")
    if p[0] != -1 or any(not (0 <= p[j] < j) for j in range(1, len(p))):
        raise ValueError(f"{who}: parents[0] must be -1 and 0 <= parents[j] < j, got {p}")
    return p


def op_morph_pose(betas, pose, j_template, j_dirs, parents, device=None, lib=None):
    """mvd_op_morph_pose on ``device`` (default: betas'): betas [F,NB], pose [F,J,3] (axis-angle), j_template [J,3], j_dirs
    [NB,J*3] (the joint regressor folded into the template and the shape directions), parents: J host integers.  Returns a dict
    of float32 device tensors: j_rest [F,J,3], rot [F,J,3,3], pose_feature [F,9 (J-1)], joints [F,J,3] (posed), A [F,J,3,4]."""
    who = "op_morph_pose"
    _float_arg(who, "betas", betas, (None, None))
    F, NB = betas.shape
    _float_arg(who, "pose", pose, (F, None, 3))
    J = pose.shape[1]
    if J > MORPH_MAX_JOINTS:
        raise ValueError(f"{who}: at most {MORPH_MAX_JOINTS} joints, got {J}")
    _float_arg(who, "j_template", j_template, (J, 3))
    _float_arg(who, "j_dirs", j_dirs, (NB, J * 3))
    par = morph_parents(who, parents, J)
    if F * J * 12 >= 2 ** 31:
        raise ValueError(f"{who}: F J 12 must be below 2^31")
    dev = betas.device if device is None else device
    b, p, jt, jd = _f32(betas, dev), _f32(pose, dev), _f32(j_template, dev), _f32(j_dirs, dev)
    lib = lib or L.load()
    nan = float("nan")
    out = {"j_rest": torch.full((F, J, 3), nan, device=dev), "rot": torch.full((F, J, 3, 3), nan, device=dev),
           "pose_feature": torch.full((F, 9 * (J - 1)), nan, device=dev), "joints": torch.full((F, J, 3), nan, device=dev),
           "A": torch.full((F, J, 3, 4), nan, device=dev)}
    par_c = (C.c_int32 * J)(*par)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_pose(L.ptr(b), L.ptr(p), L.ptr(jt), L.ptr(jd), C.addressof(par_c), F, NB, J, L.ptr(out["j_rest"]),
                                      L.ptr(out["rot"]), L.ptr(out["pose_feature"]) if J > 1 else None, L.ptr(out["joints"]),
                                      L.ptr(out["A"]), _stream()))
    return out


def op_morph_skin(basis, v_template, coef, weights, A, post=None, n_betas=None, device=None, lib=None):
    """mvd_op_morph_skin on ``device`` (default: basis'): basis [L,3V] (shape directions [NB,3V], then pose directions
    [9 (J-1),3V]), v_template [V,3], coef [F,L], weights [V,J], A [F,J,3,4] or [F,J,12], post [3,4] or None.  n_betas: NB
    (default L - 9 (J-1)); L must be NB + 9 (J-1).  Returns verts [F,V,3] float32 on the device."""
    who = "op_morph_skin"
    _float_arg(who, "v_template", v_template, (None, 3))
    V = v_template.shape[0]
    _float_arg(who, "basis", basis, (None, 3 * V))
    Lb = basis.shape[0]
    _float_arg(who, "coef", coef, (None, Lb))
    F = coef.shape[0]
    _float_arg(who, "weights", weights, (V, None))
    J = weights.shape[1]
    if J > MORPH_MAX_JOINTS:
        raise ValueError(f"{who}: at most {MORPH_MAX_JOINTS} joints, got {J}")
    if torch.is_tensor(A) and A.dim() == 4:
        _float_arg(who, "A", A, (F, J, 3, 4))
    else:
        _float_arg(who, "A", A, (F, J, 12))
    NB = Lb - 9 * (J - 1) if n_betas is None else int(n_betas)
    if NB < 1 or Lb != NB + 9 * (J - 1):
        raise ValueError(f"{who}: basis has L = {Lb} rows, which must be NB + 9 (J - 1) with NB >= 1 (J = {J}, NB = {NB})")
    if post is not None:
        _float_arg(who, "post", post, (3, 4))
    if F * V * 3 >= 2 ** 31:
        raise ValueError(f"{who}: F V 3 must be below 2^31, got F = {F}, V = {V}")
    dev = basis.device if device is None else device
    bs, vt, cf, wt, a = _f32(basis, dev), _f32(v_template, dev), _f32(coef, dev), _f32(weights, dev), _f32(A, dev)
    ps = None if post is None else _f32(post, dev)
    lib = lib or L.load()
    verts = torch.full((F, V, 3), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_skin(L.ptr(bs), L.ptr(vt), L.ptr(cf), L.ptr(wt), L.ptr(a), L.ptr(ps), F, V, Lb, NB, J, L.ptr(verts),
                                      _stream()))
    return verts


def op_morph_landmarks(verts, faces, lmk_face, lmk_bary, device=None, lib=None):
    """mvd_op_morph_landmarks on ``device`` (default: verts'): verts [F,V,3] float, faces [Nf,3] and lmk_face [M] int32, lmk_bary
    [M,3] float.  Returns [F,M,3] float32 on the device; a landmark whose face or vertex index is out of range is NaN."""
    who = "op_morph_landmarks"
    _float_arg(who, "verts", verts, (None, None, 3))
    F, V = verts.shape[:2]
    _i32("faces", faces, (None, 3), who)
    _i32("lmk_face", lmk_face, (None,), who)
    Nf, M = faces.shape[0], lmk_face.shape[0]
    if Nf < 1 or M < 1:
        raise ValueError(f"{who}: at least one face and one landmark are needed, got Nf = {Nf}, M = {M}")
    _float_arg(who, "lmk_bary", lmk_bary, (M, 3))
    if F * V * 3 >= 2 ** 31 or F * M * 3 >= 2 ** 31:
        raise ValueError(f"{who}: F V 3 and F M 3 must be below 2^31")
    dev = verts.device if device is None else device
    v, bc = _f32(verts, dev), _f32(lmk_bary, dev)
    fc, lf = (t.detach().to(dev).contiguous() for t in (faces, lmk_face))
    lib = lib or L.load()
    out = torch.full((F, M, 3), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_landmarks(L.ptr(v), L.ptr(fc), L.ptr(lf), L.ptr(bc), F, V, Nf, M, L.ptr(out), _stream()))
    return out


# ---- the morphable-model backward and fitter (include/mvd.h: mvd_op_morph_skin_ex, mvd_op_morph_*_bwd, mvd_op_morph_fit_*,
# mvd_morph_fit_run; csrc/k_morph_bwd.hip): context-free.  Shapes and dtypes are checked before anything is copied.
def morph_bwd_counts(V, lib=None):
    """(chunks, slabs) of mvd_op_morph_skin_bwd's two partial buffers for V vertices: both follow from V alone."""
    lib = lib or L.load()
    return int(lib.mvd_morph_bwd_chunks(int(V))), int(lib.mvd_morph_bwd_slabs(int(V)))


def _skin_args(who, basis, v_template, coef, weights, A, post, n_betas):
    """The shape checks op_morph_skin makes, shared by the extended forward: (F, V, L, NB, J)."""
    _float_arg(who, "v_template", v_template, (None, 3))
    V = v_template.shape[0]
    _float_arg(who, "basis", basis, (None, 3 * V))
    Lb = basis.shape[0]
    _float_arg(who, "coef", coef, (None, Lb))
    F = coef.shape[0]
    _float_arg(who, "weights", weights, (V, None))
    J = weights.shape[1]
    if J > MORPH_MAX_JOINTS:
        raise ValueError(f"{who}: at most {MORPH_MAX_JOINTS} joints, got {J}")
    _float_arg(who, "A", A, (F, J, 3, 4) if torch.is_tensor(A) and A.dim() == 4 else (F, J, 12))
    NB = Lb - 9 * (J - 1) if n_betas is None else int(n_betas)
    if NB < 1 or Lb != NB + 9 * (J - 1):
        raise ValueError(f"{who}: basis has L = {Lb} rows, which must be NB + 9 (J - 1) with NB >= 1 (J = {J}, NB = {NB})")
    if post is not None:
        _float_arg(who, "post", post, (3, 4))
    if F * V * 3 >= 2 ** 31:
        raise ValueError(f"{who}: F V 3 must be below 2^31, got F = {F}, V = {V}")
    return F, V, Lb, NB, J


def op_morph_skin_ex(basis, v_template, coef, weights, A, post=None, transl=None, n_betas=None, want_blend=False, device=None, lib=None):
    """mvd_op_morph_skin_ex on ``device`` (default: basis'): op_morph_skin's arguments, an optional transl [F,3] added before post,
    and with want_blend the blended template [F,V,3] that the backward needs.  Returns verts, or (verts, blend)."""
    who = "op_morph_skin_ex"
    F, V, Lb, NB, J = _skin_args(who, basis, v_template, coef, weights, A, post, n_betas)
    if transl is not None:
        _float_arg(who, "transl", transl, (F, 3))
    dev = basis.device if device is None else device
    bs, vt, cf, wt, a = _f32(basis, dev), _f32(v_template, dev), _f32(coef, dev), _f32(weights, dev), _f32(A, dev)
    ps, tr = (None if t is None else _f32(t, dev) for t in (post, transl))
    lib = lib or L.load()
    verts = torch.full((F, V, 3), float("nan"), device=dev)
    blend = torch.full((F, V, 3), float("nan"), device=dev) if want_blend else None
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_skin_ex(L.ptr(bs), L.ptr(vt), L.ptr(cf), L.ptr(wt), L.ptr(a), L.ptr(ps), L.ptr(tr), F, V, Lb, NB, J,
                                         L.ptr(verts), L.ptr(blend), _stream()))
    return (verts, blend) if want_blend else verts


def sum_partials(part):
    """A partial buffer [n, ...] summed over its first axis in ascending order starting from part[0], in float32: the order of
    the kernels that consume mvd_op_morph_skin_bwd's partials."""
    s = part[0].clone()
    for i in range(1, part.shape[0]):
        s += part[i]
    return s


def op_morph_skin_bwd(g_y, weights, A, blend, basis, post=None, n_betas=None, device=None, lib=None):
    """mvd_op_morph_skin_bwd on ``device`` (default: basis'): g_y [F,V,3], weights [V,J], A [F,J,3,4] or [F,J,12], blend [F,V,3]
    (op_morph_skin_ex's), basis [L,3V], post [3,4] or None.  Returns a dict of float32 device tensors: g_b [F,V,3], part_a
    [chunks,F,J*12+3], part_c [slabs,F,L], and their ascending sums g_A [F,J,3,4], g_transl [F,3], g_coef [F,L]."""
    who = "op_morph_skin_bwd"
    _float_arg(who, "g_y", g_y, (None, None, 3))
    F, V = g_y.shape[:2]
    _float_arg(who, "basis", basis, (None, 3 * V))
    Lb = basis.shape[0]
    _float_arg(who, "weights", weights, (V, None))
    J = weights.shape[1]
    if J > MORPH_MAX_JOINTS:
        raise ValueError(f"{who}: at most {MORPH_MAX_JOINTS} joints, got {J}")
    _float_arg(who, "A", A, (F, J, 3, 4) if torch.is_tensor(A) and A.dim() == 4 else (F, J, 12))
    _float_arg(who, "blend", blend, (F, V, 3))
    NB = Lb - 9 * (J - 1) if n_betas is None else int(n_betas)
    if NB < 1 or Lb != NB + 9 * (J - 1):
        raise ValueError(f"{who}: basis has L = {Lb} rows, which must be NB + 9 (J - 1) with NB >= 1 (J = {J}, NB = {NB})")
    if post is not None:
        _float_arg(who, "post", post, (3, 4))
    lib = lib or L.load()
    nchunk, nslab = morph_bwd_counts(V, lib)
    if F * V * 3 >= 2 ** 31 or nslab * F * Lb >= 2 ** 31 or nchunk * F * (J * 12 + 3) >= 2 ** 31:
        raise ValueError(f"{who}: F V 3 and the partial buffers must be below 2^31 elements, got F = {F}, V = {V}")
    dev = basis.device if device is None else device
    gy, wt, a, bl, bs = _f32(g_y, dev), _f32(weights, dev), _f32(A, dev), _f32(blend, dev), _f32(basis, dev)
    ps = None if post is None else _f32(post, dev)
    nan = float("nan")
    out = {"g_b": torch.full((F, V, 3), nan, device=dev), "part_a": torch.full((nchunk, F, J * 12 + 3), nan, device=dev),
           "part_c": torch.full((nslab, F, Lb), nan, device=dev)}
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_skin_bwd(L.ptr(gy), L.ptr(ps), L.ptr(wt), L.ptr(a), L.ptr(bl), L.ptr(bs), F, V, Lb, NB, J,
                                          L.ptr(out["g_b"]), L.ptr(out["part_a"]), L.ptr(out["part_c"]), _stream()))
    sa = sum_partials(out["part_a"])
    out["g_A"], out["g_transl"], out["g_coef"] = sa[:, :J * 12].reshape(F, J, 3, 4), sa[:, J * 12:], sum_partials(out["part_c"])
    return out


def op_morph_pose_bwd(pose, j_rest, A, j_dirs, parents, part_a, part_c, g_joints=None, device=None, lib=None):
    """mvd_op_morph_pose_bwd on ``device`` (default: pose's): pose [F,J,3], j_rest [F,J,3] and A [F,J,3,4] or [F,J,12] as
    op_morph_pose returned them, j_dirs [NB,J*3], parents, the partials of op_morph_skin_bwd (part_a [chunks,F,J*12+3], part_c
    [slabs,F,NB+9(J-1)]; a single "chunk" holding g_A | g_transl and a single "slab" holding g_coef are the plain adjoints),
    g_joints [F,J,3] or None.  Returns {"betas" [F,NB], "pose" [F,J,3], "transl" [F,3]}."""
    who = "op_morph_pose_bwd"
    _float_arg(who, "pose", pose, (None, None, 3))
    F, J = pose.shape[:2]
    if J > MORPH_MAX_JOINTS:
        raise ValueError(f"{who}: at most {MORPH_MAX_JOINTS} joints, got {J}")
    _float_arg(who, "j_rest", j_rest, (F, J, 3))
    _float_arg(who, "A", A, (F, J, 3, 4) if torch.is_tensor(A) and A.dim() == 4 else (F, J, 12))
    _float_arg(who, "j_dirs", j_dirs, (None, J * 3))
    NB = j_dirs.shape[0]
    par = morph_parents(who, parents, J)
    _float_arg(who, "part_a", part_a, (None, F, J * 12 + 3))
    _float_arg(who, "part_c", part_c, (None, F, NB + 9 * (J - 1)))
    if g_joints is not None:
        _float_arg(who, "g_joints", g_joints, (F, J, 3))
    if max(part_a.numel(), part_c.numel()) >= 2 ** 31:
        raise ValueError(f"{who}: the partial buffers must be below 2^31 elements")
    dev = pose.device if device is None else device
    p, jr, a, jd, pa, pc = (_f32(t, dev) for t in (pose, j_rest, A, j_dirs, part_a, part_c))
    gj = None if g_joints is None else _f32(g_joints, dev)
    lib = lib or L.load()
    nan = float("nan")
    out = {"betas": torch.full((F, NB), nan, device=dev), "pose": torch.full((F, J, 3), nan, device=dev),
           "transl": torch.full((F, 3), nan, device=dev)}
    par_c = (C.c_int32 * J)(*par)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_pose_bwd(L.ptr(p), L.ptr(jr), L.ptr(a), L.ptr(jd), C.addressof(par_c), L.ptr(pa), pa.shape[0], L.ptr(pc),
                                          pc.shape[0], L.ptr(gj), F, NB, J, L.ptr(out["betas"]), L.ptr(out["pose"]),
                                          L.ptr(out["transl"]), _stream()))
    return out


def landmark_csr(faces, lmk_face, lmk_bary, V):
    """The vertex -> (landmark, corner) table of a static embedding, built on the host: (csr_ptr [V+1], csr_ent [3M]) int32 numpy
    arrays, the entries landmark * 3 + corner of vertex v at csr_ent[csr_ptr[v] : csr_ptr[v+1]], ascending."""
    import numpy as np
    faces, lmk_face = np.asarray(faces, dtype=np.int64), np.asarray(lmk_face, dtype=np.int64).reshape(-1)
    vert = faces[lmk_face].reshape(-1)  # vertex of entry landmark * 3 + corner
    if vert.size and (vert.min() < 0 or vert.max() >= V):
        raise ValueError(f"landmark_csr: a landmark's face names a vertex outside 0..{V - 1}")
    order = np.argsort(vert, kind="stable")  # stable: ascending entries within a vertex
    ptr = np.zeros(V + 1, dtype=np.int64)
    np.add.at(ptr, vert + 1, 1)
    return np.cumsum(ptr).astype(np.int32), order.astype(np.int32)


def _csr_args(who, csr_ptr, csr_ent, lmk_bary, V):
    _i32("csr_ptr", csr_ptr, (V + 1,), who)
    _i32("csr_ent", csr_ent, (None,), who)
    _float_arg(who, "lmk_bary", lmk_bary, (None, 3))
    if csr_ent.shape[0] < 1:
        raise ValueError(f"{who}: the landmark table is empty")
    return lmk_bary.shape[0], csr_ent.shape[0]


def op_morph_landmarks_bwd(g_lmk, csr_ptr, csr_ent, lmk_bary, V, g_in=None, device=None, lib=None):
    """mvd_op_morph_landmarks_bwd on ``device`` (default: g_lmk's): g_lmk [F,M,3], the table of landmark_csr as int32 tensors,
    lmk_bary [M,3], g_in [F,V,3] or None.  Returns g_verts [F,V,3] = g_in + the gathered landmark adjoint."""
    who = "op_morph_landmarks_bwd"
    V = int(V)
    M, n_ent = _csr_args(who, csr_ptr, csr_ent, lmk_bary, V)
    _float_arg(who, "g_lmk", g_lmk, (None, M, 3))
    F = g_lmk.shape[0]
    if g_in is not None:
        _float_arg(who, "g_in", g_in, (F, V, 3))
    if F * V * 3 >= 2 ** 31 or F * M * 3 >= 2 ** 31:
        raise ValueError(f"{who}: F V 3 and F M 3 must be below 2^31")
    dev = g_lmk.device if device is None else device
    gl, bc = _f32(g_lmk, dev), _f32(lmk_bary, dev)
    gi = None if g_in is None else _f32(g_in, dev)
    cp, ce = (t.detach().to(dev).contiguous() for t in (csr_ptr, csr_ent))
    lib = lib or L.load()
    out = torch.full((F, V, 3), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_landmarks_bwd(L.ptr(gl), L.ptr(gi), L.ptr(cp), L.ptr(ce), L.ptr(bc), F, V, M, n_ent, L.ptr(out), _stream()))
    return out


def _fit_data_args(who, F, V, target, vertex_weight, lmk, target_lmk, lmk_weight, lmk_lambda, csr, dev):
    """The data term's arguments checked and on the device: (target, frames, vw, inv_vw_sum, lmk, target_lmk, frames, lw, lmk_scale,
    csr_ptr, csr_ent, lmk_bary, M, n_ent).  The two weight sums are taken here, on the host, once."""
    if target is None and target_lmk is None:
        raise ValueError(f"{who}: give target vertices, target landmarks or both")
    tg = vw = tl = lw = cp = ce = bc = None
    tf = tlf = 1
    inv_vw, scale, M, n_ent = 0.0, 0.0, 0, 0
    if vertex_weight is not None and target is None:
        raise ValueError(f"{who}: vertex_weight without target vertices")
    if target is not None:
        _float_arg(who, "target", target, (None, V, 3))
        tf = target.shape[0]
        if tf not in (1, F):
            raise ValueError(f"{who}: target must have 1 or F = {F} frames, got {tf}")
        tg, total = _f32(target, dev), float(V)
        if vertex_weight is not None:
            _float_arg(who, "vertex_weight", vertex_weight, (V,))
            vw = _f32(vertex_weight, dev)
            total = float(vw.double().sum())
            if not (float(vw.min()) >= 0.0 and 0.0 < total < float("inf")):
                raise ValueError(f"{who}: vertex_weight must be non-negative with a positive finite sum")
        inv_vw = 1.0 / total
    if lmk_weight is not None and target_lmk is None:
        raise ValueError(f"{who}: landmark_weight without target landmarks")
    if target_lmk is not None:
        if csr is None or lmk is None:
            raise ValueError(f"{who}: target landmarks need a model with a landmark embedding")
        cp, ce, bc = csr
        M, n_ent = _csr_args(who, cp, ce, bc, V)
        _float_arg(who, "lmk", lmk, (F, M, 3))
        _float_arg(who, "target_lmk", target_lmk, (None, M, 3))
        tlf = target_lmk.shape[0]
        if tlf not in (1, F):
            raise ValueError(f"{who}: target_lmk must have 1 or F = {F} frames, got {tlf}")
        lmk_lambda = float(lmk_lambda)
        if not (0.0 <= lmk_lambda < float("inf")):
            raise ValueError(f"{who}: lmk_lambda must be non-negative and finite, got {lmk_lambda}")
        tl, total = _f32(target_lmk, dev), float(M)
        if lmk_weight is not None:
            _float_arg(who, "lmk_weight", lmk_weight, (M,))
            lw = _f32(lmk_weight, dev)
            total = float(lw.double().sum())
            if not (float(lw.min()) >= 0.0 and 0.0 < total < float("inf")):
                raise ValueError(f"{who}: lmk_weight must be non-negative with a positive finite sum")
        scale = lmk_lambda / total
        lmk, bc = _f32(lmk, dev), _f32(bc, dev)
        cp, ce = (t.detach().to(dev).contiguous() for t in (cp, ce))
    if F > 65535 or F * V * 3 >= 2 ** 31:
        raise ValueError(f"{who}: at most 65535 frames and F V 3 below 2^31, got F = {F}, V = {V}")
    return tg, tf, vw, inv_vw, (lmk if target_lmk is not None else None), tl, tlf, lw, scale, cp, ce, bc, M, n_ent


def op_morph_fit_data(verts, target=None, vertex_weight=None, lmk=None, target_lmk=None, lmk_weight=None, lmk_lambda=1.0, csr=None,
                      device=None, lib=None):
    """mvd_op_morph_fit_data on ``device`` (default: verts'): verts [F,V,3]; target [F,V,3] or [1,V,3] with an optional
    vertex_weight [V]; lmk [F,M,3] (the landmarks of verts), target_lmk [F,M,3] or [1,M,3], an optional lmk_weight [M] and
    csr = (csr_ptr, csr_ent, lmk_bary) as int32 / float tensors.  E_f = sum_v w |y - t|^2 / sum_v w + lmk_lambda sum_m w' |l -
    l'|^2 / sum_m w'.  Returns (E [F], g_y [F,V,3] = dE_f / dverts_f with the landmark term gathered through the table)."""
    who = "op_morph_fit_data"
    _float_arg(who, "verts", verts, (None, None, 3))
    F, V = verts.shape[:2]
    dev = verts.device if device is None else device
    tg, tf, vw, inv_vw, lm, tl, tlf, lw, scale, cp, ce, bc, M, n_ent = _fit_data_args(who, F, V, target, vertex_weight, lmk, target_lmk,
                                                                                      lmk_weight, lmk_lambda, csr, dev)
    y = _f32(verts, dev)
    lib = lib or L.load()
    nan = float("nan")
    g_y, E = torch.full((F, V, 3), nan, device=dev), torch.full((F,), nan, device=dev)
    e_part = torch.full((morph_bwd_counts(V, lib)[0], F), nan, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_fit_data(L.ptr(y), L.ptr(tg), tf, L.ptr(vw), inv_vw, L.ptr(lm), L.ptr(tl), tlf, L.ptr(lw), scale,
                                          L.ptr(cp), L.ptr(ce), L.ptr(bc), F, V, M, n_ent, L.ptr(g_y), L.ptr(e_part), L.ptr(E), _stream()))
    return E, g_y


def _corr_args(who, F, V, vertex_weight, lmk, target_lmk, lmk_weight, lmk_lambda, csr, dev):
    """The correspondence data term's arguments checked and on the device: (vw, lmk, target_lmk, frames, lw, lmk_scale, csr_ptr,
    csr_ent, lmk_bary, M, n_ent).  The vertex normaliser is the device's (it depends on what matched); the landmarks' is taken here."""
    vw = None
    if vertex_weight is not None:
        _float_arg(who, "vertex_weight", vertex_weight, (V,))
        vw = _f32(vertex_weight, dev)
        if not (float(vw.min()) >= 0.0 and float(vw.double().sum()) < float("inf")):
            raise ValueError(f"{who}: vertex_weight must be non-negative and finite")
    if target_lmk is None:
        if lmk_weight is not None:
            raise ValueError(f"{who}: landmark_weight without target landmarks")
        if F > 65535 or F * V * 3 >= 2 ** 31:
            raise ValueError(f"{who}: at most 65535 frames and F V 3 below 2^31, got F = {F}, V = {V}")
        return vw, None, None, 1, None, 0.0, None, None, None, 0, 0
    _, _, _, _, lm, tl, tlf, lw, scale, cp, ce, bc, M, n_ent = _fit_data_args(who, F, V, None, None, lmk, target_lmk, lmk_weight, lmk_lambda,
                                                                             csr, dev)
    return vw, lm, tl, tlf, lw, scale, cp, ce, bc, M, n_ent


def op_morph_fit_data_corr(verts, corr_point, corr_face, vertex_weight=None, lmk=None, target_lmk=None, lmk_weight=None, lmk_lambda=1.0,
                           csr=None, device=None, lib=None):
    """mvd_op_morph_fit_data_corr on ``device`` (default: verts'): verts, corr_point [F,V,3] float, corr_face [F,V] int32 (as
    op_mesh_closest_point returns point and face for the vertices as queries; < 0 = no match, and that corr_point is never
    read); the landmark arguments of op_morph_fit_data.  E_f = sum_v w m |y - c|^2 / W_f + the landmark term, W_f = sum_v w m.
    Returns (E [F], g_y [F,V,3], n_matched [F] int32)."""
    who = "op_morph_fit_data_corr"
    _float_arg(who, "verts", verts, (None, None, 3))
    F, V = verts.shape[:2]
    _float_arg(who, "corr_point", corr_point, (F, V, 3))
    _i32("corr_face", corr_face, (F, V), who)
    dev = verts.device if device is None else device
    vw, lm, tl, tlf, lw, scale, cp, ce, bc, M, n_ent = _corr_args(who, F, V, vertex_weight, lmk, target_lmk, lmk_weight, lmk_lambda, csr, dev)
    y, c, cf = _f32(verts, dev), _f32(corr_point, dev), corr_face.detach().to(dev).contiguous()
    lib = lib or L.load()
    nan = float("nan")
    g_y, E = torch.full((F, V, 3), nan, device=dev), torch.full((F,), nan, device=dev)
    nblk = morph_bwd_counts(V, lib)[0]
    e_part, w_part = torch.full((nblk, F), nan, device=dev), torch.full((nblk + 1, F), nan, device=dev)
    n_matched = torch.full((F,), -1, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_fit_data_corr(L.ptr(y), L.ptr(c), L.ptr(cf), L.ptr(vw), L.ptr(lm), L.ptr(tl), tlf, L.ptr(lw), scale,
                                               L.ptr(cp), L.ptr(ce), L.ptr(bc), F, V, M, n_ent, L.ptr(g_y), L.ptr(e_part), L.ptr(w_part),
                                               L.ptr(E), L.ptr(n_matched), _stream()))
    return E, g_y, n_matched


ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8  # torch.optim.Adam's defaults


def _fit_update_args(who, p, m, v, lr, lam, p0):
    for name, t in (("p", p), ("m", m), ("v", v)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda or \
                t.shape != p.shape or t.device != p.device:
            raise ValueError(f"{who}: {name} must be a contiguous float32 device tensor [F,P] (updated in place), got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    F, P = p.shape
    if F < 1 or P < 1 or F * P >= 2 ** 31:
        raise ValueError(f"{who}: p must be [F,P] with F, P >= 1 and F P < 2^31, got {tuple(p.shape)}")
    for name, t in (("lr", lr), ("lam", lam), ("p0", p0)):
        _float_arg(who, name, t, (P,))
    return F, P


def op_morph_fit_update(p, g, m, v, lr, lam, p0, step, betas=ADAM_BETAS, eps=ADAM_EPS, lib=None):
    """mvd_op_morph_fit_update: p, m, v [F,P] float32 device tensors, updated IN PLACE; g [F,P]; lr, lam, p0 [P]; step >= 1.
    g' = g + 2 lam (p - p0), then torch.optim.Adam's step; a column with lr == 0 keeps the bits of p, m and v."""
    who = "op_morph_fit_update"
    F, P = _fit_update_args(who, p, m, v, lr, lam, p0)
    _float_arg(who, "g", g, (F, P))
    step, b1, b2, eps = int(step), float(betas[0]), float(betas[1]), float(eps)
    if step < 1 or not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps > 0.0):
        raise ValueError(f"{who}: step must be at least 1, betas in [0, 1) and eps positive, got {step}, {betas}, {eps}")
    dev = p.device
    gg, lrd, lamd, p0d = (_f32(t, dev) for t in (g, lr, lam, p0))
    lib = lib or L.load()
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_fit_update(L.ptr(p), L.ptr(gg), L.ptr(m), L.ptr(v), L.ptr(lrd), L.ptr(lamd), L.ptr(p0d), F, P, step,
                                            b1, b2, eps, _stream()))


def morph_fit_run(model, p, m, v, lr, lam, p0, iters, target=None, vertex_weight=None, target_lmk=None, lmk_weight=None, lmk_lambda=1.0,
                  post=None, step0=0, betas=ADAM_BETAS, eps=ADAM_EPS, lib=None):
    """mvd_morph_fit_run: ``iters`` Adam iterations enqueued without a host synchronisation between them.  model: an object with
    the device tensors of morphable.MorphableModel (basis, v_template, weights, j_template, j_dirs, parents, faces, lmk_face,
    lmk_bary, csr_ptr, csr_ent).  p, m, v [F,P] with P = NB + 3 J + 3 (betas | pose | transl), float32 on the model's device,
    updated IN PLACE; lr, lam, p0 [P].  Returns loss_history [iters,F]."""
    who = "morph_fit_run"
    F, P = _fit_update_args(who, p, m, v, lr, lam, p0)
    V, NB, J = model.v_template.shape[0], model.j_dirs.shape[0], model.weights.shape[1]
    if P != NB + 3 * J + 3:
        raise ValueError(f"{who}: p must have P = NB + 3 J + 3 = {NB + 3 * J + 3} columns, got {P}")
    dev = p.device
    if model.basis.device != dev:
        raise ValueError(f"{who}: the model is on {model.basis.device}, the parameters on {dev}")
    iters, step0, b1, b2, eps = int(iters), int(step0), float(betas[0]), float(betas[1]), float(eps)
    if iters < 1 or step0 < 0 or iters * F >= 2 ** 31 or not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps > 0.0):
        raise ValueError(f"{who}: iters must be at least 1 (iters F < 2^31), step0 at least 0, betas in [0, 1), eps positive")
    if post is not None:
        _float_arg(who, "post", post, (3, 4))
    use_lmk = target_lmk is not None
    csr = (model.csr_ptr, model.csr_ent, model.lmk_bary) if use_lmk and getattr(model, "csr_ptr", None) is not None else None
    lmk_stub = torch.empty((F, model.lmk_bary.shape[0], 3), device=dev) if csr is not None else None  # shape check only
    tg, tf, vw, inv_vw, _, tl, tlf, lw, scale, cp, ce, bc, M, n_ent = _fit_data_args(who, F, V, target, vertex_weight, lmk_stub, target_lmk,
                                                                                     lmk_weight, lmk_lambda, csr, dev)
    par = morph_parents(who, model.parents, J)
    lrd, lamd, p0d = (_f32(t, dev) for t in (lr, lam, p0))
    ps = None if post is None else _f32(post, dev)
    lib = lib or L.load()
    n_ws_c = C.c_int64(0)
    L.check(lib.mvd_morph_fit_workspace(F, V, NB, J, M, C.addressof(n_ws_c)))
    n_ws = int(n_ws_c.value)
    ws = torch.full((n_ws,), float("nan"), device=dev)
    hist = torch.full((iters, F), float("nan"), device=dev)
    par_c = (C.c_int32 * J)(*par)
    fc, lf = (model.faces, model.lmk_face) if use_lmk else (None, None)
    with torch.cuda.device(dev):
        L.check(lib.mvd_morph_fit_run(L.ptr(model.basis), L.ptr(model.v_template), L.ptr(model.weights), L.ptr(model.j_template),
                                      L.ptr(model.j_dirs), C.addressof(par_c), L.ptr(ps), L.ptr(fc), L.ptr(lf), L.ptr(bc), L.ptr(cp),
                                      L.ptr(ce), F, V, NB, J, 0 if fc is None else fc.shape[0], M, n_ent, L.ptr(tg), tf, L.ptr(vw),
                                      inv_vw, L.ptr(tl), tlf, L.ptr(lw), scale, L.ptr(p), L.ptr(m), L.ptr(v), L.ptr(lrd), L.ptr(lamd),
                                      L.ptr(p0d), iters, step0, b1, b2, eps, L.ptr(ws), n_ws, L.ptr(hist), _stream()))
    return hist


def scan_args(who, scans, F):
    """``scans``: a list of (verts [n,3] float, faces [k,3] int32) tensors, one shared or one per frame -> (scan_verts [sum n,3],
    scan_faces [sum k,3], vptr, fptr as host lists [Fs+1]); face indices stay local to their scan."""
    if not isinstance(scans, (list, tuple)) or len(scans) not in (1, F):
        raise ValueError(f"{who}: one scan, or one per frame (F = {F}), got {len(scans) if isinstance(scans, (list, tuple)) else type(scans)}")
    vptr, fptr = [0], [0]
    for i, sc in enumerate(scans):
        if not isinstance(sc, (list, tuple)) or len(sc) != 2:
            raise ValueError(f"{who}: scan {i} must be a (verts, faces) pair")
        sv, sf = sc
        if not torch.is_tensor(sv) or not sv.is_floating_point() or sv.dim() != 2 or sv.shape[1] != 3 or sv.shape[0] < 1:
            raise ValueError(f"{who}: the vertices of scan {i} must be a float tensor [n,3] with n >= 1")
        _i32(f"the faces of scan {i}", sf, (None, 3), who)
        if sf.shape[0] < 1:
            raise ValueError(f"{who}: scan {i} has no face (a point cloud is passed as faces (i, i, i))")
        if 3 * max(sv.shape[0], sf.shape[0]) >= 2 ** 31:
            raise ValueError(f"{who}: scan {i} is too large: 3 Nv and 3 Nf must be below 2^31")
        vptr.append(vptr[-1] + sv.shape[0])
        fptr.append(fptr[-1] + sf.shape[0])
    if 3 * max(vptr[-1], fptr[-1]) >= 2 ** 31:
        raise ValueError(f"{who}: the scans together are too large: 3 Nv and 3 Nf must be below 2^31")
    return vptr, fptr


def morph_fit_scan_run(model, p, m, v, lr, lam, p0, iters, scans, incidence=None, normal_cos=None, max_dist2=float("inf"), refresh=1,
                       vertex_weight=None, target_lmk=None, lmk_weight=None, lmk_lambda=1.0, post=None, step0=0, betas=ADAM_BETAS,
                       eps=ADAM_EPS, lib=None):
    """mvd_morph_fit_scan_run: morph_fit_run's loop with the target replaced by the closest points of a scan, found again every
    ``refresh`` iterations.  scans: a list of (verts, faces) device or host tensors, one shared or one per frame (scan_args).
    normal_cos: None (no normal gate) or cos_min, which needs the model's faces and incidence = (inc_ptr, inc_face) of them
    (mesh.face_incidence).  Returns (loss_history [iters,F], matched_history [iters,F] int32, corr_face [F,V] int32)."""
    who = "morph_fit_scan_run"
    F, P = _fit_update_args(who, p, m, v, lr, lam, p0)
    V, NB, J = model.v_template.shape[0], model.j_dirs.shape[0], model.weights.shape[1]
    if P != NB + 3 * J + 3:
        raise ValueError(f"{who}: p must have P = NB + 3 J + 3 = {NB + 3 * J + 3} columns, got {P}")
    dev = p.device
    if model.basis.device != dev:
        raise ValueError(f"{who}: the model is on {model.basis.device}, the parameters on {dev}")
    iters, step0, refresh, b1, b2, eps = int(iters), int(step0), int(refresh), float(betas[0]), float(betas[1]), float(eps)
    if iters < 1 or step0 < 0 or iters * F >= 2 ** 31 or not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps > 0.0):
        raise ValueError(f"{who}: iters must be at least 1 (iters F < 2^31), step0 at least 0, betas in [0, 1), eps positive")
    if refresh < 1:
        raise ValueError(f"{who}: refresh must be at least 1, got {refresh}")
    max_dist2 = float(max_dist2)
    if not max_dist2 > 0.0:
        raise ValueError(f"{who}: max_dist2 must be positive (inf: no gate), got {max_dist2}")
    gate = normal_cos is not None
    cos_min = float(normal_cos) if gate else 0.0
    if not -1.0 <= cos_min <= 1.0:
        raise ValueError(f"{who}: normal_cos must be in [-1, 1], got {cos_min}")
    ip = ic = None
    if gate:
        if model.faces is None or incidence is None:
            raise ValueError(f"{who}: the normal gate needs the model's faces and their incidence table")
        ip, ic = incidence
        _i32("inc_ptr", ip, (V + 1,), who)
        _i32("inc_face", ic, (3 * model.faces.shape[0],), who)
    if post is not None:
        _float_arg(who, "post", post, (3, 4))
    vptr, fptr = scan_args(who, scans, F)
    use_lmk = target_lmk is not None
    csr = (model.csr_ptr, model.csr_ent, model.lmk_bary) if use_lmk and getattr(model, "csr_ptr", None) is not None else None
    lmk_stub = torch.empty((F, model.lmk_bary.shape[0], 3), device=dev) if csr is not None else None  # shape check only
    vw, _, tl, tlf, lw, scale, cp, ce, bc, M, n_ent = _corr_args(who, F, V, vertex_weight, lmk_stub, target_lmk, lmk_weight, lmk_lambda, csr,
                                                                dev)
    par = morph_parents(who, model.parents, J)
    lrd, lamd, p0d = (_f32(t, dev) for t in (lr, lam, p0))
    ps = None if post is None else _f32(post, dev)
    sv = torch.cat([_f32(a, dev) for a, _ in scans])
    sf = torch.cat([b.detach().to(dev) for _, b in scans]).contiguous()
    if gate:
        ip, ic = (t.detach().to(dev).contiguous() for t in (ip, ic))
    lib = lib or L.load()
    n_ws_c = C.c_int64(0)
    L.check(lib.mvd_morph_fit_scan_workspace(F, V, NB, J, M, C.addressof(n_ws_c)))
    n_ws = int(n_ws_c.value)
    ws = torch.full((n_ws,), float("nan"), device=dev)
    hist = torch.full((iters, F), float("nan"), device=dev)
    matched = torch.full((iters, F), -1, device=dev, dtype=torch.int32)
    corr_face = torch.full((F, V), -2, device=dev, dtype=torch.int32)
    par_c = (C.c_int32 * J)(*par)
    Fs = len(scans)
    vptr_c, fptr_c = (C.c_int32 * (Fs + 1))(*vptr), (C.c_int32 * (Fs + 1))(*fptr)
    fc = model.faces if (use_lmk or gate) else None
    lf = model.lmk_face if use_lmk else None
    with torch.cuda.device(dev):
        L.check(lib.mvd_morph_fit_scan_run(
            L.ptr(model.basis), L.ptr(model.v_template), L.ptr(model.weights), L.ptr(model.j_template), L.ptr(model.j_dirs),
            C.addressof(par_c), L.ptr(ps), L.ptr(fc), L.ptr(lf), L.ptr(bc), L.ptr(cp), L.ptr(ce), L.ptr(ip), L.ptr(ic), F, V, NB, J,
            0 if fc is None else fc.shape[0], M, n_ent, L.ptr(sv), L.ptr(sf), C.addressof(vptr_c), C.addressof(fptr_c), Fs, int(gate), cos_min,
            max_dist2, refresh, L.ptr(vw), L.ptr(tl), tlf, L.ptr(lw), scale, L.ptr(p), L.ptr(m), L.ptr(v), L.ptr(lrd), L.ptr(lamd),
            L.ptr(p0d), iters, step0, b1, b2, eps, L.ptr(ws), n_ws, L.ptr(hist), L.ptr(matched), L.ptr(corr_face), _stream()))
    return hist, matched, corr_face


# ---- the 2-D multi-view landmark term and the per-view contour landmarks (include/mvd.h: mvd_op_morph_project, _fit_data_2d,
# mvd_op_morph_contour_*, mvd_morph_fit_2d_run; csrc/k_morph_2d.hip): context-free.
Z_NEAR_2D = 1e-3  # metres: a landmark nearer to a camera than this does not count


def _camera_args(who, K, RT, F):
    """K [Fc,C,3,3] and RT [Fc,C,3,4] float tensors with Fc 1 or F (a [C,3,3] / [C,3,4] pair is shared by the frames): (K, RT, Fc, C)."""
    if torch.is_tensor(K) and torch.is_tensor(RT) and K.dim() == 3 and RT.dim() == 3:
        K, RT = K[None], RT[None]
    _float_arg(who, "K", K, (None, None, 3, 3))
    Fc, C_ = K.shape[:2]
    _float_arg(who, "RT", RT, (Fc, C_, 3, 4))
    if Fc not in (1, F):
        raise ValueError(f"{who}: the cameras must have 1 or F = {F} frames, got {Fc}")
    return K, RT, Fc, C_


def _z_near(who, z_near):
    z_near = float(z_near)
    if not (0.0 < z_near < float("inf")):
        raise ValueError(f"{who}: z_near must be positive and finite, got {z_near}")
    return z_near


def op_morph_project(points, K, RT, z_near=Z_NEAR_2D, device=None, lib=None):
    """mvd_op_morph_project on ``device`` (default: points'): points [F,M,3], K [Fc,C,3,3], RT [Fc,C,3,4] (Fc 1 or F; a [C,..] pair is
    shared).  Returns (uv [F,C,M,2] float32 in pixels, mvd_op_mesh_project's convention; valid [F,C,M] int32)."""
    who = "op_morph_project"
    _float_arg(who, "points", points, (None, None, 3))
    F, M = points.shape[:2]
    K, RT, Fc, C_ = _camera_args(who, K, RT, F)
    z_near = _z_near(who, z_near)
    if F * C_ * M * 3 >= 2 ** 31:
        raise ValueError(f"{who}: F C M 2 must be below 2^31")
    dev = points.device if device is None else device
    pt, k, rt = _f32(points, dev), _f32(K, dev), _f32(RT, dev)
    lib = lib or L.load()
    uv = torch.full((F, C_, M, 2), float("nan"), device=dev)
    valid = torch.full((F, C_, M), -1, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_project(L.ptr(pt), L.ptr(k), L.ptr(rt), Fc, F, C_, M, z_near, L.ptr(uv), L.ptr(valid), _stream()))
    return uv, valid


def op_morph_project_bwd(points, K, RT, g_uv, z_near=Z_NEAR_2D, device=None, lib=None):
    """mvd_op_morph_project_bwd: the cotangent g_uv [F,C,M,2] of op_morph_project's uv pulled back to the points, g_points [F,M,3];
    a view in which the point is not valid adds nothing."""
    who = "op_morph_project_bwd"
    _float_arg(who, "points", points, (None, None, 3))
    F, M = points.shape[:2]
    K, RT, Fc, C_ = _camera_args(who, K, RT, F)
    _float_arg(who, "g_uv", g_uv, (F, C_, M, 2))
    z_near = _z_near(who, z_near)
    if F * C_ * M * 3 >= 2 ** 31:
        raise ValueError(f"{who}: F C M 2 must be below 2^31")
    dev = points.device if device is None else device
    pt, k, rt, g = _f32(points, dev), _f32(K, dev), _f32(RT, dev), _f32(g_uv, dev)
    lib = lib or L.load()
    out = torch.full((F, M, 3), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_project_bwd(L.ptr(pt), L.ptr(k), L.ptr(rt), Fc, L.ptr(g), F, C_, M, z_near, L.ptr(out), _stream()))
    return out


def _term_2d_args(who, F, C_, M, Md, target_uv, weight, dyn_target_uv, dyn_weight, z_near, px_scale, lambda2, dev):
    """The 2-D term's targets and numbers checked and on the device: (target_uv, weight, dyn_target_uv, dyn_weight, Ft, z_near,
    px_scale, lambda2).  A [C,M,2] target is shared by the frames."""
    def one(name, t, n, last):
        if t is None:
            return None, None
        t = t[None] if torch.is_tensor(t) and t.dim() == len(last) + 2 else t
        _float_arg(who, name, t, (None, C_, n) + last)
        return _f32(t, dev), t.shape[0]
    tu, ft = one("target_uv", target_uv, M, (2,))
    if tu is None:
        raise ValueError(f"{who}: target_uv is needed")
    counts = [ft]
    w, n = one("weight", weight, M, ())
    counts += [] if n is None else [n]
    du = dw = None
    if dyn_target_uv is not None:
        du, n = one("dyn_target_uv", dyn_target_uv, Md, (2,))
        counts.append(n)
        dw, n = one("dyn_weight", dyn_weight, Md, ())
        counts += [] if n is None else [n]
    elif dyn_weight is not None:
        raise ValueError(f"{who}: dyn_weight without dyn_target_uv")
    Ft = counts[0]
    if Ft not in (1, F) or any(c != Ft for c in counts):
        raise ValueError(f"{who}: the 2-D targets and their weights must all have 1 or all have F = {F} frames, got {counts}")
    z_near, px_scale, lambda2 = _z_near(who, z_near), float(px_scale), float(lambda2)
    if not (0.0 <= px_scale < float("inf") and 0.0 <= lambda2 < float("inf")):
        raise ValueError(f"{who}: px_scale and lambda2 must be finite and not negative, got {px_scale} and {lambda2}")
    if F > 65535 or F * C_ * max(M, Md, 1) * 3 >= 2 ** 31:
        raise ValueError(f"{who}: at most 65535 frames, F C M 2 and F C Md 3 below 2^31")
    return tu, w, du, dw, Ft, z_near, px_scale, lambda2


def op_morph_fit_data_2d(lmk, K, RT, target_uv, weight=None, dyn_lmk=None, dyn_target_uv=None, dyn_weight=None, z_near=Z_NEAR_2D,
                         px_scale=1.0, lambda2=1.0, E_add=None, device=None, lib=None):
    """mvd_op_morph_fit_data_2d on ``device`` (default: lmk's): lmk [F,M,3]; cameras as op_morph_project; target_uv [Ft,C,M,2] in
    pixels with an optional weight [Ft,C,M] (Ft 1 or F); optionally the contour set dyn_lmk [F,C,Md,3], dyn_target_uv [Ft,C,Md,2],
    dyn_weight [Ft,C,Md].  E2_f = lambda2 sum w |px_scale (uv - target)|^2 / W_f over the observations that count (w > 0, Z >=
    z_near, finite), W_f the sum of their weights.  Returns a dict: uv, dyn_uv (or None), E2 [F] (+ E_add), n_valid [F] int32,
    g_lmk [F,M,3], g_dyn [F,C,Md,3] (or None), inv_w [F] = 1 / W_f (0 where nothing counts)."""
    who = "op_morph_fit_data_2d"
    _float_arg(who, "lmk", lmk, (None, None, 3))
    F, M = lmk.shape[:2]
    K, RT, Fc, C_ = _camera_args(who, K, RT, F)
    if (dyn_lmk is None) != (dyn_target_uv is None):
        raise ValueError(f"{who}: dyn_lmk and dyn_target_uv go together")
    Md = 0
    if dyn_lmk is not None:
        _float_arg(who, "dyn_lmk", dyn_lmk, (F, C_, None, 3))
        Md = dyn_lmk.shape[2]
    dev = lmk.device if device is None else device
    tu, w, du, dw, Ft, z_near, px_scale, lambda2 = _term_2d_args(who, F, C_, M, Md, target_uv, weight, dyn_target_uv, dyn_weight, z_near,
                                                                 px_scale, lambda2, dev)
    if E_add is not None:
        _float_arg(who, "E_add", E_add, (F,))
    lm, k, rt = _f32(lmk, dev), _f32(K, dev), _f32(RT, dev)
    dl = None if dyn_lmk is None else _f32(dyn_lmk, dev)
    ea = None if E_add is None else _f32(E_add, dev)
    lib = lib or L.load()
    nan = float("nan")
    nblk = int(lib.mvd_morph_2d_blocks(M, Md))
    out = {"uv": torch.full((F, C_, M, 2), nan, device=dev), "dyn_uv": None if dl is None else torch.full((F, C_, Md, 2), nan, device=dev),
           "E2": torch.full((F,), nan, device=dev), "n_valid": torch.full((F,), -1, device=dev, dtype=torch.int32),
           "g_lmk": torch.full((F, M, 3), nan, device=dev), "g_dyn": None if dl is None else torch.full((F, C_, Md, 3), nan, device=dev)}
    part = torch.full((3 * nblk + 1, F), nan, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_fit_data_2d(L.ptr(lm), L.ptr(dl), L.ptr(k), L.ptr(rt), Fc, L.ptr(tu), L.ptr(w), L.ptr(du), L.ptr(dw), Ft, F, C_,
                                             M, Md, z_near, px_scale, lambda2, L.ptr(ea), L.ptr(out["uv"]), L.ptr(out["dyn_uv"]), L.ptr(part),
                                             L.ptr(out["E2"]), L.ptr(out["n_valid"]), L.ptr(out["g_lmk"]), L.ptr(out["g_dyn"]), _stream()))
    out["inv_w"] = part[3 * nblk].clone()
    return out


def op_morph_contour_select(A, RT, neck_joint, R, device=None, lib=None):
    """mvd_op_morph_contour_select on ``device`` (default: A's): A [F,J,3,4] or [F,J,12] as op_morph_pose returns it, RT [Fc,C,3,4]
    (or [C,3,4]), neck_joint in 0..J-1, R (odd) rows of the contour table.  Returns (row [F,C] int32, yaw_deg [F,C])."""
    who = "op_morph_contour_select"
    if torch.is_tensor(A) and A.dim() == 4:
        _float_arg(who, "A", A, (None, None, 3, 4))
    else:
        _float_arg(who, "A", A, (None, None, 12))
    F, J = A.shape[:2]
    RT = RT[None] if torch.is_tensor(RT) and RT.dim() == 3 else RT
    _float_arg(who, "RT", RT, (None, None, 3, 4))
    Fc, C_ = RT.shape[:2]
    neck_joint, R = int(neck_joint), int(R)
    if Fc not in (1, F) or J > MORPH_MAX_JOINTS or not 0 <= neck_joint < J or R < 1 or R % 2 == 0 or F * C_ * 12 >= 2 ** 31:
        raise ValueError(f"{who}: needs 1 or F camera frames, J <= 64, neck_joint in 0..J-1, an odd R >= 1 and F C 12 < 2^31; got "
                         f"Fc = {Fc}, F = {F}, J = {J}, neck_joint = {neck_joint}, R = {R}")
    dev = A.device if device is None else device
    a, rt = _f32(A, dev), _f32(RT, dev)
    lib = lib or L.load()
    row = torch.full((F, C_), -1, device=dev, dtype=torch.int32)
    yaw = torch.full((F, C_), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_contour_select(L.ptr(a), L.ptr(rt), Fc, F, C_, J, neck_joint, R, L.ptr(row), L.ptr(yaw), _stream()))
    return row, yaw


def op_morph_contour_landmarks(verts, faces, dyn_lmk_face, dyn_lmk_bary, row, device=None, lib=None):
    """mvd_op_morph_contour_landmarks on ``device`` (default: verts'): verts [F,V,3], faces [Nf,3] int32, the contour table
    dyn_lmk_face [R,Md] int32 and dyn_lmk_bary [R,Md,3], row [F,C] int32.  Returns dyn_lmk [F,C,Md,3]; an index out of range: NaN."""
    who = "op_morph_contour_landmarks"
    _float_arg(who, "verts", verts, (None, None, 3))
    F, V = verts.shape[:2]
    _i32("faces", faces, (None, 3), who)
    _i32("dyn_lmk_face", dyn_lmk_face, (None, None), who)
    R, Md = dyn_lmk_face.shape
    _float_arg(who, "dyn_lmk_bary", dyn_lmk_bary, (R, Md, 3))
    _i32("row", row, (F, None), who)
    C_, Nf = row.shape[1], faces.shape[0]
    if Nf < 1 or R < 1 or Md < 1 or C_ < 1 or F * V * 3 >= 2 ** 31 or F * C_ * Md * 3 >= 2 ** 31 or R * Md * 3 >= 2 ** 31:
        raise ValueError(f"{who}: needs at least one face, row, landmark and view, and F V 3, F C Md 3, R Md 3 below 2^31")
    dev = verts.device if device is None else device
    v, bc = _f32(verts, dev), _f32(dyn_lmk_bary, dev)
    fc, lf, rw = (t.detach().to(dev).contiguous() for t in (faces, dyn_lmk_face, row))
    lib = lib or L.load()
    out = torch.full((F, C_, Md, 3), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_contour_landmarks(L.ptr(v), L.ptr(fc), L.ptr(lf), L.ptr(bc), L.ptr(rw), F, C_, V, Nf, R, Md, L.ptr(out),
                                                   _stream()))
    return out


def contour_table(faces, dyn_lmk_face, V):
    """The vertex -> (row, landmark, corner) table of a contour embedding, built on the host: (ct_vert [n_list], ct_ptr [n_list+1],
    ct_ent [n_ent]) int32 numpy arrays.  ct_vert: the vertices that appear, ascending; the entries (row Md + landmark) 3 + corner of
    ct_vert[i] are ct_ent[ct_ptr[i] : ct_ptr[i+1]], ascending.  A face index outside the mesh contributes no entry."""
    import numpy as np
    faces, lf = np.asarray(faces, dtype=np.int64), np.asarray(dyn_lmk_face, dtype=np.int64)
    ok = ((lf >= 0) & (lf < len(faces))).reshape(-1)
    vert = faces[np.where(ok, lf.reshape(-1), 0)].reshape(-1)  # vertex of entry (row Md + landmark) 3 + corner
    ent = np.arange(vert.size)[np.repeat(ok, 3) & (vert >= 0) & (vert < V)]
    order = ent[np.argsort(vert[ent], kind="stable")]
    listed, counts = np.unique(vert[order], return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    return listed.astype(np.int32), ptr.astype(np.int32), order.astype(np.int32)


def op_morph_contour_bwd(g_dyn, row, table, dyn_lmk_bary, V, g_in=None, device=None, lib=None):
    """mvd_op_morph_contour_bwd on ``device`` (default: g_dyn's): g_dyn [F,C,Md,3], row [F,C] int32, table = (ct_vert, ct_ptr,
    ct_ent) of contour_table as int32 tensors, dyn_lmk_bary [R,Md,3], g_in [F,V,3] or None.  Returns g_verts [F,V,3] = g_in + the
    contour landmarks' adjoint gathered per vertex."""
    who = "op_morph_contour_bwd"
    V = int(V)
    _float_arg(who, "g_dyn", g_dyn, (None, None, None, 3))
    F, C_, Md = g_dyn.shape[:3]
    _i32("row", row, (F, C_), who)
    cv, cp, ce = table
    _i32("ct_vert", cv, (None,), who)
    n_list = cv.shape[0]
    _i32("ct_ptr", cp, (n_list + 1,), who)
    _i32("ct_ent", ce, (None,), who)
    _float_arg(who, "dyn_lmk_bary", dyn_lmk_bary, (None, Md, 3))
    R, n_ent = dyn_lmk_bary.shape[0], ce.shape[0]
    if n_list < 1 or n_ent < 1:
        raise ValueError(f"{who}: the contour table is empty")
    if g_in is not None:
        _float_arg(who, "g_in", g_in, (F, V, 3))
    if F * V * 3 >= 2 ** 31 or F * C_ * Md * 3 >= 2 ** 31 or R * Md * 3 >= 2 ** 31:
        raise ValueError(f"{who}: F V 3, F C Md 3 and R Md 3 must be below 2^31")
    dev = g_dyn.device if device is None else device
    gd, bc = _f32(g_dyn, dev), _f32(dyn_lmk_bary, dev)
    gi = None if g_in is None else _f32(g_in, dev)
    rw, cv, cp, ce = (t.detach().to(dev).contiguous() for t in (row, cv, cp, ce))
    lib = lib or L.load()
    out = torch.full((F, V, 3), float("nan"), device=dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_morph_contour_bwd(L.ptr(gd), L.ptr(gi), L.ptr(rw), L.ptr(cv), L.ptr(cp), L.ptr(ce), L.ptr(bc), F, C_, V, R, Md,
                                             n_list, n_ent, L.ptr(out), _stream()))
    return out


def morph_fit_2d_run(model, p, m, v, lr, lam, p0, iters, K, RT, target_uv, weight=None, dyn_target_uv=None, dyn_weight=None,
                     z_near=Z_NEAR_2D, px_scale=1.0, lambda2=1.0, target=None, vertex_weight=None, post=None, step0=0, betas=ADAM_BETAS,
                     eps=ADAM_EPS, lib=None):
    """mvd_morph_fit_2d_run: morph_fit_run's loop with the 2-D multi-view landmark term.  model: morph_fit_run's, with a static
    landmark embedding and, for a contour target, dyn_lmk_face / dyn_lmk_bary / ct_vert / ct_ptr / ct_ent / neck_joint.  K, RT,
    target_uv, weight, dyn_target_uv, dyn_weight: op_morph_fit_data_2d's; target [F,V,3] / vertex_weight: an optional 3-D vertex
    term added to it.  p, m, v are updated IN PLACE.  Returns (loss_history [iters,F], n_valid_history [iters,F] int32)."""
    who = "morph_fit_2d_run"
    F, P = _fit_update_args(who, p, m, v, lr, lam, p0)
    V, NB, J = model.v_template.shape[0], model.j_dirs.shape[0], model.weights.shape[1]
    if P != NB + 3 * J + 3:
        raise ValueError(f"{who}: p must have P = NB + 3 J + 3 = {NB + 3 * J + 3} columns, got {P}")
    dev = p.device
    if model.basis.device != dev:
        raise ValueError(f"{who}: the model is on {model.basis.device}, the parameters on {dev}")
    iters, step0, b1, b2, eps = int(iters), int(step0), float(betas[0]), float(betas[1]), float(eps)
    if iters < 1 or step0 < 0 or iters * F >= 2 ** 31 or not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps > 0.0):
        raise ValueError(f"{who}: iters must be at least 1 (iters F < 2^31), step0 at least 0, betas in [0, 1), eps positive")
    if post is not None:
        _float_arg(who, "post", post, (3, 4))
    if getattr(model, "csr_ptr", None) is None:
        raise ValueError(f"{who}: the 2-D term needs a model with a landmark embedding")
    M, n_ent = _csr_args(who, model.csr_ptr, model.csr_ent, model.lmk_bary, V)
    K, RT, Fc, C_ = _camera_args(who, K, RT, F)
    dyn = dyn_target_uv is not None
    df = db = cv = cp = ce = None
    R = Md = n_list = ct_n = neck = 0
    if dyn:
        if getattr(model, "dyn_lmk_face", None) is None:
            raise ValueError(f"{who}: a contour target is given, and the model has no contour tables")
        df, db, cv, cp, ce, neck = model.dyn_lmk_face, model.dyn_lmk_bary, model.ct_vert, model.ct_ptr, model.ct_ent, int(model.neck_joint)
        (R, Md), n_list, ct_n = df.shape, cv.shape[0], ce.shape[0]
        if not 0 <= neck < J:
            raise ValueError(f"{who}: neck_joint must be in 0..{J - 1}, got {neck}")
    tu, w, du, dw, Ft, z_near, px_scale, lambda2 = _term_2d_args(who, F, C_, M, Md, target_uv, weight, dyn_target_uv, dyn_weight, z_near,
                                                                 px_scale, lambda2, dev)
    tg, tf, vw, inv_vw = None, 1, None, 0.0
    if target is not None:
        tg, tf, vw, inv_vw = _fit_data_args(who, F, V, target, vertex_weight, None, None, None, 1.0, None, dev)[:4]
    elif vertex_weight is not None:
        raise ValueError(f"{who}: vertex_weight without target vertices")
    par = morph_parents(who, model.parents, J)
    lrd, lamd, p0d, k, rt = (_f32(t, dev) for t in (lr, lam, p0, K, RT))
    ps = None if post is None else _f32(post, dev)
    lib = lib or L.load()
    n_ws_c = C.c_int64(0)
    L.check(lib.mvd_morph_fit_2d_workspace(F, V, NB, J, M, Md, C_, C.addressof(n_ws_c)))
    n_ws = int(n_ws_c.value)
    ws = torch.full((n_ws,), float("nan"), device=dev)
    hist = torch.full((iters, F), float("nan"), device=dev)
    n_hist = torch.full((iters, F), -1, device=dev, dtype=torch.int32)
    par_c = (C.c_int32 * J)(*par)
    with torch.cuda.device(dev):
        L.check(lib.mvd_morph_fit_2d_run(
            L.ptr(model.basis), L.ptr(model.v_template), L.ptr(model.weights), L.ptr(model.j_template), L.ptr(model.j_dirs),
            C.addressof(par_c), L.ptr(ps), L.ptr(model.faces), L.ptr(model.lmk_face), L.ptr(model.lmk_bary), L.ptr(model.csr_ptr),
            L.ptr(model.csr_ent), L.ptr(df), L.ptr(db), L.ptr(cv), L.ptr(cp), L.ptr(ce), F, V, NB, J, model.faces.shape[0], M, n_ent, R, Md,
            n_list, ct_n, neck, L.ptr(k), L.ptr(rt), Fc, C_, L.ptr(tu), L.ptr(w), L.ptr(du), L.ptr(dw), Ft, z_near, px_scale, lambda2,
            L.ptr(tg), tf, L.ptr(vw), inv_vw, L.ptr(p), L.ptr(m), L.ptr(v), L.ptr(lrd), L.ptr(lamd), L.ptr(p0d), iters, step0, b1, b2, eps,
            L.ptr(ws), n_ws, L.ptr(hist), L.ptr(n_hist), _stream()))
    return hist, n_hist


# ---- the sparse voxel CNN's kernels one at a time (include/mvd.h: mvd_op_sparse_conv ...): context-free like op_train_loss.
# w: the 3x3x3 kernel in checkpoint layout 0 [Cout,Cin,3,3,3], 1 [Cout,3,3,3,Cin] or 2 [3,3,3,Cin,Cout]; nbr [n_out,27] int32.
SPARSE_FORMS = ("site", "mfma")  # form of mvd_op_sparse_conv / mvd_op_sparse_conv_bwd, by index


def _sparse_args(x, nbr, w, layout, form, device, lib):
    if form not in SPARSE_FORMS:
        raise ValueError(f"form must be one of {SPARSE_FORMS}, not {form!r}")
    dev = x.device if device is None else device
    x, w = _f32(x, dev), _f32(w, dev)
    nbr = nbr.detach().to(device=dev, dtype=torch.int32).contiguous()
    cin = x.shape[1]
    if x.dim() != 2 or nbr.dim() != 2 or nbr.shape[1] != 27 or w.numel() % (27 * cin):
        raise ValueError("sparse op: x [n_in,Cin], nbr [n_out,27], w with 27 * Cin * Cout elements expected")
    if nbr.numel() and (int(nbr.max()) >= x.shape[0] or int(nbr.min()) < -1):
        raise ValueError("sparse op: nbr indexes rows outside x")
    return lib or L.load(), dev, x, nbr, w, cin, w.numel() // (27 * cin), SPARSE_FORMS.index(form)


def op_sparse_conv(x, nbr, w, layout, form="mfma", scale=None, shift=None, device=None, lib=None):
    """mvd_op_sparse_conv: one production launch of a sparse layer -> [n_out,Cout]; scale / shift: the folded BatchNorm + ReLU."""
    lib, dev, x, nbr, w, cin, cout, f = _sparse_args(x, nbr, w, layout, form, device, lib)
    sc, sh = (None if t is None else _f32(t, dev) for t in (scale, shift))
    out = torch.full((nbr.shape[0], cout), float("nan"), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_sparse_conv(L.ptr(x), L.ptr(nbr), nbr.shape[0], cin, cout, L.ptr(w), int(layout), L.ptr(sc), L.ptr(sh), f,
                                       L.ptr(out), _stream()))
    return out


def op_sparse_conv_bwd(x, nbr, d_out, w, layout, form="mfma", strided=False, level0_subm=False, deterministic=False, grad_w=None,
                       poison=False, device=None, lib=None):
    """mvd_op_sparse_conv_bwd: one layer's backward as the conditioner's backward runs it -> (d_in [n_in,Cin], dW shaped like w).
    grad_w (shaped like w): the weight gradient is added to a copy of it (default zeros).  d_in starts from NaN: every element
    must be written."""
    lib, dev, x, nbr, w, cin, cout, f = _sparse_args(x, nbr, w, layout, form, device, lib)
    dy = _f32(d_out, dev).clone()  # level 0: folded in place
    if dy.shape != (nbr.shape[0], cout):
        raise ValueError(f"op_sparse_conv_bwd: d_out must be [{nbr.shape[0]},{cout}]")
    gw = torch.zeros_like(w) if grad_w is None else _f32(grad_w, dev).clone().reshape(w.shape)
    d_in = torch.full_like(x, float("nan"))
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_sparse_conv_bwd(L.ptr(x), L.ptr(nbr), L.ptr(dy), x.shape[0], nbr.shape[0], cin, cout, bool(strided),
                                           bool(level0_subm), bool(deterministic), f, L.ptr(w), int(layout), bool(poison),
                                           L.ptr(d_in), L.ptr(gw), _stream()))
    return d_in, gw


def op_bn_rows_relu(x, gamma, beta, eps=1e-3, running=None, momentum=0.01, inplace=False, want_stats=True, device=None, lib=None):
    """mvd_op_bn_rows_relu: train-mode BatchNorm1d + ReLU over x [n,C] -> (y, stats [2,C] = [mean | rstd] or None, running).
    running = (mean, var): copies of them are updated with ``momentum`` and returned; inplace: y aliases the kernel's input."""
    lib = lib or L.load()
    dev = x.device if device is None else device
    x, g, b = _f32(x, dev), _f32(gamma, dev), _f32(beta, dev)
    n, Cc = x.shape
    xin = x.clone()
    y = xin if inplace else torch.full_like(x, float("nan"))
    stats = torch.full((2, Cc), float("nan"), device=dev, dtype=torch.float32) if want_stats else None
    rm, rv = (None, None) if running is None else (_f32(running[0], dev).clone(), _f32(running[1], dev).clone())
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_bn_rows_relu(L.ptr(xin), n, Cc, L.ptr(g), L.ptr(b), float(eps), float(momentum), L.ptr(y), L.ptr(stats),
                                        L.ptr(rm), L.ptr(rv), _stream()))
    return y, stats, (None if running is None else (rm, rv))


def op_bn_rows_relu_bwd(xraw, dy, stats, gamma, beta, accum=None, poison=False, device=None, lib=None):
    """mvd_op_bn_rows_relu_bwd -> (d xraw [n,C], dgamma [C], dbeta [C]); accum = (dgamma0, dbeta0): what the gradients start from."""
    lib = lib or L.load()
    dev = xraw.device if device is None else device
    x, st, g, b = _f32(xraw, dev), _f32(stats, dev), _f32(gamma, dev), _f32(beta, dev)
    d = _f32(dy, dev).clone()
    n, Cc = x.shape
    dg, db = (torch.zeros_like(g), torch.zeros_like(g)) if accum is None else (_f32(accum[0], dev).clone(), _f32(accum[1], dev).clone())
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_bn_rows_relu_bwd(L.ptr(x), L.ptr(d), n, Cc, L.ptr(g), L.ptr(b), L.ptr(st), bool(poison), L.ptr(dg), L.ptr(db),
                                            _stream()))
    return d, dg, db


def _nan_guarded(rows, width, dev, dtype=torch.float32):
    """[rows + 1][width] of 0xFF bytes (NaN in fp32 and in both 16-bit types): a result buffer with one guard row behind it."""
    t = torch.empty(rows + 1, width, device=dev, dtype=dtype)
    t.view(torch.int32 if dtype == torch.float32 else torch.int16).fill_(-1)
    return t


def _guard_ok(t, rows, width=None, exact=True):
    """Everything behind row `rows` (and, with width, right of column `width`) is as a hook must leave it.  exact: still the 0xFF
    bytes the buffer was preset with.  Not exact: NaN -- for a result the hook converts from its own poisoned 16-bit image, guard
    included; such a buffer is preset to zero, so that a guard the hook did not write shows too."""
    if exact:
        t = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    held = (lambda x: x == -1) if exact else torch.isnan
    return bool(held(t[rows:]).all()) and (width is None or bool(held(t[:rows, width:]).all()))


def _nan_guard_intact(t, rows, what, width=None):
    if width is None:
        assert _guard_ok(t, rows), f"{what}: the launch wrote behind its result (guard row changed)"
    else:
        assert _guard_ok(t, rows, width), f"{what}: the launch wrote outside its result (guard row / pad columns changed)"


def op_train_depth_attn(q, k, v, HW, D, hn, device=None, lib=None):
    """mvd_op_train_depth_attn (depth_fwd_kernel): q [R,I], k / v [(R/HW)*D*HW, I] -> (attn [R,hn,D], z [R,I]).  Results start as NaN
    with a guard row behind them; a shape the launcher refuses raises MvdError with its text."""
    lib = lib or L.load()
    dev = q.device if device is None else device
    q, k, v = _f32(q, dev), _f32(k, dev), _f32(v, dev)
    R, I = q.shape
    if I % hn or R % HW or k.shape != (R // HW * D * HW, I) or v.shape != k.shape:
        raise ValueError("op_train_depth_attn: q [R,I], k and v [(R/HW)*D*HW, I] with I = hn * hd expected")
    attn, z = _nan_guarded(R, hn * D, dev), _nan_guarded(R, I, dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_train_depth_attn(L.ptr(q), L.ptr(k), L.ptr(v), R, HW, D, hn, I // hn, L.ptr(attn), L.ptr(z), _stream()))
    _nan_guard_intact(attn, R, "op_train_depth_attn (attn)")
    _nan_guard_intact(z, R, "op_train_depth_attn (z)")
    return attn[:R].reshape(R, hn, D).clone(), z[:R].clone()


def op_train_depth_attn_bwd(q, k, v, attn, dz, HW, D, hn, device=None, lib=None):
    """mvd_op_train_depth_attn_bwd (depth_bwd_kernel) -> (dq [R,I], dk, dv shaped like k); NaN presets and guard rows as above."""
    lib = lib or L.load()
    dev = q.device if device is None else device
    q, k, v, a, dz = _f32(q, dev), _f32(k, dev), _f32(v, dev), _f32(attn, dev), _f32(dz, dev)
    R, I = q.shape
    RC = R // HW * D * HW
    if I % hn or R % HW or k.shape != (RC, I) or v.shape != k.shape or a.numel() != R * hn * D or dz.shape != q.shape:
        raise ValueError("op_train_depth_attn_bwd: operands do not match q [R,I]")
    dq, dk, dv = _nan_guarded(R, I, dev), _nan_guarded(RC, I, dev), _nan_guarded(RC, I, dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_train_depth_attn_bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(a), L.ptr(dz), R, HW, D, hn, I // hn, L.ptr(dq),
                                                L.ptr(dk), L.ptr(dv), _stream()))
    for t, n, name in ((dq, R, "dq"), (dk, RC, "dk"), (dv, RC, "dv")):
        _nan_guard_intact(t, n, f"op_train_depth_attn_bwd ({name})")
    return dq[:R].clone(), dk[:RC].clone(), dv[:RC].clone()


def op_train_im2col3(x, device=None, lib=None):
    """mvd_op_train_im2col3: x [B,H,W,C] -> col [B*H*W, 9*C] (tap-major columns, zero outside the image)."""
    lib = lib or L.load()
    dev = x.device if device is None else device
    x = _f32(x, dev)
    B, H, W, Cc = x.shape
    col = _nan_guarded(B * H * W, 9 * Cc, dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_train_im2col3(L.ptr(x), B, H, W, Cc, L.ptr(col), _stream()))
    _nan_guard_intact(col, B * H * W, "op_train_im2col3")
    return col[:B * H * W].clone()


def op_train_col2im3(dcol, B, H, W, device=None, lib=None):
    """mvd_op_train_col2im3: dcol [B*H*W, 9*C] -> dx [B,H,W,C], the transpose of op_train_im2col3."""
    lib = lib or L.load()
    dev = dcol.device if device is None else device
    dcol = _f32(dcol, dev)
    if dcol.dim() != 2 or dcol.shape[0] != B * H * W or dcol.shape[1] % 9:
        raise ValueError("op_train_col2im3: dcol [B*H*W, 9*C] expected")
    Cc = dcol.shape[1] // 9
    dx = _nan_guarded(B * H * W, Cc, dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_train_col2im3(L.ptr(dcol), B, H, W, Cc, L.ptr(dx), _stream()))
    _nan_guard_intact(dx, B * H * W, "op_train_col2im3")
    return dx[:B * H * W].reshape(B, H, W, Cc).clone()


def op_train_perm_w3(src, N, Cc, to_mat, device=None, lib=None):
    """mvd_op_train_perm_w3: conv weight [N,C,3,3] -> GEMM matrix [N,9,C] (to_mat) or the reverse."""
    lib = lib or L.load()
    dev = src.device if device is None else device
    src = _f32(src, dev)
    if src.numel() != N * Cc * 9:
        raise ValueError("op_train_perm_w3: N * C * 9 elements expected")
    dst = _nan_guarded(N, 9 * Cc, dev)
    with torch.cuda.device(dev):
        L.check(lib.mvd_op_train_perm_w3(L.ptr(src), N, Cc, bool(to_mat), L.ptr(dst), _stream()))
    _nan_guard_intact(dst, N, "op_train_perm_w3")
    return dst[:N].reshape((N, 9, Cc) if to_mat else (N, Cc, 3, 3)).clone()


IncompatibleKeys = collections.namedtuple("IncompatibleKeys", ["missing_keys", "unexpected_keys"])
MAX_SAMPLE_SLOTS = 64  # per-sample mesh / camera tables kept resident in the context (mvd_select_sample)


def _level_dims(d, s):
    """(depth, size) of the four frustum levels: stride-2 convolutions with padding 1 (network.py:320-333), i.e. (x - 1) // 2 + 1
    per level -- the same rule csrc/engine_cond.hip uses (x >> level only agrees for multiples of 8)."""
    out = []
    for _ in range(4):
        out.append((d, s))
        d, s = (d - 1) // 2 + 1, (s - 1) // 2 + 1
    return out


class Engine:
    def __init__(self, ucfg: UNetConfig, vcfg: VolumeConfig, device="cuda:0", workspace_gb: float = 16.0,
                 precision_level: int = 3, train: bool = False, vae_exact: bool = False, deterministic: bool = False):
        """precision_level: mvd_set_precision_level (0..6): how many of the output-side layers run with split fp16 operands
        (extended precision); 3 is the default the parity bounds are stated for (include/mvd.h: the ladder).
        deterministic (needs train): mvd_train_set_deterministic, see ``train_set_deterministic``."""
        if deterministic and not train:
            raise ValueError("deterministic=True needs train=True: the mode selects kernels of the backward pass")
        self.deterministic = bool(deterministic)
        self.precision_level = int(precision_level)
        self.vae_exact = bool(vae_exact)  # mvd_set_vae_precision: first-stage model in extended precision (~3x its cost)
        self.train_mode = bool(train)  # mvd_train_enable: master parameters / gradients kept in flat arenas (training step)
        if not torch.cuda.is_available():
            raise L.MvdError("no MI355X visible: the denoiser has no CPU path")
        self.lib = L.load()
        ucfg.validate()
        vcfg.validate()
        self.ucfg, self.vcfg = ucfg, vcfg
        self.device = torch.device(device)
        self._workspace_gb = workspace_gb
        self._ctx = None
        self._loaded = False
        self._create()

    def _create(self):
        ucfg, vcfg, workspace_gb = self.ucfg, self.vcfg, self._workspace_gb
        uc = L.UNetConfigC()
        uc.image_size, uc.in_channels, uc.out_channels = ucfg.image_size, ucfg.in_channels, ucfg.out_channels
        uc.model_channels, uc.num_res_blocks = ucfg.model_channels, ucfg.num_res_blocks
        for i in range(4):
            uc.channel_mult[i] = ucfg.channel_mult[i]
            uc.volume_dims[i] = ucfg.volume_dims[i]
        uc.num_heads, uc.context_dim = ucfg.num_heads, ucfg.context_dim
        uc.attention_levels = sum(int(r) for r in ucfg.attention_resolutions)
        vc = L.VolumeConfigC()
        vc.time_dim, vc.view_dim, vc.num_views = vcfg.time_dim, vcfg.view_dim, vcfg.num_views
        vc.input_image_size, vc.frustum_volume_depth = vcfg.input_image_size, vcfg.frustum_volume_depth
        vc.spatial_volume_size = vcfg.spatial_volume_size
        vc.spatial_volume_length, vc.frustum_volume_length = vcfg.spatial_volume_length, vcfg.frustum_volume_length
        if vcfg.projection not in ("perspective", "orthographic"):
            raise NotImplementedError(vcfg.projection)  # utils.py:41,66
        vc.projection = 0 if vcfg.projection == "perspective" else 1
        for i in range(4):
            vc.frustum_dims[i] = vcfg.frustum_dims[i]
        vc.voxel_size = vcfg.voxel_size
        self._ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.mvd_create(C.byref(uc), C.byref(vc), self.device.index or 0,
                                        int(workspace_gb * (1 << 30)), C.byref(self._ctx)))
        L.check(self.lib.mvd_set_precision_level(self._ctx, self.precision_level))
        L.check(self.lib.mvd_set_spatial_volume(self._ctx, bool(vcfg.use_spatial_volume),
                                                (C.c_int * 4)(*vcfg.spatial_dims)))
        L.check(self.lib.mvd_train_enable(self._ctx, self.train_mode))
        if self.deterministic:  # (a context rebuilt by load_state_dict keeps the mode)
            L.check(self.lib.mvd_train_set_deterministic(self._ctx, True))
        L.check(self.lib.mvd_set_vae_precision(self._ctx, self.vae_exact))
        self._loaded = False
        self.flat_params = self.flat_grads = self.flat_m = self.flat_v = None
        self.param_table = {}
        self.lora_params = self.lora_grads = self.lora_m = self.lora_v = None  # lora_attach
        self.lora_table, self.lora_rank = {}, 0
        self.num_vertices = 0
        self._slot_nv = {}

    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.mvd_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False, expected=None):
        """Key-for-key upload of a reference state_dict (generate_face.py:75-76) and packing.  Like nn.Module it may be
        called again (another checkpoint, EMA weights): the context is rebuilt, so every call must carry the complete set.
        Returns (missing_keys, unexpected_keys) w.r.t. ``expected`` (default: the hot-path manifest); ``strict`` raises on
        either, as torch does.
        Keys outside the path (``num_batches_tracked``, schedule buffers, the CLIP text tower, ...) count as unexpected only
        under strict=True, exactly as they would for a module that does not declare them."""
        if self._loaded:  # packed weights are immutable: start from a fresh context
            self.close()
            self._create()
        if expected is None:  # the hot-path manifest; a stand-alone UNet passes its own (DepthWiseAttention.load_state_dict)
            from .spec import full_manifest
            expected = full_manifest(self.ucfg, self.vcfg)
        want = set(expected)
        have = {k for k, v in sd.items() if torch.is_tensor(v)}
        missing = sorted(want - have)
        side = ("first_stage_model.", "clip_image_encoder.", "model_ema.")  # (EMA shadows: SyncMultiviewDiffusion reads them)
        unexpected = sorted(k for k in have - want if not k.startswith(side))
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]} (+{max(0, len(missing) - 5)}), "
                               f"unexpected {unexpected[:5]} (+{max(0, len(unexpected) - 5)})")
        self.has_vae_decoder = any(k.startswith("first_stage_model.decoder.") for k in sd)
        self.has_vae_encoder = any(k.startswith("first_stage_model.encoder.") for k in sd)
        self.has_clip = any(k.startswith("clip_image_encoder.model.visual.") for k in sd)
        for k, v in sd.items():
            if not torch.is_tensor(v) or not v.dtype.is_floating_point or k.startswith("model_ema."):
                continue
            t = v.detach().to(dtype=torch.float32).contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            L.check(self.lib.mvd_upload_weight(self._ctx, k.encode(), L.ptr(t), shape, t.dim(), t.is_cuda))
        L.check(self.lib.mvd_finalize_weights(self._ctx))
        self._loaded = True
        if self.train_mode:
            self._adopt_arenas()
            # what a checkpoint written after training must carry besides the masters (export_state_dict): references to the
            # tensors the training step does not change (first stage, CLIP, schedule buffers, ...) -- no copies
            self._loaded_sd = {k: v for k, v in sd.items() if not k.startswith("model_ema.")}
        return IncompatibleKeys(missing, unexpected)

    def get_tensor(self, key):
        """Current value of a resident tensor of a training context (a master parameter or a BatchNorm running statistic)."""
        ref = self._loaded_sd[key]
        out = torch.empty(tuple(ref.shape), device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_train_get_tensor(self._ctx, key.encode(), L.ptr(out), out.numel(), _stream()))
        return out

    def train_bn_calls(self):
        """mvd_train_bn_calls: train-mode forwards of the sparse CNN so far (each moves its BatchNorm running statistics)."""
        return int(self.lib.mvd_train_bn_calls(self._ctx))

    def export_state_dict(self):
        """The loaded state_dict with every trained tensor replaced by its current value: master parameters from the arena, the
        sparse CNN's BatchNorm running statistics as the train-mode forwards left them (momentum 0.01, network.py:105),
        ``num_batches_tracked`` advanced by the number of those forwards.  Same keys, shapes and dtypes as what was loaded --
        the reference's ``torch.save({'state_dict': model.state_dict()})`` of a fine-tuned model."""
        if not self.train_mode or not self._loaded:
            raise L.MvdError("export_state_dict needs a training context with loaded weights")
        out = collections.OrderedDict()
        calls = self.lib.mvd_train_bn_calls(self._ctx)
        for k, v in self._loaded_sd.items():
            if not torch.is_tensor(v):
                out[k] = v
            elif k in self.param_table:
                out[k] = self.param_view(k).detach().clone().to(dtype=v.dtype)
            elif k.startswith("spatial_volume.") and k.endswith((".running_mean", ".running_var")):
                out[k] = self.get_tensor(k).to(dtype=v.dtype)
            elif k.startswith("spatial_volume.") and k.endswith(".num_batches_tracked"):
                out[k] = v.detach().clone() + calls
            else:
                out[k] = v
        return out

    # ---- stages --------------------------------------------------------------------------------
    def unet_forward(self, x, timesteps, context, source_dict, n_ctx: Optional[int] = None):
        """DepthWiseAttention.forward (attention.py:117-138). source_dict {res: [n_ctx,C,D,res,res]}."""
        dev = self.device
        Bv = x.shape[0]
        s = self.ucfg.image_size
        if context.dim() != 3 or context.shape[1] != 1:
            raise NotImplementedError("cross-attention context must be a single token [B,1,768] "
                                      "(morphable_diffusion.py:512)")
        x = _f32(x, dev)
        t = timesteps.to(device=dev, dtype=torch.int64).contiguous()
        ctx = _f32(context, dev)
        srcs = []
        for lvl in range(4):
            r = s >> lvl
            if r not in source_dict:
                raise KeyError(r)
            srcs.append(_f32(source_dict[r], dev))
        if n_ctx is None:
            n_ctx = srcs[0].shape[0]
        depth0 = srcs[0].shape[2]
        out = torch.empty(Bv, self.ucfg.out_channels, s, s, device=dev, dtype=torch.float32)
        L.check(self.lib.mvd_unet_forward(self._ctx, L.ptr(x), L.ptr(t), L.ptr(ctx), Bv, n_ctx, L.ptr(srcs[0]),
                                          L.ptr(srcs[1]), L.ptr(srcs[2]), L.ptr(srcs[3]), depth0, L.ptr(out), _stream()))
        return out

    def unet_block(self, path, x, timesteps=None, context=None, volume=None, n_ctx=None):
        """One block of DepthWiseAttention through the production block code: ``path`` is the reference module path below
        ``model.diffusion_model`` ("input_blocks.4.0", "output_blocks.8.2", "middle_conditions", "output_conditions.8", ...);
        ResBlocks take ``timesteps`` [B], SpatialTransformers ``context`` [B,1,768], DepthTransformers ``volume`` [n_ctx,C,D,H,W]:
        the context volumes of the FIRST ``n_ctx`` samples (default: as many as ``volume`` holds), the other samples are
        context-free (classifier-free guidance's unconditional half); ``n_ctx=0`` needs no volume."""
        dev = self.device
        x = _f32(x, dev)
        B, Cx, H, W = x.shape
        t = timesteps.to(device=dev, dtype=torch.int64).contiguous() if timesteps is not None else None
        ctx = _f32(context, dev) if context is not None else None
        vol = _f32(volume, dev) if volume is not None else None
        if n_ctx is None:
            n_ctx = vol.shape[0] if vol is not None else B
        if vol is not None and vol.shape[0] != n_ctx:
            raise ValueError(f"unet_block: volume holds {vol.shape[0]} samples, n_ctx is {n_ctx}")
        cap = B * H * W * 4 * self.ucfg.model_channels * 8
        out = torch.empty(cap, device=dev, dtype=torch.float32)
        shape = (C.c_int * 4)()
        L.check(self.lib.mvd_unet_block(self._ctx, path.encode(), L.ptr(x), B, Cx, H, W, L.ptr(t), L.ptr(ctx),
                                        L.ptr(vol) if n_ctx > 0 else None, vol.shape[2] if vol is not None else 0, n_ctx,
                                        L.ptr(out), cap, shape, _stream()))
        n = shape[0] * shape[1] * shape[2] * shape[3]
        return out[:n].view(shape[0], shape[1], shape[2], shape[3]).clone()

    def embed_time(self, t):
        t = t.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty(t.shape[0], self.vcfg.time_dim, device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_embed_time(self._ctx, L.ptr(t), t.shape[0], L.ptr(out), _stream()))
        return out

    def select_sample(self, slot: int):
        """Makes slot ``slot`` (0..MAX_SAMPLE_SLOTS-1) of per-sample mesh / camera tables the active one; set_mesh /
        set_cameras write into the active slot.  With B > 1 every sample keeps its tables across steps."""
        L.check(self.lib.mvd_select_sample(self._ctx, slot))
        self._slot = int(slot)
        self.num_vertices = self._slot_nv.get(self._slot, 0)

    def set_mesh(self, vertices, coord, out_sh, bounds):
        """Per-sample mesh metadata (hoists the .tolist() sync of morphable_diffusion.py:251-252).  Host tensors are read before
        the call returns; the tables reach the device in the order of the current stream (mvd_set_mesh_async), so a training
        step that sees a new mesh per sample neither allocates nor synchronises here."""
        v = vertices.detach().cpu().float().contiguous()
        c = coord.detach().cpu().to(torch.int32).contiguous()
        o = out_sh.detach().cpu().to(torch.int32).contiguous()
        b = bounds.detach().cpu().float().contiguous()
        L.check(self.lib.mvd_set_mesh_async(self._ctx, L.ptr(v), L.ptr(c), L.ptr(o), L.ptr(b), v.shape[0], _stream()))
        self.num_vertices = v.shape[0]
        self._slot_nv[getattr(self, "_slot", 0)] = v.shape[0]

    def set_samples(self, slots, vertices, coord, out_sh, bounds, K, RT):
        """mvd_set_samples_async: mesh + cameras of several samples (lists, one entry per sample) into the slots ``slots``; the
        rule books are built on one host thread per sample, the uploads are enqueued on the current stream."""
        n = len(slots)
        v = [t.detach().cpu().float().contiguous() for t in vertices]
        c = [t.detach().cpu().to(torch.int32).contiguous() for t in coord]
        o = [t.detach().cpu().to(torch.int32).contiguous() for t in out_sh]
        b = [t.detach().cpu().float().contiguous() for t in bounds]
        k = [t.detach().cpu().float().contiguous() for t in K]
        r = [t.detach().cpu().float().contiguous() for t in RT]
        if any(t.shape[-2:] != (4, 4) for t in k):
            raise ValueError("target_K must be [N,4,4] (morphable_diffusion.py:296)")
        if len({t.shape[0] for t in k}) != 1:
            raise ValueError("every sample of a batch has the same number of target views")
        arr = lambda ts, ty: (ty * n)(*[C.cast(L.ptr(t), ty) for t in ts])
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.check(self.lib.mvd_set_samples_async(self._ctx, n, (C.c_int * n)(*slots), arr(v, fp), arr(c, ip), arr(o, ip),
                                               arr(b, fp), (C.c_int * n)(*[t.shape[0] for t in v]), arr(k, fp), arr(r, fp),
                                               k[0].shape[0], _stream()))
        for sl, t in zip(slots, v):
            self._slot_nv[int(sl)] = t.shape[0]
        self.num_vertices = self._slot_nv.get(getattr(self, "_slot", 0), 0)

    def set_cameras(self, K, RT):
        K = K.detach().cpu().float().contiguous()
        RT = RT.detach().cpu().float().contiguous()
        if K.shape[-2:] != (4, 4):
            raise ValueError("target_K must be [N,4,4] (morphable_diffusion.py:296)")
        L.check(self.lib.mvd_set_cameras_async(self._ctx, L.ptr(K), L.ptr(RT), K.shape[0], _stream()))

    def vertex_features(self, x_noisy, t_embed, v_embed, view_idx, add_bias=True):
        dev = self.device
        x = _f32(x_noisy, dev)
        te, ve = _f32(t_embed, dev), _f32(v_embed, dev)
        vi = view_idx.to(device=dev, dtype=torch.int32).contiguous()
        out = torch.empty(self.num_vertices, 16, device=dev, dtype=torch.float32)
        L.check(self.lib.mvd_vertex_features(self._ctx, L.ptr(x), L.ptr(te), L.ptr(ve), L.ptr(vi), x.shape[0],
                                             bool(add_bias), L.ptr(out), _stream()))
        return out

    def vertex_view_features(self, x_noisy, t_embed, v_embed, view_idx, out=None):
        """Per-view vertex features [n_local,Nv,16] (no view reduction): the operand of the all-gather view exchange."""
        dev = self.device
        x = _f32(x_noisy, dev)
        te, ve = _f32(t_embed, dev), _f32(v_embed, dev)
        vi = view_idx.to(device=dev, dtype=torch.int32).contiguous()
        if out is None:
            out = torch.empty(x.shape[0], self.num_vertices, 16, device=dev, dtype=torch.float32)
        L.check(self.lib.mvd_vertex_view_features(self._ctx, L.ptr(x), L.ptr(te), L.ptr(ve), L.ptr(vi), x.shape[0],
                                                  L.ptr(out), _stream()))
        return out

    def vertex_features_stream_safe(self):
        """mvd_vertex_features_stream_safe: vertex_view_features may run on a side stream beside denoise_views of this engine."""
        return bool(self.lib.mvd_vertex_features_stream_safe(self._ctx))

    def fuse_vertex_features(self, vf_all, out=None):
        """SMPLFeatureExtractor over all views in index order: [num_views,Nv,16] -> [Nv,16]."""
        vf = _f32(vf_all, self.device)
        if out is None:
            out = torch.empty(self.num_vertices, 16, device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_fuse_vertex_features(self._ctx, L.ptr(vf), vf.shape[0], L.ptr(out), _stream()))
        return out

    # ---- the sharded step's exchange behind the C ABI (RCCL communicator owned by the library) ----------------------------
    def comm_init(self, rank=None, world=None):
        """Creates the library's RCCL communicator over the ranks of the default torch.distributed group (the 128-byte unique id
        is created on rank 0 and broadcast through that group -- any backend); world 1 needs no process group."""
        import torch.distributed as dist
        if world is None:
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if rank is None:  # derived independently of `world`: comm_init(world=W) alone must not leave rank 0 without the id
            rank = dist.get_rank() if (world > 1 and dist.is_available() and dist.is_initialized()) else 0
        ident = (C.c_char * 128)()
        if rank == 0:
            L.check(self.lib.mvd_comm_unique_id(C.byref(ident)))
        if world > 1:
            box = [bytes(ident)]
            dist.broadcast_object_list(box, src=0)
            ident = (C.c_char * 128).from_buffer_copy(box[0])
        L.check(self.lib.mvd_comm_init(self._ctx, C.byref(ident), rank, world))
        self.comm_world = world

    def comm_destroy(self):
        L.check(self.lib.mvd_comm_destroy(self._ctx))
        self.comm_world = 0

    def exchange_view_features(self, vf_local, vf_all):
        """ncclAllGather of this rank's [n_local,Nv,16] into vf_all [N,Nv,16] on the current stream (mvd_exchange_view_features)."""
        assert vf_local.is_contiguous() and vf_all.is_contiguous() and vf_local.dtype == vf_all.dtype == torch.float32
        L.check(self.lib.mvd_exchange_view_features(self._ctx, L.ptr(vf_local), L.ptr(vf_all), vf_local.shape[0], _stream()))
        return vf_all

    def comm_all_reduce(self, buf):
        """In-place sum all-reduce of a contiguous float32 device tensor on the library's communicator (mvd_comm_all_reduce)."""
        assert buf.is_contiguous() and buf.dtype == torch.float32
        L.check(self.lib.mvd_comm_all_reduce(self._ctx, L.ptr(buf), buf.numel(), _stream()))
        return buf

    def sync_gradients(self, phase, comm_stream):
        """mvd_train_sync_gradients: phase 0 = all buckets of the last train_unet_step on ``comm_stream`` (a torch.cuda.Stream),
        phase 1 = the rest of the arena, the join with the current stream and the 1 / world scale."""
        L.check(self.lib.mvd_train_sync_gradients(self._ctx, phase, comm_stream.cuda_stream, _stream()))

    def stage_target_encoder(self, x_noisy, t_embed, v_embed):
        """NoisyTargetViewEncoder alone (network.py:181-207): x_noisy [n,4,s,s], t_embed [time_dim], v_embed [n,view_dim] ->
        [n,16,s,s].  Parity probe."""
        dev = self.device
        x, te, ve = _f32(x_noisy, dev), _f32(t_embed, dev), _f32(v_embed, dev)
        out = torch.empty(x.shape[0], 16, x.shape[2], x.shape[3], device=dev, dtype=torch.float32)
        L.check(self.lib.mvd_stage_target_encoder(self._ctx, L.ptr(x), L.ptr(te), L.ptr(ve), x.shape[0], L.ptr(out), _stream()))
        return out

    def stage_sparse_dense(self, fused, train=False):
        """The sparse voxel CNN alone (network.py:74-96): fused [Nv,16] -> dense [C,d,h,w] of the coarsest level.  Parity probe."""
        shp = (C.c_int32 * 4)()
        L.check(self.lib.mvd_stage_sparse_dense(self._ctx, None, 0, None, shp, _stream()))
        f = _f32(fused, self.device)
        out = torch.empty(*[int(v) for v in shp], device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_stage_sparse_dense(self._ctx, L.ptr(f), bool(train), L.ptr(out), shp, _stream()))
        return out

    def stage_unproject(self, feats):
        """The dense multi-view unprojection alone (morphable_diffusion.py:197-225): encoder maps [N,16,s,s] of all views of the
        active sample -> [N*16,V,V,V], view-major as the reference stacks them.  Parity probe (use_spatial_volume=True)."""
        f = _f32(feats, self.device)
        V = self.vcfg.spatial_volume_size
        out = torch.empty(f.shape[0] * 16, V, V, V, device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_stage_unproject(self._ctx, L.ptr(f), f.shape[0], L.ptr(out), _stream()))
        return out

    def spatial_time_volume(self, x_noisy, t_embed, v_embed, want_output=True):
        """use_spatial_volume=True: encoder -> unprojection -> SpatialTime3DNet for all views of the active sample; the result
        is added into the volume the engine holds for that sample (call it after volume_from_fused, on the same stream).
        Returns the network's own output [64,V,V,V] (before the add) when ``want_output``."""
        dev = self.device
        x, te, ve = _f32(x_noisy, dev), _f32(t_embed, dev), _f32(v_embed, dev)
        V = self.vcfg.spatial_volume_size
        out = torch.empty(64, V, V, V, device=dev, dtype=torch.float32) if want_output else None
        L.check(self.lib.mvd_spatial_time_volume(self._ctx, L.ptr(x), L.ptr(te), L.ptr(ve), x.shape[0], L.ptr(out), _stream()))
        return out

    def set_volume_ready_event(self, event):
        """event: torch.cuda.Event recorded after volume_from_fused on another stream (kept alive by the caller), or None."""
        L.check(self.lib.mvd_set_volume_ready_event(self._ctx, None if event is None else event.cuda_event))

    def volume_from_fused(self, fused, want_output=True, train=False):
        """train: BatchNorm layers of the sparse CNN use batch statistics (the reference's module in train mode)."""
        V = self.vcfg.spatial_volume_size
        out = torch.empty(64, V, V, V, device=self.device, dtype=torch.float32) if want_output else None
        f = _f32(fused, self.device)
        fn = self.lib.mvd_volume_from_fused_train if train else self.lib.mvd_volume_from_fused
        L.check(fn(self._ctx, L.ptr(f), L.ptr(out), _stream()))
        return out

    # ---- training -----------------------------------------------------------------
    def _adopt_arenas(self):
        """The engine's master-parameter and gradient arenas move into torch-owned memory, so that parameters / gradients are
        VIEWS of two flat tensors (one collective for the DDP gradient averaging, torch optimisers work on them too)."""
        n = self.lib.mvd_train_arena_size(self._ctx)
        self.flat_params = torch.empty(n, device=self.device, dtype=torch.float32)
        self.flat_grads = torch.empty(n, device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_train_adopt_arena(self._ctx, 0, L.ptr(self.flat_params), n))
        L.check(self.lib.mvd_train_adopt_arena(self._ctx, 1, L.ptr(self.flat_grads), n))
        self.flat_m = self.flat_v = self.flat_ema = None
        self.last_grad_norm = None
        self.param_table = {}
        name = C.create_string_buffer(512)
        off, numel, nd = C.c_int64(0), C.c_int64(0), C.c_int(0)
        shape = (C.c_int64 * 8)()
        for i in range(self.lib.mvd_train_param_count(self._ctx)):
            L.check(self.lib.mvd_train_param_info(self._ctx, i, name, len(name), C.byref(off), C.byref(numel), shape,
                                                  C.byref(nd)))
            self.param_table[name.value.decode()] = (off.value, numel.value, tuple(int(shape[k]) for k in range(nd.value)))

    def param_view(self, key, grad=False):
        """View of one master parameter (or its gradient) inside the flat arena, in the reference's layout."""
        off, numel, shape = self.param_table[key]
        return (self.flat_grads if grad else self.flat_params)[off:off + numel].view(shape)

    def zero_grad(self):
        L.check(self.lib.mvd_train_zero_grad(self._ctx, _stream()))

    def train_unet_step(self, x, timesteps, context, source_dict, target, loss_scale=1.0, recompute=False, want_dsrc=False,
                        sample_weight=None, pixel_weight=None, loss_type="l2", huber_delta=1.0, per_sample=False):
        """mvd_train_unet_step: forward + MSE loss + backward through every UNet block.  Returns (pred, loss[, dsrc dict]);
        parameter gradients (x loss_scale) are accumulated into ``flat_grads``.
        sample_weight [B] / pixel_weight [B,1,s,s] / loss_type "l2" | "huber" (with huber_delta) / per_sample: any of them set
        runs mvd_train_unet_step_ex, the step with the weighted / masked / Huber loss stage (include/mvd.h); per_sample appends
        (loss_per_sample [B], mse_per_sample [B]) to the result.  With the defaults the call is mvd_train_unet_step as before."""
        if not self.train_mode:
            raise L.MvdError("the engine was not created with train=True")
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type must be one of {LOSS_TYPES}, not {loss_type!r}")
        dev = self.device
        B = x.shape[0]
        s = self.ucfg.image_size
        x = _f32(x, dev)
        t = timesteps.to(device=dev, dtype=torch.int64).contiguous()
        ctx = _f32(context, dev)
        tgt = _f32(target, dev)
        srcs = [_f32(source_dict[s >> lvl], dev) for lvl in range(4)]
        depth0 = srcs[0].shape[2]
        pred = torch.empty(B, self.ucfg.out_channels, s, s, device=dev, dtype=torch.float32)
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        dsrc = [torch.empty_like(v) for v in srcs] if want_dsrc else [None] * 4
        ex = sample_weight is not None or pixel_weight is not None or loss_type != "l2" or per_sample
        extra = ()
        if not ex:
            L.check(self.lib.mvd_train_unet_step(self._ctx, L.ptr(x), L.ptr(t), L.ptr(ctx), B, L.ptr(srcs[0]), L.ptr(srcs[1]),
                                                 L.ptr(srcs[2]), L.ptr(srcs[3]), depth0, L.ptr(tgt), loss_scale,
                                                 bool(recompute), L.ptr(pred), L.ptr(loss), L.ptr(dsrc[0]), L.ptr(dsrc[1]),
                                                 L.ptr(dsrc[2]), L.ptr(dsrc[3]), _stream()))
        else:
            w = None if sample_weight is None else _f32(sample_weight, dev).reshape(-1)
            m = None if pixel_weight is None else _f32(pixel_weight, dev)
            if w is not None and w.numel() != B:
                raise ValueError(f"sample_weight must have {B} elements, got {tuple(sample_weight.shape)}")
            if m is not None and tuple(m.shape) not in ((B, 1, s, s), (B, s, s)):
                raise ValueError(f"pixel_weight must be [{B},1,{s},{s}], got {tuple(pixel_weight.shape)}")
            lps = torch.empty(B, device=dev, dtype=torch.float32) if per_sample else None
            mps = torch.empty(B, device=dev, dtype=torch.float32) if per_sample else None
            L.check(self.lib.mvd_train_unet_step_ex(self._ctx, L.ptr(x), L.ptr(t), L.ptr(ctx), B, L.ptr(srcs[0]), L.ptr(srcs[1]),
                                                    L.ptr(srcs[2]), L.ptr(srcs[3]), depth0, L.ptr(tgt), loss_scale,
                                                    bool(recompute), L.ptr(w), L.ptr(m), LOSS_TYPES.index(loss_type),
                                                    float(huber_delta), L.ptr(pred), L.ptr(loss), L.ptr(lps), L.ptr(mps),
                                                    L.ptr(dsrc[0]), L.ptr(dsrc[1]), L.ptr(dsrc[2]), L.ptr(dsrc[3]), _stream()))
            if per_sample:
                extra = (lps, mps)
        if want_dsrc:
            return (pred, loss[0], {s >> lvl: dsrc[lvl] for lvl in range(4)}) + extra
        return (pred, loss[0]) + extra

    def op_train_loss(self, pred, target, sample_weight=None, pixel_weight=None, loss_type="l2", huber_delta=1.0, loss_scale=1.0,
                      want_grad=False):
        """mvd_op_train_loss: the loss stage of mvd_train_unet_step_ex alone, on channels-last buffers -- pred / target [B,HW,C],
        sample_weight [B], pixel_weight [B,HW].  Returns (L, loss_per_sample [B], mse_per_sample [B][, dpred [B,HW,C]]); without
        ``want_grad`` nothing but the loss is computed (the held-out loss of ``validation_loss``).  Needs no training context."""
        return op_train_loss(pred, target, sample_weight, pixel_weight, loss_type, huber_delta, loss_scale, want_grad,
                             device=self.device, lib=self.lib)

    def op_image_metrics(self, pred, target, mask=None, mask_mode=None):
        """mvd_op_image_metrics on this engine's device: see the module-level op_image_metrics."""
        return op_image_metrics(pred, target, mask, mask_mode, device=self.device, lib=self.lib)

    def op_mesh_project(self, verts, K, RT, z_near):
        """mvd_op_mesh_project on this engine's device: see the module-level op_mesh_project."""
        return op_mesh_project(verts, K, RT, z_near, device=self.device, lib=self.lib)

    def op_mesh_raster(self, xy, key, faces, H, W):
        """mvd_op_mesh_raster on this engine's device: see the module-level op_mesh_raster."""
        return op_mesh_raster(xy, key, faces, H, W, device=self.device, lib=self.lib)

    def op_mesh_vertex_colors(self, images, xy, key, faces, face_id, pix_key, verts, normals, centres, **kw):
        """mvd_op_mesh_vertex_colors on this engine's device: see the module-level op_mesh_vertex_colors."""
        return op_mesh_vertex_colors(images, xy, key, faces, face_id, pix_key, verts, normals, centres, device=self.device,
                                     lib=self.lib, **kw)

    def op_mesh_vertex_normals(self, verts, faces, inc_ptr, inc_face):
        """mvd_op_mesh_vertex_normals on this engine's device: see the module-level op_mesh_vertex_normals."""
        return op_mesh_vertex_normals(verts, faces, inc_ptr, inc_face, device=self.device, lib=self.lib)

    def op_mesh_texel_bake(self, images, face_id, pix_key, K, RT, centres, z_near, verts, normals, faces, uv_xy, face_uv, tex_face, **kw):
        """mvd_op_mesh_texel_bake on this engine's device: see the module-level op_mesh_texel_bake."""
        return op_mesh_texel_bake(images, face_id, pix_key, K, RT, centres, z_near, verts, normals, faces, uv_xy, face_uv, tex_face,
                                  device=self.device, lib=self.lib, **kw)

    def op_mesh_texture_dilate(self, texture, valid, passes):
        """mvd_op_mesh_texture_dilate on this engine's device: see the module-level op_mesh_texture_dilate."""
        return op_mesh_texture_dilate(texture, valid, passes, device=self.device, lib=self.lib)

    def op_mesh_render_uv(self, xy, key, face_id, faces, face_uv, uv, texture, **kw):
        """mvd_op_mesh_render_uv on this engine's device: see the module-level op_mesh_render_uv."""
        return op_mesh_render_uv(xy, key, face_id, faces, face_uv, uv, texture, device=self.device, lib=self.lib, **kw)

    def op_mesh_closest_point(self, queries, verts, faces, **kw):
        """mvd_op_mesh_closest_point on this engine's device: see the module-level op_mesh_closest_point."""
        return op_mesh_closest_point(queries, verts, faces, device=self.device, lib=self.lib, **kw)

    # the sparse voxel CNN's kernels one at a time: the module-level functions above on this engine's device and library
    def op_sparse_conv(self, x, nbr, w, layout, form="mfma", scale=None, shift=None):
        return op_sparse_conv(x, nbr, w, layout, form, scale, shift, device=self.device, lib=self.lib)

    def op_sparse_conv_bwd(self, x, nbr, d_out, w, layout, form="mfma", strided=False, level0_subm=False, deterministic=False,
                           grad_w=None, poison=False):
        return op_sparse_conv_bwd(x, nbr, d_out, w, layout, form, strided, level0_subm, deterministic, grad_w, poison,
                                  device=self.device, lib=self.lib)

    def op_bn_rows_relu(self, x, gamma, beta, eps=1e-3, running=None, momentum=0.01, inplace=False, want_stats=True):
        return op_bn_rows_relu(x, gamma, beta, eps, running, momentum, inplace, want_stats, device=self.device, lib=self.lib)

    def op_bn_rows_relu_bwd(self, xraw, dy, stats, gamma, beta, accum=None, poison=False):
        return op_bn_rows_relu_bwd(xraw, dy, stats, gamma, beta, accum, poison, device=self.device, lib=self.lib)

    def train_cond_backward(self, cond_index, x, context, d_out):
        """mvd_train_cond_backward (parity hook): one DepthTransformer's backward from exact inputs -> (dx, dcontext)."""
        dev = self.device
        x, context, d_out = _f32(x, dev), _f32(context, dev), _f32(d_out, dev)
        B, _, H, W = x.shape
        depth0 = context.shape[2] * (self.ucfg.image_size // H)
        dx, dc = torch.empty_like(x), torch.empty_like(context)
        L.check(self.lib.mvd_train_cond_backward(self._ctx, cond_index, L.ptr(x), L.ptr(context), L.ptr(d_out), B, H, W, depth0,
                                                 L.ptr(dx), L.ptr(dc), _stream()))
        return dx, dc

    def train_conditioner_backward(self, x_noisy, timestep, v_embed, target_index, dsrc, debug=False):
        """mvd_train_conditioner_backward for the ACTIVE sample: x_noisy [N,4,s,s], v_embed [N,4], dsrc {res: [1,C,D,res,res]}
        (loss-scaled).  Accumulates the gradients of spatial_volume.* / time_embed.*; debug=True also returns the intermediate
        gradients (d volume, d fused, d encoder features, d step embedding)."""
        dev = self.device
        x, ve = _f32(x_noisy, dev), _f32(v_embed, dev)
        s = self.vcfg.input_image_size // 8
        ds = [_f32(dsrc[s >> lvl], dev) for lvl in range(4)]
        dbg = [None] * 4
        if debug:
            V = self.vcfg.spatial_volume_size
            dbg = [torch.empty(64, V, V, V, device=dev), torch.empty(self.num_vertices, 16, device=dev),
                   torch.empty(x.shape[0], 16, x.shape[2], x.shape[3], device=dev), torch.empty(self.vcfg.time_dim, device=dev)]
        L.check(self.lib.mvd_train_conditioner_backward(self._ctx, L.ptr(x), timestep, L.ptr(ve), x.shape[0],
                                                        target_index, L.ptr(ds[0]), L.ptr(ds[1]), L.ptr(ds[2]), L.ptr(ds[3]),
                                                        L.ptr(dbg[0]), L.ptr(dbg[1]), L.ptr(dbg[2]), L.ptr(dbg[3]), _stream()))
        return dbg if debug else None

    def train_conditioner_backward_batch(self, slots, x_noisy, timesteps, v_embed, target_index, dsrc):
        """mvd_train_conditioner_backward_batch: the conditioner's backward for the samples resident in ``slots`` -- x_noisy
        [B,N,4,s,s], timesteps / target_index host ints [B], v_embed [B,N,4], dsrc {res: [B,C,D,res,res]} (loss-scaled).  The frustum
        network runs once with the samples as its batch; everything mesh-specific per sample."""
        dev = self.device
        x, ve = _f32(x_noisy, dev), _f32(v_embed, dev)
        B = x.shape[0]
        s = self.vcfg.input_image_size // 8
        ds = [_f32(dsrc[s >> lvl], dev) for lvl in range(4)]
        assert len(slots) == B == len(timesteps) == len(target_index) and all(d.shape[0] == B for d in ds)
        L.check(self.lib.mvd_train_conditioner_backward_batch(
            self._ctx, B, (C.c_int * B)(*slots), L.ptr(x), (C.c_int64 * B)(*timesteps), L.ptr(ve),
            x.shape[1], (C.c_int * B)(*target_index), L.ptr(ds[0]), L.ptr(ds[1]), L.ptr(ds[2]), L.ptr(ds[3]),
            None, None, None, None, _stream()))

    def train_set_deterministic(self, on=True):
        """mvd_train_set_deterministic: from the next backward call on, the conditioner's three gather adjoints (frustum, lattice,
        vertex) and the fold of duplicate vertices' rows run as gathers with index-ordered sums instead of fp32 atomic scatters:
        identical inputs then give bit-identical gradients over the whole arena.  Off (the default) restores the atomic forms."""
        L.check(self.lib.mvd_train_set_deterministic(self._ctx, bool(on)))
        self.deterministic = bool(on)

    def adjoint_calls(self):
        """mvd_probe_adjoint_calls: launches so far of the (frustum, latent, vertex) adjoints as {"atomic": (..), "gather": (..)}."""
        n = (C.c_int64 * 6)()
        L.check(self.lib.mvd_probe_adjoint_calls(self._ctx, n))
        return {"atomic": tuple(int(v) for v in n[:3]), "gather": tuple(int(v) for v in n[3:])}

    def _view_idx(self, view_idx, n):
        idx = list(range(n)) if view_idx is None else [int(v) for v in view_idx]
        return (C.c_int32 * len(idx))(*idx), len(idx)

    def op_frustum_adjoint(self, d_out, view_idx=None, deterministic=False):
        """mvd_op_frustum_adjoint: the adjoint of the frustum gather alone.  d_out [TN,D,S,S,64] (channels-last) = dL/d(gathered
        frustum) of the views ``view_idx`` (default 0..TN-1) of the active sample -> dL/d(volume) [V,V,V,64]."""
        g = _f32(d_out, self.device)
        TN, D, S = g.shape[0], g.shape[1], g.shape[2]
        assert g.dim() == 5 and g.shape[3] == S and g.shape[4] == 64
        idx, n = self._view_idx(view_idx, TN)
        assert n == TN
        V = self.vcfg.spatial_volume_size
        out = torch.full((V, V, V, 64), float("nan"), device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_op_frustum_adjoint(self._ctx, L.ptr(g), idx, TN, D, S, bool(deterministic), L.ptr(out), _stream()))
        return out

    def op_latent_adjoint(self, d_vol, deterministic=False):
        """mvd_op_latent_adjoint: the adjoint of the lattice gather alone.  d_vol [V,V,V,64] (channels-last) -> the gradient of the
        coarsest sparse level's rows [n_rows,64] of the active sample's mesh."""
        g = _f32(d_vol, self.device)
        V = self.vcfg.spatial_volume_size
        assert tuple(g.shape) == (V, V, V, 64)
        n = C.c_int32(0)
        L.check(self.lib.mvd_op_latent_adjoint(self._ctx, None, 0, None, C.byref(n), _stream()))
        out = torch.full((n.value, 64), float("nan"), device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_op_latent_adjoint(self._ctx, L.ptr(g), bool(deterministic), L.ptr(out), None, _stream()))
        return out

    def op_vertex_adjoint(self, d_vf, view_idx=None, deterministic=False):
        """mvd_op_vertex_adjoint: the adjoint of the vertex gather alone.  d_vf [n,Nv,16] = dL/d(per-view vertex features) of the
        views ``view_idx`` (default 0..n-1) of the active sample -> dL/d(2-D encoder maps) [n,s,s,16] (channels-last)."""
        g = _f32(d_vf, self.device)
        assert g.dim() == 3 and g.shape[1] == self.num_vertices and g.shape[2] == 16
        idx, n = self._view_idx(view_idx, g.shape[0])
        assert n == g.shape[0]
        s = self.ucfg.image_size
        out = torch.full((n, s, s, 16), float("nan"), device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_op_vertex_adjoint(self._ctx, L.ptr(g), idx, n, bool(deterministic), L.ptr(out), _stream()))
        return out

    def op_vertex_gather(self, feats, view_idx=None):
        """mvd_op_vertex_gather: the vertex gather alone.  feats [n,s,s,16] (channels-last 2-D encoder maps) of the views
        ``view_idx`` (default 0..n-1) of the active sample -> per-view vertex features [n,Nv,16]."""
        f = _f32(feats, self.device)
        s = self.ucfg.image_size
        assert f.dim() == 4 and tuple(f.shape[1:]) == (s, s, 16)
        idx, n = self._view_idx(view_idx, f.shape[0])
        assert n == f.shape[0]
        out = torch.full((n, self.num_vertices, 16), float("nan"), device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_op_vertex_gather(self._ctx, L.ptr(f), idx, n, L.ptr(out), _stream()))
        return out

    def op_latent_gather(self, rows):
        """mvd_op_latent_gather: the lattice gather alone.  rows [n_rows,64] of the coarsest sparse level of the active sample's
        mesh -> the mesh volume [V,V,V,64] (channels-last)."""
        r = _f32(rows, self.device)
        n = C.c_int32(0)
        L.check(self.lib.mvd_op_latent_adjoint(self._ctx, None, 0, None, C.byref(n), _stream()))
        assert tuple(r.shape) == (n.value, 64)
        V = self.vcfg.spatial_volume_size
        out = torch.full((V, V, V, 64), float("nan"), device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_op_latent_gather(self._ctx, L.ptr(r), L.ptr(out), _stream()))
        return out

    def op_frustum_gather(self, vol, view_idx, D, S):
        """mvd_op_frustum_gather: the frustum gather alone.  vol [V,V,V,64] (channels-last) -> the D x S x S frusta of the views
        ``view_idx`` of the active sample [TN,D,S,S,64], the operand-type values widened to fp32."""
        v = _f32(vol, self.device)
        V = self.vcfg.spatial_volume_size
        assert tuple(v.shape) == (V, V, V, 64)
        idx, TN = self._view_idx(view_idx, 0)
        out = torch.full((TN, D, S, S, 64), float("nan"), device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_op_frustum_gather(self._ctx, L.ptr(v), idx, TN, D, S, L.ptr(out), _stream()))
        return out

    def get_grad(self, key: str, shape):
        out = torch.empty(tuple(shape), device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_train_get_grad(self._ctx, key.encode(), L.ptr(out), out.numel(), _stream()))
        return out

    def grad_buckets(self):
        """Gradient buckets of the last train_unet_step (mvd_train_grad_bucket*): a list, in the order the gradients become final
        during the backward pass, of lists of (offset, length) ranges of ``flat_grads``; together model.diffusion_model.* once."""
        out = []
        for k in range(self.lib.mvd_train_grad_bucket_count(self._ctx)):
            n = C.c_int(0)
            L.check(self.lib.mvd_train_grad_bucket(self._ctx, k, 0, None, None, C.byref(n)))
            offs, lens = (C.c_int64 * max(1, n.value))(), (C.c_int64 * max(1, n.value))()
            L.check(self.lib.mvd_train_grad_bucket(self._ctx, k, n.value, offs, lens, C.byref(n)))
            out.append([(int(offs[i]), int(lens[i])) for i in range(n.value)])
        return out

    def grad_bucket_wait(self, k, stream):
        """Makes ``stream`` (a torch.cuda.Stream: the communication stream) wait until bucket k's gradients are final."""
        L.check(self.lib.mvd_train_grad_bucket_wait(self._ctx, k, stream.cuda_stream))

    def set_bucket_snapshot(self, arena):
        """Test hook (mvd_train_set_bucket_snapshot): ``arena`` = a float32 device tensor shaped like ``flat_grads``, or None."""
        L.check(self.lib.mvd_train_set_bucket_snapshot(self._ctx, L.ptr(arena)))
        self._bucket_snapshot = arena  # keep it alive while the engine writes to it

    def adamw_step(self, lr, lr_aux, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, inv_scale=1.0, finetune_unet=True,
                   check=True, max_grad_norm=None, ema_decay=None):
        """torch.optim.AdamW on the arena (two learning-rate groups, morphable_diffusion.py:627-646) + in-place re-pack of the
        fp16 weights.  Returns True when the update was skipped because a gradient was inf / nan (check=False: not read back).
        max_grad_norm: clip the gradients to that global norm first (clip_grad_norm_); ``last_grad_norm`` then holds the norm as
        a device scalar (no synchronisation).  ema_decay: this step's decay of the EMA weights in ``flat_ema``.  With either set
        the step is mvd_train_adamw_step_ex (norm pass + one fused kernel), otherwise mvd_train_adamw_step as before."""
        self.ensure_moments()
        skipped = C.c_int(0)
        sk = C.byref(skipped) if check else None
        if max_grad_norm is None and ema_decay is None:
            L.check(self.lib.mvd_train_adamw_step(self._ctx, lr, lr_aux, betas[0], betas[1], eps, weight_decay, step, inv_scale,
                                                  bool(finetune_unet), sk, _stream()))
        else:
            if ema_decay is not None:
                self.ensure_ema()
            clip = float(max_grad_norm) if max_grad_norm is not None else 0.0
            L.check(self.lib.mvd_train_adamw_step_ex(self._ctx, lr, lr_aux, betas[0], betas[1], eps, weight_decay, step, inv_scale,
                                                     bool(finetune_unet), sk, clip, -1.0 if ema_decay is None else float(ema_decay),
                                                     None, _stream()))
            if clip > 0.0:
                norm = torch.empty(1, device=self.device, dtype=torch.float32)
                L.check(self.lib.mvd_train_last_grad_norm(self._ctx, L.ptr(norm), _stream()))
                self.last_grad_norm = norm[0]
        self.repack()
        return bool(skipped.value)

    def grad_norm(self, inv_scale=1.0, finetune_unet=True):
        """Global norm of the (un-scaled) gradients the optimiser step would use, as a device scalar: mvd_train_grad_norm, the
        deterministic two-stage reduction over the step's arena ranges."""
        out = torch.empty(1, device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_train_grad_norm(self._ctx, inv_scale, bool(finetune_unet), L.ptr(out), _stream()))
        return out[0]

    def ensure_ema(self):
        """The EMA arena ``flat_ema`` (LitEma's shadow parameters): created as a copy of the parameters, adopted by the library."""
        if self.flat_ema is None:
            self.flat_ema = torch.empty_like(self.flat_params)
            L.check(self.lib.mvd_train_adopt_arena(self._ctx, 4, L.ptr(self.flat_ema), self.flat_ema.numel()))
        return self.flat_ema

    def ema_swap(self):
        """Exchange ``flat_params`` and ``flat_ema`` in place (mvd_train_ema_swap); the caller re-packs (``repack``)."""
        if self.flat_ema is None:
            raise L.MvdError("ema_swap: no EMA arena (ensure_ema)")
        L.check(self.lib.mvd_train_ema_swap(self._ctx, _stream()))

    def ensure_moments(self):
        """The two Adam moment arenas (zero until the first update), adopted by the library like the master / gradient arenas."""
        if self.flat_m is None:
            self.flat_m = torch.zeros_like(self.flat_params)
            self.flat_v = torch.zeros_like(self.flat_params)
            n = self.flat_params.numel()
            L.check(self.lib.mvd_train_adopt_arena(self._ctx, 2, L.ptr(self.flat_m), n))
            L.check(self.lib.mvd_train_adopt_arena(self._ctx, 3, L.ptr(self.flat_v), n))

    def repack(self):
        """Re-derive every packed fp16 weight from the master parameters (after they changed), in place, in the order of the
        current stream (mvd_train_repack_async: behind the optimiser update enqueued on it, ahead of the next forward)."""
        if os.environ.get("MVD_REPACK_SYNC") == "1":  # A/B switch: the device-synchronising form
            L.check(self.lib.mvd_train_repack(self._ctx))
        else:
            L.check(self.lib.mvd_train_repack_async(self._ctx, _stream()))

    # ---- LoRA (mvd_lora_*) ---------------------------------------------------------------------------------------------
    def lora_attach(self, keys, rank, alpha):
        """Low-rank adapters W0 + (alpha / rank) B A on the parameters ``keys`` (each of shape (out, in[, 1...])): the library
        snapshots W0 and creates four adapter arenas, adopted here as ``lora_params`` / ``lora_grads`` / ``lora_m`` / ``lora_v``
        (flat fp32 device tensors, zero: the masters do not change until B does).  ``lora_table[key]`` = (offset of A, offset of
        B, out, in); ``lora_view`` gives the tensors."""
        if not self.train_mode or not self._loaded:
            raise L.MvdError("lora_attach needs a training context with loaded weights")
        keys = list(keys)
        was_attached = bool(self.lora_rank)
        arr = (C.c_char_p * max(1, len(keys)))(*[k.encode() for k in keys])
        L.check(self.lib.mvd_lora_attach(self._ctx, arr, len(keys), int(rank), float(alpha)))
        numel = C.c_int64(0)
        L.check(self.lib.mvd_lora_arena_size(self._ctx, C.byref(numel)))
        n = numel.value
        flats = [torch.empty(n, device=self.device, dtype=torch.float32) for _ in range(4)]
        for which, t in enumerate(flats):
            L.check(self.lib.mvd_lora_adopt_arena(self._ctx, which, L.ptr(t), n))
        self.lora_params, self.lora_grads, self.lora_m, self.lora_v = flats
        self.lora_rank, self.lora_alpha, self.lora_scale = int(rank), float(alpha), float(alpha) / int(rank)
        self.lora_table = {}
        name = C.create_string_buffer(512)
        a, b, o, i = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        for t in range(self.lib.mvd_lora_target_count(self._ctx)):
            L.check(self.lib.mvd_lora_info(self._ctx, t, name, len(name), C.byref(a), C.byref(b), C.byref(o), C.byref(i)))
            self.lora_table[name.value.decode()] = (a.value, b.value, o.value, i.value)
        if was_attached:  # the library put W0 back into the masters before it took the new snapshot
            self.repack()

    def lora_detach(self, keep_merged=False):
        """Frees the adapters; keep_merged=False puts W0 back into the masters first.  Re-packs."""
        L.check(self.lib.mvd_lora_detach(self._ctx, bool(keep_merged)))
        self.lora_params = self.lora_grads = self.lora_m = self.lora_v = None
        self.lora_table, self.lora_rank = {}, 0
        self.repack()

    def lora_view(self, key, which, grad=False):
        """A ([rank, in]) or B ([out, rank]) of one target -- or its gradient -- as a view of the flat adapter arena."""
        a, b, out, in_ = self.lora_table[key]
        flat = self.lora_grads if grad else self.lora_params
        if which == "A":
            return flat[a:a + self.lora_rank * in_].view(self.lora_rank, in_)
        return flat[b:b + out * self.lora_rank].view(out, self.lora_rank)

    def lora_project(self):
        """mvd_lora_project: ``lora_grads`` = the projection of the dense gradients in ``flat_grads`` (what lora_step starts with)."""
        L.check(self.lib.mvd_lora_project(self._ctx, _stream()))

    def lora_set_scale(self, scale):
        """Merge W0 + scale B A into the masters (0: W0 again) and re-pack; the adapters are not touched."""
        L.check(self.lib.mvd_lora_set_scale(self._ctx, float(scale), _stream()))
        self.lora_scale = float(scale)
        self.repack()

    def lora_step(self, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, inv_scale=1.0, check=True, max_grad_norm=None):
        """mvd_lora_step (project the dense gradients onto the adapters, norm pass, fused AdamW on the adapter arenas, merge) +
        re-pack.  Returns True when the update was skipped for a non-finite gradient; with max_grad_norm ``last_grad_norm`` holds
        the norm of the un-scaled adapter gradients as a device scalar."""
        skipped = C.c_int(0)
        clip = float(max_grad_norm) if max_grad_norm is not None else 0.0
        L.check(self.lib.mvd_lora_step(self._ctx, lr, betas[0], betas[1], eps, weight_decay, step, inv_scale, clip,
                                       C.byref(skipped) if check else None, None, _stream()))
        if clip > 0.0:
            norm = torch.empty(1, device=self.device, dtype=torch.float32)
            L.check(self.lib.mvd_train_last_grad_norm(self._ctx, L.ptr(norm), _stream()))
            self.last_grad_norm = norm[0]
        self.repack()
        return bool(skipped.value)

    def set_volume(self, volume):
        v = _f32(volume, self.device)
        L.check(self.lib.mvd_set_volume(self._ctx, L.ptr(v), _stream()))

    def mse_loss(self, a, b):
        a, b = _f32(a, self.device), _f32(b, self.device)
        out = torch.empty(1, device=self.device, dtype=torch.float32)
        L.check(self.lib.mvd_mse_loss(self._ctx, L.ptr(a), L.ptr(b), a.numel(), L.ptr(out), _stream()))
        return out[0]

    def frustum_volumes_batch(self, slots, volumes, t_embed, v_rows, view_idx):
        """mvd_frustum_volumes_batch: one target view per sample -- volumes [B,64,V,V,V], t_embed [B,time_dim], v_rows [B,view_dim],
        view_idx [B]; the samples' cameras are resident in ``slots``.  Returns {res: [B,C,D,res,res]}."""
        dev = self.device
        vol, te, vr = _f32(volumes, dev), _f32(t_embed, dev), _f32(v_rows, dev)
        vi = view_idx.to(device=dev, dtype=torch.int32).contiguous()
        B = vol.shape[0]
        outs, ptrs = {}, []
        for lvl, (Dl, Sl) in enumerate(_level_dims(self.vcfg.frustum_volume_depth, self.vcfg.frustum_volume_size)):
            o = torch.empty(B, self.vcfg.frustum_dims[lvl], Dl, Sl, Sl, device=dev, dtype=torch.float32)
            outs[Sl] = o
            ptrs.append(L.ptr(o))
        L.check(self.lib.mvd_frustum_volumes_batch(self._ctx, B, (C.c_int * B)(*slots), L.ptr(vol), L.ptr(te), L.ptr(vr),
                                                   L.ptr(vi), *ptrs, _stream()))
        return outs

    def frustum_volumes(self, t_embed, v_embed, view_idx):
        dev = self.device
        vi = view_idx.to(device=dev, dtype=torch.int32).contiguous()
        TN = vi.shape[0]
        outs = {}
        ptrs = []
        for lvl, (Dl, Sl) in enumerate(_level_dims(self.vcfg.frustum_volume_depth, self.vcfg.frustum_volume_size)):
            o = torch.empty(TN, self.vcfg.frustum_dims[lvl], Dl, Sl, Sl, device=dev, dtype=torch.float32)
            outs[Sl] = o
            ptrs.append(L.ptr(o))
        te, ve = _f32(t_embed, dev), _f32(v_embed, dev)
        L.check(self.lib.mvd_frustum_volumes(self._ctx, L.ptr(te), L.ptr(ve), L.ptr(vi), TN, *ptrs, _stream()))
        return outs

    def denoise_views(self, x_noisy, x_input, clip, timestep, t_embed, v_embed, view_idx, cfg_scale, noise, coef,
                      want_eps=False, out=None, eps_out=None):
        """coef = (sqrt_one_minus_at, sqrt_at, sqrt_aprev, dir_coef, sigma) python floats.  ``out`` / ``eps_out``: contiguous
        float32 device tensors shaped like x_noisy that receive x_prev / the guided eps directly (no copy afterwards)."""
        dev = self.device
        x = _f32(x_noisy, dev)
        vi = view_idx.to(device=dev, dtype=torch.int32).contiguous()
        TN = vi.shape[0]

        def direct(t):
            return t is not None and t.is_contiguous() and t.dtype == torch.float32 and t.device == x.device and t.shape == x.shape

        x_prev = out if direct(out) else torch.empty_like(x)
        eps = (eps_out if direct(eps_out) else torch.empty_like(x)) if want_eps else None
        nz = None if noise is None else _f32(noise, dev)
        xi, cl, te, ve = _f32(x_input, dev), _f32(clip, dev), _f32(t_embed, dev), _f32(v_embed, dev)
        L.check(self.lib.mvd_denoise_views(
            self._ctx, L.ptr(x), L.ptr(xi), L.ptr(cl), timestep, L.ptr(te), L.ptr(ve), L.ptr(vi), TN, cfg_scale, L.ptr(nz),
            *coef[:5], L.ptr(eps), L.ptr(x_prev), _stream()))
        if out is not None and x_prev is not out:
            out.copy_(x_prev)
        if want_eps and eps_out is not None and eps is not eps_out:
            eps_out.copy_(eps)
        return (x_prev, eps) if want_eps else x_prev

    def denoise_views_batch(self, slots, x_noisy, x_input, clip, timesteps, t_embed, v_embed, view_idx, cfg_scale, noise, coef,
                            want_eps=False):
        """B samples in one UNet pass (mvd_denoise_views_batch): x_noisy / noise [B,TN,4,h,w], x_input [B,4,h,w], clip [B,768],
        timesteps: B python ints, t_embed [B,td], v_embed [B,TN,vd]; slots[b] holds sample b's tables, cameras and volume."""
        dev = self.device
        x = _f32(x_noisy, dev)
        B, TN = x.shape[:2]
        vi = view_idx.to(device=dev, dtype=torch.int32).contiguous()
        assert vi.shape[0] == TN and len(slots) == B and len(timesteps) == B
        x_prev = torch.empty_like(x)
        eps = torch.empty_like(x) if want_eps else None
        nz = None if noise is None else _f32(noise, dev)
        xi, cl, te, ve = _f32(x_input, dev), _f32(clip, dev), _f32(t_embed, dev), _f32(v_embed, dev)
        sl = (C.c_int * B)(*slots)
        ts = (C.c_int64 * B)(*timesteps)
        L.check(self.lib.mvd_denoise_views_batch(
            self._ctx, B, sl, L.ptr(x), L.ptr(xi), L.ptr(cl), ts, L.ptr(te), L.ptr(ve), L.ptr(vi), TN, cfg_scale,
            L.ptr(nz), *coef[:5], L.ptr(eps), L.ptr(x_prev), _stream()))
        return (x_prev, eps) if want_eps else x_prev

    def denoise_views_ms(self, slots, x_noisy, x_input, clip, timesteps, t_embed, v_embed, view_idx, cfg_scale, noise, coef,
                         x0_hist, first, want_eps=False, out=None, eps_out=None):
        """One denoising step with the DPM-Solver++ multistep update (mvd_denoise_views_ms).  slots None: one sample, shaped as for
        denoise_views (x_noisy [TN,4,h,w], timesteps one int); else the shapes of denoise_views_batch.  coef = (s1m, sqrt_at, c_x,
        c_d, c_c, c_n) python floats (DPMSolverSchedule.coefficients); x0_hist: contiguous float32 device tensor shaped like
        x_noisy, read (unless ``first``) and overwritten with this step's x0.  ``out`` / ``eps_out`` as for denoise_views."""
        dev = self.device
        x = _f32(x_noisy, dev)
        single = slots is None
        B, TN = (1, x.shape[0]) if single else x.shape[:2]
        vi = view_idx.to(device=dev, dtype=torch.int32).contiguous()
        steps = [timesteps] if single else list(timesteps)
        assert vi.shape[0] == TN and len(steps) == B and (single or len(slots) == B)
        if not (x0_hist.is_contiguous() and x0_hist.dtype == torch.float32 and x0_hist.device == x.device and x0_hist.shape == x.shape):
            raise ValueError("x0_hist must be a contiguous float32 tensor on the engine's device shaped like x_noisy")

        def direct(t):
            return t is not None and t.is_contiguous() and t.dtype == torch.float32 and t.device == x.device and t.shape == x.shape

        x_next = out if direct(out) else torch.empty_like(x)
        eps = (eps_out if direct(eps_out) else torch.empty_like(x)) if want_eps else None
        nz = None if noise is None else _f32(noise, dev)
        xi, cl, te, ve = _f32(x_input, dev), _f32(clip, dev), _f32(t_embed, dev), _f32(v_embed, dev)
        sl = None if single else (C.c_int * B)(*slots)
        ts = (C.c_int64 * B)(*steps)
        L.check(self.lib.mvd_denoise_views_ms(
            self._ctx, B, sl, L.ptr(x), L.ptr(xi), L.ptr(cl), ts, L.ptr(te), L.ptr(ve), L.ptr(vi), TN, cfg_scale,
            L.ptr(nz), *coef, L.ptr(x0_hist), bool(first), L.ptr(eps), L.ptr(x_next), _stream()))
        if out is not None and x_next is not out:
            out.copy_(x_next)
        if want_eps and eps_out is not None and eps is not eps_out:
            eps_out.copy_(eps)
        return (x_next, eps) if want_eps else x_next

    # ---- single-kernel hooks (parity tests) -------------------------------------------------------
    def op_cfg_ms(self, eps_c, eps_u, scale, x, noise, coef, x0_hist, first, want_eps=False):
        """The update kernel of denoise_views_ms alone (mvd_op_cfg_ms) over flat float32 device tensors: returns x_next (and the
        guided eps); x0_hist is updated in place.  eps_u / noise may be None."""
        dev = self.device
        ec, x = _f32(eps_c, dev), _f32(x, dev)
        eu = None if eps_u is None else _f32(eps_u, dev)
        nz = None if noise is None else _f32(noise, dev)
        assert x0_hist.is_contiguous() and x0_hist.dtype == torch.float32 and x0_hist.numel() == x.numel()
        x_next = torch.empty_like(x)
        eps = torch.empty_like(x) if want_eps else None
        L.check(self.lib.mvd_op_cfg_ms(L.ptr(ec), L.ptr(eu), scale, L.ptr(x), L.ptr(nz), *coef, L.ptr(x0_hist), bool(first),
                                       L.ptr(eps), L.ptr(x_next), x.numel(), _stream()))
        return (x_next, eps) if want_eps else x_next

    def op_conv(self, x, w, bias=None, stride=1, upsample=0, resid=None, force_splitk=0):
        dev = self.device
        x, w = _f32(x, dev), _f32(w, dev)
        B, Cin, H, W = x.shape
        Cout, k = w.shape[0], w.shape[2]
        Ho, Wo = ((H << upsample) - 1) // stride + 1, ((W << upsample) - 1) // stride + 1
        out = torch.empty(B, Cout, Ho, Wo, device=dev)
        b = None if bias is None else _f32(bias, dev)
        r = None if resid is None else _f32(resid, dev)
        L.check(self.lib.mvd_op_conv(self._ctx, L.ptr(x), B, Cin, H, W, L.ptr(w), L.ptr(b), Cout, k, stride, upsample,
                                     L.ptr(r), L.ptr(out), force_splitk, _stream()))
        return out

    def op_conv3d(self, x, w, bias=None, stride=1, transposed=False, resid=None):
        dev = self.device
        x, w = _f32(x, dev), _f32(w, dev)
        B, Cin, D, H, W = x.shape
        Cout = w.shape[1] if transposed else w.shape[0]
        if transposed:
            od = (2 * D, 2 * H, 2 * W)
        else:
            od = ((D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1)
        out = torch.empty(B, Cout, *od, device=dev)
        b = None if bias is None else _f32(bias, dev)
        r = None if resid is None else _f32(resid, dev)
        L.check(self.lib.mvd_op_conv3d(self._ctx, L.ptr(x), B, Cin, D, H, W, L.ptr(w), L.ptr(b), Cout, stride,
                                       bool(transposed), L.ptr(r), L.ptr(out), _stream()))
        return out

    def op_linear(self, a, w, bias=None, geglu=False, resid=None, a_half=False, force_splitk=0):
        dev = self.device
        a, w = _f32(a, dev), _f32(w, dev)
        M, K = a.shape
        N = w.shape[0]
        out = torch.empty(M, N // 2 if geglu else N, device=dev)
        b = None if bias is None else _f32(bias, dev)
        r = None if resid is None else _f32(resid, dev)
        L.check(self.lib.mvd_op_linear(self._ctx, L.ptr(a), M, K, L.ptr(w), L.ptr(b), N, bool(geglu), L.ptr(r),
                                       bool(a_half), force_splitk, L.ptr(out), _stream()))
        return out

    # ---- forward-form hooks (tests/test_gpu_epilogue_forms.py): result buffers are allocated here with one guard row behind them
    # (and pad columns where ld > width), preset to 0xFF bytes -- NaN in every type the kernels write; each wrapper asserts that
    # the guard came back unchanged
    def _guarded(self, rows, ld, f32=True):
        return _nan_guarded(rows, ld, self.device, torch.float32 if f32 else (torch.float16 if L.DTYPE == "f16" else torch.bfloat16))

    @staticmethod
    def _guard_intact(t, rows, width, what):
        _nan_guard_intact(t, rows, what, width)

    def _epi_args(self, rows, N, B, bias, rowbias, rb_ld, resid, ldr, out_f16, out_split, ldc, defer_cap):
        """Stages the epilogue operands shared by op_linear_ex / op_conv_ex; rows: output rows."""
        dev = self.device
        if out_split and not out_f16:
            raise ValueError("out_split is a form of the 16-bit result")
        width = 3 * N if out_split else N
        ldc = ldc or width
        b = None if bias is None else _f32(bias, dev)
        rb = None
        if rowbias is not None:
            rb_ld = rb_ld or N
            rb = torch.full((B, rb_ld), float("nan"), device=dev)
            rb[:, :N] = _f32(rowbias, dev).reshape(B, N)
        r = None
        if resid is not None:
            ldr = ldr or N
            r = torch.full((rows, ldr), float("nan"), device=dev)
            r[:, :N] = _f32(resid, dev).reshape(rows, N)
        out = self._guarded(rows, ldc, f32=not out_f16)
        slabs = None
        if defer_cap:
            slabs = torch.empty(defer_cap + N, device=dev)  # one guard row behind the offered capacity
            slabs.view(torch.int32).fill_(-1)
        return b, rb, rb_ld or 0, r, ldr or 0, out, ldc, width, slabs

    def _epi_result(self, what, out, rows, N, width, out_split, slabs, defer_cap, sk_used):
        self._guard_intact(out, rows, width, what)
        res = types.SimpleNamespace(raw=out[:rows], sk_used=sk_used, slabs=None, hi=None, lo=None, third=None)
        bits = out.view(torch.int32 if out.dtype == torch.float32 else torch.int16)
        res.out_untouched = bool((bits == -1).all())
        if out_split:
            res.hi, res.lo, res.third = out[:rows, :N], out[:rows, N:2 * N], out[:rows, 2 * N:3 * N]
            res.out = res.hi.float() + res.lo.float()
        else:
            res.out = out[:rows, :N].float()
        if slabs is not None:
            used = sk_used * rows * N if sk_used > 1 else 0
            assert used <= defer_cap, f"{what}: sk_used = {sk_used} does not fit the offered slab capacity"
            assert bool((slabs.view(torch.int32)[used:] == -1).all()), f"{what}: the launch wrote behind the slabs it reported"
            if sk_used > 1:
                res.slabs = slabs[:used].reshape(sk_used, rows, N)
        return res

    def op_linear_ex(self, a, w, bias=None, B=1, rowbias=None, rb_ld=0, alpha=1.0, act=0, use_bias=True, out_f16=False,
                     out_split=False, ldc=0, resid=None, resid_f16=False, ldr=0, a_half=False, force_splitk=0, xp=False, defer_cap=0,
                     defer_epilogue=False, poison=True):
        """mvd_op_linear_ex: a [rows][K], w [N][K], rowbias [B][N], resid [rows][N] -> a namespace with .out (fp32 [rows][N]; hi + lo
        with out_split, then also .hi / .lo / .third, the raw 16-bit blocks), .raw (the result rows as written), .sk_used, .slabs
        ([sk_used][rows][N] when the launch deferred its reduction, else None) and .out_untouched (all of `out` still 0xFF)."""
        dev = self.device
        a, w = _f32(a, dev), _f32(w, dev)
        rows, K = a.shape
        N = w.shape[0]
        b, rb, rb_ld, r, ldr, out, ldc, width, slabs = self._epi_args(rows, N, B, bias, rowbias, rb_ld, resid, ldr, out_f16, out_split,
                                                                      ldc, defer_cap)
        sk = C.c_int(-1)
        L.check(self.lib.mvd_op_linear_ex(self._ctx, L.ptr(a), B, rows, K, L.ptr(w), L.ptr(b), N, L.ptr(rb), rb_ld, alpha, act,
                                          bool(use_bias and b is not None), bool(out_f16), bool(out_split), ldc, L.ptr(r), bool(resid_f16),
                                          ldr, bool(a_half), force_splitk, bool(xp), L.ptr(slabs), defer_cap, bool(defer_epilogue),
                                          C.byref(sk), bool(poison), L.ptr(out), _stream()))
        return self._epi_result("op_linear_ex", out, rows, N, width, out_split, slabs, defer_cap, sk.value)

    def op_conv_ex(self, x, w, bias=None, stride=1, upsample=0, up_fold=False, tap_shift=0, rowbias=None, rb_ld=0, alpha=1.0, act=0,
                   use_bias=True, out_f16=False, out_split=False, ldc=0, resid=None, resid_f16=False, ldr=0, a_half=True, force_splitk=0,
                   xp=False, conv3x=True, defer_cap=0, defer_epilogue=False, poison=True):
        """mvd_op_conv_ex: x [B,Cin,H,W], w [Cout,Cin,k,k], rowbias [B,Cout], resid [B,Cout,Ho,Wo] (reference layouts; the hook's
        channels-last images are made here) -> the namespace of op_linear_ex, plus .nchw ([B,Cout,Ho,Wo] fp32)."""
        dev = self.device
        x, w = _f32(x, dev), _f32(w, dev)
        B, Cin, H, W = x.shape
        Cout, k = w.shape[0], w.shape[2]
        Ho, Wo = ((H << upsample) - 1) // stride + 1, ((W << upsample) - 1) // stride + 1
        rows = B * Ho * Wo
        xl = x.permute(0, 2, 3, 1).contiguous()
        rl = None if resid is None else _f32(resid, dev).permute(0, 2, 3, 1).reshape(rows, Cout)
        b, rb, rb_ld, r, ldr, out, ldc, width, slabs = self._epi_args(rows, Cout, B, bias, rowbias, rb_ld, rl, ldr, out_f16, out_split,
                                                                      ldc, defer_cap)
        sk = C.c_int(-1)
        L.check(self.lib.mvd_op_conv_ex(self._ctx, L.ptr(xl), B, H, W, Cin, L.ptr(w), L.ptr(b), Cout, k, stride, upsample, bool(up_fold),
                                        tap_shift, L.ptr(rb), rb_ld, alpha, act, bool(use_bias and b is not None), bool(out_f16),
                                        bool(out_split), ldc, L.ptr(r), bool(resid_f16), ldr, bool(a_half), force_splitk, bool(xp),
                                        bool(conv3x), L.ptr(slabs), defer_cap, bool(defer_epilogue), C.byref(sk), bool(poison), L.ptr(out),
                                        _stream()))
        res = self._epi_result("op_conv_ex", out, rows, Cout, width, out_split, slabs, defer_cap, sk.value)
        res.nchw = res.out.reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2).contiguous()
        return res

    def op_conv3d_ex(self, x, w, bias=None, stride=1, transposed=False, use_bias=True, resid=None, ldr=0, in_place=False,
                     out_f16=False, ldc=0, a_half=True, force_splitk=0, poison=True, form=None):
        """mvd_op_conv3d_ex (form None) / mvd_op_conv3d_form: x [B,Cin,D,H,W], w [Cout,Cin,3,3,3] ([Cin,Cout,3,3,3] transposed), resid [B,Cout,Do,Ho,Wo] (reference
        layouts; the hook's channels-last images are made here) -> a namespace with .out (fp32 [B,Cout,Do,Ho,Wo]) and .raw (the
        result rows [rows][Cout] as written, fp32 or the library's 16-bit type).  The guard row and the pad columns of the result
        buffer are asserted unchanged."""
        dev = self.device
        x, w = _f32(x, dev), _f32(w, dev)
        B, Cin, D, H, W = x.shape
        Cout = w.shape[1] if transposed else w.shape[0]
        od = (2 * D, 2 * H, 2 * W) if transposed else tuple((n - 1) // stride + 1 for n in (D, H, W))
        rows = B * od[0] * od[1] * od[2]
        xl = x.permute(0, 2, 3, 4, 1).contiguous()
        b = None if bias is None else _f32(bias, dev)
        r = None
        if resid is not None:
            ldr = ldr or Cout
            r = torch.full((rows, ldr), float("nan"), device=dev)
            r[:, :Cout] = _f32(resid, dev).permute(0, 2, 3, 4, 1).reshape(rows, Cout)
        ldc = ldc or Cout
        out = self._guarded(rows, ldc, f32=not out_f16)
        head = (self._ctx, L.ptr(xl), B, D, H, W, Cin, L.ptr(w), L.ptr(b), Cout, stride, bool(transposed),
                bool(use_bias and b is not None), L.ptr(r), ldr or 0, bool(in_place), bool(out_f16), ldc, bool(a_half), force_splitk)
        tail = (bool(poison), L.ptr(out), _stream())
        if form is None:
            L.check(self.lib.mvd_op_conv3d_ex(*head, *tail))
        else:
            L.check(self.lib.mvd_op_conv3d_form(*head, int(form), *tail))
        self._guard_intact(out, rows, Cout, "op_conv3d_ex")
        raw = out[:rows, :Cout]
        return types.SimpleNamespace(raw=raw, out=raw.float().reshape(B, *od, Cout).permute(0, 4, 1, 2, 3).contiguous())

    def op_conv3d_form(self, x, w, form, **kw):
        """mvd_op_conv3d_form: op_conv3d_ex on the kernel form the caller names (0: the engine's routing, 1: conv3z, the plane-halo
        kernel of the 3x3x3 stride-1 layers); a layer outside the form's limits raises MvdError"""
        return self.op_conv3d_ex(x, w, form=form, **kw)

    def op_group_norm_ex(self, x, groups, gamma, beta, eps=1e-5, act=0, form=0, ld=0, preadd=None, pld=0, split=0, bias2=None,
                         resid=None, ldr=0, mat=False, ldm=0, ldo=0, poison=True):
        """mvd_op_group_norm_ex: x [nslab, B, rows, C] channels-last slabs (or [B, rows, C]); preadd [B, C], bias2 [C], resid
        [B, rows, C] -> (out fp32 [B, rows, C] -- hi + lo with split = 1, NaN where the third block differs from the first --,
        mat fp32 [B, rows, C] or None).  ld / pld / ldr / ldm / ldo: row strides (0: dense); pad columns of the inputs hold NaN."""
        dev = self.device
        x = _f32(x, dev)
        if x.dim() == 3:
            x = x[None]
        nslab, B, rows, Cc = x.shape
        ld = ld or Cc

        def padded(t, lead, ldt):
            p = torch.full((*lead, ldt), float("nan"), device=dev)
            p[..., :Cc] = _f32(t, dev).reshape(*lead, Cc)
            return p
        xs = padded(x, (nslab, B, rows), ld)
        pre = None if preadd is None else padded(preadd, (B,), pld or Cc)
        res = None if resid is None else padded(resid, (B, rows), ldr or Cc)
        b2 = None if bias2 is None else _f32(bias2, dev)
        g, bt = _f32(gamma, dev), _f32(beta, dev)
        wmul = 3 if split == 1 else 1
        ldo_h = ldo or ((2 if split == 2 else wmul) * Cc)  # in 16-bit elements, as run_group_norm counts it
        if split == 2:
            out = self._guarded(B * rows, ldo_h // 2, f32=True)
        else:
            out = self._guarded(B * rows, ldo_h, f32=False)
        m = self._guarded(B * rows, ldm or Cc, f32=True) if mat else None
        L.check(self.lib.mvd_op_group_norm_ex(self._ctx, L.ptr(xs), B, rows, Cc, ld, groups, L.ptr(g), L.ptr(bt), eps, act, form,
                                              L.ptr(pre), (pld or Cc) if pre is not None else 0, split, nslab, B * rows * ld, L.ptr(b2),
                                              L.ptr(res), (ldr or Cc) if res is not None else 0, L.ptr(m), (ldm or Cc) if mat else 0,
                                              ldo_h, bool(poison), L.ptr(out), _stream()))
        self._guard_intact(out, B * rows, wmul * Cc, "op_group_norm_ex")
        if mat:
            self._guard_intact(m, B * rows, Cc, "op_group_norm_ex (mat)")
        if split == 1:
            hi, lo, third = out[:-1, :Cc], out[:-1, Cc:2 * Cc], out[:-1, 2 * Cc:3 * Cc]
            y = hi.float() + lo.float()
            y[hi.view(torch.int16) != third.view(torch.int16)] = float("nan")
        else:
            y = out[:-1, :Cc].float()
        return y.reshape(B, rows, Cc), (m[:-1, :Cc].reshape(B, rows, Cc).clone() if mat else None)

    def op_layer_norm_slabs(self, slabs, gamma, beta, bias=None, rowbias=None, rb_ld=0, T=None, resid=None, ldr=0, eps=1e-5,
                            plain=False, raw=False, ld_raw=0, poison=True):
        """mvd_op_layer_norm_slabs: slabs [nslab, rows, C] (or [rows, C]), rowbias [ceil(rows / T), C], resid [rows, C] ->
        (out fp32 [rows, C], mat fp32 [rows, C] or None with plain, raw 16-bit [rows, C] or None)."""
        dev = self.device
        x = _f32(slabs, dev)
        if x.dim() == 2:
            x = x[None]
        nslab, rows, Cc = x.shape
        g, bt = _f32(gamma, dev), _f32(beta, dev)
        b = None if bias is None else _f32(bias, dev)
        rb = None
        if rowbias is not None:
            rb = torch.full((rowbias.shape[0], rb_ld or Cc), float("nan"), device=dev)
            rb[:, :Cc] = _f32(rowbias, dev)
        r = None
        if resid is not None:
            r = torch.full((rows, ldr or Cc), float("nan"), device=dev)
            r[:, :Cc] = _f32(resid, dev)
        out = self._guarded(rows, Cc, f32=False)
        m = None if plain else self._guarded(rows, Cc, f32=True)
        rw = self._guarded(rows, ld_raw or Cc, f32=False) if raw else None
        L.check(self.lib.mvd_op_layer_norm_slabs(self._ctx, L.ptr(x), nslab, rows * Cc, rows, Cc, L.ptr(b), L.ptr(rb),
                                                 (rb_ld or Cc) if rb is not None else 0, T or rows, L.ptr(r),
                                                 (ldr or Cc) if r is not None else 0, L.ptr(g), L.ptr(bt), eps, bool(plain),
                                                 (ld_raw or Cc) if raw else 0, bool(poison), L.ptr(m), L.ptr(rw), L.ptr(out), _stream()))
        self._guard_intact(out, rows, Cc, "op_layer_norm_slabs")
        if m is not None:
            self._guard_intact(m, rows, Cc, "op_layer_norm_slabs (mat)")
        if rw is not None:
            self._guard_intact(rw, rows, Cc, "op_layer_norm_slabs (raw)")
        return out[:rows].float(), (None if m is None else m[:rows].clone()), (None if rw is None else rw[:rows, :Cc].clone())

    def op_folded_group_norm(self, x, w, cpg, gamma, beta, B, eps=1e-5, poison=True):
        """mvd_op_folded_group_norm: x [B * rps][K], w [N][K] -> (partials [B, rps / 256, N / cpg, 2], scale [B, N], shift [B, N],
        out fp32 [B * rps][N] = relu(group_norm(x @ w^T)) as the apply pass wrote it in 16 bits)."""
        dev = self.device
        x, w, g, bt = _f32(x, dev), _f32(w, dev), _f32(gamma, dev), _f32(beta, dev)
        rows, K = x.shape
        N = w.shape[0]
        if B <= 0 or rows % B or cpg <= 0 or N % cpg:
            raise L.MvdError("op_folded_group_norm: rows % B == 0 and N % cpg == 0 expected")
        rps, G = rows // B, N // cpg
        ntile = max(rps // 256, 1)
        part = self._guarded(B * ntile, 2 * G)
        sc, sh = self._guarded(B, N), self._guarded(B, N)
        out = self._guarded(rows, N, f32=False)
        L.check(self.lib.mvd_op_folded_group_norm(self._ctx, L.ptr(x), B, rps, K, L.ptr(w), N, cpg, L.ptr(g), L.ptr(bt), eps,
                                                  bool(poison), L.ptr(part), L.ptr(sc), L.ptr(sh), L.ptr(out), _stream()))
        for t, n, name in ((part, B * ntile, "partials"), (sc, B, "scale"), (sh, B, "shift"), (out, rows, "out")):
            self._guard_intact(t, n, t.shape[1], f"op_folded_group_norm ({name})")
        return part[:-1].reshape(B, ntile, G, 2).clone(), sc[:B].clone(), sh[:B].clone(), out[:rows].float()

    def op_softmax_rows(self, scores, out_f32=False):
        """mvd_op_softmax_rows: [rows][cols] fp32 scores -> probabilities, fp32 or the kernels' 16-bit type (returned as written)."""
        s = _f32(scores, self.device)
        rows, cols = s.shape
        out = self._guarded(rows, cols, f32=bool(out_f32))
        L.check(self.lib.mvd_op_softmax_rows(self._ctx, L.ptr(s), rows, cols, bool(out_f32), L.ptr(out), _stream()))
        self._guard_intact(out, rows, cols, "op_softmax_rows")
        return out[:rows].clone()

    def op_rows_split(self, x, lda=0):
        """mvd_op_rows_split (launch_rows_f32_to_f16_split): x [rows][C] -> (hi, lo, third), the raw 16-bit blocks."""
        dev = self.device
        x = _f32(x, dev)
        rows, Cc = x.shape
        lda = lda or Cc
        xp = torch.full((rows, lda), float("nan"), device=dev)
        xp[:, :Cc] = x
        out = self._guarded(rows, 3 * Cc, f32=False)
        L.check(self.lib.mvd_op_rows_split(self._ctx, L.ptr(xp), lda, rows, Cc, L.ptr(out), _stream()))
        self._guard_intact(out, rows, 3 * Cc, "op_rows_split")
        return out[:rows, :Cc].clone(), out[:rows, Cc:2 * Cc].clone(), out[:rows, 2 * Cc:].clone()

    def op_group_norm(self, x, groups, gamma, beta, eps, act=0):
        dev = self.device
        x = _f32(x, dev)
        B, Cc = x.shape[:2]
        HW = x[0, 0].numel()
        out = torch.empty_like(x)
        g, b = _f32(gamma, dev), _f32(beta, dev)  # keep alive across the call
        L.check(self.lib.mvd_op_group_norm(self._ctx, L.ptr(x), B, Cc, HW, groups, L.ptr(g), L.ptr(b), eps,
                                           act, L.ptr(out), _stream()))
        return out

    def op_layer_norm(self, x, gamma, beta):
        """launch_layernorm with eps = 1e-5 on x [rows, C]: the plain form of op_layer_norm_slabs (16-bit result, returned as fp32)."""
        return self.op_layer_norm_slabs(x, gamma, beta, eps=1e-5, plain=True)[0]

    def op_st_tail(self, xin, ln_g, ln_b, w1, b1, w2, b2, ao=None, w_ao=None, b_ao=None, rowbias=None, T=None, w_po=None, b_po=None,
                   resid=None, split=False, iters=0, xp_out=False):
        """Row-chain kernel (csrc/k_rowchain.hip) through the C ABI: [to_out + t0] -> LayerNorm3 -> FF -> + t2 [-> proj_out + x_in].
        Returns the fp32 result (and the mean milliseconds per launch when iters > 0)."""
        dev = self.device
        xin = _f32(xin, dev)
        rows, Cc = xin.shape
        keep = [_f32(t, dev) if t is not None else None for t in (ao, rowbias, w_ao, b_ao, ln_g, ln_b, w1, b1, w2, b2, w_po, b_po, resid)]
        ao_, rb_, wao_, bao_, g_, b_, w1_, b1_, w2_, b2_, wpo_, bpo_, res_ = keep
        flags = (1 if ao is not None else 0) | (2 if w_po is not None else 0) | (4 if split else 0) | (8 if xp_out else 0)
        out = torch.empty_like(xin)
        ms = C.c_float(0)
        L.check(self.lib.mvd_op_st_tail(self._ctx, Cc, rows, T or rows, L.ptr(ao_), L.ptr(xin), L.ptr(rb_), L.ptr(wao_), L.ptr(bao_),
                                        L.ptr(g_), L.ptr(b_), L.ptr(w1_), L.ptr(b1_), L.ptr(w2_), L.ptr(b2_), L.ptr(wpo_), L.ptr(bpo_),
                                        L.ptr(res_), L.ptr(out), flags, iters, C.byref(ms), _stream()))
        return (out, ms.value) if iters > 0 else out

    def op_st_head(self, n0, w_pi, b_pi, ln_g, ln_b, w_q, w_k, w_v, iters=0, xp=False):
        """Row-head kernel (csrc/k_rowchain.hip) through the C ABI: proj_in -> t0, LayerNorm1, q | k | v.  Returns (t0, qkv[, ms])."""
        dev = self.device
        n0 = _f32(n0, dev)
        rows, Cc = n0.shape
        keep = [_f32(t, dev) for t in (w_pi, b_pi, ln_g, ln_b, w_q, w_k, w_v)]
        t0 = torch.empty(rows, Cc, device=dev)
        qkv = torch.empty(rows, 3 * Cc, device=dev)
        ms = C.c_float(0)
        L.check(self.lib.mvd_op_st_head(self._ctx, rows, bool(xp), L.ptr(n0), *[L.ptr(t) for t in keep], L.ptr(t0), L.ptr(qkv), iters,
                                        C.byref(ms), _stream()))
        return (t0, qkv, ms.value) if iters > 0 else (t0, qkv)

    def op_attention(self, q, k, v, heads):
        return self.op_attention_ex(q, k, v, heads)

    def op_attention_ex(self, q, k, v, heads, Tstride=0, ld_pad=0, xcd=-1):
        """mvd_op_attention_ex: attn_kernel on the fused 16-bit image with samples ``Tstride`` rows apart (0 = T) and ``ld_pad`` pad
        columns, everything but q, k, v preset to NaN.  Asserts that every pad row and the guard row of the result are still NaN
        (the kernel wrote its own rows only) and returns [B,T,C] fp32.  xcd: -1 environment, 0 / 1 without / with the XCD remap."""
        dev = self.device
        q, k, v = _f32(q, dev), _f32(k, dev), _f32(v, dev)
        B, T, Cc = q.shape
        Ts = Tstride or T
        out = torch.zeros(B * max(Ts, T) + 1, Cc, device=dev, dtype=torch.float32)
        L.check(self.lib.mvd_op_attention_ex(self._ctx, L.ptr(q), L.ptr(k), L.ptr(v), B, T, heads, Cc // heads, Tstride, ld_pad, xcd,
                                             L.ptr(out), _stream()))
        body = out[:B * Ts].reshape(B, Ts, Cc)
        assert _guard_ok(out, B * Ts, exact=False) and bool(torch.isnan(body[:, T:]).all()), \
            "op_attention_ex: the launch wrote outside its result (a pad row or the guard row changed)"
        return body[:, :T].clone()

    def op_attention_bwd_ex(self, q, k, v, d_out, heads):
        """mvd_op_attention_bwd_ex -> (dq, dk, dv [B,T,C], lse [B,heads,T] in log2 units, delta [B,heads,T], o [B,T,C]).  Asserts the
        guard rows behind dqkv, o, lse and delta and that the kernels wrote every element they return."""
        dev = self.device
        q, k, v, d_out = _f32(q, dev), _f32(k, dev), _f32(v, dev), _f32(d_out, dev)
        B, T, Cc = q.shape
        rows, nstat = B * T, B * heads * T
        dq, dk, dv, o = (torch.zeros(rows + 1, Cc, device=dev, dtype=torch.float32) for _ in range(4))
        lse, delta = (torch.zeros(nstat + 1, device=dev, dtype=torch.float32) for _ in range(2))
        L.check(self.lib.mvd_op_attention_bwd_ex(self._ctx, L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(d_out), B, T, heads, Cc // heads,
                                                 L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(lse), L.ptr(delta), L.ptr(o), _stream()))
        for t, n, name in ((dq, rows, "dq"), (dk, rows, "dk"), (dv, rows, "dv"), (o, rows, "o"), (lse, nstat, "lse"), (delta, nstat, "delta")):
            assert _guard_ok(t, n, exact=False), f"op_attention_bwd_ex: the launch wrote behind {name} (guard changed)"
            assert not bool(torch.isnan(t[:n]).any()), f"op_attention_bwd_ex: elements of {name} were never written (still NaN)"
        return (dq[:rows].reshape(B, T, Cc), dk[:rows].reshape(B, T, Cc), dv[:rows].reshape(B, T, Cc),
                lse[:nstat].reshape(B, heads, T), delta[:nstat].reshape(B, heads, T), o[:rows].reshape(B, T, Cc))

    def op_depth_attn(self, qk, ctx, fill_row=None, nfill=0, split=False, ldx=0, heads=4, return_hi=False):
        """depth_attn_kernel (csrc/k_depth.hip) on its own: qk [n_cond*HW, 4, Cc] (the folded query), ctx [n_cond, D, HW, Cc]
        (rounded to fp16 by the hook, rows ``ldx`` halfs apart, pad columns NaN), fill_row [4*Cc] with nfill > 0.  Returns
        [n_cond*HW + nfill + 1, 4*Cc] fp32: z, the fill rows, and the hook's guard row (NaN when the launch kept inside its rows);
        split: the kernel's [hi | lo | hi] form, returned as hi + lo (with return_hi also hi alone)."""
        dev = self.device
        qk, ctx = _f32(qk, dev), _f32(ctx, dev)
        n_cond, D, HW, Cc = ctx.shape
        fr = None if fill_row is None else _f32(fill_row, dev)
        err = self.op_depth_attn_check(D, Cc, heads=heads, ldx=ldx, nfill=nfill)
        if err is not None:
            raise L.MvdError(err)
        if qk.numel() != n_cond * HW * 4 * Cc or (nfill > 0 and (fr is None or fr.numel() != 4 * Cc)):
            raise ValueError("op_depth_attn: qk / fill_row do not match the context's shape")
        out = torch.empty(n_cond * HW + nfill + 1, 4 * Cc, device=dev, dtype=torch.float32)
        hi = torch.empty_like(out) if split and return_hi else None
        L.check(self.lib.mvd_op_depth_attn(self._ctx, L.ptr(qk), L.ptr(ctx), L.ptr(fr), n_cond, HW, D, Cc, heads, ldx, bool(split),
                                           nfill, 0, L.ptr(out), L.ptr(hi), _stream()))
        return (out, hi) if return_hi else out

    def op_depth_attn_check(self, D, Cc, heads=4, ldx=0, nfill=0):
        """The depth-attention launcher's verdict on a shape, without launching: None, or the text of its refusal."""
        rc = self.lib.mvd_op_depth_attn(self._ctx, None, None, None, 0, 1, D, Cc, heads, ldx, 0, nfill, 1, None, None, _stream())
        return None if rc == 0 else self.lib.mvd_last_error().decode()

    def op_attention_bwd(self, q, k, v, d_out, heads):
        return self.op_attention_bwd_ex(q, k, v, d_out, heads)[:3]

    def op_group_norm_bwd(self, x, dy, groups, gamma, beta, eps, act=0):
        """x, dy [B, rows, C] channels-last -> (dx, dgamma, dbeta)"""
        dev = self.device
        x, dy, g, b = _f32(x, dev), _f32(dy, dev), _f32(gamma, dev), _f32(beta, dev)
        B, rows, Cc = x.shape
        dx, dg, db = torch.empty_like(x), torch.empty_like(g), torch.empty_like(g)
        L.check(self.lib.mvd_op_group_norm_bwd(self._ctx, L.ptr(x), L.ptr(dy), B, rows, Cc, groups, L.ptr(g), L.ptr(b), eps,
                                               act, L.ptr(dx), L.ptr(dg), L.ptr(db), _stream()))
        return dx, dg, db

    def op_layer_norm_bwd(self, x, dy, gamma):
        dev = self.device
        x, dy, g = _f32(x, dev), _f32(dy, dev), _f32(gamma, dev)
        dx, dg, db = torch.empty_like(x), torch.empty_like(g), torch.empty_like(g)
        L.check(self.lib.mvd_op_layer_norm_bwd(self._ctx, L.ptr(x), L.ptr(dy), x.shape[0], x.shape[1], L.ptr(g), L.ptr(dx), L.ptr(dg),
                                               L.ptr(db), _stream()))
        return dx, dg, db

    # ---- the training backward's norms and reductions in their production forms (tests/test_gpu_norm_bwd_ops.py).  Operands go in
    # as rows `ld` floats apart inside NaN-filled buffers (ld = 0: dense); results come back compact from guarded buffers, after the
    # guard row and the pad columns were found bit-exact.  accum: the values a result that is added to starts from.
    def _rows_in(self, t, ld=0, off=0):
        """t [rows, C] -> (buffer [rows, ld] of NaN with t at columns off .. off + C, device pointer of t[0][0] in it, ld)"""
        t = _f32(t, self.device)
        rows, Cc = t.shape
        ld = ld or Cc
        if off + Cc > ld:
            raise ValueError("the operand does not fit its rows")
        buf = torch.full((rows, ld), float("nan"), device=self.device)
        buf[:, off:off + Cc] = t
        return buf, buf.data_ptr() + 4 * off, ld

    def _rows_out(self, rows, Cc, ld=0, start=None, off=0):
        """A guarded result: [rows + 1][ld] of 0xFF bytes, columns off .. off + C of the body preset to `start` where given."""
        ld = ld or Cc
        buf = _nan_guarded(rows, ld, self.device)
        if start is not None:
            buf[:rows, off:off + Cc] = _f32(start, self.device).reshape(rows, Cc)
        return buf, buf.data_ptr() + 4 * off, ld

    @staticmethod
    def _rows_result(buf, rows, Cc, what, off=0):
        _nan_guard_intact(buf, rows, what, off + Cc)
        assert bool((buf.view(torch.int32)[:rows, :off] == -1).all()), f"{what}: the launch wrote left of its columns"
        return buf[:rows, off:off + Cc].clone()

    def _refused(self, rc, bufs, before):
        """rc != 0: raises MvdError with the library's text; its results_untouched says whether every result buffer still holds its
        preset, bit for bit (what a refusal must leave)."""
        if rc == 0:
            return
        torch.cuda.synchronize(self.device)
        err = L.MvdError(self.lib.mvd_last_error().decode())
        err.results_untouched = all(torch.equal(t.view(torch.int32), u.view(torch.int32)) for t, u in zip(bufs, before))
        raise err

    def op_group_norm_bwd_ex(self, x, dy, groups, gamma, beta, eps, act=0, pre=None, pld=0, pre_off=0, form=0, S_force=0, ld=0, x_off=0,
                             ldy=0, lddx=0, accum=None, want_dpre=False, ldp=0, dpre_off=0, poison=False):
        """mvd_op_group_norm_bwd_ex: gn_backward on x, dy [B, rows, C]; pre [B, C] (optional) at column pre_off of rows of pld floats;
        accum = (dx0, dgamma0, dbeta0).  Returns a namespace: dx [B, rows, C], dgamma, dbeta [C], dpre [B, C] or None, S_used."""
        B, rows, Cc = x.shape
        xb, xp, ld = self._rows_in(x.reshape(B * rows, Cc), ld, x_off)
        yb, yp, ldy = self._rows_in(dy.reshape(B * rows, Cc), ldy)
        g, b = _f32(gamma, self.device), _f32(beta, self.device)
        pb, pp, pld = (None, None, 0) if pre is None else self._rows_in(pre.reshape(B, Cc), pld, pre_off)
        a = accum or (None, torch.zeros(Cc), torch.zeros(Cc))
        dxb, dxp, lddx = self._rows_out(B * rows, Cc, lddx, a[0])
        dgb, dgp, _ = self._rows_out(1, Cc, 0, a[1])
        dbb, dbp, _ = self._rows_out(1, Cc, 0, a[2])
        dpb, dpp, ldp = self._rows_out(B, Cc, ldp, None, dpre_off) if want_dpre else (None, None, 0)
        S_used = C.c_int(-1)
        bufs = [t for t in (dxb, dgb, dbb, dpb) if t is not None]
        before = [t.clone() for t in bufs]
        self._refused(self.lib.mvd_op_group_norm_bwd_ex(self._ctx, xp, ld, pp, pld, yp, ldy, B, rows, Cc, groups, L.ptr(g), L.ptr(b), eps, act,
                                                        form, S_force, dxp, lddx, accum is not None, dgp, dbp, dpp, ldp, bool(poison),
                                                        C.byref(S_used), _stream()), bufs, before)
        what = "op_group_norm_bwd_ex"
        return types.SimpleNamespace(dx=self._rows_result(dxb, B * rows, Cc, what + " (dx)").reshape(B, rows, Cc),
                                     dgamma=self._rows_result(dgb, 1, Cc, what + " (dgamma)")[0],
                                     dbeta=self._rows_result(dbb, 1, Cc, what + " (dbeta)")[0],
                                     dpre=self._rows_result(dpb, B, Cc, what + " (dpre)", dpre_off) if want_dpre else None,
                                     S_used=S_used.value)

    def op_group_norm_fwd32(self, x, groups, gamma, beta, eps, act=0, S_force=0, ld=0, x_off=0, ldy=0, poison=False):
        """mvd_op_group_norm_fwd32: gn_forward32 on x [B, rows, C] -> (y [B, rows, C], S_used)."""
        B, rows, Cc = x.shape
        xb, xp, ld = self._rows_in(x.reshape(B * rows, Cc), ld, x_off)
        g, b = _f32(gamma, self.device), _f32(beta, self.device)
        yb, yp, ldy = self._rows_out(B * rows, Cc, ldy)
        S_used = C.c_int(-1)
        L.check(self.lib.mvd_op_group_norm_fwd32(self._ctx, xp, ld, B, rows, Cc, groups, L.ptr(g), L.ptr(b), eps, act, S_force, yp, ldy,
                                                 bool(poison), C.byref(S_used), _stream()))
        return self._rows_result(yb, B * rows, Cc, "op_group_norm_fwd32").reshape(B, rows, Cc), S_used.value

    def op_layer_norm_bwd_ex(self, x, dy, gamma, eps, ld=0, x_off=0, ldy=0, lddx=0, accum=None, poison=False):
        """mvd_op_layer_norm_bwd_ex: ln_backward on x, dy [rows, C]; accum = (dx0, dgamma0, dbeta0).  Returns a namespace: dx,
        dgamma, dbeta, nblk_used."""
        rows, Cc = x.shape
        xb, xp, ld = self._rows_in(x, ld, x_off)
        yb, yp, ldy = self._rows_in(dy, ldy)
        g = _f32(gamma, self.device)
        a = accum or (None, torch.zeros(Cc), torch.zeros(Cc))
        dxb, dxp, lddx = self._rows_out(rows, Cc, lddx, a[0])
        dgb, dgp, _ = self._rows_out(1, Cc, 0, a[1])
        dbb, dbp, _ = self._rows_out(1, Cc, 0, a[2])
        before = [t.clone() for t in (dxb, dgb, dbb)]
        nblk = C.c_int(-1)
        rc = self.lib.mvd_op_layer_norm_bwd_ex(self._ctx, xp, ld, yp, ldy, rows, Cc, L.ptr(g), eps, dxp, lddx, accum is not None, dgp, dbp,
                                               bool(poison), C.byref(nblk), _stream())
        self._refused(rc, (dxb, dgb, dbb), before)
        what = "op_layer_norm_bwd_ex"
        return types.SimpleNamespace(dx=self._rows_result(dxb, rows, Cc, what + " (dx)"),
                                     dgamma=self._rows_result(dgb, 1, Cc, what + " (dgamma)")[0],
                                     dbeta=self._rows_result(dbb, 1, Cc, what + " (dbeta)")[0], nblk_used=nblk.value)

    def op_train_colsum(self, v, B, src_half=False, ld=0, ldo=0, out_off=0):
        """mvd_op_train_colsum: v [B * rows, C] -> [B, C] per-sample column sums, written at column out_off of rows of ldo floats."""
        R, Cc = v.shape
        vb, vp, ld = self._rows_in(v, ld)
        ob, op, ldo = self._rows_out(B, Cc, ldo, None, out_off)
        L.check(self.lib.mvd_op_train_colsum(self._ctx, vp, bool(src_half), ld, B, R // B, Cc, op, ldo, _stream()))
        return self._rows_result(ob, B, Cc, "op_train_colsum", out_off)

    def op_train_sum_rows(self, jobs):
        """mvd_op_train_sum_rows: jobs = [(part [R, C], ldp, out0 [C] or None)], 1..4 of them in ONE launch; out0: the job adds to
        these values (accum = 1), None: it writes.  Returns the [C] results."""
        n = len(jobs)
        parts = [self._rows_in(p, ldp) for p, ldp, _ in jobs]
        outs = [self._rows_out(1, p.shape[1], 0, o) for p, _, o in jobs]
        arr = lambda ty, vals: (ty * n)(*vals)  # noqa: E731
        L.check(self.lib.mvd_op_train_sum_rows(self._ctx, n, arr(C.c_void_p, [p[1] for p in parts]), arr(C.c_int, [j[0].shape[0] for j in jobs]),
                                               arr(C.c_int, [j[0].shape[1] for j in jobs]), arr(C.c_long, [p[2] for p in parts]),
                                               arr(C.c_void_p, [o[1] for o in outs]), arr(C.c_int, [j[2] is not None for j in jobs]),
                                               _stream()))
        return [self._rows_result(o[0], 1, j[0].shape[1], f"op_train_sum_rows (job {k})")[0] for k, (o, j) in enumerate(zip(outs, jobs))]

    def op_train_outer_add(self, a, b, out0, lda=0, ldb=0):
        """mvd_op_train_outer_add: out0 [M, N] + sum_k a[k][:, None] * b[k][None, :] with a [K, M], b [K, N]."""
        ab, ap, lda = self._rows_in(a, lda)
        bb, bp, ldb = self._rows_in(b, ldb)
        (K, M), N = a.shape, b.shape[1]
        ob, op, _ = self._rows_out(M, N, 0, out0)
        L.check(self.lib.mvd_op_train_outer_add(self._ctx, ap, lda, bp, ldb, op, M, N, K, _stream()))
        return self._rows_result(ob, M, N, "op_train_outer_add")

    # ---- small-op hooks (tests/test_gpu_small_ops.py): one production launcher per call, written straight into guarded 0xFF
    # buffers allocated here; a refusal raises MvdError with .results_untouched (Engine._refused).  Operands may be None where a
    # test wants the hook's own refusal.
    def _dev(self, t, dtype=torch.float32):
        return None if t is None else t.detach().to(device=self.device, dtype=dtype).contiguous()

    @staticmethod
    def _bits(t):
        """a result buffer of any element size as the int32 words Engine._refused compares"""
        flat = t.reshape(-1)
        return flat[:flat.numel() * t.element_size() // 4 * 4 // t.element_size()].view(torch.int32)

    def _call_hook(self, fn, args, bufs, form=False):
        """fn(ctx, *args[, &form], stream) with the result buffers watched -> form_used (or None)"""
        before = [t.clone() for t in bufs]
        used = C.c_int(-1)
        tail = (C.byref(used), _stream()) if form else (_stream(),)
        self._refused(fn(self._ctx, *args, *tail), bufs, before)
        return used.value if form else None

    def op_target_encoder(self, x, pre, w, bias, gamma, beta, n=None, out=None):
        """mvd_op_target_encoder: x [n, 4, 32, 32], pre [n, 48], w / bias 8 fp32 tensors, gamma / beta 7 -> the guarded result buffer
        [n * 1024 + 1, 16] (`out`: a buffer of an earlier call, written again as it is)."""
        x, pre = self._dev(x), self._dev(pre)
        n = x.shape[0] if n is None else n
        lists = [[self._dev(t) for t in ts] for ts in (w, bias, gamma, beta)]
        arr = lambda ts: (C.c_void_p * len(ts))(*[L.ptr(t) for t in ts])  # noqa: E731
        rows = max(n, 1) * 1024
        out = _nan_guarded(rows, 16, self.device) if out is None else out
        self._call_hook(self.lib.mvd_op_target_encoder, (L.ptr(x), L.ptr(pre), n, *[arr(ts) for ts in lists], L.ptr(out)), [out])
        _nan_guard_intact(out, rows, "op_target_encoder")
        return out

    def op_small_linear(self, a, w, bias, rows, act=0, lda=0, ldo=0, start=None, a_off=0):
        """mvd_op_small_linear: a [in rows, K] placed a_off floats into a NaN buffer with rows of lda; w [N, K]; start: the result
        is added to these values -> (out [|rows|, N], form_used)."""
        in_rows, K = (1, 1) if a is None else a.shape
        N = 1 if w is None else w.shape[0]
        lda = lda or K
        abuf = torch.full((in_rows * max(lda, K) + 8,), float("nan"), device=self.device)
        if a is not None:
            abuf[a_off:a_off + in_rows * lda].view(in_rows, lda)[:, :K] = self._dev(a)
        w, b = self._dev(w), self._dev(bias)
        ob, op, ldo_ = self._rows_out(abs(rows) or 1, N, max(ldo, N), start)
        form = self._call_hook(self.lib.mvd_op_small_linear, (None if a is None else abuf.data_ptr() + 4 * a_off, lda, rows, K, L.ptr(w),
                                                             L.ptr(b), N, act, op, ldo or N, start is not None), [ob], form=True)
        return self._rows_result(ob, abs(rows), N, "op_small_linear"), form

    def op_timestep_embedding(self, t, dim):
        t = self._dev(t, torch.int64)
        B = t.shape[0]
        ob, op, _ = self._rows_out(B, max(dim, 1))
        self._call_hook(self.lib.mvd_op_timestep_embedding, (L.ptr(t), B, dim, op), [ob])
        return self._rows_result(ob, B, dim, "op_timestep_embedding")

    def op_layout(self, op, x, B, Cc, HW, ld, cpad=0):
        """mvd_op_layout.  op 0: x [B, C, HW] -> ([B * HW, cpad], form), rows of ld floats whose columns from cpad on must come back
        untouched; op 1: x [B * HW, C] in NaN rows of ld floats -> ([B, C, HW], form)."""
        if op == 1:
            xb, xp, _ = self._rows_in(x, max(ld, Cc))
            ob, optr, _ = self._rows_out(B * Cc, HW)
        else:
            xb = self._dev(x)
            xp = L.ptr(xb)
            ob, optr, _ = self._rows_out(B * HW, max(cpad, 1), max(ld, 1))
        form = self._call_hook(self.lib.mvd_op_layout, (op, xp, B, Cc, HW, ld, cpad, optr), [ob], form=True)
        if op == 1:
            return self._rows_result(ob, B * Cc, HW, "op_layout").reshape(B, Cc, HW), form
        return self._rows_result(ob, B * HW, cpad, "op_layout"), form

    def op_pack_weight(self, src, N, Cin, taps, transposed=0, geglu=0, cin_src=0, xp=0, dst_off=0):
        """mvd_op_pack_weight at dst_off halfs into a 16-bit 0xFF buffer -> ([taps, N, Cin] as written, form)."""
        src = self._dev(src)
        n = max(taps * N * Cin, 1)
        buf = torch.full((max(dst_off, 0) + n + 64,), -1, dtype=torch.int16, device=self.device)
        form = self._call_hook(self.lib.mvd_op_pack_weight, (L.ptr(src), N, Cin, taps, transposed, geglu, cin_src, xp, dst_off, L.ptr(buf)),
                               [buf.view(torch.int32)], form=True)
        assert bool((buf[:dst_off] == -1).all()) and bool((buf[dst_off + n:] == -1).all()), "op_pack_weight: the launch wrote outside its result"
        return buf[dst_off:dst_off + n].view(torch.float16 if L.DTYPE == "f16" else torch.bfloat16).reshape(taps, N, Cin).clone(), form

    def op_move(self, op, a, b, ints, rows, width, ld=0, f32=False):
        """mvd_op_move: a (fp32) and b (fp32 or int32) as the op takes them, ints (i0 .. i4, padded with 0) -> [rows, width] of a
        guarded result with rows of ld."""
        a = self._dev(a)
        b = None if b is None else b.detach().to(self.device).contiguous()
        ints = tuple(ints) + (0,) * (5 - len(ints))
        out = self._guarded(rows, ld or width, f32=f32)
        self._call_hook(self.lib.mvd_op_move, (op, L.ptr(a), L.ptr(b), *ints, L.ptr(out)), [self._bits(out)])
        self._guard_intact(out, rows, width, f"op_move (op {op})")
        return out[:rows, :width].clone()

    def op_fold(self, op, a, b, heads=1, hd=1, Cc=1, I=1, scale=1.0, M=0, N=0, K=0, lda=0, ldb=0, ldc=0, out_f32=True):
        """mvd_op_fold: op 0 (Wq, Wk) -> [heads Cc, I]; 1 (Wo, Wv) -> [I, heads Cc]; 2 a [M, lda], b [K, ldb] -> [M, N] in rows of ldc."""
        a, b = self._dev(a), self._dev(b)
        rows, width, ld = ((heads * Cc, I, I), (I, heads * Cc, heads * Cc), (M, N, ldc or N))[min(max(op, 0), 2)]
        out = self._guarded(max(rows, 1), max(ld, width, 1), f32=out_f32)
        self._call_hook(self.lib.mvd_op_fold, (op, L.ptr(a), L.ptr(b), heads, hd, Cc, I, scale, M, N, K, lda, ldb, ldc, bool(out_f32), L.ptr(out)),
                        [self._bits(out)])
        self._guard_intact(out, rows, width, f"op_fold (op {op})")
        return out[:rows, :width].clone()

    def op_cfg_assemble(self, x_noisy, x_input, clip, timesteps, copies):
        """mvd_op_cfg_assemble: x_noisy [B, TN, 4, HW], x_input [B, 4, HW], clip [B, dim], timesteps (host ints) -> (xin [rows, HW, 8],
        ctx [rows, dim], tt [rows]), rows = copies B TN; results preset to NaN / -1 with a guard behind each."""
        B, TN, _, HW = x_noisy.shape
        dim = clip.shape[1]
        rows = max(copies, 1) * B * TN
        xn, xi, cl = self._dev(x_noisy), self._dev(x_input), self._dev(clip)
        ts = None if timesteps is None else (C.c_int64 * B)(*[int(t) for t in timesteps])
        xin, ctx = _nan_guarded(rows * HW, 8, self.device), _nan_guarded(rows, dim, self.device)
        tt = torch.full((rows + 1,), -1, dtype=torch.int64, device=self.device)
        self._call_hook(self.lib.mvd_op_cfg_assemble, (L.ptr(xn), L.ptr(xi), L.ptr(cl), ts, B, TN, HW, dim, copies, L.ptr(xin), L.ptr(ctx),
                                                       L.ptr(tt)), [xin, ctx, tt.view(torch.int32)])
        _nan_guard_intact(xin, rows * HW, "op_cfg_assemble (xin)")
        _nan_guard_intact(ctx, rows, "op_cfg_assemble (ctx)")
        assert int(tt[rows]) == -1, "op_cfg_assemble: the launch wrote behind the timesteps"
        return xin[:rows * HW].reshape(rows, HW, 8).clone(), ctx[:rows].clone(), tt[:rows].clone()

    def op_cfg_ddim(self, ec, eu, x, noise, k, want_eps=True, want_x=True):
        """mvd_op_cfg_ddim over flat tensors; k: dict(scale, s1m, sqrt_at, sqrt_aprev, dir_coef, sigma) -> (eps or None, x_prev or None)"""
        ec, eu, x, noise = self._dev(ec), self._dev(eu), self._dev(x), self._dev(noise)
        n = 0 if ec is None else ec.numel()
        eb = _nan_guarded(1, max(n, 1), self.device) if want_eps else None
        xb = _nan_guarded(1, max(n, 1), self.device) if want_x else None
        self._call_hook(self.lib.mvd_op_cfg_ddim, (L.ptr(ec), L.ptr(eu), k["scale"], L.ptr(x), L.ptr(noise), k["s1m"], k["sqrt_at"], k["sqrt_aprev"],
                                                   k["dir_coef"], k["sigma"], L.ptr(eb), L.ptr(xb), n), [t for t in (eb, xb) if t is not None])
        for t in (eb, xb):
            if t is not None:
                _nan_guard_intact(t, 1, "op_cfg_ddim")
        return None if eb is None else eb[0].clone(), None if xb is None else xb[0].clone()

    def op_small_mix(self, op, a, b=None, w=None, ints=(), n=0, rows=1, width=1, start=None):
        """mvd_op_small_mix: op 0 fuse_views (ints: n_views, Nv, total_views, accumulate), 1 mse, 2 accumulate_f32 (start += a),
        3 add_rows -> [rows, width]"""
        a, b, w = self._dev(a), self._dev(b), self._dev(w)
        ints = tuple(ints) + (0,) * (4 - len(ints))
        ob, op_, _ = self._rows_out(rows, width, 0, start)
        self._call_hook(self.lib.mvd_op_small_mix, (op, L.ptr(a), L.ptr(b), L.ptr(w), *ints, n, op_), [ob])
        return self._rows_result(ob, rows, width, f"op_small_mix (op {op})")

    # ---- training-backward adjoints of one layer (mvd_op_*_bwd, mvd_op_tgemm): reference layouts in, reference layouts out.
    # accum = (dx0, dW0, db0): the gradients start from these values (otherwise from zero: dx written, dW / db added to zero).
    def _pad_last(self, t, n):
        t = _f32(t, self.device)
        return t if t.shape[-1] == n else torch.nn.functional.pad(t, (0, n - t.shape[-1])).contiguous()

    def op_conv_bwd(self, x, w, dy, kind=0, x_half=False, xp=False, accum=None, need_din=True, poison=False):
        """Conv2d k1 / k3 (kind 0), Downsample (1: stride 2), Upsample (2: nearest x2, then k3) adjoint.  x [B,Cin,H,W], w
        [Cout,Cin,k,k], dy [B,Cout,Ho,Wo] -> (dx [B,Cin,H,W] or None, dW like w, db [Cout])."""
        dev = self.device
        B, Cin, H, W = x.shape
        Cout, k = w.shape[0], w.shape[2]
        cp = (Cin + 7) // 8 * 8
        xn = self._pad_last(x.permute(0, 2, 3, 1), cp)
        dyn = _f32(dy.permute(0, 2, 3, 1), dev)
        ww = _f32(w, dev)
        dx = torch.zeros(B, H, W, cp, device=dev)
        dW = torch.zeros(Cout, Cin * k * k, device=dev)
        db = torch.zeros(Cout, device=dev)
        if accum is not None:
            dx.copy_(self._pad_last(accum[0].permute(0, 2, 3, 1), cp))
            dW.copy_(accum[1].reshape(Cout, -1))
            db.copy_(accum[2])
        L.check(self.lib.mvd_op_conv_bwd(self._ctx, kind, k, B, Cin, H, W, Cout, L.ptr(xn), bool(x_half), L.ptr(ww), L.ptr(dyn),
                                         bool(xp), accum is not None, bool(need_din), bool(poison),
                                         L.ptr(dx), L.ptr(dW), L.ptr(db), _stream()))
        dxo = dx[..., :Cin].permute(0, 3, 1, 2).contiguous() if need_din else None
        return dxo, dW.view_as(w), db

    def op_linear_bwd(self, x, w, dy, B=1, bias=None, x_half=False, geglu=False, dx_half=False, staged=True, xp=False, accum=None,
                      poison=False):
        """Linear adjoint: x [rows,K], w [N,K], dy [rows,N] (geglu: dy = dL/d(value * gelu(gate)) [rows,N/2], bias needed)
        -> (dx [rows,K], dW [N,K], db [N])."""
        dev = self.device
        rows, K = x.shape
        N = w.shape[0]
        kp = (K + 7) // 8 * 8
        xn, dyn, ww = self._pad_last(x, kp), _f32(dy, dev), _f32(w, dev)
        bb = None if bias is None else _f32(bias, dev)
        dx = torch.zeros(rows, kp, device=dev)
        dW = torch.zeros(N, K, device=dev)
        db = torch.zeros(N, device=dev)
        if accum is not None:
            dx.copy_(self._pad_last(accum[0], kp))
            dW.copy_(accum[1])
            db.copy_(accum[2])
        L.check(self.lib.mvd_op_linear_bwd(self._ctx, B, rows, K, N, L.ptr(xn), bool(x_half), L.ptr(ww), L.ptr(bb), L.ptr(dyn),
                                           bool(geglu), bool(dx_half), bool(staged), bool(xp), accum is not None, bool(poison), L.ptr(dx), L.ptr(dW), L.ptr(db), _stream()))
        return dx[:, :K].contiguous(), dW, db

    def op_conv3d_bwd(self, x, w, dy, kind=0, x_half=False, accum=None, poison=False):
        """Conv3d k3 p1 stride 1 (kind 0) / stride 2 (1), ConvTranspose3d(k3, s2, p1, op1) (2) adjoint.  x [B,Cin,D,H,W], w
        [Cout,Cin,3,3,3] (kind 2: [Cin,Cout,3,3,3]), dy on the output grid -> (dx, dW like w, db [Cout])."""
        dev = self.device
        B, Cin, D, H, W = x.shape
        Cout = w.shape[1] if kind == 2 else w.shape[0]
        xn = _f32(x.permute(0, 2, 3, 4, 1), dev)
        dyn = _f32(dy.permute(0, 2, 3, 4, 1), dev)
        ww = _f32(w, dev)
        dx = torch.zeros(B, D, H, W, Cin, device=dev)
        dW = torch.zeros(w.shape, device=dev)
        db = torch.zeros(Cout, device=dev)
        if accum is not None:
            dx.copy_(accum[0].permute(0, 2, 3, 4, 1))
            dW.copy_(accum[1])
            db.copy_(accum[2])
        L.check(self.lib.mvd_op_conv3d_bwd(self._ctx, kind, B, Cin, D, H, W, Cout, L.ptr(xn), bool(x_half), L.ptr(ww), L.ptr(dyn),
                                           accum is not None, bool(poison), L.ptr(dx), L.ptr(dW), L.ptr(db), _stream()))
        return dx.permute(0, 4, 1, 2, 3).contiguous(), dW, db

    def op_tgemm(self, a, b, a_trans=False, b_trans=False, a_half=False, b_half=False, xp=False, out=None, poison=False):
        """op(A) op(B) through the training step's tgemm: a stored [M,K] ([K,M] with a_trans), b stored [K,N] ([N,K] with b_trans).
        out (optional, [M,N]): accumulated into.  Returns the [M,N] result."""
        dev = self.device
        a, b = _f32(a, dev), _f32(b, dev)
        M, K = (a.shape[1], a.shape[0]) if a_trans else a.shape
        N = b.shape[0] if b_trans else b.shape[1]
        o = torch.zeros(M, N, device=dev) if out is None else _f32(out, dev).clone()
        L.check(self.lib.mvd_op_tgemm(self._ctx, M, N, K, L.ptr(a), bool(a_half), bool(a_trans), a.shape[1],
                                      L.ptr(b), bool(b_half), bool(b_trans), b.shape[1], L.ptr(o), N,
                                      out is not None, bool(xp), bool(poison), _stream()))
        return o

    def bench_conv(self, B, Cc, H, W, Cout, iters=20):
        ms = C.c_float(0)
        L.check(self.lib.mvd_bench_conv(self._ctx, B, Cc, H, W, Cout, iters, C.byref(ms), _stream()))
        return ms.value

    def bench_linear(self, M, K, N, resid=False, out_half=False, geglu=False, iters=20, bias=False, rowbias=False, cold=False,
                     a_f32=False):
        ms = C.c_float(0)
        flags = ((1 if resid else 0) | (2 if out_half else 0) | (4 if geglu else 0) | (8 if bias else 0) | (16 if rowbias else 0) |
                 (32 if cold else 0) | (64 if a_f32 else 0))
        L.check(self.lib.mvd_bench_linear(self._ctx, M, K, N, flags, iters, C.byref(ms), _stream()))
        return ms.value

    def bench_group_norm(self, B, Cc, HW, groups=32, split=False, iters=20, apply_only=False):
        ms = C.c_float(0)
        L.check(self.lib.mvd_bench_group_norm(self._ctx, B, Cc, HW, groups, (1 if split else 0) | (2 if apply_only else 0), iters, C.byref(ms),
                                              _stream()))
        return ms.value

    def probe_config(self, mode, family=None, stride=1):
        """mvd_probe_config: 0 off, 1 every launch of every kernel family, 2 a 1-in-stride sample of ``family``."""
        L.check(self.lib.mvd_probe_config(self._ctx, mode, None if family is None else family.encode(), stride))

    def probe_report(self):
        """Per-family table since the last probe_config: list of dicts (family, launches, sampled, ms, flops, bytes, ...)."""
        import json
        buf = C.create_string_buffer(1 << 16)
        L.check(self.lib.mvd_probe_report(self._ctx, buf, len(buf)))
        return json.loads(buf.value.decode())

    def vae_decode(self, z):
        """AutoencoderKL.decode (autoencoder.py:330-333) for a batch of latents z [B,4,h,w] (already divided by the
        first-stage scale factor) -> [B,3,8h,8w]; needs the first_stage_model.decoder.* weights in load_state_dict."""
        if not getattr(self, "has_vae_decoder", False):
            raise L.MvdError("first-stage decoder weights were not part of the uploaded state_dict")
        z = _f32(z, self.device)
        B, _, h, w = z.shape
        out = torch.empty(B, 3, 8 * h, 8 * w, device=self.device)
        # chunks of at most 16 x 256^2 output pixels: the kernels address an operand with 32-bit byte offsets (4 GiB), and the
        # widest decoder activation is 128 channels x 4 bytes per pixel
        per = max(1, (16 * 256 * 256) // (64 * h * w))
        for i in range(0, B, per):
            zc = z[i:i + per].contiguous()
            L.check(self.lib.mvd_vae_decode(self._ctx, L.ptr(zc), zc.shape[0], h, w, L.ptr(out[i:i + per]), _stream()))
        return out

    def clip_encode(self, x):
        """FrozenCLIPImageEmbedder.encode (ldm/modules/encoders/modules.py:363-382): x [B,3,H,W] in [-1,1] ->
        [B,1,embed]; needs the clip_image_encoder.model.visual.* weights in load_state_dict."""
        if not getattr(self, "has_clip", False):
            raise L.MvdError("CLIP vision-tower weights were not part of the uploaded state_dict")
        x = _f32(x, self.device)
        B, ch, H, W = x.shape
        if ch != 3:
            raise ValueError("clip_encode expects [B,3,H,W]")
        out = torch.empty(B, self.lib.mvd_clip_embed_dim(self._ctx), device=self.device)
        L.check(self.lib.mvd_clip_encode(self._ctx, L.ptr(x), B, H, W, L.ptr(out), _stream()))
        return out.unsqueeze(1)

    def vae_encode_moments(self, x):
        """AutoencoderKL.encode(x).parameters (autoencoder.py:324-328): x [B,3,H,W] in [-1,1] -> [B,8,H/8,W/8]
        (mean | logvar); needs the first_stage_model.encoder.* weights in load_state_dict."""
        if not getattr(self, "has_vae_encoder", False):
            raise L.MvdError("first-stage encoder weights were not part of the uploaded state_dict")
        x = _f32(x, self.device)
        B, _, H, W = x.shape
        out = torch.empty(B, 8, H // 8, W // 8, device=self.device)
        L.check(self.lib.mvd_vae_encode(self._ctx, L.ptr(x), B, H, W, L.ptr(out), _stream()))
        return out

"""``python -m morphablediffusion_amd.generate_face`` -- the reference's inference entry script (generate_face.py:90-262) on the
MI355X engine: same flags, same batch construction, same outputs.

  --input_img IMG --exp_img IMG --mesh MESH.{ply,obj} --cfg configs/facescape.yaml --ckpt CKPT --output_dir DIR
  [--cfg_scale 2.0] [--batch_view_num 8] [--seed 6033] [--sampler ddim|dpmpp_2m|dpmpp_2m_sde] [--sample_steps 50]
  [--camera_trajectory virtual|real] [--prepare_neus2_data] [--gt_dir DIR] [--export_mesh] [--mesh_overlay]

writes ``<output_dir>/<input>_<exp>.png`` (the input view followed by the 16 generated views, generate_face.py:244-253) and, with
--prepare_neus2_data, ``<output_dir>/neus2_data/<input>_<exp>/{transform.json, images/00..15.png}`` (:145-192,255-262).

Differences, all outside the denoising path and stated here:
  * the reference runs carvekit's BackgroundRemoval (a third-party segmentation network, generate_face.py:46-69) on the input
    image; it is not part of this repository.  An input with an alpha channel is used as the matte (exactly what the reference
    does with carvekit's RGBA output, process_im :79-88); an input without one is taken to be already on a white background
    (alpha = 1), which is what the reference's demo inputs are after matting;
  * meshes are read by a small PLY / OBJ vertex reader instead of trimesh (``process=False``: vertices as stored);
  * --camera_file names the pickle / JSON of the 'real' trajectory (default: the reference's ./assets/facescape_test_traj.pkl);
  * --exp_img only names the output, as in the reference (the expression enters through the mesh);
  * --gt_dir DIR (not a reference flag) scores the saved strip's 16 views against the captured views in DIR (metrics.py: SSIM,
    PSNR, MSE, MAE under the reference's evaluation protocol) and writes ``<output_dir>/<input>_<exp>_metrics.json``;
  * --export_mesh / --mesh_overlay (not reference flags; mesh.py): the conditioning mesh coloured from the 16 generated views as
    ``<output_dir>/<input>_<exp>_mesh.ply`` with its statistics in ``<input>_<exp>_mesh.json``, and the mesh drawn over the views
    as ``<input>_<exp>_overlay.png`` (a check of the mesh's alignment).  Both need a mesh file with faces.
  * --export_texture [--texture_size 1024] [--uv_mesh FILE.obj] (not reference flags; mesh.py, csrc/k_mesh_uv.hip): a UV texture
    atlas baked from the 16 generated views, as ``<input>_<exp>_textured.obj`` / ``.mtl`` / ``<input>_<exp>_texture.png`` with
    its coverage, consistency and reprojection PSNR / SSIM per view in ``<input>_<exp>_texture.json``.  The texture
    coordinates are --mesh's when it is an OBJ with vt lines, else --uv_mesh's (same vertex and face counts), else one chart
    per triangle (mesh.triangle_atlas).  Works on the --frames path as --export_mesh does.
  * --flame_model MODEL.{npz,pkl} --flame_params PARAMS.npz (not reference flags; morphable.py) replace --mesh: the conditioning
    mesh is computed from FLAME parameters (any of shape, expression, global_pose, neck, jaw, eyes; a leading frame axis gives
    several frames) on the device, the step the reference leaves to MICA's FLAME module, and aligned in the same pass.  With
    --neutral_params NEUTRAL.npz --frames K the K frames sweep from the neutral to the target parameters.  One frame writes
    ``<input>_<exp>.png`` as before, several write ``<input>_<exp>_fNN.png`` each (and the --export_mesh / --mesh_overlay /
    --gt_dir files with the same ``_fNN``); frames are sampled --frame_batch at a time.  With none of these flags the program
    does exactly what it did without them.
  * --flame_model MODEL --fit_scan SCAN.{ply,obj} (not reference flags; mesh.closest_point, csrc/k_closest.hip) does the same
    against a scan of any topology, with --fit_scan_max_dist / _normal_cos / _refresh / _landmarks.
  * --flame_model MODEL --fit_landmarks2d LMK.npz (not a reference flag; MorphableModel.fit_flame_2d, csrc/k_morph_2d.hip) does
    the same against 2-D key points in calibrated views: the file holds landmarks [C,M,2] or [F,C,M,2] in pixels, K [C,3,3], RT
    [C,3,4] and optionally weights and image_size; the .json reports reprojection_px per view.  It excludes --fit_mesh / --fit_scan.
  * --flame_model MODEL --fit_mesh MESH.{ply,obj} (not reference flags; morphable.py, csrc/k_morph_bwd.hip) fit the model's
    parameters to a mesh of the model's topology, in the model's frame (what metrical-tracker exports), with Adam on the device
    (--fit_iters, --fit_lr), and write ``<input>_<exp>_fit.npz`` (shape, expression, global_pose, neck, jaw, eyes, transl) and
    ``<input>_<exp>_fit.json`` (RMS residual, iterations).  Alone, the fitted mesh conditions the views.  With --flame_params
    the fit takes the place of --neutral_params: the --frames K frames sweep from the fit to the fitted identity, global pose
    and translation combined with the given expression and jaw (and neck / eyes when given).
"""
import argparse
import json
import os
import pickle
import struct
from pathlib import Path

import numpy as np
import torch

from . import batch as B

NUM_VIEWS = 16  # hard-wired in the reference (generate_face.py:141,156,256)


def read_ply_header(f, path):
    """The header of a PLY file opened in binary mode, leaving ``f`` at the first byte of the data: (format, elements) with
    elements = [(name, count, properties)] in file order and a property (name, type), or (name, "list", count type, item type)."""
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: truncated PLY header")
        t = line.decode("ascii", "replace").split()
        if not t:
            continue
        if t[0] == "format":
            fmt = t[1]
        elif t[0] == "element":
            elements.append((t[1], int(t[2]), []))
        elif t[0] == "property" and elements:
            elements[-1][2].append((t[4], "list", t[2], t[3]) if t[1] == "list" else (t[2], t[1]))
        elif t[0] == "end_header":
            return fmt, elements


def read_mesh_vertices(path) -> np.ndarray:
    """Vertex positions [Nv,3] (float64) of a Wavefront OBJ or a PLY file (ascii, binary little / big endian), in file order --
    what ``trimesh.load(path, process=False).vertices`` returns (generate_face.py:200)."""
    path = str(path)
    if path.lower().endswith(".obj"):
        vs = []
        with open(path) as f:
            for line in f:
                if line.startswith("v "):
                    p = line.split()
                    vs.append([float(p[1]), float(p[2]), float(p[3])])
        if not vs:
            raise ValueError(f"{path}: no vertices")
        return np.asarray(vs, dtype=np.float64)
    if not path.lower().endswith(".ply"):
        raise ValueError(f"{path}: expected a .ply or .obj mesh")
    with open(path, "rb") as f:
        fmt, elements = read_ply_header(f, path)
        nverts, props = 0, []
        for name, count, eprops in elements:
            if name == "vertex":
                nverts, props = count, eprops
        if any(p[1] == "list" for p in props):
            raise ValueError(f"{path}: list property on vertices is not supported")
        names = [p[0] for p in props]
        if not all(a in names for a in "xyz"):
            raise ValueError(f"{path}: vertex element has no x/y/z")
        if fmt == "ascii":
            out = np.empty((nverts, 3))
            ix = [names.index(a) for a in "xyz"]
            for i in range(nverts):
                p = f.readline().split()
                out[i] = [float(p[j]) for j in ix]
            return out
        codes = {"char": "b", "int8": "b", "uchar": "B", "uint8": "B", "short": "h", "int16": "h", "ushort": "H", "uint16": "H",
                 "int": "i", "int32": "i", "uint": "I", "uint32": "I", "float": "f", "float32": "f", "double": "d", "float64": "d"}
        end = "<" if fmt == "binary_little_endian" else ">"
        rec = struct.Struct(end + "".join(codes[p[1]] for p in props))
        raw = f.read(rec.size * nverts)
        if len(raw) != rec.size * nverts:
            raise ValueError(f"{path}: truncated vertex data")
        ix = [names.index(a) for a in "xyz"]
        return np.asarray([[r[j] for j in ix] for r in rec.iter_unpack(raw)], dtype=np.float64)


def load_input_image(path, size=256) -> torch.Tensor:
    """generate_face.py:117-123 + process_im (:79-88): RGBA -> white background, bicubic resize to size x size, [-1,1], HWC."""
    from PIL import Image
    im = Image.open(path)
    rgba = np.asarray(im.convert("RGBA")).astype(np.float32) / 255.0
    mask = rgba[:, :, 3:]
    rgb = rgba[:, :, :3] * mask + 1 - mask
    im = Image.fromarray(np.uint8(rgb * 255.0)).convert("RGB").resize((size, size), resample=Image.BICUBIC)
    return torch.from_numpy(np.asarray(im).astype(np.float32) / 255.0) * 2.0 - 1.0


def load_camera_dict(path):
    if str(path).lower().endswith(".json"):
        with open(path) as f:
            return json.load(f)
    with open(path, "rb") as f:
        return pickle.load(f)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--input_img", type=str, required=True)
    p.add_argument("--exp_img", type=str, required=True)
    p.add_argument("--mesh", type=str, default=None, help="required unless --flame_model / --flame_params are given")
    p.add_argument("--cfg", type=str, default="configs/facescape.yaml")
    p.add_argument("--ckpt", type=str, default="ckpt/facescape_flame.ckpt")
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--cfg_scale", type=float, default=2.0)
    p.add_argument("--batch_view_num", type=int, default=8)
    p.add_argument("--seed", type=int, default=6033)
    p.add_argument("--sampler", type=str, default="ddim", choices=["ddim", "dpmpp_2m", "dpmpp_2m_sde"],
                   help="ddim: the reference's sampler; dpmpp_2m / dpmpp_2m_sde: DPM-Solver++(2M) on the logSNR grid (not reference)")
    p.add_argument("--sample_steps", type=int, default=50)
    p.add_argument("--camera_trajectory", type=str, default="virtual", choices=["real", "virtual"])
    p.add_argument("--prepare_neus2_data", action="store_true")
    p.add_argument("--camera_file", type=str, default="./assets/facescape_test_traj.pkl",
                   help="not a reference flag: the camera dict of --camera_trajectory real (the reference hard-codes this path)")
    p.add_argument("--device", type=str, default="cuda:0", help="not a reference flag")
    p.add_argument("--lora", type=str, default=None,
                   help="not a reference flag: a LoRA adapter file (save_lora), merged into the checkpoint's weights at load time")
    p.add_argument("--lora_scale", type=float, default=1.0, help="not a reference flag: strength of --lora (0: the base model)")
    p.add_argument("--gt_dir", type=str, default=None,
                   help="not a reference flag: a folder with the 16 captured views (sorted *.png, 256 x 256; RGBA: alpha 0 is "
                        "background); the saved strip's views are scored against them into <output_dir>/<img>_<exp>_metrics.json")
    p.add_argument("--export_mesh", action="store_true",
                   help="not a reference flag: write <output_dir>/<img>_<exp>_mesh.ply (the mesh file's vertices and faces with "
                        "colours fused from the generated views) and <img>_<exp>_mesh.json (coverage, consistency, visible counts)")
    p.add_argument("--mesh_overlay", action="store_true",
                   help="not a reference flag: write <output_dir>/<img>_<exp>_overlay.png, the mesh drawn over the generated views")
    p.add_argument("--export_texture", action="store_true",
                   help="not a reference flag: write <output_dir>/<img>_<exp>_textured.obj / .mtl, <img>_<exp>_texture.png (a UV "
                        "texture atlas baked from the generated views) and <img>_<exp>_texture.json (coverage, consistency, "
                        "reprojection PSNR / SSIM per view)")
    p.add_argument("--texture_size", type=int, default=1024, help="not a reference flag: texels on a side of --export_texture's atlas")
    p.add_argument("--uv_mesh", type=str, default=None,
                   help="not a reference flag: an OBJ with vt lines and the mesh's vertex and face counts, whose texture coordinates "
                        "--export_texture uses when --mesh has none (default: one chart per triangle, mesh.triangle_atlas)")
    p.add_argument("--flame_model", type=str, default=None,
                   help="not a reference flag: a FLAME model file (.npz or .pkl with the FLAME pickle's key names); with "
                        "--flame_params the mesh is computed from parameters instead of read from --mesh")
    p.add_argument("--flame_params", type=str, default=None,
                   help="not a reference flag: an .npz with any of shape, expression, global_pose, neck, jaw, eyes (a leading "
                        "frame axis is allowed)")
    p.add_argument("--neutral_params", type=str, default=None,
                   help="not a reference flag: an .npz like --flame_params; with --frames K the frames sweep from it to --flame_params")
    p.add_argument("--frames", type=int, default=1, help="not a reference flag: frames of the sweep (needs --neutral_params)")
    p.add_argument("--frame_batch", type=int, default=1, help="not a reference flag: frames sampled in one batch")
    p.add_argument("--fit_mesh", type=str, default=None,
                   help="not a reference flag: a mesh file of the model's topology; --flame_model's parameters are fitted to it")
    p.add_argument("--fit_iters", type=int, default=300, help="not a reference flag: Adam iterations of --fit_mesh")
    p.add_argument("--fit_lr", type=float, default=0.05, help="not a reference flag: Adam's learning rate for --fit_mesh")
    p.add_argument("--fit_scan", type=str, default=None,
                   help="not a reference flag: a scan of ANY topology (.ply / .obj; no faces: a point cloud); --flame_model's "
                        "parameters are fitted to it through closest points (--fit_iters, --fit_lr apply)")
    p.add_argument("--fit_scan_max_dist", type=float, default=None,
                   help="not a reference flag: --fit_scan ignores correspondences farther than this (the scan's units)")
    p.add_argument("--fit_scan_normal_cos", type=float, default=None,
                   help="not a reference flag: --fit_scan admits only scan faces whose normal makes at least this cosine with the "
                        "model vertex's")
    p.add_argument("--fit_scan_refresh", type=int, default=1,
                   help="not a reference flag: --fit_scan looks for closest points every this many iterations")
    p.add_argument("--fit_scan_landmarks", type=str, default=None,
                   help="not a reference flag: an .npz with `landmarks` [M,3], the scan's 3-D landmarks in the order of the model's "
                        "embedding: a landmark-only fit of global pose and translation seeds --fit_scan, and the term stays on")
    p.add_argument("--fit_landmarks2d", type=str, default=None,
                   help="not a reference flag: an .npz with `landmarks` [C,M,2] or [F,C,M,2] (pixels; M = the model's static landmarks, "
                        "or 68 in iBUG order for a model with 51 + 17), `K` [C,3,3], `RT` [C,3,4] and optionally `weights` [C,M] and "
                        "`image_size` (H, W): --flame_model's parameters are fitted to the key points in these calibrated views "
                        "(--fit_iters, --fit_lr apply)")
    p.add_argument("--flame_n_shape", type=int, default=None,
                   help="not a reference flag: identity columns of the model's shapedirs to keep (MICA: 300; default: all)")
    p.add_argument("--flame_n_exp", type=int, default=None,
                   help="not a reference flag: expression columns (from column 300 on) to keep (MICA: 100; default: all)")
    return p


FLAME_PARAM_KEYS = ("shape", "expression", "global_pose", "neck", "jaw", "eyes")
FLAME_FILE_KEYS = FLAME_PARAM_KEYS + ("transl",)  # what a parameter file may hold: MorphableModel.flame's arguments


def parse_args(argv=None):
    """build_parser().parse_args plus the rules between the flags: --mesh alone as ever; --flame_model and --flame_params go
    together and replace --mesh; --neutral_params and --frames > 1 go together and need them; --fit_mesh needs --flame_model,
    excludes --mesh and --neutral_params, and with --flame_params takes the place of the neutral end; --fit_scan follows
    --fit_mesh's rules and excludes it; --fit_landmarks2d follows them too and excludes both."""
    p = build_parser()
    flags = p.parse_args(argv)
    scan_only = [n for n in ("fit_scan_max_dist", "fit_scan_normal_cos", "fit_scan_landmarks") if getattr(flags, n) is not None]
    if (scan_only or flags.fit_scan_refresh != 1) and not flags.fit_scan:
        p.error("--fit_scan_max_dist, --fit_scan_normal_cos, --fit_scan_refresh and --fit_scan_landmarks need --fit_scan")
    if flags.fit_scan and flags.fit_mesh:
        p.error("--fit_scan excludes --fit_mesh (one target)")
    if flags.fit_landmarks2d and (flags.fit_mesh or flags.fit_scan):
        p.error("--fit_landmarks2d excludes --fit_mesh and --fit_scan (one target)")
    if flags.fit_scan:
        if flags.fit_scan_max_dist is not None and not flags.fit_scan_max_dist > 0:
            p.error("--fit_scan_max_dist must be positive")
        if flags.fit_scan_normal_cos is not None and not -1.0 <= flags.fit_scan_normal_cos <= 1.0:
            p.error("--fit_scan_normal_cos must be in [-1, 1]")
        if flags.fit_scan_refresh < 1:
            p.error("--fit_scan_refresh must be at least 1")
    if flags.fit_mesh or flags.fit_scan or flags.fit_landmarks2d:
        name = "--fit_mesh" if flags.fit_mesh else ("--fit_scan" if flags.fit_scan else "--fit_landmarks2d")
        if not flags.flame_model:
            p.error(f"{name} needs --flame_model")
        if flags.mesh or flags.neutral_params:
            p.error(f"{name} excludes --mesh and --neutral_params (the fit is the neutral end)")
        if flags.fit_iters < 1 or not flags.fit_lr > 0:
            p.error("--fit_iters must be at least 1 and --fit_lr positive")
        if flags.frames < 1 or flags.frame_batch < 1:
            p.error("--frames and --frame_batch must be at least 1")
        if flags.frames > 1 and not flags.flame_params:
            p.error(f"--frames K > 1 with {name} needs --flame_params (the other end of the sweep)")
        return flags
    flame = [flags.flame_model, flags.flame_params]
    if not any(flame) and (flags.neutral_params or flags.frames != 1 or flags.frame_batch != 1):
        p.error("--neutral_params, --frames and --frame_batch need --flame_model and --flame_params")
    if any(flame):
        if not all(flame):
            p.error("--flame_model and --flame_params go together")
        if flags.mesh:
            p.error("give either --mesh or --flame_model / --flame_params, not both")
        if flags.frames < 1 or flags.frame_batch < 1:
            p.error("--frames and --frame_batch must be at least 1")
        if (flags.frames > 1) != bool(flags.neutral_params):
            p.error("--neutral_params and --frames K > 1 go together")
    elif not flags.mesh:
        p.error("the following arguments are required: --mesh (or --flame_model and --flame_params)")
    return flags


def load_flame_params(path):
    """{key: float64 array} of the FLAME_FILE_KEYS an .npz holds; any other key is an error (a misspelt name would be zeros)."""
    with np.load(path, allow_pickle=False) as z:
        unknown = [k for k in z.files if k not in FLAME_FILE_KEYS]
        if unknown:
            raise ValueError(f"{path}: unknown parameter names {unknown}; known: {list(FLAME_FILE_KEYS)}")
        return {k: np.asarray(z[k], dtype=np.float64) for k in z.files}


def fit_to_mesh(fm, flags, stem):
    """--fit_mesh: the model's parameters fitted to the mesh file (same topology, the model's frame: no post).  Writes
    <stem>_fit.npz and <stem>_fit.json; returns {key: float64 vector} over FLAME_FILE_KEYS."""
    target = read_mesh_vertices(flags.fit_mesh)
    if target.shape[0] != fm.V:
        raise ValueError(f"{flags.fit_mesh}: the mesh has {target.shape[0]} vertices, the model {fm.V}: fitting needs the model's topology")
    fit = fm.fit_flame(target_vertices=torch.from_numpy(target)[None], iters=flags.fit_iters, lr=flags.fit_lr)
    params = {k: fit[k][0].cpu().numpy().astype(np.float64) for k in FLAME_FILE_KEYS}
    np.savez(f"{stem}_fit.npz", **params)
    with open(f"{stem}_fit.json", "w") as f:
        json.dump({"mesh": str(flags.fit_mesh), "vertices": int(fm.V), "iterations": int(flags.fit_iters), "lr": float(flags.fit_lr),
                   "rms": float(fit["rms"][0]), "loss_first": float(fit["loss_history"][0, 0]),
                   "loss_last": float(fit["loss_history"][-1, 0])}, f, indent=2)
    return params


def fit_to_scan(fm, flags, stem):
    """--fit_scan: the model's parameters fitted to a scan of any topology in the model's frame (MorphableModel.fit_flame_scan).
    With --fit_scan_landmarks a landmark-only fit of global pose and translation comes first and seeds the start.  Writes
    <stem>_fit.npz and <stem>_fit.json (iterations, matched share, model-to-scan rms, scan-to-mesh statistics); returns {key:
    float64 vector} over FLAME_FILE_KEYS."""
    from . import mesh as MS
    sv, sf = MS.read_mesh(flags.fit_scan)
    sf = sf if sf is not None and len(sf) else None
    init, tl = None, None
    if flags.fit_scan_landmarks:
        with np.load(flags.fit_scan_landmarks, allow_pickle=False) as z:
            if "landmarks" not in z.files:
                raise ValueError(f"{flags.fit_scan_landmarks}: no array named 'landmarks'")
            tl = torch.from_numpy(np.asarray(z["landmarks"], dtype=np.float32))[None]
        rigid = fm.fit_flame(target_landmarks=tl, free=("global_pose", "transl"), iters=flags.fit_iters, lr=flags.fit_lr)
        init = {"global_pose": rigid["global_pose"].cpu().numpy(), "transl": rigid["transl"].cpu().numpy()}
    fit = fm.fit_flame_scan(torch.from_numpy(sv), None if sf is None else torch.from_numpy(sf), target_landmarks=tl, init=init,
                            max_dist=flags.fit_scan_max_dist, normal_cos=flags.fit_scan_normal_cos, refresh=flags.fit_scan_refresh,
                            iters=flags.fit_iters, lr=flags.fit_lr)
    params = {k: fit[k][0].cpu().numpy().astype(np.float64) for k in FLAME_FILE_KEYS}
    np.savez(f"{stem}_fit.npz", **params)
    report = {"scan": str(flags.fit_scan), "scan_vertices": int(sv.shape[0]), "scan_faces": 0 if sf is None else int(sf.shape[0]),
              "vertices": int(fm.V), "iterations": int(flags.fit_iters), "lr": float(flags.fit_lr), "refresh": int(flags.fit_scan_refresh),
              "matched": float(fit["matched"][0]) / fm.V, "rms": float(fit["rms"][0]), "loss_first": float(fit["loss_history"][0, 0]),
              "loss_last": float(fit["loss_history"][-1, 0])}
    if fm.faces is not None:  # the standard 3-D error: every scan vertex against the fitted surface
        s2m = MS.surface_distance(sv, fit["vertices"][0], fm.faces, max_dist=flags.fit_scan_max_dist)
        report["scan_to_mesh"] = {k: s2m[k] for k in ("mean", "rms", "median", "p90", "max", "matched")}
    with open(f"{stem}_fit.json", "w") as f:
        json.dump(report, f, indent=2)
    return params


def fit_to_landmarks2d(fm, flags, stem):
    """--fit_landmarks2d: the model's parameters fitted to 2-D key points in calibrated views (MorphableModel.fit_flame_2d; 68
    points are taken in iBUG order).  A file with a frame axis is fitted frame by frame and frame 0 is what the run uses.  Writes
    <stem>_fit.npz and <stem>_fit.json (iterations, counted observations, reprojection_px per view); returns {key: float64 vector}
    over FLAME_FILE_KEYS."""
    with np.load(flags.fit_landmarks2d, allow_pickle=False) as z:
        missing = [k for k in ("landmarks", "K", "RT") if k not in z.files]
        if missing:
            raise ValueError(f"{flags.fit_landmarks2d}: missing {missing}")
        d = {k: np.asarray(z[k]) for k in ("landmarks", "K", "RT", "weights", "image_size") if k in z.files}
    lm = d["landmarks"]
    if lm.ndim not in (3, 4) or lm.shape[-1] != 2:
        raise ValueError(f"{flags.fit_landmarks2d}: landmarks must be [C,M,2] or [F,C,M,2], got {lm.shape}")
    order = "ibug68" if lm.shape[-2] == 68 and fm.lmk_face is not None and fm.lmk_face.shape[0] != 68 else None
    fit = fm.fit_flame_2d(lm.astype(np.float32), d["K"].astype(np.float32), d["RT"].astype(np.float32),
                          weights=None if "weights" not in d else d["weights"].astype(np.float32), image_size=d.get("image_size"),
                          landmark_order=order, iters=flags.fit_iters, lr=flags.fit_lr)
    params = {k: fit[k][0].cpu().numpy().astype(np.float64) for k in FLAME_FILE_KEYS}
    np.savez(f"{stem}_fit.npz", **params)
    with open(f"{stem}_fit.json", "w") as f:
        json.dump({"landmarks2d": str(flags.fit_landmarks2d), "views": int(lm.shape[-3]), "points": int(lm.shape[-2]),
                   "frames": int(fit["betas"].shape[0]), "iterations": int(flags.fit_iters), "lr": float(flags.fit_lr),
                   "observations": int(fit["n_valid"][0]), "reprojection_px": [float(x) for x in fit["reprojection_px"][0]],
                   "rms": float(fit["rms"][0]), "loss_first": float(fit["loss_history"][0, 0]),
                   "loss_last": float(fit["loss_history"][-1, 0])}, f, indent=2)
    return params


def flame_frames(flags, device, stem=None):
    """The conditioning meshes of --flame_model with --flame_params and / or --fit_mesh: (verts [F,Nv,3] on the device in the
    frame of batch["vertices"], model-frame vertices [F,Nv,3] as a mesh file would store them, faces [Nf,3] or None).  stem:
    where --fit_mesh writes its files (<stem>_fit.npz / .json)."""
    from . import morphable as MM
    fm = MM.MorphableModel.load(flags.flame_model, n_shape=flags.flame_n_shape, n_exp=flags.flame_n_exp, device=device)
    if getattr(flags, "fit_mesh", None) or getattr(flags, "fit_scan", None) or getattr(flags, "fit_landmarks2d", None):
        params = fit_to_mesh(fm, flags, stem) if getattr(flags, "fit_mesh", None) else (
            fit_to_scan(fm, flags, stem) if getattr(flags, "fit_scan", None) else fit_to_landmarks2d(fm, flags, stem))
        if flags.flame_params:
            given = load_flame_params(flags.flame_params)
            if any(v.ndim > 1 for v in given.values()):
                raise ValueError(f"{flags.flame_params}: a sweep goes to ONE target, parameters with a frame axis cannot be swept to")
            # the fitted identity, global pose and translation with the given expression and jaw (neck, eyes when given)
            end = dict(params, expression=given.get("expression", np.zeros_like(params["expression"])),
                       jaw=given.get("jaw", np.zeros(3)), **{k: given[k] for k in ("neck", "eyes") if k in given})
            params = MM.interpolate_params(params, end, flags.frames)
        verts = fm.flame(post=MM.flame_alignment(), **params)["vertices"]
        stored = fm.flame(**params)["vertices"]
        return verts, stored.cpu().numpy().astype(np.float64), None if fm.faces is None else fm.faces.cpu().numpy()
    params = load_flame_params(flags.flame_params)
    if flags.neutral_params:
        if any(v.ndim > 1 for v in params.values()):
            raise ValueError(f"{flags.flame_params}: a sweep goes to ONE target, parameters with a frame axis cannot be swept to")
        params = MM.interpolate_params(load_flame_params(flags.neutral_params), params, flags.frames)
    if "shape" not in params:
        params["shape"] = np.zeros(fm.n_shape)
    verts = fm.flame(post=MM.flame_alignment(), **params)["vertices"]
    stored = fm.flame(**params)["vertices"]
    return verts, stored.cpu().numpy().astype(np.float64), None if fm.faces is None else fm.faces.cpu().numpy()


def mesh_outputs(x_sample, cams, verts, faces, file_verts, output_dir, stem, export_mesh=False, mesh_overlay=False, **kw):
    """The post-sampling work of --export_mesh / --mesh_overlay: x_sample [N,3,H,W] (or [B,N,3,H,W]: sample 0) in [-1, 1], cams
    (K [N,4,4] or [N,3,3], RT [N,3,4]), verts [Nv,3] in the frame of batch["vertices"], faces [Nf,3], file_verts [Nv,3] as the
    mesh file stores them (what the PLY holds).  Writes <output_dir>/<stem>_mesh.ply and <stem>_mesh.json with export_mesh,
    <stem>_overlay.png with mesh_overlay, nothing without either; kw goes to mesh.texture_mesh.  Returns the paths written."""
    written = {}
    if not (export_mesh or mesh_overlay):
        return written
    from . import mesh as MS
    x = x_sample[0] if x_sample.dim() == 5 else x_sample
    K, RT = cams
    tex = MS.texture_mesh(x, verts, faces, K, RT, **kw)
    out = Path(output_dir)
    if export_mesh:
        written["ply"] = str(out / f"{stem}_mesh.ply")
        MS.write_ply(written["ply"], np.asarray(file_verts), faces, tex["colors"])
        written["json"] = str(out / f"{stem}_mesh.json")
        with open(written["json"], "w") as f:
            json.dump({"vertices": int(tex["colors"].shape[0]), "faces": int(len(faces)), "coverage": tex["coverage"],
                       "consistency": None if np.isnan(tex["consistency"]) else tex["consistency"], "visible_per_view": tex["visible"].sum(1).tolist(),
                       "seen_in_two_or_more_views": int((tex["n_seen"] >= 2).sum())}, f, indent=2)
    if mesh_overlay:
        from PIL import Image
        written["overlay"] = str(out / f"{stem}_overlay.png")
        Image.fromarray(MS.overlay_views(x, tex["mask"], tex["face_id"]).cpu().numpy()).save(written["overlay"])
    return written


def texture_coordinates(mesh_path, uv_mesh, n_verts, faces, size):
    """The texture coordinates of --export_texture, (uv [Nt,2], face_uv [Nf,3]): of ``mesh_path`` when it is an OBJ with vt lines,
    else of ``uv_mesh`` (an OBJ with vt and the same vertex and face counts, or ValueError), else mesh.triangle_atlas."""
    from . import mesh as MS
    if mesh_path and str(mesh_path).lower().endswith(".obj"):
        with open(mesh_path) as f:
            if any(line.startswith("vt ") for line in f):
                _, f2, uv, face_uv = MS.read_mesh_uv(mesh_path)
                if len(f2) != len(faces):
                    raise ValueError(f"{mesh_path}: {len(f2)} faces with texture coordinates, the mesh has {len(faces)}")
                return uv, face_uv
    if uv_mesh:
        v2, f2, uv, face_uv = MS.read_mesh_uv(uv_mesh)
        if len(v2) != n_verts or len(f2) != len(faces):
            raise ValueError(f"{uv_mesh}: {len(v2)} vertices and {len(f2)} faces, the mesh has {n_verts} and {len(faces)}")
        return uv, face_uv
    return MS.triangle_atlas(len(faces), size, size)


def texture_outputs(x_sample, cams, verts, faces, file_verts, uv, face_uv, output_dir, stem, export_texture=False, size=1024, **kw):
    """The post-sampling work of --export_texture: x_sample [N,3,H,W] (or [B,N,3,H,W]: sample 0) in [-1, 1], cams, verts, faces,
    file_verts as mesh_outputs takes them, uv [Nt,2] / face_uv [Nf,3] (texture_coordinates).  Writes <output_dir>/
    <stem>_textured.obj and .mtl, <stem>_texture.png and <stem>_texture.json (coverage, consistency, the reprojection PSNR /
    SSIM of the atlas rendered back into every view); nothing without the flag; kw goes to mesh.bake_texture.  Returns the
    paths written."""
    if not export_texture:
        return {}
    from . import mesh as MS
    from . import metrics as M
    x = x_sample[0] if x_sample.dim() == 5 else x_sample
    K, RT = cams
    bake = MS.bake_texture(x, verts, faces, uv, face_uv, K, RT, size=size, **kw)
    rep = MS.reprojection_metrics(x, bake, verts, faces, uv, face_uv, K, RT)
    out = Path(output_dir)
    written = MS.write_obj(str(out / f"{stem}_textured.obj"), np.asarray(file_verts), faces, uv, face_uv, bake["texture"],
                           texture_name=f"{stem}_texture.png")
    written["json"] = str(out / f"{stem}_texture.json")
    with open(written["json"], "w") as f:
        json.dump(dict(M.summarise(rep, keys=("psnr", "ssim")), vertices=int(len(file_verts)), faces=int(len(faces)),
                       texture_coordinates=int(len(uv)), size=[int(bake["texture"].shape[0]), int(bake["texture"].shape[1])],
                       coverage=bake["coverage"], consistency=None if np.isnan(bake["consistency"]) else bake["consistency"],
                       valid_after_dilation=float(bake["valid"].double().mean())), f, indent=2)
    return written


def load_model(cfg, ckpt, device="cuda:0", lora=None, lora_scale=1.0, **overrides):
    """batch.load_model: the reference's ``load_model`` plus ``lora`` / ``lora_scale`` (an adapter file merged at load time)."""
    return B.load_model(cfg, ckpt, device=device, lora=lora, lora_scale=lora_scale, **overrides)


def run(flags, model=None):
    """The body of generate_face.py:main (:107-262).  ``model``: an already loaded SyncMultiviewDiffusion (tests); default:
    batch.load_model(flags.cfg, flags.ckpt).  Returns (strip uint8 [256, 17*256, 3], output path)."""
    from PIL import Image
    from .model import SyncDDIMSampler, SyncDPMSolverSampler, SyncMultiviewDiffusion
    img_name = flags.input_img.split("/")[-1].split(".")[0]
    exp_name = flags.exp_img.split("/")[-1].split(".")[0]
    torch.random.manual_seed(flags.seed)
    input_img = load_input_image(flags.input_img)
    if model is None:
        model = load_model(flags.cfg, flags.ckpt, device=flags.device, lora=getattr(flags, "lora", None),
                           lora_scale=getattr(flags, "lora_scale", 1.0))
    assert isinstance(model, SyncMultiviewDiffusion)
    Path(flags.output_dir).mkdir(exist_ok=True, parents=True)
    if flags.sampler == "ddim":
        sampler = SyncDDIMSampler(model, flags.sample_steps, latent_size=model.image_size // 8)
    elif flags.sampler in ("dpmpp_2m", "dpmpp_2m_sde"):
        sampler = SyncDPMSolverSampler(model, flags.sample_steps, flags.sampler, latent_size=model.image_size // 8)
    else:
        raise NotImplementedError(flags.sampler)
    if flags.camera_trajectory == "real":
        cams = B.cameras_from_dict(load_camera_dict(flags.camera_file), NUM_VIEWS)
    else:
        cams = B.virtual_cameras(NUM_VIEWS, 256)
    want_mesh = getattr(flags, "export_mesh", False) or getattr(flags, "mesh_overlay", False)
    want_tex = getattr(flags, "export_texture", False)
    if getattr(flags, "flame_model", None):
        return run_flame(flags, model, sampler, cams, input_img, img_name, exp_name, want_mesh)
    faces = None
    if want_mesh or want_tex:
        from .mesh import read_mesh
        file_verts, faces = read_mesh(flags.mesh)
        if not len(faces):
            raise ValueError(f"{flags.mesh}: --export_mesh / --mesh_overlay / --export_texture need a mesh with faces")
        if want_tex:
            uv, face_uv = texture_coordinates(flags.mesh, getattr(flags, "uv_mesh", None), len(file_verts), faces,
                                              getattr(flags, "texture_size", 1024))
    else:
        file_verts = read_mesh_vertices(flags.mesh)
    verts = B.align_flame_vertices(torch.from_numpy(file_verts).float())
    data = B.build_batch(input_img, verts, num_views=NUM_VIEWS, image_size=256, device=model.device, cameras=cams)
    neus2_root = None
    if flags.prepare_neus2_data:
        neus2_root = os.path.join(flags.output_dir, "neus2_data", f"{img_name}_{exp_name}")
        os.makedirs(os.path.join(neus2_root, "images"), exist_ok=True)
        with open(os.path.join(neus2_root, "transform.json"), "w") as f:
            json.dump(B.neus2_transform(cams[0], cams[1], 256), f, indent=4)
    x_sample = model.sample(sampler, data, flags.cfg_scale, flags.batch_view_num)
    strip = B.views_to_uint8(x_sample, data["input_image"])
    output_fn = Path(flags.output_dir) / f"{img_name}_{exp_name}.png"
    Image.fromarray(strip).save(output_fn)
    if getattr(flags, "gt_dir", None):
        # scored from the strip's bytes, which are what the reference's evaluation reads back from the saved file
        from . import metrics as M
        gt, gt_mask = M.load_target_views(flags.gt_dir, NUM_VIEWS, 256)
        res = M.summarise(M.image_metrics(M.strip_to_views(strip, NUM_VIEWS, 256)[0].to(model.device), gt, gt_mask))
        with open(Path(flags.output_dir) / f"{img_name}_{exp_name}_metrics.json", "w") as f:
            json.dump(dict(res, sampler=flags.sampler, sample_steps=flags.sample_steps), f, indent=2)
    if want_mesh:
        mesh_outputs(x_sample, cams, verts, faces, file_verts, flags.output_dir, f"{img_name}_{exp_name}",
                     export_mesh=getattr(flags, "export_mesh", False), mesh_overlay=getattr(flags, "mesh_overlay", False))
    if want_tex:
        texture_outputs(x_sample, cams, verts, faces, file_verts, uv, face_uv, flags.output_dir, f"{img_name}_{exp_name}",
                        export_texture=True, size=getattr(flags, "texture_size", 1024))
    if neus2_root:
        # generate_face.py:255-262 slices idx*256 of the strip for idx in range(16): view 0 of the export is the INPUT view and
        # the last generated view is dropped -- reproduced as is
        for idx in range(NUM_VIEWS):
            bgra = B.neus2_view_bgra(strip, idx, 256)
            rgba = np.concatenate([bgra[:, :, 2::-1], bgra[:, :, 3:]], -1).astype(np.uint8)  # cv2.imwrite(BGRA) == PNG(RGBA)
            Image.fromarray(rgba, "RGBA").save(os.path.join(neus2_root, f"images/{str(idx).zfill(2)}.png"))
    return strip, str(output_fn)


def run_flame(flags, model, sampler, cams, input_img, img_name, exp_name, want_mesh):
    """run() with the mesh computed from FLAME parameters: every frame is one sample of a batch (frames_to_batch), sampled
    --frame_batch at a time; returns (strip of the LAST frame, its path).  --prepare_neus2_data is a single-mesh export and is
    refused for more than one frame."""
    from PIL import Image
    from . import morphable as MM
    verts, stored, faces = flame_frames(flags, model.device, stem=str(Path(flags.output_dir) / f"{img_name}_{exp_name}"))
    F = verts.shape[0]
    want_tex = getattr(flags, "export_texture", False)
    if (want_mesh or want_tex) and faces is None:
        raise ValueError(f"{flags.flame_model}: --export_mesh / --mesh_overlay / --export_texture need a model file with faces ('f')")
    if want_tex:
        uv, face_uv = texture_coordinates(None, getattr(flags, "uv_mesh", None), verts.shape[1], faces, getattr(flags, "texture_size", 1024))
        from .mesh import face_incidence
        incidence = face_incidence(faces, verts.shape[1])  # one topology for every frame: the table is built once
    if flags.prepare_neus2_data and F > 1:
        raise ValueError("--prepare_neus2_data exports one mesh's views: run it with a single frame")
    strip, output_fn = None, None
    for f0 in range(0, F, flags.frame_batch):
        chunk = verts[f0:f0 + flags.frame_batch]
        data = MM.frames_to_batch(input_img, chunk, num_views=NUM_VIEWS, image_size=256, device=model.device, cameras=cams)
        x_sample = model.sample(sampler, data, flags.cfg_scale, flags.batch_view_num)
        for i in range(chunk.shape[0]):
            f = f0 + i
            stem = f"{img_name}_{exp_name}" + (f"_f{f:02d}" if F > 1 else "")
            strip = B.views_to_uint8(x_sample[i:i + 1], data["input_image"][i:i + 1])
            output_fn = Path(flags.output_dir) / f"{stem}.png"
            Image.fromarray(strip).save(output_fn)
            if getattr(flags, "gt_dir", None):
                from . import metrics as M
                gt, gt_mask = M.load_target_views(flags.gt_dir, NUM_VIEWS, 256)
                res = M.summarise(M.image_metrics(M.strip_to_views(strip, NUM_VIEWS, 256)[0].to(model.device), gt, gt_mask))
                with open(Path(flags.output_dir) / f"{stem}_metrics.json", "w") as fh:
                    json.dump(dict(res, sampler=flags.sampler, sample_steps=flags.sample_steps), fh, indent=2)
            if want_mesh:
                mesh_outputs(x_sample[i], cams, chunk[i], faces, stored[f], flags.output_dir, stem,
                             export_mesh=getattr(flags, "export_mesh", False), mesh_overlay=getattr(flags, "mesh_overlay", False))
            if want_tex:
                texture_outputs(x_sample[i], cams, chunk[i], faces, stored[f], uv, face_uv, flags.output_dir, stem, export_texture=True,
                                size=getattr(flags, "texture_size", 1024), incidence=incidence)
    if flags.prepare_neus2_data:
        neus2_root = os.path.join(flags.output_dir, "neus2_data", f"{img_name}_{exp_name}")
        os.makedirs(os.path.join(neus2_root, "images"), exist_ok=True)
        with open(os.path.join(neus2_root, "transform.json"), "w") as fh:
            json.dump(B.neus2_transform(cams[0], cams[1], 256), fh, indent=4)
        for idx in range(NUM_VIEWS):
            bgra = B.neus2_view_bgra(strip, idx, 256)
            rgba = np.concatenate([bgra[:, :, 2::-1], bgra[:, :, 3:]], -1).astype(np.uint8)
            Image.fromarray(rgba, "RGBA").save(os.path.join(neus2_root, f"images/{str(idx).zfill(2)}.png"))
    return strip, str(output_fn)


def main(argv=None):
    run(parse_args(argv))


if __name__ == "__main__":
    main()

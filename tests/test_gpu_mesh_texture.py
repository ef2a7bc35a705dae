"""GPU: morphablediffusion_amd/mesh.py end to end on the two-sphere scene of tests/mesh_ref.py -- texture_mesh and rasterize_mesh
against the oracle, the post-sampling function of generate_face with synthetic views, and the argument checks of
SyncMultiviewDiffusion.texture_mesh through a stub batch.  No model is built."""
import json
import os
import types

import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import generate_face as G
from morphablediffusion_amd import mesh as MS
from tests import mesh_ref as R
from tests.test_gpu_mesh_ops import EPS, check_colours, dev

pytestmark = pytest.mark.gpu


def scene_views(s, seed=4):
    return np.random.default_rng(seed).uniform(-1, 1, (s["N"], 3, s["H"], s["W"])).astype(np.float32)


def test_texture_mesh_end_to_end():
    s = R.texture_scene()
    views = scene_views(s)
    out = MS.texture_mesh(dev(views), torch.from_numpy(s["verts"]), torch.from_numpy(s["faces"]), torch.from_numpy(s["K"]),
                          torch.from_numpy(s["RT"]), z_near=s["z_near"])
    # the integers of the GPU projection, by the projection test's rule ...
    xy, key = (t.cpu().numpy() for t in E.op_mesh_project(dev(s["verts"]), dev(s["K"]), dev(s["RT"]), s["z_near"]))
    ref = s["proj"]
    assert ref["valid"].all() and np.array_equal(key != 0, ref["valid"])
    Kd, RTd, x = s["K"].astype(np.float64), s["RT"].astype(np.float64), s["verts"].astype(np.float64)
    e = 8 * EPS * (np.einsum("nij,vj->nvi", np.abs(RTd[:, :, :3]), np.abs(x)) + np.abs(RTd[:, None, :, 3]))
    X, Y, Z = ref["cam"][..., 0], ref["cam"][..., 1], ref["cam"][..., 2]
    tau_u = (np.abs(Kd[:, None, 0, 0]) * e[..., 0] + np.abs(Kd[:, None, 0, 1]) * e[..., 1]) / Z \
        + np.abs(Kd[:, None, 0, 0] * X + Kd[:, None, 0, 1] * Y) * e[..., 2] / Z ** 2 + 4 * EPS * np.abs(ref["u"])
    tau_v = np.abs(Kd[:, None, 1, 1]) * e[..., 1] / Z + np.abs(Kd[:, None, 1, 1] * Y) * e[..., 2] / Z ** 2 + 4 * EPS * np.abs(ref["v"])
    tau_q = ref["q"] * e[..., 2] / Z + 4 * EPS * ref["q"]
    ru = (np.abs(xy[..., 0] / 16.0 - ref["u"]) / (1 / 32 + tau_u)).max()
    rv = (np.abs(xy[..., 1] / 16.0 - ref["v"]) / (1 / 32 + tau_v)).max()
    rq = (np.abs(key - np.clip(ref["q"], 1, R.KMAX)) / (0.5 + tau_q)).max()
    print(f"texture_mesh: projection worst error / bound: u {ru:.4f}, v {rv:.4f}, key {rq:.4f}")
    assert ru <= 1.0 and rv <= 1.0 and rq <= 1.0
    # ... then fed to the oracle's raster and fusion: everything downstream is compared as in the op tests
    face_id, pix_key, bad = R.raster(xy, key, s["faces"], s["H"], s["W"])
    assert bad == 0 and np.array_equal(out["face_id"].cpu().numpy(), face_id) and np.array_equal(out["mask"].cpu().numpy(), face_id >= 0)
    normals = MS.vertex_normals(s["verts"].astype(np.float64), s["faces"])
    want = R.vertex_colors(R.to_unit(views, "nchw"), xy, key, s["faces"], face_id, pix_key, s["verts"], normals.astype(np.float32),
                           R.camera_centres(s["RT"]).astype(np.float32))
    assert (want["weight_sum"] < 1e-6).mean() <= 0.02
    check_colours({"color": out["colors"], "spread": out["spread"], "weight_sum": out["weight_sum"], "n_seen": out["n_seen"],
                   "visible": out["visible"]}, want, "texture_mesh")
    multi = want["n_seen"] >= 2
    assert abs(out["consistency"] - np.nanmean(want["spread"][multi])) <= 1e-5 and out["consistency"] > 0.05  # noise views disagree
    assert out["coverage"] == float((out["weight_sum"] > 0).double().mean()) and abs(out["coverage"] - (want["weight_sum"] > 0).mean()) <= 0.005
    same = MS.texture_mesh(dev(np.full_like(views, 0.25)), s["verts"], s["faces"], s["K"], s["RT"], z_near=s["z_near"])
    assert same["consistency"] <= 1e-6 and same["coverage"] == out["coverage"]


def test_rasterize_mesh_mask_and_depth():
    s = R.texture_scene()
    K4 = np.tile(np.eye(4, dtype=np.float32), (s["N"], 1, 1))
    K4[:, :3, :3] = s["K"]
    out = MS.rasterize_mesh(s["verts"], s["faces"], K4, s["RT"], s["H"], s["W"])  # [N,4,4] intrinsics, the default z_near
    z_near = 0.5 * s["proj"]["Z"].min()
    assert abs(out["z_near"] - z_near) <= 1e-12
    xy, key = (t.cpu().numpy() for t in E.op_mesh_project(dev(s["verts"]), dev(s["K"]), dev(s["RT"]), out["z_near"]))
    face_id, pix_key, _ = R.raster(xy, key, s["faces"], s["H"], s["W"])
    assert np.array_equal(out["face_id"].cpu().numpy(), face_id) and np.array_equal(out["pix_key"].cpu().numpy(), pix_key)
    mask = out["mask"].cpu().numpy()
    assert mask.dtype == bool and np.array_equal(mask, face_id >= 0) and 0.1 < mask.mean() < 0.6
    depth = out["depth"].cpu().numpy()
    assert np.isinf(depth[~mask]).all()
    assert np.allclose(depth[mask], (out["z_near"] * R.KMAX / pix_key[mask].astype(np.float64)).astype(np.float32), rtol=1e-6, atol=0)
    # the nearest surface point of all views is the small sphere's front (centre c, radius 0.1) in the camera nearest to it: the
    # cameras look at the origin from 4.5 away; 0.01 covers the facets of 80 faces (0.006) and the sampling at pixel centres
    nearest = (4.5 - (s["centres"] / 4.5) @ np.array([0.08, -0.05, 0.43]) - 0.1).min()
    assert abs(depth[mask].min() - nearest) < 0.01 and depth[mask].max() < 5.0
    with pytest.raises(ValueError, match="outside"):
        bad = s["faces"].copy()
        bad[7, 1] = len(s["verts"])
        MS.rasterize_mesh(s["verts"], bad, s["K"], s["RT"], s["H"], s["W"])


def test_generate_face_mesh_outputs(tmp_path):
    s = R.texture_scene()
    views = scene_views(s)
    views[:, 0], views[:, 1], views[:, 2] = 0.5, -0.25, 0.25  # constant views: every seen vertex takes exactly this colour
    file_verts = s["verts"].astype(np.float64) * 3.0 + 1.0  # the file's frame is not the batch's
    cams = (torch.from_numpy(s["K"]), torch.from_numpy(s["RT"]))
    x = dev(views)[None]  # [B,N,3,H,W]
    none = G.mesh_outputs(x, cams, torch.from_numpy(s["verts"]), s["faces"], file_verts, tmp_path, "a_b")
    assert none == {} and os.listdir(tmp_path) == []  # without the flags no file appears
    got = G.mesh_outputs(x, cams, torch.from_numpy(s["verts"]), s["faces"], file_verts, tmp_path, "a_b", export_mesh=True,
                         mesh_overlay=True, z_near=s["z_near"])
    assert sorted(os.listdir(tmp_path)) == ["a_b_mesh.json", "a_b_mesh.ply", "a_b_overlay.png"]
    assert sorted(got) == ["json", "overlay", "ply"]
    v, f = MS.read_mesh(got["ply"])
    assert np.array_equal(v, file_verts) and np.array_equal(f, s["faces"])
    raw = open(got["ply"], "rb").read()
    rec = np.frombuffer(raw[raw.index(b"end_header\n") + 11:][:len(v) * 27], dtype=[("p", "<f8", (3,)), ("c", "u1", (3,))])
    tex = MS.texture_mesh(x[0], s["verts"], s["faces"], *cams, z_near=s["z_near"])
    seen = (tex["weight_sum"] > 0).cpu().numpy()
    assert (rec["c"][seen] == [191, 96, 159]).all() and (rec["c"][~seen] == 128).all() and 0 < (~seen).sum() < 0.02 * len(v)
    meta = json.load(open(got["json"]))
    assert meta["vertices"] == len(v) and meta["faces"] == len(f) and meta["coverage"] == tex["coverage"]
    assert meta["consistency"] <= 1e-6 and meta["visible_per_view"] == tex["visible"].sum(1).tolist() and len(meta["visible_per_view"]) == s["N"]
    from PIL import Image
    strip = np.asarray(Image.open(got["overlay"]))
    assert strip.shape == (s["H"], s["N"] * s["W"], 3) and strip.dtype == np.uint8
    mask = np.concatenate(list(tex["mask"].cpu().numpy()), 1)
    plain = np.array([191, 96, 159])
    assert (np.abs(strip[~mask].astype(int) - plain) <= 1).all() and (np.abs(strip[mask].astype(int) - plain).sum(-1) > 10).all()


def test_overlay_views_shapes_and_conventions():
    s = R.texture_scene()
    face_id = dev(s["face_id"])
    a = MS.overlay_views(dev(scene_views(s)), face_id >= 0, face_id)
    b = MS.overlay_views(dev((np.clip(scene_views(s), -1, 1) * 127.5 + 127.5).astype(np.uint8).transpose(0, 2, 3, 1)), face_id >= 0, face_id)
    assert a.shape == b.shape == (s["H"], s["N"] * s["W"], 3) and a.dtype == torch.uint8
    assert (a.int() - b.int()).abs().max() <= 2
    with pytest.raises(ValueError):
        MS.overlay_views(dev(scene_views(s)), face_id[:, :5] >= 0, face_id)


def test_model_texture_mesh_argument_checks_through_a_stub():
    from morphablediffusion_amd.model import SyncMultiviewDiffusion
    s = R.texture_scene()
    stub = types.SimpleNamespace(image_size=s["H"])
    call = SyncMultiviewDiffusion.texture_mesh
    N, H, W = s["N"], s["H"], s["W"]
    K4 = torch.eye(4).repeat(1, N, 1, 1)
    K4[0, :, :3, :3] = torch.from_numpy(s["K"])
    batch = {"vertices": torch.from_numpy(s["verts"])[None], "target_K": K4, "target_RT": torch.from_numpy(s["RT"])[None]}
    x = torch.zeros(1, N, 3, H, H)
    with pytest.raises(ValueError, match="input_image_size"):
        call(stub, batch, torch.zeros(1, N, 3, H, W), s["faces"])  # W is not the conditioner's size
    with pytest.raises(ValueError, match="input_image_size"):
        call(types.SimpleNamespace(image_size=256), batch, x, s["faces"])
    with pytest.raises(ValueError, match="target_RT"):
        call(stub, {k: v for k, v in batch.items() if k != "target_RT"}, x, s["faces"])
    with pytest.raises(ValueError, match="sample"):
        call(stub, batch, x, s["faces"], sample=1)
    with pytest.raises(ValueError, match="cameras"):
        call(stub, batch, x[:, :3], s["faces"])
    with pytest.raises(ValueError):
        call(stub, batch, x[0], s["faces"])
    # a square batch goes through: the cameras of the scene with the principal point of an H x H image
    K4[0, :, 0, 2] = H / 2.0
    out = call(stub, {k: v.cuda() for k, v in batch.items()}, dev(np.full((1, N, 3, H, H), 0.5, np.float32)), torch.from_numpy(s["faces"]),
               z_near=s["z_near"])
    seen = out["weight_sum"] > 0
    assert out["coverage"] > 0.95 and (out["colors"][seen] - 0.75).abs().max() <= 1e-6

"""GPU: morphablediffusion_amd/mesh.py's UV atlas functions end to end on the two-sphere scene of tests/mesh_uv_ref.py -- views
rendered from a known texture are baked back and reprojected (figures reported, not thresholded), the constant-texture
identities, SyncMultiviewDiffusion.bake_texture's argument checks through a stub, and generate_face's --export_texture files.
No model is built."""
import json
import os
import types

import numpy as np
import pytest
import torch

from morphablediffusion_amd import generate_face as G
from morphablediffusion_amd import mesh as MS
from tests import mesh_uv_ref as U
from tests.test_gpu_mesh_ops import EPS, dev
from tests.test_gpu_mesh_uv_ops import smooth_texture

pytestmark = pytest.mark.gpu
SIZE = (48, 64)


def scene_args(s):
    a = s["atlases"][SIZE]
    return (torch.from_numpy(s["verts"]), torch.from_numpy(s["faces"]), a["uv"], a["face_uv"], torch.from_numpy(s["K"]),
            torch.from_numpy(s["RT"]))


def test_bake_render_and_reprojection_end_to_end():
    """Reported, not asserted (no threshold is invented for them): the reprojection PSNR of an atlas baked from views that were
    rendered from a known smooth texture, and the texel error of that atlas against the known texture."""
    s = U.uv_scene()
    args = scene_args(s)
    known = smooth_texture(*SIZE)
    r = MS.render_textured(dev(known), *args, s["H"], s["W"], z_near=s["z_near"])
    assert tuple(r["images"].shape) == (s["N"], 3, s["H"], s["W"]) and r["images"].dtype == torch.float32
    assert np.array_equal(r["face_id"].cpu().numpy() >= 0, r["mask"].cpu().numpy()) and 0.1 < float(r["mask"].float().mean()) < 0.6
    assert (r["images"].permute(0, 2, 3, 1)[~r["mask"]] == 1.0).all() and float(r["images"].abs().max()) <= 1.0
    bake = MS.bake_texture(r["images"], *args, size=SIZE, z_near=s["z_near"])
    Ht, Wt = SIZE
    assert tuple(bake["texture"].shape) == (Ht, Wt, 3) and tuple(bake["valid"].shape) == (Ht, Wt) and bake["valid"].dtype == torch.bool
    assert np.array_equal(bake["tex_face"].cpu().numpy(), s["atlases"][SIZE]["tex_face"])
    seen = bake["weight_sum"] > 0
    chart = bake["tex_face"] >= 0
    assert bake["coverage"] == float((seen & chart).sum().double() / chart.sum().double()) and 0.8 < bake["coverage"] <= 1.0
    assert (bake["valid"] | ~seen).all() and int(bake["valid"].sum()) > int(seen.sum())  # the dilation only adds
    assert (bake["texture"][~bake["valid"]] == 0.5).all() and bake["consistency"] >= 0.0
    rep = MS.reprojection_metrics(r["images"], bake, *args)
    err = (bake["texture"] - dev(known)).abs()[seen]
    print(f"bake_texture of rendered views, {Wt} x {Ht} atlas, {s['N']} views of {s['W']} x {s['H']}: coverage {bake['coverage']:.4f}, "
          f"consistency {bake['consistency']:.4f}, texel error against the known texture mean {float(err.mean()):.4f} max "
          f"{float(err.max()):.4f}; reprojection PSNR mean {float(rep['psnr'].mean()):.2f} dB (min {float(rep['psnr'].min()):.2f}), "
          f"SSIM mean {float(rep['ssim'].mean()):.4f}")
    assert tuple(rep["psnr"].shape) == (s["N"],) and torch.isfinite(rep["ssim"]).all() and torch.equal(rep["mask"], r["mask"])


def test_constant_texture_survives_render_bake_and_reprojection():
    """A constant texture rendered over a background of the same colour gives constant views (a bilinear sample at a silhouette
    blends in the background, as it does for the vertices, so another background would show in the atlas): the atlas baked from
    them is that constant wherever it is seen, and its reprojection equals, on the mask, the render of the constant texture."""
    s = U.uv_scene()
    args = scene_args(s)
    c = np.float32([0.625, 0.125, 0.875])  # exact in fp32, 2 c - 1 too; 255 c is away from an integer, so 8-bit quantisation is stable
    const = dev(np.broadcast_to(c, SIZE + (3,)).copy())
    r = MS.render_textured(const, *args, s["H"], s["W"], z_near=s["z_near"], background=tuple(float(x) for x in c))
    assert (r["images"].permute(0, 2, 3, 1) == dev(2 * c - 1)).all()
    bake = MS.bake_texture(r["images"], *args, size=SIZE, z_near=s["z_near"])
    seen = bake["weight_sum"] > 0
    assert float((bake["texture"][seen] - dev(c)).abs().max()) <= (s["N"] + 2) * EPS and bake["consistency"] <= 1e-6
    # the dilated texels are means of seen ones: at most 10 u more per round of the pad
    grown = bake["valid"] & ~seen
    assert bool(grown.any()) and float((bake["texture"][grown] - dev(c)).abs().max()) <= (s["N"] + 2 + 4 * 10) * EPS
    white = MS.render_textured(const, *args, s["H"], s["W"], z_near=s["z_near"])  # the same views over white: image_metrics' convention
    rep = MS.reprojection_metrics(white["images"], bake, *args)
    wrong = (rep["images"].permute(0, 2, 3, 1)[rep["mask"]] - dev(2 * c - 1)).abs().amax(-1) > 2 * (s["N"] + 2 + 4 * 10 + 8) * EPS
    print(f"reprojection of a constant texture: {int(wrong.sum())} of {int(rep['mask'].sum())} covered pixels differ; mse per view "
          f"{rep['mse'].tolist()}")
    assert int(wrong.sum()) == 0 and (rep["mse"] == 0).all() and torch.isinf(rep["psnr"]).all()


def test_vertex_normals_device_matches_the_host_function_and_batches():
    s = U.uv_scene()
    v, f = s["verts"], s["faces"]
    one = MS.vertex_normals_device(dev(v), f)
    assert tuple(one.shape) == v.shape and one.is_cuda and one.dtype == torch.float32
    assert np.abs(one.cpu().numpy() - MS.vertex_normals(v, f)).max() <= 1e-6
    many = MS.vertex_normals_device(torch.stack([dev(v) * 2, dev(v), dev(v) + 1]), torch.from_numpy(f))
    assert torch.equal(many[1], one)


def test_model_bake_texture_argument_checks_through_a_stub():
    from morphablediffusion_amd.model import SyncMultiviewDiffusion
    s = U.uv_scene()
    a = s["atlases"][(40, 40)]
    stub = types.SimpleNamespace(image_size=s["H"])
    call = SyncMultiviewDiffusion.bake_texture
    N, H, W = s["N"], s["H"], s["W"]
    K4 = torch.eye(4).repeat(1, N, 1, 1)
    K4[0, :, :3, :3] = torch.from_numpy(s["K"])
    batch = {"vertices": torch.from_numpy(s["verts"])[None], "target_K": K4, "target_RT": torch.from_numpy(s["RT"])[None]}
    x = torch.zeros(1, N, 3, H, H)
    uvs = (s["faces"], a["uv"], a["face_uv"])
    with pytest.raises(ValueError, match="input_image_size"):
        call(stub, batch, torch.zeros(1, N, 3, H, W), *uvs)
    with pytest.raises(ValueError, match="input_image_size"):
        call(types.SimpleNamespace(image_size=256), batch, x, *uvs)
    with pytest.raises(ValueError, match="target_RT"):
        call(stub, {k: v for k, v in batch.items() if k != "target_RT"}, x, *uvs)
    with pytest.raises(ValueError, match="sample"):
        call(stub, batch, x, *uvs, sample=1)
    with pytest.raises(ValueError, match="cameras"):
        call(stub, batch, x[:, :3], *uvs)
    with pytest.raises(ValueError):
        call(stub, batch, x[0], *uvs)
    with pytest.raises(ValueError, match="face_uv"):
        call(stub, batch, x, s["faces"], a["uv"], a["face_uv"][:7])
    K4[0, :, 0, 2] = H / 2.0  # a square batch goes through: the scene's cameras with the principal point of an H x H image
    out = call(stub, {k: v.cuda() for k, v in batch.items()}, dev(np.full((1, N, 3, H, H), 0.5, np.float32)), torch.from_numpy(s["faces"]),
               a["uv"], a["face_uv"], size=(40, 40), z_near=s["z_near"])
    seen = out["weight_sum"] > 0
    assert out["coverage"] > 0.8 and float((out["texture"][seen] - 0.75).abs().max()) <= (N + 2) * EPS


def test_generate_face_texture_outputs(tmp_path):
    s = U.uv_scene()
    N, H, W = s["N"], s["H"], s["W"]
    views = np.empty((N, 3, H, W), np.float32)
    views[:, 0], views[:, 1], views[:, 2] = 0.5, -0.25, 0.25
    file_verts = s["verts"].astype(np.float64) * 3.0 + 1.0  # the file's frame is not the batch's
    cams = (torch.from_numpy(s["K"]), torch.from_numpy(s["RT"]))
    x = dev(views)[None]
    # the texture coordinates: --mesh's own vt, else --uv_mesh's, else one chart per triangle
    uv, face_uv = G.texture_coordinates(None, None, len(file_verts), s["faces"], 64)
    assert np.array_equal(uv, MS.triangle_atlas(len(s["faces"]), 64, 64)[0])
    MS.write_obj(tmp_path / "uv.obj", file_verts, s["faces"], uv[::-1].copy(), (len(uv) - 1 - face_uv).astype(np.int32), np.zeros((4, 4, 3)))
    for f in ("uv.mtl", "uv.png"):
        os.remove(tmp_path / f)
    uv2, face_uv2 = G.texture_coordinates(None, str(tmp_path / "uv.obj"), len(file_verts), s["faces"], 64)
    assert np.array_equal(uv2, uv[::-1]) and np.array_equal(uv2[face_uv2], uv[face_uv])
    uv3, _ = G.texture_coordinates(str(tmp_path / "uv.obj"), None, len(file_verts), s["faces"], 64)
    assert np.array_equal(uv3, uv2)
    with pytest.raises(ValueError, match="vertices"):
        G.texture_coordinates(None, str(tmp_path / "uv.obj"), len(file_verts) + 1, s["faces"], 64)
    os.remove(tmp_path / "uv.obj")
    none = G.texture_outputs(x, cams, torch.from_numpy(s["verts"]), s["faces"], file_verts, uv, face_uv, tmp_path, "a_b")
    assert none == {} and os.listdir(tmp_path) == []  # without the flag no file appears
    got = G.texture_outputs(x, cams, torch.from_numpy(s["verts"]), s["faces"], file_verts, uv, face_uv, tmp_path, "a_b", export_texture=True,
                            size=64, z_near=s["z_near"])
    assert sorted(os.listdir(tmp_path)) == ["a_b_texture.json", "a_b_texture.png", "a_b_textured.mtl", "a_b_textured.obj"]
    assert sorted(got) == ["json", "mtl", "obj", "png"]
    v, f, uvr, fuvr = MS.read_mesh_uv(got["obj"])
    assert np.array_equal(v, file_verts) and np.array_equal(f, s["faces"]) and np.array_equal(uvr, uv) and np.array_equal(fuvr, face_uv)
    from PIL import Image
    png = np.asarray(Image.open(got["png"]))
    bake = MS.bake_texture(x[0], s["verts"], s["faces"], uv, face_uv, *cams, size=64, z_near=s["z_near"])
    valid = bake["valid"].cpu().numpy()
    assert png.shape == (64, 64, 3) and (png[valid] == [191, 96, 159]).all() and (png[~valid] == 128).all() and 0.1 < valid.mean() < 1
    meta = json.load(open(got["json"]))
    assert meta["vertices"] == len(v) and meta["faces"] == len(f) and meta["size"] == [64, 64] and meta["coverage"] == bake["coverage"]
    assert meta["consistency"] <= 1e-6 and len(meta["psnr"]) == N and len(meta["ssim"]) == N and "psnr_mean" in meta
    flags = G.parse_args(["--input_img", "a.png", "--exp_img", "b.png", "--mesh", "m.obj", "--output_dir", "o", "--export_texture",
                          "--texture_size", "512", "--uv_mesh", "u.obj"])
    assert flags.export_texture and flags.texture_size == 512 and flags.uv_mesh == "u.obj"
    plain = G.parse_args(["--input_img", "a.png", "--exp_img", "b.png", "--mesh", "m.obj", "--output_dir", "o"])
    assert not plain.export_texture and plain.texture_size == 1024 and plain.uv_mesh is None

"""GPU: generate_face --export_texture through run() and run_flame() on the synthetic checkpoint of the end-to-end tests: with --mesh
an OBJ that carries vt, and on the --frames path of a seeded FLAME-shaped model file with the per-triangle fallback atlas.  One
model is loaded and shared by the three runs."""
import json

import numpy as np
import pytest
import torch

from tests import mesh_ref
from tests import morphable_ref as R

pytestmark = pytest.mark.gpu


def test_generate_face_export_texture_with_a_mesh_file_and_on_the_frames_path(tmp_path):
    import yaml
    from PIL import Image
    from morphablediffusion_amd import generate_face as GF
    from morphablediffusion_amd import mesh as MS
    from morphablediffusion_amd.spec import (ClipConfig, UNetConfig, VaeConfig, VolumeConfig, clip_manifest, full_manifest,
                                             vae_decoder_manifest, vae_encoder_manifest)
    from morphablediffusion_amd.weights import seeded_state_dict
    from tests.test_gpu_eval_caller import facescape_yaml
    ucfg, vcfg = UNetConfig(model_channels=64), VolumeConfig(num_views=16)
    Wt = seeded_state_dict(full_manifest(ucfg, vcfg), 7)
    vae = VaeConfig(ch=32)
    Wt.update(seeded_state_dict(vae_decoder_manifest(vae), 7))
    Wt.update(seeded_state_dict(vae_encoder_manifest(vae), 7))
    Wt.update({k: v.half() for k, v in seeded_state_dict(clip_manifest(ClipConfig(width=128, layers=2, heads=2, embed=768)), 7).items()})
    torch.save({"state_dict": Wt}, tmp_path / "m.ckpt")
    (tmp_path / "facescape.yaml").write_text(yaml.safe_dump(facescape_yaml(view_num=16)))
    model = GF.load_model(str(tmp_path / "facescape.yaml"), str(tmp_path / "m.ckpt"))
    rgba = np.full((300, 280, 4), 255, np.uint8)
    rgba[..., :3] = np.random.RandomState(1).randint(0, 255, (300, 280, 3))
    Image.fromarray(rgba, "RGBA").save(tmp_path / "subject.png")
    base = ["--input_img", str(tmp_path / "subject.png"), "--exp_img", str(tmp_path / "kiss.jpg"), "--cfg", str(tmp_path / "facescape.yaml"),
            "--ckpt", str(tmp_path / "m.ckpt"), "--sample_steps", "2", "--batch_view_num", "8"]
    # ---- run(): --mesh is an OBJ with vt lines, whose texture coordinates are used
    sv, sf = mesh_ref.icosphere(3, 0.1)  # a head-sized sphere in metres
    uv, face_uv = MS.triangle_atlas(len(sf), 200, 200, gutter=2)  # not the atlas the flag would fall back to
    MS.write_obj(tmp_path / "head.obj", sv, sf, uv, face_uv, np.zeros((2, 2, 3)))
    plain, out = tmp_path / "plain", tmp_path / "out"
    GF.run(GF.parse_args(base + ["--mesh", str(tmp_path / "head.obj"), "--output_dir", str(plain)]), model=model)
    assert sorted(p.name for p in plain.iterdir()) == ["subject_kiss.png"]  # without the flag: what it wrote before
    strip, _ = GF.run(GF.parse_args(base + ["--mesh", str(tmp_path / "head.obj"), "--output_dir", str(out), "--export_texture",
                                            "--texture_size", "256"]), model=model)
    assert sorted(p.name for p in out.iterdir()) == ["subject_kiss.png", "subject_kiss_texture.json", "subject_kiss_texture.png",
                                                     "subject_kiss_textured.mtl", "subject_kiss_textured.obj"]
    assert np.array_equal(np.asarray(Image.open(out / "subject_kiss.png")), np.asarray(Image.open(plain / "subject_kiss.png")))
    v, f, uv2, fuv2 = MS.read_mesh_uv(out / "subject_kiss_textured.obj")
    assert np.array_equal(v, sv) and np.array_equal(f, sf) and np.array_equal(uv2, uv) and np.array_equal(fuv2, face_uv)
    meta = json.load(open(out / "subject_kiss_texture.json"))
    assert meta["vertices"] == len(sv) and meta["faces"] == len(sf) and meta["size"] == [256, 256] and meta["texture_coordinates"] == len(uv)
    assert 0.0 < meta["coverage"] <= 1.0 and len(meta["psnr"]) == 16 and len(meta["ssim"]) == 16 and np.isfinite(meta["psnr_mean"])
    png = np.asarray(Image.open(out / "subject_kiss_texture.png"))
    assert png.shape == (256, 256, 3) and len(np.unique(png.reshape(-1, 3), axis=0)) > 100  # colours of the views, not the fill alone
    # ---- run_flame(): two frames of a sweep, the fallback atlas, one set of files per frame
    V, NB = len(sv), 10
    m = R.synthetic_model(31, V, NB, 5, parents=[-1, 0, 1, 1, 1])
    kt = np.array([[2 ** 32 - 1, 0, 1, 1, 1], [0, 1, 2, 3, 4]], dtype=np.uint32)
    np.savez(tmp_path / "flame.npz", v_template=sv.astype(np.float32), shapedirs=m["shapedirs"], posedirs=m["posedirs"],
             J_regressor=m["J_regressor"], kintree_table=kt, weights=m["weights"], f=sf)
    shape = np.random.default_rng(2).normal(size=6)
    np.savez(tmp_path / "neutral.npz", shape=shape)
    np.savez(tmp_path / "target.npz", shape=shape, jaw=np.array([0.3, 0.0, 0.0]))
    sweep = tmp_path / "sweep"
    GF.run(GF.parse_args(base + ["--output_dir", str(sweep), "--flame_model", str(tmp_path / "flame.npz"), "--flame_params",
                                 str(tmp_path / "target.npz"), "--neutral_params", str(tmp_path / "neutral.npz"), "--frames", "2",
                                 "--frame_batch", "2", "--export_texture", "--texture_size", "256"]), model=model)
    assert sorted(p.name for p in sweep.iterdir()) == sorted(
        f"subject_kiss_f{k:02d}{s}" for k in range(2) for s in (".png", "_textured.obj", "_textured.mtl", "_texture.png", "_texture.json"))
    want_uv, want_fuv = MS.triangle_atlas(len(sf), 256, 256)
    frames = [MS.read_mesh_uv(sweep / f"subject_kiss_f{k:02d}_textured.obj") for k in range(2)]
    for v, f, uv3, fuv3 in frames:
        assert len(v) == V and np.array_equal(f, sf) and np.array_equal(uv3, want_uv) and np.array_equal(fuv3, want_fuv)
    assert not np.array_equal(frames[0][0], frames[1][0])  # the mesh moved between the frames
    for k in range(2):
        meta = json.load(open(sweep / f"subject_kiss_f{k:02d}_texture.json"))
        assert meta["faces"] == len(sf) and 0.0 < meta["coverage"] <= 1.0 and len(meta["psnr"]) == 16

"""GPU: generate_face with the mesh computed from FLAME parameters (--flame_model / --flame_params / --neutral_params / --frames)
on the synthetic checkpoint of the end-to-end tests and a seeded FLAME-shaped model file: one strip and one textured mesh per
frame of the sweep, the end frames being the neutral and the target parameters."""
import numpy as np
import pytest
import torch

from tests import mesh_ref
from tests import morphable_ref as R

pytestmark = pytest.mark.gpu


def test_generate_face_sweeps_flame_parameters(tmp_path):
    import yaml
    from PIL import Image
    from morphablediffusion_amd import generate_face as GF
    from morphablediffusion_amd import morphable as MM
    from morphablediffusion_amd.mesh import read_mesh
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
    # a head-sized sphere in metres with FLAME's joints; expression and jaw move it
    sv, sf = mesh_ref.icosphere(3, 0.1)
    V, NB = len(sv), 10
    m = R.synthetic_model(31, V, NB, 5, parents=[-1, 0, 1, 1, 1])
    kt = np.array([[2 ** 32 - 1, 0, 1, 1, 1], [0, 1, 2, 3, 4]], dtype=np.uint32)
    np.savez(tmp_path / "flame.npz", v_template=sv.astype(np.float32), shapedirs=m["shapedirs"], posedirs=m["posedirs"],
             J_regressor=m["J_regressor"], kintree_table=kt, weights=m["weights"], f=sf)
    g = np.random.default_rng(2)
    shape = g.normal(size=6)
    np.savez(tmp_path / "neutral.npz", shape=shape)
    np.savez(tmp_path / "target.npz", shape=shape, expression=g.normal(size=4) * 2, jaw=np.array([0.3, 0.0, 0.0]))
    rgba = np.full((300, 280, 4), 255, np.uint8)
    rgba[..., :3] = np.random.RandomState(1).randint(0, 255, (300, 280, 3))
    Image.fromarray(rgba, "RGBA").save(tmp_path / "subject.png")
    out = tmp_path / "out"
    args = ["--input_img", str(tmp_path / "subject.png"), "--exp_img", str(tmp_path / "kiss.jpg"), "--cfg", str(tmp_path / "facescape.yaml"),
            "--ckpt", str(tmp_path / "m.ckpt"), "--output_dir", str(out), "--sample_steps", "2", "--batch_view_num", "8",
            "--flame_model", str(tmp_path / "flame.npz"), "--flame_params", str(tmp_path / "target.npz"),
            "--neutral_params", str(tmp_path / "neutral.npz"), "--frames", "4", "--frame_batch", "2", "--export_mesh"]
    strip, path = GF.run(GF.parse_args(args))
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted(f"subject_kiss_f{f:02d}{s}" for f in range(4) for s in (".png", "_mesh.ply", "_mesh.json"))
    strips = [np.asarray(Image.open(out / f"subject_kiss_f{f:02d}.png")) for f in range(4)]
    assert path.endswith("subject_kiss_f03.png") and np.array_equal(strips[3], strip)
    assert all(s.shape == (256, 17 * 256, 3) for s in strips)
    assert all(np.array_equal(s[:, :256], strips[0][:, :256]) for s in strips)  # the input view leads every strip
    assert all(not np.array_equal(strips[f][:, 256:], strips[f + 1][:, 256:]) for f in range(3))  # the mesh moved, and the views with it
    # the meshes written are the model's vertices at the sweep's parameters, end points exact
    fm = MM.MorphableModel.load(tmp_path / "flame.npz", device="cuda:0")
    ends = {0: fm.flame(shape), 3: fm.flame(shape, **{k: v for k, v in np.load(tmp_path / "target.npz").items() if k != "shape"})}
    for f, o in ends.items():
        v, faces = read_mesh(out / f"subject_kiss_f{f:02d}_mesh.ply")
        assert np.array_equal(v, o["vertices"][0].cpu().double().numpy()) and np.array_equal(faces, sf)
    assert not np.array_equal(read_mesh(out / "subject_kiss_f01_mesh.ply")[0], read_mesh(out / "subject_kiss_f02_mesh.ply")[0])

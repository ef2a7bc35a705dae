"""GPU: generate_face --fit_landmarks2d on the synthetic checkpoint of the end-to-end tests and a seeded FLAME-shaped model file
with a landmark embedding: the fit files it writes, the flag rules, and that the flag only feeds the pipeline that --flame_params
has always fed (the strip of the fitted parameters is the strip of the same parameters given as a file)."""
import json

import numpy as np
import pytest
import torch

from tests import mesh_ref
from tests import morphable_2d_ref as R2
from tests import morphable_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_flag_rules():
    from morphablediffusion_amd import generate_face as GF
    base = ["--input_img", "a.png", "--exp_img", "b.jpg", "--output_dir", "o", "--flame_model", "m.npz"]
    flags = GF.parse_args(base + ["--fit_landmarks2d", "l.npz", "--fit_iters", "7"])
    assert flags.fit_landmarks2d == "l.npz" and flags.fit_iters == 7 and flags.fit_mesh is None and flags.fit_scan is None
    assert GF.parse_args(base + ["--flame_params", "p.npz"]).fit_landmarks2d is None
    for extra in (["--fit_mesh", "m.ply"], ["--fit_scan", "s.ply"], ["--mesh", "m.ply"], ["--neutral_params", "n.npz"], ["--fit_iters", "0"],
                  ["--frames", "3"]):
        with pytest.raises(SystemExit):
            GF.parse_args(base + ["--fit_landmarks2d", "l.npz"] + extra)
    with pytest.raises(SystemExit):
        GF.parse_args(base[:6] + ["--fit_landmarks2d", "l.npz"])  # no --flame_model


def test_generate_face_fits_2d_landmarks(tmp_path):
    import yaml
    from PIL import Image
    from morphablediffusion_amd import engine as E
    from morphablediffusion_amd import generate_face as GF
    from morphablediffusion_amd import morphable as MM
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
    sv, sf = mesh_ref.icosphere(3, 0.1)
    V, NB, M = len(sv), 10, 24
    m = R.synthetic_model(31, V, NB, 5, parents=[-1, 0, 1, 1, 1])
    g = np.random.default_rng(2)
    bc = g.random((M, 3)) + 0.1
    kt = np.array([[2 ** 32 - 1, 0, 1, 1, 1], [0, 1, 2, 3, 4]], dtype=np.uint32)
    np.savez(tmp_path / "flame.npz", v_template=sv.astype(np.float32), shapedirs=m["shapedirs"] * 4, posedirs=m["posedirs"],
             J_regressor=m["J_regressor"], kintree_table=kt, weights=m["weights"], f=sf,
             static_lmk_faces_idx=g.choice(len(sf), M, replace=False), static_lmk_bary_coords=bc / bc.sum(1, keepdims=True))
    fm = MM.MorphableModel.load(tmp_path / "flame.npz", device=DEV)
    known = dict(shape=np.zeros(NB), global_pose=np.array([0.05, -0.1, 0.03]), jaw=np.array([0.2, 0.0, 0.0]), transl=np.array([0.01, -0.02, 0.015]))
    K, RT = R2.cameras([-35.0, 0.0, 40.0], pitch_deg=10.0)
    uv, valid = E.op_morph_project(fm.flame(**known)["landmarks"], torch.from_numpy(K).to(DEV), torch.from_numpy(RT).to(DEV))
    assert valid.all()
    w = np.ones((3, M), np.float32)
    w[1, :3] = 0
    lm = uv[0].cpu().numpy()
    lm[1, :3] = np.nan  # not detected
    np.savez(tmp_path / "lmk.npz", landmarks=lm, K=K, RT=RT, weights=w, image_size=np.array([512, 512]))
    rgba = np.full((300, 280, 4), 255, np.uint8)
    rgba[..., :3] = np.random.RandomState(1).randint(0, 255, (300, 280, 3))
    Image.fromarray(rgba, "RGBA").save(tmp_path / "subject.png")
    out = tmp_path / "out"
    base = ["--input_img", str(tmp_path / "subject.png"), "--exp_img", str(tmp_path / "kiss.jpg"), "--cfg", str(tmp_path / "facescape.yaml"),
            "--ckpt", str(tmp_path / "m.ckpt"), "--output_dir", str(out), "--sample_steps", "2", "--batch_view_num", "8",
            "--flame_model", str(tmp_path / "flame.npz")]
    model = GF.load_model(str(tmp_path / "facescape.yaml"), str(tmp_path / "m.ckpt"), device=DEV)
    strip, path = GF.run(GF.parse_args(base + ["--fit_landmarks2d", str(tmp_path / "lmk.npz"), "--fit_iters", "300"]), model=model)
    assert sorted(p.name for p in out.iterdir()) == ["subject_kiss.png", "subject_kiss_fit.json", "subject_kiss_fit.npz"]
    assert path.endswith("subject_kiss.png") and strip.shape == (256, 17 * 256, 3)
    js = json.loads((out / "subject_kiss_fit.json").read_text())
    fitted = dict(np.load(out / "subject_kiss_fit.npz"))
    assert sorted(fitted) == sorted(GF.FLAME_FILE_KEYS) and js["iterations"] == 300 and js["views"] == 3 and js["points"] == M
    assert js["observations"] == 3 * M - 3 and len(js["reprojection_px"]) == 3
    # the file's figure is the reprojection error of the parameters it wrote, and the fit lowered it
    uv_fit, _ = E.op_morph_project(fm.flame(**fitted)["landmarks"], torch.from_numpy(K).to(DEV), torch.from_numpy(RT).to(DEV))
    uv_rest, _ = E.op_morph_project(fm.flame(np.zeros(NB))["landmarks"], torch.from_numpy(K).to(DEV), torch.from_numpy(RT).to(DEV))
    again, first = (MM.reprojection_error(u, lm[None], w[None])["mean_px"][0] for u in (uv_fit, uv_rest))
    print(f"--fit_landmarks2d: reprojection {first} -> {again} px (the file says {js['reprojection_px']})")
    assert np.allclose(again, js["reprojection_px"], rtol=1e-3, atol=1e-4) and (again < 0.05 * first).all() and js["loss_last"] < js["loss_first"]
    # the flag only feeds the pipeline --flame_params feeds: the same parameters as a file give the same strip
    out2 = tmp_path / "out2"
    args = [a if a != str(out) else str(out2) for a in base] + ["--flame_params", str(out / "subject_kiss_fit.npz")]
    strip2, _ = GF.run(GF.parse_args(args), model=model)
    assert np.array_equal(strip, strip2) and sorted(p.name for p in out2.iterdir()) == ["subject_kiss.png"]
    # a file without cameras is refused by name
    np.savez(tmp_path / "bad.npz", landmarks=lm)
    with pytest.raises(ValueError, match="missing"):
        GF.run(GF.parse_args(base + ["--fit_landmarks2d", str(tmp_path / "bad.npz")]), model=model)

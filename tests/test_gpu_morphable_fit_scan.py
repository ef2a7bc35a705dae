"""GPU: fitting to an unregistered scan (MorphableModel.fit_scan / fit_flame_scan over mvd_morph_fit_scan_run, mesh.surface_distance,
generate_face --fit_scan) on the inputs of tests/closest_ref.scan_case: the icosphere(2) topology with a non-symmetric template, the
scan being the posed surface with every triangle split in four, shuffled.

Convergence is a condition: from zero, lr 0.05, 300 iterations, the model-to-scan surface RMS must fall to at most 1e-2 of its start
(the float64 loop reaches 1e-6 of it; tests/test_closest_cpu.py checks that).  The trajectory after 20 and 100 iterations may differ
from the float64 ICP loop by at most 4 times what the same loop run in float32 differs from it (tests/golden/fit_scan_trajectory.npz,
which tests/test_closest_cpu.py checks against the loop).  The loop against the per-op entries, and repeats, are bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import mesh as MS
from morphablediffusion_amd import morphable as MM
from tests import closest_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_scan_trajectory.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def model_of(m, **kw):
    return MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"],
                                         faces=m["faces"], lmk_face=m["lmk_face"], lmk_bary=m["lmk_bary"], device=DEV, **kw)


def packed(fit):
    return torch.cat([fit["betas"], fit["pose"].reshape(fit["betas"].shape[0], -1), fit["transl"]], 1)


@pytest.fixture(scope="module")
def one():
    m, p_true, scans = R.scan_case()
    return m, model_of(m), p_true, scans


@pytest.fixture(scope="module")
def fitted(one):
    m, fm, p_true, scans = one
    return fm.fit_scan(scans[0][0], scans[0][1], iters=300, lr=0.05)


def test_fit_scan_meets_the_convergence_condition(one, fitted):
    m, fm, p_true, scans = one
    fit = fitted
    first = R.surface_rms(m, np.zeros_like(p_true), scans)
    last = R.surface_rms(m, packed(fit).cpu().numpy(), scans)
    print(f"fit_scan from zero: model-to-scan surface RMS {first} -> {last}, ratio {last / first}; fit_scan's rms {fit['rms'].cpu().numpy()}")
    assert fit["loss_history"].shape == (300, 1) and torch.isfinite(fit["loss_history"]).all()
    assert fit["matched_history"].shape == (300, 1) and (fit["matched_history"] == 162).all() and (fit["matched"] == 162).all()
    assert fit["corr_face"].shape == (1, 162) and fit["corr_face"].dtype == torch.int32 and (fit["corr_face"] >= 0).all()
    assert (last <= 1e-2 * first).all()


def test_rms_is_a_fresh_query_and_surface_distance_matches_the_oracle(one, fitted):
    m, fm, p_true, scans = one
    fit = fitted
    sv, sf = scans[0]
    y = fit["vertices"][0]
    q = MS.closest_point(y, sv, sf)
    assert torch.equal(q["face"], fit["corr_face"][0])
    assert abs(float(q["dist2"].double().mean().sqrt()) - float(fit["rms"][0])) <= 1e-6 * float(fit["rms"][0]) + 1e-12
    # scan-to-mesh and back, against the oracle's statistics within the distance bound of each direction
    y64 = y.cpu().numpy().astype(np.float64)
    got = MS.surface_distance(sv, y, fm.faces, symmetric=True, point_faces=sf)
    want_f = np.sqrt(R.distance_matrix(sv, y64, m["faces"]).min(1))
    want_b = np.sqrt(R.distance_matrix(y64, sv, sf).min(1))
    bound_f, _ = R.bound(sv, y64, m["faces"], want_f)
    bound_b, _ = R.bound(y64, sv, sf, want_b)
    for name, g, want, bound in (("scan to mesh", got, want_f, bound_f), ("mesh to scan", got["back"], want_b, bound_b)):
        st = R.statistics(want)
        err = np.abs(g["dist"].cpu().numpy().astype(np.float64) - want).max()
        print(f"{name}: worst distance error {err:.3e}, bound {bound:.3e}; " + ", ".join(f"{k} {g[k]:.3e}" for k in st))
        assert err <= bound and g["matched"] == 1.0
        for k in ("mean", "rms", "median", "p90", "max"):
            assert abs(g[k] - st[k]) <= bound, (name, k)
    assert abs(got["chamfer"] - 0.5 * (got["mean"] + got["back"]["mean"])) < 1e-15
    far = MS.surface_distance(sv, y, fm.faces, max_dist=1e-9)
    assert far["matched"] < 1.0 and torch.isinf(far["dist"]).any()


def test_fit_scan_follows_the_float64_trajectory(one):
    m, fm, p_true, scans = one
    gold = np.load(GOLD)
    for k in (20, 100):
        fit = fm.fit_scan(scans[0][0], scans[0][1], iters=k, lr=0.05)
        got = packed(fit).cpu().numpy().astype(np.float64)
        yard, err = float(gold[f"yard{k}"]), np.abs(got - gold[f"p{k}"]).max()
        print(f"fit_scan after {k} iterations: worst parameter difference to the float64 loop {err:.3e}, float32 loop {yard:.3e}, "
              f"ratio {err / yard:.2f}")
        assert err <= 4 * yard, k
        if k == 20:
            assert np.allclose(fit["loss_history"][:, 0].cpu().numpy(), gold["loss20"][:, 0], rtol=1e-3)


def test_fit_scan_repeats_and_frames_are_independent():
    m, p_true, scans = R.scan_case(F=2, M=5)
    fm = model_of(m)
    sv, sf = [s[0] for s in scans], [s[1] for s in scans]
    kw = dict(iters=25, normal_cos=0.2, max_dist=0.05, refresh=3)
    a, b = fm.fit_scan(sv, sf, **kw), fm.fit_scan(sv, sf, **kw)
    keys = ("betas", "pose", "transl", "vertices", "loss_history", "matched_history", "corr_face", "matched")
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    alone = fm.fit_scan(sv[1], sf[1], **kw)
    for k in ("betas", "pose", "transl", "vertices", "corr_face", "matched"):
        assert torch.equal(a[k][1:2], alone[k]), k
    assert torch.equal(a["loss_history"][:, 1:2], alone["loss_history"]) and torch.equal(a["matched_history"][:, 1:2], alone["matched_history"])
    # a shared scan for two frames that start apart: one launch with Q = F V; each frame equals the frame fitted alone
    init = {"transl": np.float32([[0.0, 0.0, 0.0], [0.01, -0.01, 0.0]])}
    both = fm.fit_scan(sv[0], sf[0], init=init, **kw)
    second = fm.fit_scan(sv[0], sf[0], init={"transl": init["transl"][1:]}, **kw)
    assert both["betas"].shape[0] == 2
    for k in ("betas", "pose", "transl", "corr_face"):
        assert torch.equal(both[k][1:2], second[k]), k
    # a point cloud: no faces
    cloud = fm.fit_scan(sv[0], None, iters=5)
    assert (cloud["matched"] == 162).all() and torch.isfinite(cloud["rms"]).all()


def composed(fm, start, lrv, lam, p0, iters, scans, incidence, normal_cos, max_dist2, refresh, vertex_weight, target_lmk, lmk_lambda, post):
    """mvd_morph_fit_scan_run's iterations out of the per-op entries: (p, m, v, loss_history, matched_history, corr_face)."""
    F, NB, J, V = start.shape[0], fm.NB, fm.J, fm.V
    q, qm, qv = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
    hist, matched = [], []
    use_l = target_lmk is not None
    cp = cf = None
    for it in range(iters):
        betas, pose, transl = q[:, :NB].contiguous(), q[:, NB:NB + 3 * J].reshape(F, J, 3).contiguous(), q[:, NB + 3 * J:].contiguous()
        pr = E.op_morph_pose(betas, pose, fm.j_template, fm.j_dirs, fm.parents)
        coef = torch.cat([betas, pr["pose_feature"]], 1)
        verts, blend = E.op_morph_skin_ex(fm.basis, fm.v_template, coef, fm.weights, pr["A"], post=post, transl=transl, want_blend=True)
        lmk = E.op_morph_landmarks(verts, fm.faces, fm.lmk_face, fm.lmk_bary) if use_l else None
        if it % refresh == 0:
            nrm = E.op_mesh_vertex_normals(verts, fm.faces, incidence[0], incidence[1])[0] if normal_cos is not None else None
            kw = dict(cos_min=0.0 if normal_cos is None else normal_cos, max_dist2=max_dist2)
            if len(scans) == 1:
                o = E.op_mesh_closest_point(verts.reshape(-1, 3), scans[0][0], scans[0][1],
                                            query_normals=None if nrm is None else nrm.reshape(-1, 3), **kw)
                cp, cf = o["point"].reshape(F, V, 3), o["face"].reshape(F, V)
            else:
                per = [E.op_mesh_closest_point(verts[f], scans[f][0], scans[f][1], query_normals=None if nrm is None else nrm[f], **kw)
                       for f in range(F)]
                cp, cf = torch.stack([o["point"] for o in per]), torch.stack([o["face"] for o in per])
        Ef, g_y, n = E.op_morph_fit_data_corr(verts, cp, cf, vertex_weight=vertex_weight, lmk=lmk, target_lmk=target_lmk, lmk_lambda=lmk_lambda,
                                              csr=(fm.csr_ptr, fm.csr_ent, fm.lmk_bary) if use_l else None)
        hist.append(Ef), matched.append(n)
        sb = E.op_morph_skin_bwd(g_y, fm.weights, pr["A"], blend, fm.basis, post=post)
        g = E.op_morph_pose_bwd(pose, pr["j_rest"], pr["A"], fm.j_dirs, fm.parents, sb["part_a"], sb["part_c"])
        E.op_morph_fit_update(q, torch.cat([g["betas"], g["pose"].reshape(F, -1), g["transl"]], 1), qm, qv, lrv, lam, p0, it + 1)
    return q, qm, qv, torch.stack(hist), torch.stack(matched), cf


def test_fit_scan_run_equals_the_ops_composed():
    m, p_true, scans = R.scan_case(F=2, M=5)
    fm = model_of(m)
    F, V, P = 2, fm.V, fm.NB + 3 * fm.J + 3
    rng = np.random.default_rng(1)
    lrv, lam, p0 = (dev(a.astype(np.float32)) for a in fm.fit_vectors(0.05, reg={"betas": 1e-3}, prior={"betas": rng.normal(size=fm.NB)}))
    start = dev((rng.normal(size=(F, P)) * 0.02).astype(np.float32))
    post = dev(MM.flame_alignment().numpy().astype(np.float32))
    vw = dev(rng.random(V).astype(np.float32))
    tl = fm.forward(dev(np.float32(p_true[:, :10])), dev(np.float32(p_true[:, 10:25].reshape(2, 5, 3))),
                    transl=dev(np.float32(p_true[:, 25:])))["landmarks"]
    inc = tuple(torch.from_numpy(a).to(DEV) for a in MS.face_incidence(fm.faces, V))
    # the second scan loses faces and vertices: two per-frame scans of different sizes
    sv1, sf1 = scans[1][0][:600], scans[1][1][(scans[1][1] < 600).all(1)]
    per_frame = [(dev(scans[0][0]), dev(scans[0][1])), (dev(sv1), dev(sf1))]
    shared = per_frame[:1]
    assert 0 < len(sf1) < 1280
    d2 = float(np.float32(0.01 ** 2))  # below the start's RMS distance of 0.008-0.01: some vertices drop out
    cases = (dict(scans=shared, refresh=1), dict(scans=per_frame, refresh=2),
             dict(scans=per_frame, refresh=1, normal_cos=0.3, max_dist2=d2, vertex_weight=vw, target_lmk=tl, lmk_lambda=0.5),
             dict(scans=shared, refresh=2, normal_cos=0.0, target_lmk=tl[:1], post=None),
             dict(scans=shared, refresh=1, max_dist2=d2),
             dict(scans=per_frame, refresh=2, post=post))
    for kw in cases:
        args = dict(normal_cos=kw.get("normal_cos"), max_dist2=kw.get("max_dist2", float("inf")), refresh=kw["refresh"],
                    vertex_weight=kw.get("vertex_weight"), target_lmk=kw.get("target_lmk"), lmk_lambda=kw.get("lmk_lambda", 1.0),
                    post=kw.get("post"))
        sc = kw["scans"]
        if kw.get("post") is not None:  # the scan in the posted frame, where the fitted vertices live
            Pm = post.reshape(3, 4)
            sc = [(a @ Pm[:, :3].T + Pm[:, 3], b) for a, b in sc]
        p, mm, vv = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
        hist, matched, cf = E.morph_fit_scan_run(fm, p, mm, vv, lrv, lam, p0, 5, sc, incidence=inc, **args)
        q, qm, qv, hist2, matched2, cf2 = composed(fm, start, lrv, lam, p0, 5, sc, inc, **{k: args[k] for k in args})
        assert torch.equal(p, q) and torch.equal(mm, qm) and torch.equal(vv, qv), kw.keys()
        assert torch.equal(hist, hist2) and torch.equal(matched, matched2) and torch.equal(cf, cf2), kw.keys()
        assert not torch.equal(p, start) and (matched > 0).all()
        if "max_dist2" in kw:
            assert (matched < V).any()  # the gate dropped something, and the loop went on


def test_generate_face_fits_a_scan_and_sweeps_from_the_fit(tmp_path):
    import yaml
    from PIL import Image
    from morphablediffusion_amd import generate_face as GF
    from morphablediffusion_amd.mesh import write_ply
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
    m, p_true, scans = R.scan_case()
    kt = np.array([[2 ** 32 - 1, 0, 1, 1, 1], [0, 1, 2, 3, 4]], dtype=np.uint32)
    np.savez(tmp_path / "flame.npz", v_template=m["v_template"], shapedirs=m["shapedirs"], posedirs=m["posedirs"],
             J_regressor=m["J_regressor"], kintree_table=kt, weights=m["weights"], f=m["faces"])
    write_ply(str(tmp_path / "scan.ply"), scans[0][0].astype(np.float64), scans[0][1])
    np.savez(tmp_path / "smile.npz", jaw=np.array([0.4, 0.0, 0.0]))
    rgba = np.full((300, 280, 4), 255, np.uint8)
    rgba[..., :3] = np.random.RandomState(1).randint(0, 255, (300, 280, 3))
    Image.fromarray(rgba, "RGBA").save(tmp_path / "subject.png")
    out = tmp_path / "out"
    base = ["--input_img", str(tmp_path / "subject.png"), "--exp_img", str(tmp_path / "kiss.jpg"), "--cfg", str(tmp_path / "facescape.yaml"),
            "--ckpt", str(tmp_path / "m.ckpt"), "--output_dir", str(out), "--sample_steps", "2", "--batch_view_num", "8",
            "--flame_model", str(tmp_path / "flame.npz"), "--fit_scan", str(tmp_path / "scan.ply")]
    with pytest.raises(SystemExit):
        GF.parse_args(base + ["--fit_mesh", str(tmp_path / "scan.ply")])
    model = GF.load_model(str(tmp_path / "facescape.yaml"), str(tmp_path / "m.ckpt"), device=DEV)
    strip, path = GF.run(GF.parse_args(base + ["--fit_iters", "300"]), model=model)
    assert sorted(p.name for p in out.iterdir()) == ["subject_kiss.png", "subject_kiss_fit.json", "subject_kiss_fit.npz"]
    assert path.endswith("subject_kiss.png") and strip.shape == (256, 17 * 256, 3)
    js = json.loads((out / "subject_kiss_fit.json").read_text())
    fitted = dict(np.load(out / "subject_kiss_fit.npz"))
    assert sorted(fitted) == sorted(GF.FLAME_FILE_KEYS) and js["iterations"] == 300 and js["vertices"] == 162
    assert js["scan_vertices"] == 642 and js["scan_faces"] == 1280 and js["matched"] == 1.0 and js["scan_to_mesh"]["matched"] == 1.0
    p = np.concatenate([fitted[k] for k in ("shape", "expression", "global_pose", "neck", "jaw", "eyes", "transl")])[None]
    first, last = R.surface_rms(m, np.zeros_like(p), scans), R.surface_rms(m, p, scans)
    print(f"--fit_scan: model-to-scan surface RMS {first} -> {last} (the file says {js['rms']:.3e}); scan to mesh {js['scan_to_mesh']}")
    assert (last <= 1e-2 * first).all() and abs(js["rms"] - last[0]) <= 1e-2 * last[0] + 1e-7
    assert 0 < js["scan_to_mesh"]["rms"] < 1e-2 * first[0] and js["scan_to_mesh"]["max"] >= js["scan_to_mesh"]["p90"] >= js["scan_to_mesh"]["median"]
    # with --flame_params the fit is the neutral end of a sweep
    out2 = tmp_path / "out2"
    args = [a if a != str(out) else str(out2) for a in base] + ["--fit_iters", "50", "--flame_params", str(tmp_path / "smile.npz"),
                                                                   "--frames", "2", "--frame_batch", "2", "--fit_scan_refresh", "5"]
    GF.run(GF.parse_args(args), model=model)
    assert sorted(p.name for p in out2.iterdir()) == ["subject_kiss_f00.png", "subject_kiss_f01.png", "subject_kiss_fit.json",
                                                      "subject_kiss_fit.npz"]
    assert json.loads((out2 / "subject_kiss_fit.json").read_text())["refresh"] == 5

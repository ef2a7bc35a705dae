"""GPU: the morphable-model fitter (MorphableModel.fit / fit_flame / vjp / differentiable over mvd_morph_fit_run and the per-op
entries) against the float64 loop of tests/morphable_bwd_ref.py.

Convergence is a condition: from zero, lr 0.05, 300 iterations, vertex term only, the vertex RMS must fall to at most 1e-3 of its
initial value (the float64 loop reaches 3e-7; tests/test_morphable_bwd_cpu.py checks that).  The trajectory after 20 and after 100
iterations may differ from the float64 loop by at most 4 times what the same loop run in float32 differs from it, on the same
inputs (printed here, quoted in DESIGN.md section 7).  Everything else is bit for bit."""
import json

import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import morphable as MM
from tests import morphable_bwd_ref as BR
from tests import morphable_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def model_of(m, **kw):
    return MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"],
                                         faces=m["faces"], lmk_face=m["lmk_face"], lmk_bary=m["lmk_bary"], device=DEV, **kw)


def case(V=257, NB=12, J=5, F=3, M=0, parents=None):
    m = R.synthetic_model(5, V, NB, J, M=M, parents=parents)
    betas, pose = R.seeded_params(7, F, NB, J)
    fw = BR.forward(BR.Folded(m), betas, pose)
    return m, model_of(m), fw["vertices"].astype(np.float32), None if fw["landmarks"] is None else fw["landmarks"].astype(np.float32)


def packed(fit):
    return torch.cat([fit["betas"], fit["pose"].reshape(fit["betas"].shape[0], -1), fit["transl"]], 1)


@pytest.mark.parametrize("V,NB,J,F", [(257, 12, 5, 3), (63, 7, 1, 1)])
def test_fit_meets_the_convergence_condition(V, NB, J, F):
    m, fm, target, _ = case(V, NB, J, F)
    fit = fm.fit(target_vertices=target, iters=300, lr=0.05)
    rest = fm.forward(torch.zeros(F, NB), torch.zeros(F, J, 3))["vertices"].cpu().numpy().astype(np.float64)
    first = np.sqrt(((rest - target) ** 2).sum(-1).mean(-1))
    last = fit["rms"].cpu().numpy().astype(np.float64)
    print(f"fit V={V} NB={NB} J={J}: vertex RMS {first} -> {last}, ratio {last / first}")
    assert fit["loss_history"].shape == (300, F) and torch.isfinite(fit["loss_history"]).all()
    assert fit["vertices"].shape == (F, V, 3) and fit["betas"].shape == (F, NB) and fit["pose"].shape == (F, J, 3)
    assert (last <= 1e-3 * first).all()
    # rms is the distance of the returned vertices
    again = np.sqrt(((fit["vertices"].cpu().numpy().astype(np.float64) - target) ** 2).sum(-1).mean(-1))
    assert np.allclose(again, last, rtol=1e-5)


def test_fit_follows_the_float64_trajectory():
    m, fm, target, _ = case()
    o64 = BR.fit_oracle(m, target=target, iters=100, lr=0.05, keep=(20, 100))
    o32 = BR.fit_oracle(m, target=target, iters=100, lr=0.05, keep=(20, 100), dtype=np.float32)
    for k in (20, 100):
        got = packed(fm.fit(target_vertices=target, iters=k, lr=0.05)).cpu().numpy().astype(np.float64)
        yard = np.abs(o32["snapshots"][k].astype(np.float64) - o64["snapshots"][k]).max()
        err = np.abs(got - o64["snapshots"][k]).max()
        print(f"fit after {k} iterations: worst parameter difference to the float64 loop {err:.3e}, float32 loop {yard:.3e}, "
              f"ratio {err / yard:.2f}")
        assert err <= 4 * yard, k
    # the loss history is the data term before each step
    hist = fm.fit(target_vertices=target, iters=20, lr=0.05)["loss_history"].cpu().numpy().astype(np.float64)
    assert np.allclose(hist, o64["loss_history"][:20], rtol=1e-3)


def test_fit_repeats_and_frames_are_independent():
    m, fm, target, _ = case()
    a, b = fm.fit(target_vertices=target, iters=40), fm.fit(target_vertices=target, iters=40)
    for k in ("betas", "pose", "transl", "vertices", "loss_history", "rms"):
        assert torch.equal(a[k], b[k]), k
    one = fm.fit(target_vertices=target[1:2], iters=40)
    for k in ("betas", "pose", "transl", "vertices"):
        assert torch.equal(a[k][1:2], one[k]), k
    assert torch.allclose(a["rms"][1:2], one["rms"], rtol=1e-5, atol=0)  # rms is a torch reduction over the returned vertices
    assert torch.equal(a["loss_history"][:, 1:2], one["loss_history"])


def test_fit_flame_frees_what_it_is_told_to():
    m = R.synthetic_model(5, 257, 12, 5, parents=[-1, 0, 1, 1, 1])
    fm = model_of(m, n_shape=8)
    betas, pose = R.seeded_params(7, 2, 12, 5)
    target = BR.forward(BR.Folded(m), betas, pose)["vertices"].astype(np.float32)
    init = {"shape": betas[:, :8], "global_pose": pose[:, 0], "neck": pose[:, 1], "eyes": pose[:, 3:].reshape(2, 6), "transl": [0.01, 0.0, -0.02]}
    fit = fm.fit_flame(target_vertices=target, free=("expression", "jaw"), init=init, iters=30, reg={"expression": 1e-6, "jaw": 1e-6})
    assert torch.equal(fit["shape"].cpu(), torch.from_numpy(betas[:, :8])) and torch.equal(fit["betas"][:, :8].cpu(), torch.from_numpy(betas[:, :8]))
    assert torch.equal(fit["global_pose"].cpu(), torch.from_numpy(pose[:, 0])) and torch.equal(fit["neck"].cpu(), torch.from_numpy(pose[:, 1]))
    assert torch.equal(fit["eyes"].cpu(), torch.from_numpy(pose[:, 3:].reshape(2, 6)))
    assert torch.equal(fit["transl"].cpu(), torch.tensor([[0.01, 0.0, -0.02]] * 2))
    assert fit["expression"].abs().max() > 0 and fit["jaw"].abs().max() > 0 and torch.equal(fit["jaw"], fit["pose"][:, 2])
    assert (fit["loss_history"][-1] < fit["loss_history"][0]).all()
    # flame() with the fitted parts gives the fitted vertices
    again = fm.flame(fit["shape"], fit["expression"], fit["global_pose"], fit["neck"], fit["jaw"], fit["eyes"], transl=fit["transl"])
    assert torch.equal(again["vertices"], fit["vertices"])


def test_fit_run_equals_the_ops_composed():
    m, fm, target, tl = case(M=9)
    F, NB, J, V = 3, fm.NB, fm.J, fm.V
    P = NB + 3 * J + 3
    rng = np.random.default_rng(1)
    lrv, lam, p0 = (dev(a.astype(np.float32)) for a in fm.fit_vectors(0.05, reg={"betas": 1e-3}, prior={"betas": rng.normal(size=NB)}))
    start = dev((rng.normal(size=(F, P)) * 0.05).astype(np.float32))
    tv, tld, post = dev(target), dev(tl), dev(MM.flame_alignment().numpy().astype(np.float32))
    vw, lw = dev(rng.random(V).astype(np.float32)), dev(rng.random(9).astype(np.float32))
    for kw in (dict(target=tv), dict(target=tv, vertex_weight=vw, target_lmk=tld, lmk_weight=lw, lmk_lambda=0.5, post=post),
               dict(target_lmk=tld[:1], lmk_lambda=2.0)):
        p, mm, vv = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
        hist = E.morph_fit_run(fm, p, mm, vv, lrv, lam, p0, 5, **kw)
        q, qm, qv = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
        post_k, use_l = kw.get("post"), "target_lmk" in kw
        for it in range(5):
            betas, pose, transl = q[:, :NB].contiguous(), q[:, NB:NB + 3 * J].reshape(F, J, 3).contiguous(), q[:, NB + 3 * J:].contiguous()
            pr = E.op_morph_pose(betas, pose, fm.j_template, fm.j_dirs, fm.parents)
            coef = torch.cat([betas, pr["pose_feature"]], 1)
            verts, blend = E.op_morph_skin_ex(fm.basis, fm.v_template, coef, fm.weights, pr["A"], post=post_k, transl=transl, want_blend=True)
            lmk = E.op_morph_landmarks(verts, fm.faces, fm.lmk_face, fm.lmk_bary) if use_l else None
            Ef, g_y = E.op_morph_fit_data(verts, target=kw.get("target"), vertex_weight=kw.get("vertex_weight"), lmk=lmk,
                                          target_lmk=kw.get("target_lmk"), lmk_weight=kw.get("lmk_weight"),
                                          lmk_lambda=kw.get("lmk_lambda", 1.0), csr=(fm.csr_ptr, fm.csr_ent, fm.lmk_bary) if use_l else None)
            assert torch.equal(Ef, hist[it]), it
            sb = E.op_morph_skin_bwd(g_y, fm.weights, pr["A"], blend, fm.basis, post=post_k)
            g = E.op_morph_pose_bwd(pose, pr["j_rest"], pr["A"], fm.j_dirs, fm.parents, sb["part_a"], sb["part_c"])
            E.op_morph_fit_update(q, torch.cat([g["betas"], g["pose"].reshape(F, -1), g["transl"]], 1), qm, qv, lrv, lam, p0, it + 1)
        assert torch.equal(p, q) and torch.equal(mm, qm) and torch.equal(vv, qv)
        assert not torch.equal(p, start)


def test_differentiable_backward_is_the_vjp():
    m, fm, _, _ = case(M=9)
    betas, pose = (dev(a) for a in R.seeded_params(3, 3, fm.NB, fm.J, zero_pose_frames=(2,)))
    transl = dev(np.random.default_rng(0).normal(size=(3, 3)).astype(np.float32) * 0.02)
    post = dev(MM.flame_alignment().numpy().astype(np.float32))
    g = torch.Generator().manual_seed(0)
    gv, gj, gl = (torch.randn(s, generator=g).to(DEV) for s in ((3, fm.V, 3), (3, fm.J, 3), (3, 9, 3)))
    for use_post, use_t in ((None, None), (post, transl)):
        b, p = betas.clone().requires_grad_(), pose.clone().requires_grad_()
        t = None if use_t is None else use_t.clone().requires_grad_()
        out = fm.differentiable(b, p, post=use_post, transl=t)
        plain = fm.forward(betas, pose, post=use_post, transl=use_t)
        assert all(torch.equal(out[k].detach(), plain[k]) for k in ("vertices", "joints", "landmarks"))
        ((out["vertices"] * gv).sum() + (out["joints"] * gj).sum() + (out["landmarks"] * gl).sum()).backward()
        want = fm.vjp(betas, pose, grad_vertices=gv, grad_joints=gj, grad_landmarks=gl, post=use_post, transl=use_t)
        assert torch.equal(b.grad, want["betas"]) and torch.equal(p.grad, want["pose"])
        assert t is None or torch.equal(t.grad, want["transl"])
        # a loss on the vertices alone, written in torch
        b2 = betas.clone().requires_grad_()
        fm.differentiable(b2, pose, post=use_post, transl=use_t)["vertices"].square().sum().backward()
        v = plain["vertices"]
        assert torch.equal(b2.grad, fm.vjp(betas, pose, grad_vertices=2 * v, post=use_post, transl=use_t)["betas"])
    # and it is the gradient: against the float64 oracle, within 4 x the oracle's own float32 error
    fo = BR.Folded(m)
    cot = dict(g_verts=gv.cpu().numpy(), g_joints=gj.cpu().numpy(), g_lmk=gl.cpu().numpy())
    args = (betas.cpu().numpy(), pose.cpu().numpy())
    w64 = BR.vjp(fo, *args, transl=transl.cpu().numpy(), post=post.cpu().numpy(), **cot)
    w32 = BR.vjp(BR.Folded(m, np.float32), *args, transl=transl.cpu().numpy(), post=post.cpu().numpy(), **cot)
    got = fm.vjp(betas, pose, grad_vertices=gv, grad_joints=gj, grad_landmarks=gl, post=post, transl=transl)
    for k in ("betas", "pose", "transl"):
        err = np.abs(got[k].cpu().numpy().astype(np.float64) - w64[k]).max()
        yard = np.abs(w32[k].astype(np.float64) - w64[k]).max()
        print(f"vjp g_{k}: worst error {err:.3e}, float32 oracle {yard:.3e}, ratio {err / yard:.2f}")
        assert err <= 4 * yard, k


def test_a_landmark_only_fit_lowers_the_landmark_residual():
    m, fm, _, tl = case(M=9)
    res = lambda l: np.sqrt(((l.cpu().numpy().astype(np.float64) - tl) ** 2).sum(-1).mean(-1))
    first = res(fm.forward(torch.zeros(3, fm.NB), torch.zeros(3, fm.J, 3))["landmarks"])
    fit = fm.fit(target_landmarks=tl, lmk_lambda=2.0, iters=60, reg={"betas": 1e-4})
    last = res(fm.forward(fit["betas"], fit["pose"], transl=fit["transl"])["landmarks"])
    print(f"landmark-only fit: landmark RMS {first} -> {last}")
    assert (last < first).all() and np.allclose(fit["rms"].cpu().numpy(), last, rtol=1e-5)
    assert (fit["loss_history"][-1] < fit["loss_history"][0]).all()


def test_generate_face_fits_a_mesh_and_sweeps_from_the_fit(tmp_path):
    import yaml
    from PIL import Image
    from morphablediffusion_amd import generate_face as GF
    from morphablediffusion_amd.mesh import write_ply
    from morphablediffusion_amd.spec import (ClipConfig, UNetConfig, VaeConfig, VolumeConfig, clip_manifest, full_manifest,
                                             vae_decoder_manifest, vae_encoder_manifest)
    from morphablediffusion_amd.weights import seeded_state_dict
    from tests import mesh_ref
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
    V, NB = len(sv), 10
    m = R.synthetic_model(31, V, NB, 5, parents=[-1, 0, 1, 1, 1])
    kt = np.array([[2 ** 32 - 1, 0, 1, 1, 1], [0, 1, 2, 3, 4]], dtype=np.uint32)
    np.savez(tmp_path / "flame.npz", v_template=sv.astype(np.float32), shapedirs=m["shapedirs"], posedirs=m["posedirs"],
             J_regressor=m["J_regressor"], kintree_table=kt, weights=m["weights"], f=sf)
    # the mesh to fit: the model at known parameters, moved a little, as a tracker would export it
    fm = MM.MorphableModel.load(tmp_path / "flame.npz", device=DEV)
    g = np.random.default_rng(2)
    known = dict(shape=g.normal(size=NB), global_pose=np.array([0.1, -0.2, 0.05]), jaw=np.array([0.25, 0.0, 0.0]),
                 transl=np.array([0.01, -0.02, 0.015]))
    mesh = fm.flame(**known)["vertices"][0].cpu().double().numpy()
    write_ply(str(tmp_path / "tracked.ply"), mesh, sf)
    np.savez(tmp_path / "smile.npz", jaw=np.array([0.4, 0.0, 0.0]))
    rgba = np.full((300, 280, 4), 255, np.uint8)
    rgba[..., :3] = np.random.RandomState(1).randint(0, 255, (300, 280, 3))
    Image.fromarray(rgba, "RGBA").save(tmp_path / "subject.png")
    out = tmp_path / "out"
    base = ["--input_img", str(tmp_path / "subject.png"), "--exp_img", str(tmp_path / "kiss.jpg"), "--cfg", str(tmp_path / "facescape.yaml"),
            "--ckpt", str(tmp_path / "m.ckpt"), "--output_dir", str(out), "--sample_steps", "2", "--batch_view_num", "8",
            "--flame_model", str(tmp_path / "flame.npz"), "--fit_mesh", str(tmp_path / "tracked.ply")]
    model = GF.load_model(str(tmp_path / "facescape.yaml"), str(tmp_path / "m.ckpt"), device=DEV)
    strip, path = GF.run(GF.parse_args(base + ["--fit_iters", "300"]), model=model)
    assert sorted(p.name for p in out.iterdir()) == ["subject_kiss.png", "subject_kiss_fit.json", "subject_kiss_fit.npz"]
    assert path.endswith("subject_kiss.png") and strip.shape == (256, 17 * 256, 3)
    js = json.loads((out / "subject_kiss_fit.json").read_text())
    fitted = dict(np.load(out / "subject_kiss_fit.npz"))
    assert sorted(fitted) == sorted(GF.FLAME_FILE_KEYS) and js["iterations"] == 300 and js["vertices"] == V
    got = fm.flame(**fitted)["vertices"][0].cpu().double().numpy()
    rms = lambda a: float(np.sqrt(((a - mesh) ** 2).sum(-1).mean()))
    first, last = rms(sv.astype(np.float32).astype(np.float64)), rms(got)
    print(f"--fit_mesh: vertex RMS {first:.3e} -> {last:.3e} (the file says {js['rms']:.3e})")
    assert last <= 1e-3 * first and abs(js["rms"] - last) <= 1e-3 * last + 1e-9
    assert set(GF.load_flame_params(out / "subject_kiss_fit.npz")) == set(GF.FLAME_FILE_KEYS)  # transl is a seventh key
    # with --flame_params the fit is the neutral end of a sweep
    out2 = tmp_path / "out2"
    args = [a if a != str(out) else str(out2) for a in base] + ["--fit_iters", "50", "--flame_params", str(tmp_path / "smile.npz"),
                                                                   "--frames", "2", "--frame_batch", "2", "--export_mesh"]
    GF.run(GF.parse_args(args), model=model)
    names = sorted(p.name for p in out2.iterdir())
    assert names == sorted([f"subject_kiss_f{f:02d}{s}" for f in range(2) for s in (".png", "_mesh.ply", "_mesh.json")] +
                           ["subject_kiss_fit.json", "subject_kiss_fit.npz"])
    from morphablediffusion_amd.mesh import read_mesh
    f2 = dict(np.load(out2 / "subject_kiss_fit.npz"))
    ends = {0: f2, 1: dict(f2, jaw=np.array([0.4, 0.0, 0.0]))}
    for f, prm in ends.items():  # frame 0 is the fit, frame 1 its identity, global pose and translation with the given jaw
        v, _ = read_mesh(out2 / f"subject_kiss_f{f:02d}_mesh.ply")
        assert np.array_equal(v, fm.flame(**prm)["vertices"][0].cpu().double().numpy()), f
    # a mesh of another topology is refused, and both counts are named
    write_ply(str(tmp_path / "other.ply"), mesh[:-1], sf[(sf < V - 1).all(1)])
    bad = [a if a != str(tmp_path / "tracked.ply") else str(tmp_path / "other.ply") for a in base]
    with pytest.raises(ValueError, match=f"{V - 1} vertices, the model {V}"):
        GF.run(GF.parse_args(bad), model=model)

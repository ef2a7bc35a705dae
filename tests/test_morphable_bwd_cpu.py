"""CPU: the oracle of the morphable-model backward (tests/morphable_bwd_ref.py) against the reference's own autograd run recorded
in tests/golden/morphable_lbs_bwd.npz and against central differences of morphable_ref.forward; the landmark table; the packing
of free / reg / prior into the optimiser's vectors and the Python argument errors (a model on device="cpu" is enough); the argument
errors of the new entry points, which return before the first HIP call; and the fitter's convergence condition for the oracle.

Agreement between two float64 evaluations is measured (and printed), and asserted at 16 times the value measured when the test was
written: golden 9.9e-16 of the largest entry, central differences (fourth-order stencil, h = 1e-3, six random directions) 1.6e-12.
A wrong formula shows at 1e-3 or more."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from morphablediffusion_amd import morphable as MM
from tests import morphable_bwd_ref as BR
from tests import morphable_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_AGREEMENT, DIFFERENCE_AGREEMENT = 16 * 9.9e-16, 16 * 1.6e-12


def golden():
    g = {}
    for name in ("morphable_lbs.npz", "morphable_lbs_bwd.npz"):
        with np.load(os.path.join(HERE, "golden", name)) as z:
            g.update({k: z[k] for k in z.files})
    g["parents"] = [int(p) for p in g["parents"]]
    return g


def test_oracle_vjp_equals_the_reference_autograd():
    g = golden()
    fm = BR.Folded(g)
    whole = BR.vjp(fm, g["betas"], g["pose"], g_verts=g["g_verts"], g_joints=g["g_joints"], g_lmk=g["g_lmk"])
    pose = BR.pose_vjp(g["betas"], g["pose"], fm.jt, fm.jd, fm.parents, g_A=g["g_A"], g_joints=g["g_joints"], g_pose_feature=g["g_pf"])
    for name, got in (("whole", whole), ("pose", pose)):
        for k in ("betas", "pose"):
            want = g[f"{name}_{k}_f64"]
            assert want.dtype == np.float64 and want.shape == got[k].shape
            rel = np.abs(got[k] - want).max() / np.abs(want).max()
            print(f"{name} {k}: oracle against the reference's float64 autograd: {rel:.3e} of the largest entry")
            assert rel < 1e-10 and rel <= GOLDEN_AGREEMENT
            err = g[f"ref_err_{name}_{k}"]
            assert err == np.abs(g[f"{name}_{k}_f32"].astype(np.float64) - want).max() and 0 < err < 1e-5


@pytest.mark.parametrize("post", [False, True])
def test_oracle_vjp_equals_central_differences(post):
    g = golden()
    fm = BR.Folded(g)
    post = MM.flame_alignment().numpy() if post else None
    rng = np.random.default_rng(3)
    b0, p0, t0 = g["betas"].astype(np.float64), g["pose"].astype(np.float64), rng.normal(size=(3, 3)) * 0.01
    cot = (g["g_verts"], g["g_joints"], g["g_lmk"])
    got = BR.vjp(fm, b0, p0, transl=t0, post=post, g_verts=cot[0], g_joints=cot[1], g_lmk=cot[2])

    def loss(b, p, t):  # morphable_ref.forward knows no translation: it moves the vertices and landmarks by post's linear part
        o = R.forward(g, b, p, post)
        shift = t if post is None else t @ post[:, :3].T
        return (cot[0] * (o["vertices"] + shift[:, None])).sum() + (cot[1] * o["joints"]).sum() + \
            (cot[2] * (o["landmarks"] + shift[:, None] * g["lmk_bary"].astype(np.float64).sum(1)[None, :, None])).sum()

    worst, h = 0.0, 1e-3
    for _ in range(6):
        db, dp, dt = rng.normal(size=b0.shape), rng.normal(size=p0.shape) * 0.3, rng.normal(size=t0.shape)
        f = lambda s: loss(b0 + s * h * db, p0 + s * h * dp, t0 + s * h * dt)
        num = (-f(2) + 8 * f(1) - 8 * f(-1) + f(-2)) / (12 * h)
        ana = (got["betas"] * db).sum() + (got["pose"] * dp).sum() + (got["transl"] * dt).sum()
        worst = max(worst, abs(num - ana) / abs(ana))
    print(f"post={post is not None}: directional derivative against central differences: {worst:.3e}")
    assert worst < 1e-10 and worst <= DIFFERENCE_AGREEMENT


def test_gradient_at_a_zero_pose_is_finite_and_the_rotation_generators():
    for dt in (np.float64, np.float32):
        gR = np.arange(9.0).reshape(3, 3)
        got = BR.rodrigues_vjp(np.zeros(3), gR, dt)
        assert got.dtype == dt and np.isfinite(got).all()
        want = np.array([gR[2, 1] - gR[1, 2], gR[0, 2] - gR[2, 0], gR[1, 0] - gR[0, 1]])  # d/dr_i of exp(K(r)) at 0: the generators
        assert np.abs(got - want).max() < 1e-6 * np.abs(want).max()
    g = golden()
    fm = BR.Folded(g)
    out = BR.vjp(fm, g["betas"], np.zeros_like(g["pose"]), g_verts=g["g_verts"], g_joints=g["g_joints"], g_lmk=g["g_lmk"])
    assert all(np.isfinite(v).all() for v in out.values()) and np.abs(out["pose"]).max() > 0


def test_landmark_table_equals_a_brute_force_scatter():
    rng = np.random.default_rng(0)
    V, Nf, M = 40, 30, 25
    faces = rng.integers(0, V, (Nf, 3))
    faces[3] = (7, 8, 9)
    faces[4] = (9, 10, 11)  # faces 3 and 4 share vertex 9
    lmk_face = rng.integers(0, Nf, M)
    lmk_face[:4] = (3, 3, 4, 3)  # landmarks on one face, and on faces that share a vertex
    bary = rng.random((M, 3))
    ptr, ent = E.landmark_csr(faces, lmk_face, bary, V)
    want = BR.landmark_entries(faces, lmk_face, V)
    assert ptr.dtype == np.int32 and ent.dtype == np.int32 and ptr.shape == (V + 1,) and ent.shape == (3 * M,) and ptr[0] == 0
    for v in range(V):
        assert list(ent[ptr[v]:ptr[v + 1]]) == want[v], v
    assert len(want[9]) >= 4 and sorted(ent.tolist()) == list(range(3 * M))
    # the gather through the table is the scatter
    g_lmk = rng.normal(size=(2, M, 3))
    scat, _ = BR.landmarks_bwd(g_lmk, faces, lmk_face, bary, V)
    gath = np.zeros((2, V, 3))
    for v in range(V):
        for e in ent[ptr[v]:ptr[v + 1]]:
            gath[:, v] += bary[e // 3, e % 3] * g_lmk[:, e // 3]
    assert np.abs(gath - scat).max() < 1e-14
    with pytest.raises(ValueError, match="outside"):
        E.landmark_csr(faces + V, lmk_face, bary, V)


def flame_like(device="cpu", M=4):
    m = R.synthetic_model(11, 31, 10, 5, parents=[-1, 0, 1, 1, 1], M=M)
    return MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"],
                                         faces=m["faces"], lmk_face=m["lmk_face"], lmk_bary=m["lmk_bary"], device=device, n_shape=6)


def test_fit_vectors_pack_free_reg_and_prior():
    fm = flame_like()
    P = 10 + 15 + 3
    g = fm.param_groups()
    assert g["shape"] == slice(0, 6) and g["expression"] == slice(6, 10) and g["jaw"] == slice(16, 19) and g["transl"] == slice(25, 28)
    assert fm.csr_ptr.shape == (32,) and fm.csr_ent.shape == (12,)
    lr, lam, p0 = fm.fit_vectors()
    assert lr.shape == lam.shape == p0.shape == (P,) and (lr == 0.05).all() and not lam.any() and not p0.any()
    lr, lam, p0 = fm.fit_vectors(fit_transl=False)
    assert (lr[:25] == 0.05).all() and not lr[25:].any()
    shape = np.arange(6.0) + 1
    lr, lam, p0 = fm.fit_vectors(0.01, free=("expression", "jaw"), reg={"shape": 1e-4, "expression": 2e-4, "jaw": 3e-4},
                                 prior={"shape": shape})
    want = np.zeros(P)
    want[6:10] = want[16:19] = 0.01
    assert np.array_equal(lr, want)
    assert np.array_equal(lam[:6], np.full(6, 1e-4)) and np.array_equal(lam[6:10], np.full(4, 2e-4)) and np.array_equal(lam[16:19], np.full(3, 3e-4))
    assert lam.sum() == pytest.approx(6e-4 + 8e-4 + 9e-4) and np.array_equal(p0[:6], shape) and not p0[6:].any()
    # a frozen part starts at its prior, init overrides
    start = fm._fit_init("t", {"jaw": [0.1, 0.2, 0.3]}, 2, p0, lr)
    assert start.shape == (2, P) and np.array_equal(start[1, :6], shape) and np.array_equal(start[0, 16:19], [0.1, 0.2, 0.3])
    lr, _, _ = fm.fit_vectors(free=("betas", "transl"))
    assert (lr[:10] == 0.05).all() and not lr[10:25].any() and (lr[25:] == 0.05).all()


def test_fit_argument_errors_come_before_the_device():
    fm = flame_like()
    tv = np.zeros((2, 31, 3), np.float32)
    bad = [dict(free=("nose",)), dict(free="jaw"), dict(reg={"jaw": -1.0}), dict(reg={"chin": 1.0}), dict(prior={"shape": np.zeros(5)}),
           dict(prior={"brow": np.zeros(3)}), dict(lr=0.0), dict(free=("transl",), fit_transl=False), dict(iters=0),
           dict(init={"tongue": np.zeros(3)}), dict(init={"jaw": np.zeros(4)})]
    for kw in bad:
        with pytest.raises(ValueError):
            fm.fit_flame(target_vertices=tv, **kw)
    with pytest.raises(ValueError, match="target_vertices, target_landmarks or both"):
        fm.fit_flame()
    with pytest.raises(ValueError, match="topology"):
        fm.fit_flame(target_vertices=np.zeros((2, 30, 3), np.float32))
    with pytest.raises(ValueError, match="target_landmarks must be"):
        fm.fit_flame(target_landmarks=np.zeros((2, 5, 3), np.float32))
    with pytest.raises(ValueError, match="same number of frames"):
        fm.fit_flame(target_vertices=tv, target_landmarks=np.zeros((3, 4, 3), np.float32))
    with pytest.raises(ValueError, match="GPU only"):
        fm.fit_flame(target_vertices=tv)
    with pytest.raises(ValueError, match="GPU only"):
        fm.vjp(torch.zeros(2, 10), torch.zeros(2, 5, 3), grad_vertices=torch.zeros(2, 31, 3))
    with pytest.raises(ValueError, match="no landmark embedding"):
        flame_like(M=0).fit(target_landmarks=np.zeros((1, 4, 3), np.float32))
    m = R.synthetic_model(1, 9, 3, 2)
    two = MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"],
                                        device="cpu")
    with pytest.raises(ValueError, match="FLAME model has 5 joints"):
        two.fit_flame(target_vertices=np.zeros((1, 9, 3), np.float32))
    assert sorted(two.param_groups()) == ["betas", "pose", "transl"]
    with pytest.raises(ValueError, match="transl must be"):
        flame_like_cuda_stub()._params("t", torch.zeros(2, 10), torch.zeros(2, 5, 3), torch.zeros(3, 3))


def flame_like_cuda_stub():
    """A CPU model that claims a GPU, for the shape errors that come after the device check and before any launch."""
    fm = flame_like()
    fm.device = torch.device("cuda:0")
    return fm


def test_engine_wrappers_refuse_bad_shapes_before_anything_is_copied():
    z = torch.zeros
    with pytest.raises(ValueError, match="transl"):
        E.op_morph_skin_ex(z(7, 9), z(3, 3), z(2, 7), z(3, 1), z(2, 1, 12), transl=z(3, 3))
    with pytest.raises(ValueError, match="blend"):
        E.op_morph_skin_bwd(z(2, 3, 3), z(3, 1), z(2, 1, 12), z(2, 4, 3), z(7, 9))
    with pytest.raises(ValueError, match="part_a"):
        E.op_morph_pose_bwd(z(2, 2, 3), z(2, 2, 3), z(2, 2, 12), z(4, 6), [-1, 0], z(1, 2, 26), z(1, 2, 13))
    with pytest.raises(ValueError, match="parents"):
        E.op_morph_pose_bwd(z(2, 2, 3), z(2, 2, 3), z(2, 2, 12), z(4, 6), [-1, 1], z(1, 2, 27), z(1, 2, 13))
    ptr, ent = torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="csr_ptr"):
        E.op_morph_landmarks_bwd(z(2, 1, 3), ptr.long(), ent, z(1, 3), 3)
    with pytest.raises(ValueError, match="g_lmk"):
        E.op_morph_landmarks_bwd(z(2, 2, 3), ptr, ent, z(1, 3), 3)
    with pytest.raises(ValueError, match="give target"):
        E.op_morph_fit_data(z(2, 3, 3))
    with pytest.raises(ValueError, match="1 or F"):
        E.op_morph_fit_data(z(3, 3, 3), target=z(2, 3, 3))
    with pytest.raises(ValueError, match="vertex_weight without"):
        E.op_morph_fit_data(z(3, 3, 3), vertex_weight=z(3), lmk=z(3, 1, 3), target_lmk=z(1, 1, 3), csr=(ptr, ent, z(1, 3)))
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        E.op_morph_fit_update(z(2, 4), z(2, 4), z(2, 4), z(2, 4), z(4), z(4), z(4), 1)


def test_entry_points_refuse_bad_arguments_before_the_first_hip_call():
    lib = L.load()
    buf = (C.c_float * 4096)()
    par = (C.c_int32 * 2)(-1, 0)
    bad_par = (C.c_int32 * 2)(-1, 1)
    ip = (C.c_int32 * 8)()
    p, i = C.addressof(buf), C.addressof(ip)

    def fails(rc, text):
        assert rc != 0 and text in lib.mvd_last_error().decode(), lib.mvd_last_error().decode()

    assert lib.mvd_morph_bwd_chunks(1) == 1 and lib.mvd_morph_bwd_chunks(256) == 1 and lib.mvd_morph_bwd_chunks(257) == 2
    assert lib.mvd_morph_bwd_slabs(85) == 1 and lib.mvd_morph_bwd_slabs(86) == 2 and lib.mvd_morph_bwd_slabs(0) == 0
    n = C.c_int64(0)
    assert lib.mvd_morph_fit_workspace(1, 1, 1, 1, 0, C.addressof(n)) == 0 and n.value > 0
    fails(lib.mvd_morph_fit_workspace(1, 1, 1, 65, 0, C.addressof(n)), "J in 1..64")
    fails(lib.mvd_morph_fit_workspace(1, 1, 1, 1, 0, None), "null argument")
    fails(lib.mvd_op_morph_skin_ex(p, p, p, p, p, None, None, 1, 1, 2, 1, 1, p, None, None), "L must be NB + 9 (J - 1)")
    fails(lib.mvd_op_morph_skin_ex(p, p, p, p, p, None, None, 1, 1, 1, 1, 1, None, None, None), "null argument")
    fails(lib.mvd_op_morph_skin_bwd(p, None, p, p, None, p, 1, 1, 1, 1, 1, p, p, p, None), "null argument")
    fails(lib.mvd_op_morph_skin_bwd(p, None, p, p, p, p, 1, 1, 1, 1, 65, p, p, p, None), "J must be in 1..64")
    fails(lib.mvd_op_morph_skin_bwd(p, None, p, p, p, p, 0, 1, 1, 1, 1, p, p, p, None), "at least 1")
    fails(lib.mvd_op_morph_pose_bwd(p, p, p, p, C.addressof(bad_par), p, 1, p, 1, None, 1, 1, 2, p, p, p, None), "parents[j]")
    fails(lib.mvd_op_morph_pose_bwd(p, p, p, p, C.addressof(par), p, 0, p, 1, None, 1, 1, 2, p, p, p, None), "at least 1")
    fails(lib.mvd_op_morph_pose_bwd(p, p, p, p, C.addressof(par), None, 1, p, 1, None, 1, 1, 2, p, p, p, None), "null argument")
    fails(lib.mvd_op_morph_landmarks_bwd(p, None, i, i, p, 1, 1, 0, 1, p, None), "at least 1")
    fails(lib.mvd_op_morph_landmarks_bwd(p, None, None, i, p, 1, 1, 1, 1, p, None), "null argument")
    fails(lib.mvd_op_morph_fit_data(p, None, 1, None, 1.0, None, None, 1, None, 0.0, None, None, None, 1, 1, 0, 0, p, p, p, None),
          "neither a vertex nor a landmark target")
    fails(lib.mvd_op_morph_fit_data(p, p, 2, None, 1.0, None, None, 1, None, 0.0, None, None, None, 3, 1, 0, 0, p, p, p, None), "1 or F frames")
    fails(lib.mvd_op_morph_fit_data(p, None, 1, None, 1.0, None, p, 1, None, 1.0, None, None, None, 1, 1, 1, 1, p, p, p, None),
          "a landmark target needs")
    fails(lib.mvd_op_morph_fit_update(p, p, p, p, p, p, p, 1, 4, 0, 0.9, 0.999, 1e-8, None), "step must be at least 1")
    fails(lib.mvd_op_morph_fit_update(p, p, p, p, p, p, p, 1, 4, 1, 1.0, 0.999, 1e-8, None), "beta1 and beta2")
    fails(lib.mvd_op_morph_fit_update(p, None, p, p, p, p, p, 1, 4, 1, 0.9, 0.999, 1e-8, None), "null argument")
    run = lambda **kw: lib.mvd_morph_fit_run(*[kw.get(k, d) for k, d in (
        ("basis", p), ("vt", p), ("w", p), ("jt", p), ("jd", p), ("par", C.addressof(par)), ("post", None), ("faces", None), ("lf", None),
        ("bary", None), ("cp", None), ("ce", None), ("F", 1), ("V", 1), ("NB", 1), ("J", 2), ("Nf", 0), ("M", 0), ("n_ent", 0),
        ("target", p), ("tf", 1), ("vw", None), ("ivw", 1.0), ("tl", None), ("tlf", 1), ("lw", None), ("ls", 0.0), ("p", p), ("m", p),
        ("v", p), ("lr", p), ("lam", p), ("p0", p), ("iters", 1), ("step0", 0), ("b1", 0.9), ("b2", 0.999), ("eps", 1e-8), ("ws", p),
        ("nws", 4096), ("hist", p), ("stream", None))])
    fails(run(iters=0), "iters must be at least 1")
    fails(run(nws=8), "workspace is smaller")
    fails(run(ws=None), "null argument")
    fails(run(par=C.addressof(bad_par)), "parents[j]")
    fails(run(target=None), "neither a vertex nor a landmark target")
    fails(run(tl=p), "needs the landmark embedding")
    fails(run(lr=None), "null argument")
    fails(run(J=65), "J in 1..64")


@pytest.mark.parametrize("V,NB,J,F", [(257, 12, 5, 3), (63, 7, 1, 1)])
def test_the_oracle_meets_the_convergence_condition(V, NB, J, F):
    """Start at zero, lr 0.05, 300 iterations, vertex term only, each frame's loss its own: the vertex RMS falls to at most 1e-3 of
    its initial value.  A condition, not a measurement; the float64 loop clears it by more than three orders of magnitude."""
    m = R.synthetic_model(5, V, NB, J)
    betas, pose = R.seeded_params(7, F, NB, J)
    target = BR.forward(BR.Folded(m), betas, pose)["vertices"]
    fit = BR.fit_oracle(m, target=target, iters=300, lr=0.05)
    first, last = BR.vertex_rms(m, np.zeros_like(fit["p"]), target), BR.vertex_rms(m, fit["p"], target)
    print(f"V={V} NB={NB} J={J}: vertex RMS {first} -> {last}")
    assert (last <= 1e-3 * first).all() and (last <= 1e-5 * first).all()
    assert (fit["loss_history"][-1] < fit["loss_history"][0] * 1e-6).all()


def test_fit_mesh_flag_rules(tmp_path, capsys):
    from morphablediffusion_amd import generate_face as GF
    base = ["--input_img", "a.png", "--exp_img", "b.png", "--output_dir", str(tmp_path)]
    fit = ["--flame_model", "f.npz", "--fit_mesh", "t.ply"]
    flags = GF.parse_args(base + fit)
    assert flags.fit_mesh == "t.ply" and (flags.fit_iters, flags.fit_lr, flags.frames) == (300, 0.05, 1) and flags.flame_params is None
    flags = GF.parse_args(base + fit + ["--flame_params", "p.npz", "--frames", "3", "--fit_iters", "40", "--fit_lr", "0.1"])
    assert (flags.frames, flags.fit_iters, flags.fit_lr) == (3, 40, 0.1)
    assert GF.parse_args(base + ["--mesh", "m.ply"]).fit_mesh is None
    for bad in (base + ["--fit_mesh", "t.ply"], base + fit + ["--mesh", "m.ply"], base + fit + ["--neutral_params", "n.npz"],
                base + fit + ["--frames", "3"], base + fit + ["--fit_iters", "0"], base + fit + ["--fit_lr", "0"],
                base + fit + ["--flame_params", "p.npz", "--frames", "0"]):
        with pytest.raises(SystemExit):
            GF.parse_args(bad)
    capsys.readouterr()
    np.savez(tmp_path / "p.npz", shape=np.zeros(3), transl=np.zeros(3))
    assert set(GF.load_flame_params(tmp_path / "p.npz")) == {"shape", "transl"}
    np.savez(tmp_path / "q.npz", translation=np.zeros(3))
    with pytest.raises(ValueError, match="translation"):
        GF.load_flame_params(tmp_path / "q.npz")

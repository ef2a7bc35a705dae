"""CPU: the morphable-model oracle (tests/morphable_ref.py) against the reference's own float64 run recorded in
tests/golden/morphable_lbs.npz (which checks the folds of the joint regressor and the re-packed basis), the host side of
morphablediffusion_amd/morphable.py (loaders, restricted unpickler, column selection, alignment, interpolation), the Python
argument checks, and the argument errors of the three entry points, which return before the first HIP call."""
import ctypes as C
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

from morphablediffusion_amd import batch as B
from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from morphablediffusion_amd import morphable as MM
from tests import morphable_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morphable_lbs.npz")


def golden():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    g["parents"] = [int(p) for p in g["parents"]]
    return g


def test_oracle_equals_the_reference_float64_run():
    g = golden()
    out = R.forward(g, g["betas"], g["pose"])
    for k in ("A", "joints", "vertices", "landmarks"):
        want = g[k + "_f64"]
        assert want.dtype == np.float64
        rel = np.abs(out[k] - want).max() / np.abs(want).max()
        assert rel < 1e-12, (k, rel)
    # the frame at rest: the rotations are exact; the textbook chain leaves its translations at rounding level, not at zero
    assert (g["pose"][1] == 0).all() and np.array_equal(out["A"][1][..., :3], np.tile(np.eye(3), (5, 1, 1)))
    assert np.abs(out["A"][1][..., 3]).max() < 1e-16
    # the recorded float32 errors are those of the recorded runs
    for k in ("A", "joints", "vertices", "landmarks"):
        assert g["ref_err_" + k] == np.abs(g[k + "_f32"].astype(np.float64) - g[k + "_f64"]).max() and 0 < g["ref_err_" + k] < 1e-6


def test_rodrigues_at_zero_is_the_identity_exactly():
    for dt in (np.float64, np.float32):
        r = R.rodrigues(np.zeros((2, 3)), dt)
        assert r.dtype == dt and np.array_equal(r, np.tile(np.eye(3), (2, 1, 1)))
    q = R.rodrigues(np.array([0.3, -0.2, 0.5]))
    assert np.abs(q @ q.T - np.eye(3)).max() < 1e-7 and abs(np.linalg.det(q) - 1) < 1e-7  # the 1e-8 of the formula shows here


def test_skin_bound_dominates_a_float32_evaluation():
    """The bound is for any fp32 order: numpy's own float32 evaluation of the same sums stays inside it, and not by orders."""
    m = R.synthetic_model(5, 63, 7, 5, M=0)
    betas, pose = R.seeded_params(6, 3, 7, 5)
    jt, jd, basis = (a.astype(np.float32) for a in R.fold(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"]))
    p = R.pose(betas, pose, jt, jd, m["parents"])
    A, coef = p["A"].astype(np.float32), np.concatenate([betas, p["pose_feature"]], 1).astype(np.float32)
    post = MM.flame_alignment().numpy().astype(np.float32)
    want, bound = R.skin(basis, m["v_template"], coef, m["weights"], A, post)
    b = (m["v_template"].reshape(1, -1) + coef @ basis).reshape(3, 63, 3)
    T = np.einsum("vj,fje->fve", m["weights"], A.reshape(3, 5, 12)).reshape(3, 63, 3, 4)
    o = np.einsum("fvik,fvk->fvi", T[..., :3], b) + T[..., 3]
    o = np.einsum("ik,fvk->fvi", post[:, :3], o) + post[:, 3]
    assert o.dtype == np.float32
    err = np.abs(o - want)
    assert (err <= bound).all() and err.max() > bound.max() / 1000


def test_flame_alignment_equals_align_flame_vertices():
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(200, 3, generator=g) - 0.5) * 0.25  # a head in metres
    M = MM.flame_alignment()
    assert M.dtype == torch.float64 and tuple(M.shape) == (3, 4)
    got = x.double() @ M[:, :3].T + M[:, 3]
    want = B.align_flame_vertices(x)
    # align_flame_vertices rounds after each of its five fp32 steps, at magnitudes below 1
    assert (got - want.double()).abs().max() < 8 * 2.0 ** -24


def test_interpolate_params_end_points_are_exact():
    g = np.random.default_rng(1)
    a = {"shape": g.normal(size=9), "jaw": g.normal(size=3)}
    b = {"shape": g.normal(size=9), "expression": g.normal(size=4)}
    out = MM.interpolate_params(a, b, 5)
    assert set(out) == {"shape", "jaw", "expression"} and all(v.shape[0] == 5 for v in out.values())
    assert np.array_equal(out["shape"][0], a["shape"]) and np.array_equal(out["shape"][-1], b["shape"])
    assert np.array_equal(out["jaw"][0], a["jaw"]) and (out["jaw"][-1] == 0).all()
    assert (out["expression"][0] == 0).all() and np.array_equal(out["expression"][-1], b["expression"])
    assert np.allclose(out["shape"][2], 0.5 * (a["shape"] + b["shape"]))
    assert np.array_equal(MM.interpolate_params(a, b, 1)["shape"][0], b["shape"])
    with pytest.raises(ValueError):
        MM.interpolate_params(a, {"shape": np.zeros(3)}, 4)
    with pytest.raises(ValueError):
        MM.interpolate_params(a, b, 0)


# ---- model files
def flame_like(seed=3, V=40, n_id=300, n_exp=6):
    """Model arrays with the pickle's key names and FLAME's column layout (expression from column 300 on)."""
    m = R.synthetic_model(seed, V, n_id + n_exp, 5, parents=[-1, 0, 1, 1, 1], M=4)
    kt = np.array([[2 ** 32 - 1, 0, 1, 1, 1], [0, 1, 2, 3, 4]], dtype=np.uint32)  # as the FLAME pickle stores it
    return {"v_template": m["v_template"], "shapedirs": m["shapedirs"], "posedirs": m["posedirs"], "J_regressor": m["J_regressor"],
            "kintree_table": kt, "weights": m["weights"], "f": m["faces"], "static_lmk_faces_idx": m["lmk_face"],
            "static_lmk_bary_coords": m["lmk_bary"]}


def same_model(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("v_template", "basis", "weights", "j_template", "j_dirs", "faces",
                                                                   "lmk_face", "lmk_bary")) and a.parents == b.parents


def test_npz_round_trip_and_the_folds(tmp_path):
    d = flame_like()
    np.savez(tmp_path / "flame.npz", **d)
    fm = MM.MorphableModel.load(tmp_path / "flame.npz", device="cpu")
    assert (fm.V, fm.NB, fm.J, fm.parents, fm.n_shape) == (40, 306, 5, [-1, 0, 1, 1, 1], 306)
    jt, jd, basis = R.fold(d["v_template"], d["shapedirs"], d["posedirs"], d["J_regressor"])
    assert torch.equal(fm.basis, torch.from_numpy(basis.astype(np.float32))) and tuple(fm.basis.shape) == (306 + 36, 120)
    assert torch.equal(fm.j_template, torch.from_numpy(jt.astype(np.float32)))
    assert torch.equal(fm.j_dirs, torch.from_numpy(jd.astype(np.float32)))
    assert fm.faces.dtype == torch.int32 and fm.lmk_face.dtype == torch.int32 and tuple(fm.lmk_bary.shape) == (4, 3)
    direct = MM.MorphableModel.from_arrays(d["v_template"], d["shapedirs"], d["posedirs"], d["J_regressor"], [-1, 0, 1, 1, 1],
                                           d["weights"], faces=d["f"], lmk_face=d["static_lmk_faces_idx"],
                                           lmk_bary=d["static_lmk_bary_coords"], device="cpu")
    assert same_model(fm, direct)
    mm = MM.MorphableModel.load(tmp_path / "flame.npz", device="cpu", unit_scale=1000.0)
    assert torch.allclose(mm.v_template, fm.v_template * 1000) and torch.allclose(mm.basis, fm.basis * 1000)
    assert torch.allclose(mm.j_dirs, fm.j_dirs * 1000) and torch.equal(mm.weights, fm.weights)
    with pytest.raises(ValueError, match="GPU"):
        fm.forward(torch.zeros(1, 306), torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match="missing"):
        np.savez(tmp_path / "bad.npz", v_template=d["v_template"])
        MM.MorphableModel.load(tmp_path / "bad.npz", device="cpu")
    with pytest.raises(ValueError, match="expected"):
        MM.MorphableModel.load(tmp_path / "flame.json", device="cpu")


def test_n_shape_n_exp_select_columns_as_the_reference_does(tmp_path):
    d = flame_like()
    np.savez(tmp_path / "flame.npz", **d)
    fm = MM.MorphableModel.load(tmp_path / "flame.npz", n_shape=10, n_exp=4, device="cpu")
    S = d["shapedirs"]
    want = np.concatenate([S[:, :, :10], S[:, :, 300:304]], 2).reshape(120, 14).T
    assert (fm.NB, fm.n_shape) == (14, 10) and torch.equal(fm.basis[:14], torch.from_numpy(want))
    fm = MM.MorphableModel.load(tmp_path / "flame.npz", n_shape=10, device="cpu")  # FLAME.__init__: everything from column 300 on
    assert fm.NB == 16 and torch.equal(fm.basis[10:16], torch.from_numpy(S[:, :, 300:].reshape(120, 6).T))
    with pytest.raises(ValueError):
        MM.MorphableModel.load(tmp_path / "flame.npz", n_shape=10, n_exp=7, device="cpu")


def test_pkl_with_plain_arrays_and_with_a_fake_chumpy(tmp_path):
    d = flame_like()
    np.savez(tmp_path / "flame.npz", **d)
    want = MM.MorphableModel.load(tmp_path / "flame.npz", device="cpu")
    with open(tmp_path / "plain.pkl", "wb") as f:
        pickle.dump(dict(d, bs_type="lrotmin", bs_style="lbs"), f, protocol=2)
    assert same_model(MM.MorphableModel.load(tmp_path / "plain.pkl", device="cpu"), want)

    assert "chumpy" not in sys.modules
    pkg, mod = types.ModuleType("chumpy"), types.ModuleType("chumpy.ch")

    class Ch:
        def __init__(self, x):
            self.x, self.dterms = np.asarray(x), ("x",)

    Ch.__module__, Ch.__qualname__ = "chumpy.ch", "Ch"
    mod.Ch = pkg.ch = Ch
    sys.modules["chumpy"], sys.modules["chumpy.ch"] = pkg, mod
    try:
        wrapped = dict(d, v_template=Ch(d["v_template"]), shapedirs=Ch(d["shapedirs"]), posedirs=Ch(d["posedirs"]))
        for proto in (0, 2, 4):  # copyreg._reconstructor and the NEWOBJ opcode
            with open(tmp_path / f"chumpy{proto}.pkl", "wb") as f:
                pickle.dump(wrapped, f, protocol=proto)
    finally:
        del sys.modules["chumpy"], sys.modules["chumpy.ch"]
    for proto in (0, 2, 4):
        assert same_model(MM.MorphableModel.load(tmp_path / f"chumpy{proto}.pkl", device="cpu"), want)
    assert "chumpy" not in sys.modules

    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
    if sp is not None:
        with open(tmp_path / "sparse.pkl", "wb") as f:
            pickle.dump(dict(d, J_regressor=sp.csc_matrix(d["J_regressor"])), f, protocol=2)
        assert same_model(MM.MorphableModel.load(tmp_path / "sparse.pkl", device="cpu"), want)


def test_pickle_naming_any_other_global_raises(tmp_path):
    d = flame_like()
    for i, evil in enumerate((os.getcwd, types.SimpleNamespace(a=1), pickle.Unpickler, np.load, torch.zeros(1))):
        with open(tmp_path / f"evil{i}.pkl", "wb") as f:
            pickle.dump(dict(d, extra=evil), f)
        with pytest.raises(pickle.UnpicklingError, match="not allowed"):
            MM.MorphableModel.load(tmp_path / f"evil{i}.pkl", device="cpu")

    class Boom:
        def __reduce__(self):
            return (os.system, ("true",))

    with open(tmp_path / "boom.pkl", "wb") as f:
        pickle.dump(dict(d, extra=Boom()), f)
    with pytest.raises(pickle.UnpicklingError, match="not allowed"):
        MM.read_model_file(tmp_path / "boom.pkl")


def test_python_argument_checks_precede_any_launch():
    m = R.synthetic_model(2, 9, 4, 3, parents=[-1, 0, 1], M=2)
    t = lambda a: torch.from_numpy(np.asarray(a))
    jt, jd, basis = (t(a.astype(np.float32)) for a in R.fold(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"]))
    betas, pose = torch.zeros(2, 4), torch.zeros(2, 3, 3)
    bad_pose = [(betas[:, :3], pose, jt, jd, [-1, 0, 1]), (betas, pose[:, :2], jt, jd, [-1, 0, 1]), (betas.long(), pose, jt, jd, [-1, 0, 1]),
                (betas, pose, jt[:2], jd, [-1, 0, 1]), (betas, pose, jt, jd[:, :6], [-1, 0, 1]), (betas, pose, jt, jd, [-1, 0]),
                (betas, pose, jt, jd, [0, 0, 1]), (betas, pose, jt, jd, [-1, 1, 0]), (betas, pose, jt, jd, [-1, 0, 2]),
                (betas, pose, jt, jd, [-1, -1, 0]),
                (torch.zeros(1, 4), torch.zeros(1, 65, 3), torch.zeros(65, 3), torch.zeros(4, 195), [-1] + list(range(64)))]
    for args in bad_pose:
        with pytest.raises(ValueError):
            E.op_morph_pose(*args)
    vt, W = t(m["v_template"]), t(m["weights"])
    coef, A = torch.zeros(2, 4 + 18), torch.zeros(2, 3, 3, 4)
    bad_skin = [(basis[:, :26], vt, coef, W, A), (basis, vt[:, :2], coef, W, A), (basis, vt, coef[:, :21], W, A), (basis, vt, coef, W[:8], A),
                (basis, vt, coef, W, A[:1]), (basis, vt, coef, W, A[:, :2]), (basis.double().long(), vt, coef, W, A),
                (basis, vt, coef, W, A, torch.zeros(4, 4)), (basis, vt, coef, torch.zeros(9, 65), torch.zeros(2, 65, 12))]
    for args in bad_skin:
        with pytest.raises(ValueError):
            E.op_morph_skin(*args)
    with pytest.raises(ValueError):
        E.op_morph_skin(basis, vt, coef, W, A, n_betas=5)  # L != NB + 9 (J - 1)
    verts, faces, lf, lb = torch.zeros(2, 9, 3), t(m["faces"]), t(m["lmk_face"]), t(m["lmk_bary"])
    for args in [(verts[..., :2], faces, lf, lb), (verts, faces.long(), lf, lb), (verts, faces, lf.long(), lb), (verts, faces, lf, lb[:1]),
                 (verts, faces[:, :2], lf, lb), (verts, faces, lf, lb.long())]:
        with pytest.raises(ValueError):
            E.op_morph_landmarks(*args)
    arrays = (m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"])
    for i, bad in ((0, m["v_template"][:, :2]), (1, m["shapedirs"][:8]), (2, m["posedirs"][:, :, :17]), (3, m["J_regressor"][:, :8]),
                   (4, [-1, 1, 0]), (5, m["weights"][:, :2])):
        with pytest.raises(ValueError):
            MM.MorphableModel.from_arrays(*(arrays[:i] + (bad,) + arrays[i + 1:]), device="cpu")
    with pytest.raises(ValueError):
        MM.MorphableModel.from_arrays(*arrays, lmk_face=m["lmk_face"], lmk_bary=m["lmk_bary"], device="cpu")  # landmarks need faces
    fm = MM.MorphableModel.from_arrays(*arrays, device="cpu")
    with pytest.raises(ValueError, match="joints"):
        fm.flame(np.zeros(4))  # three joints: not a FLAME model
    with pytest.raises(ValueError):
        MM.frames_to_batch(torch.zeros(8, 8, 3), torch.zeros(9, 3))


# ---- the C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    lib = L.load()
    for name, nargs in (("mvd_op_morph_pose", 14), ("mvd_op_morph_skin", 13), ("mvd_op_morph_landmarks", 10)):
        assert name in L.PROTOTYPES and len(L.PROTOTYPES[name][1]) == nargs
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs


def abi_error_cases(p, parents):
    """{entry point: {case: arguments with one argument error}}; p: any non-null address (never read); parents: addresses of
    host int32 arrays, "ok" = [-1, 0] and three bad ones."""
    pose = dict(betas=p, pose=p, j_template=p, j_dirs=p, parents=parents["ok"], F=1, NB=1, J=2, j_rest=p, rot=p, pose_feature=p, joints=p,
                A=p, stream=None)
    skin = dict(basis=p, v_template=p, coef=p, weights=p, A=p, post=None, F=1, V=1, L=10, NB=1, J=2, verts=p, stream=None)
    lmk = dict(verts=p, faces=p, lmk_face=p, lmk_bary=p, F=1, V=1, Nf=1, M=1, out=p, stream=None)
    joints = {"J < 1": dict(J=0), "J > 64": dict(J=65)}
    bad = {"mvd_op_morph_pose": (pose, dict({f"null {k}": {k: None} for k in ("betas", "pose", "j_template", "j_dirs", "parents", "j_rest",
                                                                             "rot", "pose_feature", "joints", "A")},
                                            **joints, **{"F < 1": dict(F=0), "NB < 1": dict(NB=0), "F J 12 >= 2^31": dict(F=2 ** 27),
                                                         "parents[0] != -1": dict(parents=parents["root"]),
                                                         "parents[1] >= 1": dict(parents=parents["forward"]),
                                                         "parents[1] < 0": dict(parents=parents["negative"])})),
           "mvd_op_morph_skin": (skin, dict({f"null {k}": {k: None} for k in ("basis", "v_template", "coef", "weights", "A", "verts")},
                                            **joints, **{"F < 1": dict(F=0), "V < 1": dict(V=0), "L < 1": dict(L=0), "NB < 1": dict(NB=0),
                                                         "L != NB + 9 (J-1)": dict(L=11), "F V 3 >= 2^31": dict(F=2 ** 15, V=2 ** 15)})),
           "mvd_op_morph_landmarks": (lmk, dict({f"null {k}": {k: None} for k in ("verts", "faces", "lmk_face", "lmk_bary", "out")},
                                                **{"F < 1": dict(F=0), "V < 1": dict(V=0), "Nf < 1": dict(Nf=0), "M < 1": dict(M=0),
                                                   "F V 3 >= 2^31": dict(F=2 ** 15, V=2 ** 15), "F M 3 >= 2^31": dict(F=2 ** 15, M=2 ** 15)}))}
    return {fn: {k: tuple(dict(ok, **v).values()) for k, v in cases.items()} for fn, (ok, cases) in bad.items()}


def test_c_abi_argument_errors_need_no_device():
    """Every argument error returns before the first HIP call, so this holds on a machine without a GPU."""
    lib = L.load()
    buf = (C.c_double * 8)()
    arrays = {"ok": (C.c_int32 * 2)(-1, 0), "root": (C.c_int32 * 2)(0, 0), "forward": (C.c_int32 * 2)(-1, 1),
              "negative": (C.c_int32 * 2)(-1, -1)}
    n = 0
    for fn, cases in abi_error_cases(C.addressof(buf), {k: C.addressof(v) for k, v in arrays.items()}).items():
        for name, args in cases.items():
            assert getattr(lib, fn)(*args) != 0, (fn, name)
            assert lib.mvd_last_error().decode().startswith(fn + ": "), (fn, name)
            n += 1
    assert n == 18 + 14 + 11


# ---- generate_face
def test_generate_face_argument_rules(tmp_path, capsys):
    from morphablediffusion_amd import generate_face as GF
    base = ["--input_img", "a.png", "--exp_img", "b.png", "--output_dir", str(tmp_path)]
    flags = GF.parse_args(base + ["--mesh", "m.ply"])
    assert flags.mesh == "m.ply" and flags.flame_model is None and flags.flame_params is None and flags.neutral_params is None
    assert (flags.frames, flags.frame_batch) == (1, 1)
    assert vars(flags) == vars(GF.build_parser().parse_args(base + ["--mesh", "m.ply"]))  # --mesh alone: nothing else changes
    flame = ["--flame_model", "f.npz", "--flame_params", "p.npz"]
    flags = GF.parse_args(base + flame + ["--neutral_params", "n.npz", "--frames", "4", "--frame_batch", "2", "--export_mesh"])
    assert flags.mesh is None and (flags.frames, flags.frame_batch, flags.export_mesh) == (4, 2, True)
    assert GF.parse_args(base + flame).frames == 1
    for bad in (base, base + ["--flame_model", "f.npz"], base + ["--flame_params", "p.npz"], base + flame + ["--mesh", "m.ply"],
                base + flame + ["--frames", "4"], base + flame + ["--neutral_params", "n.npz"], base + flame + ["--frame_batch", "0"],
                base + ["--mesh", "m.ply", "--frames", "4"], base + ["--mesh", "m.ply", "--neutral_params", "n.npz"]):
        with pytest.raises(SystemExit):
            GF.parse_args(bad)
    capsys.readouterr()
    np.savez(tmp_path / "p.npz", shape=np.zeros(3), jaw=np.zeros(3))
    assert set(GF.load_flame_params(tmp_path / "p.npz")) == {"shape", "jaw"}
    np.savez(tmp_path / "q.npz", shape=np.zeros(3), jaw_pose=np.zeros(3))
    with pytest.raises(ValueError, match="jaw_pose"):
        GF.load_flame_params(tmp_path / "q.npz")

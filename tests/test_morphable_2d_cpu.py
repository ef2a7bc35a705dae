"""CPU: the oracle of the 2-D multi-view landmark term (tests/morphable_2d_ref.py) checked against itself -- its gradient against
central differences, the row selection at its boundaries, the contour adjoint as the transpose of the forward gather -- and the
conditions the GPU tests rely on: the float64 loop converges on the inputs tests/test_gpu_morphable_fit_2d.py uses, the float32 and
float64 oracles select the same rows there, and the fit with per-view contour rows beats the fit with row 0 everywhere.  Also the
host-side pieces that need no GPU: the contour table, reprojection_error, the model file keys, the command line's flag rules."""
import functools

import numpy as np
import pytest

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import morphable as MM
from tests import morphable_2d_ref as R2
from tests import morphable_bwd_ref as BR
from tests import morphable_ref as R

ITERS, PX = 300, 1.0 / 512  # the fit tests' iteration count and pixel scale (a 512 x 512 image)


def small_case(F=2, C=3, M=7, Md=4, seed=0):
    g = np.random.default_rng(seed)
    K, RT = R2.cameras(np.linspace(-40, 35, C))
    lmk, dyn = g.normal(size=(F, M, 3)) * 0.1, g.normal(size=(F, C, Md, 3)) * 0.1
    uv = R2.project(lmk, K, RT, 1e-3)["uv"]
    duv = R2.project(dyn, K, RT, 1e-3, per_view=True)["uv"]
    tgt, dtgt = uv[:1] + g.normal(size=(1, C, M, 2)) * 5, duv + g.normal(size=duv.shape) * 5
    w, dw = g.random((1, C, M)) * (g.random((1, C, M)) > 0.2), g.random((F, C, Md))
    return dict(lmk=lmk, K=K, RT=RT, target_uv=tgt, weight=w, dyn_lmk=dyn, dyn_target_uv=dtgt, dyn_weight=dw, px_scale=PX, lambda2=1.7)


def test_the_gradient_is_the_derivative_of_the_energy():
    c = small_case(C=2, M=4, Md=2)
    t = R2.term(**c)
    assert (t["n_valid"] > 0).all() and t["g_dyn"].shape == c["dyn_lmk"].shape
    worst = 0.0
    for name, key in (("lmk", "g_lmk"), ("dyn_lmk", "g_dyn")):
        x, g = c[name], t[key]
        num = np.zeros_like(x)
        for idx in np.ndindex(x.shape):
            f = idx[0]
            h = 1e-6
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            num[idx] = (R2.term(**{**c, name: xp})["E2"][f] - R2.term(**{**c, name: xm})["E2"][f]) / (2 * h)
        err = np.abs(num - g).max() / np.abs(g).max()
        worst = max(worst, err)
        print(f"2-D term, d E2 / d {name}: worst difference to central differences, relative to the largest entry: {err:.3e}")
    assert worst < 1e-8


def test_uncounted_observations_never_leak():
    c = small_case()
    base = R2.term(**c)
    tgt = c["target_uv"].copy()
    tgt[(c["weight"] == 0)] = np.nan
    lmk = c["lmk"].copy()
    lmk[0, 2] = (0.0, 0.0, 5.0)  # behind every camera of the ring (they sit at distance 1)
    a, b = R2.term(**{**c, "target_uv": tgt}), R2.term(**{**c, "lmk": lmk})
    assert np.array_equal(a["E2"], base["E2"]) and np.array_equal(a["g_lmk"], base["g_lmk"])
    assert (b["g_lmk"][0, 2] == 0).all() and b["n_valid"][0] < base["n_valid"][0] and np.isfinite(b["E2"]).all()
    z = R2.term(**{**c, "weight": np.zeros_like(c["weight"]), "dyn_weight": np.zeros_like(c["dyn_weight"])})
    assert (z["E2"] == 0).all() and (z["g_lmk"] == 0).all() and (z["g_dyn"] == 0).all() and (z["n_valid"] == 0).all()


def test_the_row_rule_at_its_boundaries():
    yaw = [0.0, 0.49, -0.49, 0.51, -0.51, 39.0, -39.0, 39.6, -39.6, 80.0, -80.0, 0.5, 1.5, -0.5, -38.6]
    want = [0, 0, 0, 1, 40, 39, 78, 39, 78, 39, 78, 0, 2, 0, 78]  # -0.51 -> -1 -> 39 + 1; -39 -> 39 + 39; below -39 -> 78; ties to even
    assert R2.contour_row(yaw, 79).tolist() == want
    assert R2.contour_row([0.0, 0.6, 1.7, 9.0, -0.6, -1.4, -1.6, -2.4, -2.6, -50.0], 5).tolist() == [0, 1, 2, 2, 3, 3, 4, 4, 4, 4]
    assert R2.contour_row([3.0, -3.0], 1).tolist() == [0, 0]


def test_a_frontal_camera_on_an_unposed_head_selects_row_0_and_the_ring_its_own_angles():
    m = R2.head_model()
    fm = BR.Folded(m)
    fw = BR.forward(fm, np.zeros((1, fm.NB)), np.zeros((1, fm.J, 3)))
    yaws = np.array([0.0, 10.3, -10.3, 38.7, -38.7, 45.0, -45.0])
    K, RT = R2.cameras(yaws)
    rows, yaw = R2.contour_select(fw["A"], RT, 1, 79)
    print("yaw of an unposed head in a ring of cameras:", yaw[0])
    assert np.allclose(np.abs(yaw[0]), np.abs(yaws), atol=1e-4) and rows[0, 0] == 0
    assert rows[0].tolist() == [0, 10, 49, 39, 78, 39, 78]  # 38.7 rounds to 39, 45 is clamped to it; -38.7 -> 39 + 39, -45 -> 78
    # turning the head by a global rotation about y moves every view's yaw by as much
    pose = np.zeros((1, fm.J, 3))
    pose[0, 0, 1] = np.deg2rad(7.0)
    yaw7 = R2.contour_yaw(BR.forward(fm, np.zeros((1, fm.NB)), pose)["A"], RT, 1)
    assert np.allclose(np.abs(yaw7 - yaw), 7.0, atol=1e-3)


def test_the_contour_adjoint_is_the_transpose_of_the_gather():
    m = R.synthetic_model(3, 40, 4, 2, M=3)
    for Rr, Md in ((5, 4), (79, 17)):
        df, db = R2.synthetic_contour(1, m, Rr, Md)
        df[Rr // 2, Md - 1] = len(m["faces"]) + 3  # one face outside the mesh
        g = np.random.default_rng(2)
        rows = np.array([[0, Rr // 2, Rr // 2, Rr - 1], [1 % Rr, 1 % Rr, 0, Rr // 2]], dtype=np.int32)
        verts, g_dyn = g.normal(size=(2, 40, 3)), g.normal(size=(2, 4, Md, 3))
        dyn = R2.contour_landmarks(verts, m["faces"], df, db, rows)
        back = R2.contour_bwd(np.where(np.isnan(dyn), 0, g_dyn), rows, m["faces"], df, db, 40)
        for f in range(2):
            Mt = R2.contour_matrix(m["faces"], df, db, rows[f], 40)
            want = (Mt @ verts[f]).reshape(4, Md, 3)
            ok = ~np.isnan(dyn[f])
            assert np.isnan(dyn[f, list(rows[f]).index(Rr // 2), Md - 1]).all() and np.allclose(dyn[f][ok], want[ok], atol=1e-13)
            assert np.allclose(back[f], Mt.T @ np.where(np.isnan(dyn[f]), 0, g_dyn[f]).reshape(-1, 3), atol=1e-13)
        # the table the kernel gathers through: per listed vertex the ascending entries (row Md + landmark) 3 + corner
        cv, cp, ce = E.contour_table(m["faces"], df, 40)
        brute = {}
        for r in range(Rr):
            for d in range(Md):
                if 0 <= df[r, d] < len(m["faces"]):
                    for k in range(3):
                        brute.setdefault(int(m["faces"][df[r, d], k]), []).append((r * Md + d) * 3 + k)
        assert cv.tolist() == sorted(brute) and all(ce[cp[i]:cp[i + 1]].tolist() == sorted(brute[v]) for i, v in enumerate(cv.tolist()))


@functools.lru_cache(maxsize=None)
def loops(contours):
    c = R2.fit_case(contours=contours, LR=0.05)
    kw = dict(dyn_target_uv=c["dyn_target_uv"], lr=c["lr"], px_scale=PX, iters=ITERS)
    o64 = R2.fit_oracle_2d(c["model"], c["K"], c["RT"], c["target_uv"], keep=(20, 100), **kw)
    o32 = R2.fit_oracle_2d(c["model"], c["K"], c["RT"], c["target_uv"], keep=(20, 100), dtype=np.float32, iters=100,
                           **{k: v for k, v in kw.items() if k != "iters"})
    return c, o64, o32


@pytest.mark.parametrize("contours", [False, True])
def test_the_float64_loop_converges_on_the_gpu_tests_inputs(contours):
    c, o64, o32 = loops(contours)
    args = (c["K"], c["RT"], c["target_uv"])
    first = R2.reprojection_px(c["model"], np.zeros_like(c["truth"]), *args, dyn_target_uv=c["dyn_target_uv"])
    last = R2.reprojection_px(c["model"], o64["p"], *args, dyn_target_uv=c["dyn_target_uv"])
    print(f"float64 2-D loop, contours={contours}: reprojection {first.mean(1)} -> {last.mean(1)} px, factor {(last / first).max():.3e}")
    for k in (20, 100):
        print(f"  float32 loop after {k} iterations: worst parameter difference {np.abs(o32['snapshots'][k] - o64['snapshots'][k]).max():.3e}")
    assert (first > 20).all() and (last <= 1e-5 * first).all()  # the GPU test asks for 1e-3: two decades of margin
    assert (o64["n_valid_history"] == 3 * (51 + (17 if contours else 0))).all()
    if contours:
        # the rows settle on those of the truth, in both precisions, and the head's turn gives every view its own
        assert np.array_equal(o64["rows_history"][-1], c["rows"]) and np.array_equal(o32["rows_history"], o64["rows_history"][:100])
        assert all(len(set(r.tolist())) == 3 for r in c["rows"])


def test_per_view_rows_beat_row_0_everywhere_on_the_contour():
    c, o64, _ = loops(True)
    args = (c["K"], c["RT"], c["target_uv"])
    o0 = R2.fit_oracle_2d(c["model"], c["K"], c["RT"], c["target_uv"], dyn_target_uv=c["dyn_target_uv"], lr=c["lr"], px_scale=PX, iters=ITERS,
                          fixed_rows=np.zeros_like(c["rows"]))
    a = R2.reprojection_px(c["model"], o64["p"], *args, dyn_target_uv=c["dyn_target_uv"], which="contour")
    b = R2.reprojection_px(c["model"], o0["p"], *args, dyn_target_uv=c["dyn_target_uv"], which="contour")
    print(f"contour reprojection: per-view rows {a.max():.3e} px, row 0 everywhere {b.min():.3e} px")
    assert (a < 0.01 * b).all()


def test_op_test_yaws_are_away_from_the_rounding_boundaries():
    m = R2.head_model()
    betas, pose = R.seeded_params(7, 3, 12, 5)
    K, RT = R2.cameras(R2.OP_YAWS)
    y64 = R2.contour_yaw(BR.forward(BR.Folded(m), betas, pose)["A"], RT, 1)
    y32 = R2.contour_yaw(BR.forward(BR.Folded(m, np.float32), betas, pose)["A"], RT, 1, np.float32)
    frac = np.abs(y64 - np.floor(y64) - 0.5)
    print(f"op-test yaws: nearest distance to a rounding boundary {frac.min():.3f} deg, float32 oracle off by {np.abs(y32 - y64).max():.2e}")
    assert frac.min() >= 0.05
    for Rr in (5, 79):
        assert np.array_equal(R2.contour_row(y32, Rr), R2.contour_row(y64, Rr))


def check_entry_errors():
    """Every argument error of the 2-D entries, on host buffers: each returns non-zero with its message, before any HIP call (so
    this runs without a GPU too; tests/test_gpu_morphable_2d_ops.py runs it again next to a device)."""
    import ctypes as C
    from morphablediffusion_amd import lib as L
    lib = L.load()
    buf, ints = (C.c_float * 8192)(), (C.c_int32 * 64)()
    par = (C.c_int32 * 2)(-1, 0)
    p, i, pp = C.addressof(buf), C.addressof(ints), C.addressof(par)
    inf, nan = float("inf"), float("nan")

    def fails(rc, text):
        assert rc != 0 and text in lib.mvd_last_error().decode(), lib.mvd_last_error().decode()

    assert [lib.mvd_morph_2d_blocks(*a) for a in ((1, 0), (51, 17), (256, 0), (240, 17), (0, 0), (-1, 5))] == [1, 1, 1, 2, 0, 0]
    proj = lambda **k: lib.mvd_op_morph_project(*[{**dict(pt=p, K=p, RT=p, fc=1, F=1, C=1, M=1, z=0.1, uv=p, valid=i, s=None), **k}[n]
                                                   for n in ("pt", "K", "RT", "fc", "F", "C", "M", "z", "uv", "valid", "s")])
    fails(proj(pt=None), "null argument")
    fails(proj(K=None), "null argument")
    fails(proj(fc=2, F=3), "1 or F frames")
    fails(proj(C=0), "F and C must be at least 1")
    fails(proj(z=0.0), "z_near must be positive")
    fails(proj(z=inf), "z_near must be positive")
    fails(proj(F=2 ** 15, fc=2 ** 15, C=2 ** 8, M=2 ** 8), "below 2^31")
    fails(lib.mvd_op_morph_project_bwd(p, p, p, 1, None, 1, 1, 1, 0.1, p, None), "null argument")
    fails(lib.mvd_op_morph_project_bwd(p, p, p, 1, p, 1, 1, 0, 0.1, p, None), "M must be at least 1")
    names = ("lmk", "dyn", "K", "RT", "fc", "tu", "w", "dtu", "dw", "ft", "F", "C", "M", "Md", "z", "px", "lam", "ea", "uv", "duv", "part",
             "E2", "nv", "gl", "gd", "s")
    base = dict(lmk=p, dyn=None, K=p, RT=p, fc=1, tu=p, w=None, dtu=None, dw=None, ft=1, F=1, C=1, M=1, Md=0, z=0.1, px=1.0, lam=1.0, ea=None,
                uv=p, duv=None, part=p, E2=p, nv=i, gl=p, gd=None, s=None)
    term = lambda **k: lib.mvd_op_morph_fit_data_2d(*[{**base, **k}[n] for n in names])
    for k in ("lmk", "K", "RT", "tu", "uv", "part", "E2", "nv", "gl"):
        fails(term(**{k: None}), "null argument")
    fails(term(fc=2, F=3), "cameras must have 1 or F frames")
    fails(term(ft=2, F=3), "2-D target must have 1 or F frames")
    fails(term(C=0), "F and C must be at least 1")
    fails(term(M=0), "M must be at least 1")
    fails(term(F=65536, fc=1, ft=1), "at most 65535 frames")
    fails(term(F=2 ** 13, C=2 ** 9, M=2 ** 9), "F C M 2 must be below 2^31")
    for z in (0.0, -1.0, inf, nan):
        fails(term(z=z), "z_near must be positive and finite")
    for bad in (dict(px=-1.0), dict(px=inf), dict(px=nan), dict(lam=-0.5), dict(lam=inf), dict(lam=nan)):
        fails(term(**bad), "px_scale and lambda2 must be finite and not negative")
    fails(term(dyn=p, Md=1), "go together")
    fails(term(dtu=p, Md=1), "go together")
    fails(term(dw=p, Md=1), "go together")
    fails(term(dyn=p, dtu=p, duv=p, gd=p, Md=0), "Md must be at least 1")
    sel = lambda **k: lib.mvd_op_morph_contour_select(*[{**dict(A=p, RT=p, fc=1, F=1, C=1, J=2, neck=1, R=5, row=i, yaw=None, s=None), **k}[n]
                                                        for n in ("A", "RT", "fc", "F", "C", "J", "neck", "R", "row", "yaw", "s")])
    fails(sel(A=None), "null argument")
    fails(sel(row=None), "null argument")
    fails(sel(neck=2), "neck_joint must be in 0..J-1")
    fails(sel(neck=-1), "neck_joint must be in 0..J-1")
    fails(sel(R=4), "odd number of rows")
    fails(sel(R=0), "odd number of rows")
    fails(sel(J=65), "J must be in 1..64")
    fails(sel(fc=2, F=3), "1 or F frames")
    fails(lib.mvd_op_morph_contour_landmarks(p, i, i, p, None, 1, 1, 1, 1, 5, 1, p, None), "null argument")
    fails(lib.mvd_op_morph_contour_landmarks(p, i, i, p, i, 1, 1, 1, 1, 5, 0, p, None), "at least 1")
    fails(lib.mvd_op_morph_contour_bwd(p, None, i, i, i, None, p, 1, 1, 1, 5, 1, 1, 1, p, None), "null argument")
    fails(lib.mvd_op_morph_contour_bwd(p, None, i, i, i, i, p, 1, 1, 1, 5, 1, 0, 1, p, None), "at least 1")
    n = C.c_int64(0)
    assert lib.mvd_morph_fit_2d_workspace(1, 1, 1, 1, 1, 0, 1, C.addressof(n)) == 0 and n.value > 0
    small = n.value
    assert lib.mvd_morph_fit_2d_workspace(2, 9, 3, 2, 4, 3, 2, C.addressof(n)) == 0 and n.value > small
    fails(lib.mvd_morph_fit_2d_workspace(1, 1, 1, 1, 0, 0, 1, C.addressof(n)), "at least 1")
    fails(lib.mvd_morph_fit_2d_workspace(1, 1, 1, 1, 1, 0, 1, None), "null argument")
    rn = ("basis", "vt", "wts", "jt", "jd", "par", "post", "faces", "lf", "lb", "cp", "ce", "df", "db", "cv", "ctp", "cte", "F", "V", "NB", "J",
          "Nf", "M", "n_ent", "R", "Md", "n_list", "ct_n", "neck", "K", "RT", "fc", "C", "tu", "w", "dtu", "dw", "ft", "z", "px", "lam", "tg",
          "tf3", "vw", "ivw", "p", "m", "v", "lr", "lamv", "p0", "iters", "step0", "b1", "b2", "eps", "ws", "nws", "hist", "nhist", "s")
    rbase = dict(basis=p, vt=p, wts=p, jt=p, jd=p, par=pp, post=None, faces=i, lf=i, lb=p, cp=i, ce=i, df=i, db=p, cv=i, ctp=i, cte=i, F=1, V=3,
                 NB=1, J=2, Nf=1, M=1, n_ent=3, R=5, Md=1, n_list=3, ct_n=3, neck=1, K=p, RT=p, fc=1, C=1, tu=p, w=None, dtu=None, dw=None,
                 ft=1, z=0.1, px=1.0, lam=1.0, tg=None, tf3=1, vw=None, ivw=0.0, p=p, m=p, v=p, lr=p, lamv=p, p0=p, iters=1, step0=0, b1=0.9,
                 b2=0.999, eps=1e-8, ws=p, nws=8192, hist=p, nhist=i, s=None)
    run = lambda **k: lib.mvd_morph_fit_2d_run(*[{**rbase, **k}[n] for n in rn])
    fails(run(ws=None), "null argument")
    fails(run(nhist=None), "null argument")
    fails(run(iters=0), "iters must be at least 1")
    fails(run(lf=None), "needs the landmark embedding")
    fails(run(dtu=p, df=None), "a contour target is given, and the model has no contour tables")
    fails(run(dtu=p, cv=None), "a contour target is given, and the model has no contour tables")
    fails(run(dw=p), "contour weights without a contour target")
    fails(run(dtu=p, neck=2), "neck_joint must be in 0..J-1")
    fails(run(dtu=p, R=4), "odd number of rows")
    fails(run(fc=2, F=3), "cameras must have 1 or F frames")
    fails(run(ft=3, F=2), "2-D target must have 1 or F frames")
    fails(run(C=0), "at least 1")
    fails(run(z=0.0), "z_near must be positive and finite")
    fails(run(px=nan), "px_scale and lambda2")
    fails(run(lam=-1.0), "px_scale and lambda2")
    fails(run(nws=16), "workspace is smaller")
    fails(run(tg=p, tf3=2), "vertex target must have 1 or F frames")
    fails(run(b1=1.0), "beta1 and beta2")
    fails(run(J=65), "J in 1..64")


def test_entry_points_refuse_bad_arguments_before_the_first_hip_call():
    check_entry_errors()


def test_fit_landmarks2d_follows_fit_meshs_flag_rules():
    from morphablediffusion_amd import generate_face as GF
    base = ["--input_img", "a.png", "--exp_img", "b.jpg", "--output_dir", "o", "--flame_model", "m.npz"]
    flags = GF.parse_args(base + ["--fit_landmarks2d", "l.npz", "--fit_iters", "7", "--fit_lr", "0.01"])
    assert flags.fit_landmarks2d == "l.npz" and flags.fit_iters == 7 and flags.fit_lr == 0.01
    assert GF.parse_args(base + ["--flame_params", "p.npz"]).fit_landmarks2d is None
    assert GF.parse_args(base + ["--fit_landmarks2d", "l.npz", "--flame_params", "p.npz", "--frames", "3"]).frames == 3
    for extra in (["--fit_mesh", "m.ply"], ["--fit_scan", "s.ply"], ["--mesh", "m.ply"], ["--neutral_params", "n.npz"], ["--fit_iters", "0"],
                  ["--fit_lr", "0"], ["--frames", "3"]):
        with pytest.raises(SystemExit):
            GF.parse_args(base + ["--fit_landmarks2d", "l.npz"] + extra)
    with pytest.raises(SystemExit):
        GF.parse_args(base[:6] + ["--fit_landmarks2d", "l.npz"])


def test_reprojection_error_read_out():
    uv = np.zeros((2, 3, 4, 2))
    tgt = uv.copy()
    tgt[..., 0] = [1.0, 3.0, 5.0, 100.0]
    w = np.ones((2, 3, 4))
    w[..., 3] = 0
    tgt[..., 3, :] = np.nan
    r = MM.reprojection_error(uv, tgt, w, thresholds=(2, 4))
    assert np.allclose(r["mean_px"], 3.0) and (r["count"] == 3).all()
    assert np.allclose(r["pck"][2.0], 1 / 3) and np.allclose(r["pck"][4.0], 2 / 3)
    none = MM.reprojection_error(uv, tgt, np.zeros_like(w))
    assert np.isnan(none["mean_px"]).all()
    with pytest.raises(ValueError, match="weights must be"):
        MM.reprojection_error(uv, tgt, w[0])


def test_model_files_carry_the_contour_table(tmp_path):
    m = R2.head_model(V=40, NB=3, M=3, Rr=5, Md=2)
    kt = np.array([[2 ** 32 - 1, 0, 1, 1, 1], [0, 1, 2, 3, 4]], dtype=np.uint32)
    np.savez(tmp_path / "m.npz", v_template=m["v_template"], shapedirs=m["shapedirs"], posedirs=m["posedirs"], J_regressor=m["J_regressor"],
             kintree_table=kt, weights=m["weights"], f=m["faces"], static_lmk_faces_idx=m["lmk_face"], static_lmk_bary_coords=m["lmk_bary"],
             dynamic_lmk_faces_idx=m["dyn_lmk_face"], dynamic_lmk_bary_coords=m["dyn_lmk_bary"])
    d = MM.read_model_file(tmp_path / "m.npz")
    assert d["dynamic_lmk_faces_idx"].shape == (5, 2) and d["dynamic_lmk_bary_coords"].shape == (5, 2, 3)
    fm = MM.MorphableModel.load(tmp_path / "m.npz", device="cpu")
    assert fm.neck_joint == 1 and tuple(fm.dyn_lmk_face.shape) == (5, 2) and fm.ct_ptr.shape[0] == fm.ct_vert.shape[0] + 1
    assert fm.ct_ent.shape[0] == 5 * 2 * 3
    with pytest.raises(ValueError, match="R odd"):
        MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"],
                                      faces=m["faces"], dyn_lmk_face=m["dyn_lmk_face"][:4], dyn_lmk_bary=m["dyn_lmk_bary"][:4], device="cpu")
    with pytest.raises(ValueError, match="runs on the GPU only"):
        fm.fit_2d(np.zeros((2, 3, 2)), *R2.cameras([0.0, 20.0]))
    with pytest.raises(ValueError, match="3 static landmarks"):
        fm.fit_2d(np.zeros((2, 4, 2)), *R2.cameras([0.0, 20.0]))
    with pytest.raises(ValueError, match="ibug68"):
        fm.fit_2d(np.zeros((2, 68, 2)), *R2.cameras([0.0, 20.0]), landmark_order="ibug68")

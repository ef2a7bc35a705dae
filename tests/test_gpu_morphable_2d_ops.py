"""GPU: the 2-D multi-view landmark term and the per-view contour landmarks, one mvd_op_* entry at a time (csrc/k_morph_2d.hip)
against tests/morphable_2d_ref.py.  The projection has a forward-error bound for any fp32 order (morphable_2d_ref.project_bound)
and must give mvd_op_mesh_project's integers exactly; E2 and the gradients may differ from the float64 oracle by at most 4 times
what the same formulas in float32 differ from it (the rule of tests/test_gpu_morphable_bwd_ops.py); counts and rows are exact."""
import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from tests import morphable_2d_ref as R2
from tests import morphable_bwd_ref as BR
from tests import morphable_ref as R
from tests.test_morphable_2d_cpu import check_entry_errors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, NB, J, NECK, Z_NEAR, PX, LAM = 257, 12, 5, 1, 1e-3, 1.0 / 512, 1.7
# (F, C, M, Md, R, Fc, Ft); Md = 0: no contour set.  M + Md crosses a wave of 64 and, in the last case, a block of 256 points
CASES = [(1, 1, 1, 1, 5, 1, 1), (3, 2, 51, 17, 79, 1, 1), (3, 5, 70, 17, 79, 3, 3), (3, 5, 70, 1, 5, 1, 3), (1, 5, 51, 17, 5, 1, 1),
         (3, 1, 70, 0, 5, 3, 1), (3, 2, 300, 17, 5, 3, 3)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def num(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ring(C, Fc):
    """The validated camera ring (tests/test_morphable_2d_cpu.py keeps every (frame, camera) yaw off the rounding boundaries): shared,
    or per frame the same ring rolled by the frame index."""
    K, RT = R2.cameras(R2.OP_YAWS)
    if Fc == 1:
        return K[:C], RT[:C]
    idx = [[(c + f) % 5 for c in range(C)] for f in range(Fc)]
    return K[idx], RT[idx]


_cache = {}


def case(F, C, M, Md, Rr, Fc, Ft):
    """Inputs as the kernels get them (float32 values) and the float64 / float32 oracles of the term on them, computed once."""
    key = (F, C, M, Md, Rr, Fc, Ft)
    if key in _cache:
        return _cache[key]
    m = R.synthetic_model(5, V, NB, J, M=M, parents=[-1, 0, 1, 1, 1])
    betas, pose = R.seeded_params(7, F, NB, J)
    fw = BR.forward(BR.Folded(m), betas, pose)
    K, RT = ring(C, Fc)
    g = np.random.default_rng(F * 100 + C * 10 + M)
    c = dict(model=m, betas=betas, pose=pose, A=fw["A"].astype(np.float32), verts=fw["vertices"].astype(np.float32), K=K, RT=RT,
             lmk=fw["landmarks"].astype(np.float32))
    uv = R2.project(c["lmk"], K, RT, Z_NEAR)["uv"]
    c["target_uv"] = (uv[:Ft] + g.normal(size=(Ft, C, M, 2)) * 3).astype(np.float32)
    c["weight"] = (g.random((Ft, C, M)) * (g.random((Ft, C, M)) > 0.15)).astype(np.float32) if M > 1 else None
    c["dyn_lmk"] = c["dyn_target_uv"] = c["dyn_weight"] = None
    if Md:
        c["dyn_face"], c["dyn_bary"] = R2.synthetic_contour(3, m, Rr, Md)
        c["rows"], c["yaw"] = R2.contour_select(c["A"], RT, NECK, Rr)
        c["dyn_lmk"] = R2.contour_landmarks(c["verts"], m["faces"], c["dyn_face"], c["dyn_bary"], c["rows"]).astype(np.float32)
        duv = R2.project(c["dyn_lmk"], K, RT, Z_NEAR, per_view=True)["uv"]
        c["dyn_target_uv"] = (duv[:Ft] + g.normal(size=(Ft, C, Md, 2)) * 3).astype(np.float32)
        c["dyn_weight"] = (g.random((Ft, C, Md)) + 0.1).astype(np.float32)
    c["term_kw"] = {k: c[k] for k in ("lmk", "K", "RT", "target_uv", "weight", "dyn_lmk", "dyn_target_uv", "dyn_weight")}
    c["o64"] = R2.term(**c["term_kw"], z_near=Z_NEAR, px_scale=PX, lambda2=LAM)
    c["o32"] = R2.term(**c["term_kw"], z_near=Z_NEAR, px_scale=PX, lambda2=LAM, dtype=np.float32)
    _cache[key] = c
    return c


def run_term(c, **over):
    kw = {**c["term_kw"], **over}
    lmk = kw.pop("lmk")
    K, RT, tu = kw.pop("K"), kw.pop("RT"), kw.pop("target_uv")
    return E.op_morph_fit_data_2d(dev(lmk), dev(K), dev(RT), dev(tu), z_near=Z_NEAR, px_scale=PX, lambda2=LAM,
                                  **{k: dev(v) for k, v in kw.items()})


OUTS = ("uv", "dyn_uv", "E2", "n_valid", "g_lmk", "g_dyn", "inv_w")


def same_bits(a, b, keys=OUTS):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


@pytest.mark.parametrize("F,C,M,Md,Rr,Fc,Ft", CASES)
def test_uv_is_mesh_projects_chain_to_the_bit(F, C, M, Md, Rr, Fc, Ft):
    c = case(F, C, M, Md, Rr, Fc, Ft)
    uv, valid = E.op_morph_project(dev(c["lmk"]), dev(c["K"]), dev(c["RT"]), Z_NEAR)
    got = run_term(c)
    assert torch.equal(uv.view(torch.int32), got["uv"].view(torch.int32)) and valid.all()
    for f in range(F):
        K, RT = (c["K"], c["RT"]) if Fc == 1 else (c["K"][f], c["RT"][f])
        xy, key = E.op_mesh_project(dev(c["lmk"][f]), dev(K), dev(RT), Z_NEAR)
        assert (key > 0).all()
        assert torch.equal(torch.round(uv[f] * 16).to(torch.int32), xy), f
    bound = R2.project_bound(c["lmk"], c["K"], c["RT"])
    err = np.abs(num(uv) - c["o64"]["uv"])
    print(f"uv F={F} C={C} M={M}: worst error / bound {np.max(err / bound):.3f} (largest error {err.max():.2e} px)")
    assert (err <= bound).all()
    if Md:
        err = np.abs(num(got["dyn_uv"]) - c["o64"]["dyn_uv"])
        assert (err <= R2.project_bound(c["dyn_lmk"], c["K"], c["RT"], per_view=True)).all()


@pytest.mark.parametrize("F,C,M,Md,Rr,Fc,Ft", CASES)
def test_term_and_gradient_against_the_oracle(F, C, M, Md, Rr, Fc, Ft):
    c = case(F, C, M, Md, Rr, Fc, Ft)
    got, o64, o32 = run_term(c), c["o64"], c["o32"]
    assert np.array_equal(got["n_valid"].cpu().numpy(), o64["n_valid"]) and (o64["n_valid"] > 0).all()
    assert np.allclose(num(got["inv_w"]), 1.0 / o64["W"], rtol=1e-5)
    for k in ("E2", "g_lmk") + (("g_dyn",) if Md else ()):
        err, yard = np.abs(num(got[k]) - o64[k]).max(), np.abs(o32[k].astype(np.float64) - o64[k]).max()
        print(f"{k} F={F} C={C} M={M} Md={Md}: worst error {err:.3e}, float32 oracle {yard:.3e}, ratio {err / yard:.2f}")
        assert err <= 4 * yard, k
    # E_add is one rounded addition
    base = torch.tensor([0.25, -3.0, 1e-3][:F], device=DEV)
    with_add = E.op_morph_fit_data_2d(dev(c["lmk"]), dev(c["K"]), dev(c["RT"]), dev(c["target_uv"]), weight=dev(c["weight"]),
                                      dyn_lmk=dev(c["dyn_lmk"]), dyn_target_uv=dev(c["dyn_target_uv"]), dyn_weight=dev(c["dyn_weight"]),
                                      z_near=Z_NEAR, px_scale=PX, lambda2=LAM, E_add=base)
    assert torch.equal(with_add["E2"], base + got["E2"])
    same_bits(got, with_add, ("uv", "g_lmk", "n_valid", "inv_w"))


def test_two_calls_agree_and_a_frame_of_a_batch_is_the_frame_alone():
    for key in (CASES[2], CASES[6], CASES[5]):
        c = case(*key)
        F, Fc, Ft = key[0], key[5], key[6]
        a, b = run_term(c), run_term(c)
        same_bits(a, b)
        for f in range(F):
            cut = lambda x, n: None if x is None else (x[f:f + 1] if n == F and x.shape[0] == F else x)
            one = run_term(c, lmk=c["lmk"][f:f + 1], K=cut(c["K"], Fc) if Fc > 1 else c["K"], RT=cut(c["RT"], Fc) if Fc > 1 else c["RT"],
                           target_uv=cut(c["target_uv"], Ft), weight=cut(c["weight"], Ft), dyn_lmk=cut(c["dyn_lmk"], F),
                           dyn_target_uv=cut(c["dyn_target_uv"], Ft), dyn_weight=cut(c["dyn_weight"], Ft))
            for k in OUTS:
                if a[k] is not None:
                    x, y = a[k][f:f + 1], one[k]
                    assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                       y.view(torch.int32) if y.dtype == torch.float32 else y), (key, f, k)


def test_what_does_not_count_leaves_no_trace():
    c = case(*CASES[2])
    base = run_term(c)
    F, C, M = 3, 5, 70
    # weight 0 with a NaN target: no output bit changes
    tgt = c["target_uv"].copy()
    tgt[c["weight"] == 0] = np.nan
    assert (c["weight"] == 0).sum() > 10
    same_bits(base, run_term(c, target_uv=tgt))
    # a landmark behind the cameras, one nearer than z_near, one NaN: not counted, gradient exactly 0, the rest finite
    lmk = c["lmk"].copy()
    RT0 = c["RT"][0, 0].astype(np.float64)
    centre = -RT0[:, :3].T @ RT0[:, 3]
    lmk[0, 3] = (0.0, 0.0, 4.0)  # behind every camera of the ring: they sit at distance 1 on the +z side and look at the origin
    lmk[0, 4] = centre + RT0[2, :3] * 5e-4  # in front of camera (0, 0) by less than z_near
    lmk[1, 5] = np.nan
    got, want = run_term(c, lmk=lmk), R2.term(**{**c["term_kw"], "lmk": lmk}, z_near=Z_NEAR, px_scale=PX, lambda2=LAM)
    assert np.array_equal(got["n_valid"].cpu().numpy(), want["n_valid"]) and (want["n_valid"] < c["o64"]["n_valid"])[:2].all()
    assert (got["g_lmk"][0, 3] == 0).all() and (got["g_lmk"][1, 5] == 0).all()
    assert torch.isfinite(got["E2"]).all() and torch.isfinite(got["g_lmk"]).all() and torch.isnan(got["uv"][1, :, 5]).all()
    assert np.allclose(num(got["E2"]), want["E2"], rtol=1e-4) and np.allclose(num(got["g_lmk"]), want["g_lmk"], rtol=1e-3, atol=1e-8)
    same_bits({k: base[k][2:] for k in ("E2", "g_lmk", "g_dyn", "n_valid")}, {k: got[k][2:] for k in ("E2", "g_lmk", "g_dyn", "n_valid")},
              ("E2", "g_lmk", "g_dyn", "n_valid"))
    # a frame with every weight 0: E2 = 0 and zero gradients exactly, the other frames untouched
    w, dw = c["weight"].copy(), c["dyn_weight"].copy()
    w[1], dw[1] = 0, 0
    z = run_term(c, weight=w, dyn_weight=dw)
    assert z["E2"][1] == 0 and z["n_valid"][1] == 0 and z["inv_w"][1] == 0 and (z["g_lmk"][1] == 0).all() and (z["g_dyn"][1] == 0).all()
    for f in (0, 2):
        same_bits({k: base[k][f] for k in OUTS}, {k: z[k][f] for k in OUTS})


@pytest.mark.parametrize("F,C,M,Md,Rr,Fc,Ft", [k for k in CASES if k[3]])
def test_contour_rows_and_landmarks(F, C, M, Md, Rr, Fc, Ft):
    c = case(F, C, M, Md, Rr, Fc, Ft)
    m = c["model"]
    # the rows from the pose kernel's own A, and from the oracle's
    pr = E.op_morph_pose(dev(c["betas"]), dev(c["pose"]), *(dev(a.astype(np.float32)) for a in R.fold(
        m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"])[:2]), m["parents"])
    for A in (pr["A"], dev(c["A"])):
        row, yaw = E.op_morph_contour_select(A, dev(c["RT"]), NECK, Rr)
        assert np.array_equal(row.cpu().numpy(), c["rows"]) and np.abs(num(yaw) - c["yaw"]).max() < 1e-3
    faces, df, db = dev(m["faces"]), dev(c["dyn_face"]), dev(c["dyn_bary"])
    dyn = E.op_morph_contour_landmarks(dev(c["verts"]), faces, df, db, row)
    want = R2.contour_landmarks(c["verts"], m["faces"], c["dyn_face"], c["dyn_bary"], c["rows"])
    tri = m["faces"][c["dyn_face"][c["rows"]]]
    x = np.abs(c["verts"].astype(np.float64))[np.arange(F)[:, None, None, None], tri]
    bound = R.gamma(3) * np.einsum("fcdki,fcdk->fcdi", x, np.abs(c["dyn_bary"].astype(np.float64))[c["rows"]])
    assert (np.abs(num(dyn) - want) <= bound).all()
    assert torch.equal(dyn, E.op_morph_contour_landmarks(dev(c["verts"]), faces, df, db, row))
    # a face outside the mesh: NaN landmarks, nothing dereferenced; their observations drop out of the term
    bad = c["dyn_face"].copy()
    bad[c["rows"][0, 0], 0], bad[c["rows"][-1, -1], Md - 1] = 2 ** 30, -7
    dyn_bad = E.op_morph_contour_landmarks(dev(c["verts"]), faces, dev(bad), db, row)
    hole = np.isnan(R2.contour_landmarks(c["verts"], m["faces"], bad, c["dyn_bary"], c["rows"]))
    assert hole.any() and np.array_equal(torch.isnan(dyn_bad).cpu().numpy(), hole)
    assert torch.equal(dyn_bad[~torch.from_numpy(hole).to(DEV)], dyn[~torch.from_numpy(hole).to(DEV)])
    got = run_term(c, dyn_lmk=dyn_bad.cpu().numpy())
    want_t = R2.term(**{**c["term_kw"], "dyn_lmk": dyn_bad.cpu().numpy()}, z_near=Z_NEAR, px_scale=PX, lambda2=LAM)
    assert np.array_equal(got["n_valid"].cpu().numpy(), want_t["n_valid"]) and (got["g_dyn"][torch.from_numpy(hole).to(DEV)] == 0).all()
    assert torch.isfinite(got["E2"]).all() and torch.isfinite(got["g_dyn"]).all()


@pytest.mark.parametrize("Rr,Md,C", [(5, 1, 2), (5, 4, 5), (79, 17, 5)])
def test_contour_bwd_is_the_adjoint_gather(Rr, Md, C):
    F = 3
    m = R.synthetic_model(5, V, NB, J, M=1, parents=[-1, 0, 1, 1, 1])
    df, db = R2.synthetic_contour(3, m, Rr, Md)
    df[Rr // 2, 0] = len(m["faces"]) + 1  # no entry in the table
    g = np.random.default_rng(4)
    # frame 0: every view the same row; frame 1: different rows (their first landmarks share a vertex); frame 2: seeded
    rows = np.stack([np.full(C, 1), np.arange(C) % Rr, g.integers(0, Rr, C)]).astype(np.int32)
    g_dyn, g_in = g.normal(size=(F, C, Md, 3)).astype(np.float32), g.normal(size=(F, V, 3)).astype(np.float32)
    table = tuple(dev(a) for a in E.contour_table(m["faces"], df, V))
    ones = np.ones_like(g_dyn, dtype=np.float64)
    terms = R2.contour_bwd(ones, rows, m["faces"], df, np.ones_like(db), V)  # how many products meet at a vertex
    assert terms.max() >= 2 and (terms[1].max() >= 2 or C == 1)
    for gi in (None, g_in):
        got = E.op_morph_contour_bwd(dev(g_dyn), dev(rows), table, dev(db), V, g_in=dev(gi))
        want = R2.contour_bwd(g_dyn, rows, m["faces"], df, db, V, gi)
        mag = R2.contour_bwd(np.abs(g_dyn), rows, m["faces"], df, np.abs(db), V, None if gi is None else np.abs(gi))
        bound = R.gamma(terms + 1) * mag * BR.SECOND_ORDER
        err = np.abs(num(got) - want)
        print(f"contour_bwd R={Rr} Md={Md} C={C} g_in={gi is not None}: worst error / bound "
              f"{np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)):.3f}")
        assert (err <= bound).all()
        untouched = terms[..., 0] == 0
        assert np.array_equal(got.cpu().numpy()[untouched], (np.zeros_like(g_in) if gi is None else gi)[untouched])
        assert torch.equal(got, E.op_morph_contour_bwd(dev(g_dyn), dev(rows), table, dev(db), V, g_in=dev(gi)))
        one = E.op_morph_contour_bwd(dev(g_dyn[1:2]), dev(rows[1:2]), table, dev(db), V, g_in=dev(None if gi is None else gi[1:2]))
        assert torch.equal(got[1:2], one)


def test_project_bwd_against_the_oracle():
    c = case(*CASES[2])
    g = np.random.default_rng(9)
    g_uv = g.normal(size=(3, 5, 70, 2)).astype(np.float32)
    lmk = c["lmk"].copy()
    lmk[2, 7] = -np.asarray(c["RT"][2, 1, :, :3], dtype=np.float64).T @ c["RT"][2, 1, :, 3] * 2.5  # behind camera (2, 1)
    got = E.op_morph_project_bwd(dev(lmk), dev(c["K"]), dev(c["RT"]), dev(g_uv), Z_NEAR)
    res = {}
    for dt in (np.float64, np.float32):
        pj = R2.project(lmk, c["K"], c["RT"], Z_NEAR, dt)
        gp = R2.pullback(np.where(pj["valid"][..., None], pj["cam"], 1).astype(dt), c["K"], c["RT"], g_uv.astype(dt), dt)
        res[dt] = np.where(pj["valid"][..., None], gp, 0).sum(1, dtype=dt)
    assert not R2.project(lmk, c["K"], c["RT"], Z_NEAR)["valid"][2, :, 7].all()
    err, yard = np.abs(num(got) - res[np.float64]).max(), np.abs(res[np.float32].astype(np.float64) - res[np.float64]).max()
    print(f"project_bwd: worst error {err:.3e}, float32 oracle {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= 4 * yard
    assert torch.equal(got, E.op_morph_project_bwd(dev(lmk), dev(c["K"]), dev(c["RT"]), dev(g_uv), Z_NEAR))


def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    torch.cuda.synchronize()
    check_entry_errors()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="1 or F"):
        E.op_morph_project(torch.zeros(3, 2, 3, device=DEV), torch.zeros(2, 1, 3, 3), torch.zeros(2, 1, 3, 4))
    with pytest.raises(ValueError, match="go together"):
        E.op_morph_fit_data_2d(torch.zeros(1, 2, 3, device=DEV), torch.zeros(1, 3, 3), torch.zeros(1, 3, 4), torch.zeros(1, 2, 2),
                               dyn_lmk=torch.zeros(1, 1, 1, 3))
    with pytest.raises(ValueError, match="px_scale"):
        E.op_morph_fit_data_2d(torch.zeros(1, 2, 3, device=DEV), torch.zeros(1, 3, 3), torch.zeros(1, 3, 4), torch.zeros(1, 2, 2), px_scale=-1.0)

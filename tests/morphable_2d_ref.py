"""numpy oracle of the 2-D multi-view landmark term and the per-view contour landmarks (csrc/k_morph_2d.hip), restated from their
definitions in include/mvd.h: the pinhole projection and its adjoint, the masked, weight-normalised squared reprojection error and
its gradient, the yaw of the head in a view and the row of the contour table it selects, the contour gather and its adjoint (a
scatter here, a gather in the kernel), and ``fit_oracle_2d``: the fitter's loop with Adam.  float64 by default; ``dtype=np.float32``
runs the same formulas in float32, which is the yardstick where no closed bound exists."""
import numpy as np

from tests import morphable_bwd_ref as BR
from tests import morphable_ref as R

U, gamma = R.U, R.gamma
OP_YAWS = (-52.3, 20.0, 0.2, 8.4, 33.3)  # the camera ring of the per-op tests, degrees about the model's y axis


def cameras(yaws_deg, dist=1.0, focal=800.0, skew=3.0, centre=(256.0, 250.0), pitch_deg=0.0):
    """A ring of cameras looking at the origin (x right, y down, z forward), one per yaw about the model's y axis (0 = frontal, on
    the +z side): K [C,3,3] with a non-zero skew K01, RT [C,3,4] world -> camera, float32."""
    Ks, RTs = [], []
    for i, yaw in enumerate(np.atleast_1d(yaws_deg)):
        a, b = np.deg2rad(yaw), np.deg2rad(pitch_deg)
        c = dist * np.array([np.sin(a) * np.cos(b), np.sin(b), np.cos(a) * np.cos(b)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, -1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        Rm = np.stack([x, y, z])
        RTs.append(np.concatenate([Rm, (-Rm @ c)[:, None]], 1))
        Ks.append([[focal + 5.0 * i, skew, centre[0]], [0.0, focal - 3.0 * i, centre[1]], [0.0, 0.0, 1.0]])
    return np.asarray(Ks, dtype=np.float32), np.asarray(RTs, dtype=np.float32)


def _cams(K, RT, F, dtype):
    K, RT = np.asarray(K, dtype=dtype), np.asarray(RT, dtype=dtype)
    K, RT = (K[None], RT[None]) if K.ndim == 3 else (K, RT)
    return np.broadcast_to(K, (F,) + K.shape[1:]), np.broadcast_to(RT, (F,) + RT.shape[1:])


def project(points, K, RT, z_near, dtype=np.float64, per_view=False):
    """points [F,M,3] (per_view: [F,C,M,3], view c's own points) -> dict of cam [F,C,M,3], uv [F,C,M,2], valid [F,C,M]."""
    p = np.asarray(points, dtype=dtype)
    F = p.shape[0]
    K, RT = _cams(K, RT, F, dtype)
    pv = p if per_view else p[:, None]
    with np.errstate(all="ignore"):
        cam = np.einsum("fcik,fcmk->fcmi", RT[..., :3], np.broadcast_to(pv, (F, K.shape[1]) + p.shape[-2:])) + RT[:, :, None, :, 3]
        X, Y, Z = cam[..., 0], cam[..., 1], cam[..., 2]
        u = (K[:, :, None, 0, 0] * X + K[:, :, None, 0, 1] * Y) / Z + K[:, :, None, 0, 2]
        v = K[:, :, None, 1, 1] * Y / Z + K[:, :, None, 1, 2]
        uv = np.stack([u, v], -1).astype(dtype)
        valid = (Z >= dtype(z_near)) & np.isfinite(cam).all(-1) & np.isfinite(uv).all(-1)
    return {"cam": cam, "uv": uv, "valid": valid}


def project_bound(points, K, RT, per_view=False):
    """A forward-error bound [F,C,M,2] of uv for ANY fp32 evaluation of the chain on these (exact) inputs, valid points only:
    |dcam_i| <= gamma_4 (sum_k |R_ik| |p_k| + |t_i|); the numerator of u takes gamma_3 more on its magnitude and the camera errors
    through |K|; the quotient one more rounding and the error of Z relatively; the final addition one rounding on the result."""
    p = np.asarray(points, dtype=np.float64)
    F = p.shape[0]
    K, RT = _cams(K, RT, F, np.float64)
    pj = project(p, K, RT, 1e-30, per_view=per_view)
    cam = pj["cam"]
    dcam = gamma(4) * (np.einsum("fcik,fcmk->fcmi" if per_view else "fcik,fmk->fcmi", np.abs(RT[..., :3]), np.abs(p)) +
                       np.abs(RT[:, :, None, :, 3]))
    aX, aY, aZ = (np.abs(cam[..., i]) for i in range(3))
    k00, k01, k11 = (np.abs(K[:, :, None, i, j]) for i, j in ((0, 0), (0, 1), (1, 1)))
    rz = dcam[..., 2] / aZ
    out = []
    for mag, dnum, res in ((k00 * aX + k01 * aY, k00 * dcam[..., 0] + k01 * dcam[..., 1], pj["uv"][..., 0]),
                           (k11 * aY, k11 * dcam[..., 1], pj["uv"][..., 1])):
        dn = gamma(3) * mag + dnum
        out.append((dn / aZ + (mag / aZ) * (rz + 2 * U)) * (1 + 4 * rz) + 2 * U * np.abs(res))
    return np.stack(out, -1) * BR.SECOND_ORDER


def pullback(cam, K, RT, duv, dtype=np.float64):
    """J^T duv: cam [F,C,M,3], duv [F,C,M,2] -> the gradient with respect to the world point [F,C,M,3]."""
    F = cam.shape[0]
    K, RT = _cams(K, RT, F, dtype)
    X, Y, Z = cam[..., 0], cam[..., 1], cam[..., 2]
    k00, k01, k11 = (K[:, :, None, i, j] for i, j in ((0, 0), (0, 1), (1, 1)))
    du, dv = duv[..., 0], duv[..., 1]
    g = np.stack([du * k00 / Z, (du * k01 + dv * k11) / Z, -(du * (k00 * X + k01 * Y) + dv * k11 * Y) / (Z * Z)], -1)
    return np.einsum("fcik,fcmi->fcmk", RT[..., :3], g).astype(dtype)


def term(lmk, K, RT, target_uv, weight=None, dyn_lmk=None, dyn_target_uv=None, dyn_weight=None, z_near=1e-3, px_scale=1.0, lambda2=1.0,
         dtype=np.float64):
    """mvd_op_morph_fit_data_2d: dict of uv, dyn_uv, E2 [F], n_valid [F], W [F], g_lmk [F,M,3], g_dyn [F,C,Md,3] (or None)."""
    lmk = np.asarray(lmk, dtype=dtype)
    F = lmk.shape[0]
    sets = [(project(lmk, K, RT, z_near, dtype), target_uv, weight)]
    if dyn_lmk is not None:
        sets.append((project(dyn_lmk, K, RT, z_near, dtype, per_view=True), dyn_target_uv, dyn_weight))
    res, W, E, n = [], np.zeros(F, dtype=dtype), np.zeros(F, dtype=dtype), np.zeros(F, dtype=np.int64)
    for pj, tgt, wt in sets:
        shape = pj["uv"].shape[:-1]
        tgt = np.broadcast_to(np.asarray(tgt, dtype=dtype).reshape((-1,) + shape[1:] + (2,)), shape + (2,))
        w = np.ones(shape, dtype=dtype) if wt is None else np.broadcast_to(np.asarray(wt, dtype=dtype).reshape((-1,) + shape[1:]), shape)
        ok = pj["valid"] & (w > 0)
        diff = np.where(ok[..., None], pj["uv"] - np.where(ok[..., None], tgt, 0), 0).astype(dtype)
        w = np.where(ok, w, 0).astype(dtype)
        r = dtype(px_scale) * diff
        E = E + (w * (r * r).sum(-1)).sum((1, 2), dtype=dtype)
        W = W + w.sum((1, 2), dtype=dtype)
        n = n + ok.sum((1, 2))
        res.append((pj, diff, w))
    inv = np.where(W > 0, dtype(1) / np.where(W > 0, W, 1), 0).astype(dtype)
    grads = []
    for pj, diff, w in res:
        cf = (dtype(2.0 * lambda2) * dtype(px_scale) * dtype(px_scale)) * w * inv[:, None, None]
        cam = np.where((w > 0)[..., None], pj["cam"], 1).astype(dtype)  # an uncounted observation contributes an exact zero
        grads.append(np.where((w > 0)[..., None], pullback(cam, K, RT, cf[..., None] * diff, dtype), 0).astype(dtype))
    return {"uv": res[0][0]["uv"], "dyn_uv": res[1][0]["uv"] if dyn_lmk is not None else None, "E2": (dtype(lambda2) * E * inv).astype(dtype),
            "n_valid": n, "W": W, "g_lmk": grads[0].sum(1, dtype=dtype), "g_dyn": grads[1] if dyn_lmk is not None else None}


def contour_row(yaw_deg, Rr):
    """The row of a table of Rr = 2 h + 1 rows: y = rint(min(yaw, h)) (half to even); y >= 0: y; -h <= y < 0: h - y; y < -h: 2 h."""
    h = (Rr - 1) // 2
    y = np.rint(np.minimum(np.asarray(yaw_deg, dtype=np.float64), h)).astype(np.int64)
    return np.where(y >= 0, y, np.where(y < -h, 2 * h, h - y)).astype(np.int32)


def contour_yaw(A, RT, neck_joint, dtype=np.float64):
    """yaw_deg [F,C] of the head in every view: Mx = S R_c G_neck with S = diag(1, -1, -1), -atan2(-Mx20, sqrt(Mx00^2 + Mx10^2))."""
    A = np.asarray(A, dtype=dtype)
    F = A.shape[0]
    G = A.reshape(F, -1, 3, 4)[:, neck_joint, :, :3]
    RT = np.asarray(RT, dtype=dtype)
    RT = np.broadcast_to(RT[None] if RT.ndim == 3 else RT, (F,) + RT.shape[-3:])
    Mx = np.einsum("ij,fcjk,fkl->fcil", np.diag([1.0, -1.0, -1.0]).astype(dtype), RT[..., :3], G)
    return (-np.arctan2(-Mx[..., 2, 0], np.sqrt(Mx[..., 0, 0] ** 2 + Mx[..., 1, 0] ** 2)) * dtype(180.0 / np.pi)).astype(dtype)


def contour_select(A, RT, neck_joint, Rr, dtype=np.float64):
    yaw = contour_yaw(A, RT, neck_joint, dtype)
    return contour_row(yaw, Rr), yaw


def contour_landmarks(verts, faces, dyn_face, dyn_bary, row, dtype=np.float64):
    """dyn_lmk [F,C,Md,3] from row[f,c] of the table; a face outside the mesh gives NaN."""
    v, faces, dyn_face = np.asarray(verts, dtype=dtype), np.asarray(faces), np.asarray(dyn_face)
    fsel = dyn_face[np.asarray(row)]  # [F,C,Md]
    ok = (fsel >= 0) & (fsel < len(faces))
    tri = faces[np.where(ok, fsel, 0)]  # [F,C,Md,3]
    x = v[np.arange(v.shape[0])[:, None, None, None], tri]  # [F,C,Md,corner,3]
    out = np.einsum("fcdki,fcdk->fcdi", x, np.asarray(dyn_bary, dtype=dtype)[np.asarray(row)])
    return np.where(ok[..., None], out, np.nan).astype(dtype)


def contour_matrix(faces, dyn_face, dyn_bary, row_f, V):
    """The forward gather of ONE frame as a dense matrix [C Md, V] (one scalar row per contour landmark; acts on each coordinate)."""
    faces, dyn_face, dyn_bary = np.asarray(faces), np.asarray(dyn_face), np.asarray(dyn_bary, dtype=np.float64)
    C, Md = len(row_f), dyn_face.shape[1]
    Mt = np.zeros((C * Md, V))
    for c in range(C):
        for d in range(Md):
            face = dyn_face[row_f[c], d]
            if 0 <= face < len(faces):
                for k in range(3):
                    Mt[c * Md + d, faces[face, k]] += dyn_bary[row_f[c], d, k]
    return Mt


def contour_bwd(g_dyn, row, faces, dyn_face, dyn_bary, V, g_in=None, dtype=np.float64):
    """mvd_op_morph_contour_bwd as a scatter: g_verts [F,V,3] = g_in + sum over (view, landmark, corner) of bary g_dyn."""
    g = np.asarray(g_dyn, dtype=dtype)
    F, C, Md = g.shape[:3]
    faces, dyn_face, dyn_bary = np.asarray(faces), np.asarray(dyn_face), np.asarray(dyn_bary, dtype=dtype)
    out = np.zeros((F, V, 3), dtype=dtype) if g_in is None else np.asarray(g_in, dtype=dtype).copy()
    for f in range(F):
        for c in range(C):
            for d in range(Md):
                face = dyn_face[row[f, c], d]
                if 0 <= face < len(faces):
                    for k in range(3):
                        out[f, faces[face, k]] += dyn_bary[row[f, c], d, k] * g[f, c, d]
    return out


def synthetic_contour(seed, model, Rr, Md, sliding=False):
    """A seeded contour table for a morphable_ref.synthetic_model: dyn_face [Rr,Md] int32, dyn_bary [Rr,Md,3] float32 (convex).
    sliding=False: a random face per (row, landmark), the first landmark of every row on a face that has the vertex faces[0,0] as a
    corner, so that different rows share a vertex.  sliding=True: as on a head, landmark d stays on one face and slides across it
    with the row, from b0 (row 0) towards b1 over the rows of positive yaw and towards b2 over those of negative yaw, so that
    neighbouring rows give neighbouring points."""
    g = np.random.default_rng(seed)
    faces = np.asarray(model["faces"])
    if sliding:
        h = (Rr - 1) // 2
        df = np.broadcast_to(g.integers(0, len(faces), (1, Md)), (Rr, Md)).astype(np.int32)
        b0, b1, b2 = (g.random((Md, 3)) + 0.05 for _ in range(3))
        t = (np.concatenate([np.arange(h + 1), np.arange(1, h + 1)]) / max(h, 1))[:, None, None]
        end = np.concatenate([np.broadcast_to(b1, (h + 1, Md, 3)), np.broadcast_to(b2, (h, Md, 3))])
        bc = (1 - t) * b0[None] + t * end
    else:
        df = g.integers(0, len(faces), (Rr, Md)).astype(np.int32)
        touching = np.nonzero((faces == faces[0, 0]).any(1))[0]
        df[:, 0] = touching[np.arange(Rr) % len(touching)]
        bc = g.random((Rr, Md, 3)) + 0.05
    return df, (bc / bc.sum(-1, keepdims=True)).astype(np.float32)


def head_model(seed=5, V=257, NB=12, M=51, Rr=79, Md=17, shape_scale=8.0):
    """The synthetic FLAME-shaped model of the fit tests (5 joints, the neck a child of the root), with M static and Rr x Md contour
    landmarks; the blend shapes are scaled up so that a few pixels of reprojection error separate the start from the target."""
    m = R.synthetic_model(seed, V, NB, 5, M=M, parents=[-1, 0, 1, 1, 1])
    m["shapedirs"] = (m["shapedirs"] * shape_scale).astype(np.float32)
    m["dyn_lmk_face"], m["dyn_lmk_bary"] = synthetic_contour(seed + 3, m, Rr, Md, sliding=True)
    m["neck_joint"] = 1
    return m


def landmarks_of(model, p, K, RT, post=None, z_near=1e-3, dtype=np.float64, rows=None):
    """Forward + selection + projection at the parameters p [F,P]: dict of fw (morphable_bwd_ref.forward), uv, valid and, with a
    contour table, rows, dyn_lmk, dyn_uv, dyn_valid.  rows: use these instead of selecting."""
    fm = BR.Folded(model, dtype)
    p = np.asarray(p, dtype=dtype)
    fw = BR.forward(fm, p[:, :fm.NB], p[:, fm.NB:fm.NB + 3 * fm.J], p[:, fm.NB + 3 * fm.J:], post)
    pj = project(fw["landmarks"], K, RT, z_near, dtype)
    out = {"fm": fm, "fw": fw, "uv": pj["uv"], "valid": pj["valid"]}
    if model.get("dyn_lmk_face") is not None:
        out["rows"] = contour_select(fw["A"], RT, model["neck_joint"], len(model["dyn_lmk_face"]), dtype)[0] if rows is None else rows
        out["dyn_lmk"] = contour_landmarks(fw["vertices"], model["faces"], model["dyn_lmk_face"], model["dyn_lmk_bary"], out["rows"], dtype)
        dj = project(out["dyn_lmk"], K, RT, z_near, dtype, per_view=True)
        out["dyn_uv"], out["dyn_valid"] = dj["uv"], dj["valid"]
    return out


def fit_oracle_2d(model, K, RT, target_uv, weight=None, dyn_target_uv=None, dyn_weight=None, target=None, vertex_weight=None, iters=100,
                  lr=0.05, lam=None, p0=None, init=None, z_near=1e-3, px_scale=1.0, lambda2=1.0, post=None, dtype=np.float64, keep=(),
                  fixed_rows=None, F=None):
    """The 2-D fitter's loop in ``dtype``: forward, landmarks, contour selection and landmarks (only with dyn_target_uv), the 3-D
    vertex term (only with ``target``), the 2-D term, both landmark adjoints, the model's vjp, Adam.  Dict of p [F,P],
    loss_history, n_valid_history, rows_history (or None), snapshots.  fixed_rows [F,C]: skip the selection (the row-0 ablation)."""
    fm = BR.Folded(model, dtype)
    P = fm.NB + 3 * fm.J + 3
    tu = np.asarray(target_uv, dtype=dtype)
    F = F or (tu.shape[0] if tu.ndim == 4 else 1)
    c = lambda a, fill: np.full(P, fill, dtype=dtype) if a is None else np.broadcast_to(np.asarray(a, dtype=dtype), (P,)).copy()
    lrv, lamv, p0v = c(lr, 0.0), c(lam, 0.0), c(p0, 0.0)
    p = np.zeros((F, P), dtype=dtype) if init is None else np.asarray(init, dtype=dtype).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    hist, nhist, rhist, snaps = np.zeros((iters, F), dtype=dtype), np.zeros((iters, F), dtype=np.int64), [], {}
    dyn = dyn_target_uv is not None
    for it in range(iters):
        betas, pose, transl = p[:, :fm.NB], p[:, fm.NB:fm.NB + 3 * fm.J], p[:, fm.NB + 3 * fm.J:]
        fw = BR.forward(fm, betas, pose, transl, post)
        E3, gv = np.zeros(F, dtype=dtype), None
        dl = rows = None
        if dyn:
            rows = fixed_rows if fixed_rows is not None else contour_select(fw["A"], RT, model["neck_joint"], len(model["dyn_lmk_face"]), dtype)[0]
            dl = contour_landmarks(fw["vertices"], model["faces"], model["dyn_lmk_face"], model["dyn_lmk_bary"], rows, dtype)
            rhist.append(np.array(rows))
        if target is not None:
            d3 = BR.fit_data(fw["vertices"], target, vertex_weight, dtype=dtype)
            E3, gv = d3["E"], d3["g_verts"]
        t = term(fw["landmarks"], K, RT, tu, weight, dl, dyn_target_uv, dyn_weight, z_near, px_scale, lambda2, dtype)
        hist[it], nhist[it] = E3 + t["E2"], t["n_valid"]
        if dyn:
            gv = contour_bwd(t["g_dyn"], rows, model["faces"], model["dyn_lmk_face"], model["dyn_lmk_bary"], fm.V, gv, dtype)
        g = BR.vjp(fm, betas, pose, transl, post, g_verts=gv, g_lmk=t["g_lmk"], fw=fw)
        BR.adam_step(p, BR.pack(g["betas"], g["pose"], g["transl"]).astype(dtype), m, v, lrv, lamv, p0v, it + 1)
        if it + 1 in keep:
            snaps[it + 1] = p.copy()
    return {"p": p, "loss_history": hist, "n_valid_history": nhist, "rows_history": np.array(rhist) if dyn else None, "snapshots": snaps}


def reprojection_px(model, p, K, RT, target_uv, weight=None, dyn_target_uv=None, dyn_weight=None, post=None, z_near=1e-3, rows=None,
                    which="all"):
    """The mean pixel distance [F,C] of the counted observations at the parameters p, in float64; which: "all", "static" or
    "contour"."""
    o = landmarks_of(model, p, K, RT, post, z_near, rows=rows)
    parts = []
    if which in ("all", "static"):
        parts.append((o["uv"], target_uv, weight, o["valid"]))
    if which in ("all", "contour") and dyn_target_uv is not None:
        parts.append((o["dyn_uv"], dyn_target_uv, dyn_weight, o["dyn_valid"]))
    tot, n = 0.0, 0
    for uv, tgt, w, ok in parts:
        tgt = np.broadcast_to(np.asarray(tgt, dtype=np.float64).reshape((-1,) + uv.shape[1:]), uv.shape)
        if w is not None:
            ok = ok & (np.broadcast_to(np.asarray(w).reshape((-1,) + uv.shape[1:-1]), uv.shape[:-1]) > 0)
        d = np.sqrt((np.where(ok[..., None], uv - np.where(ok[..., None], tgt, 0), 0) ** 2).sum(-1))
        tot, n = tot + d.sum(-1), n + ok.sum(-1)
    return tot / n


def fit_case(contours=False, F=2, yaws=(-30.0, 0.0, 30.0), seed=11, LR=0.05):
    """The inputs of the fit tests, shared by the CPU test (which asserts that the float64 loop converges on them) and the GPU test:
    the head model, 3 cameras, known parameters (expression, jaw, global pose, translation; shape zero) and their landmarks as
    targets.  Dict of model, K, RT, target_uv, dyn_target_uv (or None), truth [F,P], lr [P] (shape frozen), rows (of the truth)."""
    model = head_model()
    fm = BR.Folded(model)
    n_shape = 4
    K, RT = cameras(yaws)
    g = np.random.default_rng(seed)
    P = fm.NB + 3 * fm.J + 3
    truth = np.zeros((F, P))
    truth[:, n_shape:fm.NB] = g.normal(size=(F, fm.NB - n_shape)) * 1.0
    truth[:, fm.NB:fm.NB + 3] = g.normal(size=(F, 3)) * 0.08   # global pose
    truth[:, fm.NB + 6:fm.NB + 9] = g.normal(size=(F, 3)) * 0.15  # jaw
    truth[:, -3:] = g.normal(size=(F, 3)) * 0.01
    truth = truth.astype(np.float32).astype(np.float64)
    o = landmarks_of(model, truth, K, RT)
    lr = np.zeros(P)
    lr[n_shape:fm.NB] = lr[fm.NB:fm.NB + 3] = lr[fm.NB + 6:fm.NB + 9] = lr[-3:] = LR
    return {"model": model, "K": K, "RT": RT, "target_uv": o["uv"].astype(np.float32),
            "dyn_target_uv": o["dyn_uv"].astype(np.float32) if contours else None, "truth": truth, "lr": lr, "rows": o["rows"],
            "n_shape": n_shape}

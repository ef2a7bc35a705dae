"""numpy float64 oracle of the morphable-model forward (csrc/k_morph.hip), written from the formulas of linear blend skinning:
the three ops as the C ABI defines them, and the whole forward from the model arrays.  The pose op follows the textbook chain
(world transforms, then t - G j_rest), not the kernel's cancelled form, so that the kernel's restructuring is what gets tested.
The skin op returns, next to each value, a forward-error bound for ANY fp32 evaluation order of the same sums."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def gamma(n):
    return n * U / (1.0 - n * U)


def rodrigues(r, dtype=np.float64):
    """[..., 3] axis-angle -> [..., 3, 3]: angle = |r + 1e-8|, k = r / angle, R = I + sin K + (1 - cos) K^2, in ``dtype``."""
    r = np.asarray(r, dtype=dtype)
    q = r + dtype(1e-8)
    angle = np.sqrt((q * q).sum(-1, keepdims=True, dtype=dtype))
    k = r / angle
    K = np.zeros(r.shape[:-1] + (3, 3), dtype=dtype)
    K[..., 0, 1], K[..., 0, 2] = -k[..., 2], k[..., 1]
    K[..., 1, 0], K[..., 1, 2] = k[..., 2], -k[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -k[..., 1], k[..., 0]
    s, c = np.sin(angle)[..., None], np.cos(angle)[..., None]
    return np.eye(3, dtype=dtype) + s * K + (dtype(1.0) - c) * (K @ K)


def fold(v_template, shapedirs, posedirs, J_regressor):
    """(j_template [J,3], j_dirs [NB,3J], basis [NB + 9 (J-1), 3V]) of model arrays in the pickle's layout (posedirs [V,3,P] or
    [P,3V])."""
    vt, S, Jr = (np.asarray(a, dtype=np.float64) for a in (v_template, shapedirs, J_regressor))
    V, _, NB = S.shape
    P = np.asarray(posedirs, dtype=np.float64)
    P = P.reshape(3 * V, P.shape[2]).T if P.ndim == 3 else P
    return Jr @ vt, np.einsum("jv,vkn->njk", Jr, S).reshape(NB, -1), np.concatenate([S.reshape(3 * V, NB).T, P], 0)


def pose(betas, pose, j_template, j_dirs, parents, dtype=np.float64):
    """mvd_op_morph_pose: dict of j_rest [F,J,3], rot [F,J,3,3], pose_feature [F,9 (J-1)], joints [F,J,3], A [F,J,3,4].
    dtype=np.float32 runs the same textbook chain in float32: what the reference's own arithmetic loses on these inputs."""
    betas, pose, jt, jd = (np.asarray(a, dtype=dtype) for a in (betas, pose, j_template, j_dirs))
    F, J = pose.shape[:2]
    j_rest = jt[None] + (betas @ jd).reshape(F, J, 3)
    R = rodrigues(pose, dtype)
    G = np.zeros((F, J, 3, 3), dtype=dtype)
    t = np.zeros((F, J, 3), dtype=dtype)
    for j in range(J):
        p = parents[j]
        if j == 0:
            G[:, 0], t[:, 0] = R[:, 0], j_rest[:, 0]
        else:
            G[:, j] = G[:, p] @ R[:, j]
            t[:, j] = np.einsum("fik,fk->fi", G[:, p], j_rest[:, j] - j_rest[:, p]) + t[:, p]
    a = t - np.einsum("fjik,fjk->fji", G, j_rest)
    return {"j_rest": j_rest, "rot": R, "pose_feature": (R[:, 1:] - np.eye(3, dtype=dtype)).reshape(F, -1), "joints": t,
            "A": np.concatenate([G, a[..., None]], -1)}


def _affine(T, dT, b, db):
    """out_i = sum_k T_ik b_k + T_i3 with its bound: T [...,3,4] with error dT, b [...,3] with error db."""
    out = np.einsum("...ik,...k->...i", T[..., :3], b) + T[..., 3]
    mag = np.einsum("...ik,...k->...i", np.abs(T[..., :3]), np.abs(b)) + np.abs(T[..., 3])
    err = gamma(4) * mag + np.einsum("...ik,...k->...i", dT[..., :3], np.abs(b)) + \
        np.einsum("...ik,...k->...i", np.abs(T[..., :3]), db) + dT[..., 3]
    return out, err


def skin(basis, v_template, coef, weights, A, post=None):
    """mvd_op_morph_skin: (verts [F,V,3], bound [F,V,3]).  The inputs are taken as exact (pass them as the kernel gets them,
    rounded to float32).  |db_k| <= gamma_{L+1} (|t_k| + sum_l |c_l| |B_lk|); |dT| <= gamma_J sum_j |w_j| |A_j|; one affine
    step |dout_i| <= gamma_4 (sum_k |T_ik| |b_k| + |T_i3|) + sum_k (|dT_ik| |b_k| + |T_ik| |db_k|) + |dT_i3|, once more for
    post; times (1 + 2^-10) for the second-order terms."""
    Bm, vt, c, W = (np.asarray(a, dtype=np.float64) for a in (basis, v_template, coef, weights))
    F, L = c.shape
    V, J = W.shape
    A = np.asarray(A, dtype=np.float64).reshape(F, J, 12)
    b = (vt.reshape(1, -1) + c @ Bm).reshape(F, V, 3)
    db = gamma(L + 1) * (np.abs(vt).reshape(1, -1) + np.abs(c) @ np.abs(Bm)).reshape(F, V, 3)
    T = np.einsum("vj,fje->fve", W, A).reshape(F, V, 3, 4)
    dT = gamma(J) * np.einsum("vj,fje->fve", np.abs(W), np.abs(A)).reshape(F, V, 3, 4)
    out, err = _affine(T, dT, b, db)
    if post is not None:
        Pm = np.broadcast_to(np.asarray(post, dtype=np.float64).reshape(3, 4), (F, V, 3, 4))
        out, err = _affine(Pm, np.zeros_like(Pm), out, err)
    return out, err * (1.0 + 2.0 ** -10)


def landmarks(verts, faces, lmk_face, lmk_bary):
    """mvd_op_morph_landmarks: (out [F,M,3], bound [F,M,3] = gamma_3 sum_c |w_c| |x_c|)."""
    v, w = np.asarray(verts, dtype=np.float64), np.asarray(lmk_bary, dtype=np.float64)
    tri = np.asarray(faces)[np.asarray(lmk_face)]  # [M,3]
    x = v[:, tri]  # [F,M,3 corners,3]
    return np.einsum("fmck,mc->fmk", x, w), gamma(3) * np.einsum("fmck,mc->fmk", np.abs(x), np.abs(w))


def forward(model, betas, pose_aa, post=None):
    """The whole forward from model arrays (dict with the pickle's key names, ``parents``, optionally faces / lmk_face /
    lmk_bary): dict of vertices, joints, A, landmarks (or None)."""
    jt, jd, basis = fold(model["v_template"], model["shapedirs"], model["posedirs"], model["J_regressor"])
    betas = np.asarray(betas, dtype=np.float64)
    p = pose(betas, np.asarray(pose_aa, dtype=np.float64).reshape(len(betas), -1, 3), jt, jd, model["parents"])
    verts, _ = skin(basis, model["v_template"], np.concatenate([betas, p["pose_feature"]], 1), model["weights"], p["A"], post)
    lm = None
    if model.get("lmk_face") is not None:
        lm = landmarks(verts, model["faces"], model["lmk_face"], model["lmk_bary"])[0]
    return {"vertices": verts, "joints": p["joints"], "A": p["A"], "landmarks": lm}


def seeded_tree(J, seed, min_depth=0):
    """parents [J] with parents[0] = -1 and parents[i] < i: a spine of min_depth joints, the rest attached at random."""
    g = np.random.default_rng(seed)
    par = [-1] + [i - 1 if i <= min_depth else int(g.integers(0, i)) for i in range(1, J)]
    depth = [0] * J
    for i in range(1, J):
        depth[i] = depth[par[i]] + 1
    assert max(depth) >= min(min_depth, J - 1)
    return par


def synthetic_model(seed, V, NB, J, parents=None, M=0, zero_weight_columns=()):
    """A seeded model of FLAME's / SMPL-X's shapes in float32 (dict, the pickle's key names): template of about 0.1 in size,
    blend shapes of a few per cent of it, a sparse convex joint regressor, convex skinning weights with whole zero columns
    where asked, a triangle soup and M static landmarks."""
    g = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    Jr = g.random((J, V)) * (g.random((J, V)) < max(0.05, 2.0 / V))
    Jr[np.arange(J), g.integers(0, V, J)] += 0.5
    W = g.random((V, J)) ** 4
    for c in zero_weight_columns:
        W[:, c] = 0.0
    W[W.sum(1) == 0, 0] = 1.0
    Nf = max(1, 2 * V)
    m = {"v_template": f32(g.normal(size=(V, 3)) * 0.1), "shapedirs": f32(g.normal(size=(V, 3, NB)) * 0.004),
         "posedirs": f32(g.normal(size=(V, 3, 9 * (J - 1))) * 0.002), "J_regressor": f32(Jr / Jr.sum(1, keepdims=True)),
         "weights": f32(W / W.sum(1, keepdims=True)), "parents": list(parents) if parents is not None else seeded_tree(J, seed + 1),
         "faces": g.integers(0, V, (Nf, 3)).astype(np.int32), "lmk_face": None, "lmk_bary": None}
    if M:
        bc = g.random((M, 3))
        bc[0] = (1.0, 0.0, 0.0)
        m["lmk_face"], m["lmk_bary"] = g.integers(0, Nf, M).astype(np.int32), f32(bc / bc.sum(1, keepdims=True))
    return m


def seeded_params(seed, F, NB, J, zero_pose_frames=()):
    """(betas [F,NB], pose [F,J,3]) float32: betas of a few sigma, rotations up to about 0.6 rad, chosen frames at rest."""
    g = np.random.default_rng(seed)
    betas, pose_aa = g.normal(size=(F, NB)) * 1.5, g.normal(size=(F, J, 3)) * 0.35
    for f in zero_pose_frames:
        pose_aa[f] = 0.0
    return betas.astype(np.float32), pose_aa.astype(np.float32)

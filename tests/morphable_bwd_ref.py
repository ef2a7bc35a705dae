"""numpy oracle of the morphable-model backward and fitter (csrc/k_morph_bwd.hip): the vector-Jacobian products written from the
textbook chain of morphable_ref.pose (world transforms, a = t - G j_rest; Rodrigues through the cross-product matrix), not from
the kernel's cancelled form, forward-error bounds for the skin backward that hold for ANY fp32 order of the same sums, the data
term, Adam as torch.optim.Adam steps it, and ``fit_oracle``: the fitter's loop.  float64 by default; ``dtype=np.float32`` runs the
same formulas in float32, which is the yardstick for the kernels whose error has no closed bound."""
import numpy as np

from tests import morphable_ref as R

U, gamma = R.U, R.gamma
SECOND_ORDER = 1.0 + 2.0 ** -10


def rodrigues_vjp(r, gR, dtype=np.float64):
    """g_r [...,3] of morphable_ref.rodrigues for the cotangent gR [...,3,3]: q = r + 1e-8, angle = |q|, k = r / angle
    differentiated as written (finite at r = 0: the rotation generators)."""
    r, gR = np.asarray(r, dtype=dtype), np.asarray(gR, dtype=dtype)
    q = r + dtype(1e-8)
    angle = np.sqrt((q * q).sum(-1, keepdims=True, dtype=dtype))
    k = r / angle
    K = np.zeros(r.shape[:-1] + (3, 3), dtype=dtype)
    K[..., 0, 1], K[..., 0, 2] = -k[..., 2], k[..., 1]
    K[..., 1, 0], K[..., 1, 2] = k[..., 2], -k[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -k[..., 1], k[..., 0]
    s, c = np.sin(angle)[..., None], np.cos(angle)[..., None]
    Kt = np.swapaxes(K, -1, -2)
    gK = s * gR + (dtype(1.0) - c) * (gR @ Kt + Kt @ gR)
    g_s = (gR * K).sum((-1, -2), dtype=dtype)[..., None]
    g_1mc = (gR * (K @ K)).sum((-1, -2), dtype=dtype)[..., None]
    gk = np.stack([gK[..., 2, 1] - gK[..., 1, 2], gK[..., 0, 2] - gK[..., 2, 0], gK[..., 1, 0] - gK[..., 0, 1]], -1)
    g_angle = g_s * np.cos(angle) + g_1mc * np.sin(angle) - (gk * r).sum(-1, keepdims=True, dtype=dtype) / (angle * angle)
    return (gk / angle + g_angle * q / angle).astype(dtype)


def pose_vjp(betas, pose, j_template, j_dirs, parents, g_A=None, g_joints=None, g_pose_feature=None, dtype=np.float64):
    """mvd_op_morph_pose_bwd: {"betas" [F,NB], "pose" [F,J,3]} for the cotangents g_A [F,J,3,4], g_joints [F,J,3] and
    g_pose_feature [F,9 (J-1)] of morphable_ref.pose's outputs (None = zero)."""
    betas, pose, jt, jd = (np.asarray(a, dtype=dtype) for a in (betas, pose, j_template, j_dirs))
    F, J = pose.shape[:2]
    fw = R.pose(betas, pose, jt, jd, parents, dtype)
    jr, Rm, G = fw["j_rest"], fw["rot"], fw["A"][..., :3]
    zero = lambda *s: np.zeros(s, dtype=dtype)
    gA = zero(F, J, 3, 4) if g_A is None else np.asarray(g_A, dtype=dtype).reshape(F, J, 3, 4)
    gG, ga = gA[..., :3].copy(), gA[..., 3]
    gt = (zero(F, J, 3) if g_joints is None else np.asarray(g_joints, dtype=dtype).copy()) + ga  # a = t - G j_rest
    gG -= ga[..., :, None] * jr[..., None, :]
    gjr = -np.einsum("fjik,fji->fjk", G, ga)
    gR = zero(F, J, 3, 3)
    for j in range(J - 1, 0, -1):
        p = parents[j]
        Gp = G[:, p]
        gR[:, j] = np.einsum("fik,fil->fkl", Gp, gG[:, j])
        gG[:, p] += gG[:, j] @ np.swapaxes(Rm[:, j], -1, -2) + gt[:, j, :, None] * (jr[:, j] - jr[:, p])[:, None, :]
        grel = np.einsum("fik,fi->fk", Gp, gt[:, j])
        gjr[:, j] += grel
        gjr[:, p] -= grel
        gt[:, p] += gt[:, j]
    gR[:, 0] = gG[:, 0]
    gjr[:, 0] += gt[:, 0]
    if g_pose_feature is not None and J > 1:
        gR[:, 1:] += np.asarray(g_pose_feature, dtype=dtype).reshape(F, J - 1, 3, 3)
    return {"betas": (gjr.reshape(F, -1) @ jd.T).astype(dtype), "pose": rodrigues_vjp(pose, gR, dtype)}


def skin_bwd(g_y, weights, A, blend, basis, post=None):
    """mvd_op_morph_skin_bwd: dict of (value, bound) pairs for g_b [F,V,3], g_coef [F,L], g_A [F,J,3,4], g_transl [F,3].  The
    inputs are taken as exact (pass them as the kernel gets them).  With u = 2^-24: |dT| <= gamma_J sum |w| |A|; |dg_o| <=
    gamma_3 sum |P| |g_y|; |dg_b_k| <= gamma_3 sum_i |T_ik| |g_o_i| + sum_i (|dT_ik| |g_o_i| + |T_ik| |dg_o_i|); |dg_coef_l| <=
    gamma_3V sum_k |B_lk| |g_b_k| + sum_k |B_lk| |dg_b_k|; |dg_T| <= u |g_o| |b| + |dg_o| |b|; |dg_A| <= gamma_{V+1} sum_v |w|
    |g_T| + sum_v |w| |dg_T|, and the same form for g_transl; times (1 + 2^-10)."""
    gy, W, Bm, b = (np.asarray(a, dtype=np.float64) for a in (g_y, weights, basis, blend))
    F, V = gy.shape[:2]
    J = W.shape[1]
    A = np.asarray(A, dtype=np.float64).reshape(F, J, 12)
    T = np.einsum("vj,fje->fve", W, A).reshape(F, V, 3, 4)
    dT = gamma(J) * np.einsum("vj,fje->fve", np.abs(W), np.abs(A)).reshape(F, V, 3, 4)
    if post is None:
        go, dgo = gy, np.zeros_like(gy)
    else:
        P3 = np.asarray(post, dtype=np.float64).reshape(3, 4)[:, :3]
        go, dgo = gy @ P3, gamma(3) * (np.abs(gy) @ np.abs(P3))
    T3, dT3, ago = T[..., :3], dT[..., :3], np.abs(go)
    gb = np.einsum("fvik,fvi->fvk", T3, go)
    dgb = gamma(3) * np.einsum("fvik,fvi->fvk", np.abs(T3), ago) + np.einsum("fvik,fvi->fvk", dT3, ago) + \
        np.einsum("fvik,fvi->fvk", np.abs(T3), dgo)
    aB = np.abs(Bm)
    gc = gb.reshape(F, -1) @ Bm.T
    dgc = gamma(3 * V) * (np.abs(gb).reshape(F, -1) @ aB.T) + dgb.reshape(F, -1) @ aB.T
    gT = np.concatenate([go[..., :, None] * b[..., None, :], go[..., :, None]], -1)  # [F,V,3,4]
    agT = np.abs(gT)
    dgT = np.concatenate([(U * ago + dgo)[..., :, None] * np.abs(b)[..., None, :], dgo[..., :, None]], -1)
    aW = np.abs(W)
    gA = np.einsum("vj,fvik->fjik", W, gT)
    dgA = gamma(V + 1) * np.einsum("vj,fvik->fjik", aW, agT) + np.einsum("vj,fvik->fjik", aW, dgT)
    gtr, dgtr = go.sum(1), gamma(V + 1) * ago.sum(1) + dgo.sum(1)
    s = SECOND_ORDER
    return {"g_b": (gb, dgb * s), "g_coef": (gc, dgc * s), "g_A": (gA, dgA * s), "g_transl": (gtr, dgtr * s)}


def landmark_entries(faces, lmk_face, V):
    """Brute force: for every vertex the ascending list of entries landmark * 3 + corner that touch it."""
    tri = np.asarray(faces)[np.asarray(lmk_face).reshape(-1)]
    out = [[] for _ in range(V)]
    for m in range(tri.shape[0]):
        for c in range(3):
            out[int(tri[m, c])].append(m * 3 + c)
    return out


def landmarks_bwd(g_lmk, faces, lmk_face, lmk_bary, V, g_in=None):
    """mvd_op_morph_landmarks_bwd: (g_verts [F,V,3], bound [F,V,3] = gamma_n sum |w| |g| with n the entries at the vertex (one
    more with g_in))."""
    g, w = np.asarray(g_lmk, dtype=np.float64), np.asarray(lmk_bary, dtype=np.float64)
    F = g.shape[0]
    out = np.zeros((F, V, 3)) if g_in is None else np.asarray(g_in, dtype=np.float64).copy()
    mag, n = np.abs(out), np.zeros(V) + (g_in is not None)
    tri = np.asarray(faces)[np.asarray(lmk_face).reshape(-1)]
    for m in range(tri.shape[0]):
        for c in range(3):
            out[:, tri[m, c]] += w[m, c] * g[:, m]
            mag[:, tri[m, c]] += abs(w[m, c]) * np.abs(g[:, m])
            n[tri[m, c]] += 1
    return out, gamma(n)[None, :, None] * mag * SECOND_ORDER


def fit_data(verts, target=None, vertex_weight=None, lmk=None, target_lmk=None, lmk_weight=None, lmk_lambda=1.0, dtype=np.float64):
    """mvd_op_morph_fit_data before the landmark gather: dict of E [F], g_verts [F,V,3] (the vertex term's gradient), g_lmk
    [F,M,3] or None (the landmark term's, to be pulled back by landmarks_bwd)."""
    y = np.asarray(verts, dtype=dtype)
    F, V = y.shape[:2]
    E, gv, gl = np.zeros(F, dtype=dtype), np.zeros_like(y), None
    if target is not None:
        w = np.ones(V, dtype=dtype) if vertex_weight is None else np.asarray(vertex_weight, dtype=dtype)
        r = y - np.asarray(target, dtype=dtype)
        E = E + (w[None] * (r * r).sum(-1)).sum(-1) / w.sum()
        gv = dtype(2.0) * w[None, :, None] * r / w.sum()
    if target_lmk is not None:
        l = np.asarray(lmk, dtype=dtype)
        w = np.ones(l.shape[1], dtype=dtype) if lmk_weight is None else np.asarray(lmk_weight, dtype=dtype)
        r = l - np.asarray(target_lmk, dtype=dtype)
        E = E + dtype(lmk_lambda) * (w[None] * (r * r).sum(-1)).sum(-1) / w.sum()
        gl = dtype(2.0 * lmk_lambda) * w[None, :, None] * r / w.sum()
    return {"E": E.astype(dtype), "g_verts": gv.astype(dtype), "g_lmk": None if gl is None else gl.astype(dtype)}


class Folded:
    """A model dict of morphable_ref.synthetic_model folded once, in ``dtype``: what the forward and backward below read."""

    def __init__(self, model, dtype=np.float64):
        jt, jd, basis = R.fold(model["v_template"], model["shapedirs"], model["posedirs"], model["J_regressor"])
        c = lambda a: np.asarray(a, dtype=dtype)
        self.dtype, self.jt, self.jd, self.basis, self.vt, self.W = dtype, c(jt), c(jd), c(basis), c(model["v_template"]), c(model["weights"])
        self.parents, self.faces, self.lmk_face = list(model["parents"]), model.get("faces"), model.get("lmk_face")
        self.lmk_bary = None if model.get("lmk_bary") is None else c(model["lmk_bary"])
        self.V, self.J, self.NB = self.vt.shape[0], self.W.shape[1], self.jd.shape[0]


def forward(fm, betas, pose, transl=None, post=None):
    """The forward in fm.dtype with what the backward needs: dict of vertices, joints, landmarks (or None), A, blend, T."""
    dt = fm.dtype
    betas, pose = np.asarray(betas, dtype=dt), np.asarray(pose, dtype=dt).reshape(len(betas), fm.J, 3)
    F = betas.shape[0]
    p = R.pose(betas, pose, fm.jt, fm.jd, fm.parents, dt)
    coef = np.concatenate([betas, p["pose_feature"]], 1)
    b = (fm.vt.reshape(1, -1) + coef @ fm.basis).reshape(F, fm.V, 3)
    T = np.einsum("vj,fjik->fvik", fm.W, p["A"])
    o = np.einsum("fvik,fvk->fvi", T[..., :3], b) + T[..., 3]
    if transl is not None:
        o = o + np.asarray(transl, dtype=dt).reshape(F, 1, 3)
    y = o
    if post is not None:
        Pm = np.asarray(post, dtype=dt).reshape(3, 4)
        y = o @ Pm[:, :3].T + Pm[:, 3]
    lm = None
    if fm.lmk_face is not None:
        lm = np.einsum("fmck,mc->fmk", y[:, np.asarray(fm.faces)[np.asarray(fm.lmk_face)]], fm.lmk_bary)
    return {"vertices": y.astype(dt), "joints": p["joints"], "landmarks": lm, "A": p["A"], "blend": b, "T": T, "pose": pose, "betas": betas}


def vjp(fm, betas, pose, transl=None, post=None, g_verts=None, g_joints=None, g_lmk=None, fw=None):
    """{"betas", "pose", "transl"}: the cotangents of forward()'s vertices, joints and landmarks pulled back to the parameters."""
    dt = fm.dtype
    fw = fw or forward(fm, betas, pose, transl, post)
    F = fw["betas"].shape[0]
    gy = np.zeros((F, fm.V, 3), dtype=dt) if g_verts is None else np.asarray(g_verts, dtype=dt).copy()
    if g_lmk is not None:
        tri = np.asarray(fm.faces)[np.asarray(fm.lmk_face)]
        gl = np.asarray(g_lmk, dtype=dt)
        for c in range(3):
            np.add.at(gy, (slice(None), tri[:, c]), fm.lmk_bary[None, :, c, None] * gl)
    go = gy if post is None else gy @ np.asarray(post, dtype=dt).reshape(3, 4)[:, :3]
    T, b = fw["T"], fw["blend"]
    gb = np.einsum("fvik,fvi->fvk", T[..., :3], go)
    gcoef = gb.reshape(F, -1) @ fm.basis.T
    gT = np.concatenate([go[..., :, None] * b[..., None, :], go[..., :, None]], -1)
    gA = np.einsum("vj,fvik->fjik", fm.W, gT)
    g = pose_vjp(fw["betas"], fw["pose"], fm.jt, fm.jd, fm.parents, g_A=gA, g_joints=g_joints, g_pose_feature=gcoef[:, fm.NB:], dtype=dt)
    return {"betas": (g["betas"] + gcoef[:, :fm.NB]).astype(dt), "pose": g["pose"], "transl": go.sum(1).astype(dt)}


def pack(betas, pose, transl):
    F = len(betas)
    return np.concatenate([np.asarray(betas).reshape(F, -1), np.asarray(pose).reshape(F, -1), np.asarray(transl).reshape(F, 3)], 1)


def adam_step(p, g, m, v, lr, lam, p0, step, betas=(0.9, 0.999), eps=1e-8):
    """One torch.optim.Adam step on g' = g + 2 lam (p - p0) in p's dtype, in place; lr [P], 0 = frozen."""
    dt = p.dtype.type
    b1, b2 = dt(betas[0]), dt(betas[1])
    free = np.asarray(lr) != 0
    gg = g + dt(2.0) * lam * (p - p0)
    m[:, free] = (m + (dt(1.0) - b1) * (gg - m))[:, free]
    v[:, free] = (v * b2 + (dt(1.0) - b2) * gg * gg)[:, free]
    bias1, bias2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    denom = np.sqrt(v) / dt(bias2 ** 0.5) + dt(eps)
    step_size = (np.asarray(lr, dtype=np.float64) / bias1).astype(p.dtype)
    p[:, free] = (p - step_size * (m / denom))[:, free]


def fit_oracle(model, target=None, target_lmk=None, iters=300, lr=0.05, lam=None, p0=None, init=None, vertex_weight=None,
               lmk_weight=None, lmk_lambda=1.0, post=None, dtype=np.float64, keep=()):
    """The fitter's loop (forward, data term, vjp, Adam) in ``dtype``: dict of p [F,P] (betas | pose | transl), loss_history
    [iters,F], and snapshots {k: p after k iterations} for k in ``keep``.  lr: a number or [P] (0 = frozen)."""
    fm = Folded(model, dtype)
    P = fm.NB + 3 * fm.J + 3
    F = max(np.shape(t)[0] for t in (target, target_lmk) if t is not None)
    c = lambda a, fill: np.full(P, fill, dtype=dtype) if a is None else np.broadcast_to(np.asarray(a, dtype=dtype), (P,)).copy()
    lrv, lamv, p0v = c(lr, 0.0), c(lam, 0.0), c(p0, 0.0)
    p = np.zeros((F, P), dtype=dtype) if init is None else np.asarray(init, dtype=dtype).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    hist, snaps = np.zeros((iters, F), dtype=dtype), {}
    for it in range(iters):
        betas, pose, transl = p[:, :fm.NB], p[:, fm.NB:fm.NB + 3 * fm.J], p[:, fm.NB + 3 * fm.J:]
        fw = forward(fm, betas, pose, transl, post)
        d = fit_data(fw["vertices"], target, vertex_weight, fw["landmarks"], target_lmk, lmk_weight, lmk_lambda, dtype)
        hist[it] = d["E"]
        g = vjp(fm, betas, pose, transl, post, g_verts=d["g_verts"], g_lmk=d["g_lmk"], fw=fw)
        adam_step(p, pack(g["betas"], g["pose"], g["transl"]).astype(dtype), m, v, lrv, lamv, p0v, it + 1)
        if it + 1 in keep:
            snaps[it + 1] = p.copy()
    return {"p": p, "loss_history": hist, "snapshots": snaps}


def vertex_rms(fm_model, p, target, post=None):
    """The root mean square vertex distance [F] of the parameters p [F,P] to ``target``, in float64."""
    fm = Folded(fm_model)
    fw = forward(fm, p[:, :fm.NB], p[:, fm.NB:fm.NB + 3 * fm.J], p[:, fm.NB + 3 * fm.J:], post)
    return np.sqrt(((fw["vertices"] - np.asarray(target, dtype=np.float64)) ** 2).sum(-1).mean(-1))

"""The oracle of the closest-point query (include/mvd.h: mvd_op_mesh_closest_point), numpy only, written from the definition in
that header: the seven-region test in its fixed order, vectorised over queries x faces, in float64 or -- for the error bounds of
the GPU tests -- in float32; a second, independent derivation of the distance to a triangle (plane projection if inside, else the
best of three clamped segments) to check the first against; and the data term against correspondences with the ICP loop composed
from tests/morphable_bwd_ref.py.

The tolerance convention of the GPU tests: the worst error of the device against the float64 oracle may be at most 4 x the worst
error of this same oracle run in float32 on the same inputs (``bound``)."""
import numpy as np

U32 = 2.0 ** -24  # float32 unit roundoff


def _dot(x, y):
    return x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]


def _div(num, den):
    """num / den, 0 where den == 0 (the header's rule)."""
    safe = np.where(den != 0, den, 1)
    return np.where(den != 0, num / safe, 0)


def on_triangles(q, a, b, c):
    """Closest points of triangles (a, b, c) to points q, all [...,3] of one float dtype and broadcastable: (w [...,3], point
    [...,3], dist2 [...]), computed in that dtype with the regions in the header's order."""
    ab, ac = b - a, c - a
    d1, d2 = _dot(ab, q - a), _dot(ac, q - a)
    d3, d4 = _dot(ab, q - b), _dot(ac, q - b)
    d5, d6 = _dot(ab, q - c), _dot(ac, q - c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    s = (va + vb) + vc
    v, u = np.maximum(_div(vb, s), 0), np.maximum(_div(vc, s), 0)
    w = np.stack([np.maximum((1 - v) - u, 0), v, u], -1)  # interior
    t_ab, t_ac, t_bc = _div(d1, d1 - d3), _div(d2, d2 - d6), _div(e1, e1 + e2)
    regions = [  # in REVERSE order of priority: a later assignment overrides
        ((va <= 0) & (e1 >= 0) & (e2 >= 0), np.stack([zero, 1 - t_bc, t_bc], -1)),
        ((vb <= 0) & (d2 >= 0) & (d6 <= 0), np.stack([1 - t_ac, zero, t_ac], -1)),
        ((d6 >= 0) & (d5 <= d6), np.stack([zero, zero, one], -1)),
        ((vc <= 0) & (d1 >= 0) & (d3 <= 0), np.stack([1 - t_ab, t_ab, zero], -1)),
        ((d3 >= 0) & (d4 <= d3), np.stack([zero, one, zero], -1)),
        ((d1 <= 0) & (d2 <= 0), np.stack([one, zero, zero], -1))]
    for cond, wr in regions:
        w = np.where(cond[..., None], wr, w)
    p = w[..., 2:3] * c + (w[..., 1:2] * b + w[..., 0:1] * a)
    r = q - p
    return w, p, _dot(r, r)


def good_faces(verts, faces):
    """[Nf] bool: indices inside [0, Nv) and finite corners -- the faces the op does not skip."""
    f = np.asarray(faces, dtype=np.int64)
    ok = ((f >= 0) & (f < len(verts))).all(1)
    fin = np.isfinite(np.asarray(verts, dtype=np.float64)).all(1)
    ok[ok] &= fin[f[ok]].all(1)
    return ok


def face_normals(verts, faces, dtype=np.float64):
    v, f = np.asarray(verts).astype(dtype), np.clip(np.asarray(faces, dtype=np.int64), 0, len(verts) - 1)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def gate_cosines(normals, verts, faces):
    """[Q,Nf] float64: the cosine between each query normal and each face normal; +inf where either is zero (always passes)."""
    n, N = np.asarray(normals, dtype=np.float64), face_normals(verts, faces)
    den = np.linalg.norm(n, axis=1)[:, None] * np.linalg.norm(N, axis=1)[None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, (n @ N.T) / np.where(den > 0, den, 1), np.inf)


def distance_matrix(queries, verts, faces, dtype=np.float64):
    """dist2 [Q,Nf] of every query to every face in ``dtype``; +inf for skipped faces and for non-finite queries."""
    q, v = np.asarray(queries).astype(dtype), np.asarray(verts).astype(dtype)
    ok = good_faces(v, faces)
    f = np.where(ok[:, None], np.asarray(faces, dtype=np.int64), 0)
    with np.errstate(invalid="ignore", over="ignore"):
        _, _, d2 = on_triangles(q[:, None, :], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None])
    d2 = np.where(ok[None], d2, np.inf)
    return np.where(np.isfinite(d2), d2, np.inf)


def closest_point(queries, verts, faces, normals=None, cos_min=0.0, max_dist2=np.inf, dtype=np.float64):
    """The op in ``dtype``: {"face" int32 [Q] (-1: no match), "bary", "point" [Q,3], "dist2" [Q] (+inf: no match)}; the smallest
    distance, ties to the smallest face index (numpy's argmin returns the first)."""
    q, v = np.asarray(queries).astype(dtype), np.asarray(verts).astype(dtype)
    d2 = distance_matrix(q, v, faces, dtype)
    if normals is not None:
        n, N = np.asarray(normals).astype(dtype), face_normals(v, faces, dtype)
        with np.errstate(invalid="ignore"):
            ok = (n @ N.T) >= dtype(cos_min) * (np.sqrt(_dot(n, n))[:, None] * np.sqrt(_dot(N, N))[None])
        d2 = np.where(ok, d2, np.inf)
    face = np.argmin(d2, axis=1)
    best = d2[np.arange(len(q)), face]
    hit = np.isfinite(best) & (best <= max_dist2)
    f = np.asarray(faces, dtype=np.int64)[np.where(hit, face, 0)]
    f = np.where(hit[:, None], f, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        w, p, dd = on_triangles(q, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    z = np.zeros_like(w)
    return {"face": np.where(hit, face, -1).astype(np.int32), "bary": np.where(hit[:, None], w, z), "point": np.where(hit[:, None], p, z),
            "dist2": np.where(hit, dd, np.inf)}


def distance_to_faces(queries, verts, faces, face):
    """float64 distance of query i to face face[i] (+inf where face[i] < 0)."""
    q, v = np.asarray(queries, dtype=np.float64), np.asarray(verts, dtype=np.float64)
    hit = np.asarray(face) >= 0
    f = np.asarray(faces, dtype=np.int64)[np.where(hit, face, 0)]
    _, _, d2 = on_triangles(q, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    return np.where(hit, np.sqrt(d2), np.inf)


# ---- the second derivation: plane projection if inside, else the best of three clamped segments
def _segment_d2(q, a, b):
    ab = b - a
    t = np.clip(_div(_dot(q - a, ab), _dot(ab, ab)), 0.0, 1.0)
    r = q - (a + t[..., None] * ab)
    return _dot(r, r)


def on_triangles_alt(q, a, b, c):
    """dist2 [...] of q to triangles (a, b, c), float64, by projection: the foot of the perpendicular if it lies inside the
    triangle (three same-side tests against the edges), else the nearest of the three edges as clamped segments."""
    q, a, b, c = (np.asarray(x, dtype=np.float64) for x in (q, a, b, c))
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    h = _div(_dot(q - a, n), nn)
    foot = q - h[..., None] * n
    inside = (nn > 0) & (_dot(np.cross(b - a, foot - a), n) >= 0) & (_dot(np.cross(c - b, foot - b), n) >= 0) & \
        (_dot(np.cross(a - c, foot - c), n) >= 0)
    edges = np.minimum(np.minimum(_segment_d2(q, a, b), _segment_d2(q, b, c)), _segment_d2(q, c, a))
    return np.where(inside, h * h * nn, edges)


def bound(queries, verts, faces, want):
    """The convention's bound on |sqrt(dist2) - want|: 4 x the worst error of this oracle's float32 run (its minimum distance per
    query, ungated) against ``want`` [Q], the float64 one, over the finite entries.  Returns (bound, the float32 run's worst error)."""
    d32 = np.sqrt(distance_matrix(np.float32(queries), np.float32(verts), faces, np.float32).min(1).astype(np.float64))
    ok = np.isfinite(want)
    worst32 = float(np.abs(d32[ok] - want[ok]).max()) if ok.any() else 0.0
    return 4.0 * worst32, worst32


def statistics(dist):
    """mean / rms / median / p90 / max of the finite entries and their share, float64 (mesh.distance_statistics)."""
    d = np.asarray(dist, dtype=np.float64)
    ok = np.isfinite(d)
    d = d[ok]
    if d.size == 0:
        return {k: float("nan") for k in ("mean", "rms", "median", "p90", "max")} | {"matched": 0.0}
    return {"mean": float(d.mean()), "rms": float(np.sqrt((d * d).mean())), "median": float(np.percentile(d, 50)),
            "p90": float(np.percentile(d, 90)), "max": float(d.max()), "matched": d.size / ok.size}


def subdivide(verts, faces):
    """Every triangle split in four at its edge midpoints: the same piecewise-flat surface with 4 Nf faces."""
    v, mid, out = [np.asarray(p, dtype=np.float64) for p in verts], {}, []

    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            v.append(0.5 * (v[a] + v[b]))
            mid[k] = len(v) - 1
        return mid[k]
    for a, b, c in np.asarray(faces, dtype=np.int64):
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.asarray(v), np.asarray(out, dtype=np.int32)


# ---- the data term against correspondences and the ICP loop (the fitter of tests/morphable_bwd_ref.py with a moving target)
def fit_data_corr(verts, corr_point, corr_face, vertex_weight=None, lmk=None, target_lmk=None, lmk_weight=None, lmk_lambda=1.0,
                  dtype=np.float64):
    """mvd_op_morph_fit_data_corr before the landmark gather: dict of E [F], g_verts [F,V,3], g_lmk [F,M,3] or None, n_matched [F].
    corr_point is read only where corr_face >= 0."""
    from tests import morphable_bwd_ref as BR
    y = np.asarray(verts, dtype=dtype)
    F, V = y.shape[:2]
    m = np.asarray(corr_face) >= 0
    c = np.where(m[..., None], np.asarray(corr_point, dtype=dtype), 0)
    w = np.ones(V, dtype=dtype) if vertex_weight is None else np.asarray(vertex_weight, dtype=dtype)
    wm = w[None] * m
    W = wm.sum(1)
    inv = np.where(W > 0, 1 / np.where(W > 0, W, 1), 0).astype(dtype)
    r = np.where(m[..., None], y - c, 0)
    out = {"E": (wm * (r * r).sum(-1)).sum(1) * inv, "g_verts": (dtype(2.0) * wm * inv[:, None])[..., None] * r, "g_lmk": None,
           "n_matched": m.sum(1).astype(np.int32)}
    if target_lmk is not None:
        d = BR.fit_data(y, None, None, lmk, target_lmk, lmk_weight, lmk_lambda, dtype)
        out["E"], out["g_lmk"] = out["E"] + d["E"], d["g_lmk"]
    out["E"], out["g_verts"] = out["E"].astype(dtype), out["g_verts"].astype(dtype)
    return out


def correspondences(verts, scans, max_dist2=np.inf, dtype=np.float64):
    """(corr_point [F,V,3], corr_face [F,V]) of vertices [F,V,3] against scans [(verts, faces)], one shared or one per frame."""
    pts, faces = [], []
    for f in range(len(verts)):
        sv, sf = scans[0] if len(scans) == 1 else scans[f]
        c = closest_point(verts[f], sv, sf, max_dist2=max_dist2, dtype=dtype)
        pts.append(c["point"]), faces.append(c["face"])
    return np.stack(pts), np.stack(faces)


def icp_oracle(model, scans, iters=300, lr=0.05, refresh=1, max_dist2=np.inf, target_lmk=None, lmk_lambda=1.0, lam=None, p0=None, init=None,
               post=None, frames=None, dtype=np.float64, keep=()):
    """mvd_morph_fit_scan_run's loop in ``dtype`` (no normal gate): forward, closest points every ``refresh`` iterations, data
    term, vjp, Adam.  dict of p [F,P], loss_history, matched_history [iters,F] and snapshots {k: p after k iterations}."""
    from tests import morphable_bwd_ref as BR
    fm = BR.Folded(model, dtype)
    P = fm.NB + 3 * fm.J + 3
    F = max(len(scans), 1 if target_lmk is None else np.shape(target_lmk)[0], frames or 1, 1 if init is None else np.shape(init)[0])
    c = lambda a, fill: np.full(P, fill, dtype=dtype) if a is None else np.broadcast_to(np.asarray(a, dtype=dtype), (P,)).copy()
    lrv, lamv, p0v = c(lr, 0.0), c(lam, 0.0), c(p0, 0.0)
    p = np.zeros((F, P), dtype=dtype) if init is None else np.asarray(init, dtype=dtype).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    hist, matched, snaps = np.zeros((iters, F), dtype=dtype), np.zeros((iters, F), dtype=np.int32), {}
    sc = [(np.asarray(a).astype(dtype), b) for a, b in scans]
    for it in range(iters):
        betas, pose, transl = p[:, :fm.NB], p[:, fm.NB:fm.NB + 3 * fm.J], p[:, fm.NB + 3 * fm.J:]
        fw = BR.forward(fm, betas, pose, transl, post)
        if it % refresh == 0:
            cp, cf = correspondences(fw["vertices"], sc, max_dist2, dtype)
        d = fit_data_corr(fw["vertices"], cp, cf, None, fw["landmarks"], target_lmk, None, lmk_lambda, dtype)
        hist[it], matched[it] = d["E"], d["n_matched"]
        g = BR.vjp(fm, betas, pose, transl, post, g_verts=d["g_verts"], g_lmk=d["g_lmk"], fw=fw)
        BR.adam_step(p, BR.pack(g["betas"], g["pose"], g["transl"]).astype(dtype), m, v, lrv, lamv, p0v, it + 1)
        if it + 1 in keep:
            snaps[it + 1] = p.copy()
    return {"p": p, "loss_history": hist, "matched_history": matched, "snapshots": snaps}


def surface_rms(model, p, scans, post=None):
    """[F] float64: the root mean square distance of the model's vertices at parameters p [F,P] to the scan surface(s)."""
    from tests import morphable_bwd_ref as BR
    fm = BR.Folded(model)
    p = np.asarray(p, dtype=np.float64)
    y = BR.forward(fm, p[:, :fm.NB], p[:, fm.NB:fm.NB + 3 * fm.J], p[:, fm.NB + 3 * fm.J:], post)["vertices"]
    out = []
    for f in range(len(y)):
        sv, sf = scans[0] if len(scans) == 1 else scans[f]
        out.append(np.sqrt(distance_matrix(y[f], np.asarray(sv, dtype=np.float64), sf).min(1).mean()))
    return np.asarray(out)


def scan_case(seed=31, F=1, M=0, param_seed=1):
    """The fit-to-scan inputs: the icosphere(2, 0.1) topology with a non-symmetric template -- scaled by (1, 1.4, 0.7), with
    low-frequency bumps; a near-sphere slides under ICP and stalls -- and the seeded directions of synthetic_model(seed, 162, 10, 5);
    F frames posed at known parameters (betas 1.5 sigma, pose 0.1 rad, a translation of 0.01-0.02); each frame's scan is its posed
    surface with every triangle split in four (642 vertices, 1280 faces), vertices and faces shuffled.  ICP has local minima: of
    twelve (template, parameter seed) pairs tried, the float64 loop from zero reached a surface RMS below 1e-3 of its start for
    six and stalled at 0.3-0.75 for the others (param_seed 32 among them); param_seed 1 reaches 1e-6, and
    tests/test_closest_cpu.py asserts it.  Returns (model dict, p_true [F,P], scans [(verts float32, faces int32)] * F)."""
    from tests import mesh_ref as M_
    from tests import morphable_bwd_ref as BR
    from tests import morphable_ref as MR
    v, f = M_.icosphere(2, 0.1)
    x, y, z = v.T / 0.1
    bump = 1.0 + 0.15 * np.sin(2.0 * x + 0.5) * np.cos(1.5 * y) + 0.1 * np.sin(2.5 * z + 1.0) * x
    m = MR.synthetic_model(seed, 162, 10, 5, parents=[-1, 0, 1, 1, 1], M=M)
    m["v_template"] = np.float32(v * [1.0, 1.4, 0.7] * bump[:, None])
    m["faces"] = f
    if M:
        g0 = np.random.default_rng(seed + 5)
        m["lmk_face"] = g0.integers(0, len(f), M).astype(np.int32)
    g = np.random.default_rng(param_seed)
    betas, pose = g.normal(size=(F, 10)) * 1.5, g.normal(size=(F, 5, 3)) * 0.1
    d = g.normal(size=(F, 3))
    transl = d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(0.01, 0.02, (F, 1))
    p_true = BR.pack(betas, pose, transl)
    posed = BR.forward(BR.Folded(m), betas, pose.reshape(F, -1), transl)["vertices"]
    scans = []
    for fr in range(F):
        sv, sf = subdivide(posed[fr], f)
        pv, pf = g.permutation(len(sv)), g.permutation(len(sf))
        inv = np.empty_like(pv)
        inv[pv] = np.arange(len(pv))
        scans.append((np.float32(sv[pv]), inv[sf[pf]].astype(np.int32)))
    return m, p_true, scans

"""GPU: the closest-point query (csrc/k_closest.hip) and the data term against correspondences, one op at a time against the numpy
oracle tests/closest_ref.py.  Distances follow the project's convention: the worst error against the float64 oracle may be at most
4 x the worst error of the same oracle run in float32 on the same inputs; each test prints both.  Face indices are never compared
with the oracle's (two faces that share an edge are equally near, and float32 and float64 break the tie differently): instead the
float64 distance from the query to the RETURNED face must lie within the same bound of the float64 minimum.  Everything that is
defined exactly -- ties, no-match values, the key, independence of the slab count -- is compared for equality."""
import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from tests import closest_ref as R
from tests import mesh_ref as M
from tests.test_closest_cpu import abi_error_cases, query_set, sphere

pytestmark = pytest.mark.gpu

U = R.U32
INF = np.float32(np.inf)
NONE_KEY = (0x7F800000 << 32) | 0xFFFFFFFF


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(q, v, f, normals=None, **kw):
    out = E.op_mesh_closest_point(dev(np.float32(q)), dev(np.float32(v)), dev(np.int32(f)),
                                  query_normals=None if normals is None else dev(np.float32(normals)), **kw)
    out = {k: t.cpu().numpy() for k, t in out.items()}
    out["key"] = out["key"].view(np.uint64)
    return out


def check_invariants(out, v, f):
    """bary >= 0 and sums to 1 within 4u; point is the combination of the corners (three roundings: 3u sum |w_k x_k|); dist2's bits
    are the key's high word and face its low word; a no-match row holds exactly the no-match values."""
    hit = out["face"] >= 0
    assert out["face"].dtype == np.int32 and ((out["face"] >= -1) & (out["face"] < len(f))).all()
    assert (out["key"] & np.uint64(0xFFFFFFFF) == out["face"].astype(np.uint32)).all()
    assert ((out["key"] >> np.uint64(32)).astype(np.uint32) == out["dist2"].view(np.uint32)).all()
    miss = ~hit
    assert (out["key"][miss] == np.uint64(NONE_KEY)).all() and (out["dist2"][miss] == INF).all()
    assert (out["bary"][miss] == 0).all() and (out["point"][miss] == 0).all()
    w = out["bary"][hit].astype(np.float64)
    assert (w >= 0).all() and np.isfinite(out["dist2"][hit]).all()
    if hit.any():
        assert np.abs(w.sum(1) - 1).max() <= 4 * U
        c = np.float32(v).astype(np.float64)[np.int64(f)[out["face"][hit]]]  # [n,3 corners,3]
        comb, mag = (w[:, :, None] * c).sum(1), (w[:, :, None] * np.abs(c)).sum(1)
        assert (np.abs(out["point"][hit] - comb) <= 3 * U * mag + 1e-45).all()


def check_distances(out, q, v, f, bound, what, d2_ref=None):
    """sqrt(dist2), and the float64 distance to the returned face, within ``bound`` of the float64 minimum -- for every query."""
    q, v = np.float32(q), np.float32(v)
    want = np.sqrt((R.distance_matrix(q, v, f) if d2_ref is None else d2_ref).min(1))
    fin = np.isfinite(want)
    assert ((out["face"] >= 0) == fin).all(), what
    got = np.sqrt(out["dist2"].astype(np.float64))
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    back = R.distance_to_faces(q, v, f, out["face"])
    err_face = float(np.abs(back[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"{what}: |sqrt(dist2) - float64| = {err:.3e}, returned face's float64 distance off by {err_face:.3e}, bound {bound:.3e} "
          f"(ratios {err / bound if bound else 0:.3f}, {err_face / bound if bound else 0:.3f})")
    assert err <= bound and err_face <= bound, what


GROUPS = {"inside": slice(0, 60), "outside": slice(60, 160), "edge midpoints": slice(160, 640), "far": slice(640, 680)}


@pytest.fixture(scope="module")
def scene():
    """The mesh, the 680 queries (inside, outside, edge midpoints, far) and their float64 distance matrix: computed once."""
    v, f = sphere()
    q = query_set(v, f)
    return {"v": v, "f": f, "q": q, "d2": R.distance_matrix(q, v, f)}


def test_accuracy_over_inside_outside_edge_and_far_queries(scene):
    """The convention is applied to each group of queries by itself, which asks more than applying it to all 680 at once: the far
    queries' float32 error (an ulp of a distance of 50) would otherwise be the bound of the edge midpoints' (distances of 1e-9)."""
    s = scene
    out = run(s["q"], s["v"], s["f"])
    check_invariants(out, s["v"], s["f"])
    for name, sl in GROUPS.items():
        bound, worst32 = R.bound(s["q"][sl], s["v"], s["f"], np.sqrt(s["d2"][sl].min(1)))
        assert 0 < worst32 < 1e-5
        print(f"{name}: float32 oracle's worst error {worst32:.3e}")
        check_distances({k: a[sl] for k, a in out.items()}, s["q"][sl], s["v"], s["f"], bound, name, s["d2"][sl])


@pytest.mark.parametrize("Nf", [1, 255, 257, 320])
@pytest.mark.parametrize("Q", [1, 63, 257, 300])
def test_tile_and_slab_tails(scene, Q, Nf):
    """Q around the 64-lane wave and the 256-query tile, Nf around the 128-face chunk (255 = a chunk and a tail, 257 = two and one
    face).  The bound is the float32 oracle's worst error over the whole query set against the cut mesh, not over the Q queries
    alone: a single query's float32 error can be zero by luck, which says nothing about the arithmetic's."""
    s = scene
    g = np.random.default_rng(5)
    q_all = s["q"][:640][g.permutation(640)]  # without the far queries, whose float32 error would be everybody's bound
    f = s["f"][:Nf]
    d2 = R.distance_matrix(q_all, s["v"], f)
    bound, _ = R.bound(q_all, s["v"], f, np.sqrt(d2.min(1)))
    out = run(q_all[:Q], s["v"], f)
    assert all(len(out[k]) == Q for k in out)
    check_invariants(out, s["v"], f)
    check_distances(out, q_all[:Q], s["v"], f, bound, f"Q {Q} Nf {Nf}", d2[:Q])


def test_result_does_not_depend_on_the_slab_count(scene):
    s = scene
    q = s["q"][:300]
    planned = run(q, s["v"], s["f"])
    assert E.mesh_closest_slabs(300, 320) > 1  # the planned launch is itself split
    n = R.face_normals(s["v"], s["f"])[planned["face"]]
    gated = run(q, s["v"], s["f"], normals=n, cos_min=0.3)
    for slabs in (1, 2, 7, 400):
        for ref, kw in ((planned, {}), (gated, dict(normals=n, cos_min=0.3))):
            got = run(q, s["v"], s["f"], slabs=slabs, **kw)
            for k in ref:
                assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (slabs, k)


def test_exact_ties_go_to_the_smallest_face_index(scene):
    s = scene
    v32 = np.float32(s["v"])
    # a face appended twice: its copies 320 and 641 land in other chunks and slabs than the original
    f = np.concatenate([s["f"], s["f"][17:18], s["f"], s["f"][17:18]])
    c = v32[s["f"][17]].astype(np.float64).mean(0)
    q = np.float32([c * 1.5, c * 0.5])
    for slabs in (0, 1, 3, 700):
        out = run(q, v32, f, slabs=slabs)
        assert (out["face"] == 17).all(), slabs
    # a query exactly on a mesh vertex: distance 0 and the smallest incident face
    vid = np.arange(len(v32))
    out = run(v32, v32, s["f"])
    first = np.array([np.nonzero((s["f"] == i).any(1))[0].min() for i in vid])
    assert (out["dist2"] == 0).all() and (out["face"] == first).all()
    assert (out["point"] == v32).all()


def test_normal_and_distance_gates(scene):
    """An outward sphere (r = 0.1) and, nearer to the queries (r = 0.14), an inward one of r = 0.12: with radial query normals and
    cos_min = 0.5 the answer must come from the outward one.  Checked tolerantly on both sides of the gate's rounding."""
    v0, f0 = M.icosphere(2, 0.1)
    v1, f1 = M.icosphere(2, 0.12, inward=True)
    v, f = np.float32(np.concatenate([v0, v1])), np.concatenate([f0, f1 + len(v0)]).astype(np.int32)
    g = np.random.default_rng(9)
    d = g.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    q, cos_min, eps = np.float32(d * 0.14), 0.5, 1e-4
    free = run(q, v, f)
    assert (free["face"] >= len(f0)).all()  # ungated, the inward sphere is nearer
    out = run(q, v, f, normals=d, cos_min=cos_min)
    check_invariants(out, v, f)
    assert (out["face"] >= 0).all() and (out["face"] < len(f0)).all()
    cosines = R.gate_cosines(np.float32(d), v, f)
    assert (cosines[np.arange(len(q)), out["face"]] >= cos_min - eps).all()
    d2 = R.distance_matrix(q, v, f)
    want = np.sqrt(np.where(cosines >= cos_min + eps, d2, np.inf).min(1))
    bound, worst32 = R.bound(q, v, f, np.sqrt(d2.min(1)))
    got = np.sqrt(out["dist2"].astype(np.float64))
    print(f"gate: worst excess over the strict-side minimum {float((got - want).max()):.3e}, bound {bound:.3e}")
    assert (got <= want + bound).all()
    # a zero normal passes every face; a NaN normal passes none
    n2 = np.float32(d).copy()
    n2[0], n2[1] = 0, np.nan
    out2 = run(q, v, f, normals=n2, cos_min=cos_min)
    assert out2["face"][0] == free["face"][0] and out2["face"][1] == -1 and (out2["face"][2:] == out["face"][2:]).all()
    # the distance gate: the queries are 0.02 from the inward sphere and 0.04 from the outward one
    far = run(q, v, f, normals=d, cos_min=cos_min, max_dist2=float(np.float32(0.03 ** 2)))
    check_invariants(far, v, f)
    assert (far["face"] == -1).all() and (far["dist2"] == INF).all()
    near = run(q, v, f, max_dist2=float(np.float32(0.03 ** 2)))
    assert np.array_equal(near["face"], free["face"]) and np.array_equal(near["dist2"], free["dist2"])
    # max_dist2 exactly at a query's dist2 keeps it; the float32 below drops it
    d0 = free["dist2"][0]
    assert run(q[:1], v, f, max_dist2=float(d0))["face"][0] == free["face"][0]
    assert run(q[:1], v, f, max_dist2=float(np.nextafter(d0, np.float32(0))))["face"][0] == -1


def test_bad_faces_and_bad_queries_are_skipped(scene):
    s = scene
    q = s["q"][:300]
    ref = run(q, s["v"], s["f"])
    Nv = len(s["v"])
    # out-of-range indices and a NaN / inf corner in appended faces and vertices: nothing else changes
    v = np.concatenate([np.float32(s["v"]), np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0]])])
    bad = np.int32([[0, 1, Nv + 3], [-1, 2, 3], [2 ** 31 - 1, 0, 1], [0, Nv, 1], [0, Nv + 1, 1], [Nv, Nv, Nv], [-2 ** 31, 5, 6]])
    f = np.concatenate([bad[:3], s["f"], bad[3:]])
    out = run(q, v, f)
    check_invariants(out, v, f)
    assert np.array_equal(out["face"], ref["face"] + 3)
    for k in ("bary", "point", "dist2"):
        assert np.array_equal(out[k], ref[k]), k
    # non-finite queries have no match; their neighbours are untouched
    q2 = np.float32(q).copy()
    q2[3, 1], q2[64, 0], q2[299, 2] = np.nan, np.inf, -np.inf
    out = run(q2, s["v"], s["f"])
    check_invariants(out, s["v"], s["f"])
    hit = np.ones(300, bool)
    hit[[3, 64, 299]] = False
    assert (out["face"][~hit] == -1).all() and np.array_equal(out["face"][hit], ref["face"][hit])
    assert np.array_equal(out["dist2"][hit], ref["dist2"][hit])
    # all faces bad: all -1
    out = run(q, v, bad)
    check_invariants(out, v, bad)
    assert (out["face"] == -1).all()


def test_a_point_cloud_gives_nearest_vertex_distances(scene):
    s = scene
    Nv = len(s["v"])
    f = np.repeat(np.arange(Nv, dtype=np.int32)[:, None], 3, 1)
    out = run(s["q"], s["v"], f)
    check_invariants(out, s["v"], f)
    assert (out["bary"] == np.float32([1, 0, 0])).all() and (out["point"] == np.float32(s["v"])[out["face"]]).all()
    d2 = R.distance_matrix(s["q"], s["v"], f)
    brute = ((np.float32(s["q"]).astype(np.float64)[:, None] - np.float32(s["v"]).astype(np.float64)[None]) ** 2).sum(-1)
    assert np.allclose(d2, brute, rtol=1e-12, atol=0)
    bound, _ = R.bound(s["q"], s["v"], f, np.sqrt(d2.min(1)))
    check_distances(out, s["q"], s["v"], f, bound, "point cloud", d2)
    # zero-area faces that are not points: a segment (i, j, j) answers with a point of itself, never a NaN
    seg = np.int32([[0, 1, 1], [2, 2, 3], [4, 5, 4]])
    out = run(s["q"][:64], s["v"], seg)
    check_invariants(out, s["v"], seg)
    assert (out["face"] >= 0).all()


def test_every_argument_error_returns_before_the_launch():
    lib = L.load()
    buf = torch.zeros(64, device="cuda")
    n = 0
    for fn, cases in abi_error_cases(buf.data_ptr()).items():
        for name, args in cases.items():
            assert getattr(lib, fn)(*args) != 0, (fn, name)
            assert lib.mvd_last_error().decode().startswith(fn + ": "), (fn, name)
            n += 1
    assert n >= 17
    torch.cuda.synchronize()
    assert (buf == 0).all()


# ---- the data term against correspondences
def corr_inputs(F=3, V=300, M=7, seed=2):
    """verts / corr_point [F,V,3], corr_face [F,V] with a third unmatched (and NaN in those corr_points), frame F-1 wholly
    unmatched; vertex weights with zeros; a landmark embedding on a triangle soup."""
    from morphablediffusion_amd.engine import landmark_csr
    g = np.random.default_rng(seed)
    y = np.float32(g.normal(size=(F, V, 3)) * 0.1)
    c = np.float32(y + g.normal(size=(F, V, 3)) * 0.01)
    face = g.integers(0, 1000, (F, V)).astype(np.int32)
    face[g.random((F, V)) < 0.33] = -1
    face[F - 1] = -1
    c[face < 0] = np.nan
    w = np.float32(g.random(V))
    w[::7] = 0
    faces = g.integers(0, V, (2 * V, 3)).astype(np.int32)
    lf, lb = g.integers(0, 2 * V, M).astype(np.int32), g.random((M, 3))
    lb = np.float32(lb / lb.sum(1, keepdims=True))
    lmk = np.einsum("fmck,mc->fmk", y[:, faces[lf]], lb).astype(np.float32)
    tl = np.float32(lmk + g.normal(size=lmk.shape) * 0.01)
    csr = tuple(dev(a) for a in landmark_csr(faces, lf, lb, V)) + (dev(lb),)
    return dict(y=y, c=c, face=face, w=w, faces=faces, lf=lf, lb=lb, lmk=lmk, tl=tl, csr=(csr[0], csr[1], csr[2]))


@pytest.mark.parametrize("landmarks", [False, True])
@pytest.mark.parametrize("weights", [False, True])
def test_fit_data_corr_against_the_oracle(landmarks, weights):
    from tests import morphable_bwd_ref as BR
    i = corr_inputs()
    F, V = i["face"].shape
    kw = dict(vertex_weight=i["w"] if weights else None)
    if landmarks:
        kw.update(lmk=i["lmk"], target_lmk=i["tl"], lmk_lambda=0.5)
    E_, g_y, n = E.op_morph_fit_data_corr(dev(i["y"]), dev(i["c"]), dev(i["face"]), csr=i["csr"] if landmarks else None,
                                          **{k: (dev(a) if isinstance(a, np.ndarray) else a) for k, a in kw.items()})
    E_, g_y, n = E_.cpu().numpy(), g_y.cpu().numpy(), n.cpu().numpy()
    want = {}
    for dt in (np.float64, np.float32):
        o = R.fit_data_corr(i["y"], i["c"], i["face"], dtype=dt, **kw)
        g = o["g_verts"].astype(np.float64)
        if landmarks:
            g = BR.landmarks_bwd(o["g_lmk"].astype(np.float64), i["faces"], i["lf"], i["lb"], V, g_in=g)[0]
        want[dt] = (o["E"].astype(np.float64), g, o["n_matched"])
    assert np.array_equal(n, want[np.float64][2]) and n.dtype == np.int32 and n[F - 1] == 0
    assert np.isfinite(E_).all() and np.isfinite(g_y).all()  # the NaN of an unmatched corr_point does not leak
    for name, got, k in (("E", E_, 0), ("g_y", g_y, 1)):
        err = np.abs(got - want[np.float64][k]).max()
        yard = np.abs(want[np.float32][k] - want[np.float64][k]).max()
        print(f"fit_data_corr {name} (landmarks {landmarks}, weights {weights}): worst error {err:.3e}, float32 oracle {yard:.3e}, "
              f"ratio {err / yard:.2f}")
        assert err <= 4 * yard, name
    # unmatched vertices off the landmark table, and zero-weight ones, get exactly zero gradient
    touched = np.zeros(V, bool)
    if landmarks:
        touched[i["faces"][i["lf"]].reshape(-1)] = True
    zero = (i["face"] < 0) | ((i["w"] == 0)[None] if weights else False)
    assert (g_y[zero & ~touched[None]] == 0).all()
    # a frame with W_f = 0: the vertex term and its gradient are exactly zero
    if not landmarks:
        assert E_[F - 1] == 0 and (g_y[F - 1] == 0).all()


def test_fit_data_corr_repeats_and_frames_stand_alone():
    i = corr_inputs()
    a = E.op_morph_fit_data_corr(dev(i["y"]), dev(i["c"]), dev(i["face"]), vertex_weight=dev(i["w"]))
    b = E.op_morph_fit_data_corr(dev(i["y"]), dev(i["c"]), dev(i["face"]), vertex_weight=dev(i["w"]))
    one = E.op_morph_fit_data_corr(dev(i["y"][1:2]), dev(i["c"][1:2]), dev(i["face"][1:2]), vertex_weight=dev(i["w"]))
    for x, y, z in zip(a, b, one):
        assert torch.equal(x, y) and torch.equal(x[1:2], z)
    # everything matched and unit weights: mvd_op_morph_fit_data against the same points as a target
    face = np.zeros_like(i["face"])
    c = np.nan_to_num(i["c"])
    E1, g1, n1 = E.op_morph_fit_data_corr(dev(i["y"]), dev(c), dev(face))
    E0, g0 = E.op_morph_fit_data(dev(i["y"]), target=dev(c))
    assert (n1 == face.shape[1]).all()
    assert torch.allclose(E1, E0, rtol=1e-6, atol=0) and torch.allclose(g1, g0, rtol=1e-6, atol=0)

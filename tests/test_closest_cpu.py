"""No device: the closest-point oracle (tests/closest_ref.py) against a second derivation, the slab plan of
mvd_mesh_closest_slabs, the argument errors of the C entry points and of the Python wrappers, and the shared inputs of the GPU tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from morphablediffusion_amd import mesh as MS
from tests import closest_ref as R
from tests import mesh_ref as M


def sphere():
    """icosphere(2, 0.1): 162 vertices, 320 faces, as float32 values."""
    v, f = M.icosphere(2, 0.1)
    return np.float32(v), f


def query_set(v, f):
    """680 float32 queries: 60 inside, 100 outside, the 480 edge midpoints, 40 far away."""
    g = np.random.default_rng(21)

    def shell(n, lo, hi):
        d = g.normal(size=(n, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(lo, hi, (n, 1))
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    e = np.unique(e, axis=0)
    mid = 0.5 * (v[e[:, 0]].astype(np.float64) + v[e[:, 1]].astype(np.float64))
    q = np.concatenate([shell(60, 0.0, 0.08), shell(100, 0.1, 0.2), mid, shell(40, 5.0, 50.0)])
    assert q.shape == (680, 3)
    return np.float32(q)


# ---- the oracle
def random_triangles(n, seed):
    g = np.random.default_rng(seed)
    a, b, c = g.normal(size=(3, n, 3))
    q = g.normal(size=(n, 3)) * g.choice([0.3, 1.0, 4.0], size=(n, 1))
    return q, a, b, c


def test_the_seven_regions_agree_with_projection_and_clamped_segments():
    q, a, b, c = random_triangles(20000, 1)
    w, p, d2 = R.on_triangles(q, a, b, c)
    alt = R.on_triangles_alt(q, a, b, c)
    assert np.abs(np.sqrt(d2) - np.sqrt(alt)).max() < 1e-12
    assert (w >= 0).all() and np.abs(w.sum(1) - 1).max() < 1e-14
    assert np.abs(p - (w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c)).max() < 1e-14
    # every region occurs: 3 corners, 3 edges, the interior
    kinds = {tuple(r) for r in (w > 0)}
    assert len(kinds) == 7
    # no point of the triangle is nearer: barycentric samples
    g = np.random.default_rng(2)
    s = g.dirichlet([1, 1, 1], size=(64, len(q)))
    pts = s[..., :1] * a + s[..., 1:2] * b + s[..., 2:] * c
    assert (((pts - q) ** 2).sum(-1) >= d2 - 1e-12).all()


def test_degenerate_faces_answer_with_a_point_of_themselves():
    g = np.random.default_rng(3)
    q, a, b = g.normal(size=(3, 500, 3))
    for tri, alt in (((a, a, a), ((q - a) ** 2).sum(1)), ((a, b, b), R._segment_d2(q, a, b)), ((a, b, a), R._segment_d2(q, a, b)),
                     ((a, a, b), R._segment_d2(q, a, b)), ((a, b, 0.5 * (a + b)), R._segment_d2(q, a, b))):
        for dtype in (np.float64, np.float32):
            w, p, d2 = R.on_triangles(*(x.astype(dtype) for x in (q,) + tri))
            assert np.isfinite(d2).all() and (w >= 0).all() and d2.dtype == dtype
            # a point of the face, so never nearer than the segment; the collinear sliver may miss the nearest point
            assert (d2 >= alt - (1e-9 if dtype is np.float64 else 1e-4)).all()
    w, p, d2 = R.on_triangles(q, a, a, a)
    assert (w == [1, 0, 0]).all() and np.array_equal(p, a)


def test_the_op_oracle_selects_skips_and_gates():
    v, f = sphere()
    q = query_set(v, f)[:200]
    ref = R.closest_point(q, v, f)
    d2 = R.distance_matrix(q, v, f)
    assert np.array_equal(ref["face"], d2.argmin(1)) and np.allclose(ref["dist2"], d2.min(1), rtol=0, atol=0)
    assert np.abs(np.sqrt(R.on_triangles_alt(q[:, None], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None])) - np.sqrt(d2)).max() < 1e-12
    # float32 run: near the float64 one, and the faces disagree only between equally near ones
    r32 = R.closest_point(q, v, f, dtype=np.float32)
    assert r32["dist2"].dtype == np.float32
    assert np.abs(np.sqrt(r32["dist2"].astype(np.float64)) - np.sqrt(ref["dist2"])).max() < 1e-7
    assert np.abs(R.distance_to_faces(q, v, f, r32["face"]) - np.sqrt(ref["dist2"])).max() < 1e-7
    bound, worst = R.bound(q, v, f, np.sqrt(d2.min(1)))
    assert 0 < worst < 1e-7 and bound == 4 * worst
    # a duplicate face loses to the smaller index; bad faces are skipped; the gates give -1
    f2 = np.concatenate([np.int32([[0, 1, 999], [-1, 0, 1]]), f, f[:5]])
    r2 = R.closest_point(q, v, f2)
    assert np.array_equal(r2["face"], ref["face"] + 2) and np.array_equal(r2["dist2"], ref["dist2"])
    far = R.closest_point(q, v, f, max_dist2=1e-12)
    miss = far["face"] < 0
    assert miss.any() and (far["dist2"][miss] == np.inf).all() and (far["bary"][miss] == 0).all() and (far["point"][miss] == 0).all()
    qn = q.copy()
    qn[0] = np.nan
    assert R.closest_point(qn, v, f)["face"][0] == -1
    n = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-9)
    gated = R.closest_point(q, v, f, normals=n, cos_min=0.5)
    cs = R.gate_cosines(n, v, f)
    assert (cs[np.arange(len(q)), gated["face"]] >= 0.5 - 1e-9).all()
    assert (R.closest_point(q, v, f, normals=-n, cos_min=0.5)["face"] != gated["face"]).any()


def test_subdivision_keeps_the_surface():
    v, f = sphere()
    v2, f2 = R.subdivide(v, f)
    assert v2.shape == (642, 3) and f2.shape == (1280, 3)
    q = query_set(v, f)[::7]
    assert np.abs(np.sqrt(R.distance_matrix(q, v2, f2).min(1)) - np.sqrt(R.distance_matrix(q, v, f).min(1))).max() < 1e-9


def test_statistics_match_the_package():
    g = np.random.default_rng(4)
    d = np.abs(g.normal(size=1001))
    d[::50] = np.inf
    want, got = R.statistics(d), MS.distance_statistics(torch.from_numpy(d))
    assert set(want) == set(got)
    for k in want:
        assert abs(want[k] - got[k]) <= 1e-12 * max(1.0, abs(want[k])), k
    none = MS.distance_statistics(torch.full((3,), float("inf")))
    assert none["matched"] == 0.0 and np.isnan(none["rms"])


# ---- the slab plan
def test_the_slab_plan_is_a_host_function_of_q_and_nf():
    lib = L.load()
    assert "mvd_mesh_closest_slabs" in L.PROTOTYPES and len(L.PROTOTYPES["mvd_op_mesh_closest_point"][1]) == 16
    plan = lambda Q, Nf: lib.mvd_mesh_closest_slabs(Q, Nf)
    for Q in (1, 63, 256, 257, 5023, 10475, 250000, 262144, 10 ** 7):
        for Nf in (1, 127, 128, 129, 320, 9976, 100000, 500000):
            n = plan(Q, Nf)
            tiles, chunks = -(-Q // 256), -(-Nf // 128)
            assert n >= 1 and n == plan(Q, Nf) == E.mesh_closest_slabs(Q, Nf)
            assert n <= chunks  # a slab is never cut below one chunk of faces
            if tiles >= 1024:
                assert n == 1  # the query tiles fill the chip (256 CUs x 4 SIMDs) by themselves
            else:
                assert n == min(chunks, -(-1024 // tiles))
    assert plan(5023, 100000) == 52 and plan(5023, 100000) * 20 >= 1024  # 20 tiles alone would leave 236 of 256 CUs idle
    assert plan(0, 5) == 1 and plan(5, 0) == 1 and plan(-3, -3) == 1


# ---- the C ABI
def abi_error_cases(p):
    """{entry point: {case: arguments with one argument error}}; p: any non-null address (never read)."""
    inf, nan = float("inf"), float("nan")
    ok = dict(queries=p, query_normals=None, verts=p, faces=p, Q=1, Nv=1, Nf=1, cos_min=0.0, max_dist2=inf, slabs=0, key=p, face=p, bary=p,
              point=p, dist2=p, stream=None)
    cases = dict({f"null {k}": {k: None} for k in ("queries", "verts", "faces", "key", "face", "bary", "point", "dist2")},
                 **{"Q < 1": dict(Q=0), "Nv < 1": dict(Nv=0), "Nf < 1": dict(Nf=-1), "3 Q >= 2^31": dict(Q=0x2aaaaaab),
                    "3 Nv >= 2^31": dict(Nv=0x2aaaaaab), "3 Nf >= 2^31": dict(Nf=0x2aaaaaab), "max_dist2 0": dict(max_dist2=0.0),
                    "max_dist2 < 0": dict(max_dist2=-1.0), "max_dist2 nan": dict(max_dist2=nan), "cos_min > 1": dict(cos_min=1.5),
                    "cos_min < -1": dict(cos_min=-1.0001), "cos_min nan": dict(cos_min=nan), "slabs < 0": dict(slabs=-1),
                    "normals with a bad count": dict(query_normals=p, Q=0)})
    bad = {"mvd_op_mesh_closest_point": (ok, cases)}
    return {fn: {k: tuple(dict(ok, **v).values()) for k, v in cases.items()} for fn, (ok, cases) in bad.items()}


def test_c_abi_argument_errors_need_no_device():
    """Every argument error returns before the first HIP call, so this holds on a machine without a GPU."""
    lib = L.load()
    buf = (C.c_double * 8)()
    n = 0
    for fn, cases in abi_error_cases(C.addressof(buf)).items():
        assert hasattr(lib, fn)
        for name, args in cases.items():
            assert getattr(lib, fn)(*args) != 0, (fn, name)
            assert lib.mvd_last_error().decode().startswith(fn + ": "), (fn, name)
            n += 1
    assert n == 22


# ---- the wrappers
def test_wrappers_raise_before_anything_is_copied():
    v, f = sphere()
    q = torch.from_numpy(query_set(v, f)[:5])
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    op = E.op_mesh_closest_point
    for args, kw in (((q[:, :2], vt, ft), {}), ((q, vt[:0], ft), {}), ((q, vt, ft.long()), {}), ((q, vt, ft[:, :2]), {}),
                     ((q, vt, ft[:0]), {}), ((q.int(), vt, ft), {}), ((q.numpy(), vt, ft), {}),
                     ((q, vt, ft), dict(query_normals=q[:3])), ((q, vt, ft), dict(query_normals=q.int())),
                     ((q, vt, ft), dict(max_dist2=0.0)), ((q, vt, ft), dict(max_dist2=float("nan"))), ((q, vt, ft), dict(cos_min=2.0)),
                     ((q, vt, ft), dict(cos_min=float("nan"))), ((q, vt, ft), dict(slabs=-1))):
        with pytest.raises(ValueError, match="op_mesh_closest_point"):
            op(*args, **kw)
    for fn in (MS.closest_point, MS.surface_distance):
        for args, kw in (((q[:, :2], v, f), {}), ((q, v[:, :2], f), {}), ((q, v, f[:, :2]), {}), ((q, v, f), dict(cos_min=0.5)),
                         ((q, v, f), dict(normals=q[:2])), ((q, v, f), dict(normals=q, cos_min=1.5)), ((q, v, f), dict(max_dist=0.0)),
                         ((q, v, f), dict(max_dist=-1.0))):
            with pytest.raises(ValueError):
                fn(*args, **kw)


# ---- fitting to a scan
def test_the_float64_loop_meets_the_convergence_condition_on_the_gpu_tests_inputs():
    """The GPU test asks fit_scan for a surface RMS of at most 1e-2 of its start; that is only a fair question on inputs for which
    the float64 loop alone reaches 1e-3.  Also checks tests/golden/fit_scan_trajectory.npz, which the GPU tests read instead of
    running this loop, against the loop (tools/make_fit_scan_golden.py wrote it)."""
    import os
    m, p_true, scans = R.scan_case()
    assert scans[0][0].shape == (642, 3) and scans[0][1].shape == (1280, 3) and scans[0][0].dtype == np.float32
    o = R.icp_oracle(m, scans, iters=300, lr=0.05, keep=(20, 100))
    first, last = R.surface_rms(m, np.zeros_like(p_true), scans), R.surface_rms(m, o["p"], scans)
    print(f"float64 ICP from zero: surface RMS {first} -> {last}, ratio {last / first}")
    assert (last <= 1e-3 * first).all() and (o["matched_history"] == 162).all()
    assert R.surface_rms(m, p_true, scans)[0] < 1e-7  # the scan is the posed surface (as float32 stores it)
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_scan_trajectory.npz"))
    for k, want in ((20, gold["p20"]), (100, gold["p100"])):
        assert np.abs(o["snapshots"][k] - want).max() <= 1e-9, k
    assert np.abs(o["p"] - gold["p300"]).max() <= 1e-8 and np.allclose(o["loss_history"][:20], gold["loss20"], rtol=1e-9, atol=0)
    assert np.allclose(first, gold["rms_first"], rtol=1e-9) and 0 < gold["yard20"] < 1e-4 and 0 < gold["yard100"] < 1e-4


def test_icp_pieces():
    m, p_true, scans = R.scan_case(F=2)
    assert len(scans) == 2 and p_true.shape == (2, 28)
    # at the truth the correspondences are the vertices themselves and the gradient vanishes
    from tests import morphable_bwd_ref as BR
    fm = BR.Folded(m)
    y = BR.forward(fm, p_true[:, :10], p_true[:, 10:25], p_true[:, 25:])["vertices"]
    cp, cf = R.correspondences(y, scans)
    assert (cf >= 0).all() and np.abs(cp - y).max() < 1e-8
    d = R.fit_data_corr(y, cp, cf)
    assert d["E"].max() < 1e-15 and (d["n_matched"] == 162).all()
    # the distance gate drops vertices, and the normaliser follows
    cp2, cf2 = R.correspondences(y + 0.05, scans, max_dist2=0.06 ** 2)
    d2 = R.fit_data_corr(y + 0.05, cp2, cf2)
    assert (0 < d2["n_matched"]).all() and (d2["n_matched"] < 162).all() and (d2["g_verts"][cf2 < 0] == 0).all()
    r = np.where((cf2 >= 0)[..., None], y + 0.05 - cp2, 0)
    assert np.allclose(d2["E"], (r * r).sum(-1).sum(1) / d2["n_matched"])


def test_fit_scan_flag_rules(capsys):
    from morphablediffusion_amd import generate_face as GF
    base = ["--input_img", "a.png", "--exp_img", "b.png", "--output_dir", "out"]
    ok = GF.parse_args(base + ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--fit_scan_max_dist", "0.01", "--fit_scan_normal_cos", "0.5",
                               "--fit_scan_refresh", "5", "--fit_scan_landmarks", "l.npz"])
    assert ok.fit_scan == "s.ply" and ok.fit_scan_max_dist == 0.01 and ok.fit_scan_refresh == 5 and ok.fit_mesh is None
    two = GF.parse_args(base + ["--flame_model", "m.npz", "--fit_scan", "s.obj", "--flame_params", "p.npz", "--frames", "2"])
    assert two.frames == 2
    for bad in (["--fit_scan", "s.ply"],  # needs --flame_model
                ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--fit_mesh", "t.ply"],
                ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--mesh", "t.ply"],
                ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--neutral_params", "n.npz"],
                ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--frames", "2"],
                ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--fit_scan_refresh", "0"],
                ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--fit_scan_max_dist", "0"],
                ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--fit_scan_normal_cos", "1.5"],
                ["--flame_model", "m.npz", "--fit_scan", "s.ply", "--fit_iters", "0"],
                ["--flame_model", "m.npz", "--fit_mesh", "t.ply", "--fit_scan_max_dist", "0.1"],
                ["--mesh", "t.ply", "--fit_scan_refresh", "2"]):
        with pytest.raises(SystemExit):
            GF.parse_args(base + bad)
    capsys.readouterr()


def test_fit_scan_wrappers_raise_before_anything_is_copied():
    from morphablediffusion_amd import morphable as MM
    m, _, scans = R.scan_case(M=4)
    fm = MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"],
                                       faces=m["faces"], lmk_face=m["lmk_face"], lmk_bary=m["lmk_bary"], device="cpu")
    sv, sf = scans[0]
    for kw in (dict(scan_vertices=sv[:, :2]), dict(scan_vertices=sv, scan_faces=sf[:, :2]), dict(scan_vertices=sv, scan_faces=np.float32(sf)),
               dict(scan_vertices=[sv, sv], scan_faces=sf), dict(scan_vertices=[]), dict(scan_vertices=sv, refresh=0),
               dict(scan_vertices=sv, iters=0), dict(scan_vertices=sv, max_dist=0.0), dict(scan_vertices=sv, normal_cos=1.5),
               dict(scan_vertices=sv, target_landmarks=np.zeros((1, 5, 3))), dict(scan_vertices=[sv, sv, sv], frames=2),
               dict(scan_vertices=sv, free=("nothing",)), dict(scan_vertices=sv, lr=0.0),
               dict(scan_vertices=sv, scan_faces=sf)):  # a valid call: the fitter runs on the GPU only
        with pytest.raises(ValueError, match="MorphableModel.fit_scan"):
            fm.fit_scan(**kw)
    with pytest.raises(ValueError, match="fit_flame_scan"):
        fm.fit_flame_scan(sv, sf, free=("tongue",))
    # the engine's entries: nothing here is a device tensor, so every one of these stops at its checks
    y = torch.zeros(2, 162, 3)
    face = torch.zeros(2, 162, dtype=torch.int32)
    for args, kw in (((y[0], y, face), {}), ((y, y[:1], face), {}), ((y, y, face.long()), {}), ((y, y, face[:, :5]), {}),
                     ((y, y, face), dict(vertex_weight=torch.ones(5))), ((y, y, face), dict(vertex_weight=-torch.ones(162))),
                     ((y, y, face), dict(lmk_weight=torch.ones(4))), ((y, y, face), dict(target_lmk=torch.zeros(2, 4, 3)))):
        with pytest.raises(ValueError, match="op_morph_fit_data_corr"):
            E.op_morph_fit_data_corr(*args, **kw)
    with pytest.raises(ValueError, match="morph_fit_scan_run"):
        E.morph_fit_scan_run(fm, torch.zeros(1, 28), torch.zeros(1, 28), torch.zeros(1, 28), torch.zeros(28), torch.zeros(28), torch.zeros(28),
                             5, [(torch.from_numpy(sv), torch.from_numpy(sf))])  # p is not a device tensor
    for scans_bad in ([], [(torch.from_numpy(sv),)], [(torch.from_numpy(sv), torch.from_numpy(sf).long())],
                      [(torch.from_numpy(sv), torch.from_numpy(sf)[:0])], [(torch.from_numpy(sv), torch.from_numpy(sf))] * 3):
        with pytest.raises(ValueError, match="scans"):
            E.scan_args("scans", scans_bad, 2)
    assert E.scan_args("scans", [(torch.from_numpy(sv), torch.from_numpy(sf))] * 2, 2) == ([0, 642, 1284], [0, 1280, 2560])

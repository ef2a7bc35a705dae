"""CPU: the mesh texturing oracle (tests/mesh_ref.py) checked against itself -- watertight fill rule, int64 against unbounded
integers at the guard-band extreme, the tie rule -- the mesh file readers and writer of morphablediffusion_amd/mesh.py, and the
argument errors of the three entry points (which return before the first HIP call)."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from morphablediffusion_amd import lib as L
from morphablediffusion_amd import mesh as MS
from morphablediffusion_amd.generate_face import read_mesh_vertices
from tests import mesh_ref as R


def ortho_points(p, scale, off, z=2.0):
    """xy / key [1,Nv,...] of points drawn orthographically at one depth: integer inputs made without the projection."""
    xy = np.rint((np.asarray(p)[:, :2] * scale + off) * R.ONE).astype(np.int32)[None]
    key = np.full((1, len(p)), 1000, dtype=np.int32)
    return xy, key


def test_closed_sphere_covers_interior_pixels_twice_and_a_quad_once():
    """The fill rule is watertight: no pixel of a shared edge or vertex is drawn by both neighbours or by neither."""
    v, f = R.icosphere(1)
    xy, key = ortho_points(v, 10.0, (16.0, 12.0))  # vertices on the 1/16 grid, many edges through pixel centres
    cnt = R.coverage_count(xy, key, f, 24, 32)
    jj, ii = np.meshgrid(np.arange(32), np.arange(24))
    r = np.hypot(jj - 16.0, ii - 12.0)
    assert (cnt[0][r < 9.0] == 2).all()  # inside the inscribed circle of the 80-face silhouette (10 cos 18 deg > 9)
    assert (cnt[0][r > 10.0] == 0).all() and set(np.unique(cnt)) <= {0, 2}
    quad = np.array([[2, 3], [29, 3], [29, 20], [2, 20]]) * R.ONE  # corners and edges exactly on pixel centres
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]], [[2, 1, 0], [0, 2, 3]]):
        cnt = R.coverage_count(quad[None].astype(np.int32), np.full((1, 4), 7, np.int32), np.array(faces, np.int32), 24, 32)
        assert set(np.unique(cnt)) == {0, 1}
        # top-left rule: of the 28 x 18 pixel centres on or inside the outline, one row and one column are not owned
        assert cnt.sum() == 27 * 17


def test_int64_raster_equals_unbounded_integers_at_the_guard_band():
    g = np.random.default_rng(3)
    H, W = 9, 11
    for trial in range(40):
        xy = g.integers(-R.GUARD, R.GUARD + 1, size=(1, 3, 2)).astype(np.int32)
        if trial % 4 == 0:  # the extreme itself: corners of the guard band, the largest keys
            xy = (np.array([[[-1, -1], [1, -1], [0, 1]]]) * R.GUARD).astype(np.int32)[:, g.permutation(3)]
        key = g.integers(1, R.KMAX + 1, size=(1, 3)).astype(np.int32)
        if trial % 4 == 1:
            key[:] = R.KMAX
        faces = np.array([[0, 1, 2]], np.int32)
        a, b = R.raster(xy, key, faces, H, W), R.raster(xy, key, faces, H, W, bigint=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), trial


def test_tie_goes_to_the_smaller_face_index_and_larger_key_wins():
    xy = (np.array([[[1, 1], [9, 1], [1, 9], [9, 9]]]) * R.ONE).astype(np.int32)
    key = np.full((1, 4), 500, np.int32)
    for order in ([[0, 1, 2], [2, 1, 0], [0, 1, 2]], [[2, 1, 0], [0, 1, 2]]):
        fid, pk, bad = R.raster(xy, key, np.array(order, np.int32), 12, 12)
        assert bad == 0 and set(np.unique(fid)) == {-1, 0} and (pk[fid == 0] == 500).all()
    xy2 = np.concatenate([xy, xy], 1)
    key2 = np.concatenate([key, key + 1], 1)
    fid, pk, _ = R.raster(xy2, key2, np.array([[0, 1, 2], [4, 5, 6]], np.int32), 12, 12)
    assert set(np.unique(fid)) == {-1, 1} and (pk[fid == 1] == 501).all()


def test_oracle_skips_invalid_degenerate_and_out_of_range_faces():
    xy = (np.array([[[1, 1], [9, 1], [1, 9], [5, 5], [9, 9]]]) * R.ONE).astype(np.int32)
    key = np.array([[5, 5, 5, 0, 5]], np.int32)
    faces = np.array([[0, 1, 3], [0, 1, 7], [0, 4, 4], [-1, 0, 1], [0, 1, 2]], np.int32)
    fid, pk, bad = R.raster(xy, key, faces, 12, 12)
    assert bad == 2 and set(np.unique(fid)) == {-1, 4}


# ---- mesh files
QUAD_V = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [1.0, 1.0, 0.25], [0.0, 1.0, -0.125], [0.5, 0.5, 1.0]]
QUAD_TRIS = [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4]]  # a quad (fan) and three triangles


def test_read_mesh_obj_index_forms_quads_and_negative_indices(tmp_path):
    p = tmp_path / "m.obj"
    lines = ["# comment", "vt 0 0", "vn 0 0 1"] + [f"v {a} {b} {c}" for a, b, c in QUAD_V]
    lines += ["f 1 2 3 4", "f 1/1 2/1 5/1", "f 2//1 3//1 5//1", "f -3/1/1 -2/1/1 -1/1/1"]
    p.write_text("\n".join(lines) + "\n")
    v, f = MS.read_mesh(p)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert np.array_equal(v, np.array(QUAD_V)) and f.tolist() == QUAD_TRIS
    assert np.array_equal(read_mesh_vertices(p), v)


def _ply_bytes(fmt, index_name):
    end = {"binary_little_endian": "<", "binary_big_endian": ">"}.get(fmt)
    polys = [[0, 1, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4]]
    head = ["ply", f"format {fmt} 1.0", "comment made by a test", f"element vertex {len(QUAD_V)}", "property float x",
            "property uchar red", "property double y", "property float z", f"element face {len(polys)}",
            "property uchar flag", f"property list uchar int {index_name}", "end_header"]
    out = ("\n".join(head) + "\n").encode()
    if end is None:
        body = [f"{a} 7 {b} {c}" for a, b, c in QUAD_V] + ["1 " + " ".join(str(i) for i in [len(q)] + q) for q in polys]
        return out + ("\n".join(body) + "\n").encode()
    for a, b, c in QUAD_V:
        out += struct.pack(end + "fBdf", a, 7, b, c)
    for q in polys:
        out += struct.pack(end + "BB" + "i" * len(q), 1, len(q), *q)
    return out


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_read_mesh_ply_formats(tmp_path, fmt):
    for name in ("vertex_indices", "vertex_index"):
        p = tmp_path / f"{name}.ply"
        p.write_bytes(_ply_bytes(fmt, name))
        v, f = MS.read_mesh(p)
        assert np.array_equal(v, np.array(QUAD_V)) and f.tolist() == QUAD_TRIS and f.dtype == np.int32
        assert np.array_equal(read_mesh_vertices(p), v)


def test_read_mesh_rejects_what_it_cannot_read(tmp_path):
    p = tmp_path / "bad.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 9\n")
    with pytest.raises(ValueError, match="outside"):
        MS.read_mesh(p)
    with pytest.raises(ValueError, match="expected"):
        MS.read_mesh(tmp_path / "m.stl")
    q = tmp_path / "nofaces.ply"
    q.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                  b"element face 1\nproperty uchar flag\nend_header\n0 0 0\n1\n")
    with pytest.raises(ValueError, match="vertex_indices"):
        MS.read_mesh(q)


def test_write_ply_round_trip(tmp_path):
    v, f = R.icosphere(1)
    g = np.random.default_rng(0)
    c = g.random((len(v), 3))
    c[0], c[1] = (0.0, 1.0, 0.5), (np.nan, 2.0, -1.0)  # 0.5 * 255 = 127.5 rounds to even; out of range is clamped
    p = tmp_path / "out.ply"
    MS.write_ply(p, v, f, torch.from_numpy(c))
    v2, f2 = MS.read_mesh(p)
    assert np.array_equal(v2, v) and np.array_equal(f2, f)  # float64 vertices are stored as doubles
    raw = p.read_bytes()
    body = raw[raw.index(b"end_header\n") + 11:]
    rec = np.frombuffer(body[:len(v) * 27], dtype=[("p", "<f8", (3,)), ("c", "u1", (3,))])
    want = np.rint(np.clip(np.nan_to_num(c), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(rec["c"], want) and rec["c"][0].tolist() == [0, 255, 128] and rec["c"][1].tolist() == [0, 255, 0]
    MS.write_ply(p, v.astype(np.float32), f)  # no colours, float vertices
    v3, f3 = MS.read_mesh(p)
    assert np.array_equal(v3, v.astype(np.float32).astype(np.float64)) and np.array_equal(f3, f)


def test_vertex_normals_on_a_sphere():
    v, f = R.icosphere(2, 0.7, (0.1, -0.2, 0.3))
    n = MS.vertex_normals(v, f)
    want = (v - np.array([0.1, -0.2, 0.3])) / 0.7
    assert n.dtype == np.float64 and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12
    assert (n * want).sum(1).min() > 0.999  # outward, within the faceting of 320 faces
    assert np.allclose(MS.vertex_normals(v, f[:, [0, 2, 1]]), -n)
    assert np.allclose(n, R.vertex_normals(v, f))
    lone = MS.vertex_normals(np.concatenate([v, [[9.0, 9.0, 9.0]]]), f)
    assert (lone[-1] == 0).all()


def test_default_z_near_and_python_argument_checks_precede_any_launch():
    from morphablediffusion_amd import engine as E
    from morphablediffusion_amd.batch import virtual_cameras
    K, RT = virtual_cameras(3, 32)
    v, f = R.icosphere(0, 0.3)
    z = MS.default_z_near(v, RT)
    assert abs(z - 0.5 * R.project(v, K[:, :3, :3], RT, 1e-3)["Z"].min()) < 1e-12
    with pytest.raises(ValueError, match="behind"):
        MS.default_z_near(v * 40, RT)
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(ValueError):
        E.op_mesh_project(vt[:, :2], K[:, :3, :3], RT, 1.0)
    with pytest.raises(ValueError):
        E.op_mesh_project(vt, K, RT, 1.0)  # K is [N,4,4] here
    with pytest.raises(ValueError):
        E.op_mesh_project(vt, K[:, :3, :3], RT, 0.0)
    xy, key = torch.zeros(3, 12, 2, dtype=torch.int32), torch.zeros(3, 12, dtype=torch.int32)
    with pytest.raises(ValueError):
        E.op_mesh_raster(xy.long(), key, ft, 8, 8)
    with pytest.raises(ValueError):
        E.op_mesh_raster(xy, key[:, :5], ft, 8, 8)
    with pytest.raises(ValueError):
        E.op_mesh_raster(xy, key, ft, 8, 4097)
    with pytest.raises(ValueError):
        E.op_mesh_raster(xy, key, ft, 0, 8)
    fid = torch.zeros(3, 8, 8, dtype=torch.int32)
    img = torch.zeros(3, 3, 8, 8)
    nrm, cen = torch.zeros(12, 3), torch.zeros(3, 3)
    with pytest.raises(ValueError):
        E.op_mesh_vertex_colors(img.long(), xy, key, ft, fid, fid, vt, nrm, cen)
    with pytest.raises(ValueError):
        E.op_mesh_vertex_colors(img, xy, key, ft, fid[:, :7], fid, vt, nrm, cen)
    with pytest.raises(ValueError):
        E.op_mesh_vertex_colors(img, xy, key, ft, fid, fid, vt, nrm, cen, power=0.5)
    with pytest.raises(ValueError):
        E.op_mesh_vertex_colors(img, xy, key, ft, fid, fid, vt, nrm[:5], cen)
    with pytest.raises(ValueError):
        MS.texture_mesh(img, vt, ft, K[:2], RT[:2])


# ---- the C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    lib = L.load()
    for name, nargs in (("mvd_op_mesh_project", 9), ("mvd_op_mesh_raster", 12), ("mvd_op_mesh_vertex_colors", 28)):
        assert name in L.PROTOTYPES and len(L.PROTOTYPES[name][1]) == nargs
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs


def abi_error_cases(p):
    """{entry point: {case: arguments with one argument error}}; p: any non-null address (never read)."""
    inf, nan = float("inf"), float("nan")
    proj = dict(verts=p, K=p, RT=p, N=1, Nv=1, z_near=1.0, xy=p, key=p, stream=None)
    rast = dict(xy=p, key=p, faces=p, N=1, Nv=1, Nf=1, H=4, W=4, face_id=p, pix_key=p, bad=p, stream=None)
    colr = dict(images=p, dtype=0, layout=0, xy=p, key=p, faces=p, face_id=p, pix_key=p, verts=p, normals=p, centres=p, N=1, Nv=1,
                Nf=1, H=4, W=4, power=2.0, bias=4096, two_sided=0, fr=0.5, fg=0.5, fb=0.5, color=p, weight_sum=p, n_seen=p, spread=p,
                visible=None, stream=None)
    image = {"H < 1": dict(H=0), "W < 1": dict(W=0), "H > 4096": dict(H=4097), "W > 4096": dict(W=4097),
             "N H W >= 2^31": dict(N=128, H=4096, W=4096), "N < 1": dict(N=0), "Nv < 1": dict(Nv=0), "Nf < 1": dict(Nf=0)}
    bad = {"mvd_op_mesh_project": (proj, dict({f"null {k}": {k: None} for k in ("verts", "K", "RT", "xy", "key")},
                                              **{"N < 1": dict(N=0), "Nv < 1": dict(Nv=0), "z_near 0": dict(z_near=0.0),
                                                 "z_near < 0": dict(z_near=-1.0), "z_near inf": dict(z_near=inf),
                                                 "z_near nan": dict(z_near=nan)})),
           "mvd_op_mesh_raster": (rast, dict({f"null {k}": {k: None} for k in ("xy", "key", "faces", "face_id", "pix_key", "bad")},
                                             **image)),
           "mvd_op_mesh_vertex_colors": (colr, dict({f"null {k}": {k: None} for k in
                                                     ("images", "xy", "key", "faces", "face_id", "pix_key", "verts", "normals",
                                                      "centres", "color", "weight_sum", "n_seen", "spread")},
                                                    **image, **{"power < 1": dict(power=0.99), "power nan": dict(power=nan),
                                                                "dtype": dict(dtype=2), "dtype < 0": dict(dtype=-1),
                                                                "layout": dict(layout=2), "layout < 0": dict(layout=-1)}))}
    return {fn: {k: tuple(dict(ok, **v).values()) for k, v in cases.items()} for fn, (ok, cases) in bad.items()}


def test_c_abi_argument_errors_need_no_device():
    """Every argument error returns before the first HIP call, so this holds on a machine without a GPU."""
    lib = L.load()
    buf = (C.c_double * 8)()
    n = 0
    for fn, cases in abi_error_cases(C.addressof(buf)).items():
        for name, args in cases.items():
            assert getattr(lib, fn)(*args) != 0, (fn, name)
            assert lib.mvd_last_error().decode().startswith(fn + ": "), (fn, name)
            n += 1
    assert n == 11 + 14 + 27

"""CPU: the UV atlas oracle (tests/mesh_uv_ref.py) checked against itself, mesh.triangle_atlas, the textured-OBJ reader and writer
of morphablediffusion_amd/mesh.py, and the argument errors of the four entry points (which return before the first HIP call)."""
import ctypes as C

import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from morphablediffusion_amd import mesh as MS
from tests import mesh_ref as R
from tests import mesh_uv_ref as U


def texels(*pts):
    """Chart coordinates in 1/16 texel of points given in texel indices (texel (i, j) has its centre at (x, y) = (j, i))."""
    return np.rint(np.asarray(pts, dtype=np.float64) * R.ONE).astype(np.int32)


# ---- the oracle against itself
def test_barycentrics_sum_to_one_and_reproduce_a_corner_on_a_texel_centre():
    uv_xy = texels((4, 4), (12.5, 2.25), (5.75, 13))
    tf = U.tex_face(uv_xy, [[0, 1, 2]], 16, 16)
    assert tf[4, 4] == 0 and (tf >= 0).sum() > 30  # the corner on a texel centre is owned (top-left rule)
    b = U.texel_barycentrics(uv_xy, np.array([[0, 1, 2]]), tf)
    own = tf >= 0
    assert np.abs(b[own].sum(-1) - 1).max() <= 4 * 2.0 ** -53 and (b[own] >= 0).all() and np.isnan(b[~own]).all()
    assert b[4, 4].tolist() == [1.0, 0.0, 0.0]
    attr = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 8.0], [0.25, -7.0, 1.5]])
    pts = U.texel_points(b, tf, np.array([[0, 1, 2]]), attr)
    assert pts[4, 4].tolist() == attr[0].tolist()
    # the texel coordinates themselves are an affine attribute: interpolating the chart corners gives the texel centre back
    ij = U.texel_points(b, tf, np.array([[0, 1, 2]]), uv_xy / 16.0)
    ii, jj = np.nonzero(own)
    assert np.abs(ij[own] - np.stack([jj, ii], -1)).max() <= 1e-12


def test_a_mirrored_chart_gives_the_points_of_its_twin():
    tri = texels((2.25, 1.5), (13.5, 3.25), (5.75, 12.5))
    mirrored = tri.copy()
    mirrored[:, 0] = 16 * R.ONE - tri[:, 0]  # x -> 16 - x: texel centres go to texel centres, the orientation flips
    attr = np.random.default_rng(0).normal(size=(3, 3))
    face = np.array([[0, 1, 2]])
    ta, tb = U.tex_face(tri, face, 16, 17), U.tex_face(mirrored, face, 16, 17)
    pa = U.texel_points(U.texel_barycentrics(tri, face, ta), ta, face, attr)
    pb = U.texel_points(U.texel_barycentrics(mirrored, face, tb), tb, face, attr)[:, ::-1]  # texel j of the twin is texel 16 - j
    both = (ta >= 0) & (tb[:, ::-1] >= 0)
    assert both.sum() > 40 and np.array_equal(pa[both], pb[both])
    # the barycentrics belong to the corners as stored: renaming the corners permutes them
    perm = np.array([[2, 0, 1]])
    bp = U.texel_barycentrics(tri, perm, U.tex_face(tri, perm, 16, 17))
    assert np.array_equal(bp[both][:, [1, 2, 0]], U.texel_barycentrics(tri, face, ta)[both])


def test_perspective_barycentrics_equal_float64_interpolation_of_inverse_depth():
    """A quad seen obliquely: g_k = e_k key_k over their sum against e_k / Z_k over their sum.  The keys are z_near / Z KMAX rounded
    to integers, a relative error of at most 0.5 / key each, which moves a barycentric by at most twice that."""
    s = oblique_quad()
    b = U.render_barycentrics(s["xy"], s["key"], s["face_id"], s["faces"])
    bz = U.render_barycentrics(s["xy"], s["key"], s["face_id"], s["faces"], depth=s["proj"]["Z"])
    affine = U.render_barycentrics(s["xy"], s["key"], s["face_id"], s["faces"], perspective=False)
    m = s["face_id"] >= 0
    assert m.sum() > 300 and np.abs(b[m].sum(-1) - 1).max() <= 1e-15
    tol = 2 * 0.5 / s["key"].min() + 1e-15
    assert np.abs(b[m] - bz[m]).max() <= tol
    assert np.abs(affine[m] - bz[m]).max() > 100 * tol  # the affine form is another function


def oblique_quad(H=40, W=44):
    """A 1.2 x 1.2 quad through the origin turned 70 degrees about y, in the first camera of the ring: its far edge is 1.25 times
    as far as its near one."""
    K, RT = R.ring_cameras(1, H, W)
    K, RT = K[:1], RT[:1]
    c, sn = np.cos(np.radians(70.0)), np.sin(np.radians(70.0))
    Rw = RT[0, :, :3].astype(np.float64).T  # camera axes in the world: the quad is laid out in the camera's frame
    corners = np.array([[-0.6, -0.6], [0.6, -0.6], [0.6, 0.6], [-0.6, 0.6]])
    cam = np.stack([corners[:, 0] * c, corners[:, 1], corners[:, 0] * sn], -1)
    verts = (cam @ Rw.T).astype(np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    P = R.project(verts, K, RT, 2.0)
    face_id, pix_key, bad = R.raster(P["xy"], P["key"], faces, H, W)
    assert bad == 0 and P["Z"].max() / P["Z"].min() > 1.2
    uv = np.array([[0.05, 0.05], [0.95, 0.05], [0.95, 0.95], [0.05, 0.95]])
    return dict(H=H, W=W, K=K, RT=RT, verts=verts, faces=faces, proj=P, xy=P["xy"], key=P["key"], face_id=face_id, pix_key=pix_key, uv=uv,
                face_uv=faces.copy())


def test_dilation_oracle_grows_one_texel_as_a_square():
    tex, val = np.zeros((7, 9, 3)), np.zeros((7, 9), bool)
    tex[3, 4], val[3, 4] = (0.25, 0.5, 1.0), True
    for p in range(4):
        t, v = U.dilate(tex, val, p)
        want = np.zeros((7, 9), bool)
        want[max(3 - p, 0):3 + p + 1, max(4 - p, 0):4 + p + 1] = True
        assert np.array_equal(v, want) and np.array_equal(t[v], np.broadcast_to([0.25, 0.5, 1.0], (v.sum(), 3)))


# ---- triangle_atlas
@pytest.mark.parametrize("n_faces,Ht,Wt,gutter", [(100, 48, 64, 1), (100, 40, 40, 1), (7, 24, 31, 2), (1, 4, 4, 1), (20, 30, 30, 0)])
def test_triangle_atlas_charts_are_disjoint_complete_and_a_gutter_apart(n_faces, Ht, Wt, gutter):
    uv, face_uv = MS.triangle_atlas(n_faces, Ht, Wt, gutter)
    assert uv.dtype == np.float64 and face_uv.dtype == np.int32 and face_uv.shape == (n_faces, 3) and uv.min() >= 0 and uv.max() <= 1
    uv2, face_uv2 = MS.triangle_atlas(n_faces, Ht, Wt, gutter)
    assert np.array_equal(uv, uv2) and np.array_equal(face_uv, face_uv2)  # deterministic
    uv_xy = MS.uv_to_atlas(uv, Ht, Wt)
    assert np.array_equal(uv_xy, U.uv_to_atlas(uv, Ht, Wt))
    assert np.array_equal(uv_xy % 4, np.zeros_like(uv_xy))  # the corners sit on quarter texels: exact on the 1/16 grid
    cnt = R.coverage_count(uv_xy[None], np.ones((1, len(uv_xy)), np.int32), face_uv, Ht, Wt)
    assert cnt.max() == 1
    tf = U.tex_face(uv_xy, face_uv, Ht, Wt)
    assert np.array_equal(np.unique(tf[tf >= 0]), np.arange(n_faces))  # every face owns a texel
    # no texel of another chart within ``gutter`` texels (Chebyshev) of a chart's texel
    pad = np.pad(tf, gutter + 1, constant_values=-1)
    for di in range(-gutter, gutter + 1):
        for dj in range(-gutter, gutter + 1):
            other = pad[gutter + 1 + di:gutter + 1 + di + Ht, gutter + 1 + dj:gutter + 1 + dj + Wt]
            assert not ((tf >= 0) & (other >= 0) & (other != tf)).any(), (di, dj)


def test_triangle_atlas_raises_when_the_cells_are_too_small():
    with pytest.raises(ValueError, match="cells"):
        MS.triangle_atlas(100, 16, 16)  # 50 cells of 2 texels
    with pytest.raises(ValueError, match="cells"):
        MS.triangle_atlas(2, 5, 5, gutter=2)
    with pytest.raises(ValueError):
        MS.triangle_atlas(0, 16, 16)
    with pytest.raises(ValueError):
        MS.triangle_atlas(4, 16, 5000)
    MS.triangle_atlas(2, 6, 6, gutter=2)


def test_uv_to_atlas_conventions_and_refusals():
    xy = MS.uv_to_atlas(np.array([[0.0, 0.0], [1.0, 1.0], [0.5 / 8, 1 - 0.5 / 4], [0.5, 0.5]]), 4, 8)
    assert xy.dtype == np.int32 and xy.tolist() == [[-8, 56], [120, -8], [0, 0], [56, 24]]  # texel (0, 0) has its centre at u = 0.5 / Wt, v = 1 - 0.5 / Ht
    for bad in ([[0.5, np.nan]], [[np.inf, 0.5]], [[-1e-9, 0.5]], [[0.5, 1.0 + 1e-9]]):
        with pytest.raises(ValueError):
            MS.uv_to_atlas(np.array(bad), 8, 8)
    with pytest.raises(ValueError):
        MS.uv_to_atlas(np.zeros((3, 3)), 8, 8)
    with pytest.raises(ValueError):
        MS.uv_to_atlas(np.zeros((3, 2)), 0, 8)


# ---- files
OBJ_V = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [1.0, 1.0, 0.25], [0.0, 1.0, -0.125], [0.5, 0.5, 1.0]]
OBJ_VT = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.25], [0.125, 0.75]]


def test_read_mesh_uv_forms_and_refusals(tmp_path):
    p = tmp_path / "m.obj"
    lines = ["# comment", "vn 0 0 1"] + [f"v {a} {b} {c}" for a, b, c in OBJ_V] + [f"vt {a} {b}" for a, b in OBJ_VT[:5]]
    lines += ["f 1/1 2/2 3/3 4/4", "f 1/1/1 2/2/1 5/5/1", "vt 0.125 0.75 0.0", "f -4/-5 -3/-4 -1/-1"]
    p.write_text("\n".join(lines) + "\n")
    v, f, uv, fuv = MS.read_mesh_uv(p)
    assert v.dtype == np.float64 and f.dtype == np.int32 and uv.dtype == np.float64 and fuv.dtype == np.int32
    assert np.array_equal(v, np.array(OBJ_V)) and np.array_equal(uv, np.array(OBJ_VT))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4]] and fuv.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 5]]
    v2, f2 = MS.read_mesh(p)  # read_mesh reads the same file as before
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    for body, match in (("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3\n", "no vt"), ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1//1 2//1 3//1\n", "no vt"),
                        ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/2\n", "outside"), ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 9/1\n", "outside"),
                        ("v 0 0 0\nvt 0 0\n", "no faces")):
        q = tmp_path / "bad.obj"
        q.write_text(body)
        with pytest.raises(ValueError, match=match):
            MS.read_mesh_uv(q)
    with pytest.raises(ValueError, match="obj"):
        MS.read_mesh_uv(tmp_path / "m.ply")


def test_write_obj_round_trip_and_png_orientation(tmp_path):
    from PIL import Image
    v, f = R.icosphere(1, 0.3, (0.1, -0.2, 1.0 / 3.0))
    uv, fuv = MS.triangle_atlas(len(f), 32, 48)
    tex = np.full((32, 48, 3), 0.5)
    tex[0, 0] = (1.0, 0.0, 0.25)  # the top-left texel: u = 0.5 / 48, v = 1 - 0.5 / 32
    tex[31, 47] = (np.nan, 2.0, -1.0)
    got = MS.write_obj(tmp_path / "head_textured.obj", v, f, uv, fuv, torch.from_numpy(tex), texture_name="head_texture.png")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["head_texture.png", "head_textured.mtl", "head_textured.obj"]
    assert got == {k: str(tmp_path / n) for k, n in (("obj", "head_textured.obj"), ("mtl", "head_textured.mtl"), ("png", "head_texture.png"))}
    v2, f2, uv2, fuv2 = MS.read_mesh_uv(got["obj"])
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(uv2, uv) and np.array_equal(fuv2, fuv)
    assert "mtllib head_textured.mtl" in open(got["obj"]).read() and "map_Kd head_texture.png" in open(got["mtl"]).read()
    img = np.asarray(Image.open(got["png"]))
    assert img.shape == (32, 48, 3) and img.dtype == np.uint8
    assert img[0, 0].tolist() == [255, 0, 64] and img[31, 47].tolist() == [0, 255, 0] and (img[1:31] == 128).all()
    MS.write_obj(tmp_path / "plain.obj", v, f, uv, fuv, tex)  # the default texture name
    assert (tmp_path / "plain.png").exists()
    with pytest.raises(ValueError):
        MS.write_obj(tmp_path / "x.obj", v, f, uv, fuv[:5], tex)
    with pytest.raises(ValueError):
        MS.write_obj(tmp_path / "x.ply", v, f, uv, fuv, tex)


def test_face_incidence_lists_the_faces_of_a_vertex_in_ascending_order():
    v, f = R.icosphere(1)
    ptr, inc = MS.face_incidence(f, len(v) + 1)  # one vertex without a face
    assert ptr.dtype == np.int32 and inc.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == 3 * len(f) and ptr[-2] == ptr[-1]
    for k in range(len(v)):
        mine = inc[ptr[k]:ptr[k + 1]]
        assert (np.diff(mine) > 0).all() and sorted(mine) == sorted(np.nonzero((f == k).any(1))[0])
    with pytest.raises(ValueError):
        MS.face_incidence(f, len(v) - 1)


# ---- argument checks in Python precede any launch
def test_python_argument_checks_precede_any_launch():
    v, f = R.icosphere(0, 0.3)
    K, RT = R.ring_cameras(2, 16, 16)
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    uv, fuv = MS.triangle_atlas(len(f), 32, 32)
    fut = torch.from_numpy(fuv)
    ptr, inc = (torch.from_numpy(a) for a in MS.face_incidence(f, len(v)))
    with pytest.raises(ValueError):
        E.op_mesh_vertex_normals(vt, ft, ptr, inc)  # [Nv,3]: the op takes frames
    with pytest.raises(ValueError):
        E.op_mesh_vertex_normals(vt[None], ft.long(), ptr, inc)
    with pytest.raises(ValueError):
        E.op_mesh_vertex_normals(vt[None], ft, ptr[:-1], inc)
    with pytest.raises(ValueError):
        E.op_mesh_vertex_normals(vt[None], ft, ptr, inc[:-1])
    N, H, W, Nv = 4, 16, 16, len(v)
    img, fid = torch.zeros(N, 3, H, W), torch.zeros(N, H, W, dtype=torch.int32)
    Kt, RTt, cen, nrm = torch.from_numpy(K), torch.from_numpy(RT), torch.zeros(N, 3), torch.zeros(Nv, 3)
    uv_xy, tf = torch.from_numpy(MS.uv_to_atlas(uv, 32, 32)), torch.zeros(32, 32, dtype=torch.int32)
    ok = (img, fid, fid, Kt, RTt, cen, 2.0, vt, nrm, ft, uv_xy, fut, tf)
    for at, bad in ((0, img.long()), (1, fid[:, :7]), (2, fid.long()), (3, Kt[:3]), (4, RTt[:, :, :3]), (5, cen[:2]), (6, 0.0), (6, float("nan")),
                    (7, vt[:, :2]), (8, nrm[:5]), (9, ft.long()), (10, uv_xy.float()), (11, fut[:5]), (12, tf.long()),
                    (12, torch.zeros(32, 4097, dtype=torch.int32))):
        with pytest.raises(ValueError):
            E.op_mesh_texel_bake(*(ok[:at] + (bad,) + ok[at + 1:]))
    with pytest.raises(ValueError):
        E.op_mesh_texel_bake(*ok, power=0.5)
    with pytest.raises(ValueError):
        E.op_mesh_texel_bake(*ok, fill=(0.5, 0.5))
    tex, val = torch.zeros(8, 8, 3), torch.zeros(8, 8, dtype=torch.bool)
    for args in ((tex[..., :2], val, 1), (tex, val[:7], 1), (tex, val.float(), 1), (tex, val, -1), (tex, val, 65), (tex.long(), val, 1)):
        with pytest.raises(ValueError):
            E.op_mesh_texture_dilate(*args)
    xy, key = torch.zeros(N, Nv, 2, dtype=torch.int32), torch.zeros(N, Nv, dtype=torch.int32)
    uvt = torch.from_numpy(uv)
    good = (xy, key, fid, ft, fut, uvt, tex)
    for at, bad in ((0, xy.long()), (1, key[:, :5]), (2, fid.long()), (3, ft[:, :2]), (4, fut[:5]), (5, uvt[:, :1]), (5, uvt.long()), (6, tex[..., :2])):
        with pytest.raises(ValueError):
            E.op_mesh_render_uv(*(good[:at] + (bad,) + good[at + 1:]))
    with pytest.raises(ValueError):
        E.op_mesh_render_uv(*good, layout="hwc")
    with pytest.raises(ValueError):
        E.op_mesh_render_uv(*good, background=(1, 1))
    # mesh.py: refused on the host, before a device is looked for
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        MS.bake_texture(img, vt, ft, uv + 0.5, fuv, Kt, RTt, size=32)
    with pytest.raises(ValueError, match="cameras"):
        MS.bake_texture(img, vt, ft, uv, fuv, Kt[:2], RTt[:2], size=32)
    with pytest.raises(ValueError, match="face_uv"):
        MS.bake_texture(img, vt, ft, uv, fuv[:5], Kt, RTt, size=32)
    with pytest.raises(ValueError):
        MS.bake_texture(img, vt, ft, uv, fuv, Kt, RTt, size=5000)
    with pytest.raises(ValueError, match="pad"):
        MS.bake_texture(img, vt, ft, uv, fuv, Kt, RTt, size=32, pad=65)
    with pytest.raises(ValueError):
        MS.render_textured(tex[..., :2], vt, ft, uv, fuv, Kt, RTt, 16, 16)
    with pytest.raises(ValueError):
        MS.vertex_normals_device(vt[:, :2], ft)


# ---- the C ABI
def test_c_abi_declares_and_exports_the_entry_points():
    lib = L.load()
    for name, nargs in (("mvd_op_mesh_vertex_normals", 10), ("mvd_op_mesh_texel_bake", 38), ("mvd_op_mesh_texture_dilate", 8),
                        ("mvd_op_mesh_render_uv", 21)):
        assert name in L.PROTOTYPES and len(L.PROTOTYPES[name][1]) == nargs
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs


def abi_error_cases(p):
    """{entry point: {case: arguments with one argument error}}; p: any non-null address of at least 32 bytes (never read)."""
    inf, nan = float("inf"), float("nan")
    q = p + 16  # the dilation refuses outputs that alias its inputs
    nrm = dict(verts=p, faces=p, inc_ptr=p, inc_face=p, F=1, Nv=1, Nf=1, normals=p, bad=p, stream=None)
    bake = dict(images=p, dtype=0, layout=0, face_id=p, pix_key=p, K=p, RT=p, centres=p, z_near=1.0, verts=p, normals=p, faces=p, uv_xy=p,
                face_uv=p, tex_face=p, N=1, Nv=1, Nf=1, Nt=1, H=4, W=4, Ht=4, Wt=4, power=2.0, bias=4096, two_sided=0, fr=0.5, fg=0.5,
                fb=0.5, texture=p, weight_sum=p, n_seen=p, spread=p, visible=None, pos=None, txy=None, tkey=None, stream=None)
    dil = dict(texture=p, valid=p, Ht=4, Wt=4, passes=1, texture_out=q, valid_out=q, stream=None)
    rend = dict(xy=p, key=p, face_id=p, faces=p, face_uv=p, uv=p, texture=p, N=1, Nv=1, Nf=1, Nt=1, H=4, W=4, Ht=4, Wt=4, layout=0, br=1.0,
                bg=1.0, bb=1.0, images=p, stream=None)
    counts = {"N < 1": dict(N=0), "N > 65535": dict(N=65536), "Nv < 1": dict(Nv=0), "Nf < 1": dict(Nf=0), "Nt < 1": dict(Nt=0),
              "N Nv >= 2^30": dict(N=1024, Nv=1 << 20), "3 Nf >= 2^31": dict(Nf=0x2aaaaaab)}
    image = {"H < 1": dict(H=0), "W < 1": dict(W=0), "H > 4096": dict(H=4097), "W > 4096": dict(W=4097)}
    atlas = {"Ht < 1": dict(Ht=0), "Wt < 1": dict(Wt=0), "Ht > 4096": dict(Ht=4097), "Wt > 4096": dict(Wt=4097)}
    bad = {"mvd_op_mesh_vertex_normals": (nrm, dict({f"null {k}": {k: None} for k in ("verts", "faces", "inc_ptr", "inc_face", "normals", "bad")},
                                                     **{"F < 1": dict(F=0), "F > 65535": dict(F=65536), "Nv < 1": dict(Nv=0), "Nf < 1": dict(Nf=0),
                                                        "F Nv >= 2^30": dict(F=1024, Nv=1 << 20), "3 Nf >= 2^31": dict(Nf=0x2aaaaaab)})),
           "mvd_op_mesh_texel_bake": (bake, dict({f"null {k}": {k: None} for k in
                                                  ("images", "face_id", "pix_key", "K", "RT", "centres", "verts", "normals", "faces", "uv_xy",
                                                   "face_uv", "tex_face", "texture", "weight_sum", "n_seen", "spread")},
                                                 **counts, **image, **atlas,
                                                 **{"N H W >= 2^31": dict(N=128, H=4096, W=4096), "N Ht Wt >= 2^31": dict(N=128, Ht=4096, Wt=4096),
                                                    "z_near 0": dict(z_near=0.0), "z_near < 0": dict(z_near=-1.0), "z_near inf": dict(z_near=inf),
                                                    "z_near nan": dict(z_near=nan), "power < 1": dict(power=0.99), "power nan": dict(power=nan),
                                                    "power inf": dict(power=inf), "dtype": dict(dtype=2), "dtype < 0": dict(dtype=-1),
                                                    "layout": dict(layout=2), "layout < 0": dict(layout=-1)})),
           "mvd_op_mesh_texture_dilate": (dil, dict({f"null {k}": {k: None} for k in ("texture", "valid", "texture_out", "valid_out")},
                                                     **atlas, **{"passes < 0": dict(passes=-1), "passes > 64": dict(passes=65),
                                                                 "texture_out aliases": dict(texture_out=p), "valid_out aliases": dict(valid_out=p)})),
           "mvd_op_mesh_render_uv": (rend, dict({f"null {k}": {k: None} for k in
                                                 ("xy", "key", "face_id", "faces", "face_uv", "uv", "texture", "images")},
                                                **counts, **image, **atlas,
                                                **{"3 N H W >= 2^31": dict(N=64, H=4096, W=4096), "layout": dict(layout=2),
                                                   "layout < 0": dict(layout=-1)}))}
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
    assert n == 12 + 44 + 12 + 26

"""GPU: the four UV atlas ops (csrc/k_mesh_uv.hip) one at a time against the numpy oracle tests/mesh_uv_ref.py, and the existing
rasteriser on chart coordinates.  Integers are compared for equality; floats against forward-error bounds derived from the inputs
(each test prints worst error / bound) or, for the fused colours, the tolerances of tests/test_gpu_mesh_ops.check_colours."""
import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from morphablediffusion_amd import mesh as MS
from tests import mesh_ref as R
from tests import mesh_uv_ref as U
from tests.test_gpu_mesh_ops import EPS, dev
from tests.test_mesh_uv_cpu import abi_error_cases, oblique_quad, texels

pytestmark = pytest.mark.gpu


# ---- vertex normals
def normals_op(verts, faces, ptr=None, inc=None):
    if ptr is None:
        ptr, inc = MS.face_incidence(faces, verts.shape[1])
    n, bad = E.op_mesh_vertex_normals(dev(verts), dev(faces), dev(ptr), dev(inc))
    return n.cpu().numpy(), int(bad.item())


def normal_bound(verts, faces):
    """(reference normals, tau [Nv,3], |S| [Nv]) for fp32 inputs, u = 2^-24.  An edge component is one rounding of a difference; a
    cross-product component is a two-term difference of products of two edges, so it is off by at most 3u on each product plus u
    on the difference: 4u P with P = |a_y b_z| + |a_z b_y|.  The sum of deg such terms adds at most (deg - 1) u sum P.  With two
    more u for the second-order terms, E = (5 + deg) u sum P per component of S.  n = S / |S| moves by E / |S| from its own
    component and by |n| ||E|| / |S| from the length; squares, two additions, square root and division of the normalisation
    are 6u more."""
    S, P, deg = U.normal_sums(verts, faces)
    E_ = (5 + deg)[:, None] * EPS * P
    length = np.linalg.norm(S, axis=1)
    ok = length > 0
    n = np.where(ok[:, None], S / np.where(ok, length, 1.0)[:, None], 0.0)
    tau = (E_ + np.abs(n) * np.linalg.norm(E_, axis=1, keepdims=True)) / np.where(ok, length, 1.0)[:, None] + 6 * EPS
    return n, tau, length


def normals_mesh():
    """The scene's mesh plus a vertex X whose two faces (X, p, q) and (X, q, p) cancel; the far vertex has no face at all."""
    s = U.uv_scene()
    verts = np.concatenate([s["verts"], [[0.11, 0.52, -0.07]]]).astype(np.float32)
    x = len(verts) - 1
    faces = np.concatenate([s["faces"], [[x, 3, 17], [x, 17, 3]]]).astype(np.int32)
    return verts, faces, x, len(s["verts"]) - 1


def test_vertex_normals_within_the_forward_error_bound_and_frames_alone():
    verts, faces, x, lone = normals_mesh()
    g = np.random.default_rng(3)
    frames = np.stack([verts, verts * 1.7 + np.float32([0.3, -0.2, 0.9]), verts + g.normal(0, 0.02, verts.shape)]).astype(np.float32)
    got, bad = normals_op(frames, faces)
    assert bad == 0 and got.dtype == np.float32 and got.shape == frames.shape
    worst = 0.0
    for fr in range(3):
        ref, tau, length = normal_bound(frames[fr], faces)
        live = length > 1e-3 * length.max()
        assert live.sum() == len(verts) - 2
        worst = max(worst, (np.abs(got[fr] - ref)[live] / tau[live]).max())
        assert np.abs(np.linalg.norm(got[fr][live], axis=1) - 1).max() <= 4 * EPS
        alone, _ = normals_op(frames[fr:fr + 1], faces)
        assert np.array_equal(alone[0].view(np.int32), got[fr].view(np.int32)), fr  # frame f of the batch, bit for bit
        assert (got[fr][lone] == 0).all() and (got[fr][x] == 0).all()  # no face; two faces that cancel exactly
    print(f"mesh_vertex_normals: worst error / bound {worst:.4f} over 3 frames of {len(verts)} vertices")
    assert worst <= 1.0
    # against the host function it replaces on the new path
    assert np.abs(got[0] - MS.vertex_normals(frames[0], faces)).max() <= 1e-6
    again, _ = normals_op(frames, faces)
    assert np.array_equal(again.view(np.int32), got.view(np.int32))


def test_vertex_normals_of_the_level_1_sphere_are_radial():
    """Every vertex of the level-1 icosphere lies on a symmetry axis of the icosahedral group, so its area-weighted normal is
    radial in exact arithmetic.  The fp32 inputs are off the exact sphere by u r per coordinate: an edge component by 2u r, a
    cross-product component by at most 4 (2u r) L (L: the longest edge), the sum by deg times that; the radial direction of the
    rounded vertex by 2u.  That input term is added to the arithmetic bound."""
    r = 0.3
    v64, f = R.icosphere(1, r)
    v = v64.astype(np.float32)
    got, bad = normals_op(v[None], f)
    ref, tau, length = normal_bound(v, f)
    L_ = np.linalg.norm(v64[f[:, 1]] - v64[f[:, 0]], axis=1).max()
    deg = np.bincount(f.reshape(-1), minlength=len(v))
    e_in = (deg * 8 * EPS * r * L_ / length)[:, None] * (1 + np.sqrt(3.0)) + 2 * EPS
    radial = v64 / r
    ratio = (np.abs(got[0] - radial) / (tau + e_in)).max()
    print(f"mesh_vertex_normals: level-1 sphere, worst |n - radial| / bound {ratio:.4f}; largest bound {(tau + e_in).max():.3e}")
    assert bad == 0 and ratio <= 1.0 and (tau + e_in).max() < 1e-5


def test_vertex_normals_count_bad_indices_without_dereferencing_them():
    s = U.uv_scene()
    verts, faces = s["verts"], s["faces"]
    Nv, Nf = len(verts), len(faces)
    ptr, inc = MS.face_incidence(faces, Nv)
    clean, bad = normals_op(np.stack([verts, verts * 2]), faces, ptr, inc)
    assert bad == 0
    inc2, faces2 = inc.copy(), faces.copy()
    inc2[ptr[5]], inc2[ptr[9] + 1] = Nf + 5, -1  # two table entries outside [0, Nf)
    faces2[3, 1] = Nv + 7  # a corner outside [0, Nv): face 3 is listed in three rows
    faces2[8, 0] = -2
    got, bad = normals_op(np.stack([verts, verts * 2]), faces2, ptr, inc2)
    assert bad == 2 + int(np.isin(inc2, [3, 8]).sum()) and bad >= 6  # every listing of a bad face, counted once (by frame 0)
    touched = np.zeros(Nv, bool)
    touched[[5, 9]] = True
    touched[faces[3]] = touched[faces[8]] = True
    assert np.array_equal(got[:, ~touched].view(np.int32), clean[:, ~touched].view(np.int32)) and np.isfinite(got).all()


# ---- the texel -> face map: the existing rasteriser on chart coordinates
TRI = texels((2.25, 1.5), (13.5, 3.25), (5.75, 12.5))
TEX_FACE_CASES = {
    "a chart and its mirrored twin": (np.concatenate([TRI, np.stack([30 * R.ONE - TRI[:, 0], TRI[:, 1]], -1)]), [[0, 1, 2], [3, 4, 5]]),
    "two overlapping charts": (np.concatenate([TRI, TRI + [3 * R.ONE, 2 * R.ONE]]), [[3, 4, 5], [0, 1, 2]]),
    "a zero-area chart": (texels((3, 3), (6, 6), (9, 9), (2, 8), (12, 9), (4, 14)), [[0, 1, 2], [3, 4, 5]]),
    "a chart vertex on a texel centre": (texels((4, 4), (12.5, 2.25), (5.75, 13)), [[0, 1, 2]]),
    "chart edges through texel centres": (texels((2, 2), (12, 2), (2, 12), (12, 12)), [[0, 1, 2], [1, 3, 2]]),
}


@pytest.mark.parametrize("name", list(TEX_FACE_CASES))
def test_tex_face_is_the_rasteriser_on_chart_coordinates(name):
    uv_xy, face_uv = TEX_FACE_CASES[name]
    uv_xy, face_uv = uv_xy.astype(np.int32), np.asarray(face_uv, np.int32)
    owned = 0
    for Ht, Wt in ((16, 32), (17, 23)):
        want = U.tex_face(uv_xy, face_uv, Ht, Wt)
        got, _, bad = E.op_mesh_raster(dev(uv_xy[None]), dev(np.ones((1, len(uv_xy)), np.int32)), dev(face_uv), Ht, Wt)
        assert int(bad.item()) == 0 and np.array_equal(got[0].cpu().numpy(), want), (name, Ht, Wt)
        owned += int((want >= 0).sum())
        if name == "two overlapping charts":
            assert set(np.unique(want)) == {-1, 0, 1} and (want == 0).sum() > (want == 1).sum()  # the overlap goes to face 0
        if name == "a zero-area chart":
            assert set(np.unique(want)) == {-1, 1}
    assert owned > 50


# ---- the bake
def project_bounds(x32, K, RT, z_near):
    """The oracle's projection of fp32 points and the bounds of test_project_within_the_forward_error_bound_of_the_fp32_chain."""
    ref = R.project(x32, K, RT, z_near)
    Kd, RTd, x = K.astype(np.float64), RT.astype(np.float64), x32.astype(np.float64)
    e = 8 * EPS * (np.einsum("nij,vj->nvi", np.abs(RTd[:, :, :3]), np.abs(x)) + np.abs(RTd[:, None, :, 3]))
    eX, eY, eZ = e[..., 0], e[..., 1], e[..., 2]
    X, Y, Z = ref["cam"][..., 0], ref["cam"][..., 1], ref["cam"][..., 2]
    nu, nv = Kd[:, None, 0, 0] * X + Kd[:, None, 0, 1] * Y, Kd[:, None, 1, 1] * Y
    tau_u = (np.abs(Kd[:, None, 0, 0]) * eX + np.abs(Kd[:, None, 0, 1]) * eY) / Z + np.abs(nu) * eZ / Z ** 2 + 4 * EPS * np.abs(ref["u"])
    tau_v = np.abs(Kd[:, None, 1, 1]) * eY / Z + np.abs(nv) * eZ / Z ** 2 + 4 * EPS * np.abs(ref["v"])
    tau_q = ref["q"] * eZ / Z + 4 * EPS * ref["q"]
    assert ref["valid"].all() and (np.abs(Z - z_near) > eZ).all()
    return ref, tau_u, tau_v, tau_q


def bake_args(s, a, images, normals=None):
    normals = s["normals"] if normals is None else normals
    return (images, dev(s["face_id"]), dev(s["pix_key"]), dev(s["K"]), dev(s["RT"]), dev(s["centres"], torch.float32), s["z_near"],
            dev(s["verts"]), dev(normals, torch.float32), dev(s["faces"]), dev(a["uv_xy"]), dev(a["face_uv"]), dev(a["tex_face"]))


_GEOM = {}


def texel_geometry(s, size):
    """Per atlas, once: the float64 barycentrics, surface points and normals of every texel (the normals the device is given are
    the oracle's rounded to fp32)."""
    if size not in _GEOM:
        a = s["atlases"][size]
        b = U.texel_barycentrics(a["uv_xy"], a["face_uv"], a["tex_face"])
        n32 = s["normals"].astype(np.float32).astype(np.float64)
        _GEOM[size] = dict(b=b, pos=U.texel_points(b, a["tex_face"], s["faces"], s["verts"]),
                           nrm=U.texel_points(b, a["tex_face"], s["faces"], n32))
    return _GEOM[size]


def check_bake(got, ref, tf, tag, fill=(0.5, 0.5, 0.5)):
    """n_seen / visible equal on every texel; texture and spread within 1e-5, weight_sum within 1e-5 relative (the tolerances of
    check_colours), over EVERY texel of the atlas: none is left out."""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.array_equal(g["n_seen"], ref["n_seen"]), tag
    assert np.array_equal(g["visible"], ref["visible"]), tag
    none = ref["weight_sum"] == 0
    ec = np.abs(g["texture"] - ref["texture"]).max()
    es = np.abs(g["spread"][~none] - ref["spread"][~none]).max()
    ew = (np.abs(g["weight_sum"][~none] - ref["weight_sum"][~none]) / ref["weight_sum"][~none]).max()
    print(f"mesh_texel_bake {tag}: worst |texture| {ec:.3e}, |spread| {es:.3e}, weight_sum rel {ew:.3e} over {tf.size} texels "
          f"({(tf >= 0).sum()} in charts, {(~none).sum()} seen, smallest positive weight sum {ref['weight_sum'][~none].min():.3e})")
    assert np.isnan(g["spread"][none]).all() and (g["weight_sum"][none] == 0).all(), tag
    assert np.array_equal(g["texture"][none], np.broadcast_to(np.float32(fill), (none.sum(), 3))), tag
    assert ec <= 1e-5 and es <= 1e-5 and ew <= 1e-5, tag
    return g


def run_bake(s, size, images, layout, tag, **kw):
    a, geo = s["atlases"][size], texel_geometry(s, size)
    got = E.op_mesh_texel_bake(*bake_args(s, a, dev(images)), **kw)
    ref = U.bake(R.to_unit(images, layout), got["txy"].cpu().numpy(), got["tkey"].cpu().numpy(), s["face_id"], s["pix_key"], a["tex_face"],
                 geo["pos"], geo["nrm"], s["centres"].astype(np.float32), **kw)
    return check_bake(got, ref, a["tex_face"], tag, kw.get("fill", (0.5, 0.5, 0.5))), ref, got


@pytest.mark.parametrize("size", [(48, 64), (40, 40)])
def test_bake_points_and_view_integers_within_their_bounds(size):
    s = U.uv_scene()
    a, geo = s["atlases"][size], texel_geometry(s, size)
    tf = a["tex_face"]
    chart = tf >= 0
    assert chart.sum() >= 300 and (~chart).sum() > 300  # 40 x 40: tiles that hang over both edges
    got = E.op_mesh_texel_bake(*bake_args(s, a, dev(np.zeros((s["N"], 3, s["H"], s["W"]), np.float32))))
    pos, txy, tkey = got["pos"].cpu().numpy(), got["txy"].cpu().numpy(), got["tkey"].cpu().numpy()
    assert np.isnan(pos[~chart]).all() and (txy[:, ~chart] == 0).all() and (tkey[:, ~chart] == 0).all()
    # p = sum b_k v_k: b_k is an integer ratio rounded at most three times (two conversions, one division), the three products
    # and two additions round once each: 8u sum |b_k| |v_k| covers it
    mag = (np.abs(geo["b"])[..., None] * np.abs(s["verts"].astype(np.float64))[s["faces"][np.clip(tf, 0, None)]]).sum(2)
    rp = (np.abs(pos - geo["pos"])[chart] / (8 * EPS * mag[chart])).max()
    # the per-view integers: the projection's bound with the device's own point as the fp32 input
    ref, tau_u, tau_v, tau_q = project_bounds(pos[chart], s["K"], s["RT"], s["z_near"])
    xy, key = txy[:, chart], tkey[:, chart]
    assert (key >= 1).all() and (key <= R.KMAX).all()
    du = (np.abs(xy[..., 0] / 16.0 - ref["u"]) / (1 / 32 + tau_u)).max()
    dv = (np.abs(xy[..., 1] / 16.0 - ref["v"]) / (1 / 32 + tau_v)).max()
    dq = (np.abs(key - np.clip(ref["q"], 1, R.KMAX)) / (0.5 + tau_q)).max()
    print(f"mesh_texel_bake {size}: worst error / bound: pos {rp:.4f}, u {du:.4f}, v {dv:.4f}, key {dq:.4f} over {chart.sum()} texels")
    assert rp <= 1.0 and du <= 1.0 and dv <= 1.0 and dq <= 1.0


def test_bake_of_noise_views_in_both_conventions():
    s = U.uv_scene()
    N, H, W = s["N"], s["H"], s["W"]
    g = np.random.default_rng(9)
    f = g.uniform(-1.2, 1.2, (N, 3, H, W)).astype(np.float32)  # beyond [-1, 1]: clamped
    u8 = g.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    a, ref, raw = run_bake(s, (48, 64), f, "nchw", "float NCHW 64x48")
    run_bake(s, (40, 40), u8, "nhwc", "uint8 NHWC 40x40")
    run_bake(s, (40, 40), np.ascontiguousarray(f.transpose(0, 2, 3, 1)), "nhwc", "float NHWC 40x40")
    run_bake(s, (48, 64), np.ascontiguousarray(u8.transpose(0, 3, 1, 2)), "nchw", "uint8 NCHW 64x48")
    # the occluder decides: a texel of the large sphere whose nearest pixel is won by the small one is not seen there
    tf = s["atlases"][(48, 64)]["tex_face"]
    txy = raw["txy"].cpu().numpy().astype(np.int64)
    pj, pi = np.clip((txy[..., 0] + 8) >> 4, 0, W - 1), np.clip((txy[..., 1] + 8) >> 4, 0, H - 1)
    winner = np.stack([s["face_id"][n][pi[n], pj[n]] for n in range(N)])
    hidden = (tf[None] >= 0) & (tf[None] < s["n_big"]) & (winner >= s["n_big"]) & ~ref["visible"]
    assert hidden.sum() >= 3 and (ref["n_seen"] >= 2).sum() > 300 and ((ref["n_seen"] == 0) & (tf >= 0)).any()
    # power, a fill colour, and a bias that decides
    _, r0, _ = run_bake(s, (48, 64), f, "nchw", "bias -2^22", bias=-(1 << 22))
    b, r1, _ = run_bake(s, (48, 64), f, "nchw", "bias 2^22, power 3.5", bias=1 << 22, power=3.5, fill=(0.1, 0.2, 0.3))
    assert (r0["n_seen"] != r1["n_seen"]).sum() > 50
    # two calls agree bit for bit; without the taps the outputs are the same
    again = E.op_mesh_texel_bake(*bake_args(s, s["atlases"][(48, 64)], dev(f)))
    bare = E.op_mesh_texel_bake(*bake_args(s, s["atlases"][(48, 64)], dev(f)), taps=False)
    assert sorted(bare) == ["n_seen", "spread", "texture", "weight_sum"]
    for k in ("texture", "weight_sum", "spread", "n_seen", "visible", "pos", "txy", "tkey"):
        x, y = again[k].cpu().numpy(), a[k]
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y), k
    for k in bare:
        x, y = bare[k].cpu().numpy(), a[k]
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y), k


def test_bake_two_sided_on_an_inverted_mesh():
    s = dict(U.uv_scene())
    s["faces"] = np.ascontiguousarray(s["faces"][:, [0, 2, 1]])  # the other winding: the normals point inwards
    s["normals"] = U.vertex_normals(s["verts"], s["faces"])
    P = s["proj"]
    s["face_id"], s["pix_key"], _ = R.raster(P["xy"], P["key"], s["faces"], s["H"], s["W"])
    a = s["atlases"][(40, 40)]
    b = U.texel_barycentrics(a["uv_xy"], a["face_uv"], a["tex_face"])
    geo = dict(pos=U.texel_points(b, a["tex_face"], s["faces"], s["verts"]),
               nrm=U.texel_points(b, a["tex_face"], s["faces"], s["normals"].astype(np.float32).astype(np.float64)))
    img = np.random.default_rng(2).uniform(-1, 1, (s["N"], s["H"], s["W"], 3)).astype(np.float32)
    out = {}
    for two in (False, True):
        got = E.op_mesh_texel_bake(*bake_args(s, a, dev(img)), two_sided=two)
        ref = U.bake(R.to_unit(img, "nhwc"), got["txy"].cpu().numpy(), got["tkey"].cpu().numpy(), s["face_id"], s["pix_key"], a["tex_face"],
                     geo["pos"], geo["nrm"], s["centres"].astype(np.float32), two_sided=two)
        check_bake(got, ref, a["tex_face"], f"inverted, two_sided={two}")
        out[two] = ref
    chart = a["tex_face"] >= 0
    assert (out[False]["weight_sum"][chart] == 0).mean() > 0.5 and (out[True]["weight_sum"][chart] > 0).mean() > 0.9


def test_bake_of_constant_views_is_constant():
    s = U.uv_scene()
    N, H, W = s["N"], s["H"], s["W"]
    c = np.array([-0.5, 0.25, 0.75], dtype=np.float32)  # (c + 1) / 2 is exact in fp32
    img = np.broadcast_to(c[None, :, None, None], (N, 3, H, W)).copy()
    for size in ((48, 64), (40, 40)):
        a = s["atlases"][size]
        got = {k: v.cpu().numpy() for k, v in E.op_mesh_texel_bake(*bake_args(s, a, dev(img)), fill=(0.1, 0.2, 0.3)).items()}
        seen = got["weight_sum"] > 0
        chart = a["tex_face"] >= 0
        assert seen.sum() > 0.8 * chart.sum() and not seen[~chart].any() and (chart & ~seen).any()
        # sum w c / sum w with one c: N products, N - 1 additions and a division against the same sum of w: (N + 2) u
        assert np.abs(got["texture"][seen] - (c.astype(np.float64) + 1) / 2).max() <= (N + 2) * EPS
        assert got["spread"][seen].max() <= 1e-6
        # uncovered and unseen texels: the fill colour, a NaN spread
        assert np.array_equal(got["texture"][~seen], np.broadcast_to(np.float32([0.1, 0.2, 0.3]), ((~seen).sum(), 3)))
        assert np.isnan(got["spread"][~seen]).all() and (got["weight_sum"][~seen] == 0).all() and (got["n_seen"][~chart] == 0).all()


# ---- dilation
def test_dilate_equals_the_oracle_round_by_round():
    g = np.random.default_rng(6)
    Ht, Wt = 23, 37
    tex = g.random((Ht, Wt, 3)).astype(np.float32)
    val = g.random((Ht, Wt)) < 0.04
    val[0, 0] = val[Ht - 1, Wt - 1] = True
    for passes in (0, 1, 2, 5):
        t, v = E.op_mesh_texture_dilate(dev(tex), dev(val), passes)
        rt, rv = U.dilate(tex, val, passes)
        t, v = t.cpu().numpy(), v.cpu().numpy()
        assert v.dtype == bool and np.array_equal(v, rv), passes
        err = np.abs(t - rt).max()
        print(f"mesh_texture_dilate: {passes} rounds, {v.sum()} of {v.size} valid, worst error {err:.3e} (bound {passes * 10 * EPS:.3e})")
        # a mean of at most 8 values in [0, 1]: one rounding per addition and one for the division, compounding per round
        assert err <= passes * 10 * EPS
        assert np.array_equal(t[~v], tex[~v]) and np.array_equal(t[val], tex[val])  # untouched texels keep their bits
        if passes == 0:
            assert np.array_equal(t.view(np.int32), tex.view(np.int32))
    assert not U.dilate(tex, val, 2)[1].all() and U.dilate(tex, val, 5)[1].sum() > U.dilate(tex, val, 2)[1].sum()


def test_dilate_grows_one_texel_as_a_square():
    tex, val = np.full((7, 9, 3), 0.5, np.float32), np.zeros((7, 9), bool)
    tex[3, 4], val[3, 4] = (0.25, 0.5, 1.0), True
    for p in range(5):
        t, v = (x.cpu().numpy() for x in E.op_mesh_texture_dilate(dev(tex), dev(val), p))
        want = np.zeros((7, 9), bool)
        want[max(3 - p, 0):3 + p + 1, max(4 - p, 0):4 + p + 1] = True
        assert np.array_equal(v, want) and np.array_equal(t[v], np.broadcast_to(np.float32([0.25, 0.5, 1.0]), (v.sum(), 3)))
        assert (t[~v] == 0.5).all()


# ---- the UV render
def smooth_texture(Ht, Wt):
    i, j = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    return np.stack([0.5 + 0.5 * np.sin(0.31 * j + 0.2), 0.5 + 0.5 * np.cos(0.23 * i), (i + j) / (Ht + Wt - 2.0)], -1).astype(np.float32)


def check_render(s, uv, face_uv, tex, tag, layout="nchw", background=(1.0, 1.0, 1.0)):
    """Colours within delta L + 8u: delta = 8u max(Ht, Wt) is the error of the texel coordinate out of the fp32 chain (three
    products and two additions on barycentrics rounded once, times the atlas size), L the largest difference between adjacent
    texels, and 8u the bilinear blend and the map to [-1, 1]."""
    Ht, Wt = tex.shape[:2]
    got = E.op_mesh_render_uv(dev(s["xy"]), dev(s["key"]), dev(s["face_id"]), dev(s["faces"]), dev(face_uv), dev(uv, torch.float32), dev(tex),
                              layout=layout, background=background).cpu().numpy()
    if layout == "nchw":
        got = got.transpose(0, 2, 3, 1)
    ref, _, _ = U.render(s["xy"], s["key"], s["face_id"], s["faces"], face_uv, np.asarray(uv, np.float32), tex, background)
    t64 = tex.astype(np.float64)
    L_ = max(np.abs(np.diff(t64, axis=0)).max(), np.abs(np.diff(t64, axis=1)).max())
    bound = 8 * EPS * max(Ht, Wt) * L_ + 8 * EPS
    err = np.abs((got.astype(np.float64) + 1) / 2 - (ref + 1) / 2)
    mask = s["face_id"] >= 0
    print(f"mesh_render_uv {tag}: worst error / bound {err.max() / bound:.4f} (bound {bound:.3e}, L {L_:.3f}) over {mask.sum()} covered pixels")
    assert err.max() <= bound, tag
    assert np.array_equal(got[~mask], np.broadcast_to(2 * np.float32(background) - 1, ((~mask).sum(), 3)))
    return got, ref, bound


def test_render_of_smooth_and_noise_textures():
    s = U.uv_scene()
    assert (s["face_id"] >= 0).mean() > 0.1
    for size in ((48, 64), (40, 40)):
        a = s["atlases"][size]
        check_render(s, a["uv"], a["face_uv"], smooth_texture(*size), f"smooth {size}")
        noise = np.random.default_rng(8).random(size + (3,)).astype(np.float32)
        check_render(s, a["uv"], a["face_uv"], noise, f"noise {size}", layout="nhwc", background=(0.25, 0.5, 0.0))
    # a constant texture renders constant on the mask
    a = s["atlases"][(40, 40)]
    got, _, _ = check_render(s, a["uv"], a["face_uv"], np.full((40, 40, 3), 0.375, np.float32), "constant")
    assert (got[s["face_id"] >= 0] == -0.25).all() and (got[s["face_id"] < 0] == 1.0).all()
    again, _, _ = check_render(s, a["uv"], a["face_uv"], np.full((40, 40, 3), 0.375, np.float32), "constant again")
    assert np.array_equal(again, got)


def test_render_is_perspective_correct_on_an_oblique_quad():
    s = oblique_quad()
    tex = smooth_texture(64, 64)
    got, ref, bound = check_render(s, s["uv"], s["face_uv"], tex, "oblique quad")
    affine, _, _ = U.render(s["xy"], s["key"], s["face_id"], s["faces"], s["face_uv"], s["uv"].astype(np.float32), tex, perspective=False)
    mask = s["face_id"] >= 0
    gap = np.abs((got.astype(np.float64) - affine) / 2)[mask].max()
    print(f"mesh_render_uv oblique quad: the affine oracle is {gap:.3e} away, {gap / bound:.1f} bounds")
    assert gap > 100 * bound  # the wrong interpolation cannot pass


# ---- one large launch, no oracle
def test_bake_of_a_20480_face_sphere_into_a_1024_atlas():
    v, f = R.icosphere(5, 0.3)
    K, RT = R.ring_cameras(8, 256, 256)
    uv, face_uv = MS.triangle_atlas(len(f), 1024, 1024)
    views = torch.full((16, 3, 256, 256), 0.25, device="cuda")
    a = MS.bake_texture(views, v.astype(np.float32), f, uv, face_uv, K, RT, size=1024, pad=0, z_near=2.0)
    b = MS.bake_texture(views, v.astype(np.float32), f, uv, face_uv, K, RT, size=1024, pad=0, z_near=2.0)
    seen = a["weight_sum"] > 0
    print(f"mesh_texel_bake 1024^2, 20480 faces, 16 views of 256^2: coverage {a['coverage']:.4f}, {int(seen.sum())} texels seen of "
          f"{int((a['tex_face'] >= 0).sum())} in charts, consistency {a['consistency']:.3e}")
    assert a["coverage"] > 0.5 and int((a["tex_face"] >= 0).sum()) > 200000
    assert (a["texture"][seen] - 0.625).abs().max().item() <= 18 * EPS
    assert (a["texture"][~seen] == 0.5).all() and torch.isnan(a["spread"][~seen]).all()
    for k in ("texture", "weight_sum", "n_seen", "tex_face", "valid"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["spread"].view(torch.int32), b["spread"].view(torch.int32))


def test_c_abi_argument_errors_launch_nothing():
    """The shared error cases on the GPU machine: each returns an error naming its entry point, and the device stays usable."""
    lib = L.load()
    buf = torch.zeros(64, device="cuda")
    for fn, cases in abi_error_cases(buf.data_ptr()).items():
        for name, args in cases.items():
            assert getattr(lib, fn)(*args) != 0, (fn, name)
            assert lib.mvd_last_error().decode().startswith(fn + ": "), (fn, name)
    torch.cuda.synchronize()
    assert (buf == 0).all()

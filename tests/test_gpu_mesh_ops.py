"""GPU: the three mesh texturing ops (csrc/k_mesh.hip) one at a time against the numpy oracle tests/mesh_ref.py.  The projection
is held to the forward-error bound of its fp32 chain, computed from the inputs; the rasteriser, fed integers directly, to
equality; the vertex colours to equality in their integers and 1e-5 in their floats."""
import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from tests import mesh_ref as R
from tests.test_mesh_cpu import abi_error_cases

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- projection
def project_inputs():
    from morphablediffusion_amd.batch import virtual_cameras
    g = np.random.default_rng(11)
    K16, RT16 = virtual_cameras(16, 64)
    pick = [0, 7, 15, 5]
    K, RT = K16[pick, :3, :3].clone(), RT16[pick].clone()
    K[3, 0, 1], K[3, 0, 2], K[3, 1, 2] = 3.75, 29.5, 37.25  # the fourth camera: skew, an off-centre principal point, fy != fx
    K[3, 1, 1] *= 1.1
    verts = np.concatenate([g.uniform(-0.5, 0.5, (300, 3)),  # the cube of the conditioner: Z in 3.8 .. 5.2 around z_near = 4.2
                            g.uniform(-80.0, 80.0, (60, 3)),  # far out: behind the cameras, or in front and off the image
                            g.uniform(-0.5, 0.5, (30, 3)) + [0.0, 60.0, 0.0],  # in front, far above: beyond the guard band
                            [[np.nan, 0.0, 0.0], [0.1, np.inf, 0.2], [-np.inf, np.inf, np.inf]]]).astype(np.float32)
    return verts, K.numpy(), RT.numpy(), 4.2


def test_project_within_the_forward_error_bound_of_the_fp32_chain():
    verts, K, RT, z_near = project_inputs()
    ref = R.project(verts, K, RT, z_near)
    Kd, RTd, x = K.astype(np.float64), RT.astype(np.float64), verts.astype(np.float64)
    finite = np.isfinite(x).all(1)
    with np.errstate(all="ignore"):
        # 3-term dot products: 8 eps (|R||x| + |t|)
        e = 8 * EPS * (np.einsum("nij,vj->nvi", np.abs(RTd[:, :, :3]), np.abs(x)) + np.abs(RTd[:, None, :, 3]))
        eX, eY, eZ = e[..., 0], e[..., 1], e[..., 2]
        X, Y, Z = ref["cam"][..., 0], ref["cam"][..., 1], ref["cam"][..., 2]
        nu, nv = Kd[:, None, 0, 0] * X + Kd[:, None, 0, 1] * Y, Kd[:, None, 1, 1] * Y
        tau_u = (np.abs(Kd[:, None, 0, 0]) * eX + np.abs(Kd[:, None, 0, 1]) * eY) / Z + np.abs(nu) * eZ / Z ** 2 + 4 * EPS * np.abs(ref["u"])
        tau_v = np.abs(Kd[:, None, 1, 1]) * eY / Z + np.abs(nv) * eZ / Z ** 2 + 4 * EPS * np.abs(ref["v"])
        tau_q = ref["q"] * eZ / Z + 4 * EPS * ref["q"]
        # no vertex of the inputs sits within the bound of a threshold: asserted on the oracle before the GPU is touched
        front = finite[None] & (Z >= z_near)
        assert (np.abs(Z - z_near)[:, finite] > eZ[:, finite]).all()
        assert (np.abs(np.abs(ref["u"]) - R.GUARD_PX)[front] > tau_u[front]).all()
        assert (np.abs(np.abs(ref["v"]) - R.GUARD_PX)[front] > tau_v[front]).all()
    valid = ref["valid"]
    assert valid[:, :300].sum() > 600 and (~valid[:, :300]).sum() > 100 and (~valid[:, 360:390] & (Z[:, 360:390] >= z_near)).sum() > 60
    assert (valid[:, 300:360] & (np.abs(ref["u"][:, 300:360]) > 64)).sum() > 5  # inside the guard band, outside the image
    xy, key = E.op_mesh_project(dev(verts), dev(K), dev(RT), z_near)
    assert xy.dtype == torch.int32 and key.dtype == torch.int32 and tuple(xy.shape) == (4, len(verts), 2)
    xy, key = xy.cpu().numpy(), key.cpu().numpy()
    assert np.array_equal(key != 0, valid)
    assert (xy[~valid] == 0).all() and (key[valid] >= 1).all() and (key <= R.KMAX).all()
    du = np.abs(xy[..., 0] / 16.0 - ref["u"])[valid] / (1 / 32 + tau_u[valid])
    dv = np.abs(xy[..., 1] / 16.0 - ref["v"])[valid] / (1 / 32 + tau_v[valid])
    dq = np.abs(key - np.clip(ref["q"], 1, R.KMAX))[valid] / (0.5 + tau_q[valid])
    print(f"mesh_project: worst error / bound: u {du.max():.4f}, v {dv.max():.4f}, key {dq.max():.4f}; "
          f"largest tau_u {tau_u[valid].max():.3e} px, tau_q {tau_q[valid].max():.3e} keys; {valid.sum()} valid of {valid.size}")
    assert du.max() <= 1.0 and dv.max() <= 1.0 and dq.max() <= 1.0
    xy2, key2 = E.op_mesh_project(dev(verts), dev(K), dev(RT), z_near)
    assert np.array_equal(xy2.cpu().numpy(), xy) and np.array_equal(key2.cpu().numpy(), key)


# ---- rasteriser: integer inputs, equality
def P(*pts):
    return np.rint(np.asarray(pts, dtype=np.float64) * R.ONE).astype(np.int64)


def three_views(pts, keys):
    """xy [3,Nv,2], key [3,Nv]: three views holding different data -- shifted by a fraction of a pixel, and transposed (the
    other winding) with other keys (an invalid key 0 becomes valid there)."""
    pts, keys = np.asarray(pts, dtype=np.int64), np.asarray(keys, dtype=np.int64)
    xy = np.stack([pts, pts + [5, -3], pts[:, ::-1] + [-7, 9]])
    key = np.stack([keys, np.minimum(keys * 3, R.KMAX), np.minimum(keys // 2 + 1, R.KMAX)])
    return xy.astype(np.int32), key.astype(np.int32)


def check_raster(xy, key, faces, H, W, want_bad=0):
    faces = np.asarray(faces, dtype=np.int32)
    want_id, want_key, bad = R.raster(xy, key, faces, H, W)
    assert bad == want_bad
    got = E.op_mesh_raster(dev(xy), dev(key), dev(faces), H, W)
    again = E.op_mesh_raster(dev(xy), dev(key), dev(faces), H, W)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    face_id, pix_key, nbad = (t.cpu().numpy() for t in got)
    assert face_id.dtype == np.int32 and face_id.shape == (xy.shape[0], H, W)
    assert int(nbad[0]) == want_bad
    diff = int((face_id != want_id).sum()), int((pix_key != want_key).sum())
    assert diff == (0, 0), f"{diff} pixels differ in (face_id, pix_key) of {face_id.size}"
    assert ((face_id == -1) == (pix_key == 0)).all()
    return want_id


SIZES = [(32, 24), (17, 40)]
TRI = P((2.3, 1.7), (20.4, 5.2), (7.9, 15.6))
SQUARE = P((2, 2), (12, 2), (2, 12), (12, 12))
RASTER_CASES = {
    "one triangle": (TRI, [900, 5000, 70000], [[0, 1, 2]], 0),
    "one triangle, the other winding": (TRI, [900, 5000, 70000], [[0, 2, 1]], 0),
    "a vertex on a pixel centre, edges through pixel centres": (SQUARE, [100, 2000, 300, 4000], [[0, 1, 2]], 0),
    "a quad's shared diagonal": (SQUARE, [100, 2000, 300, 4000], [[0, 1, 2], [1, 3, 2]], 0),
    "coplanar faces with equal keys": (P((1, 1), (15, 2), (3, 14)), [777, 777, 777], [[0, 1, 2], [2, 1, 0], [0, 1, 2]], 0),
    "coplanar faces with equal keys, reversed": (P((1, 1), (15, 2), (3, 14)), [777, 777, 777], [[2, 1, 0], [0, 1, 2]], 0),
    "a zero-area face, two slivers": (P((3, 3), (6, 6), (9, 9), (3, 10), (3.0625, 2), (3.125, 10), (5.5, 5.5), (6.5, 5.5625), (5.5625, 6.5),
                                        (4, 4), (4, 4), (8, 4)),
                                      [5, 6, 7, 8, 9, 10, 11, 12, 13, 1, 2, 3], [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]], 0),
    "partly outside, wholly outside, larger than the image": (
        P((-10, -5), (14, 3), (2, 30), (100, 100), (140, 100), (100, 150), (-300, -200), (500, -100), (20, 600), (-4096, -4096),
          (4096, -4096), (0, 4096)),
        [R.KMAX, 1, R.KMAX // 2, 50, 60, 70, 3000, 2000, 1000, 30, 20, 10], [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]], 0),
    "invalid vertices": (np.concatenate([P((2, 2), (20, 3), (5, 15), (12, 12)), [[R.GUARD + 1, 40], [30, -R.GUARD - 1]]]),
                         [10, 0, 30, 40, 50, 60], [[0, 1, 2], [0, 2, 3], [0, 2, 4], [3, 2, 5]], 0),
    "out-of-range indices": (SQUARE, [100, 2000, 300, 4000], [[0, 1, 2], [0, 1, 99], [-1, 0, 1], [1, 3, 2], [0, 1, 4]], 3),
}


@pytest.mark.parametrize("name", list(RASTER_CASES))
def test_raster_equals_the_oracle(name):
    pts, keys, faces, bad = RASTER_CASES[name]
    xy, key = three_views(pts, keys)
    drawn = 0
    for H, W in SIZES:
        drawn += int((check_raster(xy, key, faces, H, W, bad) >= 0).sum())
    assert drawn > 0 or name.startswith("a zero-area")


def sphere_views(level, H, W, n_views=3):
    v0, f0 = R.icosphere(level, 0.3)
    v1, f1 = R.icosphere(1, 0.12, (0.05, -0.04, 0.46))  # a smaller sphere in front of it: it occludes in some views
    verts, faces = np.concatenate([v0, v1]).astype(np.float32), np.concatenate([f0, f1 + len(v0)]).astype(np.int32)
    K, RT = R.ring_cameras(3, H, W)  # the first three: from the left, the front and the right
    p = R.project(verts, K[:n_views], RT[:n_views], 2.0)
    return p["xy"], p["key"], faces, len(f0)


@pytest.mark.parametrize("level", [1, 3])
def test_raster_of_occluding_spheres_equals_the_oracle(level):
    """80 and 1280 faces (plus the 80 of the occluder); 42 + 42 and 642 + 42 vertices: no multiple of 64 anywhere."""
    for H, W in SIZES:
        xy, key, faces, n_big = sphere_views(level, H, W)
        assert len(faces) % 64 and xy.shape[1] % 64
        want = check_raster(xy, key, faces, H, W)
        assert (want >= n_big).any() and ((want >= 0) & (want < n_big)).any()  # both spheres win pixels


def test_raster_of_a_20480_face_sphere_at_256():
    v, f = R.icosphere(5, 0.3)
    K, RT = R.ring_cameras(1, 256, 256)
    p = R.project(v.astype(np.float32), K[:1], RT[:1], 2.0)
    want = check_raster(p["xy"], p["key"], f, 256, 256)
    assert (want >= 0).sum() > 30000


# ---- vertex colours
def colour_args(s, images):
    return (images, dev(s["xy"]), dev(s["key"]), dev(s["faces"]), dev(s["face_id"]), dev(s["pix_key"]), dev(s["verts"]),
            dev(s["normals"], torch.float32), dev(s["centres"], torch.float32))


def check_colours(got, ref, tag):
    """n_seen / visible equal; color, spread within 1e-5 and weight_sum within 1e-5 relative where the oracle's weight sum is at
    least 1e-6 (elsewhere a ratio of two tiny numbers is compared to nothing); returns the worst errors."""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.array_equal(g["n_seen"], ref["n_seen"]), tag
    assert np.array_equal(g["visible"], ref["visible"]), tag
    keep = ref["weight_sum"] >= 1e-6
    none = ref["weight_sum"] == 0
    assert np.isnan(g["spread"][none]).all() and (g["weight_sum"][none] == 0).all(), tag
    ec = np.abs(g["color"][keep] - ref["color"][keep]).max()
    es = np.abs(g["spread"][keep] - ref["spread"][keep]).max()
    ew = (np.abs(g["weight_sum"][keep] - ref["weight_sum"][keep]) / ref["weight_sum"][keep]).max()
    print(f"mesh_vertex_colors {tag}: worst |color| {ec:.3e}, |spread| {es:.3e}, weight_sum rel {ew:.3e} over {keep.sum()} vertices")
    assert ec <= 1e-5 and es <= 1e-5 and ew <= 1e-5, tag
    return g


def scene_and_share():
    s = R.texture_scene()
    ref = R.vertex_colors(np.zeros((s["N"], s["H"], s["W"], 3)), s["xy"], s["key"], s["faces"], s["face_id"], s["pix_key"], s["verts"],
                          s["normals"], s["centres"])
    # on the oracle alone, before the GPU is touched: at most 2 % of the vertices are left out of the float comparison
    assert (ref["weight_sum"] < 1e-6).mean() <= 0.02
    assert (ref["n_seen"] >= 2).sum() > 500 and (ref["n_seen"] == 0).any()
    return s


def oracle(s, images, layout, **kw):
    return R.vertex_colors(R.to_unit(images, layout), s["xy"], s["key"], s["faces"], s["face_id"], s["pix_key"], s["verts"], s["normals"],
                           s["centres"], **kw)


def test_vertex_colours_of_constant_views():
    s = scene_and_share()
    N, H, W = s["N"], s["H"], s["W"]
    c = np.array([-0.5, 0.25, 0.75], dtype=np.float32)  # (c + 1) / 2 is exact in fp32
    img = np.broadcast_to(c[None, :, None, None], (N, 3, H, W)).copy()
    ref = oracle(s, img, "nchw")
    got = check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(img))), ref, "constant")
    seen = ref["weight_sum"] > 0
    assert seen.sum() > 600
    assert np.abs(got["color"][seen] - (c.astype(np.float64) + 1) / 2).max() <= 1e-6 and got["spread"][seen].max() <= 1e-6
    # one constant per view: sum w_n c_n / sum w_n with the oracle's weights
    cn = np.random.default_rng(5).uniform(-1, 1, (N, 3)).astype(np.float32)
    img = np.broadcast_to(cn[:, :, None, None], (N, 3, H, W)).copy()
    ref = oracle(s, img, "nchw")
    got = check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(img))), ref, "constant per view")
    keep = ref["weight_sum"] >= 1e-6
    want = np.einsum("nv,nc->vc", ref["w"], (cn.astype(np.float64) + 1) / 2)[keep] / ref["weight_sum"][keep, None]
    assert np.abs(got["color"][keep] - want).max() <= 1e-5


def test_vertex_colours_of_noise_views_in_both_conventions():
    s = scene_and_share()
    N, H, W = s["N"], s["H"], s["W"]
    g = np.random.default_rng(9)
    f = g.uniform(-1.2, 1.2, (N, 3, H, W)).astype(np.float32)  # beyond [-1, 1]: clamped
    u8 = g.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    a = check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(f))), oracle(s, f, "nchw"), "float NCHW")
    check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(u8))), oracle(s, u8, "nhwc"), "uint8 NHWC")
    check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(f.transpose(0, 2, 3, 1)))), oracle(s, f, "nchw"), "float NHWC")
    # power, a fill colour, and a bias that decides: asserted on the oracle to change what is seen
    r0, r1 = oracle(s, f, "nchw", bias=-(1 << 22)), oracle(s, f, "nchw", bias=1 << 22, power=3.5, fill=(0.1, 0.2, 0.3))
    assert (r0["n_seen"] != r1["n_seen"]).sum() > 50
    check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(f)), bias=-(1 << 22)), r0, "bias -2^22")
    b = check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(f)), bias=1 << 22, power=3.5, fill=(0.1, 0.2, 0.3)), r1, "bias 2^22, power 3.5")
    # a vertex that no view sees: the fill colour, a NaN spread
    none = r1["n_seen"] == 0
    assert none.any() and none[-1]
    assert np.array_equal(b["color"][none], np.broadcast_to(np.float32([0.1, 0.2, 0.3]), (none.sum(), 3))) and np.isnan(b["spread"][none]).all()
    assert np.array_equal(a["color"][a["weight_sum"] == 0], np.full(((a["weight_sum"] == 0).sum(), 3), 0.5, np.float32))
    # two calls agree bit for bit
    again = E.op_mesh_vertex_colors(*colour_args(s, dev(f)))
    for k in ("color", "weight_sum", "spread", "n_seen", "visible"):
        assert np.array_equal(again[k].cpu().numpy(), a[k], equal_nan=k == "spread"), k
    assert np.array_equal(again["spread"].cpu().numpy().view(np.int32), a["spread"].view(np.int32))


def test_vertex_colours_two_sided_on_an_inverted_sphere():
    H, W = 40, 44
    K, RT = R.ring_cameras(4, H, W)
    v, f = R.icosphere(2, 0.3, inward=True)
    v = v.astype(np.float32)
    p = R.project(v, K, RT, 2.0)
    face_id, pix_key, _ = R.raster(p["xy"], p["key"], f, H, W)
    s = dict(xy=p["xy"], key=p["key"], faces=f, face_id=face_id, pix_key=pix_key, verts=v, normals=R.vertex_normals(v, f),
             centres=R.camera_centres(RT))
    assert ((s["normals"] * v).sum(1) < 0).all()  # the normals point inwards
    img = np.random.default_rng(2).uniform(-1, 1, (len(K), H, W, 3)).astype(np.float32)
    one, two = oracle(s, img, "nhwc"), oracle(s, img, "nhwc", two_sided=True)
    # one-sided, only vertices just past the limb weigh anything (their inward normal faces the camera); two-sided, all do
    assert (one["weight_sum"] == 0).mean() > 0.8 and one["weight_sum"].max() < 0.1 and (one["n_seen"] > 0).mean() > 0.9
    assert (two["weight_sum"] >= 1e-6).mean() >= 0.98
    got = check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(img))), one, "inverted, one-sided")
    none = one["weight_sum"] == 0
    assert (got["color"][none] == 0.5).all() and np.isnan(got["spread"][none]).all()
    check_colours(E.op_mesh_vertex_colors(*colour_args(s, dev(img)), two_sided=True), two, "inverted, two-sided")


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
    with pytest.raises(ValueError):
        E.op_mesh_raster(torch.zeros(1, 3, 2, dtype=torch.int32).cuda(), torch.zeros(1, 3, dtype=torch.int32).cuda(),
                         torch.zeros(1, 3, dtype=torch.int64).cuda(), 8, 8)

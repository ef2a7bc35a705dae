"""GPU: the morphable-model forward (csrc/k_morph.hip) per kernel against the float64 oracle of tests/morphable_ref.py.

Skin kernel: A and coef are given (from the oracle, rounded to float32), so only this kernel's arithmetic is under test, and every
element must lie within the oracle's forward-error bound (derived there for any fp32 order of the same sums).  The cases cover
every listed V, NB, J and F once or more: V = 1 and sizes that are no multiple of the 16 vertices of a workgroup; L below, at and
one past the 64 basis rows of an LDS tile; J = 1 (no pose block); F one past the 32 frames of a workgroup; post given or not;
weights with whole zero columns.

Pose kernel and whole forward: no fixed tolerance.  On the golden's inputs the worst error may be at most 4 times the float32
REFERENCE's own worst error against its float64 run (recorded in tests/golden/morphable_lbs.npz); on seeded inputs, where no
reference run is recorded, 4 times the worst error of the oracle's textbook chain run in float32 on the same inputs.  The margin is
for the device's sinf / cosf (a couple of ulp against libm's one) and the different but fixed order of the chain.
Measured ratios (worst error / yardstick) are printed by the tests and quoted in DESIGN.md section 7."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from morphablediffusion_amd import batch as B
from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from morphablediffusion_amd import morphable as MM
from tests import morphable_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morphable_lbs.npz")
FRAME_TILE = 32  # frames of one workgroup of the skin kernel (csrc/k_morph.hip: SKIN_FT)

# (V, NB, J, F, post, weight columns that are zero everywhere)
SKIN_CASES = [(1, 1, 1, 1, False, ()), (1, 7, 5, FRAME_TILE + 1, True, ()), (63, 7, 1, 3, True, ()), (63, 1, 5, 17, False, ()),
              (63, 150, 5, 1, False, ()), (17, 28, 5, 3, False, ()), (17, 29, 5, FRAME_TILE + 1, True, (4,)),
              (257, 7, 55, 3, True, (3, 17, 54)), (257, 150, 5, FRAME_TILE + 1, False, ()), (257, 7, 5, 17, True, (2,)),
              (5023, 150, 55, 17, True, (0, 9)), (5023, 1, 1, FRAME_TILE + 1, False, ())]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def skin_inputs(V, NB, J, F, zero_cols=(), seed=0):
    """float32 inputs of the skin op as the kernel gets them: the folded basis of a seeded model, coef and A of the oracle."""
    m = R.synthetic_model(100 + seed + V + NB + J, V, NB, J, zero_weight_columns=zero_cols)
    betas, pose = R.seeded_params(7 + seed + F, F, NB, J, zero_pose_frames=(F // 2,) if F > 1 else ())
    jt, jd, basis = R.fold(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"])
    p = R.pose(betas, pose, jt, jd, m["parents"])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"basis": f32(basis), "v_template": m["v_template"], "coef": f32(np.concatenate([betas, p["pose_feature"]], 1)),
            "weights": m["weights"], "A": f32(p["A"])}


POST = MM.flame_alignment().numpy().astype(np.float32)


def run_skin(x, post=None, frames=None):
    sl = slice(None) if frames is None else frames
    return E.op_morph_skin(dev(x["basis"]), dev(x["v_template"]), dev(x["coef"][sl]), dev(x["weights"]), dev(x["A"][sl]),
                           post=None if post is None else dev(post))


@pytest.mark.parametrize("V,NB,J,F,post,zero_cols", SKIN_CASES)
def test_skin_within_the_forward_error_bound(V, NB, J, F, post, zero_cols):
    x = skin_inputs(V, NB, J, F, zero_cols)
    assert x["basis"].shape == (NB + 9 * (J - 1), 3 * V) and all((x["weights"][:, c] == 0).all() for c in zero_cols)
    post = POST if post else None
    got = run_skin(x, post).cpu().numpy().astype(np.float64)
    want, bound = R.skin(x["basis"], x["v_template"], x["coef"], x["weights"], x["A"], post)
    err = np.abs(got - want)
    print(f"skin V={V} NB={NB} J={J} F={F}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, "
          f"worst error = {err.max():.3e}")
    assert got.shape == (F, V, 3) and np.isfinite(got).all()
    assert (err <= bound).all()


def test_skin_with_identity_transforms_gives_the_blended_template():
    V, NB, J, F = 257, 7, 5, 3
    x = dict(skin_inputs(V, NB, J, F))
    x["A"] = np.ascontiguousarray(np.broadcast_to(np.eye(3, 4, dtype=np.float32).reshape(1, 1, 12), (F, J, 12)))
    W = np.zeros((V, J), np.float32)
    W[np.arange(V), np.arange(V) % J] = 1.0  # one joint per vertex: T is [I|0] exactly, and so out = b
    x["weights"] = W
    got = run_skin(x).cpu().numpy().astype(np.float64)
    b = x["v_template"].astype(np.float64).reshape(1, -1) + x["coef"].astype(np.float64) @ x["basis"].astype(np.float64)
    want, bound = R.skin(x["basis"], x["v_template"], x["coef"], W, x["A"])
    assert np.array_equal(want, b.reshape(F, V, 3))
    assert (np.abs(got - b.reshape(F, V, 3)) <= bound).all()


def test_skin_frames_do_not_depend_on_the_batch_and_calls_repeat():
    x = skin_inputs(257, 150, 5, FRAME_TILE + 1)
    for post in (None, POST):
        full = run_skin(x, post)
        assert torch.equal(full, run_skin(x, post))
        for f in (0, 7, 8, FRAME_TILE - 1, FRAME_TILE):  # first and last slot of a wave, last frame of a tile, the next tile
            assert torch.equal(full[f:f + 1], run_skin(x, post, slice(f, f + 1))), f
        assert torch.equal(full[5:22], run_skin(x, post, slice(5, 22)))


def test_skin_and_pose_write_every_output_and_nothing_behind_it():
    lib = L.load()
    V, NB, J, F, GUARD = 63, 7, 5, FRAME_TILE + 1, 4096
    x = skin_inputs(V, NB, J, F)
    t = {k: dev(v) for k, v in x.items()}
    n = F * V * 3
    out = torch.full((n + GUARD,), float("nan"), device=DEV)
    out[n:] = 12345.0
    L.check(lib.mvd_op_morph_skin(L.ptr(t["basis"]), L.ptr(t["v_template"]), L.ptr(t["coef"]), L.ptr(t["weights"]), L.ptr(t["A"]), None,
                                  F, V, NB + 9 * (J - 1), NB, J, L.ptr(out), torch.cuda.current_stream().cuda_stream))
    assert not torch.isnan(out[:n]).any() and (out[n:] == 12345.0).all()
    assert torch.equal(out[:n].reshape(F, V, 3), run_skin(x))

    m = R.synthetic_model(3, 40, NB, J)
    betas, pose = R.seeded_params(4, F, NB, J)
    jt, jd, _ = R.fold(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"])
    sizes = {"j_rest": F * J * 3, "rot": F * J * 9, "pose_feature": F * 9 * (J - 1), "joints": F * J * 3, "A": F * J * 12}
    bufs = {}
    for k, sz in sizes.items():
        bufs[k] = torch.full((sz + GUARD,), float("nan"), device=DEV)
        bufs[k][sz:] = 12345.0
    par = (C.c_int32 * J)(*m["parents"])
    b, p, a, d = dev(betas), dev(pose), dev(jt.astype(np.float32)), dev(jd.astype(np.float32))
    L.check(lib.mvd_op_morph_pose(L.ptr(b), L.ptr(p), L.ptr(a), L.ptr(d), C.addressof(par), F, NB, J, *(L.ptr(bufs[k]) for k in sizes),
                                  torch.cuda.current_stream().cuda_stream))
    for k, sz in sizes.items():
        assert not torch.isnan(bufs[k][:sz]).any() and (bufs[k][sz:] == 12345.0).all(), k


# ---- the pose kernel
def golden():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    g["parents"] = [int(p) for p in g["parents"]]
    return g


def pose_on_device(m, betas, pose):
    jt, jd, _ = R.fold(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"])
    jt, jd = jt.astype(np.float32), jd.astype(np.float32)
    out = E.op_morph_pose(dev(betas), dev(pose), dev(jt), dev(jd), m["parents"])
    return {k: v.cpu().numpy() for k, v in out.items()}, jt, jd


def assert_rest_frames_exact(got, pose):
    rest = [f for f in range(len(pose)) if (pose[f] == 0).all()]
    assert rest
    J = pose.shape[1]
    for f in rest:
        assert np.array_equal(got["A"][f], np.tile(np.eye(3, 4, dtype=np.float32), (J, 1, 1)))
        assert np.array_equal(got["rot"][f], np.tile(np.eye(3, dtype=np.float32), (J, 1, 1)))
        assert (got["pose_feature"][f] == 0).all()


def test_pose_on_the_golden_inputs_against_the_reference():
    g = golden()
    got, _, _ = pose_on_device(g, g["betas"], g["pose"])
    for k in ("A", "joints"):
        err = np.abs(got[k].astype(np.float64) - g[k + "_f64"]).max()
        print(f"pose, golden inputs: {k}: worst error {err:.3e} = {err / g['ref_err_' + k]:.2f} x the float32 reference's {g['ref_err_' + k]:.3e}")
        assert err <= 4 * g["ref_err_" + k], k
    assert_rest_frames_exact(got, g["pose"])


@pytest.mark.parametrize("J", [1, 5, 55])
def test_pose_on_seeded_inputs_against_the_float64_oracle(J):
    NB, F = 20, 8
    m = R.synthetic_model(40 + J, 64, NB, J, parents=R.seeded_tree(J, 9, min_depth=9))
    if J == 55:
        depth = [0] * J
        for i in range(1, J):
            depth[i] = depth[m["parents"][i]] + 1
        assert max(depth) >= 9
    betas, pose = R.seeded_params(50 + J, F, NB, J, zero_pose_frames=(2,))
    got, jt, jd = pose_on_device(m, betas, pose)
    want = R.pose(betas, pose, jt, jd, m["parents"])
    f32 = R.pose(betas, pose, jt, jd, m["parents"], np.float32)  # the textbook chain in float32: the yardstick
    # the rest joints are one fused-multiply-add chain per component: their bound follows from the format alone
    jr_bound = R.gamma(NB + 1) * (np.abs(jt.astype(np.float64))[None] + (np.abs(betas.astype(np.float64)) @ np.abs(jd.astype(np.float64))).reshape(F, J, 3))
    assert (np.abs(got["j_rest"] - want["j_rest"]) <= jr_bound).all()
    for k in ("rot", "joints", "A") + (("pose_feature",) if J > 1 else ()):
        assert f32[k].dtype == np.float32
        yard = np.abs(f32[k].astype(np.float64) - want[k]).max()
        err = np.abs(got[k].reshape(want[k].shape).astype(np.float64) - want[k]).max()
        print(f"pose J={J}: {k}: worst error {err:.3e} = {err / yard:.2f} x the float32 chain's {yard:.3e}")
        assert yard > 0 and err <= 4 * yard, k
    assert got["pose_feature"].shape == (F, 9 * (J - 1))
    assert_rest_frames_exact(got, pose)


# ---- landmarks
def test_landmarks_within_gamma_3_and_exact_at_a_corner():
    m = R.synthetic_model(8, 257, 4, 5, M=7)
    verts = np.random.default_rng(1).normal(size=(3, 257, 3)).astype(np.float32)
    got = E.op_morph_landmarks(dev(verts), dev(m["faces"]), dev(m["lmk_face"]), dev(m["lmk_bary"])).cpu().numpy()
    want, bound = R.landmarks(verts, m["faces"], m["lmk_face"], m["lmk_bary"])
    assert got.shape == (3, 7, 3) and (np.abs(got - want) <= bound).all()
    assert tuple(m["lmk_bary"][0]) == (1.0, 0.0, 0.0)
    assert np.array_equal(got[:, 0], verts[:, m["faces"][m["lmk_face"][0], 0]])
    # an index out of range is never dereferenced: that landmark is NaN, its neighbours are as before
    lf = m["lmk_face"].copy()
    lf[3] = len(m["faces"])
    faces = m["faces"].copy()
    faces[lf[5], 1] = 257
    bad = E.op_morph_landmarks(dev(verts), dev(faces), dev(lf), dev(m["lmk_bary"])).cpu().numpy()
    assert np.isnan(bad[:, [3, 5]]).all() and np.array_equal(bad[:, [0, 1, 2, 4, 6]], got[:, [0, 1, 2, 4, 6]])


# ---- the whole forward
@functools.lru_cache(maxsize=None)
def golden_model():
    g = golden()
    return MM.MorphableModel.from_arrays(g["v_template"], g["shapedirs"], g["posedirs"], g["J_regressor"], g["parents"], g["weights"],
                                         faces=g["faces"], lmk_face=g["lmk_face"], lmk_bary=g["lmk_bary"], device=DEV)


def test_forward_on_the_golden_inputs_against_the_reference():
    g, fm = golden(), golden_model()
    out = fm.forward(torch.from_numpy(g["betas"]), torch.from_numpy(g["pose"]))
    assert all(out[k].device.type == "cuda" and out[k].dtype == torch.float32 for k in ("vertices", "joints", "landmarks"))
    for k in ("vertices", "joints"):
        err = np.abs(out[k].cpu().numpy().astype(np.float64) - g[k + "_f64"]).max()
        print(f"forward, golden inputs: {k}: worst error {err:.3e} = {err / g['ref_err_' + k]:.2f} x the float32 reference's")
        assert err <= 4 * g["ref_err_" + k], k
    # a landmark is a convex combination of three vertices, each within the bound just asserted, plus its own three roundings
    lm_bound = 4 * g["ref_err_vertices"] + R.landmarks(g["vertices_f64"], g["faces"], g["lmk_face"], g["lmk_bary"])[1]
    assert (np.abs(out["landmarks"].cpu().numpy() - g["landmarks_f64"]) <= lm_bound).all()
    # post rides along: the same vertices through the affine, within its own rounding of values below 1
    M = MM.flame_alignment()
    moved = fm.forward(torch.from_numpy(g["betas"]), torch.from_numpy(g["pose"]), post=M)["vertices"].cpu().double()
    want = torch.from_numpy(g["vertices_f64"]) @ M[:, :3].T + M[:, 3]
    scale = float(M[:, :3].abs().sum(1).max())
    assert (moved - want).abs().max() <= scale * 4 * g["ref_err_vertices"] + R.gamma(4) * (scale * np.abs(g["vertices_f64"]).max() + 1)


def test_flame_with_only_a_shape_is_forward_at_rest():
    g, fm = golden(), golden_model()
    shape = g["betas"][:2]
    a = fm.flame(shape)
    b = fm.forward(torch.from_numpy(shape), torch.zeros(2, 5, 3))
    assert all(torch.equal(a[k], b[k]) for k in ("vertices", "joints", "landmarks"))
    c = fm.flame(shape[:, :8], expression=shape[:, 8:], jaw=g["pose"][:2, 2], eyes=g["pose"][:2, 3:].reshape(2, 6),
                 global_pose=g["pose"][:2, 0], neck=g["pose"][:2, 1])
    d = fm.forward(torch.from_numpy(g["betas"][:2]), torch.from_numpy(g["pose"][:2]))
    assert torch.equal(c["vertices"], d["vertices"])
    one = fm.flame(shape[0])
    assert torch.equal(one["vertices"][0], a["vertices"][0])


def test_frames_to_batch_stacks_what_build_batch_makes():
    g, fm = golden(), golden_model()
    verts = fm.forward(torch.from_numpy(g["betas"][:2]), torch.from_numpy(g["pose"][:2]), post=MM.flame_alignment())["vertices"]
    img = torch.rand(32, 32, 3) * 2 - 1
    batch = MM.frames_to_batch(img, verts, num_views=4, image_size=32, device=DEV)
    assert tuple(batch["vertices"].shape) == (2, 257, 3) and tuple(batch["target_K"].shape) == (2, 4, 4, 4)
    assert tuple(batch["input_image"].shape) == (2, 32, 32, 3) and all(v.shape[0] == 2 for v in batch.values())
    for f in range(2):
        coord, out_sh, bounds = B.voxelize(verts[f])
        assert torch.equal(batch["coord"][f], coord) and torch.equal(batch["out_sh"][f], out_sh)
        assert torch.equal(batch["bounds"][f], bounds) and torch.equal(batch["vertices"][f], verts[f])

"""GPU: the morphable-model backward and the fitter's kernels (csrc/k_morph_bwd.hip) one at a time against the float64 oracle of
tests/morphable_bwd_ref.py, on seeded synthetic models.

Skin backward: A, coef and the blended template are given (from the oracle, rounded to float32), so only this kernel's arithmetic
is under test, and every element of g_b, g_coef, g_A and g_transl must lie within the oracle's forward-error bound, which holds
for any fp32 order of the same sums.  The cases cover V = 1, 17, 63, 257; V = 255, 256, 257, which sit below, at and above the
256-vertex chunk of the vertex phase and at the same time below, at and above a boundary of the 256-column slabs of the basis
phase (765, 768 and 771 columns), and V = 85, 86 around the first slab boundary; L = 64 and 65 (one past the 64 basis rows of a
workgroup); J = 1, 5, 55; F = 1, 3, 33 (one past the 32 frames of a workgroup); post given or not; weights with whole zero
columns; one FLAME-size case.

Pose backward: no closed bound; the worst error per output may be at most 4 times the float32 yardstick: on the golden's inputs the
float32 REFERENCE autograd's own worst error against its float64 run (tests/golden/morphable_lbs_bwd.npz), on seeded inputs the
oracle VJP run in float32.  Landmarks, data term: within the bounds of their sums.  Update: against torch.optim.Adam in float32."""
import functools
import os

import numpy as np
import pytest
import torch

from morphablediffusion_amd import engine as E
from morphablediffusion_amd import lib as L
from morphablediffusion_amd import morphable as MM
from tests import morphable_bwd_ref as BR
from tests import morphable_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
FRAME_TILE, CHUNK, SLAB = 32, 256, 256  # csrc/k_morph_bwd.hip: BB_FT; csrc/morph.h: MORPH_BWD_CHUNK, MORPH_BWD_SLAB
POST = MM.flame_alignment().numpy().astype(np.float32)
U, gamma = R.U, R.gamma

# (V, NB, J, F, post, weight columns that are zero everywhere)
SKIN_BWD_CASES = [(1, 1, 1, 1, False, ()), (17, 7, 5, 3, True, ()), (63, 28, 5, FRAME_TILE + 1, False, ()), (63, 29, 5, 3, True, (4,)),
                  (85, 7, 5, 3, False, ()), (86, 7, 5, 1, True, ()), (CHUNK - 1, 7, 5, 3, True, ()),
                  (CHUNK, 12, 5, FRAME_TILE + 1, False, (2,)), (CHUNK + 1, 7, 55, 3, True, (3, 17, 54)),
                  (CHUNK + 1, 1, 1, FRAME_TILE + 1, False, ()), (5023, 150, 5, 3, True, (1,))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def skin_inputs(V, NB, J, F, zero_cols=()):
    """float32 inputs of the skin backward as the kernel gets them: the folded basis of a seeded model, A and the blended template
    of the oracle, a seeded cotangent."""
    m = R.synthetic_model(200 + V + NB + J, V, NB, J, zero_weight_columns=zero_cols)
    betas, pose = R.seeded_params(9 + F, F, NB, J, zero_pose_frames=(F // 2,) if F > 1 else ())
    jt, jd, basis = R.fold(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"])
    p = R.pose(betas, pose, jt, jd, m["parents"])
    coef = f32(np.concatenate([betas, p["pose_feature"]], 1))
    basis = f32(basis)
    blend = f32((m["v_template"].reshape(1, -1).astype(np.float64) + coef.astype(np.float64) @ basis.astype(np.float64)).reshape(F, V, 3))
    g_y = f32(np.random.default_rng(V + F).normal(size=(F, V, 3)))
    return {"basis": basis, "v_template": m["v_template"], "coef": coef, "weights": m["weights"], "A": f32(p["A"]), "blend": blend,
            "g_y": g_y}


def run_skin_bwd(x, post=None, frames=None):
    sl = slice(None) if frames is None else frames
    return E.op_morph_skin_bwd(dev(x["g_y"][sl]), dev(x["weights"]), dev(x["A"][sl]), dev(x["blend"][sl]), dev(x["basis"]),
                               post=None if post is None else dev(post))


@pytest.mark.parametrize("V,NB,J,F,post,zero_cols", SKIN_BWD_CASES)
def test_skin_bwd_within_the_forward_error_bound(V, NB, J, F, post, zero_cols):
    x = skin_inputs(V, NB, J, F, zero_cols)
    post = POST if post else None
    got = run_skin_bwd(x, post)
    want = BR.skin_bwd(x["g_y"], x["weights"], x["A"], x["blend"], x["basis"], post)
    nchunk, nslab = E.morph_bwd_counts(V)
    assert nchunk == -(-V // CHUNK) and nslab == -(-3 * V // SLAB)
    assert got["part_a"].shape == (nchunk, F, J * 12 + 3) and got["part_c"].shape == (nslab, F, NB + 9 * (J - 1))
    for k in ("part_a", "part_c", "g_b"):
        assert not torch.isnan(got[k]).any(), k  # the wrapper fills every output with NaN before the call
    for k, (val, bound) in want.items():
        g = got[k].cpu().numpy().astype(np.float64)
        err = np.abs(g - val)
        print(f"skin_bwd V={V} NB={NB} J={J} F={F} {k}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, "
              f"worst error = {err.max():.3e}")
        assert g.shape == val.shape and (err <= bound).all(), k
    for c in zero_cols:  # a joint no vertex follows gets an exactly zero adjoint
        assert not got["g_A"][:, c].any()


def test_skin_bwd_frames_do_not_depend_on_the_batch_and_calls_repeat():
    x = skin_inputs(CHUNK + 1, 12, 5, FRAME_TILE + 1)
    for post in (None, POST):
        full = run_skin_bwd(x, post)
        again = run_skin_bwd(x, post)
        for k in ("g_b", "part_a", "part_c"):
            assert torch.equal(full[k], again[k]), k
        for f in (0, FRAME_TILE - 1, FRAME_TILE):  # first frame, last frame of a tile, the next tile
            one = run_skin_bwd(x, post, slice(f, f + 1))
            assert torch.equal(full["g_b"][f:f + 1], one["g_b"]), f
            assert torch.equal(full["part_a"][:, f:f + 1], one["part_a"]) and torch.equal(full["part_c"][:, f:f + 1], one["part_c"]), f
            assert torch.equal(full["g_coef"][f:f + 1], one["g_coef"]) and torch.equal(full["g_A"][f:f + 1], one["g_A"]), f


def test_skin_bwd_writes_every_output_and_nothing_behind_it():
    lib = L.load()
    V, NB, J, F, GUARD = CHUNK + 1, 7, 5, FRAME_TILE + 1, 4096
    x = skin_inputs(V, NB, J, F)
    t = {k: dev(v) for k, v in x.items()}
    Lr = NB + 9 * (J - 1)
    nchunk, nslab = E.morph_bwd_counts(V)
    sizes = {"g_b": F * V * 3, "part_a": nchunk * F * (J * 12 + 3), "part_c": nslab * F * Lr}
    out = {}
    for k, n in sizes.items():
        out[k] = torch.full((n + GUARD,), float("nan"), device=DEV)
        out[k][n:] = 12345.0
    L.check(lib.mvd_op_morph_skin_bwd(L.ptr(t["g_y"]), None, L.ptr(t["weights"]), L.ptr(t["A"]), L.ptr(t["blend"]), L.ptr(t["basis"]), F, V,
                                      Lr, NB, J, L.ptr(out["g_b"]), L.ptr(out["part_a"]), L.ptr(out["part_c"]),
                                      torch.cuda.current_stream().cuda_stream))
    ref = run_skin_bwd(x)
    for k, n in sizes.items():
        assert torch.equal(out[k][:n], ref[k].reshape(-1)), k
        assert (out[k][n:] == 12345.0).all(), k


# ---- pose backward
def golden():
    g = {}
    for name in ("morphable_lbs.npz", "morphable_lbs_bwd.npz"):
        with np.load(os.path.join(HERE, "golden", name)) as z:
            g.update({k: z[k] for k in z.files})
    g["parents"] = [int(p) for p in g["parents"]]
    return g


def run_pose_bwd(betas, pose, jt, jd, parents, g_A, g_joints, g_coef, g_transl=None, chunks=1):
    """The pose backward on the device after the device's own pose forward; the adjoints enter as one chunk and one slab, or, with
    chunks = 3, split into three partials (x/2, x/4, x/4: exact in binary, so the ascending sum gives x back bit for bit)."""
    F, J = pose.shape[:2]
    fw = E.op_morph_pose(dev(betas), dev(pose), dev(jt), dev(jd), parents)
    gt = np.zeros((F, 3), np.float32) if g_transl is None else g_transl
    pa = np.concatenate([f32(g_A).reshape(F, J * 12), f32(gt)], 1)[None]
    pc = f32(g_coef)[None]
    if chunks == 3:
        pa, pc = (np.concatenate([a * np.float32(0.5), a * np.float32(0.25), a * np.float32(0.25)], 0) for a in (pa, pc))
    return E.op_morph_pose_bwd(dev(pose), fw["j_rest"], fw["A"], dev(jd), parents, dev(pa), dev(pc),
                               g_joints=None if g_joints is None else dev(f32(g_joints)))


def test_pose_bwd_on_the_golden_inputs_against_the_reference_autograd():
    g = golden()
    jt, jd, _ = (f32(a) for a in R.fold(g["v_template"], g["shapedirs"], g["posedirs"], g["J_regressor"]))
    NB = g["betas"].shape[1]
    g_coef = np.concatenate([np.zeros((3, NB), np.float32), g["g_pf"]], 1)
    got = run_pose_bwd(g["betas"], g["pose"], jt, jd, g["parents"], g["g_A"], g["g_joints"], g_coef)
    # the folds were rounded to float32 for the device: the float64 target is the oracle on those values, which the CPU suite ties
    # to the reference's autograd to 1e-15
    want = BR.pose_vjp(g["betas"], g["pose"], jt, jd, g["parents"], g_A=g["g_A"], g_joints=g["g_joints"], g_pose_feature=g["g_pf"])
    for k in ("betas", "pose"):
        err = np.abs(got[k].cpu().numpy().astype(np.float64) - want[k]).max()
        yard = float(g[f"ref_err_pose_{k}"])
        print(f"pose_bwd golden g_{k}: worst error {err:.3e}, float32 reference autograd {yard:.3e}, ratio {err / yard:.2f}")
        assert np.isfinite(got[k].cpu().numpy()).all() and err <= 4 * yard, k
    assert (g["pose"][1] == 0).all() and torch.isfinite(got["pose"][1]).all() and got["pose"][1].abs().max() > 0  # the frame at rest
    assert not got["transl"].any()


@pytest.mark.parametrize("J,NB,F", [(1, 7, 3), (5, 12, 4), (55, 20, 3)])
def test_pose_bwd_on_seeded_inputs_against_the_float32_oracle(J, NB, F):
    parents = R.seeded_tree(J, 40 + J, min_depth=9 if J == 55 else 0)
    m = R.synthetic_model(60 + J, 97, NB, J, parents=parents)
    betas, pose = R.seeded_params(61 + J, F, NB, J, zero_pose_frames=(1,))
    jt, jd, _ = (f32(a) for a in R.fold(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"]))
    rng = np.random.default_rng(J)
    g_A, g_j, g_t = f32(rng.normal(size=(F, J, 3, 4))), f32(rng.normal(size=(F, J, 3))), f32(rng.normal(size=(F, 3)))
    g_coef = f32(rng.normal(size=(F, NB + 9 * (J - 1))))
    got = run_pose_bwd(betas, pose, jt, jd, parents, g_A, g_j, g_coef, g_t)
    split = run_pose_bwd(betas, pose, jt, jd, parents, g_A, g_j, g_coef, g_t, chunks=3)
    kw = dict(g_A=g_A, g_joints=g_j, g_pose_feature=g_coef[:, NB:])
    w64 = BR.pose_vjp(betas, pose, jt, jd, parents, **kw)
    w32 = BR.pose_vjp(betas, pose, jt, jd, parents, dtype=np.float32, **kw)
    w64["betas"] = w64["betas"] + g_coef[:, :NB].astype(np.float64)
    w32["betas"] = w32["betas"] + g_coef[:, :NB]
    for k in ("betas", "pose"):
        assert w32[k].dtype == np.float32
        err = np.abs(got[k].cpu().numpy().astype(np.float64) - w64[k]).max()
        yard = np.abs(w32[k].astype(np.float64) - w64[k]).max()
        print(f"pose_bwd J={J} g_{k}: worst error {err:.3e}, float32 oracle {yard:.3e}, ratio {err / yard:.2f}")
        assert torch.isfinite(got[k]).all() and yard > 0 and err <= 4 * yard, k
        assert torch.equal(got[k], split[k]), k  # partials summed in ascending order: x/2 + x/4 + x/4 is x exactly
    assert (pose[1] == 0).all() and got["pose"][1].abs().max() > 0
    assert torch.equal(got["transl"], dev(g_t)) and torch.equal(split["transl"], dev(g_t))
    again = run_pose_bwd(betas, pose, jt, jd, parents, g_A, g_j, g_coef, g_t)
    assert all(torch.equal(got[k], again[k]) for k in got)
    one = run_pose_bwd(betas[2:3], pose[2:3], jt, jd, parents, g_A[2:3], g_j[2:3], g_coef[2:3], g_t[2:3])
    assert all(torch.equal(got[k][2:3], one[k]) for k in got)


# ---- landmarks backward
def landmark_case():
    rng = np.random.default_rng(4)
    V, Nf, M, F = 300, 80, 12, 3
    faces = rng.integers(0, V, (Nf, 3)).astype(np.int32)
    faces[0], faces[1], faces[2] = (5, 6, 7), (7, 8, 9), (290, 291, 292)  # faces 0 and 1 share vertex 7; face 2 touches nothing else
    faces[3:][np.isin(faces[3:], (290, 291, 292))] = 0
    lmk_face = rng.integers(3, Nf, M).astype(np.int32)
    lmk_face[:4] = (0, 0, 1, 2)  # two landmarks on one face, one on a face sharing a vertex with it, one alone
    bary = rng.random((M, 3))
    bary = f32(bary / bary.sum(1, keepdims=True))
    bary[3] = (1.0, 0.0, 0.0)
    return V, F, M, faces, lmk_face, bary, f32(rng.normal(size=(F, M, 3))), f32(rng.normal(size=(F, V, 3)))


def test_landmarks_bwd_gathers_within_the_bound_of_its_sums():
    V, F, M, faces, lmk_face, bary, g_lmk, g_in = landmark_case()
    ptr, ent = (dev(a) for a in E.landmark_csr(faces, lmk_face, bary, V))
    for gi in (None, g_in):
        got = E.op_morph_landmarks_bwd(dev(g_lmk), ptr, ent, dev(bary), V, g_in=None if gi is None else dev(gi))
        want, bound = BR.landmarks_bwd(g_lmk, faces, lmk_face, bary, V, g_in=gi)
        g = got.cpu().numpy().astype(np.float64)
        assert g.shape == (F, V, 3) and (np.abs(g - want) <= bound).all()
        assert torch.equal(got, E.op_morph_landmarks_bwd(dev(g_lmk), ptr, ent, dev(bary), V, g_in=None if gi is None else dev(gi)))
    got = E.op_morph_landmarks_bwd(dev(g_lmk), ptr, ent, dev(bary), V).cpu().numpy()
    assert np.array_equal(got[:, 290], g_lmk[:, 3]) and not got[:, 291:293].any()  # barycentric (1, 0, 0), nothing shared: exact
    touched = np.unique(faces[lmk_face])
    assert not np.delete(got, touched, axis=1).any()
    assert len(BR.landmark_entries(faces, lmk_face, V)[7]) >= 3  # the shared vertex sums three entries or more


# ---- data term
def test_fit_data_energy_and_gradient_against_the_oracle():
    V, F, M, faces, lmk_face, bary, _, _ = landmark_case()
    rng = np.random.default_rng(8)
    y, t = f32(rng.normal(size=(F, V, 3)) * 0.1), f32(rng.normal(size=(F, V, 3)) * 0.1)
    vw, lw = f32(rng.random(V)), f32(rng.random(M))
    vw[[0, 7, 290]], lw[[1, 3]] = 0.0, 0.0
    ptr, ent = (dev(a) for a in E.landmark_csr(faces, lmk_face, bary, V))
    lmk = E.op_morph_landmarks(dev(y), dev(faces), dev(lmk_face), dev(bary))
    tl = f32(rng.normal(size=(F, M, 3)) * 0.1)
    lam = 0.7
    n_ent = np.array([len(e) for e in BR.landmark_entries(faces, lmk_face, V)], dtype=np.float64)
    for name, kw in (("vertices", dict(target=t)), ("weighted", dict(target=t, vertex_weight=vw)),
                     ("broadcast", dict(target=t[:1], vertex_weight=vw, target_lmk=tl[:1], lmk_weight=lw)),
                     ("landmarks", dict(target_lmk=tl)), ("both", dict(target=t, target_lmk=tl, lmk_weight=lw))):
        use_l = "target_lmk" in kw
        dkw = {k: dev(v) for k, v in kw.items()}
        E_got, g_got = E.op_morph_fit_data(dev(y), lmk=lmk if use_l else None, lmk_lambda=lam, csr=(ptr, ent, dev(bary)) if use_l else None,
                                           **dkw)
        l64 = lmk.cpu().numpy().astype(np.float64)
        o = BR.fit_data(y, kw.get("target"), kw.get("vertex_weight"), l64, kw.get("target_lmk"), kw.get("lmk_weight"), lam)
        want_g, mag_g = o["g_verts"].astype(np.float64), np.abs(o["g_verts"]).astype(np.float64)
        if use_l:
            add, _ = BR.landmarks_bwd(o["g_lmk"], faces, lmk_face, bary, V)
            amag, _ = BR.landmarks_bwd(np.abs(o["g_lmk"]), faces, lmk_face, np.abs(bary), V)
            want_g, mag_g = want_g + add, mag_g + amag
        # at most 8 roundings in a term (the residual, the weights and their sums' reciprocals as float32) and one per entry summed
        g_bound = gamma(n_ent + 8)[None, :, None] * mag_g * BR.SECOND_ORDER
        g = g_got.cpu().numpy().astype(np.float64)
        assert (np.abs(g - want_g) <= g_bound).all(), name
        E_bound = gamma(V + M + 16) * o["E"] * BR.SECOND_ORDER  # every term of E is non-negative: E is its own magnitude
        err = np.abs(E_got.cpu().numpy().astype(np.float64) - o["E"])
        print(f"fit_data {name}: E worst error / bound = {(err / E_bound).max():.3f}")
        assert E_got.shape == (F,) and (err <= E_bound).all(), name
        if "vertex_weight" in kw and not use_l:
            assert not g_got[:, [0, 7, 290]].any()  # a vertex of weight zero: an exactly zero gradient
        if name == "both":  # vertex 290 carries landmark 3 alone, whose weight is zero
            g_v = E.op_morph_fit_data(dev(y), target=dev(t))[1]
            assert torch.equal(g_got[:, 290], g_v[:, 290])
        E2, g2 = E.op_morph_fit_data(dev(y), lmk=lmk if use_l else None, lmk_lambda=lam, csr=(ptr, ent, dev(bary)) if use_l else None, **dkw)
        assert torch.equal(E_got, E2) and torch.equal(g_got, g2)
        if name == "both":  # each frame's loss is its own
            E1, g1 = E.op_morph_fit_data(dev(y[1:2]), target=dev(t[1:2]), lmk=lmk[1:2], target_lmk=dev(tl[1:2]), lmk_weight=dev(lw),
                                         lmk_lambda=lam, csr=(ptr, ent, dev(bary)))
            assert torch.equal(E1, E_got[1:2]) and torch.equal(g1, g_got[1:2])


# ---- update
ADAM_AGREEMENT = 4 * 1.2e-7  # 4 x the worst |p - torch's p| / max(|p|, 1) measured over 5 steps when the test was written (1.192e-07)


def test_fit_update_equals_torch_adam_and_leaves_frozen_columns_alone():
    rng = np.random.default_rng(12)
    F, P, steps, lr = 5, 45, 5, float(np.float32(0.05))
    p0 = f32(rng.normal(size=(F, P)))
    grads = [f32(rng.normal(size=(F, P)) * 10.0 ** rng.integers(-4, 2)) for _ in range(steps)]
    lrv = np.full(P, lr, np.float32)
    frozen = [3, 17, 44]
    lrv[frozen] = 0.0
    zero = np.zeros(P, np.float32)
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([ref], lr=lr)
    p, m, v = dev(p0), torch.zeros((F, P), device=DEV), torch.zeros((F, P), device=DEV)
    m[:, frozen], v[:, frozen] = 0.25, 0.5
    for step, g in enumerate(grads, 1):
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        E.op_morph_fit_update(p, dev(g), m, v, dev(lrv), dev(zero), dev(zero), step)
    free = np.setdiff1d(np.arange(P), frozen)
    got, want = p.cpu().numpy().astype(np.float64), ref.detach().numpy().astype(np.float64)
    worst = (np.abs(got - want) / np.maximum(np.abs(want), 1.0))[:, free].max()
    print(f"fit_update: worst |p - torch.optim.Adam's p| / max(|p|, 1) after {steps} steps: {worst:.3e}")
    assert worst <= ADAM_AGREEMENT
    assert torch.equal(p[:, frozen].cpu(), torch.from_numpy(p0[:, frozen]))  # frozen: the bits of p, m and v stay
    assert (m[:, frozen] == 0.25).all() and (v[:, frozen] == 0.5).all()
    # the penalty: g' = g + 2 lam (p - p0), against the oracle's step in float64
    lam, prior = f32(rng.random(P) * 0.1), f32(rng.normal(size=P))
    p2, m2, v2 = dev(p0), torch.zeros((F, P), device=DEV), torch.zeros((F, P), device=DEV)
    q, qm, qv = p0.astype(np.float64), np.zeros((F, P)), np.zeros((F, P))
    for step, g in enumerate(grads, 1):
        E.op_morph_fit_update(p2, dev(g), m2, v2, dev(lrv), dev(lam), dev(prior), step)
        BR.adam_step(q, g.astype(np.float64), qm, qv, lrv.astype(np.float64), lam.astype(np.float64), prior.astype(np.float64), step)
    # per step one rounding of p and a step of at most lr (1 + 8 u): 5 (u |p| + 8 u lr) <= 7 u max(|p|, 1); twice that, since m and
    # v carry their own roundings from step to step
    assert (np.abs(p2.cpu().numpy() - q) / np.maximum(np.abs(q), 1.0)).max() <= 16 * U
    assert np.array_equal(p2.cpu().numpy()[:, frozen], p0[:, frozen])


# ---- the extended forward
def test_skin_ex_is_the_skin_op_and_adds_the_translation_and_the_blend():
    V, NB, J, F = CHUNK + 1, 12, 5, FRAME_TILE + 1
    x = skin_inputs(V, NB, J, F)
    t = {k: dev(x[k]) for k in ("basis", "v_template", "coef", "weights", "A")}
    args = (t["basis"], t["v_template"], t["coef"], t["weights"], t["A"])
    transl = f32(np.random.default_rng(2).normal(size=(F, 3)) * 0.05)
    for post in (None, POST):
        pd = None if post is None else dev(post)
        plain = E.op_morph_skin(*args, post=pd)
        assert torch.equal(E.op_morph_skin_ex(*args, post=pd), plain)  # null transl, null blend: the bits of mvd_op_morph_skin
        verts, blend = E.op_morph_skin_ex(*args, post=pd, want_blend=True)
        assert torch.equal(verts, plain)
        L_ = NB + 9 * (J - 1)
        c64, B64, vt64 = (a.astype(np.float64) for a in (x["coef"], x["basis"], x["v_template"]))
        b = (vt64.reshape(1, -1) + c64 @ B64).reshape(F, V, 3)
        db = gamma(L_ + 1) * (np.abs(vt64).reshape(1, -1) + np.abs(c64) @ np.abs(B64)).reshape(F, V, 3)
        assert (np.abs(blend.cpu().numpy().astype(np.float64) - b) <= db).all()
        moved = E.op_morph_skin_ex(*args, post=pd, transl=dev(transl)).cpu().numpy().astype(np.float64)
        bare = E.op_morph_skin(*args).cpu().numpy().astype(np.float64)  # o, the kernel's own bits before post
        o = bare + transl.astype(np.float64)[:, None]
        if post is None:
            assert (np.abs(moved - o) <= U * np.abs(o)).all()  # one more rounding
        else:
            o32 = (bare.astype(np.float32) + transl[:, None]).astype(np.float64)  # that rounding, then post's chain of four
            assert (np.abs(o32 - o) <= U * np.abs(o)).all()
            P64 = post.astype(np.float64)
            want = o32 @ P64[:, :3].T + P64[:, 3]
            mag = np.abs(o32) @ np.abs(P64[:, :3]).T + np.abs(P64[:, 3])
            assert (np.abs(moved - want) <= gamma(4) * mag).all()
    zero = E.op_morph_skin_ex(*args, transl=dev(np.zeros((F, 3), np.float32)))
    assert torch.equal(zero, E.op_morph_skin(*args) + 0.0)

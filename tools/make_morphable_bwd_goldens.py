"""Generate tests/golden/morphable_lbs_bwd.npz: the gradients of the REFERENCE's own linear blend skinning
(third_party/MICA/models/lbs.py, imported by file path as tools/make_morphable_goldens.py does) under torch autograd, on the
inputs of tests/golden/morphable_lbs.npz (V = 257, NB = 12, J = 5, F = 3 with frame 1 at rest) and seeded cotangents.

Two sets, each once in float64 and once in float32:
  whole   d/d(betas, pose) of sum(g_verts . vertices) + sum(g_joints . joints) + sum(g_lmk . landmarks) through lbs() and
          vertices2landmarks()
  pose    d/d(betas, pose) of sum(g_A . A[:, :, :3]) + sum(g_joints . joints) + sum(g_pf . (rot[:, 1:] - I)) through
          vertices2joints / blend_shapes / batch_rodrigues / batch_rigid_transform: the adjoint of mvd_op_morph_pose alone
The file holds data only: the cotangents, the gradients, and the float32 run's worst absolute error against the float64 run per
gradient -- the yardstick of tests/test_gpu_morphable_bwd_ops.py.  Build container only; nothing under tests/ imports this file.

    python tools/make_morphable_bwd_goldens.py [--reference PATH]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ref_import import REFERENCE_ROOT  # noqa: E402

SEED = 31


def run(lbs, z, cot, dtype):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    F, V = z["betas"].shape[0], z["v_template"].shape[0]
    vt, S = t(z["v_template"]), t(z["shapedirs"])
    P = t(z["posedirs"].reshape(3 * V, -1).T.copy())
    Jr, W, par = t(z["J_regressor"]), t(z["weights"]), torch.from_numpy(z["parents"]).long()
    faces, lf = torch.from_numpy(z["faces"]).long(), torch.from_numpy(z["lmk_face"]).long()[None].repeat(F, 1)
    out = {}
    b, p = t(z["betas"]).requires_grad_(), t(z["pose"]).reshape(F, -1).requires_grad_()
    verts, joints = lbs.lbs(b, p, vt[None].expand(F, -1, -1), S, P, Jr, par, W, dtype=dtype)
    lm = lbs.vertices2landmarks(verts, faces, lf, t(z["lmk_bary"])[None].repeat(F, 1, 1))
    loss = (t(cot["g_verts"]) * verts).sum() + (t(cot["g_joints"]) * joints).sum() + (t(cot["g_lmk"]) * lm).sum()
    gb, gp = torch.autograd.grad(loss, (b, p))
    out["whole_betas"], out["whole_pose"] = gb.numpy(), gp.reshape(F, -1, 3).numpy()
    b, p = t(z["betas"]).requires_grad_(), t(z["pose"]).reshape(F, -1).requires_grad_()
    rest = lbs.vertices2joints(Jr, vt[None] + lbs.blend_shapes(b, S))
    rot = lbs.batch_rodrigues(p.reshape(-1, 3), dtype=dtype).view(F, -1, 3, 3)
    joints, A = lbs.batch_rigid_transform(rot, rest, par, dtype=dtype)
    pf = (rot[:, 1:] - torch.eye(3, dtype=dtype)).reshape(F, -1)
    loss = (t(cot["g_A"]) * A[:, :, :3, :]).sum() + (t(cot["g_joints"]) * joints).sum() + (t(cot["g_pf"]) * pf).sum()
    gb, gp = torch.autograd.grad(loss, (b, p))
    out["pose_betas"], out["pose_pose"] = gb.numpy(), gp.reshape(F, -1, 3).numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REFERENCE_ROOT)
    ap.add_argument("--inputs", default=os.path.join(ROOT, "tests", "golden", "morphable_lbs.npz"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "morphable_lbs_bwd.npz"))
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("reference_lbs", os.path.join(a.reference, "third_party", "MICA", "models", "lbs.py"))
    lbs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lbs)
    with np.load(a.inputs) as f:
        z = {k: f[k] for k in f.files}
    F, V, J, M = z["betas"].shape[0], z["v_template"].shape[0], z["weights"].shape[1], z["lmk_face"].shape[0]
    g = np.random.default_rng(SEED)
    cot = {"g_verts": g.normal(size=(F, V, 3)), "g_joints": g.normal(size=(F, J, 3)), "g_lmk": g.normal(size=(F, M, 3)),
           "g_A": g.normal(size=(F, J, 3, 4)), "g_pf": g.normal(size=(F, 9 * (J - 1)))}
    cot = {k: v.astype(np.float32) for k, v in cot.items()}  # exactly representable in both runs
    r32, r64 = run(lbs, z, cot, torch.float32), run(lbs, z, cot, torch.float64)
    out = dict(cot)
    for k in r32:
        out[k + "_f32"], out[k + "_f64"] = r32[k], r64[k]
        out["ref_err_" + k] = np.float64(np.abs(r32[k].astype(np.float64) - r64[k]).max())
        print(f"{k}: float32 reference against its float64 run: max abs error {out['ref_err_' + k]:.3e} "
              f"(largest entry {np.abs(r64[k]).max():.3e})")
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()

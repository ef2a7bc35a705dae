"""Generate tests/golden/morphable_lbs.npz by running the REFERENCE's own linear blend skinning (third_party/MICA/models/lbs.py,
imported by file path: it needs numpy and torch only; flame.py with its loguru / chumpy imports is not touched) on a seeded
synthetic model of FLAME's structure: V = 257, NB = 12, J = 5 with FLAME's tree [-1, 0, 1, 1, 1], F = 3 frames (frame 1 at a
zero pose), M = 7 static landmarks.  Once in float32, as the reference runs it, and once in float64 on the same values.

The file holds data only: the inputs, both sets of outputs (A, posed joints, vertices, landmarks), and the float32 run's own
worst absolute error against the float64 run, separately for A, the joints, the vertices and the landmarks -- the yardstick of
tests/test_gpu_morphable_ops.py.  Build container only; nothing under tests/ imports this file.

    python tools/make_morphable_goldens.py [--reference PATH]   (default: tools/ref_import.py's REFERENCE_ROOT)
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ref_import import REFERENCE_ROOT  # noqa: E402
from tests import morphable_ref as R  # noqa: E402

V, NB, J, F, M, SEED = 257, 12, 5, 3, 7, 20
PARENTS = [-1, 0, 1, 1, 1]


def run(lbs, m, betas, pose, dtype):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    b, p = t(betas), t(pose).reshape(F, -1)
    vt, S = t(m["v_template"]), t(m["shapedirs"])
    P = t(m["posedirs"].reshape(3 * V, -1).T.copy())  # FLAME.__init__: reshape(posedirs, [-1, P]).T
    Jr, W, par = t(m["J_regressor"]), t(m["weights"]), torch.tensor(PARENTS, dtype=torch.long)
    verts, joints = lbs.lbs(b, p, vt[None].expand(F, -1, -1), S, P, Jr, par, W, dtype=dtype)
    # the relative transforms are internal to lbs(): the same calls on the same values
    rest = lbs.vertices2joints(Jr, vt[None] + lbs.blend_shapes(b, S))
    rot = lbs.batch_rodrigues(p.reshape(-1, 3), dtype=dtype).view(F, -1, 3, 3)
    joints2, A = lbs.batch_rigid_transform(rot, rest, par, dtype=dtype)
    assert torch.equal(joints, joints2)
    faces = torch.from_numpy(m["faces"]).long()
    lf = torch.from_numpy(m["lmk_face"]).long()[None].repeat(F, 1)  # as FLAME.compute_landmarks passes them
    lm = lbs.vertices2landmarks(verts, faces, lf, t(m["lmk_bary"])[None].repeat(F, 1, 1))
    return {"A": A[:, :, :3, :].numpy(), "joints": joints.numpy(), "vertices": verts.numpy(), "landmarks": lm.numpy()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REFERENCE_ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "morphable_lbs.npz"))
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("reference_lbs", os.path.join(a.reference, "third_party", "MICA", "models", "lbs.py"))
    lbs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lbs)
    m = R.synthetic_model(SEED, V, NB, J, parents=PARENTS, M=M)
    betas, pose = R.seeded_params(SEED + 1, F, NB, J, zero_pose_frames=(1,))
    r32, r64 = run(lbs, m, betas, pose, torch.float32), run(lbs, m, betas, pose, torch.float64)
    out = {k: m[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "faces", "lmk_face", "lmk_bary")}
    out.update(parents=np.asarray(PARENTS, np.int32), betas=betas, pose=pose)
    for k in r32:
        out[k + "_f32"], out[k + "_f64"] = r32[k], r64[k]
        out["ref_err_" + k] = np.float64(np.abs(r32[k].astype(np.float64) - r64[k]).max())
        print(f"{k}: float32 reference against its float64 run: max abs error {out['ref_err_' + k]:.3e}")
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()

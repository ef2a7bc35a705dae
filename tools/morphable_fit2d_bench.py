"""Time per iteration of the 2-D fitter (mvd_morph_fit_2d_run through engine.morph_fit_2d_run) at FLAME size (V = 5023, NB = 400,
J = 5, M = 51 static + 17 contour landmarks of a 79-row table, C = 16 views) for F = 1 and 16 frames, by tools/morphable_time.py's
method: device events, the median of CALLS calls after 5 warm-up calls; one call runs ITERS iterations with one host
synchronisation at its end.  From the same run, for comparison: the 3-D-landmark iteration of mvd_morph_fit_run on the same model
(what the 2-D stages are added to: both loops share pose, skin, landmarks, landmarks_bwd, skin_bwd, pose_bwd and the update), and
the same 2-D loop composed from torch autograd ops in float32 (tools/morphable_time.py's torch_forward, a masked reprojection loss,
torch.optim.Adam; the contour rows are selected without gradient, as in the library).

  python tools/morphable_fit2d_bench.py [--calls 50] [--iters 20] [--out profiles/morphable_fit2d_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from morphablediffusion_amd import engine as E  # noqa: E402
from morphablediffusion_amd import morphable as MM  # noqa: E402
from morphable_time import SIZES, time_calls, torch_forward  # noqa: E402
from tests import morphable_2d_ref as R2  # noqa: E402
from tests import morphable_ref as R  # noqa: E402

M, MD, ROWS, VIEWS, PX = 51, 17, 79, 16, 1.0 / 512


def setup(F):
    sz = SIZES["flame"]
    V, NB, J = sz["V"], sz["NB"], sz["J"]
    m = R.synthetic_model(11, V, NB, J, M=M, parents=sz["parents"])
    m["dyn_lmk_face"], m["dyn_lmk_bary"] = R2.synthetic_contour(5, m, ROWS, MD, sliding=True)
    fm = MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"],
                                       faces=m["faces"], lmk_face=m["lmk_face"], lmk_bary=m["lmk_bary"], dyn_lmk_face=m["dyn_lmk_face"],
                                       dyn_lmk_bary=m["dyn_lmk_bary"])
    betas, pose = (torch.from_numpy(x).cuda() for x in R.seeded_params(12 + F, F, NB, J))
    K, RT = (torch.from_numpy(a).cuda() for a in R2.cameras(np.linspace(-70.0, 70.0, VIEWS)))
    pr = fm.project_landmarks(betas, pose, K, RT)
    target = {"uv": pr["uv"].clone(), "dyn_uv": pr["contour_uv"].clone(), "lmk": pr["landmarks"].clone()}
    P = NB + 3 * J + 3
    lr, lam, p0 = (torch.from_numpy(a.astype(np.float32)).cuda() for a in fm.fit_vectors(0.05))
    s2, s3 = ([torch.zeros((F, P), device="cuda") for _ in range(3)] for _ in range(2))
    run2 = lambda iters: E.morph_fit_2d_run(fm, s2[0], s2[1], s2[2], lr, lam, p0, iters, K, RT, target["uv"], dyn_target_uv=target["dyn_uv"],
                                            px_scale=PX)
    run3 = lambda iters: E.morph_fit_run(fm, s3[0], s3[1], s3[2], lr, lam, p0, iters, target_lmk=target["lmk"])
    return m, fm, K, RT, target, run2, run3


def torch_loop(m, fm, K, RT, target, F):
    """One Adam iteration of the same 2-D fit from torch autograd ops: a closure to time."""
    V = m["v_template"].shape[0]
    t = {k: torch.from_numpy(m[k]).cuda() for k in ("v_template", "shapedirs", "J_regressor", "weights")}
    t["posedirs"] = torch.from_numpy(np.ascontiguousarray(m["posedirs"].reshape(3 * V, -1).T)).cuda()
    t["parents"] = m["parents"]
    NB, J = m["shapedirs"].shape[2], m["weights"].shape[1]
    betas, pose, transl = (torch.zeros(s, device="cuda", requires_grad=True) for s in ((F, NB), (F, J, 3), (F, 3)))
    opt = torch.optim.Adam([betas, pose, transl], lr=0.05)
    tri = fm.faces[fm.lmk_face.long()].long()
    dyn_tri, Rm, tv = fm.faces[fm.dyn_lmk_face.long()].long(), RT[:, :, :3], RT[:, :, 3]
    n_obs = VIEWS * (M + MD)

    def proj(x):  # x [F,C,n,3] in the world -> uv [F,C,n,2]
        cam = torch.einsum("cik,fcnk->fcni", Rm, x) + tv[None, :, None]
        u = (K[None, :, None, 0, 0] * cam[..., 0] + K[None, :, None, 0, 1] * cam[..., 1]) / cam[..., 2] + K[None, :, None, 0, 2]
        v = K[None, :, None, 1, 1] * cam[..., 1] / cam[..., 2] + K[None, :, None, 1, 2]
        return torch.stack([u, v], -1)

    def step():
        opt.zero_grad(set_to_none=True)
        verts = torch_forward(t, betas, pose) + transl[:, None]
        lmk = (verts[:, tri] * fm.lmk_bary[None, :, :, None]).sum(2)
        with torch.no_grad():  # the library's select: its own kernels, no gradient
            A = E.op_morph_pose(betas.detach(), pose.detach(), fm.j_template, fm.j_dirs, fm.parents)["A"]
            rows = E.op_morph_contour_select(A, RT, fm.neck_joint, ROWS)[0].long()
        dyn = (verts[torch.arange(F, device="cuda")[:, None, None, None], dyn_tri[rows]] * fm.dyn_lmk_bary[rows][..., None]).sum(3)
        r = PX * (proj(lmk[:, None].expand(-1, VIEWS, -1, -1)) - target["uv"])
        rd = PX * (proj(dyn) - target["dyn_uv"])
        ((r.square().sum((1, 2, 3)) + rd.square().sum((1, 2, 3))) / n_obs).sum().backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("morphable_fit2d_bench.py measures on the GPU; no device found")
    sz = SIZES["flame"]
    res = {"device": torch.cuda.get_device_name(0), "iters_per_call": a.iters, "V": sz["V"], "NB": sz["NB"], "J": sz["J"], "M": M, "Md": MD,
           "rows": ROWS, "views": VIEWS, "frames": {}}
    for F in (1, 16):
        m, fm, K, RT, target, run2, run3 = setup(F)
        t2 = time_calls(lambda: run2(a.iters), a.calls)
        t3 = time_calls(lambda: run3(a.iters), a.calls)
        ref = time_calls(torch_loop(m, fm, K, RT, target, F), a.calls)
        ms2, ms3 = t2["median_ms"] / a.iters, t3["median_ms"] / a.iters
        res["frames"][str(F)] = {"fit_2d_run_call": t2, "fit_2d_run_ms_per_iteration": ms2, "fit_run_3d_landmarks_call": t3,
                                 "fit_run_3d_landmarks_ms_per_iteration": ms3, "added_us_per_iteration": (ms2 - ms3) * 1e3,
                                 "torch_autograd_ms_per_iteration": ref["median_ms"], "torch_autograd": ref}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=2)


if __name__ == "__main__":
    main()

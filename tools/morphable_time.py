"""Time of the morphable-model forward (morphable.MorphableModel.forward: op_morph_pose, the coefficient concatenation,
op_morph_skin) and of op_morph_skin alone at FLAME size (V = 5023, NB = 400, J = 5) and SMPL-X size (V = 10475, NB = 20, J = 55)
for F in {1, 16, 64} frames, on seeded synthetic models of those shapes, with device events over CALLS calls after a warm-up.
The baseline is the same formulas composed from torch ops on the same device (the parent commit has no such path).  Each entry
point synchronises its stream, so a call time includes the launch and that synchronisation: it is a call time, not a kernel time.

basis_GBps = bytes of the basis the skin kernel reads (L * 3V * 4, once per tile of 32 frames) over the skin call's median time.
Outputs of the two paths are compared at every timed size (max abs difference, in the model's units).

  python tools/morphable_time.py [--calls 50] [--out profiles/morphable_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from morphablediffusion_amd import engine as E  # noqa: E402
from morphablediffusion_amd import morphable as MM  # noqa: E402
from tests import morphable_ref as R  # noqa: E402

FRAME_TILE = 32
SIZES = {"flame": dict(V=5023, NB=400, J=5, parents=[-1, 0, 1, 1, 1]), "smplx": dict(V=10475, NB=20, J=55, parents=None)}


def time_calls(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "calls": calls}


def torch_forward(t, betas, pose):
    """Linear blend skinning from torch ops, float32 on the device: blend shapes, joint regression, Rodrigues, the chain, skinning."""
    F, J = pose.shape[:2]
    v_shaped = t["v_template"][None] + torch.einsum("bl,mkl->bmk", betas, t["shapedirs"])
    joints = torch.einsum("bik,ji->bjk", v_shaped, t["J_regressor"])
    r = pose.reshape(-1, 3)
    angle = torch.norm(r + 1e-8, dim=1, keepdim=True)
    k = r / angle
    zero = torch.zeros_like(k[:, 0])
    K = torch.stack([zero, -k[:, 2], k[:, 1], k[:, 2], zero, -k[:, 0], -k[:, 1], k[:, 0], zero], 1).reshape(-1, 3, 3)
    rot = (torch.eye(3, device=r.device)[None] + torch.sin(angle)[:, None] * K + (1 - torch.cos(angle))[:, None] * (K @ K)).reshape(F, J, 3, 3)
    v_posed = v_shaped + ((rot[:, 1:] - torch.eye(3, device=r.device)).reshape(F, -1) @ t["posedirs"]).reshape(F, -1, 3)
    G, tr = [rot[:, 0]], [joints[:, 0]]
    for j in range(1, J):
        p = t["parents"][j]
        G.append(G[p] @ rot[:, j])
        tr.append(torch.einsum("fik,fk->fi", G[p], joints[:, j] - joints[:, p]) + tr[p])
    G, tr = torch.stack(G, 1), torch.stack(tr, 1)
    A = torch.cat([G, (tr - torch.einsum("fjik,fjk->fji", G, joints))[..., None]], -1)
    T = (t["weights"] @ A.reshape(F, J, 12)).reshape(F, -1, 3, 4)
    return torch.einsum("fvik,fvk->fvi", T[..., :3], v_posed) + T[..., 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("morphable_time.py measures on the GPU; no device found")
    res = {"device": torch.cuda.get_device_name(0), "frame_tile": FRAME_TILE, "sizes": {}}
    for name, sz in SIZES.items():
        V, NB, J = sz["V"], sz["NB"], sz["J"]
        m = R.synthetic_model(11, V, NB, J, parents=sz["parents"] or R.seeded_tree(J, 9, min_depth=9))
        fm = MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"])
        t = {k: torch.from_numpy(m[k]).cuda() for k in ("v_template", "shapedirs", "J_regressor", "weights")}
        t["posedirs"] = torch.from_numpy(np.ascontiguousarray(m["posedirs"].reshape(3 * V, -1).T)).cuda()
        t["parents"] = m["parents"]
        L = NB + 9 * (J - 1)
        entry = {"V": V, "NB": NB, "J": J, "L": L, "basis_MB": L * 3 * V * 4 / 1e6, "frames": {}}
        for F in (1, 16, 64):
            betas, pose = (torch.from_numpy(x).cuda() for x in R.seeded_params(12 + F, F, NB, J))
            p = E.op_morph_pose(betas, pose, fm.j_template, fm.j_dirs, fm.parents)
            coef = torch.cat([betas, p["pose_feature"]], 1)
            ours, theirs = fm.forward(betas, pose)["vertices"], torch_forward(t, betas, pose)
            skin = time_calls(lambda: E.op_morph_skin(fm.basis, fm.v_template, coef, fm.weights, p["A"], n_betas=NB), a.calls)
            tiles = (F + FRAME_TILE - 1) // FRAME_TILE
            entry["frames"][str(F)] = {
                "forward": time_calls(lambda: fm.forward(betas, pose), a.calls),
                "op_morph_pose": time_calls(lambda: E.op_morph_pose(betas, pose, fm.j_template, fm.j_dirs, fm.parents), a.calls),
                "op_morph_skin": skin, "torch_composition": time_calls(lambda: torch_forward(t, betas, pose), a.calls),
                "basis_GBps": entry["basis_MB"] * tiles / skin["median_ms"], "basis_reads": tiles,
                "max_abs_diff_to_torch": float((ours - theirs).abs().max())}
        res["sizes"][name] = entry
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=2)


if __name__ == "__main__":
    main()

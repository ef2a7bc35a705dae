"""Time of one mesh.texture_mesh call (16 views of 256 x 256 on the virtual arc, a 20 480-face icosphere of radius 0.3) and of its
three entry points, with device events over CALLS calls after a warm-up.  The texture_mesh time includes the host work of the
call (vertex normals in numpy, the copies of the mesh, the read-back of the counter and the two statistics); the op times include
each entry point's own scratch allocation and synchronisation.

  python tools/mesh_texture_time.py [--calls 20] [--out profiles/mesh_texture_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from morphablediffusion_amd import engine as E  # noqa: E402
from morphablediffusion_amd import mesh as MS  # noqa: E402
from morphablediffusion_amd.batch import virtual_cameras  # noqa: E402


def icosphere(level, radius):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
                  (-t, 0, -1), (-t, 0, 1)], dtype=np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)])
    for _ in range(level):
        edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
        uniq, inv = np.unique(edges, axis=0, return_inverse=True)
        mid = len(v) + inv.reshape(3, -1)  # the midpoint vertex of each face's edges ab, bc, ca
        v = np.concatenate([v, v[uniq[:, 0]] + v[uniq[:, 1]]])
        a, b, c, ab, bc, ca = f[:, 0], f[:, 1], f[:, 2], mid[0], mid[1], mid[2]
        f = np.concatenate([np.stack(x, 1) for x in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * radius
    return v.astype(np.float32), f.astype(np.int32)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    N, S = 16, 256
    verts, faces = icosphere(5, 0.3)
    K, RT = virtual_cameras(N, S)
    K = K[:, :3, :3].contiguous()
    views = (torch.rand(N, 3, S, S, generator=torch.Generator().manual_seed(0)) * 2 - 1).cuda()
    v, f, Kd, RTd = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), K.cuda(), RT.cuda()
    z_near = MS.default_z_near(verts, RT)
    out = MS.texture_mesh(views, v, f, K, RT)
    xy, key = E.op_mesh_project(v, Kd, RTd, z_near)
    face_id, pix_key, _ = E.op_mesh_raster(xy, key, f, S, S)
    normals = torch.from_numpy(MS.vertex_normals(verts, faces)).float().cuda()
    centres = (-torch.einsum("nji,nj->ni", RT[:, :, :3].double(), RT[:, :, 3].double())).float().cuda()
    res = {"views": N, "size": S, "faces": int(len(faces)), "vertices": int(len(verts)), "device": torch.cuda.get_device_name(0),
           "coverage": out["coverage"], "consistency": out["consistency"], "covered_pixels_per_view": float((face_id >= 0).sum()) / N,
           "texture_mesh": time_calls(lambda: MS.texture_mesh(views, v, f, K, RT), a.calls),
           "op_mesh_project": time_calls(lambda: E.op_mesh_project(v, Kd, RTd, z_near), a.calls),
           "op_mesh_raster": time_calls(lambda: E.op_mesh_raster(xy, key, f, S, S), a.calls),
           "op_mesh_vertex_colors": time_calls(lambda: E.op_mesh_vertex_colors(views, xy, key, f, face_id, pix_key, v, normals, centres),
                                               a.calls)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=2)


if __name__ == "__main__":
    main()

"""Times of the UV atlas entry points (include/mvd.h: mvd_op_mesh_vertex_normals / _texel_bake / _texture_dilate / _render_uv) with
device events over CALLS calls after a warm-up, medians reported: 16 views of 256 x 256 on the virtual arc, a 20 480-face
icosphere of radius 0.3 with mesh.triangle_atlas charts, atlases of 1024^2 and 2048^2.  The op times include each wrapper's output
allocation and the entry point's own synchronisation, as tools/mesh_texture_time.py's do.  For the bake the bytes it must move
are recorded beside its time, and its time per covered texel beside op_mesh_vertex_colors' time per vertex (the same visibility
test, weight and bilinear sample per view; profiles/mesh_texture_time.json).  Normals: a FLAME-sized grid mesh (5041 vertices,
9800 faces), 1 and 64 frames, against the numpy vertex_normals they replace on the new path.

  python tools/mesh_uv_time.py [--calls 20] [--out profiles/mesh_uv_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from morphablediffusion_amd import engine as E  # noqa: E402
from morphablediffusion_amd import mesh as MS  # noqa: E402
from morphablediffusion_amd.batch import virtual_cameras  # noqa: E402
from mesh_texture_time import icosphere, time_calls  # noqa: E402


def grid_mesh(n):
    """An n x n height field: n^2 vertices, 2 (n - 1)^2 faces."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x, y = i / (n - 1.0) - 0.5, j / (n - 1.0) - 0.5
    v = np.stack([x, y, 0.1 * np.sin(7 * x) * np.cos(5 * y)], -1).reshape(-1, 3).astype(np.float32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)]).astype(np.int32)
    return v, f


def host_ms(fn, calls):
    fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "calls": calls}


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
    xy, key = E.op_mesh_project(v, Kd, RTd, z_near)
    face_id, pix_key, _ = E.op_mesh_raster(xy, key, f, S, S)
    normals = MS.vertex_normals_device(v, f)
    centres = (-torch.einsum("nji,nj->ni", RT[:, :, :3].double(), RT[:, :, 3].double())).float().cuda()
    res = {"views": N, "size": S, "faces": int(len(faces)), "vertices": int(len(verts)), "device": torch.cuda.get_device_name(0),
           "covered_pixels_per_view": float((face_id >= 0).sum()) / N}
    yard = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mesh_texture_time.json")))
    ns_per_vertex = yard["op_mesh_vertex_colors"]["median_ms"] * 1e6 / yard["vertices"]
    for T in (1024, 2048):
        uv, face_uv = MS.triangle_atlas(len(faces), T, T)
        fuv = torch.from_numpy(face_uv).cuda()
        uv_xy = torch.from_numpy(MS.uv_to_atlas(uv, T, T)).cuda()
        ones = torch.ones((1, uv_xy.shape[0]), dtype=torch.int32, device="cuda")
        tex_face = E.op_mesh_raster(uv_xy[None], ones, fuv, T, T)[0][0].contiguous()
        args = (views, face_id, pix_key, Kd, RTd, centres, z_near, v, normals, f, uv_xy, fuv, tex_face)
        out = E.op_mesh_texel_bake(*args, taps=False)
        seen = out["weight_sum"] > 0
        chart = int((tex_face >= 0).sum())
        visits = int(out["n_seen"].sum())
        bake = time_calls(lambda: E.op_mesh_texel_bake(*args, taps=False), a.calls)
        # compulsory traffic: every output and the texel -> face map once, the views and their rasters once, the mesh once;
        # gathered: per (chart texel, view) the nearest pixel's winner and key, per visible pair four taps of three channels
        compulsory = T * T * (4 + 12 + 4 + 4 + 4) + N * S * S * (12 + 8) + len(verts) * 24 + len(faces) * 24 + uv_xy.numel() * 4
        gathered = chart * N * 8 + visits * 2 * 48  # both passes sample
        uvd = torch.from_numpy(uv).float().cuda()
        res[f"atlas_{T}"] = {
            "chart_texels": chart, "seen_texels": int(seen.sum()), "coverage": float(seen.sum()) / max(chart, 1), "visible_pairs": visits,
            "op_mesh_raster_chart": time_calls(lambda: E.op_mesh_raster(uv_xy[None], ones, fuv, T, T), a.calls),
            "op_mesh_texel_bake": dict(bake, compulsory_bytes=compulsory, gathered_bytes=gathered,
                                       compulsory_gb_per_s=compulsory / bake["median_ms"] / 1e6,
                                       ns_per_chart_texel=bake["median_ms"] * 1e6 / max(chart, 1), vertex_colors_ns_per_vertex=ns_per_vertex,
                                       vertex_rate_scaled_ms=ns_per_vertex * chart / 1e6),
            "op_mesh_texture_dilate_pad4": time_calls(lambda: E.op_mesh_texture_dilate(out["texture"], seen, 4), a.calls),
            "op_mesh_render_uv": time_calls(lambda: E.op_mesh_render_uv(xy, key, face_id, f, fuv, uvd, out["texture"]), a.calls),
            "bake_texture": time_calls(lambda: MS.bake_texture(views, v, f, uv, face_uv, K, RT, size=T, z_near=z_near), max(a.calls // 4, 3),
                                       warmup=1)}
    gv, gf = grid_mesh(71)
    ptr, inc = (torch.from_numpy(x).cuda() for x in MS.face_incidence(gf, len(gv)))
    gfd = torch.from_numpy(gf).cuda()
    res["normals"] = {"vertices": int(len(gv)), "faces": int(len(gf))}
    for F in (1, 64):
        frames = torch.from_numpy(np.stack([gv * (1 + 0.01 * k) for k in range(F)])).cuda()
        host = frames.cpu().numpy()
        res["normals"][f"frames_{F}"] = {
            "op_mesh_vertex_normals": time_calls(lambda: E.op_mesh_vertex_normals(frames, gfd, ptr, inc), a.calls),
            "numpy_vertex_normals": host_ms(lambda: [MS.vertex_normals(x, gf) for x in host], max(a.calls // 4, 3))}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=2)


if __name__ == "__main__":
    main()

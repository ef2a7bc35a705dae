"""Times of the closest-point query (mvd_op_mesh_closest_point through engine.op_mesh_closest_point) and of one iteration of the scan
fitter (mvd_morph_fit_scan_run through engine.morph_fit_scan_run), by the method of tools/morphable_time.py: device events, the
median of CALLS calls after 5 warm-up calls.

  query   Q = 5023 and 10475 (FLAME's and SMPL-X's vertices) against a mesh of 100 k and of 500 k faces, and Q = 250 k scan points
          against FLAME's 9976 faces (the scan-to-mesh distance): triangle soups on a sphere, queries on a jittered shell
          around them.
  fit     one iteration at FLAME size (V = 5023, NB = 400, J = 5), F = 1, against a 200 k-face scan, closest points every iteration
          (refresh 1) and every tenth (refresh 10); next to it mvd_morph_fit_run's iteration at the same model size (the fitter
          against a registered target, as it was before the scan fitter existed).
Each next to the same formula composed from torch ops in float32 on the same device (the seven-region test vectorised over a
[queries, faces] block, chunked over queries to fit memory, argmin per chunk); for the fit, the query's torch form plus
tools/morphable_fit_time.py's torch autograd iteration.

Kernel times come from a trace run of their own, never from the timed run:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/closest_point_time.py --trace-body
  python tools/closest_point_time.py --kernel-stats DIR/.../t_kernel_stats.csv --out profiles/closest_point_time.json

Without a device the file is written with every figure as "not measured".  Nothing asserts a time.

  python tools/closest_point_time.py [--calls 50] [--out profiles/closest_point_time.json]"""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from morphablediffusion_amd import engine as E  # noqa: E402

NOT = "not measured"
QUERY_CASES = [(5023, 100_000), (5023, 500_000), (10475, 100_000), (10475, 500_000), (250_000, 9976)]
FIT_SCAN_FACES, FIT_ITERS = 200_000, 10
TORCH_PAIRS = 1 << 22  # [queries, faces] pairs of one chunk of the torch form: about 25 float32 temporaries of that size live at once


def mesh_of(n_faces, seed=0):
    """A soup of n_faces small triangles on a sphere of radius 0.1, each about the size a closed mesh of that many faces would give
    it (no Python loop over faces: 500 k of them are made at once): (verts float32 [3 n, 3], faces int32 [n, 3])."""
    g = np.random.default_rng(seed)
    c = g.normal(size=(n_faces, 1, 3))
    c *= 0.1 / np.linalg.norm(c, axis=2, keepdims=True)
    edge = np.sqrt(4 * np.pi * 0.01 / n_faces * 4 / np.sqrt(3))
    v = (c + g.normal(size=(n_faces, 3, 3)) * edge * 0.4).reshape(-1, 3)
    f = np.arange(3 * n_faces, dtype=np.int32).reshape(n_faces, 3)
    return torch.from_numpy(np.float32(v)).cuda(), torch.from_numpy(f).cuda()


def queries_of(n, seed=1):
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy(np.float32(d * g.uniform(0.08, 0.12, (n, 1)))).cuda()


def torch_closest(q, v, f):
    """The op's formula from torch ops: dist2 [Q] and face [Q], chunked over queries."""
    a, b, c = v[f[:, 0].long()][None], v[f[:, 1].long()][None], v[f[:, 2].long()][None]
    ab, ac = b - a, c - a
    rows = max(1, TORCH_PAIRS // f.shape[0])
    out_d, out_f = [], []
    dot = lambda x, y: (x * y).sum(-1)
    div = lambda n, d: torch.where(d != 0, n / torch.where(d != 0, d, torch.ones_like(d)), torch.zeros_like(d))
    for i in range(0, q.shape[0], rows):
        p = q[i:i + rows, None]
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        s = va + vb + vc
        w1, w2 = div(vb, s).clamp_min(0), div(vc, s).clamp_min(0)
        w0 = (1 - w1 - w2).clamp_min(0)
        one, zero = torch.ones_like(d1), torch.zeros_like(d1)
        for cond, (x0, x1, x2) in (((va <= 0) & (e1 >= 0) & (e2 >= 0), (zero, 1 - div(e1, e1 + e2), div(e1, e1 + e2))),
                                   ((vb <= 0) & (d2 >= 0) & (d6 <= 0), (1 - div(d2, d2 - d6), zero, div(d2, d2 - d6))),
                                   ((d6 >= 0) & (d5 <= d6), (zero, zero, one)),
                                   ((vc <= 0) & (d1 >= 0) & (d3 <= 0), (1 - div(d1, d1 - d3), div(d1, d1 - d3), zero)),
                                   ((d3 >= 0) & (d4 <= d3), (zero, one, zero)), ((d1 <= 0) & (d2 <= 0), (one, zero, zero))):
            w0, w1, w2 = torch.where(cond, x0, w0), torch.where(cond, x1, w1), torch.where(cond, x2, w2)
        r = p - (w0[..., None] * a + w1[..., None] * b + w2[..., None] * c)
        dd, ff = dot(r, r).min(1)
        out_d.append(dd), out_f.append(ff)
    return torch.cat(out_d), torch.cat(out_f)


def fit_setup(refresh):
    from morphable_fit_time import setup
    m, fm, target, run_registered = setup("flame", 1)
    sv, sf = mesh_of(FIT_SCAN_FACES)
    P = fm.NB + 3 * fm.J + 3
    lr, lam, p0 = (torch.from_numpy(a.astype(np.float32)).cuda() for a in fm.fit_vectors(0.05))
    state = [torch.zeros((1, P), device="cuda") for _ in range(3)]
    run = lambda iters: E.morph_fit_scan_run(fm, state[0], state[1], state[2], lr, lam, p0, iters, [(sv, sf)], refresh=refresh)
    return m, fm, target, run, run_registered, (sv, sf)


def kernel_table(path):
    out = {}
    for r in csv.DictReader(open(path)):
        name = re.search(r"\b(closest_\w+_kernel|morph_fit_corr_\w+_kernel)", r["Name"])
        if name:
            calls, total = out.get(name.group(0), (0, 0.0))
            out[name.group(0)] = (calls + int(r["Calls"]), total + float(r["TotalDurationNs"]))
    return {n: {"calls": c, "average_us": t / c / 1e3} for n, (c, t) in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--trace-body", action="store_true", help="run each query case and 10 fit iterations once and exit")
    ap.add_argument("--kernel-stats", type=str, default=None, help="the kernel-stats CSV of a --trace-body run")
    a = ap.parse_args()
    res = {"device": NOT, "method": "device events, median of CALLS after 5 warm-up calls", "calls": a.calls, "query": {}, "fit": {},
           "kernels": NOT}
    for Q, Nf in QUERY_CASES:
        res["query"][f"Q{Q}_Nf{Nf}"] = {"Q": Q, "Nf": Nf, "slabs": NOT, "op_ms": NOT, "torch_ms": NOT}
    for refresh in (1, 10):
        res["fit"][f"refresh{refresh}"] = {"scan_faces": FIT_SCAN_FACES, "fit_scan_run_ms_per_iteration": NOT,
                                           "fit_run_ms_per_iteration_registered_target": NOT, "torch_ms_per_iteration": NOT}
    if torch.cuda.is_available():
        from morphable_time import time_calls
        res["device"] = torch.cuda.get_device_name(0)
        for Q, Nf in QUERY_CASES:
            v, f = mesh_of(Nf)
            q = queries_of(Q)
            if a.trace_body:
                E.op_mesh_closest_point(q, v, f)
                continue
            e = res["query"][f"Q{Q}_Nf{Nf}"]
            e["slabs"] = E.mesh_closest_slabs(Q, Nf)
            e["op"] = time_calls(lambda: E.op_mesh_closest_point(q, v, f), a.calls)
            e["op_ms"] = e["op"]["median_ms"]
            e["torch"] = time_calls(lambda: torch_closest(q, v, f), 3, warmup=1)
            e["torch_ms"] = e["torch"]["median_ms"]
        for refresh in (1, 10):
            m, fm, target, run, run_registered, (sv, sf) = fit_setup(refresh)
            if a.trace_body:
                run(FIT_ITERS)
                continue
            from morphable_fit_time import torch_loop
            e = res["fit"][f"refresh{refresh}"]
            e["fit_scan_run_call"] = time_calls(lambda: run(FIT_ITERS), a.calls)
            e["fit_scan_run_ms_per_iteration"] = e["fit_scan_run_call"]["median_ms"] / FIT_ITERS
            e["fit_run_ms_per_iteration_registered_target"] = time_calls(lambda: run_registered(FIT_ITERS), a.calls)["median_ms"] / FIT_ITERS
            step = torch_loop(m, target, 1)
            y = target[0]
            q_ms = time_calls(lambda: torch_closest(y, sv, sf), 3, warmup=1)["median_ms"]
            e["torch_ms_per_iteration"] = time_calls(step, a.calls)["median_ms"] + q_ms / refresh
        if a.trace_body:
            torch.cuda.synchronize()
            return
    if a.kernel_stats:
        res["kernels"] = kernel_table(a.kernel_stats)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=2)


if __name__ == "__main__":
    main()

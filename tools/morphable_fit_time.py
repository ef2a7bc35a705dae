"""Time per iteration of the morphable-model fitter (mvd_morph_fit_run through engine.morph_fit_run) at FLAME size (V = 5023,
NB = 400, J = 5) and SMPL-X size (V = 10475, NB = 20, J = 55) for F = 1 and 16 frames, on the seeded synthetic models of
tools/morphable_time.py, by its method: device events, the median of CALLS calls after 5 warm-up calls.  One call runs ITERS
iterations (one host synchronisation at its end), so the time per iteration is the call's time over ITERS.  The comparison is the
same loop composed from torch autograd ops in float32 on the same device (tools/morphable_time.py's torch_forward, a mean-square
vertex loss, torch.optim.Adam), one iteration per call.

Kernel times come from a trace run of their own, never from the timed run:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/morphable_fit_time.py --trace-body flame 16
  python tools/morphable_fit_time.py --kernel-stats DIR/.../t_kernel_stats.csv --trace-size flame 16 --out profiles/morphable_fit_time.json

The second command runs the timed measurement and adds, from the CSV, the average duration of every morph_* kernel of that
(size, F) and the basis-phase kernel's rate over the basis bytes (L * 3V * 4, read once per tile of 32 frames), next to the forward
skin call's rate recorded in profiles/morphable_time.json.

  python tools/morphable_fit_time.py [--calls 50] [--iters 20] [--out profiles/morphable_fit_time.json]"""
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
from morphablediffusion_amd import morphable as MM  # noqa: E402
from morphable_time import FRAME_TILE, SIZES, time_calls, torch_forward  # noqa: E402
from tests import morphable_ref as R  # noqa: E402


def setup(name, F):
    sz = SIZES[name]
    V, NB, J = sz["V"], sz["NB"], sz["J"]
    m = R.synthetic_model(11, V, NB, J, parents=sz["parents"] or R.seeded_tree(J, 9, min_depth=9))
    fm = MM.MorphableModel.from_arrays(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["weights"])
    betas, pose = (torch.from_numpy(x).cuda() for x in R.seeded_params(12 + F, F, NB, J))
    target = fm.forward(betas, pose)["vertices"]
    P = NB + 3 * J + 3
    lr, lam, p0 = (torch.from_numpy(a.astype(np.float32)).cuda() for a in fm.fit_vectors(0.05))
    state = [torch.zeros((F, P), device="cuda") for _ in range(3)]
    run = lambda iters: E.morph_fit_run(fm, state[0], state[1], state[2], lr, lam, p0, iters, target=target)
    return m, fm, target, run


def torch_loop(m, target, F):
    """One Adam iteration of the same fit from torch autograd ops: a closure to time."""
    V = m["v_template"].shape[0]
    t = {k: torch.from_numpy(m[k]).cuda() for k in ("v_template", "shapedirs", "J_regressor", "weights")}
    t["posedirs"] = torch.from_numpy(np.ascontiguousarray(m["posedirs"].reshape(3 * V, -1).T)).cuda()
    t["parents"] = m["parents"]
    NB, J = m["shapedirs"].shape[2], m["weights"].shape[1]
    betas, pose, transl = (torch.zeros(s, device="cuda", requires_grad=True) for s in ((F, NB), (F, J, 3), (F, 3)))
    opt = torch.optim.Adam([betas, pose, transl], lr=0.05)

    def step():
        opt.zero_grad(set_to_none=True)
        v = torch_forward(t, betas, pose) + transl[:, None]
        ((v - target).square().sum(-1).mean(-1)).sum().backward()
        opt.step()
    return step


def kernel_table(path):
    """{kernel name without its argument list: (calls, average ns)} of a rocprofv3 kernel-stats CSV, morph_* kernels only."""
    out = {}
    for r in csv.DictReader(open(path)):
        name = re.search(r"\bmorph_\w+", r["Name"])
        if name:
            out[name.group(0)] = (int(r["Calls"]), float(r["TotalDurationNs"]) / int(r["Calls"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--trace-body", nargs=2, metavar=("SIZE", "F"), default=None, help="run 20 iterations at one size and exit")
    ap.add_argument("--kernel-stats", type=str, default=None, help="the kernel-stats CSV of a --trace-body run")
    ap.add_argument("--trace-size", nargs=2, metavar=("SIZE", "F"), default=("flame", "16"), help="what --kernel-stats was taken at")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("morphable_fit_time.py measures on the GPU; no device found")
    if a.trace_body:
        _, _, _, run = setup(a.trace_body[0], int(a.trace_body[1]))
        run(20)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "iters_per_call": a.iters, "sizes": {}}
    for name, sz in SIZES.items():
        L = sz["NB"] + 9 * (sz["J"] - 1)
        entry = {"V": sz["V"], "NB": sz["NB"], "J": sz["J"], "L": L, "basis_MB": L * 3 * sz["V"] * 4 / 1e6, "frames": {}}
        for F in (1, 16):
            m, fm, target, run = setup(name, F)
            fit = time_calls(lambda: run(a.iters), a.calls)
            ref = time_calls(torch_loop(m, target, F), a.calls)
            entry["frames"][str(F)] = {"fit_run_call": fit, "fit_run_ms_per_iteration": fit["median_ms"] / a.iters,
                                       "torch_autograd_ms_per_iteration": ref["median_ms"], "torch_autograd": ref}
        res["sizes"][name] = entry
    if a.kernel_stats:
        name, F = a.trace_size[0], int(a.trace_size[1])
        e = res["sizes"][name]
        table = kernel_table(a.kernel_stats)
        tiles = (F + FRAME_TILE - 1) // FRAME_TILE
        k = {n: {"calls": c, "average_us": ns / 1e3} for n, (c, ns) in sorted(table.items())}
        basis_us = k["morph_skin_bwd_basis_kernel"]["average_us"]
        skin_us = k["morph_skin_kernel"]["average_us"]
        tr = {"size": name, "F": F, "kernels": k, "kernel_us_per_iteration": sum(v["average_us"] for v in k.values()),
              "basis_phase_TBps": e["basis_MB"] * tiles / basis_us, "forward_skin_kernel_TBps": e["basis_MB"] * tiles / skin_us}
        fwd = os.path.join(ROOT, "profiles", "morphable_time.json")
        if os.path.exists(fwd):
            with open(fwd) as fh:
                tr["forward_skin_call_GBps_recorded"] = json.load(fh)["sizes"][name]["frames"][str(F)]["basis_GBps"]
        res["trace"] = tr
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=2)


if __name__ == "__main__":
    main()

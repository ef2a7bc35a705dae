"""GPU: the conditioner's forward gathers (k_cond.hip: vertex_gather_kernel, latent_gather_kernel, frustum_gather_kernel), each on
its own through the mvd_op_*_gather hooks on conditioner-only stage engines, at the boundary cases of
tests/test_cond_gathers_cpu.py and against that module's float64 restatements.  (unproject_views_kernel is held to the same cases
and bounds in tests/test_gpu_spatial_volume.py::test_stage_unproject_matches_the_restatement.)

Per case: (a) every element is written (the buffers start as NaN); (b) a row none of whose taps is in range -- every corner outside
the lattice, off the coarse grid, on cells without a row, behind the camera -- is exactly zero; (c) accuracy against float64, over
the whole output and over the partially-outside rows alone, the boundary code's own product:
    fp32 outputs (vertex, latent)     e_kernel <= 4 e_oracle32 + 1e-7
    operand-type output (frustum)     e_kernel <= 1.1 e_round + 4 e_oracle32,  e_round = rel_l2(want.to(OPD), want)
  where e_oracle32 is the error of the oracle's fp32 functions on the same case (computed on the CPU, never from a kernel): kernel
  and oracle are single fp32 evaluations of the same formulas, operation order moves the position rounding by a small factor, a
  wrong weight, index or stride gives 1e-2 or more; (d) two calls give identical bits; (e) adjointness against BOTH forms of the
  mvd_op_*_adjoint hooks, |<G x, y> - <x, G^T y>| <= (1e-5 + r) |G x| |y| with r = e_round for the frustum (its forward result
  carries one rounding) and 0 otherwise -- a check that does not depend on the restatements; (f) the hooks refuse null pointers,
  view indices out of range and calls before set_mesh / set_cameras without launching anything.
Each case prints a "[gather]" line with its figures before it asserts (recorded in profiles/cond_gather_parity.txt)."""
import ctypes as C

import pytest
import torch

from morphablediffusion_amd import lib as L
from tests import test_cond_gathers_cpu as G
from tests import test_train_deterministic_cpu as R
from tests.test_gpu_train_deterministic import PARITY, engine_for, set_sample

pytestmark = pytest.mark.gpu
N = G.N
OPD = torch.bfloat16 if L.DTYPE == "bf16" else torch.float16


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    from tests.test_gpu_train_deterministic import _engines
    yield
    for eng in _engines.values():
        eng.close()
    _engines.clear()


def _dot(a, b):
    return (a.double() * b.double()).sum().item()


def check_gather(tag, case, run, adjoint, y, rounded):
    """(a)-(e) for one case.  run() -> the hook's output on the device, rows as case["want"]; adjoint(y, deterministic) -> G^T y
    shaped like case["x"]; rounded: the output is stored in the operand type."""
    want, taps, full = case["want"], case["taps"].reshape(-1), case["full"]
    first, second = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(first, second), f"{tag}: two calls differ"
    got = first.cpu().reshape(want.shape)
    assert torch.isfinite(got).all(), f"{tag}: elements left unwritten"
    rows, wrows = got.reshape(taps.numel(), -1), want.reshape(taps.numel(), -1)
    partial = (taps > 0) & (taps < full)
    e_round = R.rel_l2(want.to(OPD), want) if rounded else 0.0
    e_round_p = R.rel_l2(wrows[partial].to(OPD), wrows[partial]) if rounded and partial.any() else 0.0
    e_all = R.rel_l2(got, want) if want.abs().max() > 0 else float(got.abs().max())
    e_part = R.rel_l2(rows[partial], wrows[partial]) if partial.any() else 0.0
    e32 = case["e_oracle32"]
    e32_p = R.rel_l2(case["oracle32"].reshape(wrows.shape)[partial], wrows[partial]) if partial.any() else 0.0
    gx, x = got.reshape(y.shape), case["x"]
    lhs, scale = _dot(gx, y), gx.double().norm().item() * y.double().norm().item()
    res = [abs(lhs - _dot(x, adjoint(y, det).cpu())) for det in (False, True)]
    outside, p_share, none = G.shares(case)
    print(f"[gather] {tag}: e_kernel={e_all:.3e} (partial rows {e_part:.3e}) e_oracle32={e32:.3e} (partial rows {e32_p:.3e}) "
          f"e_round={e_round:.3e} (partial rows {e_round_p:.3e}) taps outside={outside:.3f} rows partial={p_share:.3f} "
          f"rows without a tap={none:.3f} adjointness residual / (|Gx| |y|): atomic {res[0] / max(scale, 1e-300):.3e} "
          f"gather {res[1] / max(scale, 1e-300):.3e}")
    assert (rows[taps == 0] == 0).all(), f"{tag}: a row without a tap in range is not exactly zero"
    if rounded:
        assert e_all <= 1.1 * e_round + 4 * e32
        assert e_part <= 1.1 * e_round_p + 4 * e32_p
    else:
        assert e_all <= 4 * e32 + 1e-7
        assert e_part <= 4 * e32_p + 1e-7
    for r in res:
        assert r <= (PARITY + e_round) * scale, f"{tag}: the gather and its adjoint hook are not transposes of each other"


@pytest.mark.parametrize("case", G.FRUSTUM_CASES, ids=G.case_id)
def test_frustum_gather(case):
    V, D, S, TN, projection, name = case
    c = G.frustum_case(*case)
    eng = engine_for(V, projection, D, S)
    set_sample(eng, "v300", c["K"], c["RT"])
    vol = c["x"].cuda()
    y = torch.randn(TN, D, S, S, 64, generator=torch.Generator().manual_seed(7 + V + TN))
    if projection == "orthographic" and name == "stage":
        assert (c["taps"] == 0).all() and c["want"].abs().max() == 0  # the all-outside case: the output is all zeros
    check_gather(f"frustum {G.case_id(case)}", c, lambda: eng.op_frustum_gather(vol, c["views"], D, S),
                 lambda g, det: eng.op_frustum_adjoint(g.cuda(), c["views"], deterministic=det), y, True)


@pytest.mark.parametrize("case", G.LATENT_CASES, ids=G.case_id)
def test_latent_gather(case):
    V, kind = case
    c = G.latent_case(*case)
    eng = engine_for(V, "perspective", *((5, 6) if V == 8 else (6, 8)))
    K, RT = R.rig(N, "perspective", 64)
    set_sample(eng, kind, K, RT)
    rows = c["x"].cuda()
    y = torch.randn(V, V, V, 64, generator=torch.Generator().manual_seed(8 + V))
    check_gather(f"latent {G.case_id(case)} rows={c['n_rows']} grid={tuple(c['grid'].shape)}", c, lambda: eng.op_latent_gather(rows),
                 lambda g, det: eng.op_latent_adjoint(g.cuda(), deterministic=det), y, False)


@pytest.mark.parametrize("case", G.VERTEX_CASES, ids=G.case_id)
def test_vertex_gather(case):
    kind, projection, name = case
    c = G.vertex_case(*case)
    eng = engine_for(8, projection)
    set_sample(eng, kind, c["K"], c["RT"])
    feats = c["x"].cuda()
    y = torch.randn(N, c["verts"].shape[0], 16, generator=torch.Generator().manual_seed(9))
    check_gather(f"vertex {G.case_id(case)} Nv={c['verts'].shape[0]} leaving={c['leaving']}", c, lambda: eng.op_vertex_gather(feats),
                 lambda g, det: eng.op_vertex_adjoint(g.cuda(), deterministic=det), y, False)


def test_hooks_refuse_bad_arguments_without_launching():
    V, D, S = 8, 5, 6
    eng = engine_for(V, "perspective", D, S)
    K, RT = R.rig(N, "perspective", 8 * S)
    verts = set_sample(eng, "v300", K, RT)[0]
    lib, ctx = eng.lib, eng._ctx
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    feats, vf = torch.zeros(N, G.S_MAP, G.S_MAP, 16, device="cuda"), nan(N, verts.shape[0], 16)
    n_rows = R.rulebook_grid(*R.mesh("v300")[1:3])[1]
    rows, vol_out = torch.zeros(n_rows, 64, device="cuda"), nan(V, V, V, 64)
    vol, out = torch.zeros(V, V, V, 64, device="cuda"), nan(2, D, S, S, 64)
    idx4, idx2, bad4, bad2 = (C.c_int32 * 4)(0, 1, 2, 3), (C.c_int32 * 2)(2, 1), (C.c_int32 * 4)(0, 1, 2, N), (C.c_int32 * 2)(2, -1)
    p = L.ptr

    def refused(rc, match):
        assert rc != 0
        text = lib.mvd_last_error().decode()
        assert match in text, text

    # null pointers, sizes
    refused(lib.mvd_op_vertex_gather(ctx, None, idx4, 4, p(vf), None), "mvd_op_vertex_gather")
    refused(lib.mvd_op_vertex_gather(ctx, p(feats), None, 4, p(vf), None), "mvd_op_vertex_gather")
    refused(lib.mvd_op_vertex_gather(ctx, p(feats), idx4, 4, None, None), "mvd_op_vertex_gather")
    refused(lib.mvd_op_vertex_gather(ctx, p(feats), idx4, 0, p(vf), None), "mvd_op_vertex_gather")
    refused(lib.mvd_op_vertex_gather(None, p(feats), idx4, 4, p(vf), None), "null context")
    refused(lib.mvd_op_latent_gather(ctx, None, p(vol_out), None), "mvd_op_latent_gather")
    refused(lib.mvd_op_latent_gather(ctx, p(rows), None, None), "mvd_op_latent_gather")
    refused(lib.mvd_op_latent_gather(None, p(rows), p(vol_out), None), "null context")
    refused(lib.mvd_op_frustum_gather(ctx, None, idx2, 2, D, S, p(out), None), "mvd_op_frustum_gather")
    refused(lib.mvd_op_frustum_gather(ctx, p(vol), None, 2, D, S, p(out), None), "mvd_op_frustum_gather")
    refused(lib.mvd_op_frustum_gather(ctx, p(vol), idx2, 2, D, S, None, None), "mvd_op_frustum_gather")
    refused(lib.mvd_op_frustum_gather(ctx, p(vol), idx2, 2, D, 1, p(out), None), "mvd_op_frustum_gather")
    refused(lib.mvd_op_frustum_gather(ctx, p(vol), idx2, 0, D, S, p(out), None), "mvd_op_frustum_gather")
    refused(lib.mvd_op_frustum_gather(None, p(vol), idx2, 2, D, S, p(out), None), "null context")
    # a view index outside the cameras of the active slot
    refused(lib.mvd_op_vertex_gather(ctx, p(feats), bad4, 4, p(vf), None), "view index")
    refused(lib.mvd_op_frustum_gather(ctx, p(vol), bad2, 2, D, S, p(out), None), "view index")
    # an empty slot: no mesh, no cameras; then a mesh without cameras
    eng.select_sample(5)
    try:
        refused(lib.mvd_op_vertex_gather(ctx, p(feats), idx4, 4, p(vf), None), "mvd_set_mesh")
        refused(lib.mvd_op_latent_gather(ctx, p(rows), p(vol_out), None), "mvd_set_mesh")
        refused(lib.mvd_op_frustum_gather(ctx, p(vol), idx2, 2, D, S, p(out), None), "mvd_set_cameras")
        eng.set_mesh(*R.mesh("v300"))
        refused(lib.mvd_op_vertex_gather(ctx, p(feats), idx4, 4, p(vf), None), "mvd_set_cameras")
    finally:
        eng.select_sample(0)
    torch.cuda.synchronize()
    for name, t in (("vertex", vf), ("latent", vol_out), ("frustum", out)):
        assert torch.isnan(t).all(), f"a refused {name} call wrote to its output"
    # and the same buffers are filled by calls that are not refused
    L.check(lib.mvd_op_vertex_gather(ctx, p(feats), idx4, 4, p(vf), None))
    L.check(lib.mvd_op_latent_gather(ctx, p(rows), p(vol_out), None))
    L.check(lib.mvd_op_frustum_gather(ctx, p(vol), idx2, 2, D, S, p(out), None))
    torch.cuda.synchronize()
    assert (vf == 0).all() and (vol_out == 0).all() and (out == 0).all()

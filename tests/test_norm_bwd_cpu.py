"""CPU: the closed forms of tests/norm_bwd_ref.py against torch.autograd in float64, on every shape family of
tests/test_gpu_norm_bwd_ops.py, and the shape tables against the launch plans they claim to reach."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_bwd_ref as R

TOL = 1e-12


def _act(y, act):
    return F.silu(y) if act == R.ACT_SILU else (torch.relu(y) if act == R.ACT_RELU else y)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", list(R.GN_CASES))
def test_group_norm_closed_forms_match_autograd(name, family):
    c, d = R.GN_CASES[name], R.gn_inputs(name, family)
    x, gamma, beta = [d[k].double().requires_grad_(True) for k in ("x", "gamma", "beta")]
    pre = None if d["pre"] is None else d["pre"].double().requires_grad_(True)
    v = x if pre is None else x + pre[:, None, :]
    y = _act(F.group_norm(v.transpose(1, 2), c["G"], gamma, beta, c["eps"]).transpose(1, 2), c["act"])
    fwd = R.gn_forward(d["x"], d["pre"], d["gamma"], d["beta"], c["G"], c["eps"], c["act"], torch.float64)
    assert max(R.errs(fwd, y.detach())) <= TOL
    y.backward(d["dy"].double())
    got = R.gn_backward(d["x"], d["pre"], d["dy"], d["gamma"], d["beta"], c["G"], c["eps"], c["act"], torch.float64)
    want = {"dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "dpre": x.grad.sum(dim=1) if pre is None else pre.grad}
    for k in want:
        assert max(R.errs(got[k], want[k])) <= TOL, (k, R.errs(got[k], want[k]))


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", list(R.LN_CASES))
def test_layer_norm_closed_form_matches_autograd(name, family):
    c, d = R.LN_CASES[name], R.ln_inputs(name, family)
    x, gamma = d["x"].double().requires_grad_(True), d["gamma"].double().requires_grad_(True)
    beta = torch.zeros(c["C"], dtype=torch.float64, requires_grad=True)
    F.layer_norm(x, (c["C"],), gamma, beta, c["eps"]).backward(d["dy"].double())
    got = R.ln_backward(d["x"], d["dy"], d["gamma"], c["eps"], torch.float64)
    for k, want in (("dx", x.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        assert max(R.errs(got[k], want)) <= TOL, (k, R.errs(got[k], want))


def test_reductions_match_autograd():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(3 * 17, 65, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(3, 65, generator=g, dtype=torch.float64)
    # d/dbias of sum(w * (bias broadcast over the rows of each sample)) is the per-sample column sum of the upstream gradient
    bias = torch.zeros(3, 65, dtype=torch.float64, requires_grad=True)
    ((bias[:, None, :] + 0 * v.reshape(3, 17, 65)) * v.detach().reshape(3, 17, 65)).sum().backward()
    assert max(R.errs(R.colsum(v.detach(), 3, torch.float64), bias.grad)) <= TOL
    assert max(R.errs(R.sum_rows(w, torch.float64), w.sum(0))) <= TOL
    # the weight gradient of y = a W^T over K rows is sum_k dy[k] (x) a[k]
    a, dy = torch.randn(3, 7, generator=g, dtype=torch.float64), torch.randn(3, 5, generator=g, dtype=torch.float64)
    W = torch.zeros(5, 7, dtype=torch.float64, requires_grad=True)
    ((a @ W.t()) * dy).sum().backward()
    assert max(R.errs(R.outer(dy, a, torch.float64), W.grad)) <= TOL


def test_accumulated_results_are_compared_as_what_was_added():
    start, term = torch.tensor([3.0, -1.5]), torch.tensor([1e-3, 2.0])
    assert torch.equal(R.added(start, term, torch.float64), (start.double() + term.double()) - start.double())
    assert R.added(start, term, torch.float32)[0].item() != 1e-3  # the float32 evaluation carries the rounding of its final add


def test_relu_cases_keep_clear_of_the_kink():
    for name, c in R.GN_CASES.items():
        if c["act"] != R.ACT_RELU:
            continue
        for family in R.FAMILIES:
            d = R.gn_inputs(name, family)
            u = R.gn_forward(d["x"], d["pre"], d["gamma"], d["beta"], c["G"], c["eps"], R.ACT_NONE, torch.float64)
            assert u.abs().min().item() >= 0.9 * R.RELU_MARGIN


def test_offset_family_is_offset():
    for name, c in R.GN_CASES.items():
        d = R.gn_inputs(name, "offset")
        v = d["x"] if d["pre"] is None else d["x"] + d["pre"][:, None, :]
        v = v.reshape(c["B"], c["rows"], c["G"], -1).double()
        mean = v.mean(dim=(1, 3))
        assert ((mean.abs() - 4).abs() < 0.5).all(), name
        if c["rows"] * c["C"] // c["G"] >= 64:
            assert ((v.std(dim=(1, 3)) - 0.5).abs() < 0.15).all(), name
        if d["pre"] is not None:  # half of the offset rides on the pre-add
            assert torch.equal(d["pre"].abs(), torch.full_like(d["pre"], 2.0))


def test_group_norm_table_reaches_the_plans_it_claims():
    plan = {n: R.gn_slabs(c["B"], c["G"], c["rows"]) for n, c in R.GN_CASES.items()}
    cases = R.GN_CASES
    assert plan["c64_empty"] == 64 and R.gn_empty_slabs(520, 64) == 6               # empty trailing slabs at the cap of 64
    assert plan["c2560_7"] == 1 and plan["c64_1"] == 1                              # rows below 16: one slab
    assert any(c["rows"] < 16 for c in cases.values())
    assert R.gn_empty_slabs(100, 64) == 14 and cases["c128_force64"]["S_force"] == 64
    assert {c["S_force"] for c in cases.values()} == {0, 1, 2, 64}
    assert cases["enc_100"]["rows"] < R.gn_row_lanes(16, 8) == 128                  # most row lanes idle
    assert {c["C"] // c["G"] for c in cases.values()} >= {2, 8, 16, 10, 30, 80, 256}
    assert {c["rows"] for c in cases.values()} >= {1, 7, 16, 17, 100, 520, 1024}
    assert {c["B"] for c in cases.values()} == {1, 3}
    assert {c["act"] for c in cases.values()} == {0, 1, 2}
    assert {c["eps"] for c in cases.values()} == {1e-5, 1e-6}
    assert {c["pre"] for c in cases.values()} == {None, "enc", "dense"}
    for key in ("strided", "accum", "poison", "fwd"):
        assert {c[key] for c in cases.values()} == {False, True}, key
    poisoned = {n for n, c in cases.items() if c["poison"]}
    assert {"c64_empty", "c2560_7", "enc_1024"} <= poisoned
    # the plan itself: never more than 64 slabs, never more than the workgroup budget allows, at least one
    for B in (1, 2, 3, 8):
        for G in (8, 32):
            for rows in (1, 7, 8, 15, 16, 17, 100, 520, 1024, 49152):
                S = R.gn_slabs(B, G, rows)
                assert 1 <= S <= 64 and (S == 1 or (S * 8 <= rows and S * B * G <= 1024))


def test_layer_norm_table_reaches_the_plans_it_claims():
    rows = {c["rows"] for c in R.LN_CASES.values()}
    assert rows == {1, 3, 4, 5, 1023, 1024, 1025, 2051}
    assert {c["C"] for c in R.LN_CASES.values()} == {64, 100, 320, 640, 1280}
    assert R.ln_blocks(1) == 1 and R.ln_blocks(4) == 1 and R.ln_blocks(5) == 2
    assert R.ln_blocks(1020) == 255 and R.ln_blocks(1023) == 256 and R.ln_blocks(1024) == 256 and R.ln_blocks(1025) == 256
    assert 1023 < 4 * 256 == 1024 < 1025 and R.ln_blocks(2051) == 256               # below, at, above: the grid-stride loop turns twice
    assert R.LN_REFUSED_C > 1280
    for key in ("strided", "accum", "poison"):
        assert {c[key] for c in R.LN_CASES.values()} == {False, True}, key
    assert {c["eps"] for c in R.LN_CASES.values()} == {1e-5, 1e-6}


def test_reduction_tables_hold_the_sizes_the_kernels_branch_on():
    assert set(R.COLSUM_ROWS) == {1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 200} and set(R.COLSUM_C) == {1, 48, 63, 64, 65, 130}
    jobs = [j for launch in R.SUM_ROWS_LAUNCHES for j in launch]
    assert [len(launch) for launch in R.SUM_ROWS_LAUNCHES] == [1, 2, 3, 4]
    assert {j[0] for j in jobs} == {1, 31, 32, 33, 257} and {j[1] for j in jobs} == {1, 7, 8, 9, 320}
    for launch in R.SUM_ROWS_LAUNCHES[1:]:
        cmax = max(j[1] for j in launch)
        assert any(-(-j[1] // 8) < -(-cmax // 8) for j in launch)                   # a job with workgroups that must return early
        assert {j[2] for j in launch} == {0, 1}                                     # mixed accum

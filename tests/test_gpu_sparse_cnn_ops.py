"""GPU: the sparse voxel CNN's kernels (csrc/k_cond.hip, k_cond_bwd.hip) one at a time, through the parity hooks mvd_op_sparse_conv,
mvd_op_bn_rows_relu, mvd_op_bn_rows_relu_bwd and mvd_op_sparse_conv_bwd, against the float64 reference tests/sparse_cnn_ref.py on the
production rule-book tables (tests/test_sparse_cnn_cpu.py holds the reference's index vectors against them).

Tolerances.  No constant: every compared tensor is also evaluated by the same reference function in float32 on the CPU, e32 is that
evaluation's error against float64, and the kernel's error must be at most FACTOR * max(e32, 2^-22) in relative L2 and in max error
over max reference alike.  The kernel and the float32 evaluation make the same number of roundings in a different order (wave-split
taps, 256-site chunks, tree sums): two draws of one random walk; four covers the order, the floor of four ulps covers tensors the
float32 evaluation happens to get almost exactly.  fp16 / bf16 operand rounding (3e-4) or a dropped term is thousands of times
larger.  The impulse cases and the bit-identity checks have tolerance 0.

Worst measured ratio kernel error / max(e32, 2^-22) per test (MI355X; the [parity] lines print every one):
  test_sparse_conv_forward                 1.87  (matrix-core subm1, full16, epilogue, max norm)
  test_sparse_conv_forward_other_channels  1.89  (matrix-core 64 -> 32, blob, raw, max norm)
  test_sparse_conv_backward                2.25  (matrix-core det=0 subm2, blob, d_in, max norm)
  test_bn_rows_relu_forward                1.00  (n = 2, C = 32, offset inputs, y)
  test_bn_rows_relu_backward               0.85  (n = 6145, C = 64, dbeta, max norm)
"""
import functools

import pytest
import torch

from morphablediffusion_amd import lib as L
from morphablediffusion_amd.engine import op_bn_rows_relu, op_bn_rows_relu_bwd, op_sparse_conv, op_sparse_conv_bwd
from tests import sparse_cnn_ref as R
from tests.test_sparse_cnn_cpu import engine_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 4.0, 2.0 ** -22
KINDS = [k[0] for k in R.LAYER_KINDS]


@functools.lru_cache(maxsize=None)
def production_tables(name):
    return engine_tables(R.point_set(name))[1]


def nbr_of(name, kind=None):
    if kind is None:
        return production_tables(name)[0]
    _, _, _, strided, lvl = R.KIND[kind]
    return production_tables(name)[3 + lvl if strided else lvl]


def check(label, gots, ref_fn, factor=FACTOR):
    """gots: {name: kernel result}; ref_fn(dtype) -> {name: reference}, or the pair (its float64 result, its float32 result).
    Prints every figure, then asserts the bound."""
    ref64, ref32 = ref_fn if isinstance(ref_fn, tuple) else (ref_fn(torch.float64), ref_fn(torch.float32))
    bad = []
    for name, got in gots.items():
        assert torch.isfinite(got).all(), f"{label} {name}: non-finite result"
        k, e = R.errs(got, ref64[name]), R.errs(ref32[name].double(), ref64[name])
        for norm, kk, ee in zip(("L2", "max"), k, e):
            ratio = kk / max(ee, FLOOR)
            print(f"[parity] {label} {name} {norm}: kernel {kk:.3e} e32 {ee:.3e} ratio {ratio:.2f}")
            if not kk <= factor * max(ee, FLOOR):
                bad.append((name, norm, kk, ee, ratio))
    assert not bad, f"{label}: {bad}"


def conv_refs(idx, x, w5, scale, shift):
    def fn(dt):
        raw = R.conv(x, idx, w5, dt)
        return {"raw": raw, "bn+relu": R.fold_epilogue(raw, scale, shift, dt)}
    return fn


def run_forward(name, form, layout, nbr, idx, x, w5, scale, shift, label):
    w = R.to_layout(w5, layout).to(DEV)
    gots = {"raw": op_sparse_conv(x.to(DEV), nbr, w, layout, form),
            "bn+relu": op_sparse_conv(x.to(DEV), nbr, w, layout, form, scale=scale, shift=shift)}
    check(label, gots, conv_refs(idx, x, w5, scale, shift))


# ---- forward convolution -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.POINT_SETS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["site", "mfma"])
def test_sparse_conv_forward(form, kind, name):
    """One production launch per form, layer kind and point set: the raw output of the train path and the folded BatchNorm + ReLU
    epilogue of the eval path; the weight goes in through the checkpoint packers in one of the three layouts."""
    ps = R.point_set(name)
    idx, x, w5, _, scale, shift = R.conv_data(ps, kind)
    layout = (KINDS.index(kind) + R.POINT_SETS.index(name)) % 3
    run_forward(name, form, layout, nbr_of(name, kind), idx, x, w5, scale, shift, f"conv fwd {form} {kind} {name} layout {layout}")


@pytest.mark.parametrize("name", ["blob", "tiny", "plus1"])
@pytest.mark.parametrize("form,cin,cout", [("mfma", ci, co) for ci, co in R.DGRAD_CHANNELS] + [("site", ci, co) for ci, co in R.SITE_CHANNELS])
def test_sparse_conv_forward_other_channels(form, cin, cout, name):
    """The channel counts of the gather-form data gradient (matrix-core kernel) and the site kernel's scalar branch (Cin % 8 != 0)
    and idle threads (256 % Cout != 0), on the level-0 table."""
    ps = R.point_set(name)
    idx, x, w5, _, scale, shift = R.conv_data(ps, cin=cin, cout=cout)
    run_forward(name, form, (cin + cout) % 3, nbr_of(name), idx, x, w5, scale, shift, f"conv fwd {form} {cin}->{cout} {name}")


@pytest.mark.parametrize("cin,cout", [(12, 20), (16, 48), (16, 64), (64, 16), (48, 48)])
def test_matrix_core_form_rejects_channel_counts_it_does_not_take(cin, cout):
    ps = R.point_set("tiny")
    idx, x, w5, d_out, _, _ = R.conv_data(ps, cin=cin, cout=cout)
    with pytest.raises(L.MvdError, match="matrix-core"):
        op_sparse_conv(x.to(DEV), nbr_of("tiny"), w5.to(DEV), 0, "mfma")
    with pytest.raises(L.MvdError, match="matrix-core"):
        op_sparse_conv_bwd(x.to(DEV), nbr_of("tiny"), d_out.to(DEV), w5.to(DEV), 0, "mfma")


# ---- impulse cases: every output element is one product or zero, so kernel == reference bit for bit ----------------------------------
HOT = 2.0


def hot_rows(ps, kind, out_side):
    """rows that carry the impulse: a border site, the representative of a duplicate (and, for a gradient, the duplicate itself) at
    level 0; the first and the last row elsewhere"""
    _, _, _, strided, lvl = R.KIND[kind]
    if lvl == 0 and not (strided and out_side):
        rows = [ps.border_row(), int(ps.rep[ps.dup_rows[len(ps.dup_rows) // 2]])]
        return rows + [int(ps.dup_rows[len(ps.dup_rows) // 2])] if out_side else rows
    n = ps.table(kind)[0].shape[0] if out_side else ps.table(kind)[1]
    return [0, n - 1]


def assert_same_bits(got, want, what):
    got = got.cpu().double()
    assert torch.equal(got != 0, want != 0), f"{what}: the footprint moved"
    assert (want != 0).any(), f"{what}: empty footprint, the case checks nothing"
    assert torch.equal(got, want), f"{what}: max diff {(got - want).abs().max().item():.3e}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["site", "mfma"])
def test_sparse_conv_forward_impulse_is_bit_exact(form, kind):
    ps = R.point_set("blob")
    _, cin, cout, _, _ = R.KIND[kind]
    idx, n_in = ps.table(kind)
    w5 = R.exact_weight(cout, cin)
    for row in hot_rows(ps, kind, out_side=False):
        x = torch.zeros(n_in, cin)
        x[row, cin - 3] = HOT
        got = op_sparse_conv(x.to(DEV), nbr_of("blob", kind), w5.to(DEV), 0, form)
        assert_same_bits(got, R.conv(x, idx, w5), f"{form} {kind} hot row {row}")


BWD_VARIANTS = [("site", False), ("mfma", False), ("mfma", True)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form,det", BWD_VARIANTS)
def test_sparse_conv_backward_impulse_is_bit_exact(form, det, kind):
    """A one-hot d_out row: d_in is one product per element (a wrong tap flip, transposed fragment or inverse-table row moves its
    footprint), and so is the weight gradient."""
    ps = R.point_set("blob")
    _, cin, cout, strided, lvl = R.KIND[kind]
    idx, n_in = ps.table(kind)
    w5 = R.exact_weight(cout, cin)
    x = R.conv_data(ps, kind)[1]
    for row in hot_rows(ps, kind, out_side=True):
        d_out = torch.zeros(idx.shape[0], cout)
        d_out[row, cout - 5] = HOT
        d_in, gw = op_sparse_conv_bwd(x.to(DEV), nbr_of("blob", kind), d_out.to(DEV), w5.to(DEV), 0, form, strided=strided,
                                      level0_subm=(kind == "subm0"), deterministic=det)
        want_din, want_dw = R.conv_grads(x, idx, w5, d_out)
        assert_same_bits(d_in, want_din, f"{form} det={det} {kind} hot row {row}: d_in")
        assert_same_bits(gw, want_dw, f"{form} det={det} {kind} hot row {row}: dW")


# ---- backward convolution ----------------------------------------------------------------------------------------------------------
def run_backward(name, kind, form, det, layout, x, w5, d_out, prefill, poison):
    _, _, _, strided, _ = R.KIND[kind]
    return op_sparse_conv_bwd(x.to(DEV), nbr_of(name, kind), d_out.to(DEV), R.to_layout(w5, layout).to(DEV), layout, form, strided=strided,
                              level0_subm=(kind == "subm0"), deterministic=det, grad_w=R.to_layout(prefill, layout), poison=poison)


@pytest.mark.parametrize("name", R.POINT_SETS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form,det", BWD_VARIANTS)
def test_sparse_conv_backward(form, det, kind, name):
    """d_in (from NaN: the gather form writes every element, duplicates' rows exactly 0) and the weight gradient, added to a
    pre-filled buffer in each of the three layouts, against float64 autograd; clean and with the hook's scratch poisoned."""
    ps = R.point_set(name)
    _, cin, cout, strided, lvl = R.KIND[kind]
    idx, x, w5, d_out, _, _ = R.conv_data(ps, kind)
    g = torch.Generator().manual_seed(11)
    prefill = torch.randn(w5.shape, generator=g) * (0.5 * d_out.shape[0] ** 0.5)  # about half the gradient's own scale
    # atomics: the level-0 fold of the non-deterministic matrix-core form (only with duplicates), the site form's data gradient
    fold_atomic = form == "mfma" and not det and kind == "subm0" and ps.dup_rows.numel() > 0

    def refs(dt):  # the float32 evaluation adds to the pre-filled buffer in float32, as the kernel does
        d_in, dw = R.conv_grads(x, idx, w5, d_out, dt)
        return {"d_in": d_in, "dW added": (prefill.to(dt) + dw).double() - prefill.double()}

    ref64, ref32 = refs(torch.float64), refs(torch.float32)
    for layout in range(3):
        d_in, gw = run_backward(name, kind, form, det, layout, x, w5, d_out, prefill, False)
        d_in_p, gw_p = run_backward(name, kind, form, det, layout, x, w5, d_out, prefill, True)
        assert torch.isfinite(d_in).all() and torch.isfinite(d_in_p).all(), "an element of d_in was not written"
        assert torch.isfinite(gw_p).all()
        if lvl == 0 and ps.dup_rows.numel():
            assert (d_in[ps.dup_rows.to(DEV)] == 0).all() and (d_in_p[ps.dup_rows.to(DEV)] == 0).all(), "a duplicate's row is not exactly 0"
        if not fold_atomic:
            assert torch.equal(gw, gw_p), "poisoned scratch changed the weight gradient"
            if form == "mfma":
                assert torch.equal(d_in, d_in_p), "poisoned scratch changed the data gradient"
        added = gw.cpu().double() - R.to_layout(prefill, layout).double()
        in_layout = tuple({"d_in": r["d_in"], "dW added": R.to_layout(r["dW added"], layout)} for r in (ref64, ref32))
        assert added.shape == in_layout[0]["dW added"].shape
        check(f"conv bwd {form} det={int(det)} {kind} {name} layout {layout}", {"d_in": d_in, "dW added": added}, in_layout)


@pytest.mark.parametrize("kind", KINDS)
def test_deterministic_backward_repeats_bit_for_bit(kind):
    ps = R.point_set("blob")
    idx, x, w5, d_out, _, _ = R.conv_data(ps, kind)
    prefill = torch.zeros_like(w5)
    a = run_backward("blob", kind, "mfma", True, 0, x, w5, d_out, prefill, False)
    b = run_backward("blob", kind, "mfma", True, 0, x, w5, d_out, prefill, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- BatchNorm + ReLU --------------------------------------------------------------------------------------------------------------
def bn_forward_outputs(x, gamma, beta, rmean, rvar, inplace):
    y, stats, run = op_bn_rows_relu(x.to(DEV), gamma, beta, running=(rmean, rvar), inplace=inplace)
    return {"y": y, "mean": stats[0], "rstd": stats[1], "running mean": run[0], "running var": run[1]}


@pytest.mark.parametrize("n,C,offset", R.BN_FWD_CASES)
def test_bn_rows_relu_forward(n, C, offset):
    """n on both sides of the 256-thread stride and of the <24>, <48> and looped selections; offset: 50 + 0.1 randn, which a
    one-pass E[x^2] - mean^2 variance would lose.  y, [mean | rstd], the running statistics from non-trivial values; in place and
    out of place."""
    x, gamma, beta, rmean, rvar, _ = R.bn_data(n, C, offset)

    def refs(dt):
        y, stats, run = R.bn_relu(x, gamma, beta, dt, running=(rmean, rvar))
        return {"y": y, "mean": stats[0], "rstd": stats[1], "running mean": run[0], "running var": run[1]}

    out = bn_forward_outputs(x, gamma, beta, rmean, rvar, False)
    inp = bn_forward_outputs(x, gamma, beta, rmean, rvar, True)
    for k in out:
        assert torch.equal(out[k], inp[k]), f"{k}: in place differs from out of place"
    check(f"bn fwd n={n} C={C} offset={offset}", out, refs)


@pytest.mark.parametrize("n,C", [(255, 16), (6144, 32), (12288, 64)])
def test_bn_register_form_equals_looped_form_per_op(n, C, monkeypatch):
    x, gamma, beta, rmean, rvar, _ = R.bn_data(n, C, 1)
    reg = bn_forward_outputs(x, gamma, beta, rmean, rvar, False)
    monkeypatch.setenv("MVD_BN_LOOP", "1")
    loop = bn_forward_outputs(x, gamma, beta, rmean, rvar, False)
    for k in reg:
        assert torch.equal(reg[k], loop[k]), k


@pytest.mark.parametrize("n,C", R.BN_BWD_CASES)
def test_bn_rows_relu_backward(n, C):
    """n on both sides of the 128-row chunk; stats from the forward hook on the same x; dy is 0 where the float64 pre-activation is
    within 1e-4 of the ReLU's kink, so the mask the kernel re-derives in fp32 cannot differ where it matters."""
    x, gamma, beta, _, _, dy = R.bn_data(n, C)
    dy, _ = R.mask_near_ties(x, gamma, beta, dy)
    g = torch.Generator().manual_seed(n + C)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    stats = op_bn_rows_relu(x.to(DEV), gamma, beta)[1]
    clean = op_bn_rows_relu_bwd(x.to(DEV), dy, stats, gamma, beta, accum=(dg0, db0))
    poisoned = op_bn_rows_relu_bwd(x.to(DEV), dy, stats, gamma, beta, accum=(dg0, db0), poison=True)
    for u, v in zip(clean, poisoned):
        assert torch.equal(u, v), "poisoned scratch changed the result"

    def refs(dt):
        dx, dg, db = R.bn_relu_grads(x, gamma, beta, dy, dt)
        return {"d xraw": dx, "dgamma added": (dg0.to(dt) + dg).double() - dg0.double(), "dbeta added": (db0.to(dt) + db).double() - db0.double()}

    check(f"bn bwd n={n} C={C}", {"d xraw": clean[0], "dgamma added": clean[1].cpu().double() - dg0.double(),
                                  "dbeta added": clean[2].cpu().double() - db0.double()}, refs)


def test_bn_backward_rejects_a_channel_count_that_does_not_divide_256():
    x, gamma, beta, _, _, dy = R.bn_data(40, 48)
    stats = R.bn_relu(x, gamma, beta)[1].float()
    dev = [t.to(DEV) for t in (x, dy, stats, gamma, beta)]
    dg = torch.full((48,), 3.0, device=DEV)
    db = torch.full((48,), -2.0, device=DEV)
    keep = dev[1].clone()
    lib = L.load()
    rc = lib.mvd_op_bn_rows_relu_bwd(L.ptr(dev[0]), L.ptr(dev[1]), 40, 48, L.ptr(dev[3]), L.ptr(dev[4]), L.ptr(dev[2]), 0, L.ptr(dg), L.ptr(db),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"divide 256" in lib.mvd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dev[1], keep) and (dg == 3.0).all() and (db == -2.0).all()

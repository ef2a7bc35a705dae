"""GPU: the training backward's norms and row reductions (csrc/k_bwd.hip) in the forms the training step launches them in, through
mvd_op_group_norm_bwd_ex, mvd_op_group_norm_fwd32, mvd_op_layer_norm_bwd_ex (gn_backward / gn_forward32 / ln_backward themselves) and
mvd_op_train_colsum / _sum_rows / _outer_add, against the float64 closed forms of tests/norm_bwd_ref.py (tests/test_norm_bwd_cpu.py
holds those against torch.autograd and the shape tables against the launch plans).

Inputs come in two families.  "centred": the draw of tests/test_gpu_train_ops.py, x ~ 1.3 N(0,1) + 0.2.  "offset": x ~ 0.5 N(0,1) + m
with m = +-4 per (sample, group) -- per row for LayerNorm --, |mean| / std = 8, as a FiLM pre-add leaves a group; with a pre-add, half
of m rides on it.

Tolerances.  No constant (the rule of tests/test_gpu_sparse_cnn_ops.py): every compared tensor is also evaluated by the same closed
form in float32 on the CPU, e32 is that evaluation's error against float64, and the kernel's error must be at most
FACTOR * max(e32, 2^-22), FACTOR = 4, in relative L2 and in max error over max reference alike.  A result that is added to is
compared as got - preset, against what the float32 evaluation of preset + result adds.  The 16-bit column sum rounds its source on
both sides.  Two calls on the same input (the second with the workspace poisoned where the case says so) must agree bit for bit.

Worst measured ratio kernel error / max(e32, 2^-22) per test (MI355X; the [parity] lines print every one):
  test_group_norm_backward    1.97  (one-block form, c2560_7, offset, dgamma, max norm); slabbed form 1.42 (c960_16, centred, dx, max
                                    norm), on the offset family 1.14 (c64_1, dbeta, max norm)
  test_group_norm_forward32   1.06  (c2560_7, offset, max norm)
  test_layer_norm_backward    1.21  (r1023_c1280, centred, dgamma, max norm)
  test_colsum_samples         0.76  (B = 3, fp32, rows 65, C 48, max norm)
  test_sum_rows_multi         0.76  (three jobs, R 33, C 320, accum, max norm)
  test_outer_add              0.41  (1280 x 320 x 2, max norm)
Before the slab statistics were taken about a pivot (raw fp32 sums of v and v^2, E[v^2] - E[v]^2), the slabbed form measured 34.96
on the offset family (c64_1, dx, max norm; seven of its thirteen cases above 4) and the fp32 forward 21.96 (c2560_7); the centred
family (1.34) and the one-block form (1.97) were as they are now.
"""
import pytest
import torch

from morphablediffusion_amd import lib as L
from tests import norm_bwd_ref as R

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2.0 ** -22
OPD = torch.bfloat16 if L.DTYPE == "bf16" else torch.float16


@pytest.fixture(scope="module")
def eng():
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig
    e = Engine(UNetConfig(model_channels=64), VolumeConfig(), workspace_gb=2.0)
    yield e
    e.close()


def check(label, gots, ref64, ref32):
    """gots: {name: kernel result}; ref64 / ref32: {name: reference} in the two precisions.  Prints every figure, then asserts."""
    bad = []
    for name, got in gots.items():
        assert torch.isfinite(got).all(), f"{label} {name}: non-finite result"
        k, e = R.errs(got, ref64[name]), R.errs(ref32[name].double(), ref64[name])
        for norm, kk, ee in zip(("L2", "max"), k, e):
            ratio = kk / max(ee, FLOOR)
            print(f"[parity] {label} {name} {norm}: kernel {kk:.3e} e32 {ee:.3e} ratio {ratio:.2f}")
            if not kk <= FACTOR * max(ee, FLOOR):
                bad.append((name, norm, kk, ee, ratio))
    assert not bad, f"{label}: {bad}"


def same_bits(label, a, b):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{label} {k}: two calls on the same input differ"


def minus(got, start):
    """what the kernel added to `start`, the difference taken exactly"""
    return got.double().cpu() - start.double()


# ---- GroupNorm backward -------------------------------------------------------------------------------------------------------------
def gn_strides(c):
    C = c["C"]
    return dict(ld=C + 8, x_off=3, ldy=0, lddx=C + 24) if c["strided"] else {}


def run_gn_backward(eng, name, family, form, poison):
    c, d = R.GN_CASES[name], R.gn_inputs(name, family)
    kw = dict(form=form, S_force=c["S_force"], poison=poison, **gn_strides(c))
    if c["pre"] == "enc":    # block i = 1 of the view encoder: columns 16 .. 31 of the [B][48] FiLM rows and of their gradient
        kw.update(pre=d["pre"], pld=48, pre_off=16, want_dpre=True, ldp=48, dpre_off=16)
    elif c["pre"] == "dense":
        kw.update(pre=d["pre"], want_dpre=True)
    if c["accum"]:
        kw.update(accum=(d["dx0"], d["dg0"], d["db0"]))
    r = eng.op_group_norm_bwd_ex(d["x"], d["dy"], c["G"], d["gamma"], d["beta"], c["eps"], c["act"], **kw)
    want_S = 1 if form == 1 else (c["S_force"] or R.gn_slabs(c["B"], c["G"], c["rows"]))
    assert r.S_used == want_S, (r.S_used, want_S)
    out = {"dx": r.dx, "dgamma": r.dgamma, "dbeta": r.dbeta}
    if c["pre"]:
        out["dpre"] = r.dpre
    return out


@pytest.mark.parametrize("form", [0, 1], ids=["slabbed", "one_block"])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", list(R.GN_CASES))
def test_group_norm_backward(eng, name, family, form):
    """gn_backward's launch sequence per form: each form against the bound on its own, never against the other."""
    c, d = R.GN_CASES[name], R.gn_inputs(name, family)
    first = run_gn_backward(eng, name, family, form, False)
    again = run_gn_backward(eng, name, family, form, c["poison"])
    same_bits(f"GroupNorm backward {name} {family} form {form}", first, again)
    gots = {k: v.cpu() for k, v in first.items()}
    if c["accum"]:
        gots.update(dx=minus(first["dx"], d["dx0"]), dgamma=minus(first["dgamma"], d["dg0"]), dbeta=minus(first["dbeta"], d["db0"]))
    check(f"GroupNorm backward {name} {family} form {form}", gots, R.gn_reference(name, family, torch.float64),
          R.gn_reference(name, family, torch.float32))


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", [n for n, c in R.GN_CASES.items() if c["fwd"]])
def test_group_norm_forward32(eng, name, family):
    """gn_forward32 (gn_slab_stats + gn_slab_fwd): the fp32 forward of the DepthTransformer's re-computation; no pre-add in this form"""
    c, d = R.GN_CASES[name], R.gn_inputs(name, family)
    C = c["C"]
    x = d["x"] if d["pre"] is None else d["x"] + d["pre"][:, None, :]   # this form has no pre-add: the whole offset is in x
    kw = dict(ld=C + 8, x_off=3, ldy=C + 24) if c["strided"] else {}
    ys = []
    for poison in (False, c["poison"]):
        y, S = eng.op_group_norm_fwd32(x, c["G"], d["gamma"], d["beta"], c["eps"], c["act"], S_force=c["S_force"], poison=poison, **kw)
        assert S == (c["S_force"] or R.gn_slabs(c["B"], c["G"], c["rows"]))
        ys.append(y)
    same_bits(f"GroupNorm forward32 {name} {family}", {"y": ys[0]}, {"y": ys[1]})
    ref = [{"y": R.gn_forward(x, None, d["gamma"], d["beta"], c["G"], c["eps"], c["act"], dt)} for dt in (torch.float64, torch.float32)]
    check(f"GroupNorm forward32 {name} {family}", {"y": ys[0].cpu()}, *ref)


@pytest.mark.parametrize("C,groups,kw,text", [(64, 7, {}, "channels per group must divide C"), (4096, 8, {}, "channels per group must divide C"),
                                               (64, 8, dict(S_force=65), "bad argument"), (64, 8, dict(form=2), "bad argument")])
def test_group_norm_backward_refusals_leave_the_results_alone(eng, C, groups, kw, text):
    """the launcher's own refusals (C % G, more than 256 channels per group) and the hook's, before anything is launched"""
    g = torch.Generator().manual_seed(C)
    x, dy, gamma, beta = torch.randn(1, 3, C, generator=g), torch.randn(1, 3, C, generator=g), torch.ones(C), torch.zeros(C)
    with pytest.raises(L.MvdError, match=text) as info:
        eng.op_group_norm_bwd_ex(x, dy, groups, gamma, beta, 1e-5, 1, accum=(torch.randn(1, 3, C, generator=g), torch.ones(C), torch.ones(C)), **kw)
    assert info.value.results_untouched


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
def run_ln_backward(eng, name, family, poison):
    c, d = R.LN_CASES[name], R.ln_inputs(name, family)
    C = c["C"]
    kw = dict(ld=C + 8, x_off=3, ldy=C + 4, lddx=C + 24) if c["strided"] else {}
    if c["accum"]:
        kw.update(accum=(d["dx0"], d["dg0"], d["db0"]))
    r = eng.op_layer_norm_bwd_ex(d["x"], d["dy"], d["gamma"], c["eps"], poison=poison, **kw)
    assert r.nblk_used == R.ln_blocks(c["rows"])
    return {"dx": r.dx, "dgamma": r.dgamma, "dbeta": r.dbeta}


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", list(R.LN_CASES))
def test_layer_norm_backward(eng, name, family):
    c, d = R.LN_CASES[name], R.ln_inputs(name, family)
    first = run_ln_backward(eng, name, family, False)
    again = run_ln_backward(eng, name, family, c["poison"])
    same_bits(f"LayerNorm backward {name} {family}", first, again)
    gots = {k: v.cpu() for k, v in first.items()}
    if c["accum"]:
        gots.update(dx=minus(first["dx"], d["dx0"]), dgamma=minus(first["dgamma"], d["dg0"]), dbeta=minus(first["dbeta"], d["db0"]))
    check(f"LayerNorm backward {name} {family}", gots, R.ln_reference(name, family, torch.float64), R.ln_reference(name, family, torch.float32))


def test_layer_norm_backward_refuses_wide_rows(eng):
    """C = 1344 is past the 20 columns a lane keeps: the launcher's own refusal, and nothing written"""
    g = torch.Generator().manual_seed(0)
    C = R.LN_REFUSED_C
    x, dy, gamma = torch.randn(5, C, generator=g), torch.randn(5, C, generator=g), torch.ones(C)
    with pytest.raises(L.MvdError, match="bwd_layer_norm: C too large") as info:
        eng.op_layer_norm_bwd_ex(x, dy, gamma, 1e-5, accum=(torch.randn(5, C, generator=g), torch.zeros(C), torch.zeros(C)))
    assert info.value.results_untouched


# ---- reductions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_half", [False, True], ids=["fp32", "16bit"])
@pytest.mark.parametrize("B", [1, 3])
def test_colsum_samples(eng, B, src_half):
    """bwd_colsum_samples at every row count around its 16 row lanes and its four-deep unrolled loop (r + 48 < rows), and every width
    around its 64-channel slabs; every other shape with ld > C and the result inside wider rows (neighbours bit-exact)."""
    g = torch.Generator().manual_seed(7 + B)
    gots, ref64, ref32 = {}, {}, {}
    for i, rows in enumerate(R.COLSUM_ROWS):
        for j, C in enumerate(R.COLSUM_C):
            v = torch.randn(B * rows, C, generator=g) + 0.25
            if src_half:
                v = v.to(OPD).float()
            wide = (i + j) % 2 == 1
            first, again = [eng.op_train_colsum(v, B, src_half, **(dict(ld=C + 3, ldo=C + 5, out_off=2) if wide else {})) for _ in range(2)]
            key = f"rows {rows} C {C}"
            same_bits(f"colsum B={B} {key}", {"out": first}, {"out": again})
            gots[key], ref64[key], ref32[key] = first.cpu(), R.colsum(v, B, torch.float64), R.colsum(v, B, torch.float32)
    check(f"colsum B={B} {'16-bit' if src_half else 'fp32'}", gots, ref64, ref32)


@pytest.mark.parametrize("launch", range(len(R.SUM_ROWS_LAUNCHES)), ids=lambda i: f"{i + 1}job")
def test_sum_rows_multi(eng, launch):
    """bwd_sum_rows_multi: 1..4 jobs of different R / C in one launch, ldp > C, written and added-to results side by side"""
    g = torch.Generator().manual_seed(11 + launch)
    spec = R.SUM_ROWS_LAUNCHES[launch]
    parts = [torch.randn(Rr, C, generator=g) + 0.25 for Rr, C, _ in spec]
    starts = [torch.randn(C, generator=g) * 3 if acc else None for _, C, acc in spec]
    jobs = [(p, p.shape[1] + 3 + k, s) for k, (p, s) in enumerate(zip(parts, starts))]
    first, again = eng.op_train_sum_rows(jobs), eng.op_train_sum_rows(jobs)
    gots, ref64, ref32 = {}, {}, {}
    for k, (p, s) in enumerate(zip(parts, starts)):
        key = f"job {k} R {p.shape[0]} C {p.shape[1]} accum {int(s is not None)}"
        same_bits(f"sum_rows {key}", {"out": first[k]}, {"out": again[k]})
        r64, r32 = R.sum_rows(p, torch.float64), R.sum_rows(p, torch.float32)
        gots[key] = first[k].cpu() if s is None else minus(first[k], s)
        ref64[key], ref32[key] = (r64, r32) if s is None else (R.added(s, r64, torch.float64), R.added(s, r32, torch.float32))
    check(f"sum_rows launch of {len(spec)}", gots, ref64, ref32)


def test_sum_rows_multi_refuses_five_jobs(eng):
    p = torch.randn(4, 8)
    with pytest.raises(L.MvdError, match="1..4 jobs"):
        eng.op_train_sum_rows([(p, 8, None)] * 5)


@pytest.mark.parametrize("M,N,K", R.OUTER_SHAPES)
def test_outer_add(eng, M, N, K):
    """bwd_outer_add: the kernel always adds, so the target starts from random values; lda / ldb above the widths"""
    g = torch.Generator().manual_seed(M + N + K)
    a, b, start = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g), torch.randn(M, N, generator=g)
    first, again = [eng.op_train_outer_add(a, b, start, lda=M + 3, ldb=N + 5) for _ in range(2)]
    same_bits(f"outer_add {M}x{N}x{K}", {"out": first}, {"out": again})
    ref = [{"out": R.added(start, R.outer(a, b, dt), dt)} for dt in (torch.float64, torch.float32)]
    check(f"outer_add {M}x{N}x{K}", {"out": minus(first, start)}, *ref)

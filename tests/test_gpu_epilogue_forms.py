"""GPU: the forward kernels in the forms the default inference path and the first-stage model launch them in, one kernel family at
a time through the mvd_op_*_ex hooks, against the fp64 references of tests/epilogue_ref.py: every GemmArgs epilogue field (per-sample
bias, alpha, SiLU, no bias, fp16 / split output, fp16 residual, tap_shift), extended precision (ConvW::xp) and its producers,
deferred split-K and its GroupNorm / LayerNorm consumers, the GroupNorm folded into two GEMM passes, and the row softmax.

Every GEMM / conv case names the kernel family it is built to reach and asserts it with probe_config(1) / probe_report().

Extended precision, relL2 against fp64 of the unrounded operands (emulation: three fp32 products of the fp16 hi / lo parts in torch on
the CPU, tests/epilogue_ref.py; GPU: the [parity] lines of this file on an MI355X; plain: the same case without xp on the GPU):

  case                              family                        emulation  GPU xp     GPU plain
  linear K=320                      gemm_dma_kernel<64,0>         3.87e-07   3.37e-07   2.95e-04
  linear K=1280                     gemm_dma_kernel<64,0>         6.65e-07   6.36e-07   2.93e-04
  conv1x1 64->128 16x16             gemm_dma_kernel<64,0>         2.05e-07   1.92e-07   2.92e-04
  conv3x3 64->64 16x16              conv3_dma_kernel<128,16,16>   4.74e-07   4.54e-07   2.96e-04
  conv3x3 64->64 8x8                conv3_dma_kernel<128,8,8>     4.66e-07   4.46e-07   2.96e-04
  conv3x3 320->320 16x16            conv3x_kernel<5>              9.54e-07   9.57e-07   2.94e-04
  conv3x3 320->320 16x16            conv3_dma_kernel<128,16,16>   9.54e-07   9.57e-07   2.94e-04
  conv3x3 320->320 8x8              conv3x_kernel<5>              9.59e-07   9.61e-07   2.96e-04
  conv3x3 320->320 8x8              conv3_dma_kernel<128,8,8>     9.59e-07   9.61e-07   2.96e-04
  conv3x3 s2 padded 64->64 16x16    gemm_dma_kernel<64,0>         4.67e-07   4.41e-07   2.97e-04

(The emulation's error depends a little on the host's fp32 summation order: the test takes it from the machine it runs on.)
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import epilogue_ref as R
from tests.test_gpu_ops import MAX_N, REL_L2

pytestmark = pytest.mark.gpu

EXACT = 1e-6  # the bound of the existing identity tests: the arithmetic of these cases is exact, any index error is O(1)
FOUR_WAVE = os.environ.get("MVD_DENSE_BM") == "128"  # set by test_linear_forms_through_the_four_wave_tiles for its child process


@pytest.fixture(scope="module")
def eng():
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig
    e = Engine(UNetConfig(model_channels=64), VolumeConfig(), workspace_gb=2.0)
    yield e
    e.close()


def probed(eng, fn):
    """fn() with every launch booked by family: (result, the GEMM / conv families that ran)"""
    eng.probe_config(1)
    try:
        res = fn()
        rep = eng.probe_report()
    finally:
        eng.probe_config(0)
    fams = [d["family"] for d in rep if d["launches"] > 0 and not d["family"].startswith("(") and d["family"] != "splitk_reduce_kernel"]
    return res, fams, any(d["family"] == "splitk_reduce_kernel" and d["launches"] > 0 for d in rep)


def ran_on(fams, family):
    if FOUR_WAVE and family == "dense":
        family = "dense128"
    assert len(fams) == 1 and R.family_matches(fams[0], family), f"meant for {family} ({R.FAMILY[family]}), ran on {fams}"
    return fams[0]


def close(got, want, name, fam, rel=REL_L2, mx=MAX_N):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    rl2 = ((got - want).norm() / (want.norm() + 1e-300)).item()
    mxe = ((got - want).abs().max() / (want.abs().max() + 1e-300)).item()
    print(f"[parity] {name} on {fam}: relL2={rl2:.2e} maxnorm={mxe:.2e}")
    assert rl2 <= rel and mxe <= mx, f"{name} on {fam}: relL2={rl2:.3e} maxnorm={mxe:.3e}"
    return rl2


SPLIT_CARRIES = 2.0 ** -21  # hi + lo holds 22 bits of the fp32 value; the fp32 epilogue may add its terms in another order


def split_carries_the_fp32_result(name, fam, out, out32):
    """[hi | lo | hi] against the SAME launch with an fp32 result: hi alone is ~3e-4 away, so a `lo` block that is zero, negated,
    a neighbour's or in the wrong columns misses this by three orders of magnitude"""
    got, v = out.out.double().cpu(), out32.out.double().cpu()
    rl2 = ((got - v).norm() / v.norm()).item()
    mxe = ((got - v).abs().max() / v.abs().max()).item()
    hi_only = R.rel_l2(out.hi.float().cpu(), v)
    print(f"[parity] {name} on {fam}: hi + lo vs the fp32 result relL2={rl2:.2e} maxnorm={mxe:.2e} (hi alone {hi_only:.2e})")
    assert rl2 <= SPLIT_CARRIES and mxe <= SPLIT_CARRIES, f"{name} on {fam}: hi + lo is {rl2:.3e} / {mxe:.3e} from the fp32 result"
    assert hi_only > 50 * SPLIT_CARRIES, f"{name}: the values round to fp16 exactly -- the case does not test the lo block"


# ------------------------------------------------------------------------------------------------ exact epilogue arithmetic
def _linear_operands(rows, B, N, exact, seed=0):
    K = R.LINEAR_K
    if exact:
        return (R.binary(rows, K, seed=seed), R.ints64(N, K, seed=1), R.ints64(N, seed=2, span=47), R.ints64(B, N, seed=3, span=53),
                R.ints64(rows, N, seed=4, span=59))
    return (R.rnd(rows, K, seed=seed), R.rnd(N, K, seed=1, scale=K ** -0.5), R.rnd(N, seed=2), R.rnd(B, N, seed=3), R.rnd(rows, N, seed=4))


def _linear_case(eng, family, B, rps, N, rb_ld, exact, alpha=1.0, sk=0, form="all"):
    rows = B * rps
    a_half = family != "gather_f32"
    assert R.linear_family_ok(family, rows, R.LINEAR_K, N, a_half, rb_ld=rb_ld)
    a, w, bias, rb, res = _linear_operands(rows, B, N, exact)
    kw = dict(B=B, rowbias=rb, rb_ld=rb_ld, alpha=alpha, bias=bias, resid=res, a_half=a_half, force_splitk=sk or 1)  # 1: the kernel's own epilogue
    ref = dict(B=B, alpha=alpha, bias=bias, rowbias=rb, resid=res)
    if form == "no bias":          # a per-sample bias without a bias: the folded form's other entry
        kw.update(use_bias=False)
        ref.update(bias=None)
    elif form == "silu":
        kw.update(act=1)
        ref.update(act=1)
    elif form == "f16 resid":
        kw.update(resid_f16=True, ldr=N + 8)
        ref.update(resid=res.half())
    elif form == "f16 out":
        kw.update(out_f16=True, ldc=N + 16)
    elif form == "split out":
        kw.update(out_f16=True, out_split=True, ldc=3 * N + 8)
    elif form == "ldc":
        kw.update(ldc=N + 12, ldr=N + 4)
    out, fams, reduced = probed(eng, lambda: eng.op_linear_ex(a, w, **kw))
    fam = ran_on(fams, family)
    assert reduced == (sk > 1), "a forced split-K must go through splitk_reduce_kernel, and nothing else may"
    want = R.linear(a, w, **ref)
    name = f"linear {'exact' if exact else 'random'} B={B} rps={rps} N={N} alpha={alpha} sk={sk} {form}"
    if form == "split out":
        assert torch.equal(out.hi.view(torch.int16), out.third.view(torch.int16)), f"{name}: third block != first block"
    if exact:
        close(out.out, want, name, fam, rel=EXACT, mx=EXACT)
    elif form == "split out":
        close(out.out, want, name, fam)           # hi + lo: the fp16-operand bound of the product
        kw.update(out_f16=False, out_split=False, ldc=0)
        split_carries_the_fp32_result(name, fam, out, eng.op_linear_ex(a, w, **kw))
    else:
        close(out.out, want, name, fam)
    return out


@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("N,rb_ld", R.LINEAR_NS)
@pytest.mark.parametrize("B,rps", R.SAMPLE_GEOMETRIES)
@pytest.mark.parametrize("family", ["dense", "gather_f32"])
def test_linear_exact_per_sample_bias(eng, family, B, rps, N, rb_ld, alpha):
    """alpha * acc + bias + rowbias[sample] + resid with operands whose every product and sum is exact: a wrong sample, row or column
    index is an O(1) error.  alpha = 1 reaches the accumulator pre-load form where rps % 32 == 0, alpha = 0.5 never does."""
    _linear_case(eng, family, B, rps, N, rb_ld, exact=True, alpha=alpha)


FORMS = ["no bias", "silu", "f16 resid", "f16 out", "split out", "ldc"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,rps", [(16, 16), (6, 48), (3, 96)])
@pytest.mark.parametrize("family", ["dense", "gather_f32"])
def test_linear_exact_forms(eng, family, B, rps, form):
    _linear_case(eng, family, B, rps, 72, 80, exact=True, alpha=1.0 if form == "no bias" else 0.5, form=form)


@pytest.mark.parametrize("B,rps", R.SAMPLE_GEOMETRIES)
@pytest.mark.parametrize("family", ["dense", "gather_f32"])
def test_linear_exact_through_the_reduce_pass(eng, family, B, rps):
    """a forced split-K sends the epilogue through splitk_reduce_kernel (epilogue_vec4's sample index)"""
    _linear_case(eng, family, B, rps, 200, 208, exact=True, alpha=0.5, sk=2)


@pytest.mark.parametrize("bn", [96, 160])
def test_linear_forms_through_the_four_wave_tiles(bn):
    """gemm_dma_kernel<128, BN> forced for every plain dense launch (MVD_DENSE_BM / MVD_DENSE_BN, read once per process, hence the
    child process): the dense cases above must hold on the 128-row tiles, whose waves cover other rows of a sample."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-k", "test_linear_exact and dense"],
                       cwd=root, env=dict(os.environ, MVD_DENSE_BM="128", MVD_DENSE_BN=str(bn)), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("[parity] linear")]
    assert lines and all(f"gemm_dma_kernel<128x{bn}>" in l for l in lines), "the forced 128-row tiles were not used"
    worst = max(float(l.split("relL2=")[1].split()[0]) for l in lines)
    print(f"[parity] {len(lines)} exact linear cases on gemm_dma_kernel<128x{bn}>: worst relL2={worst:.2e}")


def _conv_operands(B, Cin, H, W, Cout, exact, k=3, Ho=None, Wo=None):
    Ho, Wo = Ho or H, Wo or W
    if exact:
        return (R.binary(B, Cin, H, W, seed=1), R.ints64(Cout, Cin, k, k, seed=1), R.ints64(Cout, seed=2, span=47),
                R.ints64(B, Cout, seed=3, span=53), R.ints64(B, Cout, Ho, Wo, seed=4, span=59))
    return (R.rnd(B, Cin, H, W, seed=1), R.rnd(Cout, Cin, k, k, seed=2, scale=(Cin * k * k) ** -0.5), R.rnd(Cout, seed=3),
            R.rnd(B, Cout, seed=4), R.rnd(B, Cout, Ho, Wo, seed=5))


def _conv_case(eng, case, exact, alpha=1.0, form="all", sk=0):
    name, B, Cin, H, W, Cout, a_half, stream, family = case
    out_f16 = form in ("f16 out", "split out")
    if family == "conv3x" and not R.conv_family_ok("conv3x", B, Cin, H, W, Cout, a_half, stream, out_f16=out_f16, alpha=alpha,
                                                  act=int(form == "silu"), out_split=form == "split out"):
        family = "halo"  # a form conv3x does not take falls to the LDS-halo kernel (conv3x_eligible)
    assert R.conv_family_ok(family, B, Cin, H, W, Cout, a_half, stream, out_f16=out_f16, alpha=alpha, act=int(form == "silu"),
                            out_split=form == "split out")
    x, w, bias, rb, res = _conv_operands(B, Cin, H, W, Cout, exact)
    kw = dict(rowbias=rb, rb_ld=Cout + 8, alpha=alpha, bias=bias, resid=res, a_half=a_half, conv3x=stream, force_splitk=sk or 1)
    ref = dict(alpha=alpha, bias=bias, rowbias=rb, resid=res)
    if form == "no bias":
        kw.update(use_bias=False)
        ref.update(bias=None)
    elif form == "silu":
        kw.update(act=1)
        ref.update(act=1)
    elif form == "f16 resid":
        kw.update(resid_f16=True)
        ref.update(resid=res.half())
    elif form == "f16 out":
        kw.update(out_f16=True, ldc=Cout + 8)
    elif form == "split out":
        kw.update(out_f16=True, out_split=True)
    out, fams, reduced = probed(eng, lambda: eng.op_conv_ex(x, w, **kw))
    fam = ran_on(fams, family)
    assert reduced == (sk > 1)
    want = R.conv(x, w, **ref)
    label = f"conv {'exact' if exact else 'random'} {name} alpha={alpha} sk={sk} {form}"
    if form == "split out":
        assert torch.equal(out.hi.view(torch.int16), out.third.view(torch.int16)), f"{label}: third block != first block"
    if exact:
        close(out.nchw, want, label, fam, rel=EXACT, mx=EXACT)
    else:
        close(out.nchw, want, label, fam)
        if form == "split out":
            kw.update(out_f16=False, out_split=False)
            split_carries_the_fp32_result(label, fam, out, eng.op_conv_ex(x, w, **kw))


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("case", R.CONV_CASES, ids=[c[0] for c in R.CONV_CASES])
def test_conv3_exact_per_sample_bias(eng, case, alpha):
    """3x3 convolutions with bias, per-sample bias and residual on conv3x (its own epilogue), the LDS-halo kernel (folded where a
    tile lies in one sample, per-row sample index where it straddles four), the dense tap-gather kernel and the fp32-source gather
    kernel.  (conv3x takes alpha = 1 only: at alpha = 0.5 its cases run on the halo kernel.)"""
    _conv_case(eng, case, exact=True, alpha=alpha)


@pytest.mark.parametrize("form", FORMS[:5])
@pytest.mark.parametrize("case", [R.CONV_CASES[1], R.CONV_CASES[4], R.CONV_CASES[5]], ids=lambda c: c[0])
def test_conv3_exact_forms(eng, case, form):
    _conv_case(eng, case, exact=True, alpha=1.0 if form == "no bias" else 0.5, form=form)


@pytest.mark.parametrize("case", [R.CONV_CASES[0], R.CONV_CASES[1], R.CONV_CASES[4]], ids=lambda c: c[0])
def test_conv3_exact_through_the_reduce_pass(eng, case):
    case = case[:2] + (128,) + case[3:]   # two 64-channel chunks to split
    _conv_case(eng, case, exact=True, alpha=1.0 if case[8] == "conv3x" else 0.5, sk=2)


@pytest.mark.parametrize("fold", [False, True])
def test_upsample_conv_exact_per_sample_bias(eng, fold):
    """nearest x2 + 3x3 with a per-sample bias and a residual on the output grid: fused into the tap gather (run_conv2d) and as the
    four parity-folded 2x2 convolutions in one launch (run_upconv2d), whose GEMM rows are input pixels"""
    B, Cin, H, W, Cout = 3, 64, 16, 16, 72
    x, w, bias, rb, res = _conv_operands(B, Cin, H, W, Cout, exact=True, Ho=2 * H, Wo=2 * W)
    out, fams, _ = probed(eng, lambda: eng.op_conv_ex(x, w, bias, upsample=1, up_fold=fold, rowbias=rb, rb_ld=Cout + 4, alpha=0.5,
                                                      resid=res, a_half=True, conv3x=False))
    want = R.conv(x, w, upsample=1, alpha=0.5, bias=bias, rowbias=rb, resid=res)
    close(out.nchw, want, f"upsample conv exact fold={fold}", ran_on(fams, "dense"), rel=EXACT, mx=EXACT)


# ---------------------------------------------------------------------------------------------------- random-operand parity
@pytest.mark.parametrize("form", ["all"] + FORMS)
@pytest.mark.parametrize("B,rps", [(6, 48), (3, 96)])
@pytest.mark.parametrize("family", ["dense", "gather_f32"])
def test_linear_random_forms(eng, family, B, rps, form):
    _linear_case(eng, family, B, rps, 200, 208, exact=False, alpha=1.0 if form in ("no bias", "all") else 0.5, form=form)


def test_linear_random_split_out_through_the_scalar_epilogue(eng):
    """per-sample rows that are not 16-byte aligned (rb_ld % 4 != 0) keep a GEMM off the LDS-DMA kernel and off every vector
    epilogue: igemm_epilogue_store writes hi, lo and the copy one element at a time"""
    _linear_case(eng, "gather_f16", 6, 48, 200, 201, exact=False, alpha=0.5, form="split out")
    _linear_case(eng, "gather_f32", 3, 96, 72, 73, exact=False, alpha=0.5, form="split out")


@pytest.mark.parametrize("form", ["all"] + FORMS[:5])
@pytest.mark.parametrize("case", R.CONV_CASES, ids=[c[0] for c in R.CONV_CASES])
def test_conv3_random_forms(eng, case, form):
    _conv_case(eng, case, exact=False, alpha=1.0 if form in ("no bias", "all") else 0.5, form=form)


# -------------------------------------------------------------------------------------------------------------- tap_shift
TAP_B, TAP_C = 4, 64


def _tap_family(H, W, source):
    if source == "fp32":
        return "gather_f32"
    return "dense" if TAP_B * (H // 2) * (W // 2) >= R.DENSE_MIN_M else "gather_f16"


@pytest.mark.parametrize("source", ["fp32", "xp"])
@pytest.mark.parametrize("H,W", R.TAP_SHIFT_SHAPES)
def test_tap_shift_impulse_in_the_last_row_and_column(eng, H, W, source):
    """The first-stage encoder's Downsample pads on the right and bottom only: impulses in the last row and the last column must
    reproduce F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2) exactly (a symmetric padding, or a tap_shift that is dropped, moves them
    by one tap)."""
    family = _tap_family(H, W, source)
    assert R.conv_family_ok(family, TAP_B, TAP_C, H, W, TAP_C, False, False, xp=source == "xp", stride=2)
    x = torch.zeros(TAP_B, TAP_C, H, W)
    for b in range(TAP_B):
        x[b, (5 * b + 3) % TAP_C, H - 1, (b * 3) % W] = 1.0
        x[b, (7 * b + 11) % TAP_C, (b * 5 + 1) % H, W - 1] = 2.0
        x[b, b, H - 1, W - 1] = 1.0
    w, bias = R.ints64(TAP_C, TAP_C, 3, 3, seed=1), R.ints64(TAP_C, seed=2, span=47)
    out, fams, _ = probed(eng, lambda: eng.op_conv_ex(x, w, bias, stride=2, tap_shift=1, a_half=False, xp=source == "xp", conv3x=False))
    fam = ran_on(fams, family)
    want = R.conv(x, w, tap_shift=1, bias=bias)
    assert not torch.equal(want, R.conv(x, w, stride=2, bias=bias)), "the impulses do not tell the two paddings apart"
    close(out.nchw, want, f"tap_shift impulse {H}x{W} {source}", fam, rel=EXACT, mx=EXACT)


@pytest.mark.parametrize("H,W", R.TAP_SHIFT_SHAPES)
def test_tap_shift_random(eng, H, W):
    x, w, bias, _, _ = _conv_operands(TAP_B, TAP_C, H, W, TAP_C, exact=False)
    out, fams, _ = probed(eng, lambda: eng.op_conv_ex(x, w, bias, stride=2, tap_shift=1, a_half=False, conv3x=False))
    close(out.nchw, R.conv(x, w, tap_shift=1, bias=bias), f"tap_shift random {H}x{W}", ran_on(fams, "gather_f32"))


def test_tap_shift_refuses_what_the_encoder_never_runs(eng):
    from morphablediffusion_amd.lib import MvdError
    x, w = torch.zeros(1, 64, 7, 8), torch.zeros(64, 64, 3, 3)
    with pytest.raises(MvdError, match="even H and W"):
        eng.op_conv_ex(x, w, stride=2, tap_shift=1)
    with pytest.raises(MvdError, match="tap_shift"):
        eng.op_conv_ex(torch.zeros(1, 64, 8, 8), w, stride=1, tap_shift=1)


# ------------------------------------------------------------------------------------------------------ extended precision
def _xp_run(eng, name, family, xp):
    kind, p = R.XP_CASES[name]
    a, w = R.xp_operands(name)
    if kind == "linear":
        out, fams, _ = probed(eng, lambda: eng.op_linear_ex(a, w, a_half=True, xp=xp))
        return out.out, fams
    stride, ts = p[6], p[7]
    out, fams, _ = probed(eng, lambda: eng.op_conv_ex(a, w, stride=stride, tap_shift=ts, a_half=True, xp=xp, conv3x=family == "conv3x"))
    return out.nchw, fams


@pytest.mark.parametrize("name,family", [(n, f) for n in R.XP_CASES for f in R.XP_FAMILIES[n]])
def test_extended_precision(eng, name, family):
    """(a) within 2x the error of the CPU emulation of the same three products (the 2x: another fp32 summation order);
    (b) at least 20x below the same case without xp."""
    want, emu, _ = R.xp_reference(name)
    got, fams = _xp_run(eng, name, family, True)
    fam = ran_on(fams, family)
    plain, _ = _xp_run(eng, name, family, False)
    err, err_plain = R.rel_l2(got.cpu(), want), R.rel_l2(plain.cpu(), want)
    print(f"[parity] xp {name} on {fam}: relL2={err:.2e} emulation={emu:.2e} plain={err_plain:.2e} gain={err_plain / err:.0f}x")
    assert torch.isfinite(got).all()
    assert err <= 2 * emu, f"xp {name} on {fam}: {err:.3e} against fp64, the emulation reaches {emu:.3e}"
    assert err_plain >= 20 * err, f"xp {name} on {fam}: only {err_plain / err:.1f}x below the plain form ({err_plain:.3e})"


SPLIT_BOUND = 2e-6  # ~8 fp32 roundings of 2^-24 each per element, doubled; hi + lo itself carries 22 bits (2.4e-7)


@pytest.mark.parametrize("rows,C,lda", [(37, 320, 320), (130, 64, 72), (5, 8, 12)])
def test_rows_split_producer(eng, rows, C, lda):
    x = R.rnd(rows, C, seed=3) * 3.0
    hi, lo, third = eng.op_rows_split(x, lda=lda)
    assert torch.equal(hi.view(torch.int16), third.view(torch.int16)), "third block != first block"
    assert torch.equal(hi.cpu(), x.half()), "hi is not the fp16 rounding of the input"
    err = R.rel_l2((hi.float() + lo.float()).cpu(), x)
    print(f"[parity] rows_f32_to_f16_split {rows}x{C} lda={lda}: relL2={err:.2e}")
    assert err <= 2.0 ** -22, err


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("B,rows,C,G,act", [(2, 256, 64, 32, 1), (2, 64, 320, 32, 0), (1, 1024, 64, 32, 1)])
def test_group_norm_split_producers(eng, B, rows, C, G, act, split):
    """GroupNorm's [hi | lo | hi] output (split = 1) and its fp32 output (split = 2) against fp64: far below the fp16 floor"""
    x = R.rnd(B, rows, C, seed=7) * 2.0 + 0.7
    g, b = 1 + 0.1 * R.rnd(C, seed=1), 0.1 * R.rnd(C, seed=2)
    want, _ = R.group_norm(x[None], G, g, b, 1e-5, act)
    got, _ = eng.op_group_norm_ex(x, G, g, b, 1e-5, act, split=split, ldo=(3 * C + 8) if split == 1 else (2 * C + 8))
    assert torch.isfinite(got).all(), "third block != first block (or a non-finite value)"
    err = R.rel_l2(got.cpu(), want)
    print(f"[parity] group_norm split={split} B={B} rows={rows} C={C} act={act}: relL2={err:.2e}")
    assert err <= SPLIT_BOUND, err


# ---------------------------------------------------------------------------------------------------- deferred split-K
def _serial_sum(slabs, *terms):
    s = slabs[0].clone()
    for i in range(1, slabs.shape[0]):
        s += slabs[i]
    for t in terms:
        s = s + t
    return s


DEFER_LINEAR = dict(B=2, rows=256, K=512, N=128, sk=4)


def _defer_linear(eng, sk=None, cap_delta=0, **kw):
    d = DEFER_LINEAR
    sk = sk or d["sk"]
    K = max(d["K"], 64 * sk)
    a, w = R.rnd(d["rows"], K, seed=1), R.rnd(d["N"], K, seed=2, scale=K ** -0.5)
    bias, rb, res = R.rnd(d["N"], seed=3), R.rnd(d["B"], d["N"], seed=4), R.rnd(d["rows"], d["N"], seed=5)
    base = dict(bias=bias, B=d["B"], rowbias=rb, resid=res, a_half=True, force_splitk=sk)
    base.update(kw)
    plain = eng.op_linear_ex(a, w, **base)
    deferred = eng.op_linear_ex(a, w, defer_cap=sk * d["rows"] * d["N"] + cap_delta, defer_epilogue=True, **base)
    dev = plain.out.device
    return plain, deferred, (bias.to(dev), rb.to(dev).repeat_interleave(d["rows"] // d["B"], 0), res.to(dev))


def test_deferred_split_k_linear(eng):
    plain, deferred, terms = _defer_linear(eng)
    assert deferred.sk_used == DEFER_LINEAR["sk"] and deferred.out_untouched, (deferred.sk_used, deferred.out_untouched)
    total = _serial_sum(deferred.slabs, *terms)
    err = R.rel_l2(total.cpu(), plain.out.cpu())
    print(f"[parity] deferred split-K linear sk={deferred.sk_used}: slabs + bias + rowbias + resid vs the reduce pass relL2={err:.2e}")
    assert torch.equal(total, plain.out), "the slabs do not add up to what the reduce pass writes"


@pytest.mark.parametrize("case", [R.CONV_CASES[0], R.CONV_CASES[1], R.CONV_CASES[4]], ids=lambda c: c[0])
def test_deferred_split_k_conv(eng, case):
    _, B, _, H, W, Cout, a_half, stream, family = case
    Cin, sk = 320, 5
    x, w, bias, rb, res = _conv_operands(B, Cin, H, W, Cout, exact=False)
    kw = dict(bias=bias, rowbias=rb, resid=res, a_half=a_half, conv3x=stream, force_splitk=sk)
    plain, fams, _ = probed(eng, lambda: eng.op_conv_ex(x, w, **kw))
    fam = ran_on(fams, family)
    deferred, fams, reduced = probed(eng, lambda: eng.op_conv_ex(x, w, defer_cap=sk * plain.out.numel(), defer_epilogue=True, **kw))
    ran_on(fams, family)
    assert deferred.sk_used == sk and deferred.out_untouched and not reduced, (deferred.sk_used, deferred.out_untouched, reduced)
    dev = plain.out.device
    rows = plain.out.shape[0]
    total = _serial_sum(deferred.slabs, bias.to(dev), rb.to(dev).repeat_interleave(rows // B, 0), res.to(dev).permute(0, 2, 3, 1).reshape(rows, Cout))
    err = R.rel_l2(total.cpu(), plain.out.cpu())
    print(f"[parity] deferred split-K conv {case[0]} on {fam} sk={sk}: vs the reduce pass relL2={err:.2e}")
    assert torch.equal(total, plain.out)
    close(plain.nchw, R.conv(x, w, bias=bias, rowbias=rb, resid=res), f"conv {case[0]} sk={sk}", fam)


@pytest.mark.parametrize("why,kw", [
    ("capacity one float too small", dict(cap_delta=-1)),
    ("sk > MVD_DEFER_MAX", dict(sk=17)),
    ("fp16 residual", dict(resid_f16=True)),
    ("alpha != 1", dict(alpha=0.5)),
    ("fp16 output", dict(out_f16=True)),
])
def test_split_k_that_must_not_defer(eng, why, kw):
    plain, deferred, _ = _defer_linear(eng, **kw)
    assert deferred.sk_used == 1 and deferred.slabs is None and not deferred.out_untouched, f"{why}: the launch deferred"
    assert torch.equal(deferred.out, plain.out), f"{why}: `out` is not the finished result"
    print(f"[parity] must-not-defer ({why}): sk_used=1, out finished and equal to the run without a slab buffer")


# --------------------------------------------------------------------------------------------------- GroupNorm consumer
def _gn_case(eng, B, rows, C, G, nslab, opts, seed=0, act=1):
    x = R.rnd(nslab, B, rows, C, seed=seed) * (2.0 / nslab ** 0.5) + 0.3
    g, b = 1 + 0.1 * R.rnd(C, seed=1), 0.1 * R.rnd(C, seed=2)
    bias2 = R.rnd(C, seed=3) if "bias2" in opts else None
    pre = R.rnd(B, C, seed=4) if "preadd" in opts else None
    res = R.rnd(B, rows, C, seed=5) if "resid" in opts else None
    mat = "mat" in opts
    ld, ldo, ldr, ldm, pld = (C + 6 if "ld" in opts else 0), (C + 10 if "ldo" in opts else 0), (C + 2 if "ld" in opts else 0), \
        (C + 4 if "ldo" in opts else 0), (C + 8 if "ld" in opts else 0)
    assert R.gn_group_eligible(ld or C, rows, C, G, pld or C, ldo or C)
    got, m = eng.op_group_norm_ex(x, G, g, b, 1e-5, act, ld=ld, preadd=pre, pld=pld, bias2=bias2, resid=res, ldr=ldr, mat=mat, ldm=ldm,
                                  ldo=ldo)
    want, summed = R.group_norm(x, G, g, b, 1e-5, act, bias2=bias2, preadd=pre, resid=res)
    nt, me = R.gn_tile_of(rows, C, G)
    name = f"(expected) gn_group_kernel<{nt},{me},{nslab if nslab <= 4 else 0}>"
    close(got, want, f"group_norm slabs={nslab} B={B} rows={rows} C={C} G={G} {'+'.join(sorted(opts)) or 'bare'}", name)
    if mat:
        # every addition rounds once: |error| <= (additions) * 2^-24 * (sum of the magnitudes added)
        mag = x.double().abs().sum(0)
        for t in (bias2, None if pre is None else pre[:, None, :], res):
            if t is not None:
                mag = mag + t.double().abs()
        bound = (nslab + 3) * 2.0 ** -24 * mag
        worst = ((m.double().cpu() - summed).abs() / bound).max().item()
        print(f"[parity] group_norm mat slabs={nslab} on {name}: worst error / fp32 rounding bound = {worst:.2f}")
        assert worst <= 1.0, f"mat is {worst:.2f}x the fp32 rounding bound away from the sum"


@pytest.mark.parametrize("nslab", R.GN_NSLABS)
def test_group_norm_consumer_slab_counts(eng, nslab):
    """gn_group_kernel<..., NS>: NS = 2, 3, 4 and the run-time form (four slabs at a time, clamped index) at every count around its
    step of four -- a dropped or doubled slab is an O(1 / sqrt(nslab)) error in `mat` and in the result."""
    opts = [{"mat"}, {"bias2", "mat"}, {"preadd", "resid", "mat"}, {"bias2", "preadd", "resid", "mat", "ld", "ldo"}][nslab % 4]
    _gn_case(eng, 2, 64, 64, 8, nslab, opts | {"mat"}, seed=nslab)
    _gn_case(eng, 1, 100, 40, 4, nslab, {"bias2", "resid", "mat", "ld", "ldo"}, seed=nslab + 1, act=0)


@pytest.mark.parametrize("B,rows,C,G", R.GN_TILE_CASES, ids=lambda v: str(v))
def test_group_norm_consumer_register_tiles(eng, B, rows, C, G):
    _gn_case(eng, B, rows, C, G, 2, {"bias2", "preadd", "resid", "mat"}, seed=rows)
    _gn_case(eng, B, rows, C, G, 5, {"mat", "ld", "ldo"}, seed=rows + 1)


def test_group_norm_consumer_xcd_remainder(eng):
    B, rows, C, G = R.GN_REMAINDER_CASE
    assert (B * G) % 8 != 0
    _gn_case(eng, B, rows, C, G, 3, {"bias2", "preadd", "resid", "mat", "ld", "ldo"})
    _gn_case(eng, B, rows, C, G, 6, {"preadd", "mat"})


def test_group_norm_two_pass_form(eng):
    """form 1: the two-pass pair called directly -- one slab only, anything the single-pass kernel alone does is refused"""
    from morphablediffusion_amd.lib import MvdError
    B, rows, C, G = 2, 96, 64, 8
    x = R.rnd(1, B, rows, C, seed=2) + 0.5
    g, b, pre = 1 + 0.1 * R.rnd(C, seed=1), 0.1 * R.rnd(C, seed=2), R.rnd(B, C, seed=3)
    got, _ = eng.op_group_norm_ex(x, G, g, b, 1e-5, 1, form=1, preadd=pre, ld=C + 4, pld=C + 8, ldo=C + 12)
    want, _ = R.group_norm(x, G, g, b, 1e-5, 1, preadd=pre)
    close(got, want, "group_norm two-pass form with a pre-add", "(expected) gn_stats_kernel + gn_apply_kernel")
    with pytest.raises(MvdError, match="single-pass"):
        eng.op_group_norm_ex(R.rnd(2, B, rows, C), G, g, b, 1e-5, 1, form=1)
    with pytest.raises(MvdError, match="single-pass"):
        eng.op_group_norm_ex(x, G, g, b, 1e-5, 1, form=1, mat=True)


# --------------------------------------------------------------------------------------------------- LayerNorm consumer
@pytest.mark.parametrize("nslab", R.LN_NSLABS)
@pytest.mark.parametrize("rows,C,T", R.LN_CASES)
def test_layer_norm_consumer(eng, rows, C, T, nslab):
    """layernorm_vec_kernel<L, 5, SLABS> on the slabs a deferred GEMM left: `mat` must hold the bits the reduce pass of the same
    GEMM writes (k_norm.hip), `raw` its fp16 rounding, and the normalised rows the fp64 LayerNorm of it."""
    K, B = 320, rows // T
    assert rows % R.ln_rows_per_workgroup(C) and R.ln_rows_per_workgroup(C) % T and rows == B * T
    a, w = R.rnd(rows, K, seed=1), R.rnd(C, K, seed=2, scale=K ** -0.5)
    bias, rb, res = R.rnd(C, seed=3), R.rnd(B, C, seed=4), R.rnd(rows, C, seed=5)
    g, bt = 1 + 0.1 * R.rnd(C, seed=6), 0.1 * R.rnd(C, seed=7)
    kw = dict(bias=bias, B=B, rowbias=rb, resid=res, a_half=True, force_splitk=nslab)
    finished = eng.op_linear_ex(a, w, **kw)
    if nslab > 1:
        d = eng.op_linear_ex(a, w, defer_cap=nslab * rows * C, defer_epilogue=True, **kw)
        assert d.sk_used == nslab and d.out_untouched
        slabs = d.slabs
    else:
        slabs = eng.op_linear_ex(a, w, a_half=True, force_splitk=1).out[None]
    out, mat, raw = eng.op_layer_norm_slabs(slabs, g, bt, bias=bias, rowbias=rb, rb_ld=C + 8, T=T, resid=res, ldr=C + 4, raw=True,
                                            ld_raw=C + 8)
    name = f"(expected) layernorm_vec_kernel<{C // 40},5,slabs={nslab}>"
    if nslab > 1:
        same = torch.equal(mat, finished.out)
        print(f"[parity] layer_norm slabs={nslab} rows={rows} C={C} on {name}: mat bit-identical to the reduce pass: {same}")
        assert same, "mat differs from the finished result of the same GEMM at the same split"
    else:
        close(mat, finished.out, f"layer_norm slabs=1 rows={rows} C={C} mat", name, rel=1e-6, mx=1e-6)
    assert torch.equal(raw.view(torch.int16), mat.to(raw.dtype).view(torch.int16)), "raw is not the 16-bit rounding of mat"
    want, _ = R.layer_norm(mat.cpu()[None], g, bt)
    close(out, want, f"layer_norm slabs={nslab} rows={rows} C={C} T={T}", name)
    want_all, _ = R.layer_norm(slabs.cpu(), g, bt, bias=bias, rowbias=rb, T=T, resid=res)
    close(out, want_all, f"layer_norm slabs={nslab} rows={rows} C={C} T={T} (from the slabs)", name)


@pytest.mark.parametrize("rows,C", [(70, 320), (21, 1280), (9, 2560)])
def test_layer_norm_plain_with_raw_copy(eng, rows, C):
    x = R.rnd(rows, C, seed=1) * 3.0 - 0.5
    g, bt = 1 + 0.1 * R.rnd(C, seed=6), 0.1 * R.rnd(C, seed=7)
    out, mat, raw = eng.op_layer_norm_slabs(x, g, bt, plain=True, raw=True, ld_raw=C + 16)
    assert mat is None and torch.equal(raw.cpu(), x.to(raw.dtype)), "raw is not the 16-bit rounding of the input"
    close(out, R.layer_norm(x[None], g, bt)[0], f"layer_norm plain + raw rows={rows} C={C}", f"(expected) layernorm_vec_kernel<{C // 40},5>")


# ---------------------------------------------------------------------------------------------------- folded GroupNorm
FOLD_BOUND = 1e-5  # sqrt(8192) * 2^-24 ~ 5e-6 for the 256 x 32 values of a tile and group summed in fp32, doubled


@pytest.mark.parametrize("B,rps,K,N,cpg", R.FOLDED_GN_CASES)
def test_folded_group_norm(eng, B, rps, K, N, cpg):
    x, w = R.rnd(B * rps, K, seed=1) + 0.2, R.rnd(N, K, seed=2, scale=K ** -0.5)
    g, bt = 1 + 0.1 * R.rnd(N, seed=3), 0.1 * R.rnd(N, seed=4)
    (part, sc, sh, out), fams, _ = probed(eng, lambda: eng.op_folded_group_norm(x, w, cpg, g, bt, B))
    assert sorted(f[-3:] for f in fams) == [",1>", ",2>"] and all(f.startswith("gemm_dma_kernel<") for f in fams), fams
    G = N // cpg
    v16 = (x.half().double() @ w.half().double().t()).reshape(B, rps // 256, 256, G, cpg)
    s_err = ((part[..., 0].double().cpu() - v16.sum((2, 4))).abs() / v16.abs().sum((2, 4))).max().item()
    q_want = (v16 ** 2).sum((2, 4))
    q_err = ((part[..., 1].double().cpu() - q_want).abs() / q_want).max().item()
    print(f"[parity] folded group_norm partials B={B} rps={rps} N={N} cpg={cpg} on {sorted(fams)[0]}: sum/sum|v|={s_err:.2e} "
          f"sumsq rel={q_err:.2e} (bound {FOLD_BOUND:.0e}{', ABOVE HALF OF IT' if max(s_err, q_err) > FOLD_BOUND / 2 else ''})")
    assert s_err <= FOLD_BOUND and q_err <= FOLD_BOUND, (s_err, q_err)
    v = (x.double() @ w.double().t()).reshape(1, B, rps, N)
    want, _ = R.group_norm(v, G, g, bt, 1e-5, act=2)
    close(out.reshape(B, rps, N), want, f"folded group_norm B={B} rps={rps} N={N} cpg={cpg}", sorted(fams)[1])
    # scale / shift are the statistics' only other consumer: rstd * gamma, beta - mean * rstd * gamma
    mean = v[0].reshape(B, rps, G, cpg).mean((1, 3))
    var = v[0].reshape(B, rps, G, cpg).var((1, 3), unbiased=False)
    sc_want = (1.0 / torch.sqrt(var + 1e-5)).repeat_interleave(cpg, 1) * g.double()
    close(sc, sc_want, f"folded group_norm scale N={N} cpg={cpg}", "(expected) gn_finalize_kernel")
    close(sh, bt.double() - mean.repeat_interleave(cpg, 1) * sc_want, f"folded group_norm shift N={N} cpg={cpg}", "(expected) gn_finalize_kernel")


def test_folded_group_norm_refuses_what_the_engine_does_not_fold(eng):
    from morphablediffusion_amd.lib import MvdError
    g, bt = torch.ones(64), torch.zeros(64)
    with pytest.raises(MvdError, match="rps % 256"):
        eng.op_folded_group_norm(torch.zeros(2 * 384, 64), torch.zeros(64, 64), 8, g, bt, 2)
    with pytest.raises(MvdError, match="8 / 16 / 32"):
        eng.op_folded_group_norm(torch.zeros(512, 64), torch.zeros(64, 64), 4, g, bt, 2)


# --------------------------------------------------------------------------------------------------------- softmax rows
@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
def test_softmax_rows_f32(eng, cols):
    s = R.softmax_scores(cols)
    got, want = eng.op_softmax_rows(s, out_f32=True).double().cpu(), R.softmax(s)
    assert torch.isfinite(got).all()
    rl2 = ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()
    mxe = ((got - want).abs().max(1).values / want.max(1).values).max().item()
    print(f"[parity] softmax_rows_f32 cols={cols}: worst row relL2={rl2:.2e} maxnorm={mxe:.2e}")
    assert rl2 <= 1e-6 and mxe <= 1e-6, (rl2, mxe)


@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
def test_softmax_rows_f16(eng, cols):
    s = R.softmax_scores(cols)
    got, want = eng.op_softmax_rows(s, out_f32=False), R.softmax(s)
    assert got.dtype == torch.float16
    got = got.double().cpu()
    assert torch.isfinite(got).all()
    ulp = torch.exp2(torch.floor(torch.log2(want.clamp_min(2.0 ** -14))) - 10)  # fp16 spacing at `want` (subnormals: 2^-24)
    worst = ((got - want).abs() / ulp).max().item()
    sums = (got.sum(1) - 1).abs().max().item()
    print(f"[parity] softmax_rows (fp16) cols={cols}: worst error {worst:.2f} ulp, row sums within {sums:.1e} of 1")
    assert worst <= 1.0 and sums <= 1e-3, (worst, sums)


def test_softmax_rows_refuses_more_than_4096_columns(eng):
    from morphablediffusion_amd.lib import MvdError
    for f32 in (False, True):
        with pytest.raises(MvdError, match="4096"):
            eng.op_softmax_rows(torch.zeros(2, 4097), out_f32=f32)

"""GPU: conv3z (csrc/k_conv3x.hip), the plane-halo kernel of the 3x3x3 stride-1 layers of the two 3-D U-nets, one layer at a time
through mvd_op_conv3d_form (form 1: this kernel whatever the row count) against the fp64 reference of tests/epilogue_ref.py (conv3d).

The kernel computes output plane z as a 3x3 convolution over [in[z - 1] | in[z] | in[z + 1]]: one workgroup per 16 x 16 block of one
depth plane, the depth taps as extra 64-channel chunks, a plane outside the volume as zeros.  There is no z segment: every plane is
its own tile, so D = 1 (both depth neighbours outside), D = 2 (one outside for each plane) and D = 3 (a plane with both inside) are
the depth cases.  16 x 16 is one tile with every edge an image border, 32 x 16 / 16 x 32 have an interior tile edge in one dimension;
64 -> 64 is one channel chunk per depth tap on the 64-column tile, 128 -> 128 two chunks on the 128-column tile; B = 2 throughout
(sample stride: the last plane of sample 0 and the first of sample 1 are neighbours in memory and must not be in the sum).

Every case asserts the probe family and one launch without a reduce pass, runs with the free workspace poisoned, and has its guard
row and pad columns checked by the wrapper.  Exact cases (0 / 1 / 2 activations, k / 64 weights, bias and residual: every partial sum
exact in fp32) hold to 1e-6 and a 16-bit result is compared bit for bit; the random cases hold REL_L2 / MAX_N of tests/test_gpu_ops.py.
tests/test_conv3d_halo_cpu.py checks the routing predicate without a GPU.

The family each case ran on and its relL2 against fp64 (the [parity] lines of this file on an MI355X, fp16 library):

  test      case                                              family             relL2
  exact     64->64 1x16x16 bias                               conv3z_kernel<2>   0.00e+00
  exact     64->64 2x32x16 bias resid ldc                     conv3z_kernel<2>   0.00e+00
  exact     64->64 3x16x32 f16 out ldc                        conv3z_kernel<2>   0.00e+00
  exact     128->128 1x32x16 bias resid                       conv3z_kernel<4>   0.00e+00
  exact     128->128 2x16x16 f16 out resid ldc                conv3z_kernel<4>   0.00e+00
  exact     128->128 3x16x16 bias resid ldc                   conv3z_kernel<4>   0.00e+00
  routed    64->64 65x16x16 16640 rows (form 0)               conv3z_kernel<2>   0.00e+00
  routed    64->64 64x16x16 16384 rows (form 0)               gemm_dma_kernel<64,0>  0.00e+00
  random    64->64 3x32x16                                    conv3z_kernel<2>   1.54e-04
  random    128->128 2x16x16 f16 out                          conv3z_kernel<4>   2.48e-04
"""
import collections

import pytest
import torch

from morphablediffusion_amd import lib as L
from tests import epilogue_ref as R
from tests.test_gpu_epilogue_forms import EXACT, close
from tests.test_gpu_ops import MAX_N, REL_L2

pytestmark = pytest.mark.gpu
OPD = torch.bfloat16 if L.DTYPE == "bf16" else torch.float16
B = 2


@pytest.fixture(scope="module")
def eng():
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig
    e = Engine(UNetConfig(model_channels=64), VolumeConfig(), workspace_gb=2.0)
    yield e
    e.close()


def probed(eng, fn):
    """fn() with every launch booked by family: (result, {family: launches})"""
    eng.probe_config(1)
    try:
        res = fn()
        rep = eng.probe_report()
    finally:
        eng.probe_config(0)
    return res, {d["family"]: d["launches"] for d in rep if d["launches"] > 0 and not d["family"].startswith("(")}


Case = collections.namedtuple("Case", "name C dims bias resid out_f16 ldc_pad density span")
# a 16-bit result lowers the density and the span until the reference is representable in fp16 AND bfloat16 (asserted below)
CASES = [
    Case("64->64 1x16x16 bias", 64, (1, 16, 16), True, False, False, 0, 0.15, 61),
    Case("64->64 2x32x16 bias resid ldc", 64, (2, 32, 16), True, True, False, 8, 0.15, 61),
    Case("64->64 3x16x32 f16 out ldc", 64, (3, 16, 32), False, False, True, 8, 0.01, 5),
    Case("128->128 1x32x16 bias resid", 128, (1, 32, 16), True, True, False, 0, 0.15, 61),
    Case("128->128 2x16x16 f16 out resid ldc", 128, (2, 16, 16), True, True, True, 8, 0.005, 5),
    Case("128->128 3x16x16 bias resid ldc", 128, (3, 16, 16), True, True, False, 4, 0.15, 61),
]


def operands(case, seed):
    """as R.conv3d_operands builds them: 0 / 1 / 2 activations, k / 64 weights, bias and residual"""
    small = case.out_f16
    x = R.binary(B, case.C, *case.dims, seed=seed, density=case.density)
    w = R.ints64(case.C, case.C, 3, 3, 3, seed=1, span=case.span)
    bias = R.ints64(case.C, seed=2, span=7 if small else 47) if case.bias else None
    resid = R.ints64(B, case.C, *case.dims, seed=4, span=9 if small else 59) if case.resid else None
    return x, w, bias, resid


def check_exact(name, out, want, fam, out_f16, C):
    v = want * 64
    assert torch.equal(v, v.round()) and v.abs().max().item() < 2 ** 24, "the case is not exact in fp32"
    close(out.out, want, f"conv3z exact {name}", fam, rel=EXACT, mx=EXACT)
    if out_f16:
        w32 = want.float()
        assert torch.equal(w32.half().float(), w32) and torch.equal(w32.bfloat16().float(), w32), "the reference is not representable in 16 bits"
        assert out.raw.dtype == OPD
        rows = want.permute(0, 2, 3, 4, 1).reshape(-1, C).to(OPD)
        assert torch.equal(out.raw.cpu().view(torch.int16), rows.view(torch.int16)), f"{name}: the 16-bit result is not the rounded reference"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_conv3z_exact(eng, case):
    """every product and partial sum is exact, so the result is the reference whatever the order of the sum -- and O(1) away from
    it for a wrong depth tap, plane, sample, halo pixel or column"""
    x, w, bias, resid = operands(case, CASES.index(case))
    acc = R.conv3d(x, w)
    assert (acc != 0).double().mean().item() > (0.2 if case.out_f16 else 0.5), "most accumulators are zero: the case would not see a wrong tap"
    ldc = case.C + case.ldc_pad
    ldr = case.C + (4 if case.ldc_pad else 0)
    out, fams = probed(eng, lambda: eng.op_conv3d_form(x, w, 1, bias=bias, resid=resid, ldr=ldr if case.resid else 0, out_f16=case.out_f16,
                                                       ldc=ldc, a_half=True, poison=True))
    want_fam = "conv3z_kernel<2>" if case.C == 64 else "conv3z_kernel<4>"
    assert fams == {want_fam: 1}, f"meant for one launch of {want_fam}, ran {fams}"
    check_exact(case.name, out, R.conv3d(x, w, bias=bias, resid=resid), want_fam, case.out_f16, case.C)


@pytest.mark.parametrize("D,family", [(65, "conv3z_kernel<2>"), (64, "gemm_dma_kernel<64,0>")])
def test_the_engine_routes_by_rows(eng, D, family):
    """form 0 (mvd_op_conv3d_ex): 65 x 16 x 16 = 16640 rows is above the 16384 rows up to which a 27-tap layer goes to the LDS-DMA tap
    gather and runs on conv3z; 16384 rows stay where they were"""
    x = R.binary(1, 64, D, 16, 16, seed=3, density=0.15)
    w, bias = R.ints64(64, 64, 3, 3, 3, seed=1), R.ints64(64, seed=2, span=47)
    out, fams = probed(eng, lambda: eng.op_conv3d_ex(x, w, bias, a_half=True, force_splitk=1))
    assert fams == {family: 1}, fams
    close(out.out, R.conv3d(x, w, bias=bias), f"conv3z routed 64->64 {D}x16x16 (form 0)", family, rel=EXACT, mx=EXACT)


RANDOM = [("64->64 3x32x16", 64, (3, 32, 16), False), ("128->128 2x16x16 f16 out", 128, (2, 16, 16), True)]


@pytest.mark.parametrize("name,C,dims,out_f16", RANDOM, ids=[c[0] for c in RANDOM])
def test_conv3z_random(eng, name, C, dims, out_f16):
    x = R.rnd(B, C, *dims, seed=1)
    w = R.rnd(C, C, 3, 3, 3, seed=2, scale=(C * 27) ** -0.5)
    bias, resid = R.rnd(C, seed=3), R.rnd(B, C, *dims, seed=5)
    out, fams = probed(eng, lambda: eng.op_conv3d_form(x, w, 1, bias=bias, resid=resid, out_f16=out_f16, a_half=True))
    want_fam = "conv3z_kernel<2>" if C == 64 else "conv3z_kernel<4>"
    assert fams == {want_fam: 1}, fams
    close(out.out, R.conv3d(x, w, bias=bias, resid=resid), f"conv3z random {name}", want_fam, rel=REL_L2, mx=MAX_N)


def test_form_1_refuses_what_the_kernel_does_not_take(eng):
    """each hard limit is the library's error and launches nothing: never another kernel in the named form's place"""
    def z(*s):
        return torch.zeros(*s)
    ok_x, ok_w = z(1, 64, 2, 16, 16), z(64, 64, 3, 3, 3)
    bad = [
        ("conv3z", lambda: eng.op_conv3d_form(z(1, 72, 2, 16, 16), z(64, 72, 3, 3, 3), 1)),     # Cin % 64
        ("conv3z", lambda: eng.op_conv3d_form(ok_x, z(40, 64, 3, 3, 3), 1)),                    # Cout not 64 / 128
        ("conv3z", lambda: eng.op_conv3d_form(z(1, 64, 2, 8, 16), ok_w, 1)),                    # H not a multiple of the tile
        ("conv3z", lambda: eng.op_conv3d_form(z(1, 64, 2, 16, 24), ok_w, 1)),                   # W not a multiple of the tile
        ("conv3z", lambda: eng.op_conv3d_form(ok_x, ok_w, 1, a_half=False)),                    # fp32 source
        ("stride-1", lambda: eng.op_conv3d_form(ok_x, ok_w, 1, stride=2)),
        ("stride-1", lambda: eng.op_conv3d_form(ok_x, z(64, 64, 3, 3, 3), 1, transposed=True)),
        ("form must", lambda: eng.op_conv3d_form(ok_x, ok_w, 2)),
    ]
    eng.probe_config(1)
    try:
        for text, call in bad:
            with pytest.raises(L.MvdError, match=text):
                call()
        torch.cuda.synchronize()
        rep = eng.probe_report()
    finally:
        eng.probe_config(0)
    assert not [d for d in rep if d["launches"] > 0 and ("conv" in d["family"] or "gemm" in d["family"])], rep
    assert eng.op_conv3d_form(ok_x, ok_w, 1).out.abs().max() == 0  # ... and the good shape runs

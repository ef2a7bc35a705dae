"""CPU: which 3x3x3 layers the engine's routing gives to conv3z (csrc/k_conv3x.hip), asked of the library's own predicate
(mvd_conv3d_routed_form: igemm_go's test on the descriptor run_conv3d builds, no context and no device): the two production shapes of
the frustum network, yes; every case of the table tests/test_gpu_conv3d_forms.py asserts kernel families for, no; and the exact
cases of tests/test_gpu_conv3d_halo.py are what they claim to be."""
import pytest
import torch

from morphablediffusion_amd import lib as L
from tests import epilogue_ref as R


def routed(kind, B, Cin, Cout, dims, a_half=True, out_f16=False, ldc=0, resid=False, resid_f16=False, ldr=0, force_splitk=0):
    r = L.load().mvd_conv3d_routed_form(B, *dims, Cin, Cout, 2 if kind == "s2" else 1, int(kind == "T"), int(a_half), int(out_f16),
                                        ldc or Cout, int(resid), int(resid_f16), (ldr or Cout) if resid else 0, force_splitk)
    assert r >= 0, L.load().mvd_last_error()
    return r


# the headline step: 16 views; conv0 64 -> 64 at 48 x 32 x 32, conv2 128 -> 128 at 24 x 16 x 16 (FrustumTV3DNet), and the same two
# widths in SpatialTime3DNet (one 32^3 volume: only its level 0 is above the row floor)
PRODUCTION = [("s1", 16, 64, 64, (48, 32, 32)), ("s1", 16, 128, 128, (24, 16, 16)), ("s1", 1, 64, 64, (32, 32, 32))]


@pytest.mark.parametrize("shape", PRODUCTION, ids=str)
def test_the_production_shapes_are_routed_to_conv3z(shape):
    assert routed(*shape) == 1
    assert routed(*shape, resid=True) == 1 and routed(*shape, out_f16=True, ldc=shape[3] + 8) == 1


@pytest.mark.parametrize("name", [c.name for c in R.CONV3D_CASES])
def test_no_case_of_the_forms_table_is_routed_to_conv3z(name):
    c = R.CONV3D_BY_NAME[name]
    ldc, ldr = R.conv3d_ld(c)
    for fsk in {c.force_splitk, 1}:  # the table's 0 is passed as 1 by the exact test
        assert routed(c.kind, c.B, c.Cin, c.Cout, c.dims, c.a_half, c.out_f16, ldc, True, c.in_place and c.out_f16, ldr, fsk) == 0


@pytest.mark.parametrize("shape", [("s2", 6, 64, 128, (12, 8, 8)), ("s1", 6, 128, 128, (6, 4, 4)), ("T", 6, 128, 64, (6, 4, 4)),
                                   ("s1", 1, 72, 40, (17, 32, 32))], ids=str)
def test_no_random_case_of_the_forms_file_is_routed_to_conv3z(shape):
    assert routed(*shape, resid=True, out_f16=shape[0] == "T", resid_f16=shape[0] == "T") == 0


def test_each_condition_of_the_predicate_refuses_on_its_own():
    ok = ("s1", 16, 64, 64, (48, 32, 32))
    assert routed(*ok) == 1
    assert routed("s1", 1, 64, 64, (65, 16, 16)) == 1 and routed("s1", 1, 64, 64, (64, 16, 16)) == 0   # 16640 / 16384 rows
    assert routed("s1", 2, 128, 128, (24, 16, 16)) == 0                                               # conv2's shape at two views
    assert routed("s2", *ok[1:]) == 0 and routed("T", *ok[1:]) == 0
    assert routed("s1", 16, 72, 64, (48, 32, 32)) == 0 and routed("s1", 16, 32, 64, (48, 32, 32)) == 0  # Cin % 64
    assert routed("s1", 16, 64, 40, (48, 32, 32)) == 0 and routed("s1", 16, 64, 192, (48, 32, 32)) == 0 and routed("s1", 16, 64, 256, (48, 32, 32)) == 0
    assert routed("s1", 16, 64, 64, (48, 24, 32)) == 0 and routed("s1", 16, 64, 64, (48, 32, 40)) == 0  # H / W not tile multiples
    assert routed(*ok, a_half=False) == 0                                                             # fp32 source
    assert routed(*ok, force_splitk=2) == 0 and routed(*ok, force_splitk=1) == 1                      # a forced split keeps its kernel
    assert routed(*ok, resid=True, resid_f16=True) == 0                                               # 16-bit residual
    assert L.load().mvd_conv3d_routed_form(0, 1, 16, 16, 64, 64, 1, 0, 1, 0, 64, 0, 0, 0, 0) == -1


def test_the_exact_cases_of_the_gpu_file_are_exact():
    from tests import test_gpu_conv3d_halo as T
    for i, case in enumerate(T.CASES):
        x, w, bias, resid = T.operands(case, i)
        for t in (x, w, bias, resid):
            assert t is None or (torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t))
        want = R.conv3d(x, w, bias=bias, resid=resid)
        v = want * 64
        assert torch.equal(v, v.round()) and v.abs().max().item() < 2 ** 24
        acc = R.conv3d(x, w)
        assert (acc != 0).double().mean().item() > (0.2 if case.out_f16 else 0.5), case.name
        if case.out_f16:
            w32 = want.float()
            assert torch.equal(w32.half().float(), w32) and torch.equal(w32.bfloat16().float(), w32), case.name

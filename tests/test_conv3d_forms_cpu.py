"""CPU: the fp64 reference of the 3-D convolutions (tests/epilogue_ref.py conv3d) against torch's fp32 convolutions, and the conditions
the case table of tests/test_gpu_conv3d_forms.py is built to meet: exact operands where exactness is claimed, results a 16-bit type
holds where the result is 16-bit, every routing cell igemm_go / run_convT3d allow, both sides of the row thresholds."""
import pytest
import torch
import torch.nn.functional as F

from tests import epilogue_ref as R

IDS = [c.name for c in R.CONV3D_CASES]


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("kind", ["s1", "s2", "T"])
@pytest.mark.parametrize("dims", [(5, 7, 9), (1, 3, 5), (2, 2, 2)])
def test_conv3d_reference_agrees_with_the_fp32_torch_convolutions(kind, dims):
    B, Cin, Cout = 2, 8, 12
    T = kind == "T"
    x = R.rnd(B, Cin, *dims)
    w = R.rnd(*((Cin, Cout) if T else (Cout, Cin)), 3, 3, 3, seed=1, scale=(Cin * 27) ** -0.5)
    bias = R.rnd(Cout, seed=2)
    od = R.conv3d_out_dims(kind, dims)
    res = R.rnd(B, Cout, *od, seed=3)
    if T:
        want = F.conv_transpose3d(x, w, bias, stride=2, padding=1, output_padding=1) + res
    else:
        want = F.conv3d(x, w, bias, stride=2 if kind == "s2" else 1, padding=1) + res
    got = R.conv3d(x, w, stride=2 if kind == "s2" else 1, transposed=T, bias=bias, resid=res)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, Cout, *od) == tuple(want.shape)
    assert (got - want.double()).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    # the output grids the hooks size their buffers by: (n - 1) / 2 + 1 under stride 2, 2 n transposed
    assert od == tuple(2 * n if T else ((n - 1) // 2 + 1 if kind == "s2" else n) for n in dims)


def test_transposed_reference_is_the_scatter_it_is_defined_as():
    """out[2 i - 1 + k] += x[i] w[k] per axis (ConvTranspose3d k3 s2 p1 op1), written out with loops"""
    B, Cin, Cout, dims = 1, 3, 2, (2, 3, 2)
    x, w = R.rnd(B, Cin, *dims).double(), R.rnd(Cin, Cout, 3, 3, 3, seed=1).double()
    D, H, W = dims
    want = torch.zeros(B, Cout, 2 * D, 2 * H, 2 * W, dtype=torch.float64)
    for z in range(D):
        for y in range(H):
            for xx in range(W):
                for kz in range(3):
                    for ky in range(3):
                        for kx in range(3):
                            oz, oy, ox = 2 * z - 1 + kz, 2 * y - 1 + ky, 2 * xx - 1 + kx
                            if 0 <= oz < 2 * D and 0 <= oy < 2 * H and 0 <= ox < 2 * W:
                                want[0, :, oz, oy, ox] += x[0, :, z, y, xx] @ w[:, :, kz, ky, kx]
    assert (R.conv3d(x, w, transposed=True) - want).abs().max().item() <= 1e-12


# -------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name", IDS)
def test_exact_cases_are_exact(name):
    """operands 0 / 1 / 2 and k / 64: the reference times 64 is an integer below 2^24, so the fp32 accumulator holds every partial
    sum exactly in any order; a 16-bit result must hold the reference without rounding in fp16 AND in bfloat16"""
    case = R.CONV3D_BY_NAME[name]
    x, w, bias, resid = R.conv3d_operands(case)
    for t in (x, w, bias, resid):
        assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t), "an operand is not exact in 16 bits"
    assert x.abs().max() > 0 and (x != 0).double().mean() < 0.5
    want = R.conv3d_reference(name)
    v = want * 64
    assert torch.equal(v, v.round()) and v.abs().max().item() < 2 ** 24
    # without bias and residual too (the accumulator alone), and the accumulator is not trivially zero
    acc = R.conv3d(x, w, stride=2 if case.kind == "s2" else 1, transposed=case.kind == "T") * 64
    assert torch.equal(acc, acc.round()) and acc.abs().max().item() < 2 ** 24
    assert (acc != 0).double().mean().item() > 0.5, "most accumulators are zero: the case would not see a wrong tap"
    if case.out_f16:
        w32 = want.float()
        assert torch.equal(w32.double(), want)
        assert torch.equal(w32.half().float(), w32), "the reference is not representable in fp16"
        assert torch.equal(w32.bfloat16().float(), w32), "the reference is not representable in bfloat16"
        if case.in_place:  # the residual is rounded to 16 bits when it is copied into the result buffer
            assert torch.equal(resid.bfloat16().float(), resid) and torch.equal(resid.half().float(), resid)


# ----------------------------------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize("name", IDS)
def test_each_case_is_routed_as_the_table_says(name):
    c = R.CONV3D_BY_NAME[name]
    ldc, ldr = R.conv3d_ld(c)
    args = (c.kind, c.B, c.Cin, c.Cout, c.dims, c.a_half, c.force_splitk, ldc, ldr)
    assert c.Cin % 8 == 0 and c.Cout % 4 == 0 and ldc % 4 == 0 and ldr % 4 == 0 and c.force_splitk in (0, 2)
    assert R.conv3d_family_ok(c.family, *args)
    assert not any(R.conv3d_family_ok(f, *args) for f in ("dense", "gather_f16", "gather_f32") if f != c.family)
    assert len(R.conv3d_launches(*args)) == c.launches
    assert R.conv3d_reduce_launches(*args) == c.reduces
    assert R.conv3d_cell(c) in R.CONV3D_CELLS


def test_the_table_reaches_every_allowed_cell():
    reached = {R.conv3d_cell(c) for c in R.CONV3D_CASES}
    assert reached == R.CONV3D_CELLS, sorted(R.CONV3D_CELLS - reached)
    # what the routing does not allow cannot be built: a parity-batched launch on a gather kernel
    for Cin, a_half in ((64, False), (64, True)):
        for rows_dims in ((4, 8, 8), (2, 3, 4)):
            l = R.convT3d_launches(2, Cin, 40, rows_dims, a_half)
            assert len(l) == 8 or l == [("dense", 8)]


def test_the_table_has_a_case_on_each_side_of_every_threshold():
    fwd = [R.conv3d_rows(c.kind, c.B, c.dims) for c in R.CONV3D_CASES if c.kind != "T" and c.a_half]
    assert any(m < R.DENSE_MIN_M for m in fwd) and R.DENSE_MIN_M in fwd
    assert R.CONV3D_DMA_MAX_M in fwd and any(m > R.CONV3D_DMA_MAX_M for m in fwd)
    for kind in ("s1", "s2"):  # ... above 16384 rows at both strides
        assert any(R.conv3d_rows(c.kind, c.B, c.dims) > R.CONV3D_DMA_MAX_M for c in R.CONV3D_CASES if c.kind == kind and c.a_half)
    tr = [(R.conv3d_rows("T", c.B, c.dims), c.launches) for c in R.CONV3D_CASES if c.kind == "T" and c.a_half and c.force_splitk <= 1]
    assert (R.CONVT3D_BATCH_MIN_ROWS, 1) in tr
    assert any(R.DENSE_MIN_M <= m < R.CONVT3D_BATCH_MIN_ROWS and n == 8 for m, n in tr)
    assert any(m < R.DENSE_MIN_M and n == 8 for m, n in tr)


def test_the_table_has_the_forms_the_networks_launch():
    T = [c for c in R.CONV3D_CASES if c.kind == "T"]
    # 160 columns is the widest tile (FAMILY): more than that is at least two column tiles, 200 and 320 leave a tail at 64 / 128 / 160
    assert any(c.launches == 1 and c.Cout > 160 for c in T)
    assert any(c.launches == 1 and c.Cout > 160 and c.Cout % 64 and c.Cout % 160 for c in T)
    walks = [R.parity_batch_nch(R.conv3d_rows("T", c.B, c.dims), c.Cin, c.Cout) for c in T if c.launches == 1]
    assert min(walks) == 1 and max(walks) > 1                                                    # a column walk, and none
    assert any(c.launches == 1 and c.in_place and c.out_f16 and c.ldc_pad == 8 for c in T)      # the level-0 form
    assert any(c.launches == 1 and c.in_place and not c.out_f16 for c in T)                      # levels 1 and 2
    assert any(c.launches == 8 and c.reduces == 8 for c in T) and any(c.launches == 8 and c.reduces == 7 for c in T)
    assert any(c.launches == 1 and c.Cin % 64 for c in T)                                        # a K tail through the tap gather
    fwd = [c for c in R.CONV3D_CASES if c.kind != "T"]
    assert any(c.family == "dense" and c.Cin % 64 and c.Cin > 64 for c in fwd)                   # one full chunk plus a tail
    assert any(1 in c.dims for c in fwd) and any(len(set(c.dims)) == 3 for c in fwd)
    assert any(c.kind == "s2" and any(n % 2 for n in c.dims) for c in fwd)
    # 945 rows of 5x7x9 volumes: sample and depth-slice boundaries fall inside the 128- and 256-row tiles
    assert all(m % 128 and m % 256 for m in (5 * 7 * 9, 2 * 5 * 7 * 9, 7 * 9))

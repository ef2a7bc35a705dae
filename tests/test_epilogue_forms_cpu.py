"""CPU: the fp64 references of tests/epilogue_ref.py against torch's own operations composed by hand, the error of the split-arithmetic
emulation that the GPU bound of tests/test_gpu_epilogue_forms.py is taken from, and the conditions each GPU case is built to meet
(exact operands where exactness is claimed, the eligibility conditions of the kernel family a case names)."""
import pytest
import torch
import torch.nn.functional as F

from tests import epilogue_ref as R


def same(got, want, tol=1e-12):
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())


# ----------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("act", [0, 1])
def test_linear_reference_is_f_linear_composed_by_hand(act):
    B, rps, K, N = 3, 5, 16, 12
    a, w, bias, rb, res = (R.rnd(B * rps, K).double(), R.rnd(N, K, seed=1).double(), R.rnd(N, seed=2).double(),
                           R.rnd(B, N, seed=3).double(), R.rnd(B * rps, N, seed=4).double())
    want = 0.5 * F.linear(a, w)
    want = want + bias
    want = (want.reshape(B, rps, N) + rb[:, None, :]).reshape(B * rps, N) + res
    want = F.silu(want) if act else want
    same(R.linear(a, w, B=B, alpha=0.5, bias=bias, rowbias=rb, resid=res, act=act), want)
    same(R.linear(a, w), F.linear(a, w))


@pytest.mark.parametrize("stride,ups", [(1, 0), (2, 0), (1, 1)])
def test_conv_reference_is_f_conv2d_composed_by_hand(stride, ups):
    B, Cin, H, W, Cout = 2, 4, 6, 5, 3
    x, w, bias, rb = R.rnd(B, Cin, H, W).double(), R.rnd(Cout, Cin, 3, 3, seed=1).double(), R.rnd(Cout, seed=2).double(), R.rnd(B, Cout, seed=3).double()
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if ups else x
    want = F.conv2d(xin, w, bias, stride=stride, padding=1) + rb[:, :, None, None]
    same(R.conv(x, w, stride=stride, upsample=ups, bias=bias, rowbias=rb), want)


@pytest.mark.parametrize("H,W", R.TAP_SHIFT_SHAPES)
def test_padded_stride_2_reference_and_why_only_even_sides(H, W):
    x, w = R.rnd(2, 4, H, W).double(), R.rnd(3, 4, 3, 3, seed=1).double()
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    same(R.conv(x, w, tap_shift=1), want)
    assert want.shape[2:] == (H // 2, W // 2)  # the grid run_conv2d computes: (H - 1) // 2 + 1, equal only for even sides
    assert (H - 1) // 2 + 1 == H // 2 and (W - 1) // 2 + 1 == W // 2
    # the same taps, written as the kernel addresses them: offsets {0, 1, 2} from 2 y, rows / columns past the image are zero
    y = torch.zeros_like(want)
    xp = F.pad(x, (0, 2, 0, 2))
    for ky in range(3):
        for kx in range(3):
            y += torch.einsum("bchw,oc->bohw", xp[:, :, ky:ky + H:2, kx:kx + W:2][:, :, :H // 2, :W // 2], w[:, :, ky, kx])
    same(y, want)
    assert not torch.allclose(want, F.conv2d(x, w, stride=2, padding=1))


def test_group_norm_reference_is_f_group_norm_of_the_sum():
    nslab, B, rows, C, G = 3, 2, 10, 12, 3
    x = R.rnd(nslab, B, rows, C).double()
    g, b, bias2, pre, res = (R.rnd(C, seed=1).double(), R.rnd(C, seed=2).double(), R.rnd(C, seed=3).double(), R.rnd(B, C, seed=4).double(),
                             R.rnd(B, rows, C, seed=5).double())
    v = x[0] + x[1] + x[2] + bias2 + pre[:, None, :] + res
    want = F.silu(F.group_norm(v.permute(0, 2, 1), G, g, b, 1e-5)).permute(0, 2, 1)
    got, summed = R.group_norm(x, G, g, b, 1e-5, 1, bias2=bias2, preadd=pre, resid=res)
    same(got, want)
    same(summed, v)


def test_layer_norm_reference_is_f_layer_norm_of_the_sum():
    nslab, rows, C, T = 2, 9, 16, 3
    x = R.rnd(nslab, rows, C).double()
    g, b, bias, rb, res = (R.rnd(C, seed=1).double(), R.rnd(C, seed=2).double(), R.rnd(C, seed=3).double(), R.rnd(rows // T, C, seed=4).double(),
                           R.rnd(rows, C, seed=5).double())
    v = x[0] + x[1] + bias + rb.repeat_interleave(T, 0) + res
    got, summed = R.layer_norm(x, g, b, 1e-5, bias=bias, rowbias=rb, T=T, resid=res)
    same(got, F.layer_norm(v, (C,), g, b, 1e-5))
    same(summed, v)


@pytest.mark.parametrize("cols", R.SOFTMAX_COLS)
def test_softmax_reference_and_inputs(cols):
    s = R.softmax_scores(cols)
    want = R.softmax(s)
    same(want, torch.softmax(s.double(), 1))
    assert torch.isfinite(want).all() and (want.sum(1) - 1).abs().max() < 1e-12
    if cols > 1:
        assert s[0].abs().max() > 1e4 and want[1].max() > 0.9 and (want[2] == 1.0 / cols).all()
    # the rows of magnitude 1e4: wherever exp(v - max) is not zero in fp32 (v - max > -104), v and max are close enough for the
    # kernel's fp32 subtraction to be exact -- its error elsewhere is multiplied by zero
    d, d64 = s[0] - s[0].max(), s[0].double() - s[0].double().max()
    live = d64 > -104
    assert torch.equal(d.double()[live], d64[live]) and (want[0][~live] < 1e-45).all()


# -------------------------------------------------------------------------------------------------- the split emulation
def test_split16_carries_22_bits():
    x = R.rnd(4096, seed=9) * 3
    hi, lo = R.split16(x)
    assert torch.equal(hi, x.half())
    big = x.abs() >= 0.125  # below that `lo` is an fp16 subnormal: absolute error <= 2^-25
    assert ((hi.double() + lo.double() - x.double()).abs()[big] <= 2.0 ** -22 * x.double().abs()[big]).all()
    assert ((hi.double() + lo.double() - x.double()).abs() <= 2.0 ** -22 * x.double().abs() + 2.0 ** -25).all()


@pytest.mark.parametrize("name", list(R.XP_CASES))
def test_emulation_error_is_where_the_gpu_bound_is_taken_from(name):
    """The GPU test asserts (a) err <= 2 x emulation and (b) plain >= 20 x err.  hi + lo carries 22 bits per operand (2.4e-7), the
    dropped a_lo w_lo term is 2^-22 of a product, fp32 accumulation over K terms adds ~sqrt(K) 2^-24: the emulation must sit at a
    few 1e-7 (below 2e-6: K = 2880 for the widest case), and the plain fp16-operand product (2^-11 per operand, ~3e-4) at least
    40x above twice of it -- otherwise (a) and (b) could not both hold for a correct kernel."""
    want, emu, plain = R.xp_reference(name)
    print(f"[emulation] {name}: three-product fp32 emulation relL2={emu:.2e}, plain fp16 operands relL2={plain:.2e}")
    assert 2e-8 < emu < 2e-6, emu
    assert 1e-4 < plain < 1e-3, plain
    assert plain >= 40 * (2 * emu), (plain, emu)


def test_a_zeroed_lo_block_would_fail_both_conditions():
    """what the GPU conditions are there to catch: with w_lo = 0 the result falls back to ~2^-11 of the weights"""
    a, w = R.xp_operands("linear K=320")
    want, emu, plain = R.xp_reference("linear K=320")
    ah, al = R.split16(a)
    wh, _ = R.split16(w)
    broken = ah.float() @ wh.float().t() + al.float() @ wh.float().t()
    err = R.rel_l2(broken, want)
    assert err > 2 * emu * 100 and plain < 20 * err


# ------------------------------------------------------------------------------------------ what the GPU cases must satisfy
def exact_in_fp16(t):
    return torch.equal(t.half().float(), t.float())


def test_exact_operands_are_exact():
    for t in (R.ints64(72, 128, seed=1), R.ints64(200, seed=2, span=47), R.ints64(32, 200, seed=3, span=53), R.ints64(2048, 200, seed=4, span=59),
              R.ints64(128, 64, 3, 3, seed=1)):
        assert exact_in_fp16(t) and torch.equal(t * 64, (t * 64).round()) and t.abs().max() < 0.5
    for t in (R.binary(288, 128), R.binary(6, 64, 8, 8, seed=1)):
        assert set(t.unique().tolist()) == {0.0, 1.0, 2.0}
    # asymmetric: distinct per row and per column (a transposed or shifted read shows)
    rb = R.ints64(32, 200, seed=3, span=53)
    assert not torch.equal(rb[0], rb[1]) and not torch.equal(rb[:, 0], rb[:, 1]) and len({tuple(r.tolist()) for r in rb}) == 32
    bias = R.ints64(200, seed=2, span=47)
    assert bias.unique().numel() > 40


@pytest.mark.parametrize("B,rps", R.SAMPLE_GEOMETRIES)
@pytest.mark.parametrize("N,rb_ld", R.LINEAR_NS)
def test_exact_linear_cases_are_exact_in_fp32_and_fp16(B, rps, N, rb_ld):
    rows, K = B * rps, R.LINEAR_K
    a, w = R.binary(rows, K), R.ints64(N, K, seed=1)
    bias, rb, res = R.ints64(N, seed=2, span=47), R.ints64(B, N, seed=3, span=53), R.ints64(rows, N, seed=4, span=59)
    for alpha in (0.5, 1.0):
        want = R.linear(a, w, B=B, alpha=alpha, bias=bias, rowbias=rb, resid=res)
        # every value is a multiple of 1/128 below 16: exact in fp32 whatever the summation order, and exact as an fp16 result
        assert torch.equal(want * 128, (want * 128).round()) and want.abs().max() < 16
        assert exact_in_fp16(want)
    assert rb_ld > N and rb_ld % 4 == 0 and N % 4 == 0
    assert N % 64 and N % 128 and N % 160  # a column tail at every tile width
    for fam in ("dense", "gather_f32"):
        assert R.linear_family_ok(fam, rows, K, N, a_half=fam == "dense")
    # a wrong sample index moves a result by at least 1/64
    assert (rb[0] - rb[-1]).abs().max() >= 1 / 64


def test_sample_geometries_reach_what_they_are_for():
    g = dict((b, r) for b, r in R.SAMPLE_GEOMETRIES)
    assert g[16] == 16 and g[32] == 16 and 256 // 16 > 1                      # many samples per 256-row tile
    assert g[6] % 32 != 0 and not R.folded_expected(g[6], 1.0, 1)             # unfolded
    assert g[3] % 32 == 0 and g[3] < 256 and R.folded_expected(g[3], 1.0, 1)  # folded, several samples per tile
    assert (5 * g[5]) % 256 != 0 and (5 * g[5]) % 128 != 0                    # ragged last tile (also of the 128-row tiles)
    assert g[2] % 256 == 0
    assert not R.folded_expected(96, 0.5, 1) and not R.folded_expected(96, 1.0, 2)
    assert R.LINEAR_K // 64 == 2                                             # a forced split of 2 has a k-step per slab


@pytest.mark.parametrize("case", R.CONV_CASES, ids=[c[0] for c in R.CONV_CASES])
def test_conv_cases_meet_the_conditions_of_the_family_they_name(case):
    name, B, Cin, H, W, Cout, a_half, stream, family = case
    assert R.conv_family_ok(family, B, Cin, H, W, Cout, a_half, stream)
    others = [f for f in ("conv3x", "halo", "dense", "gather_f32", "gather_f16") if f != family]
    assert not any(R.conv_family_ok(f, B, Cin, H, W, Cout, a_half, stream) for f in others), "the routing must be unambiguous"
    if family == "conv3x":  # a form conv3x does not take runs on the halo kernel
        assert R.conv_family_ok("halo", B, Cin, H, W, Cout, a_half, stream, alpha=0.5)
        assert R.conv_family_ok("halo", B, Cin, H, W, Cout, a_half, stream, out_f16=True)
    if (H, W) == (8, 8):
        assert B % 4 and B > 4  # four images per tile: a partial last tile whose first tile straddles samples
    x, w = R.binary(B, Cin, H, W, seed=1), R.ints64(Cout, Cin, 3, 3, seed=1)
    want = R.conv(x, w, alpha=0.5, bias=R.ints64(Cout, seed=2, span=47), rowbias=R.ints64(B, Cout, seed=3, span=53),
                  resid=R.ints64(B, Cout, H, W, seed=4, span=59))
    assert torch.equal(want * 128, (want * 128).round()) and want.abs().max() < 16 and exact_in_fp16(want)


@pytest.mark.parametrize("source", ["fp32", "xp"])
@pytest.mark.parametrize("H,W", R.TAP_SHIFT_SHAPES)
def test_tap_shift_cases(H, W, source):
    assert H % 2 == 0 and W % 2 == 0
    rows = 4 * (H // 2) * (W // 2)
    fam = "gather_f32" if source == "fp32" else ("dense" if rows >= R.DENSE_MIN_M else "gather_f16")
    assert R.conv_family_ok(fam, 4, 64, H, W, 64, False, False, xp=source == "xp", stride=2)


def test_xp_cases_reach_the_families_the_gpu_test_names():
    assert set(R.XP_FAMILIES) == set(R.XP_CASES)
    for name, (kind, p) in R.XP_CASES.items():
        for fam in R.XP_FAMILIES[name]:
            if kind == "linear":
                assert R.linear_family_ok(fam, p[0], p[1], p[2], True, xp=True)
            elif p[5] == 1:
                assert fam == "dense" and p[0] * p[2] * p[3] >= R.DENSE_MIN_M
            else:
                assert R.conv_family_ok(fam, p[0], p[1], p[2], p[3], p[4], True, fam == "conv3x", xp=True, stride=p[6]), (name, fam)
    # what the issue lists
    ks = [p[1] for k, p in R.XP_CASES.values() if k == "linear"]
    assert sorted(ks) == [320, 1280]


def test_group_norm_cases_cover_every_register_tile_once():
    tiles = [R.gn_tile_of(r, c, g) for _, r, c, g in R.GN_TILE_CASES]
    assert set(tiles) == {(256, 4), (512, 4), (512, 10), (512, 16), (1024, 10), (1024, 16)}
    n2 = [r * (c // g) // 2 for _, r, c, g in R.GN_TILE_CASES]
    assert n2[:7] == [1024, 1025, 2048, 5120, 8192, 10240, 16384]
    assert {c // g for _, _, c, g in R.GN_TILE_CASES} >= {10, 20, 30, 40, 80, 16, 32}
    for B, r, c, g in R.GN_TILE_CASES + [R.GN_REMAINDER_CASE, (2, 64, 64, 8), (1, 100, 40, 4)]:
        assert R.gn_group_eligible(c + 6, r, c, g, c + 8, c + 10) and R.gn_group_eligible(c, r, c, g, c, c)
    B, r, c, g = R.GN_REMAINDER_CASE
    assert (B * g) % 8 and (c, g, B) == (20, 5, 3)
    assert R.GN_NSLABS == [1, 2, 3, 4, 5, 7, 8, 9, 12, 16]  # 5, 8, 9, 12: one, just under two, two and just under three steps of four


def test_layer_norm_cases():
    assert [c for _, c, _ in R.LN_CASES] == [320, 640, 1280, 2560] and R.LN_NSLABS == [1, 2, 5]
    for rows, C, T in R.LN_CASES:
        rpw = R.ln_rows_per_workgroup(C)
        assert rows % rpw and rpw % T and rows % T == 0 and C % 40 == 0 and C // 40 in (8, 16, 32, 64)
    assert 320 // 64 >= max(R.LN_NSLABS)  # the producing GEMM (K = 320) has a k-step per slab


def test_folded_group_norm_cases():
    assert {(b, r) for b, r, _, _, _ in R.FOLDED_GN_CASES} == {(2, 256), (2, 512)}
    assert {n for _, _, _, n, _ in R.FOLDED_GN_CASES} == {64, 192, 256} and {c for *_, c in R.FOLDED_GN_CASES} == {8, 16, 32}
    for B, rps, K, N, cpg in R.FOLDED_GN_CASES:
        assert rps % 256 == 0 and B * rps >= 512 and K == 64 and N % cpg == 0 and N // cpg <= 32
    assert 192 % 128  # a column tail at bn = 128

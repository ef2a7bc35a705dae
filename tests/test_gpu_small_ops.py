"""GPU: the small-op layer one production launcher at a time -- everything in csrc/k_misc.hip and csrc/k_enc.hip, the element-wise
kernels of csrc/k_cond.hip and the samplers' batch assembly (csrc/c_api.hip) -- through the mvd_op_* small-op hooks, against the
float64 restatements of tests/small_ops_ref.py (tests/test_small_ops_cpu.py holds those against torch or index loops, and the case
tables against the launchers' path predicates).  Results are written by the launchers into 0xFF buffers with a guard row and pad
columns, which the engine wrappers check after every call; where a launcher has two forms, the form it took is asserted.

Tolerances.  The pure moves and packs (families 4, 5, the batch assembly, accumulate_f32 / add_rows: one IEEE fp32 operation) are
bit-exact.  The division of the batch assembly is compared bit for bit with the correctly rounded fp32 quotient: the Makefile
passes neither a fast-math flag nor -fno-hip-fp32-correctly-rounded-divide-sqrt, so the build's fp32 division is correctly
rounded.  The folds carry derived bounds (small_ops_ref.fold_bounds: half an ulp plus the fp64 summation slack), launch_mse one
fp32 ulp.  Everything else follows the rule of tests/test_gpu_norm_bwd_ops.py: the same closed form evaluated in float32 on the
CPU has error e32 against float64, and the kernel's error must be at most FACTOR * max(e32, 2^-22), FACTOR = 4, in relative L2
and in max error over max reference alike; a result that is added to is compared as got - preset.
The target encoder's float32 evaluation rounds its conv operands at the same eight points, so flipped 16-bit roundings are part
of e32 (they are all of it: 2e-4 against 1e-6 without them).  The impulse family has too few distinct values for e32 to hold
any flip (e32 is 0 on most views), so there the result -- exactly one rounding of silu(gn(conv0 x)), the final conv being the
centre-tap identity -- is held against the UNROUNDED float64 operand z: |got - z| <= ulp16(z) / 2 + d, with d the FACTOR rule's
allowance for z itself (e32 of z, before any rounding).  No constant is tuned.

Kernel -> test:
  target_encoder_kernel                                   test_target_encoder*, test_target_encoder_impulse
  small_linear_kernel (vector / scalar / broadcast)       test_small_linear, test_embed_time_mlp
  timestep_embedding_kernel                               test_timestep_embedding, test_embed_time_mlp
  nchw_to_nhwc(_tiled)_kernel, nhwc_to_nchw(_tiled)_kernel test_layout
  pack_weight_kernel / _taps_kernel / _taps_vec_kernel    test_pack_weight (target encoder: the init conv's 4 -> 8 pack in use)
  pack_upconv_weight, permute_geglu_bias, relu_beta_tile, fill_rows_f16, rows_f32_to_f16, upsample2_f16, add_image_rows,
  rows_f16_to_nchw, sparse_densify kernels                test_moves
  f32_to_f16_kernel                                       every hook with a 16-bit operand (test_small_linear compares its rounding)
  fold_gemm_kernel (fold_qk / fold_ov / fold_mm)          test_fold_qk_ov, test_fold_mm
  build_cfg_input_kernel, build_cfg_context_kernel        test_cfg_assemble
  cfg_ddim_kernel                                         test_cfg_ddim
  fuse_views_kernel, mse_kernel, accumulate_f32_kernel, add_rows_kernel     test_fuse_views, test_mse, test_exact_adds

Worst measured ratio kernel error / max(e32, 2^-22) per test (MI355X, fp16 build; the [parity] lines print every one):
  test_target_encoder            1.16  (random, n = 3, max norm: kernel 3.13e-4, e32 2.69e-4); offset family 1.12 (n = 16, max norm)
  test_target_encoder_impulse    0.994 of ulp16 / 2 + d (n = 16; e32 of z 1.5e-7), no element outside
  test_small_linear              0.75  (bc_vec_16_acc, max norm); vector path 0.48, scalar path 0.55, `a` one float off 0.29
  test_timestep_embedding        1.00  (dim 256, B = 1, t = 999: kernel 8.64e-6, e32 8.67e-6 -- the fp32 argument t * f)
  test_embed_time_mlp            0.95  (B = 1, L2)
  test_fold_qk_ov, test_fold_mm  1.000 of the derived bound (a half-ulp bound is met with equality by some element of a few thousand)
  test_cfg_ddim                  1.00  (n = 1); 0.55 at n = 1039, 0.48 at n = 4099
  test_fuse_views                1.06  (3 views, Nv = 37, no bias, accumulate, max norm)
  test_mse                       0.36 ulp (n = 1023)
No kernel missed its bound.  launch_fold_ov read Wo with a row stride of I instead of heads * hd (the same number in every
checkpoint, where the inner width equals I): at the shapes of test_fold_qk_ov it would have read past the operand, so the
launcher was corrected before the first run and there is no "before" figure.  The whole file takes 3 s on the GPU (96 tests).
"""
import itertools

import pytest
import torch

from morphablediffusion_amd import lib as L
from tests import small_ops_ref as R

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2.0 ** -22
OPD = torch.bfloat16 if L.DTYPE == "bf16" else torch.float16


@pytest.fixture(scope="module")
def eng():
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig
    e = Engine(UNetConfig(model_channels=64), VolumeConfig(), workspace_gb=0.25)
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


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(label, got, want):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    neq = bits(got) != bits(want)
    assert not bool(neq.any()), f"{label}: {int(neq.sum())} of {neq.numel()} elements differ, first at {neq.nonzero()[0].tolist()}"


def minus(got, start):
    """what the kernel added to `start`, the difference taken exactly"""
    return got.double().cpu() - start.double()


# ---- 1. target encoder ----------------------------------------------------------------------------------------------------------------
def run_encoder(eng, family, views, out=None, x=None):
    d = R.encoder_inputs(family)
    xs = d["x"][views] if x is None else x
    buf = eng.op_target_encoder(xs, d["pre"][views], d["w"], d["bias"], d["gamma"], d["beta"], out=out)
    return buf, buf[:len(views) * 1024].cpu()


def view_rows(t, views):
    return torch.cat([t[v * 1024:(v + 1) * 1024] for v in views])


@pytest.mark.parametrize("n", R.ENC_VIEWS)
@pytest.mark.parametrize("family", ["random", "offset"])
def test_target_encoder(eng, family, n):
    views = list(range(n))
    _, got = run_encoder(eng, family, views)
    r64, r32 = R.encoder_refs(family, OPD)
    check(f"target encoder {family} n={n}", {"feats": got}, {"feats": view_rows(r64, views)}, {"feats": view_rows(r32, views)})


@pytest.mark.parametrize("n", R.ENC_VIEWS)
def test_target_encoder_impulse(eng, n):
    """lit pixels at the corners, a mid-edge and an interior pixel through the first conv alone (tap orientation, halo zeroing, the
    (wave, tile, q, r) -> pixel map): one rounding of z = silu(gn(conv0 x)), held against the unrounded z (module docstring)"""
    views = list(range(n))
    _, got = run_encoder(eng, "impulse", views)
    d = R.encoder_inputs("impulse", n)
    z64, z32 = [R.encoder(d["x"], d["pre"], d["w"], d["bias"], d["gamma"], d["beta"], dt, OPD, final_operand=True) for dt in (torch.float64, torch.float32)]
    e32 = R.errs(z32.double(), z64)[1]
    dz = FACTOR * max(e32, FLOOR) * z64.abs().max()
    bound = 0.5 * R.ulp(z64.abs() + dz, *R.fmt16(OPD)) + dz
    err = (got.double() - z64).abs()
    worst = (err / bound).max().item()
    print(f"[parity] target encoder impulse n={n}: worst |got - z| / (ulp16 / 2 + d) = {worst:.3f}, e32(z) {e32:.3e}, {int((err > bound).sum())} outside")
    assert torch.isfinite(got).all() and worst <= 1.0
    lit = got.reshape(n, 32, 32, 16) - got.reshape(n, 32, 32, 16)[:, 16:17, 24:25]     # against a background pixel
    far = torch.ones(32, 32, dtype=torch.bool)
    for py, px in R.ENC_IMPULSES:
        far[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = False
        assert bool((lit[:, py, px].abs() > 0).any()), (py, px)
    assert bool((lit[:, far] == 0).all()), "a pixel outside every impulse's 3 x 3 footprint differs from the background"


@pytest.mark.parametrize("family", R.ENC_FAMILIES)
def test_target_encoder_views_are_independent(eng, family):
    """view v of the 16-view launch equals a 1-view launch of it, bit for bit (the engine shards views over devices); a second launch
    into the same buffer with other data in view 0 leaves the other views' results as they were"""
    buf, all16 = run_encoder(eng, family, list(range(16)))
    for v in (0, 5, 15):
        _, one = run_encoder(eng, family, [v])
        same_bits(f"target encoder {family} view {v} alone", one, all16[v * 1024:(v + 1) * 1024])
    d = R.encoder_inputs(family)
    x2 = d["x"].clone()
    x2[0] = d["x"][3].flip(1)
    buf2, again = run_encoder(eng, family, list(range(16)), out=buf, x=x2)
    assert buf2 is buf
    same_bits(f"target encoder {family} second launch, views 1..15", again[1024:], all16[1024:])
    assert not torch.equal(again[:1024], all16[:1024])


# ---- 2. small linear ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SL_CASES))
def test_small_linear(eng, name):
    c, d = R.SL_CASES[name], R.small_linear_inputs(name, OPD)
    got, form = eng.op_small_linear(d["a"], d["w"], d["bias"], c["rows"], c["act"], lda=c["lda"], ldo=c["ldo"], start=d["start"], a_off=c["a_off"])
    assert form == c["form"], (form, c["form"])
    ref = [R.small_linear(d["a"], d["w"], d["bias"], c["rows"], c["act"], dt) for dt in (torch.float64, torch.float32)]
    if c["accum"]:
        got, ref = minus(got, d["start"]), [R.added(d["start"], r, dt) for r, dt in zip(ref, (torch.float64, torch.float32))]
    check(f"small_linear {name}", {"out": got.cpu()}, {"out": ref[0]}, {"out": ref[1]})


def test_small_linear_unrounded_weights_are_rounded_once(eng):
    """the hook rounds fp32 weights with launch_f32_to_f16: the same result as weights rounded beforehand, bit for bit"""
    g = torch.Generator().manual_seed(1)
    a, w = torch.randn(3, 24, generator=g), torch.randn(5, 24, generator=g)
    got = [eng.op_small_linear(a, ww, None, 3)[0] for ww in (w, R.r16(w, OPD))]
    same_bits("small_linear weights", got[0], got[1])


# ---- 3. timestep embedding and the step MLP -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", list(R.TE_STEPS))
@pytest.mark.parametrize("dim", R.TE_DIMS)
def test_timestep_embedding(eng, dim, B):
    t = torch.tensor(R.TE_STEPS[B])
    got = eng.op_timestep_embedding(t, dim).cpu()
    if dim % 2:
        assert bool((bits(got[:, -1]) == 0).all()), "the odd last column must be written as 0"
    check(f"timestep_embedding dim={dim} B={B}", {"emb": got}, {"emb": R.timestep_embedding(t, dim, torch.float64)}, {"emb": R.timestep_embedding(t, dim, torch.float32)})


def test_embed_time_mlp():
    """mvd_embed_time: embedding, Linear, SiLU, Linear on a context that carries the step-embedding weights alone"""
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig, time_embed_manifest
    g = torch.Generator().manual_seed(3)
    td = 256
    sd = {"time_embed.0.weight": R.r16(torch.randn(td, td, generator=g) / 16, OPD), "time_embed.0.bias": 0.1 * torch.randn(td, generator=g),
          "time_embed.2.weight": R.r16(torch.randn(td, td, generator=g) / 16, OPD), "time_embed.2.bias": 0.1 * torch.randn(td, generator=g)}
    e = Engine(UNetConfig(model_channels=64), VolumeConfig(time_dim=td), workspace_gb=0.05)
    try:
        e.load_state_dict(sd, expected=time_embed_manifest(td))
        for B in R.TE_STEPS:
            t = torch.tensor(R.TE_STEPS[B])
            got = e.embed_time(t.cuda()).cpu()
            ref = [R.time_mlp(R.timestep_embedding(t, td, dt), sd["time_embed.0.weight"], sd["time_embed.0.bias"], sd["time_embed.2.weight"],
                              sd["time_embed.2.bias"], dt) for dt in (torch.float64, torch.float32)]
            check(f"embed_time B={B}", {"t_embed": got}, {"t_embed": ref[0]}, {"t_embed": ref[1]})
    finally:
        e.close()


# ---- 4. layout changes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.LAYOUT_CASES))
def test_layout(eng, name):
    C, HW, cpad, ld, want_form = R.LAYOUT_CASES[name]
    B = R.LAYOUT_B
    x = torch.randn(B, C, HW, generator=torch.Generator().manual_seed(C * HW))
    rows, form = eng.op_layout(0, x, B, C, HW, ld, cpad)      # columns cpad .. ld and the guard row: checked by the wrapper
    assert form == want_form
    same_bits(f"nchw_to_nhwc {name}", rows, R.nchw_to_nhwc(x, cpad))
    back, form = eng.op_layout(1, rows[:, :C], B, C, HW, ld)
    assert form == want_form
    same_bits(f"nhwc_to_nchw {name}", back, x)


# ---- 5. packs and fills ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.PW_CASES))
def test_pack_weight(eng, name):
    k = R.PW_CASES[name]
    N, cs, Cl, taps = k["N"], k["cin_src"], k["Cl"], k["taps"]
    src = torch.randn(N * cs * taps, generator=torch.Generator().manual_seed(N + cs + taps))
    got, form = eng.op_pack_weight(src, N, 3 * Cl if k["xp"] else Cl, taps, k["transposed"], k["geglu"], cs, k["xp"], k["dst_off"])
    assert form == k["form"], (form, k["form"])
    same_bits(f"pack_weight {name}", got, R.pack_weight(src, N, cs, Cl, taps, k["transposed"], k["geglu"], k["xp"], OPD))


def test_moves(eng):
    g = torch.Generator().manual_seed(9)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    w = rn(5, 12, 3, 3)
    same_bits("pack_upconv_weight", eng.op_move(0, w, None, (5, 12), 16, 5 * 12).reshape(16, 5, 12), R.pack_upconv_weight(w, OPD))
    b = rn(192)
    same_bits("permute_geglu_bias", eng.op_move(1, b, None, (192,), 1, 192, f32=True)[0], b[R.geglu_rows(192)])
    beta = rn(72)
    for split in (0, 1):
        same_bits(f"relu_beta_tile split={split}", eng.op_move(2, beta, None, (72, 3, split), 1, (3 if split else 1) * 216)[0], R.relu_beta_tile(beta, 3, split, OPD))
    vec = rn(40)
    same_bits("fill_rows_f16", eng.op_move(3, vec, None, (48, 7, 40), 7, 40, ld=48), vec.to(OPD).expand(7, 40))
    x = torch.full((9, 28), float("nan"))
    x[:, :20] = rn(9, 20)
    same_bits("rows_f32_to_f16", eng.op_move(4, x, None, (28, 9, 20), 9, 20), x[:, :20].to(OPD))
    img = torch.full((2 * 3 * 1, 12), float("nan"))
    img[:, :8] = rn(6, 8)
    same_bits("upsample2_f16", eng.op_move(5, img, None, (12, 2, 3, 1, 8), 2 * 6 * 2, 8).reshape(2, 6, 2, 8), R.upsample2(img[:, :8].reshape(2, 3, 1, 8), OPD))
    rows, add = torch.full((15, 12), float("nan")), rn(5, 8)
    rows[:, :8] = rn(15, 8)
    same_bits("add_image_rows", eng.op_move(6, rows, add, (12, 8, 3, 5, 16), 15, 8, ld=16, f32=True), rows[:, :8] + add.repeat(3, 1))
    r16 = R.r16(rn(37, 6), OPD)
    same_bits("rows_f16_to_nchw", eng.op_move(7, r16, None, (37, 6), 6, 37, f32=True), r16.T.contiguous())
    feats, grid = rn(11, 5), torch.randint(-1, 11, (70,), generator=g).int()
    grid[::7] = -1
    same_bits("sparse_densify", eng.op_move(8, feats, grid, (70, 5), 5, 70, f32=True), R.sparse_densify(feats, grid))


# ---- 6. folds -------------------------------------------------------------------------------------------------------------------------
def check_fold(label, got, ref, absum, K, out_f32):
    b32, b16 = R.fold_bounds(ref, absum, K, OPD)
    bound = b32 if out_f32 else b16
    err = (got.double().cpu() - ref).abs()
    worst = (err / bound).max().item()
    print(f"[parity] {label} {'fp32' if out_f32 else '16-bit'}: worst error / derived bound {worst:.3f}")
    assert torch.isfinite(got).all() and worst <= 1.0, (label, worst)


@pytest.mark.parametrize("heads,hd,Cc,I", R.FOLD_SHAPES)
def test_fold_qk_ov(eng, heads, hd, Cc, I):
    g = torch.Generator().manual_seed(heads * 1000 + hd * 100 + Cc + I)
    wq, wk, wv, wo = (torch.randn(*s, generator=g) for s in ((heads * hd, I), (heads * hd, Cc), (heads * hd, Cc), (I, heads * hd)))
    scale = float(torch.tensor(hd ** -0.5, dtype=torch.float32))
    qk, qk_abs = R.fold_qk(wq, wk, heads, hd, Cc, scale)
    ov, ov_abs = R.fold_ov(wo, wv, heads, hd, Cc)
    for out_f32 in (True, False):
        check_fold(f"fold_qk h{heads} hd{hd} Cc{Cc} I{I}", eng.op_fold(0, wq, wk, heads, hd, Cc, I, scale, out_f32=out_f32), qk, qk_abs, hd, out_f32)
        check_fold(f"fold_ov h{heads} hd{hd} Cc{Cc} I{I}", eng.op_fold(1, wo, wv, heads, hd, Cc, I, out_f32=out_f32), ov, ov_abs, hd, out_f32)


@pytest.mark.parametrize("M,N,K,lda,ldb,ldc", R.FOLD_MM)
def test_fold_mm(eng, M, N, K, lda, ldb, ldc):
    g = torch.Generator().manual_seed(M + N + K)
    a, b = torch.full((M, lda), float("nan")), torch.full((K, ldb), float("nan"))
    a[:, :K], b[:, :N] = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    ref, absum = R.fold_mm(a[:, :K], b[:, :N])
    for out_f32 in (True, False):
        got = eng.op_fold(2, a, b, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, out_f32=out_f32)
        check_fold(f"fold_mm {M}x{N}x{K}", got, ref, absum, K, out_f32)


# ---- 7. CFG assembly and DDIM update --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [8, 768])
@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("TN", [1, 3])
def test_cfg_assemble(eng, TN, copies, dim):
    B, HW = 2, 16
    g = torch.Generator().manual_seed(TN * 10 + copies)
    xn, xi, clip = torch.randn(B, TN, 4, HW, generator=g), torch.randn(B, 4, HW, generator=g), torch.randn(B, dim, generator=g)
    ts = torch.tensor([981, 21])
    xin, ctx, tt = eng.op_cfg_assemble(xn, xi, clip, ts.tolist(), copies)      # presets NaN / -1: an unwritten row shows
    wx, wc, wt = R.cfg_assemble(xn, xi, clip, ts, copies)
    same_bits("cfg input", xin, wx)
    same_bits("cfg context", ctx, wc)
    assert torch.equal(tt.cpu(), wt)
    if copies == 2:
        half = B * TN
        assert bool((bits(xin[half:, :, 4:].cpu()) == 0).all()) and bool((bits(ctx[half:].cpu()) == 0).all())


@pytest.mark.parametrize("n", R.DDIM_N)
def test_cfg_ddim(eng, n):
    g = torch.Generator().manual_seed(n)
    ec, eu, x, z = (torch.randn(n, generator=g) for _ in range(4))
    k = R.DDIM_COEF
    gots, r64, r32 = {}, {}, {}
    for has_eu, has_z, want_eps, want_x in itertools.product((0, 1), repeat=4):
        eps, xp = eng.op_cfg_ddim(ec, eu if has_eu else None, x, z if has_z else None, k, want_eps, want_x)   # None results: NULL pointers
        refs = [R.cfg_ddim(ec, eu if has_eu else None, x, z if has_z else None, k, dt) for dt in (torch.float64, torch.float32)]
        key = f"eu{has_eu} z{has_z} eps{want_eps} x{want_x}"
        if want_eps:
            gots[key + " eps"], r64[key + " eps"], r32[key + " eps"] = eps.cpu(), refs[0][0], refs[1][0]
        if want_x:
            gots[key + " x_prev"], r64[key + " x_prev"], r32[key + " x_prev"] = xp.cpu(), refs[0][1], refs[1][1]
    check(f"cfg_ddim n={n}", gots, r64, r32)


# ---- 8. small reductions and mixes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nv", R.FUSE_NV)
@pytest.mark.parametrize("n_views", [1, 3])
def test_fuse_views(eng, n_views, Nv):
    g = torch.Generator().manual_seed(n_views * 7 + Nv)
    vf, w, b, start = torch.randn(n_views, Nv, 16, generator=g), torch.randn(16, 16, generator=g) / 4, torch.randn(16, generator=g), torch.randn(Nv, 16, generator=g)
    gots, r64, r32 = {}, {}, {}
    for bias, acc in itertools.product((b, None), (0, 1)):
        got = eng.op_small_mix(0, vf, bias, w, (n_views, Nv, 16, acc), rows=Nv, width=16, start=start if acc else None)
        ref = [R.fuse_views(vf, w, bias, 16, dt) for dt in (torch.float64, torch.float32)]
        key = f"bias{int(bias is not None)} acc{acc}"
        gots[key] = minus(got, start) if acc else got.cpu()
        r64[key], r32[key] = (R.added(start, ref[0], torch.float64), R.added(start, ref[1], torch.float32)) if acc else ref
    check(f"fuse_views views={n_views} Nv={Nv}", gots, r64, r32)


@pytest.mark.parametrize("n", R.MSE_N)
def test_mse(eng, n):
    """fp64 differences, squares and sums, one rounding: within one fp32 ulp of the float64 mean"""
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    got = eng.op_small_mix(1, a, b, n=n)[0, 0].cpu().double()
    ref = R.mse(a, b)
    print(f"[parity] mse n={n}: |got - ref| / ulp32 = {(got - ref).abs().item() / R.ulp(ref, *R.FMT32).item():.3f}")
    assert (got - ref).abs() <= R.ulp(ref, *R.FMT32)


def test_exact_adds(eng):
    """accumulate_f32 and add_rows are one fp32 addition per element: bit-exact"""
    g = torch.Generator().manual_seed(12)
    for n in (4, 1028, 4100):
        a, start = torch.randn(n, generator=g), torch.randn(n, generator=g)
        same_bits(f"accumulate_f32 n={n}", eng.op_small_mix(2, a, n=n, rows=1, width=n, start=start[None])[0], start + a)
    for n in (1, 1027):
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        same_bits(f"add_rows n={n}", eng.op_small_mix(3, a, b, n=n, rows=1, width=n)[0], a + b)
        same_bits(f"add_rows n={n}, no b", eng.op_small_mix(3, a, None, n=n, rows=1, width=n)[0], a + 0.0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(eng):
    """null pointers, bad strides, unsupported shapes: non-zero with a message, and every result buffer still 0xFF"""
    d = R.encoder_inputs("random", 1)
    a, w = torch.randn(2, 8), torch.randn(4, 8)
    x = torch.randn(3, 4, 5)
    k = R.DDIM_COEF
    xn, xi, clip = torch.randn(1, 1, 4, 4), torch.randn(1, 4, 4), torch.randn(1, 8)
    cases = [
        ("null argument", lambda: eng.op_target_encoder(None, d["pre"], d["w"], d["bias"], d["gamma"], d["beta"], n=1)),
        ("null layer parameter", lambda: eng.op_target_encoder(d["x"], d["pre"], d["w"][:7] + [None], d["bias"], d["gamma"], d["beta"])),
        ("views expected", lambda: eng.op_target_encoder(d["x"], d["pre"], d["w"], d["bias"], d["gamma"], d["beta"], n=0)),
        ("null argument", lambda: eng.op_small_linear(a, None, None, 2)),
        ("act_in", lambda: eng.op_small_linear(a, w, None, 2, act=7)),
        ("lda >= K", lambda: eng.op_small_linear(a, w, None, 0)),
        ("bad argument", lambda: eng.op_timestep_embedding(torch.tensor([1]), 0)),
        ("op is 0", lambda: eng.op_layout(2, x, 3, 4, 5, 8, 8)),
        ("bad stride", lambda: eng.op_layout(0, x, 3, 4, 5, 8, 3)),
        ("bad argument", lambda: eng.op_pack_weight(torch.randn(5 * 8 * 28), 5, 8, 28, cin_src=8)),
        ("cin_src", lambda: eng.op_pack_weight(torch.randn(5 * 9 * 9), 5, 8, 9, cin_src=9)),
        ("N % 64", lambda: eng.op_pack_weight(torch.randn(5 * 8), 5, 8, 1, geglu=1, cin_src=8)),
        ("3 \\* Cl", lambda: eng.op_pack_weight(torch.randn(5 * 8), 5, 8, 1, cin_src=2, xp=1)),
        ("unknown op", lambda: eng.op_move(99, a, None, (1, 1), 2, 8)),
        ("bad stride", lambda: eng.op_move(3, a, None, (4, 2, 8), 2, 8)),
        ("multiples of 4", lambda: eng.op_move(4, torch.randn(2, 6), None, (6, 2, 6), 2, 6)),
        ("unknown op", lambda: eng.op_fold(3, a, w)),
        ("lda >= K", lambda: eng.op_fold(2, a, w, M=2, N=4, K=9, lda=8, ldb=8, ldc=4)),
        ("1 or 2 copies", lambda: eng.op_cfg_assemble(xn, xi, clip, [5], 3)),
        ("null argument", lambda: eng.op_cfg_assemble(xn, xi, clip, None, 2)),
        ("x with x_prev", lambda: eng.op_cfg_ddim(a.flatten(), None, None, None, k)),
        ("unknown op", lambda: eng.op_small_mix(9, a.flatten(), n=16, width=16)),
        ("bad argument", lambda: eng.op_small_mix(1, a.flatten(), None, n=16)),
        ("multiple of 4", lambda: eng.op_small_mix(2, a.flatten(), n=15, width=16, start=torch.zeros(1, 16))),
    ]
    for text, call in cases:
        with pytest.raises(L.MvdError, match=text) as info:
            call()
        assert info.value.results_untouched, text

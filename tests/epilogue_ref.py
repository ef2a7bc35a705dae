"""fp64 references of the forward kernels' epilogue, split-precision and slab forms, written from the reference model's definition
(not from the kernels), the torch-fp32 emulation of the split arithmetic, and the case tables of tests/test_gpu_epilogue_forms.py
with the conditions each case is built to meet (tests/test_epilogue_forms_cpu.py checks both without a GPU).  At the end: the same
for the 3-D convolutions of tests/test_gpu_conv3d_forms.py (checked by tests/test_conv3d_forms_cpu.py).

Order of a GEMM / conv epilogue:  out = act(alpha * acc + bias + rowbias[sample] + resid),  sample = row // rows_per_sample."""
import collections
import functools
import math
import re

import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------------------------------- references


def _act(v, act):
    return F.silu(v) if act == 1 else (F.relu(v) if act == 2 else v)


def epilogue(acc, B=1, alpha=1.0, bias=None, rowbias=None, resid=None, act=0):
    """acc [rows, N] (any float type) -> fp64 [rows, N]"""
    v = acc.double() * alpha
    rows, N = v.shape
    if bias is not None:
        v = v + bias.double()
    if rowbias is not None:
        v = v + rowbias.double().reshape(B, N).repeat_interleave(rows // B, 0)
    if resid is not None:
        v = v + resid.double().reshape(rows, N)
    return _act(v, act)


def linear(a, w, **epi):
    return epilogue(a.double() @ w.double().t(), **epi)


def conv(x, w, stride=1, upsample=0, tap_shift=0, B=None, alpha=1.0, bias=None, rowbias=None, resid=None, act=0):
    """x [B, Cin, H, W], w [Cout, Cin, k, k], rowbias [B, Cout], resid [B, Cout, Ho, Wo] -> fp64 [B, Cout, Ho, Wo].  tap_shift = 1: the
    first-stage encoder's Downsample, F.pad(x, (0, 1, 0, 1)) + conv(k3, s2, p0)."""
    x, w = x.double(), w.double()
    if upsample:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    if tap_shift:
        acc = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    else:
        acc = F.conv2d(x, w, stride=stride, padding=w.shape[2] // 2)
    v = acc * alpha
    if bias is not None:
        v = v + bias.double()[None, :, None, None]
    if rowbias is not None:
        v = v + rowbias.double()[:, :, None, None]
    if resid is not None:
        v = v + resid.double()
    return _act(v, act)


def slab_sum(slabs, bias=None, rowbias=None, T=None, resid=None):
    """sum(slabs [nslab, rows, C]) + bias [C] + rowbias[row // T] + resid [rows, C], fp64"""
    v = slabs.double().sum(0)
    if bias is not None:
        v = v + bias.double()
    if rowbias is not None:
        idx = torch.arange(v.shape[0]) // T
        v = v + rowbias.double()[idx]
    if resid is not None:
        v = v + resid.double()
    return v


def group_norm(slabs, groups, gamma, beta, eps, act=0, bias2=None, preadd=None, resid=None):
    """GroupNorm of sum(slabs [nslab, B, rows, C]) + bias2 [C] + preadd [B, C] + resid [B, rows, C], channels-last, fp64.
    Returns (normalised, the summed tensor)."""
    v = slabs.double().sum(0)
    if bias2 is not None:
        v = v + bias2.double()
    if preadd is not None:
        v = v + preadd.double()[:, None, :]
    if resid is not None:
        v = v + resid.double()
    B, rows, C = v.shape
    g = v.reshape(B, rows, groups, C // groups)
    mean = g.mean((1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((g - mean) / torch.sqrt(var + eps)).reshape(B, rows, C) * gamma.double() + beta.double()
    return _act(y, act), v


def layer_norm(slabs, gamma, beta, eps=1e-5, bias=None, rowbias=None, T=None, resid=None):
    """LayerNorm of slab_sum(...).  Returns (normalised, the summed rows), fp64."""
    v = slab_sum(slabs, bias, rowbias, T, resid)
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double(), v


def softmax(s):
    s = s.double()
    e = torch.exp(s - s.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


# ------------------------------------------------------------------------------------- the split arithmetic, emulated in torch fp32


def split16(x):
    """fp32 -> (hi, lo) fp16 with hi = fp16(x), lo = fp16(x - hi): hi + lo carries ~22 significand bits"""
    x = x.float()
    hi = x.half()
    return hi, (x - hi.float()).half()


def xp_linear_emulated(a, w):
    """Three products accumulated in fp32: a_hi w_hi + a_lo w_hi + a_hi w_lo (ConvW::xp, csrc/engine.h).  Never the kernel."""
    ah, al = split16(a)
    wh, wl = split16(w)
    ah, al, wh, wl = ah.float(), al.float(), wh.float(), wl.float()
    return ah @ wh.t() + al @ wh.t() + ah @ wl.t()


def xp_conv_emulated(x, w, stride=1, tap_shift=0):
    xh, xl = split16(x)
    wh, wl = split16(w)
    xh, xl, wh, wl = xh.float(), xl.float(), wh.float(), wl.float()
    if tap_shift:
        f = lambda u, v: F.conv2d(F.pad(u, (0, 1, 0, 1)), v, stride=2)
    else:
        f = lambda u, v: F.conv2d(u, v, stride=stride, padding=w.shape[2] // 2)
    return f(xh, wh) + f(xl, wh) + f(xh, wl)


def rel_l2(got, want):
    got, want = got.double(), want.double()
    return ((got - want).norm() / (want.norm() + 1e-300)).item()


# ------------------------------------------------------------------------------------------------------------------ test data


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(1000 * seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def ints64(*shape, seed=0, span=61):
    """asymmetric integers / 64 in (-span/128, span/128): exact in fp16, and every sum the tests form of them is exact in fp32"""
    n = math.prod(shape)
    i = torch.arange(n, dtype=torch.int64)
    v = (i * (2 * seed + 7) + (i // shape[-1]) * (6 * seed + 13) + 5 * seed) % span - span // 2
    return (v.double() / 64.0).float().reshape(*shape)


def binary(*shape, seed=0, density=0.15):
    """0 / 1 / 2 operands: with ints64 weights every product and every partial sum is exact in fp16 x fp16 -> fp32"""
    g = torch.Generator().manual_seed(77 + seed + sum(shape))
    u = torch.rand(*shape, generator=g)
    return (u < density).float() + (u < density / 4).float()


# ---------------------------------------------------------------------------------------------- cases and what each is built to reach
# Kernel families as mvd_probe_report names them; `bn` (the column-tile width) is the planner's and is left open.
FAMILY = {
    "dense": r"gemm_dma_kernel<(64|128|160),0>",        # LDS-DMA GEMM, 256-row tiles
    "dense128": r"gemm_dma_kernel<128x(96|128|160)>",   # ... four-wave 128-row tiles (MVD_DENSE_BM / MVD_DENSE_BN)
    "gather_f32": r"igemm_kernel<1,(64|128|160)>",      # register-staged gather kernel, fp32 source
    "gather_f16": r"igemm_kernel<0,(64|128|160)>",      # ... fp16 source
    "halo": r"conv3_dma_kernel<(128|160),(8,8|16,16)>",
    "conv3x": r"conv3x_kernel<(4|5)>",
}
DENSE_MIN_M = 64  # env.h: fewest rows routed to the LDS-DMA kernel


def family_matches(name, family):
    return re.fullmatch(FAMILY[family], name) is not None


# (samples, rows per sample) of the exact epilogue tests and what each geometry is for
SAMPLE_GEOMETRIES = [
    (16, 16),    # many samples inside one 256-row tile
    (32, 16),    # ... in each of two tiles
    (6, 48),     # rows per sample % 32 != 0: the accumulator pre-load ("folded") form must NOT be taken
    (3, 96),     # folded, and the waves of one tile belong to different samples
    (5, 32),     # ragged last tile (160 rows)
    (2, 1024),   # whole tiles inside one sample
]
LINEAR_K = 128       # two k-steps: the smallest K a forced split-K of 2 can split
LINEAR_NS = [(72, 80), (200, 208)]  # (N, rb_ld): a column tail at every tile width, per-sample rows wider than N


def linear_family_ok(family, rows, K, N, a_half, xp=False, rb_ld=0):
    """The planner's routing of a plain GEMM (engine_unet.hip igemm_go, k_gemm.hip gemm_dma_eligible), restated."""
    f16_src = a_half or xp
    dense_ok = f16_src and rows >= DENSE_MIN_M and K % 8 == 0 and N % 4 == 0 and rb_ld % 4 == 0
    if family in ("dense", "dense128"):
        return dense_ok
    if family == "gather_f32":
        return not f16_src
    if family == "gather_f16":
        return f16_src and not dense_ok
    return False


def folded_expected(rps, alpha, sk, has_bias_or_rowbias=True):
    """k_gemm.hip / k_igemm.hip: the accumulators start at bias + rowbias only for alpha == 1, no split and rps % 32 == 0"""
    return alpha == 1.0 and sk <= 1 and rps % 32 == 0 and has_bias_or_rowbias


# 3x3 stride-1 convolutions with a per-sample bias: (name, B, Cin, H, W, Cout, a_half, conv3x stream offered, family)
CONV_CASES = [
    ("8x8 B=6 conv3x", 6, 64, 8, 8, 128, True, True, "conv3x"),     # four images per tile, partial last tile
    ("8x8 B=6 halo", 6, 64, 8, 8, 128, True, False, "halo"),        # ... b_first != b_last: per-row sample index
    ("16x16 B=3 conv3x", 3, 64, 16, 16, 160, True, True, "conv3x"),
    ("16x16 B=3 halo", 3, 64, 16, 16, 160, True, False, "halo"),    # one image per tile: the folded form
    ("4x4 B=32 dense", 32, 64, 4, 4, 72, True, False, "dense"),     # dense tap-gather kernel, 16 rows per sample
    ("7x5 B=4 gather", 4, 64, 7, 5, 40, False, False, "gather_f32"),  # fp32 source, ragged everything
]


def conv_family_ok(family, B, Cin, H, W, Cout, a_half, conv3x, xp=False, stride=1, out_f16=False, alpha=1.0, act=0, out_split=False):
    """igemm_go's routing of a 3x3 convolution, restated (k_conv3x.hip conv3x_eligible, k_conv3.hip conv3_halo_eligible)."""
    f16_src = a_half or xp
    Cp = 3 * Cin if xp else Cin
    shape_ok = f16_src and stride == 1 and Cp % 64 == 0 and ((H % 16 == 0 and W % 16 == 0) or (H == 8 and W == 8))
    x_ok = shape_ok and conv3x and (Cout % 160 == 0 or Cout % 128 == 0) and not out_f16 and alpha == 1.0 and act == 0 and not out_split
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dense_ok = f16_src and not shape_ok and DENSE_MIN_M <= B * Ho * Wo <= 16384 and Cout % 4 == 0
    if family == "conv3x":
        return x_ok
    if family == "halo":
        return shape_ok and not x_ok
    if family == "dense":
        return dense_ok
    if family == "gather_f32":
        return not f16_src
    if family == "gather_f16":
        return f16_src and not shape_ok and not dense_ok
    return False


# tap_shift = 1 (stride 2, zero padding right / bottom): even sides only -- the encoder's only use
TAP_SHIFT_SHAPES = [(8, 8), (6, 10), (16, 4)]

# Extended precision: name -> (kind, parameters).  linear: (rows, K, N); conv: (B, Cin, H, W, Cout, ksize, stride, tap_shift)
XP_CASES = {
    "linear K=320": ("linear", (256, 320, 320)),
    "linear K=1280": ("linear", (128, 1280, 320)),
    "conv1x1 64->128 16x16": ("conv", (2, 64, 16, 16, 128, 1, 1, 0)),
    "conv3x3 64->64 16x16": ("conv", (2, 64, 16, 16, 64, 3, 1, 0)),
    "conv3x3 64->64 8x8": ("conv", (4, 64, 8, 8, 64, 3, 1, 0)),
    "conv3x3 320->320 16x16": ("conv", (1, 320, 16, 16, 320, 3, 1, 0)),
    "conv3x3 320->320 8x8": ("conv", (4, 320, 8, 8, 320, 3, 1, 0)),
    "conv3x3 s2 padded 64->64 16x16": ("conv", (2, 64, 16, 16, 64, 3, 2, 1)),
}

# the kernel families each extended-precision case can reach through the hooks (conv3x: with the fragment stream offered)
XP_FAMILIES = {
    "linear K=320": ["dense"], "linear K=1280": ["dense"], "conv1x1 64->128 16x16": ["dense"],
    "conv3x3 64->64 16x16": ["halo"], "conv3x3 64->64 8x8": ["halo"],
    "conv3x3 320->320 16x16": ["conv3x", "halo"], "conv3x3 320->320 8x8": ["conv3x", "halo"],
    "conv3x3 s2 padded 64->64 16x16": ["dense"],
}


def xp_operands(name):
    kind, p = XP_CASES[name]
    seed = sorted(XP_CASES).index(name)
    if kind == "linear":
        rows, K, N = p
        return rnd(rows, K, seed=seed), rnd(N, K, seed=seed + 50, scale=K ** -0.5)
    B, Cin, H, W, Cout, k, _, _ = p
    return rnd(B, Cin, H, W, seed=seed), rnd(Cout, Cin, k, k, seed=seed + 50, scale=(Cin * k * k) ** -0.5)


@functools.lru_cache(maxsize=None)
def xp_reference(name):
    """(fp64 result of the unrounded operands, relL2 of the three-product fp32 emulation, relL2 of the plain fp16-operand product)"""
    kind, p = XP_CASES[name]
    a, w = xp_operands(name)
    if kind == "linear":
        want = linear(a, w)
        emu = xp_linear_emulated(a, w)
        plain = a.half().float() @ w.half().float().t()
    else:
        stride, ts = p[6], p[7]
        want = conv(a, w, stride=stride, tap_shift=ts)
        emu = xp_conv_emulated(a, w, stride=stride, tap_shift=ts)
        plain = conv(a.half().float(), w.half().float(), stride=stride, tap_shift=ts)
    return want, rel_l2(emu, want), rel_l2(plain, want)


# GroupNorm consumer: (B, rows, C, G) per register tile of launch_gn_group (n2 = rows * (C / G) / 2 pairs per workgroup) ...
GN_TILE_CASES = [
    (2, 128, 64, 4),     # n2 = 1024: the last size of <256, 4>
    (1, 205, 40, 4),     # n2 = 1025, cpg = 10: the first of <512, 4>
    (1, 256, 64, 4),     # n2 = 2048: the last of <512, 4>
    (1, 256, 320, 8),    # n2 = 5120, cpg = 40: the last of <512, 10>
    (1, 1024, 64, 4),    # n2 = 8192: the last of <512, 16>
    (1, 256, 640, 8),    # n2 = 10240, cpg = 80: the last of <1024, 10>
    (1, 1024, 128, 4),   # n2 = 16384: the last of <1024, 16>
    (2, 64, 160, 8),     # cpg = 20
    (2, 64, 240, 8),     # cpg = 30
]
GN_REMAINDER_CASE = (3, 64, 20, 5)  # B * G = 15 workgroups: the XCD remap's remainder branch
GN_NSLABS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16]


def gn_tile_of(rows, C, G):
    """(threads, pairs per thread) launch_gn_group picks (k_norm.hip)"""
    n2 = rows * (C // G) // 2
    for nt, me in ((256, 4), (512, 4), (512, 10), (512, 16), (1024, 10)):
        if n2 <= nt * me:
            return nt, me
    return 1024, 16


def gn_group_eligible(ld, rows, C, G, pld, ldo):
    cpg = C // G
    return C % G == 0 and cpg % 2 == 0 and cpg <= 256 and ld % 2 == 0 and ldo % 2 == 0 and pld % 2 == 0 and rows * cpg <= 32768


# LayerNorm consumer: (rows, C, T) -- rows per workgroup = 4 * 64 / (C / 40) = 32 / 16 / 8 / 4; rows = samples * T, so that the
# producing GEMM (per-sample bias by row // T) can be run on the same rows
LN_CASES = [(70, 320, 35), (39, 640, 13), (21, 1280, 7), (9, 2560, 3)]


def ln_rows_per_workgroup(C):
    return 4 * (64 // (C // 40))
LN_NSLABS = [1, 2, 5]

# folded GroupNorm: (B, rps, K, N, cpg)
FOLDED_GN_CASES = [(2, 256, 64, 64, 8), (2, 512, 64, 192, 16), (2, 256, 64, 256, 32), (2, 512, 64, 256, 8), (2, 256, 64, 192, 8)]

SOFTMAX_COLS = [1, 255, 256, 257, 1000, 4096]


def softmax_scores(cols):
    """four rows: magnitude 1e4, one peaked, all equal, ordinary"""
    s = rnd(4, cols, seed=cols)
    s[0] = s[0] * 1e4
    s[1] = s[1] * 0.1
    s[1, (7 * cols) // 11] = 30.0
    s[2] = 3.25
    return s


# -------------------------------------------------------------------------------------- 3-D convolutions (tests/test_gpu_conv3d_forms.py)
# run_conv3d / run_convT3d (csrc/engine_unet.hip) as the two 3-D U-nets launch them: out = acc + bias + resid on the output grid.

CONV3D_DMA_MAX_M = 16384  # igemm_go: a multi-tap launch with more rows stays on the 128-row gather kernel
CONVT3D_BATCH_MIN_ROWS = 512  # run_convT3d: fewer input rows launch one GEMM per output-parity class


def conv3d(x, w, stride=1, transposed=False, bias=None, resid=None):
    """x [B, Cin, D, H, W]; w [Cout, Cin, 3, 3, 3] (Conv3d k3 p1) or, transposed, [Cin, Cout, 3, 3, 3] (ConvTranspose3d k3 s2 p1 op1);
    bias [Cout], resid on the output grid -> fp64 [B, Cout, Do, Ho, Wo]"""
    x, w = x.double(), w.double()
    if transposed:
        v = F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    else:
        v = F.conv3d(x, w, stride=stride, padding=1)
    if bias is not None:
        v = v + bias.double()[None, :, None, None, None]
    if resid is not None:
        v = v + resid.double()
    return v


def conv3d_out_dims(kind, dims):
    if kind == "T":
        return tuple(2 * n for n in dims)
    s = 2 if kind == "s2" else 1
    return tuple((n - 1) // s + 1 for n in dims)


def conv3d_rows(kind, B, dims):
    """the GEMM rows of a launch, which the routing goes by: output voxels, or for the transposed conv (whose classes each
    produce one output voxel per INPUT voxel) input voxels"""
    return B * math.prod(dims if kind == "T" else conv3d_out_dims(kind, dims))


def _conv3d_route(M, ntaps, Cin, Cout, a_half, ldc, ldr):
    """igemm_go for one launch of M rows and ntaps taps (k_gemm.hip gemm_dma_eligible; no 3-D launch is halo- or conv3x-eligible)"""
    if not a_half:
        return "gather_f32"
    dense = (DENSE_MIN_M <= M and (ntaps == 1 or M <= CONV3D_DMA_MAX_M) and Cin % 8 == 0 and Cout % 4 == 0 and ldc % 4 == 0
             and ldr % 4 == 0)
    return "dense" if dense else "gather_f16"


def convT3d_launches(B, Cin, Cout, dims, a_half, force_splitk=0, ldc=0, ldr=0):
    """run_convT3d restated: [(family, taps)] per launch -- one parity-batched launch of the LDS-DMA kernel, or the eight classes
    (pz, py, px) with (1 + pz)(1 + py)(1 + px) taps, each routed like a convolution of its own over the input rows"""
    M = B * math.prod(dims)
    ldc = ldc or Cout
    eligible = a_half and Cin % 8 == 0 and Cout % 4 == 0 and ldc % 4 == 0 and ldr % 4 == 0
    if eligible and force_splitk <= 1 and M >= CONVT3D_BATCH_MIN_ROWS:
        return [("dense", 8)]
    out = []
    for par in range(8):
        taps = (1 + (par >> 2)) * (1 + ((par >> 1) & 1)) * (1 + (par & 1))
        out.append((_conv3d_route(M, taps, Cin, Cout, a_half, ldc, ldr), taps))
    return out


def conv3d_launches(kind, B, Cin, Cout, dims, a_half, force_splitk=0, ldc=0, ldr=0):
    if kind == "T":
        return convT3d_launches(B, Cin, Cout, dims, a_half, force_splitk, ldc, ldr)
    return [(_conv3d_route(conv3d_rows(kind, B, dims), 27, Cin, Cout, a_half, ldc or Cout, ldr), 27)]


def conv3d_family_ok(family, kind, B, Cin, Cout, dims, a_half, force_splitk=0, ldc=0, ldr=0):
    """every launch of the layer runs on `family`"""
    return all(f == family for f, _ in conv3d_launches(kind, B, Cin, Cout, dims, a_half, force_splitk, ldc, ldr))


def conv3d_reduce_launches(kind, B, Cin, Cout, dims, a_half, force_splitk=0, ldc=0, ldr=0):
    """splitk_reduce_kernel launches of a FORCED split (plan_dense / plan_gather: sk = min(force_splitk, k-steps), a k-step being one
    tap of up to 64 channels): one per launch with at least two k-steps; the parity-batched launch never splits"""
    launches = conv3d_launches(kind, B, Cin, Cout, dims, a_half, force_splitk, ldc, ldr)
    if kind == "T" and len(launches) == 1:
        return 0
    return sum(1 for _, taps in launches if min(force_splitk, taps * ((Cin + 63) // 64)) > 1)


def igemm_pick_bn(N):
    """k_igemm.hip: the column-tile width of a launch that is not a plain GEMM"""
    if N <= 64:
        return 64
    return 160 if -(-N // 160) * 160 < -(-N // 128) * 128 else 128


def parity_batch_nch(M, Cin, Cout, npar=8, kmax=8):
    """go_parity_batch -> gemm_dma_plan (k_gemm.hip), restated: the column tiles one workgroup walks.  Cost in k-steps per round of
    256 workgroups: nch * ksteps + 4 + 2 nch."""
    bn, ksteps = igemm_pick_bn(Cout), kmax * ((Cin + 63) // 64)
    tiles_m, tiles_n = -(-M * npar // 256), -(-Cout // bn)
    best, best_nch = None, 1
    for nch in range(1, tiles_n + 1):
        cost = -(-tiles_m * -(-tiles_n // nch) // 256) * (nch * ksteps + 4 + 2 * nch)
        if best is None or cost < best:
            best, best_nch = cost, nch
    return best_nch


def conv3d_cell(case):
    """the routing cell a case is in: (stride 1 | stride 2 | transposed batched | transposed unbatched, family)"""
    if case.kind != "T":
        return case.kind, case.family
    return ("T batched" if case.launches == 1 else "T unbatched"), case.family


# the cells igemm_go / run_convT3d allow: the parity-batched launch is always the LDS-DMA kernel's
CONV3D_CELLS = {(k, f) for k in ("s1", "s2", "T unbatched") for f in ("dense", "gather_f16", "gather_f32")} | {("T batched", "dense")}

Conv3dCase = collections.namedtuple(
    "Conv3dCase", "name kind B Cin Cout dims a_half force_splitk in_place out_f16 ldc_pad family launches reduces density span")


def _c3(name, kind, B, Cin, Cout, dims, a_half, family, launches=1, reduces=0, force_splitk=0, in_place=False, out_f16=False, ldc_pad=0,
        density=0.15, span=61):
    return Conv3dCase(name, kind, B, Cin, Cout, dims, a_half, force_splitk, in_place, out_f16, ldc_pad, family, launches, reduces, density,
                      span)


# Exact-arithmetic cases.  force_splitk = 0 in the table is passed as 1 (the kernel's own epilogue; the planner's split of a small
# launch is its own choice and is left to the random-operand cases); 2 forces the reduce pass.  A 16-bit result lowers the density
# and the span until the reference is representable in fp16 AND bfloat16 (tests/test_conv3d_forms_cpu.py).
CONV3D_CASES = [
    # ---- stride 1
    _c3("s1 gather_f16 17x32x32 72->40 above 16384 rows", "s1", 1, 72, 40, (17, 32, 32), True, "gather_f16"),
    _c3("s1 dense 16x32x32 16->8 exactly 16384 rows", "s1", 1, 16, 8, (16, 32, 32), True, "dense"),
    _c3("s1 gather_f16 3x4x4 64->40 48 rows", "s1", 1, 64, 40, (3, 4, 4), True, "gather_f16"),
    _c3("s1 dense 4x4x4 64->40 exactly 64 rows", "s1", 1, 64, 40, (4, 4, 4), True, "dense"),
    _c3("s1 dense B=3 5x7x9 16->40", "s1", 3, 16, 40, (5, 7, 9), True, "dense"),
    _c3("s1 dense B=3 5x7x9 48->200 ldc", "s1", 3, 48, 200, (5, 7, 9), True, "dense", ldc_pad=12),
    _c3("s1 dense B=3 5x7x9 72->320", "s1", 3, 72, 320, (5, 7, 9), True, "dense"),
    _c3("s1 dense B=5 1x3x5 64->40 extent 1", "s1", 5, 64, 40, (1, 3, 5), True, "dense"),
    _c3("s1 dense B=3 5x7x9 128->40 split-K", "s1", 3, 128, 40, (5, 7, 9), True, "dense", reduces=1, force_splitk=2),
    _c3("s1 dense B=3 5x7x9 48->40 in place f16 out", "s1", 3, 48, 40, (5, 7, 9), True, "dense", in_place=True, out_f16=True, ldc_pad=8,
        density=0.02, span=5),
    _c3("s1 gather_f32 B=3 5x7x9 24->40", "s1", 3, 24, 40, (5, 7, 9), False, "gather_f32"),
    _c3("s1 gather_f32 B=3 5x7x9 128->200 split-K ldc", "s1", 3, 128, 200, (5, 7, 9), False, "gather_f32", reduces=1, force_splitk=2,
        ldc_pad=4),
    # ---- stride 2: odd extents ((n - 1) / 2 + 1 outputs), extent 1, one output voxel
    _c3("s2 gather_f16 51x53x51 16->8 above 16384 rows", "s2", 1, 16, 8, (51, 53, 51), True, "gather_f16"),
    _c3("s2 dense B=3 5x7x9 16->40", "s2", 3, 16, 40, (5, 7, 9), True, "dense"),
    _c3("s2 dense B=3 5x7x9 48->200", "s2", 3, 48, 200, (5, 7, 9), True, "dense"),
    _c3("s2 dense B=3 5x7x9 72->320 ldc", "s2", 3, 72, 320, (5, 7, 9), True, "dense", ldc_pad=4),
    _c3("s2 dense B=11 1x3x5 64->40 extent 1", "s2", 11, 64, 40, (1, 3, 5), True, "dense"),
    _c3("s2 gather_f16 B=2 1x3x5 64->40 extent 1", "s2", 2, 64, 40, (1, 3, 5), True, "gather_f16"),
    _c3("s2 gather_f16 B=2 2x2x2 72->40 one voxel", "s2", 2, 72, 40, (2, 2, 2), True, "gather_f16"),
    _c3("s2 gather_f32 B=3 5x7x9 24->40", "s2", 3, 24, 40, (5, 7, 9), False, "gather_f32"),
    _c3("s2 gather_f32 B=2 2x2x2 24->40 one voxel", "s2", 2, 24, 40, (2, 2, 2), False, "gather_f32"),
    # ---- transposed, all eight parity classes in one launch
    _c3("T batched B=2 4x8x8 64->200 exactly 512 rows", "T", 2, 64, 200, (4, 8, 8), True, "dense"),
    _c3("T batched B=2 4x8x8 64->320", "T", 2, 64, 320, (4, 8, 8), True, "dense"),
    _c3("T batched B=2 6x16x24 64->200 column walk", "T", 2, 64, 200, (6, 16, 24), True, "dense"),
    _c3("T batched B=1 5x7x15 48->40 in place", "T", 1, 48, 40, (5, 7, 15), True, "dense", in_place=True),
    _c3("T batched B=2 4x8x8 64->40 in place f16 out ldc (level-0 form)", "T", 2, 64, 40, (4, 8, 8), True, "dense", in_place=True,
        out_f16=True, ldc_pad=8, density=0.02, span=5),
    _c3("T batched B=2 4x8x8 72->200 f16 out", "T", 2, 72, 200, (4, 8, 8), True, "dense", out_f16=True, density=0.02, span=5),
    # ---- transposed, one launch per parity class
    _c3("T unbatched 6x7x12 64->40 504 rows", "T", 1, 64, 40, (6, 7, 12), True, "dense", launches=8),
    _c3("T unbatched 6x7x12 64->40 fp32 source", "T", 1, 64, 40, (6, 7, 12), False, "gather_f32", launches=8),
    _c3("T unbatched B=2 4x8x8 128->40 split-K", "T", 2, 128, 40, (4, 8, 8), True, "dense", launches=8, reduces=8, force_splitk=2),
    _c3("T unbatched B=2 4x8x8 64->200 split-K fp32 source", "T", 2, 64, 200, (4, 8, 8), False, "gather_f32", launches=8, reduces=7,
        force_splitk=2),
    _c3("T unbatched B=2 2x3x4 72->40 48 rows", "T", 2, 72, 40, (2, 3, 4), True, "gather_f16", launches=8),
    _c3("T unbatched 6x7x12 48->40 fp32 source in place f16 out ldc", "T", 1, 48, 40, (6, 7, 12), False, "gather_f32", launches=8,
        in_place=True, out_f16=True, ldc_pad=8, density=0.02, span=5),
]
CONV3D_BY_NAME = {c.name: c for c in CONV3D_CASES}


def conv3d_ld(case):
    """(ldc, ldr) of a case: the residual rows are padded whenever the result rows are"""
    return case.Cout + case.ldc_pad, case.Cout + (4 if case.ldc_pad else 0)


def conv3d_operands(case):
    """(x, w, bias, resid) with every product and every partial sum exact in 16-bit x 16-bit -> fp32"""
    T = case.kind == "T"
    seed = CONV3D_CASES.index(case) % 5
    small = case.out_f16
    x = binary(case.B, case.Cin, *case.dims, seed=seed, density=case.density)
    w = ints64(*((case.Cin, case.Cout) if T else (case.Cout, case.Cin)), 3, 3, 3, seed=1, span=case.span)
    od = conv3d_out_dims(case.kind, case.dims)
    return x, w, ints64(case.Cout, seed=2, span=7 if small else 47), ints64(case.B, case.Cout, *od, seed=4, span=9 if small else 59)


@functools.lru_cache(maxsize=None)
def conv3d_reference(name):
    case = CONV3D_BY_NAME[name]
    x, w, bias, resid = conv3d_operands(case)
    return conv3d(x, w, stride=2 if case.kind == "s2" else 1, transposed=case.kind == "T", bias=bias, resid=resid)

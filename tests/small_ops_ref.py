"""Plain restatements of the small-op layer (csrc/k_misc.hip, csrc/k_enc.hip, the element-wise kernels of csrc/k_cond.hip and the
samplers' batch assembly in csrc/c_api.hip), evaluated in the dtype asked for: float64 is the reference of
tests/test_gpu_small_ops.py, float32 gives the error a float32 evaluation has anyway (its bound).  The pure moves and packs are
restated with torch indexing (tests/test_small_ops_cpu.py holds them against slow index loops).  Also the launchers' path
predicates restated, the case tables of the two test files, and their seeded inputs.

`opd` is the library's 16-bit operand type (torch.float16, or torch.bfloat16 for the bf16 build)."""
import functools
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_SILU = 0, 1


def errs(got, want):
    """(relative L2, max |error| / max |reference|) against a float64 reference"""
    d = got.detach().cpu().double() - want
    return (d.norm() / (want.norm() + 1e-300)).item(), (d.abs().max() / (want.abs().max() + 1e-300)).item()


def added(start, r, dtype):
    """what an evaluation in `dtype` adds to `start` (the difference taken exactly)"""
    return (start.to(dtype) + r.to(dtype)).double() - start.double()


def r16(t, opd):
    """one rounding to the 16-bit operand type, back in t's dtype"""
    return t.to(opd).to(t.dtype)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1. target encoder --------------------------------------------------------------------------------------------------------------
ENC_VIEWS = (1, 3, 16)
ENC_FAMILIES = ("random", "impulse", "offset")
ENC_IMPULSES = ((0, 0), (0, 31), (31, 0), (31, 31), (0, 16), (13, 7))  # the four corners, one mid-edge, one interior pixel


def encoder(x, pre, w, bias, gamma, beta, dtype, opd, final_operand=False):
    """NoisyTargetViewEncoder: init conv, three blocks h + conv(silu(gn(conv(silu(gn(h + pre_i)))))), silu(gn), final conv; every conv
    operand (weights; the latent and each norm+SiLU output) rounded to `opd` -- seven norm outputs plus the latent (opd None: nowhere).
    x [n, 4, 32, 32], pre [n, 48] -> [n * 1024, 16] channels-last.  final_operand: the last norm+SiLU output before its rounding."""
    rnd = (lambda t: t) if opd is None else (lambda t: r16(t, opd))
    c = lambda t: t.to(dtype)  # noqa: E731
    conv = lambda a, i: F.conv2d(rnd(a), rnd(c(w[i])), c(bias[i]), padding=1)  # noqa: E731
    gn = lambda u, i: F.silu(F.group_norm(u, 8, c(gamma[i]), c(beta[i]), 1e-5))  # noqa: E731
    h = conv(c(x), 0)
    for i in range(3):
        t = conv(gn(h + c(pre)[:, 16 * i:16 * i + 16, None, None], 2 * i), 1 + 2 * i)
        h = conv(gn(t, 2 * i + 1), 2 + 2 * i) + h
    out = gn(h, 6) if final_operand else conv(gn(h, 6), 7)
    return out.permute(0, 2, 3, 1).reshape(-1, 16)


@functools.lru_cache(maxsize=None)
def encoder_inputs(family, n=16):
    """-> dict(x, pre, w[8], bias[8], gamma[7], beta[7]), the same for every n <= 16 (views are rows of the 16-view draw)"""
    g = _gen(100 + ENC_FAMILIES.index(family))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    w = [rn(16, 4 if i == 0 else 16, 3, 3) * (1.2 / math.sqrt(9 * (4 if i == 0 else 16))) for i in range(8)]
    bias = [0.2 * rn(16) for _ in range(8)]
    gamma = [1 + 0.3 * rn(16) for _ in range(7)]
    beta = [0.3 * rn(16) for _ in range(7)]
    x, pre = rn(16, 4, 32, 32), 0.5 * rn(16, 48)
    if family == "impulse":
        # a few lit pixels through the first conv alone: the blocks' second convs are zero, so h stays conv0(x); the final conv is the
        # centre-tap identity, so the result is silu(gn(conv0(x))) pixel by pixel -- a tap, halo or pixel-map slip moves the pattern
        x = torch.zeros(16, 4, 32, 32)
        for v in range(16):
            for k, (py, px) in enumerate(ENC_IMPULSES):
                x[v, :, py, px] = rn(4) + (k + 1) * (1 if (v + k) % 2 else -1)
        pre = torch.zeros(16, 48)
        for i in (2, 4, 6):
            w[i], bias[i] = torch.zeros(16, 16, 3, 3), torch.zeros(16)
        w[7], bias[7] = torch.zeros(16, 16, 3, 3), torch.zeros(16)
        w[7][torch.arange(16), torch.arange(16), 1, 1] = 1.0
    elif family == "offset":
        # the FiLM regime: activations of standard deviation 0.5, a pre-add of +-4 on both channels of a group: |mean| / std = 8
        w[0] = rn(16, 4, 3, 3) * (0.5 / 6.0)
        bias[0] = 0.05 * rn(16)
        sign = torch.where(torch.rand(16, 24, generator=g) < 0.5, -1.0, 1.0)
        pre = 4.0 * sign.repeat_interleave(2, dim=1)
    return dict(x=x[:n].contiguous(), pre=pre[:n].contiguous(), w=w, bias=bias, gamma=gamma, beta=beta)


def encoder_reference(family, dtype, opd):
    d = encoder_inputs(family)
    return encoder(d["x"], d["pre"], d["w"], d["bias"], d["gamma"], d["beta"], dtype, opd)


_ENC_CACHE = {}


def encoder_refs(family, opd):
    """(float64, float32) references of the 16-view draw, computed once per (family, type)"""
    key = (family, opd)
    if key not in _ENC_CACHE:
        _ENC_CACHE[key] = (encoder_reference(family, torch.float64, opd), encoder_reference(family, torch.float32, opd))
    return _ENC_CACHE[key]


# ---- 2. small linear ------------------------------------------------------------------------------------------------------------------
def small_linear_form(K, lda, a_off=0):
    """small_linear_form (csrc/k_misc.hip): 1 the 16-byte path, 0 the scalar path; a_off: floats between a 16-byte boundary and `a` (the
    weights are a workspace allocation: aligned)"""
    return int(K % 8 == 0 and lda % 4 == 0 and a_off % 4 == 0)


# name: K, lda, rows (< 0: broadcast), N, act, accumulate, ldo, bias, a_off, form
SL_FIELDS = ("K", "lda", "rows", "N", "act", "accum", "ldo", "bias", "a_off", "form")
SL_CASES = {k: dict(zip(SL_FIELDS, v)) for k, v in {
    "vec_k8_r1": (8, 8, 1, 48, ACT_NONE, 0, 48, 1, 0, 1),            # most lanes idle
    "vec_k256_r8_silu": (256, 256, 8, 6, ACT_SILU, 0, 6, 1, 0, 1),   # one full pass; N % 4 = 2
    "vec_k520_r9_acc": (520, 524, 9, 48, ACT_NONE, 1, 52, 1, 0, 1),  # lane 0 takes a second trip; second pass of one row; pad columns
    "vec_k1280_r17": (1280, 1280, 17, 1, ACT_SILU, 0, 1, 0, 0, 1),   # third pass of one row; one column; no bias
    "sc_k4_r1": (4, 4, 1, 48, ACT_NONE, 0, 48, 1, 0, 0),
    "sc_k12_r9_silu": (12, 12, 9, 6, ACT_SILU, 1, 8, 1, 0, 0),
    "sc_lda_r17": (256, 257, 17, 6, ACT_NONE, 0, 6, 0, 0, 0),        # lda = K + 1
    "sc_aoff_r8": (256, 256, 8, 48, ACT_SILU, 0, 48, 1, 1, 0),       # `a` one float past a 16-byte boundary
    "bc_vec_1": (256, 256, -1, 48, ACT_NONE, 0, 48, 1, 0, 1),
    "bc_vec_16_acc": (520, 520, -16, 6, ACT_SILU, 1, 8, 1, 0, 1),
    "bc_vec_65": (8, 8, -65, 1, ACT_NONE, 0, 1, 0, 0, 1),            # more rows than the 64 lanes that write
    "bc_sc_65": (12, 13, -65, 6, ACT_SILU, 0, 6, 1, 0, 0),
}.items()}


@functools.lru_cache(maxsize=None)
def small_linear_inputs(name, opd):
    c = SL_CASES[name]
    g = _gen(200 + list(SL_CASES).index(name))
    in_rows, out_rows = (1, -c["rows"]) if c["rows"] < 0 else (c["rows"], c["rows"])
    a = torch.randn(in_rows, c["K"], generator=g) * 1.5
    w = r16(torch.randn(c["N"], c["K"], generator=g) / math.sqrt(c["K"]), opd)  # rounded on both sides
    bias = torch.randn(c["N"], generator=g) if c["bias"] else None
    start = 3 * torch.randn(out_rows, c["N"], generator=g) if c["accum"] else None
    return dict(a=a, w=w, bias=bias, start=start)


def small_linear(a, w, bias, rows, act, dtype):
    a, w = a.to(dtype), w.to(dtype)
    if act == ACT_SILU:
        a = a * torch.sigmoid(a)
    out = a @ w.T
    if bias is not None:
        out = out + bias.to(dtype)
    return out.expand(-rows, -1).clone() if rows < 0 else out


# ---- 3. timestep embedding ------------------------------------------------------------------------------------------------------------
TE_DIMS = (256, 320, 7)
TE_STEPS = {1: (999,), 3: (0, 1, 999)}


def timestep_embedding(t, dim, dtype):
    """ldm timestep_embedding: [cos(t f_i) | sin(t f_i) | 0 where dim is odd], f_i = exp(-ln(10000) i / half)"""
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dtype) / half)
    arg = t.to(dtype)[:, None] * f[None]
    out = torch.cat([torch.cos(arg), torch.sin(arg)], dim=1)
    return F.pad(out, (0, dim - 2 * half))


def time_mlp(emb, w0, b0, w2, b2, dtype):
    """time_embed: Linear, SiLU, Linear on 16-bit-rounded weights"""
    h = emb.to(dtype) @ w0.to(dtype).T + b0.to(dtype)
    return (h * torch.sigmoid(h)) @ w2.to(dtype).T + b2.to(dtype)


# ---- 4. layout changes ----------------------------------------------------------------------------------------------------------------
def layout_form(B, C, HW, cols):
    """layout_form (csrc/k_misc.hip): 1 the 32 x 32 LDS-tiled kernel, 0 the element kernel; cols: cpad, or C towards NCHW"""
    return int(C >= 16 and HW >= 32 and B <= 65535 and -(-cols // 32) <= 65535)


LAYOUT_B = 3
# (C, HW, cpad, ld, form); towards NCHW the same (C, HW, ld) with cpad unused
LAYOUT_CASES = {
    "c4_pad8": (4, 20, 8, 8, 0),            # pad columns written as zero
    "c16_hw32": (16, 32, 16, 16, 1),        # the tiled threshold
    "c15_hw32": (15, 32, 16, 16, 0),
    "c16_hw31": (16, 31, 16, 16, 0),
    "c33_hw33": (33, 33, 33, 33, 1),        # ragged tiles on both axes
    "c20_pad24_ld40": (20, 35, 24, 40, 1),  # columns 24 .. 39 stay untouched
}


def nchw_to_nhwc(x, cpad):
    """x [B, C, HW] -> [B * HW, cpad], zero from column C on"""
    B, C, HW = x.shape
    return F.pad(x.permute(0, 2, 1).reshape(B * HW, C), (0, cpad - C))


def nhwc_to_nchw(rows, B, C):
    """rows [B * HW, >= C] -> [B, C, HW]"""
    return rows[:, :C].reshape(B, -1, C).permute(0, 2, 1).contiguous()


# ---- 5. packs and fills ---------------------------------------------------------------------------------------------------------------
def pack_weight_form(N, Cin, taps, transposed, xp, dst_off=0):
    """pack_weight_form (csrc/k_misc.hip): 0 element kernel, 1 per-tap kernel, 2 per-tap kernel with 16-byte stores; dst_off: halfs
    between a 16-byte boundary and dst"""
    if not (1 < taps <= 27 and not transposed and N <= 65535):
        return 0
    Cl = Cin // 3 if xp else Cin
    return 2 if Cl % 8 == 0 and (2 * dst_off) % 16 == 0 else 1


PW_FIELDS = ("N", "cin_src", "Cl", "taps", "transposed", "geglu", "xp", "dst_off", "form")
PW_CASES = {k: dict(zip(PW_FIELDS, v)) for k, v in {
    "lin_n5": (5, 16, 16, 1, 0, 0, 0, 0, 0),
    "lin_geglu_n128": (128, 8, 8, 1, 0, 1, 0, 0, 0),
    "lin_xp_n3": (3, 8, 8, 1, 0, 0, 1, 0, 0),
    "t27_transposed": (5, 8, 8, 27, 1, 0, 0, 0, 0),
    "t9_vec_n5": (5, 16, 16, 9, 0, 0, 0, 0, 2),
    "t9_vec_n3_4to8": (3, 4, 8, 9, 0, 0, 0, 0, 2),
    "t9_vec_70to72": (5, 70, 72, 9, 0, 0, 0, 0, 2),       # the second 64-channel tile has 6 real channels
    "t9_vec_geglu_n128": (128, 8, 8, 9, 0, 1, 0, 0, 2),
    "t27_vec_n3": (3, 16, 16, 27, 0, 0, 0, 0, 2),
    "t9_vec_xp_n5": (5, 16, 16, 9, 0, 0, 1, 0, 2),
    "t9_vec_xp_4to8": (3, 4, 8, 9, 0, 0, 1, 0, 2),
    "t9_tap_cl12": (3, 12, 12, 9, 0, 0, 0, 0, 1),         # Cl % 8 != 0
    "t9_tap_off_70to72": (5, 70, 72, 9, 0, 0, 0, 4, 1),   # dst 8 bytes past a 16-byte boundary
    "t9_tap_xp_off": (5, 16, 16, 9, 0, 0, 1, 4, 1),
    "t27_tap_cl12_10to12": (3, 10, 12, 27, 0, 0, 0, 0, 1),
}.items()}


def geglu_rows(N):
    """row nd of a GEGLU pack holds source row n: alternating 32-row blocks (value | gate)"""
    nd = torch.arange(N)
    j, wi = nd >> 6, nd & 63
    return torch.where(wi < 32, 32 * j + wi, N // 2 + 32 * j + wi - 32)


def pack_weight(src, N, cin_src, Cl, taps, transposed, geglu, xp, opd):
    """src [N][cin_src][taps] (transposed: [cin_src][N][taps]) fp32 -> [taps][N][Cl] in opd (xp: [taps][N][hi | hi | lo] of 3 Cl),
    lo = opd(w - hi)"""
    w = src.reshape(cin_src, N, taps).permute(1, 0, 2) if transposed else src.reshape(N, cin_src, taps)
    if geglu:
        w = w[geglu_rows(N)]
    wp = torch.zeros(N, Cl, taps)
    wp[:, :cin_src] = w
    wp = wp.permute(2, 0, 1)
    hi = wp.to(opd)
    if not xp:
        return hi.contiguous()
    lo = (wp - hi.float()).to(opd)
    return torch.cat([hi, hi, lo], dim=2).contiguous()


def pack_upconv_weight(src, opd):
    """src [N][Cin][3][3] -> [16][N][Cin]: slab (py, px, a, b) sums, in fp32 and in the order (ky, kx) ascending, the taps that land on
    input offset (a, b) for output parity (py, px); one rounding"""
    rng = lambda par, o: ((0, 0) if o == 0 else (1, 2)) if par == 0 else ((0, 1) if o == 0 else (2, 2))  # noqa: E731
    out = []
    for slab in range(16):
        b, a, px, py = slab & 1, (slab >> 1) & 1, (slab >> 2) & 1, slab >> 3
        (ky0, ky1), (kx0, kx1) = rng(py, a), rng(px, b)
        acc = torch.zeros(src.shape[:2])
        for ky in range(ky0, ky1 + 1):
            for kx in range(kx0, kx1 + 1):
                acc = acc + src[:, :, ky, kx]
        out.append(acc.to(opd))
    return torch.stack(out)


def relu_beta_tile(beta, heads, split, opd):
    v = torch.clamp(beta, min=0).repeat(heads)
    hi = v.to(opd)
    return torch.cat([hi, (v - hi.float()).to(opd), hi]) if split else hi


def upsample2(x, opd):
    """x [B, H, W, C] -> [B, 2H, 2W, C] nearest, one rounding"""
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).to(opd)


def sparse_densify(feats, grid):
    """feats [rows, C], grid [nvox] (-1: empty) -> [C, nvox]"""
    out = torch.where((grid >= 0)[:, None], feats[grid.clamp(min=0).long()], torch.zeros(()))
    return out.T.contiguous()


# ---- 6. folds -------------------------------------------------------------------------------------------------------------------------
FOLD_SHAPES = [(h, hd, Cc, I) for h in (1, 3) for hd in (8, 40) for Cc in (16, 72) for I in (64, 100)]
FOLD_MM = [(80, 1, 72, 72, 1, 1), (80, 100, 40, 43, 103, 108), (65, 64, 16, 16, 64, 64)]  # M, N, K, lda, ldb, ldc


def fold_qk(wq, wk, heads, hd, Cc, scale):
    """[heads Cc][I]: scale sum_c Wk[h hd + c][j] Wq[h hd + c][i]; -> (float64 result, sum of |products|)"""
    q, k = wq.double().reshape(heads, hd, -1), wk.double().reshape(heads, hd, Cc)
    s = float(torch.tensor(scale, dtype=torch.float32))
    I = q.shape[2]
    return (s * torch.einsum("hcj,hci->hji", k, q)).reshape(heads * Cc, I), (abs(s) * torch.einsum("hcj,hci->hji", k.abs(), q.abs())).reshape(heads * Cc, I)


def fold_ov(wo, wv, heads, hd, Cc):
    """[I][heads Cc]: sum_c Wo[i][h hd + c] Wv[h hd + c][j]"""
    I = wo.shape[0]
    o, v = wo.double().reshape(I, heads, hd), wv.double().reshape(heads, hd, Cc)
    return torch.einsum("ihc,hcj->ihj", o, v).reshape(I, heads * Cc), torch.einsum("ihc,hcj->ihj", o.abs(), v.abs()).reshape(I, heads * Cc)


def fold_mm(a, b):
    return a.double() @ b.double(), a.double().abs() @ b.double().abs()


def ulp(x, frac_bits, emin):
    """spacing of a binary format (frac_bits fraction bits, smallest normal exponent emin) at |x| (float64 tensor)"""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** (emin - 1)))).clamp(min=emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - frac_bits)


FMT32 = (23, -126)


def fmt16(opd):
    return (10, -14) if opd == torch.float16 else (7, -126)


def fold_bounds(ref, absum, K, opd):
    """The kernel sums K exact fp32 x fp32 products in fp64 (k ascending), scales in fp64 and rounds once to fp32.  Its fp64 value and
    the float64 reference (another summation order) are each within (K + 2) 2^-53 sum|a b| of the exact sum (K - 1 additions, the
    scaling, first order, whatever the order), so slack = 2 (K + 2) 2^-53 sum|a b| apart; the fp32 result is half an fp32 ulp
    further, the 16-bit result is rounded a second time: half a 16-bit ulp more.  The ulps are taken at |ref| + slack, so a value that the slack carries across a binade is covered.
    -> (fp32 bound, 16-bit bound), elementwise"""
    slack = 2 * (K + 2) * 2.0 ** -53 * absum
    at = ref.abs() + slack
    b32 = 0.5 * ulp(at, *FMT32) + slack
    return b32, 0.5 * ulp(at + b32, *fmt16(opd)) + b32


# ---- 7. CFG assembly and DDIM update --------------------------------------------------------------------------------------------------
def cfg_assemble(x_noisy, x_input, clip, timesteps, copies):
    """x_noisy [B, TN, 4, HW], x_input [B, 4, HW], clip [B, dim], timesteps [B] -> xin [copies B TN, HW, 8], ctx [copies B TN, dim],
    tt [copies B TN]: every conditional row first (sample by sample, view by view), then the unconditional copies -- zero image
    channels, zero context.  The quotient is the correctly rounded fp32 one."""
    B, TN, _, HW = x_noisy.shape
    xn = x_noisy.permute(0, 1, 3, 2).reshape(B * TN, HW, 4)
    img = (x_input / torch.tensor(0.18215, dtype=torch.float32)).permute(0, 2, 1)[:, None].expand(B, TN, HW, 4).reshape(B * TN, HW, 4)
    xin = [torch.cat([xn, img], dim=2)]
    ctx = [clip[:, None].expand(B, TN, -1).reshape(B * TN, -1)]
    if copies == 2:
        xin.append(torch.cat([xn, torch.zeros_like(img)], dim=2))
        ctx.append(torch.zeros_like(ctx[0]))
    return torch.cat(xin).contiguous(), torch.cat(ctx).contiguous(), timesteps.repeat_interleave(TN).repeat(copies)


DDIM_N = (1, 4 * 37 * 7 + 3, 4099)
DDIM_COEF = dict(scale=2.0, s1m=0.6, sqrt_at=0.8, sqrt_aprev=0.9, dir_coef=0.35, sigma=0.25)


def cfg_ddim(ec, eu, x, noise, k, dtype):
    """-> (eps, x_prev): eps = eu + scale (ec - eu) (eu None: ec); x0 = (x - s1m eps) / sqrt_at; x_prev = sqrt_aprev x0 + dir_coef eps
    (+ sigma noise)"""
    c = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)  # noqa: E731  (the coefficients are fp32 values)
    e = ec.to(dtype)
    if eu is not None:
        e = eu.to(dtype) + c(k["scale"]) * (e - eu.to(dtype))
    x0 = (x.to(dtype) - c(k["s1m"]) * e) / c(k["sqrt_at"])
    xp = c(k["sqrt_aprev"]) * x0 + c(k["dir_coef"]) * e
    if noise is not None:
        xp = xp + c(k["sigma"]) * noise.to(dtype)
    return e, xp


# ---- 8. small reductions and mixes ----------------------------------------------------------------------------------------------------
FUSE_NV = (1, 37, 1000)
MSE_N = (1, 1023, 1025, 4099)


def fuse_views(vf, w, b, total_views, dtype):
    """vf [views, Nv, 16], w [16, 16] -> [Nv, 16]: (sum over views of w f) / total_views + b"""
    out = torch.einsum("oc,vnc->no", w.to(dtype), vf.to(dtype)) / total_views
    return out if b is None else out + b.to(dtype)


def mse(a, b):
    return ((a.double() - b.double()) ** 2).mean()

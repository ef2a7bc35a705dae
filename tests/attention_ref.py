"""References, CPU emulations and the case tables of the attention tests (tests/test_attention_cpu.py checks them on the CPU,
tests/test_gpu_attention.py holds the HIP kernels against them).

Three kernel families:
  attn_kernel<D> (csrc/k_attn.hip)                        flash-style forward on the fused 16-bit [token][q | k | v] image
  attn_bwd_dq_kernel<D>, attn_bwd_dkv_kernel<D> (k_bwd)   its backward; lse / delta cross from the first kernel to the second
  depth_fwd / depth_bwd / im2col3 / col2im3 / perm_w3     the fp32 training form of the DepthTransformer (csrc/k_train.hip)

References are fp64 on the CPU.  The emulations repeat a kernel's ARITHMETIC (which values are rounded to the 16-bit type, what
is accumulated in fp32, where the softmax denominator comes from) in torch on the CPU: they say how far a correct kernel is from
the fp64 reference, so the bounds the GPU tests assert are derived and checked here, never fitted to what the GPU returns.

Inputs are rounded to the library's 16-bit type on both sides.  u = 2^-11 (float16) or 2^-8 (bfloat16) is the unit roundoff.

Forward bound, per element:  |got - want| <= 4 u sum_k P[q,k] |V[k,j]| + 2^-24   (2^-24: half the smallest fp16 subnormal; dropped
for bfloat16).  Rounding P perturbs numerator and denominator by at most u each relative to sum P|V|, rounding the output adds
u |O| <= u sum P|V|: 3 u; the fourth u is room for fp32 accumulation and the hardware exp2 (below 1e-6 each).  The emulation has to
stay within 1.5 u sum P|V| + 2^-24 on every case of the table (a case that does not gets other inputs, not another bound).
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

HEAD_DIMS = (8, 16, 32, 40, 64, 80, 160)
LOG2E = 1.4426950408889634


def dtype_and_u(name):
    """(torch dtype, unit roundoff) of the library's 16-bit type as mvd_compute_dtype() names it"""
    return {"f16": (torch.float16, 2.0 ** -11), "bf16": (torch.bfloat16, 2.0 ** -8)}[name]


def library_dtype():
    from morphablediffusion_amd import lib
    return dtype_and_u(lib.load().mvd_compute_dtype().decode())


def ones_column(d):
    """True where the forward kernel takes the softmax denominator from the ones column of its V image (over the ROUNDED P):
    the last 32-row fragment of O^T has padding rows, 32 ceil(d / 32) > d.  d = 32, 64, 160 sum the unrounded P explicitly."""
    return 32 * ((d + 31) // 32) > d


def rnd16(t, dt):
    return t.to(dt).to(torch.float32)


def split_heads(t, heads):
    B, T, C = t.shape
    return t.reshape(B, T, heads, C // heads).permute(0, 2, 1, 3)


def merge_heads(t):
    B, H, T, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, H * d)


# ---------------------------------------------------------------------------------------------------------------- cases
# kind: gauss | peak_last (k[T-3] = 4 q[7]) | peak_first (k[5] = 4 q[7]) | qscale (forward: queries 9 and T-2 times 6; backward: query 33) | vscale (V times
# `arg`) | gather (one-hot rows: the output is a row of V, exactly) | do_zero_tail (backward: dO = 0 on the last partial tile)
Case = namedtuple("Case", "name B T heads d Tstride ld_pad kind arg")


def _case(B, T, heads, d, Tstride=0, ld_pad=0, kind="gauss", arg=0.0):
    name = f"d{d}-T{T}-B{B}-h{heads}"
    if Tstride:
        name += f"-Ts{Tstride}"
    if ld_pad:
        name += f"-pad{ld_pad}"
    if kind != "gauss":
        name += f"-{kind}" + (f"{arg:g}" if arg else "")
    return Case(name, B, T, heads, d, Tstride, ld_pad, kind, arg)


FWD_T = (1, 7, 16, 63, 64, 65, 127, 128, 129, 200, 257)
BWD_T = (1, 16, 63, 64, 65, 129, 200)
GATHER_T = 200


def forward_cases():
    cs = [_case(2, T, 3, d) for d in HEAD_DIMS for T in FWD_T]
    cs += [_case(2, 1024, 3, 40), _case(2, 1024, 3, 64)]
    for d in (40, 64):
        for T in (16, 129, 257):
            for Ts in sorted({T + 7, 264}):
                if Ts >= T:
                    cs.append(_case(2, T, 3, d, Tstride=Ts))
            cs.append(_case(2, T, 3, d, ld_pad=8))
            cs.append(_case(2, T, 3, d, Tstride=T + 7, ld_pad=8))
    cs.append(_case(2, 257, 16, 64, Tstride=264))  # CLIP ViT-L/14: 257 tokens in 264 rows, 16 heads of 64
    for d in (8, 32, 40, 64, 160):
        for T in (129, 257):
            cs += [_case(2, T, 3, d, kind=kd) for kd in ("peak_last", "peak_first", "qscale")]
    for d, T in ((16, 63), (32, 129)):
        cs += [_case(2, T, 3, d, kind="vscale", arg=100.0), _case(2, T, 3, d, kind="vscale", arg=1e-3)]
    cs += [_case(2, GATHER_T, 3, d, kind="gather") for d in HEAD_DIMS]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def xcd_cases():
    """six forward cases run without and with the XCD remap: workgroup counts 12, 18, 6 and 12 (the remap's remainder branch), 48
    and 96 (multiples of the 8 XCDs)"""
    by = {c.name: c for c in forward_cases()}
    return [by[n] for n in ("d8-T129-B2-h3", "d40-T257-B2-h3", "d64-T65-B2-h3", "d160-T129-B2-h3-peak_last", "d40-T1024-B2-h3",
                            "d64-T257-B2-h16-Ts264")]


def backward_cases():
    cs = [_case(2, T, 3, d) for d in HEAD_DIMS for T in BWD_T]
    cs.append(_case(2, 1024, 3, 40))
    for d in (8, 40, 64, 160):
        cs += [_case(2, 129, 3, d, kind=kd) for kd in ("peak_last", "peak_first", "qscale")]
    cs.append(_case(2, 129, 3, 40, kind="do_zero_tail"))
    assert len({c.name for c in cs}) == len(cs)
    return cs


def _seed(c):
    return 1000 * c.d + c.T + 7 * c.heads + 13 * c.Tstride + c.ld_pad


def gather_perm(T, seed):
    return torch.randperm(T, generator=torch.Generator().manual_seed(seed))


def make_inputs(c, dt, backward=False):
    """q, k, v (and dO) [B][T][C] fp32 holding values of the 16-bit type dt"""
    g = torch.Generator().manual_seed(_seed(c))
    C = c.heads * c.d
    q, k, v = (torch.randn(c.B, c.T, C, generator=g) for _ in range(3))
    do = torch.randn(c.B, c.T, C, generator=g) if backward else None
    if c.kind == "peak_last":
        q = rnd16(q, dt)
        k[:, c.T - 3] = 4.0 * q[:, 7]
    elif c.kind == "peak_first":
        q = rnd16(q, dt)
        k[:, 5] = 4.0 * q[:, 7]
    elif c.kind == "qscale":
        if backward:  # one query: the 16-bit rounding of its dS row weighs 6 times in dk (query 33 keeps the emulation below half
            q[:, 33] *= 6.0  # the slice bound in both 16-bit types at every head width)
        else:
            q[:, 9] *= 6.0
            q[:, c.T - 2] *= 6.0
    elif c.kind == "vscale":
        v = v * c.arg
    elif c.kind == "gather":
        # query i is a row of signs whose first 8 entries spell i (distinct rows: q_i . q_j <= d - 2 for j != i); key perm[i] is
        # 256 q_i, so row i of the scores has one entry 512 / sqrt(d) >= 40 above all others: one-hot below 2^-24 in fp64.
        # V[key][j] are integers of at most 7 bits, exact in both 16-bit types, and distinct from row to row
        assert c.T <= 256
        bits = torch.randint(0, 2, (c.B, c.T, c.heads, c.d), generator=g)
        idx = torch.arange(c.T)
        for b in range(8):
            bits[:, :, :, b] = ((idx >> b) & 1)[None, :, None]
        q = (2.0 * bits - 1.0).reshape(c.B, c.T, C)
        perm = gather_perm(c.T, _seed(c))
        k = torch.empty_like(q)
        k[:, perm] = 256.0 * q
        key = torch.arange(c.T)[None, :, None]
        col = torch.arange(C)[None, None, :]
        v = (((key * 7 + col * 13) % 255) - 127).to(torch.float32).expand(c.B, c.T, C).contiguous()
    elif c.kind == "do_zero_tail":
        do[:, (c.T // 64) * 64:] = 0.0
    q, k, v = rnd16(q, dt), rnd16(k, dt), rnd16(v, dt)
    if backward:
        return q, k, v, rnd16(do, dt)
    return q, k, v


# ------------------------------------------------------------------------------------------------------ fp64 references
def ref_forward(q, k, v, heads):
    """fp64: (O [B,T,C], sum_k P |V| [B,T,C], natural-log LSE [B,heads,T], P [B,heads,T,T])"""
    qh, kh, vh = (split_heads(t.double(), heads) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1])
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    return merge_heads(p @ vh), merge_heads(p @ vh.abs()), lse, p


def ref_backward(q, k, v, do, heads, queries=None):
    """fp64: dq, dk, dv [B,T,C], natural-log LSE and delta = sum_j dO O [B,heads,T], O, sum P|V|, and (dq, dk) with every term
    taken by its absolute value (the scale of a slice whose gradient cancels to zero: T = 1).  queries (a slice): dk and dv take
    the contributions of those query rows only."""
    d = q.shape[-1] // heads
    o, apv, lse, p = ref_forward(q, k, v, heads)
    qh, kh, vh, doh, oh = (split_heads(t.double(), heads) for t in (q, k, v, do, o))
    delta = (doh * oh).sum(-1)
    ds = p * (doh @ vh.transpose(-1, -2) - delta[..., None])
    dq = ds @ kh / math.sqrt(d)
    ds_abs = p * (doh.abs() @ vh.abs().transpose(-1, -2) + (doh * oh).abs().sum(-1)[..., None])
    scale = (merge_heads(ds_abs @ kh.abs() / math.sqrt(d)), merge_heads(ds_abs.transpose(-1, -2) @ qh.abs() / math.sqrt(d)))
    if queries is not None:
        p, ds, doh, qh = p[:, :, queries], ds[:, :, queries], doh[:, :, queries], qh[:, :, queries]
    dk = ds.transpose(-1, -2) @ qh / math.sqrt(d)
    dv = p.transpose(-1, -2) @ doh
    return merge_heads(dq), merge_heads(dk), merge_heads(dv), lse, delta, o, apv, scale


# ---------------------------------------------------------------------------------------------------------- emulations
def _exp2_fma(s, scale, m):
    """exp2(fma(s, scale, -m)) as the kernels evaluate it: one rounding of the argument, fp32 result"""
    return torch.exp2((s.double() * float(scale) - m.double()).float())


def emulate_forward(q, k, v, heads, dt, want_stats=False):
    """attn_kernel's arithmetic: 64-key tiles, running maximum of the scaled scores, P rounded to the 16-bit type for the second
    product, the denominator from the rounded P where the kernel uses the ones column and from the unrounded P elsewhere, fp32
    accumulation, the output rounded to the 16-bit type.  -> O [B,T,C] (want_stats: also the log2-unit lse [B,heads,T])"""
    d = q.shape[-1] // heads
    qh, kh, vh = (split_heads(t.float(), heads) for t in (q, k, v))
    B, H, T, _ = qh.shape
    scale = torch.tensor(LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(d), dtype=torch.float32))
    rounded_sum = ones_column(d)
    m = torch.full((B, H, T), -math.inf)
    l = torch.zeros(B, H, T)
    l_exact = torch.zeros(B, H, T)
    o = torch.zeros(B, H, T, d)
    for k0 in range(0, T, 64):
        kt, vt = kh[:, :, k0:k0 + 64], vh[:, :, k0:k0 + 64]
        s = qh @ kt.transpose(-1, -2)
        m_new = torch.maximum(m, s.max(-1).values * scale)
        p = _exp2_fma(s, scale, m_new[..., None])
        p16 = rnd16(p, dt)
        alpha = torch.exp2(m - m_new)
        o = o * alpha[..., None] + p16 @ vt
        l = l * alpha + (p16 if rounded_sum else p).sum(-1)
        l_exact = l_exact * alpha + p.sum(-1)
        m = m_new
    out = merge_heads(rnd16(o * (1.0 / l)[..., None], dt))
    return (out, m + torch.log2(l_exact)) if want_stats else out


def emulate_backward(q, k, v, do, heads, dt):
    """the two backward kernels' arithmetic: o from the forward emulation (16-bit), delta = sum dO o and the log2 lse in fp32,
    P = exp2(S scale - lse) and dS = P (dO V^T - delta) in fp32, both rounded to the 16-bit type for the products, fp32
    accumulation, 16-bit results.  -> dq, dk, dv [B,T,C], lse (log2 units), delta [B,heads,T], o"""
    d = q.shape[-1] // heads
    o16, lse2 = emulate_forward(q, k, v, heads, dt, want_stats=True)
    qh, kh, vh, doh, oh = (split_heads(t.float(), heads) for t in (q, k, v, do, o16))
    scale_nat = 1.0 / torch.sqrt(torch.tensor(float(d), dtype=torch.float32))
    scale = torch.tensor(LOG2E, dtype=torch.float32) * scale_nat
    delta = (doh * oh).sum(-1)
    p = _exp2_fma(qh @ kh.transpose(-1, -2), scale, lse2[..., None])
    ds = p * (doh @ vh.transpose(-1, -2) - delta[..., None])
    p16, ds16 = rnd16(p, dt), rnd16(ds, dt)
    dq = rnd16((ds16 @ kh) * scale_nat, dt)
    dk = rnd16((ds16.transpose(-1, -2) @ qh) * scale_nat, dt)
    dv = rnd16(p16.transpose(-1, -2) @ doh, dt)
    return merge_heads(dq), merge_heads(dk), merge_heads(dv), lse2, delta, o16


# -------------------------------------------------------------------------------------------------------------- bounds
def forward_bound(apv, u):
    """4 u sum P|V| (+ 2^-24 for float16), per element"""
    return 4.0 * u * apv + (2.0 ** -24 if u == 2.0 ** -11 else 0.0)


def forward_ratio(got, want, apv, u, factor=4.0):
    """worst |got - want| / (factor u sum P|V| + 2^-24) over the elements"""
    bound = forward_bound(apv, u) if factor == 4.0 else factor * u * apv + (2.0 ** -24 if u == 2.0 ** -11 else 0.0)
    return ((got.double() - want).abs() / bound).max().item()


BWD_REL_L2 = 3e-3  # the project's bound on the backward (tests/test_gpu_train_ops.py), for float16; here per (sample, head) slice


def backward_bound(u):
    """3e-3 for float16; the 16-bit roundings it allows for scale with u (bfloat16: 8 x, as in tests/test_gpu_train_bf16.py)"""
    return BWD_REL_L2 * (u / 2.0 ** -11)


def worst_slice_rel_l2(got, want, heads, scale=None):
    """largest relL2 over the (sample, head) slices of a [B,T,C] tensor.  A slice whose reference is exactly zero (dq, dk at
    T = 1: one key, dS = P (dP - delta) = 0) is measured against `scale`, the same gradient with every term by its absolute value"""
    g, w = split_heads(got.double(), heads), split_heads(want.double(), heads)
    num = (g - w).flatten(2).norm(dim=-1)
    den = w.flatten(2).norm(dim=-1)
    if scale is not None:
        den = torch.where(den == 0, split_heads(scale.double(), heads).flatten(2).norm(dim=-1), den)
    return (num / (den + 1e-300)).max().item()


def lse_ratio(lse2, lse_ref):
    """worst |lse ln2 - LSE_ref| / (1e-5 max(1, |LSE_ref|))"""
    return ((lse2.double() * math.log(2.0) - lse_ref).abs() / (1e-5 * lse_ref.abs().clamp_min(1.0))).max().item()


def delta_ratio(delta, delta_ref, do, o_ref, apv, heads, u):
    """worst |delta - ref| / (4 u sum_j |dO_j| (sum_k P|V|)_j + 1e-6 sum_j |dO_j O_j|): the forward bound through the dot product"""
    doh, oh, ah = (split_heads(t.double(), heads) for t in (do, o_ref, apv))
    bound = 4.0 * u * (doh.abs() * ah).sum(-1) + 1e-6 * (doh * oh).abs().sum(-1)
    bad = (delta.double() - delta_ref).abs()
    return (bad / bound.clamp_min(1e-300)).max().item()  # bound == 0 (dO == 0 on the whole row): any non-zero delta is ~1e300 over


# ------------------------------------------------------------------------------ DepthTransformer training kernels (fp32)
DEPTH_CASES = ((2, 16, 6, 4, 16), (2, 4, 48, 4, 16), (1, 9, 64, 4, 8), (2, 4, 12, 4, 80), (1, 2, 24, 4, 256), (2, 3, 5, 1, 24),
               (1, 1, 1, 4, 16))  # (B, HW, D, hn, hd)
DEPTH_REFUSED = ((1, 2, 65, 4, 16), (1, 2, 6, 5, 16), (1, 2, 6, 4, 258))  # D = 65, hn = 5, hn * hd = 1032
DEPTH_TOL = 1e-5  # the project's fp32-kernel bound (tests/test_gpu_train_ops.py), relative to the pixel's largest element
IM2COL_CASES = ((2, 4, 4, 8), (1, 1, 1, 4), (2, 3, 5, 6), (1, 8, 8, 64))  # (B, H, W, C)
PERM_CASES = ((8, 8), (5, 12))  # (N, C)


def depth_inputs(case, peaked=True):
    """q [R,I], k, v [B*D*HW, I], dz [R,I] fp32.  Scores are O(1) Gaussians times 3 (|sim| <= 30 is asserted on the CPU); with
    hn == 4 one row (pixel 0, head 1) is peaked: its key at the last depth sample is the query scaled to sim = 24."""
    B, HW, D, hn, hd = case
    g = torch.Generator().manual_seed(sum(x * y for x, y in zip(case, (1, 10, 100, 1000, 10000))))
    I, R = hn * hd, B * HW
    q = torch.randn(R, I, generator=g) * 3.0
    k = torch.randn(B * D * HW, I, generator=g)
    v = torch.randn(B * D * HW, I, generator=g)
    dz = torch.randn(R, I, generator=g)
    if peaked and hn == 4 and D > 1:
        qr = q[0, hd:2 * hd]
        k[(D - 1) * HW, hd:2 * hd] = qr * (24.0 * math.sqrt(hd) / float(qr.double().pow(2).sum()))
    return q, k, v, dz


def ref_depth_forward(q, k, v, HW, D, hn):
    """fp64: (sim [R,hn,D], attn [R,hn,D], z [R,I])"""
    R, I = q.shape
    B, hd = R // HW, I // hn
    qd = q.double().reshape(B, HW, hn, hd)
    kd = k.double().reshape(B, D, HW, hn, hd)
    vd = v.double().reshape(B, D, HW, hn, hd)
    sim = torch.einsum("bphc,bdphc->bphd", qd, kd) / math.sqrt(hd)
    attn = torch.softmax(sim, -1)
    z = torch.einsum("bphd,bdphc->bphc", attn, vd)
    return sim.reshape(R, hn, D), attn.reshape(R, hn, D), z.reshape(R, I)


def ref_depth_backward(q, k, v, attn, dz, HW, D, hn):
    """fp64 backward from the given attn (what the kernel is handed): dq [R,I], dk, dv [B*D*HW, I]"""
    R, I = q.shape
    B, hd = R // HW, I // hn
    qd = q.double().reshape(B, HW, hn, hd)
    kd = k.double().reshape(B, D, HW, hn, hd)
    vd = v.double().reshape(B, D, HW, hn, hd)
    a = attn.double().reshape(B, HW, hn, D)
    dzd = dz.double().reshape(B, HW, hn, hd)
    dattn = torch.einsum("bphc,bdphc->bphd", dzd, vd)
    ds = a * (dattn - (a * dattn).sum(-1, keepdim=True))
    scale = 1.0 / math.sqrt(hd)
    dq = scale * torch.einsum("bphd,bdphc->bphc", ds, kd)
    dk = scale * torch.einsum("bphd,bphc->bdphc", ds, qd)
    dv = torch.einsum("bphd,bphc->bdphc", a, dzd)
    return dq.reshape(R, I), dk.reshape(B * D * HW, I), dv.reshape(B * D * HW, I)


def pixel_slices(t, B, HW, D=None):
    """[pixels][everything of that pixel]: rows of q-shaped tensors (D is None) or the D rows of a pixel in k-shaped ones"""
    if D is None:
        return t.reshape(B * HW, -1)
    return t.reshape(B, D, HW, -1).permute(0, 2, 1, 3).reshape(B * HW, -1)


def pixel_ratio(got, want, B, HW, D=None, tol=DEPTH_TOL):
    """worst |got - want| / (tol max|want over the pixel|)"""
    g, w = pixel_slices(got.double(), B, HW, D), pixel_slices(want.double(), B, HW, D)
    return ((g - w).abs().max(-1).values / (tol * w.abs().max(-1).values.clamp_min(1e-300))).max().item()


def ref_im2col3(x):
    """x [B,H,W,C] -> [B*H*W, 9*C] with column tap*C + c, tap = ky*3 + kx, through F.unfold (whose columns are c*9 + tap)"""
    B, H, W, C = x.shape
    cols = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1)  # [B, C*9, H*W]
    return cols.reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)


def ref_col2im3(dcol, B, H, W):
    """the transpose through F.fold: dcol [B*H*W, 9*C] -> [B,H,W,C]"""
    C = dcol.shape[1] // 9
    cols = dcol.reshape(B, H * W, 9, C).permute(0, 3, 2, 1).reshape(B, C * 9, H * W)
    return F.fold(cols, (H, W), 3, padding=1).permute(0, 2, 3, 1).contiguous()


def ref_perm_w3(w, to_mat):
    """[N,C,3,3] -> [N,9,C] (to_mat) or [N,9,C] -> [N,C,3,3]"""
    if to_mat:
        N, C = w.shape[:2]
        return w.reshape(N, C, 9).permute(0, 2, 1).contiguous()
    N, _, C = w.shape
    return w.permute(0, 2, 1).reshape(N, C, 3, 3).contiguous()


def impulse_images(B, H, W, C):
    """one image batch per corner / edge / centre position: a single 1 at (b, y, x, c), distinct integers elsewhere would hide
    nothing -- the impulse says which output column each tap of each border pixel lands in"""
    pos = sorted({(y, x) for y in (0, H // 2, H - 1) for x in (0, W // 2, W - 1)})
    out = []
    for i, (y, x) in enumerate(pos):
        t = torch.zeros(B, H, W, C)
        t[i % B, y, x, i % C] = 1.0
        out.append(t)
    return out

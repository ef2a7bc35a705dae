"""GPU: the attention kernels one at a time against the fp64 references of tests/attention_ref.py, at the edges of their tiles and
under bounds derived there (and checked on the CPU by tests/test_attention_cpu.py), through hooks that poison everything a launch
may touch beside its operands and results.

  attn_kernel<D>                     mvd_op_attention_ex: every head width x T in {1 .. 257}, T = 1024, padded token axis (Tstride),
                                     pad columns, CLIP's 16 x 64 at 257 / 264, peaked rows on both denominator forms, scaled V,
                                     exact one-hot gathers, and the XCD remap on / off bit for bit.  Per element:
                                     |got - want| <= 4 u sum_k P|V| + 2^-24
  attn_bwd_dq / attn_bwd_dkv<D>      mvd_op_attention_bwd_ex: ragged T (the partial-tile code), lse and delta on their own, the
                                     forward's o; dq / dk / dv per (sample, head) slice, relL2 <= 3e-3 (float16)
  depth_fwd / depth_bwd              mvd_op_train_depth_attn[_bwd]: 1e-5 of the pixel's largest element, rows of attn sum to 1
  im2col3 / col2im3 / perm_w3        exact

Observed worst ratio to the asserted bound, MI355X, float16 / bfloat16 library (the [parity] lines of this file):
  forward, per element                      0.30 / 0.28   (relL2 2.1e-4 .. 2.8e-4 / 1.6e-3 .. 2.2e-3; the CPU emulation: 0.30 of 4 u)
  backward slices  dq / dk / dv             0.36, 0.31, 0.14 / 0.34, 0.46, 0.14   (bound 3e-3, for bfloat16 times 8 = u / 2^-11)
  backward  lse / delta / o                 0.02, 0.12, 0.31 / 0.02, 0.15, 0.26
  depth attention  attn, z, dq, dk, dv      0.05, 0.05, 0.07, 0.10, 0.01; rows of attn sum to 1 within 3.2e-7
  col2im3, arbitrary dcol                   0.14 of 1e-6; gathers, the XCD comparison, im2col3, perm_w3, integer col2im3: exact

Each of these deliberate errors, in a scratch build of the library, fails tests of this file (the count of failing cases):
  forward: the `key >= T` mask removed                 test_forward at every ragged T (120), test_backward through o / delta (55)
  forward: denominator from the other half-wave        test_forward, test_backward: every case of d = 8, 16, 40, 80 (74 + 36)
  forward: tok0 = b * T                                every Tstride case (17) and the XCD case with Tstride (pad rows written)
  forward: the ones column written at column D + 1     test_forward, test_backward: every case of d = 8, 16, 40, 80 (74 + 36)
  backward: `r0 + key < T` dropped in stage_tile       test_backward at every ragged T (55): the guard row's NaN reaches dq / dk / dv
  backward: lse written without the log                test_backward: every case but T = 1 (63), on the lse bound
  depth forward: softmax over D - 1 samples            test_train_depth_attention: all 7 cases
  im2col3: right edge off by one                       test_train_im2col3_and_col2im3: all 4 cases
"""
import functools

import pytest
import torch

from tests import attention_ref as R

pytestmark = pytest.mark.gpu

DT, U = R.library_dtype()
FWD = R.forward_cases()
BWD = R.backward_cases()
XCD = R.xcd_cases()


@pytest.fixture(scope="module")
def eng():
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig
    e = Engine(UNetConfig(model_channels=64), VolumeConfig(), workspace_gb=2.0)
    yield e
    e.close()


@functools.lru_cache(maxsize=8)
def forward_reference(c):
    q, k, v = R.make_inputs(c, DT)
    want, apv, _, _ = R.ref_forward(q, k, v, c.heads)
    return q, k, v, want, apv


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", FWD, ids=[c.name for c in FWD])
def test_forward(eng, c):
    q, k, v, want, apv = forward_reference(c)
    got = eng.op_attention_ex(q, k, v, c.heads, Tstride=c.Tstride, ld_pad=c.ld_pad).cpu()
    assert got.shape == want.shape and torch.isfinite(got).all(), c.name
    if c.kind == "gather":
        sel = v[:, R.gather_perm(c.T, R._seed(c))]
        wrong = int((got != sel).any(-1).sum())
        print(f"[parity] attention forward {c.name}: {wrong} of {c.B * c.T} rows differ from the selected row of V")
        assert torch.equal(got, sel), f"{c.name}: {wrong} rows are not the selected row of V"
        return
    ratio = R.forward_ratio(got, want, apv, U)
    rl2 = ((got.double() - want).norm() / want.norm()).item()
    print(f"[parity] attention forward {c.name}: worst |err| / (4 u sum P|V| + 2^-24) = {ratio:.3f}, relL2 {rl2:.2e}")
    assert ratio <= 1.0, (c.name, ratio)


@pytest.mark.parametrize("c", XCD, ids=[c.name for c in XCD])
def test_forward_is_bit_identical_with_and_without_the_xcd_remap(eng, c):
    q, k, v, _, _ = forward_reference(c)
    off = eng.op_attention_ex(q, k, v, c.heads, Tstride=c.Tstride, ld_pad=c.ld_pad, xcd=0)
    on = eng.op_attention_ex(q, k, v, c.heads, Tstride=c.Tstride, ld_pad=c.ld_pad, xcd=1)
    print(f"[parity] attention forward {c.name}: XCD remap on / off differ in {int((off != on).sum())} elements")
    assert torch.equal(off, on)


def test_forward_hook_refuses_bad_arguments(eng):
    from morphablediffusion_amd.lib import MvdError
    q = torch.zeros(1, 16, 24)
    for kw, heads, text in ((dict(Tstride=15), 3, "Tstride"), (dict(ld_pad=4), 3, "ld_pad"), (dict(xcd=2), 3, "xcd"), (dict(), 2, "head dim")):
        with pytest.raises(MvdError, match=text):
            eng.op_attention_ex(q, q, q, heads, **kw)
    with pytest.raises(MvdError, match="head dim"):
        eng.op_attention_bwd_ex(q, q, q, q, 2)
    L = eng.lib
    p = torch.zeros(8, device=eng.device).data_ptr()
    assert L.mvd_op_attention_ex(eng._ctx, p, p, p, 1, 0, 1, 8, 0, 0, -1, p, None) != 0  # T < 1
    assert L.mvd_op_attention_ex(eng._ctx, p, None, p, 1, 1, 1, 8, 0, 0, -1, p, None) != 0 and b"null" in L.mvd_last_error()
    assert L.mvd_op_attention_ex(eng._ctx, p, p, p, 1, 1, 1, 8, 0, 0, -1, None, None) != 0 and b"null" in L.mvd_last_error()


# ----------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("c", BWD, ids=[c.name for c in BWD])
def test_backward(eng, c):
    q, k, v, do = R.make_inputs(c, DT, backward=True)
    tail = (c.T // 64) * 64
    sl = slice(0, tail) if c.kind == "do_zero_tail" else None
    dq_r, dk_r, dv_r, lse_r, delta_r, o_r, apv, scale = R.ref_backward(q, k, v, do, c.heads, queries=sl)
    dq, dk, dv, lse2, delta, o = (t.cpu() for t in eng.op_attention_bwd_ex(q, k, v, do, c.heads))
    errs = [R.worst_slice_rel_l2(g, w, c.heads, sc) for g, w, sc in ((dq, dq_r, scale[0]), (dk, dk_r, scale[1]), (dv, dv_r, None))]
    bound = R.backward_bound(U)
    rl, rd, ro = R.lse_ratio(lse2, lse_r), R.delta_ratio(delta, delta_r, do, o_r, apv, c.heads, U), R.forward_ratio(o, o_r, apv, U)
    print(f"[parity] attention backward {c.name}: worst slice relL2 / {bound:.1e}: dq {errs[0] / bound:.3f} dk {errs[1] / bound:.3f} "
          f"dv {errs[2] / bound:.3f}; ratios to bound: lse {rl:.3f} delta {rd:.3f} o {ro:.3f}")
    assert rl <= 1.0, (c.name, "lse", rl)
    assert rd <= 1.0, (c.name, "delta", rd)
    assert ro <= 1.0, (c.name, "o", ro)
    assert max(errs) <= bound, (c.name, errs)
    if c.kind == "do_zero_tail":
        assert (delta[:, :, tail:] == 0).all(), "delta of a query with dO = 0 is exactly 0"


# ------------------------------------------------------------------------------ DepthTransformer training kernels (fp32)
@pytest.mark.parametrize("case", R.DEPTH_CASES, ids=[str(c) for c in R.DEPTH_CASES])
def test_train_depth_attention(case):
    from morphablediffusion_amd import engine as E
    B, HW, D, hn, hd = case
    q, k, v, dz = R.depth_inputs(case)
    _, attn_r, z_r = R.ref_depth_forward(q, k, v, HW, D, hn)
    attn, z = (t.cpu() for t in E.op_train_depth_attn(q.cuda(), k.cuda(), v.cuda(), HW, D, hn))
    assert torch.isfinite(attn).all() and torch.isfinite(z).all()
    rows = (attn.double().sum(-1) - 1).abs().max().item()
    ra, rz = R.pixel_ratio(attn, attn_r, B, HW), R.pixel_ratio(z, z_r, B, HW)
    # the backward from the reference's attn (rounded to fp32): independent of the forward kernel
    a32 = attn_r.float()
    dq_r, dk_r, dv_r = R.ref_depth_backward(q, k, v, a32, dz, HW, D, hn)
    dq, dk, dv = (t.cpu() for t in E.op_train_depth_attn_bwd(q.cuda(), k.cuda(), v.cuda(), a32.cuda(), dz.cuda(), HW, D, hn))
    assert all(torch.isfinite(t).all() for t in (dq, dk, dv))
    rq, rk, rv = R.pixel_ratio(dq, dq_r, B, HW), R.pixel_ratio(dk, dk_r, B, HW, D), R.pixel_ratio(dv, dv_r, B, HW, D)
    print(f"[parity] train depth attention {case}: ratio to 1e-5 of the pixel maximum: attn {ra:.3f} z {rz:.3f} dq {rq:.3f} dk {rk:.3f} "
          f"dv {rv:.3f}; attn rows sum to 1 within {rows:.1e}")
    assert max(ra, rz, rq, rk, rv) <= 1.0, (case, ra, rz, rq, rk, rv)
    assert rows <= 1e-6


@pytest.mark.parametrize("case", R.DEPTH_REFUSED, ids=[str(c) for c in R.DEPTH_REFUSED])
def test_train_depth_attention_refuses_what_the_kernel_cannot_hold(case):
    """D = 65, 5 heads, heads * dim_head = 1032: the launcher's error, no launch, the results as they were"""
    from morphablediffusion_amd import lib as L
    lib = L.load()
    B, HW, D, hn, hd = case
    R_, I = B * HW, hn * hd
    dev = torch.device("cuda")
    q, dz = torch.ones(R_, I, device=dev), torch.ones(R_, I, device=dev)
    k, v = torch.ones(B * D * HW, I, device=dev), torch.ones(B * D * HW, I, device=dev)
    attn = torch.full((R_, hn, D), 3.0, device=dev)
    outs = [torch.full_like(q, 3.0), torch.full_like(q, 3.0), torch.full_like(k, 3.0), torch.full_like(k, 3.0)]
    z, dq, dk, dv = outs
    s = torch.cuda.current_stream().cuda_stream
    assert lib.mvd_op_train_depth_attn(L.ptr(q), L.ptr(k), L.ptr(v), R_, HW, D, hn, hd, L.ptr(attn), L.ptr(z), s) != 0
    assert b"train_depth: needs heads <= 4" in lib.mvd_last_error()
    assert lib.mvd_op_train_depth_attn_bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(attn), L.ptr(dz), R_, HW, D, hn, hd, L.ptr(dq), L.ptr(dk),
                                           L.ptr(dv), s) != 0
    assert b"train_depth: needs heads <= 4" in lib.mvd_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in outs + [attn])


@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=[str(c) for c in R.IM2COL_CASES])
def test_train_im2col3_and_col2im3(case):
    from morphablediffusion_amd import engine as E
    B, H, W, Cc = case
    g = torch.Generator().manual_seed(B + 10 * H + 100 * W + Cc)
    images = [torch.randn(B, H, W, Cc, generator=g)] + R.impulse_images(B, H, W, Cc)
    for i, x in enumerate(images):
        got = E.op_train_im2col3(x.cuda()).cpu()
        assert torch.equal(got, R.ref_im2col3(x)), f"im2col3 {case}: image {i} ({'random' if i == 0 else 'impulse'})"
    # col2im3 on an arbitrary dcol (not an im2col image): nine fp32 adds per element
    dcol = torch.randn(B * H * W, 9 * Cc, generator=g)
    got = E.op_train_col2im3(dcol.cuda(), B, H, W).cpu()
    want, mag = R.ref_col2im3(dcol.double(), B, H, W), R.ref_col2im3(dcol.double().abs(), B, H, W)
    ratio = ((got.double() - want).abs() / (1e-6 * mag)).max().item()
    ints = torch.randint(-50, 51, (B * H * W, 9 * Cc), generator=g).float()
    got_i = E.op_train_col2im3(ints.cuda(), B, H, W).cpu()
    taps = [torch.zeros(B * H * W, 9 * Cc) for _ in range(3)]  # impulses in dcol: a border pixel's taps that fall outside
    taps[0][0, 0] = 1.0
    taps[1][B * H * W - 1, 9 * Cc - 1] = 1.0
    taps[2][W - 1, 2 * Cc] = 1.0
    print(f"[parity] train im2col3 / col2im3 {case}: im2col exact on {len(images)} images; col2im |err| / (1e-6 sum |terms|) = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(got_i, R.ref_col2im3(ints, B, H, W))
    for t in taps:
        assert torch.equal(E.op_train_col2im3(t.cuda(), B, H, W).cpu(), R.ref_col2im3(t, B, H, W))


@pytest.mark.parametrize("N,Cc", R.PERM_CASES)
def test_train_perm_w3(N, Cc):
    from morphablediffusion_amd import engine as E
    w = torch.arange(N * Cc * 9, dtype=torch.float32).reshape(N, Cc, 3, 3) - 100.0
    mat = E.op_train_perm_w3(w.cuda(), N, Cc, True).cpu()
    assert torch.equal(mat, R.ref_perm_w3(w, True))
    back = E.op_train_perm_w3(mat.cuda(), N, Cc, False).cpu()
    assert torch.equal(back, R.ref_perm_w3(mat, False)) and torch.equal(back, w)
    print(f"[parity] train perm_w3 N={N} C={Cc}: both directions exact, the round trip is the identity")

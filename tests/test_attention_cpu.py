"""CPU: the references, emulations, case tables and bounds of tests/attention_ref.py, which tests/test_gpu_attention.py holds the
attention kernels against.  The fp64 references are checked against torch (scaled_dot_product_attention, autograd, conv2d); the
emulations of the kernels' arithmetic must stay inside the asserted bounds with room to spare on EVERY case of the tables (forward:
1.5 u sum P|V| + 2^-24 against the asserted 4 u; backward: half the slice bound) -- a case that does not gets other inputs."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attention_ref as R

DT, U = R.library_dtype()
FWD = R.forward_cases()
BWD = R.backward_cases()


def test_forward_reference_is_scaled_dot_product_attention():
    c = R._case(2, 37, 3, 40)
    q, k, v = R.make_inputs(c, DT)
    o, apv, lse, p = R.ref_forward(q, k, v, c.heads)
    qh, kh, vh = (R.split_heads(t.double(), c.heads) for t in (q, k, v))
    want = R.merge_heads(F.scaled_dot_product_attention(qh, kh, vh))
    assert (o - want).abs().max() <= 1e-13
    assert (p.sum(-1) - 1).abs().max() <= 1e-13 and (apv >= o.abs() - 1e-13).all()
    s = qh @ kh.transpose(-1, -2) / math.sqrt(c.d)
    assert (lse - torch.log(torch.exp(s).sum(-1))).abs().max() <= 1e-12


def test_backward_reference_is_autograd():
    c = R._case(2, 37, 3, 16)
    q, k, v, do = R.make_inputs(c, DT, backward=True)
    qq, kk, vv = (t.double().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (R.split_heads(t, c.heads) for t in (qq, kk, vv))
    out = R.merge_heads(torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(c.d), -1) @ vh)
    out.backward(do.double())
    dq, dk, dv, lse, delta, o, apv, _ = R.ref_backward(q, k, v, do, c.heads)
    for got, want in ((dq, qq.grad), (dk, kk.grad), (dv, vv.grad), (o, out.detach())):
        assert (got - want).abs().max() <= 1e-12 * max(1.0, want.abs().max().item())
    assert (delta - R.split_heads(do.double() * o, c.heads).sum(-1)).abs().max() <= 1e-12
    # restricted to a set of queries: the other queries' dO set to zero gives the same dk / dv
    sl = slice(0, 20)
    do0 = do.clone()
    do0[:, 20:] = 0
    _, dk_r, dv_r, *_ = R.ref_backward(q, k, v, do0, c.heads, queries=sl)
    _, dk_f, dv_f, *_ = R.ref_backward(q, k, v, do0, c.heads)
    assert (dk_r - dk_f).abs().max() <= 1e-12 and (dv_r - dv_f).abs().max() <= 1e-12


def test_case_tables_cover_what_they_claim():
    for d in R.HEAD_DIMS:
        assert R.ones_column(d) == (d in (8, 16, 40, 80)), d  # 32, 64, 160: the explicit sum of the unrounded P
        for T in R.FWD_T:
            assert any(c.d == d and c.T == T and c.kind == "gauss" and not c.Tstride and not c.ld_pad and c.B == 2 and c.heads == 3 for c in FWD)
        for T in R.BWD_T:
            assert any(c.d == d and c.T == T and c.kind == "gauss" for c in BWD)
        assert any(c.d == d and c.kind == "gather" for c in FWD)
    # both denominator forms under every peaked kind, every ragged T with a non-empty partial tile, one-tile and many-tile cases
    for kind in ("peak_last", "peak_first", "qscale"):
        assert {R.ones_column(c.d) for c in FWD if c.kind == kind} == {True, False}
        assert {R.ones_column(c.d) for c in BWD if c.kind == kind} == {True, False}
        assert all(c.T % 64 for c in FWD + BWD if c.kind == kind)
    ragged = [T for T in R.FWD_T + R.BWD_T if T % 64]
    assert all(0 < T % 64 < 64 for T in ragged) and {1, 7, 16, 63, 65, 127, 129, 200, 257} <= set(ragged)
    assert any(T % 128 == 1 for T in ragged) and any(T % 128 == 127 for T in ragged)
    assert {c.T for c in FWD if c.Tstride} == {16, 129, 257} and {c.d for c in FWD if c.Tstride} == {40, 64}
    assert all((not c.Tstride or c.Tstride >= c.T) and c.ld_pad % 8 == 0 for c in FWD)
    assert any(c.heads == 16 and c.d == 64 and c.T == 257 and c.Tstride == 264 for c in FWD)
    assert max(c.T for c in FWD + BWD) == 1024
    # the XCD remap's remainder branch (workgroup count % 8 != 0) and its even branch both run
    counts = [-(-c.T // 128) * c.heads * c.B for c in R.xcd_cases()]
    assert len(counts) == 6 and any(n % 8 for n in counts) and any(n % 8 == 0 for n in counts) and 6 in counts and 12 in counts
    z = [c for c in BWD if c.kind == "do_zero_tail"]
    assert len(z) == 1 and z[0].T % 64


@pytest.mark.parametrize("c", FWD, ids=[c.name for c in FWD])
def test_forward_emulation_within_bound(c):
    q, k, v = R.make_inputs(c, DT)
    for t in (q, k, v):
        assert torch.equal(R.rnd16(t, DT), t) and torch.isfinite(t).all()
    want, apv, _, p = R.ref_forward(q, k, v, c.heads)
    got = R.emulate_forward(q, k, v, c.heads, DT)
    if c.kind == "gather":
        # one-hot below 2^-24, at the permuted key; the emulation returns the selected row of V exactly
        perm = R.gather_perm(c.T, R._seed(c))
        top = p.max(-1)
        assert (1 - top.values).max() < 2.0 ** -24 and (top.indices == perm[None, None, :]).all()
        assert torch.equal(got, v[:, perm])
        assert len({tuple(r.tolist()) for r in v[0]}) == c.T, "V rows must be distinct"
        return
    ratio = R.forward_ratio(got, want, apv, U, factor=1.5)
    rl2 = ((got.double() - want).norm() / want.norm()).item()
    print(f"[parity] forward emulation {c.name}: worst |err| / (1.5 u sum P|V| + 2^-24) = {ratio:.3f}, relL2 {rl2:.2e}")
    assert ratio <= 1.0, (c.name, ratio)


@pytest.mark.parametrize("c", BWD, ids=[c.name for c in BWD])
def test_backward_emulation_within_half_the_bound(c):
    q, k, v, do = R.make_inputs(c, DT, backward=True)
    sl = slice(0, (c.T // 64) * 64) if c.kind == "do_zero_tail" else None
    dq_r, dk_r, dv_r, lse_r, delta_r, o_r, apv, scale = R.ref_backward(q, k, v, do, c.heads, queries=sl)
    dq, dk, dv, lse2, delta, o16 = R.emulate_backward(q, k, v, do, c.heads, DT)
    errs = [R.worst_slice_rel_l2(g, w, c.heads, sc) for g, w, sc in ((dq, dq_r, scale[0]), (dk, dk_r, scale[1]), (dv, dv_r, None))]
    rl, rd, ro = R.lse_ratio(lse2, lse_r), R.delta_ratio(delta, delta_r, do, o_r, apv, c.heads, U), R.forward_ratio(o16, o_r, apv, U)
    print(f"[parity] backward emulation {c.name}: worst slice relL2 dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}; "
          f"ratios to bound lse {rl:.3f} delta {rd:.3f} o {ro:.3f}")
    assert max(errs) <= 0.5 * R.backward_bound(U), (c.name, errs)
    assert rl <= 1.0 and rd <= 1.0 and ro <= 1.0
    if c.kind == "do_zero_tail":
        assert (delta[:, :, sl.stop:] == 0).all() and (delta_r[:, :, sl.stop:] == 0).all()


@pytest.mark.parametrize("case", R.DEPTH_CASES, ids=[str(c) for c in R.DEPTH_CASES])
def test_depth_references_are_autograd(case):
    B, HW, D, hn, hd = case
    q, k, v, dz = R.depth_inputs(case)
    sim, attn, z = R.ref_depth_forward(q, k, v, HW, D, hn)
    assert sim.abs().max() <= 30.0
    if hn == 4 and D > 1:
        assert abs(sim[0, 1, D - 1].item() - 24.0) < 1e-4 and attn[0, 1, D - 1] > 0.999  # the peaked row
    qq, kk, vv = (t.double().requires_grad_(True) for t in (q, k, v))
    I = hn * hd
    qd, kd, vd = qq.reshape(B, HW, hn, hd), kk.reshape(B, D, HW, hn, hd), vv.reshape(B, D, HW, hn, hd)
    # DepthAttention.forward: per pixel and head, softmax over the D depth samples
    a = torch.softmax((qd[:, None] * kd).sum(-1) * hd ** -0.5, 1)  # [B, D, HW, hn]
    zz = (a[..., None] * vd).sum(1).reshape(B * HW, I)
    assert (zz.detach() - z).abs().max() <= 1e-12 and (a.detach().permute(0, 2, 3, 1).reshape(B * HW, hn, D) - attn).abs().max() <= 1e-13
    zz.backward(dz.double())
    dq, dk, dv = R.ref_depth_backward(q, k, v, attn, dz, HW, D, hn)
    for got, want in ((dq, qq.grad), (dk, kk.grad), (dv, vv.grad)):
        assert (got - want).abs().max() <= 1e-11 * max(1.0, want.abs().max().item())
    assert R.pixel_slices(k, B, HW, D).shape == (B * HW, D * I) and R.pixel_ratio(dk + 1e-9, dk, B, HW, D) > 0


def test_depth_case_table_covers_what_it_claims():
    I = [hn * hd for _, _, _, hn, hd in R.DEPTH_CASES]
    assert min(I) < 256 and any(256 < i < 1024 for i in I) and max(I) == 1024  # below and above one pass of the 256 threads; the LDS limit
    assert any(hd % 64 for *_, hd in R.DEPTH_CASES) and any(hd > 64 for *_, hd in R.DEPTH_CASES)
    assert any(hn * D <= 4 for _, _, D, hn, _ in R.DEPTH_CASES) and any(hn * D > 4 and (hn * D) % 4 for _, _, D, hn, _ in R.DEPTH_CASES)  # the 4 waves
    assert {1, 64} <= {D for _, _, D, _, _ in R.DEPTH_CASES}
    assert [(D > 64, hn > 4, hn * hd > 1024) for _, _, D, hn, hd in R.DEPTH_REFUSED] == [(True, False, False), (False, True, False), (False, False, True)]


@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=[str(c) for c in R.IM2COL_CASES])
def test_data_movement_references(case):
    """im2col followed by the permuted weight matrix IS the 3x3 convolution; col2im is its transpose"""
    B, H, W, Cc = case
    g = torch.Generator().manual_seed(H * W + Cc)
    x = torch.randn(B, H, W, Cc, generator=g).double()
    w = torch.randn(5, Cc, 3, 3, generator=g).double()
    col = R.ref_im2col3(x)
    assert col.shape == (B * H * W, 9 * Cc)
    got = col @ R.ref_perm_w3(w, True).reshape(5, 9 * Cc).t()
    want = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, 5)
    assert (got - want).abs().max() <= 1e-12
    assert torch.equal(R.ref_perm_w3(R.ref_perm_w3(w, True), False), w)
    dcol = torch.randn(B * H * W, 9 * Cc, generator=g).double()
    assert abs((R.ref_col2im3(dcol, B, H, W) * x).sum() - (dcol * col).sum()) <= 1e-9  # <A^T y, x> = <y, A x>
    # the tap convention of k_train.hip: column tap * C + c holds X[y + tap / 3 - 1, x + tap % 3 - 1, c]
    xi = R.impulse_images(B, H, W, Cc)[0]
    (b, y, x_, ch), = xi.nonzero().tolist()
    ci = R.ref_im2col3(xi)
    for tap in range(9):
        yy, xx = y - (tap // 3 - 1), x_ - (tap % 3 - 1)  # the pixel whose tap `tap` sees the impulse
        if 0 <= yy < H and 0 <= xx < W:
            assert ci[(b * H + yy) * W + xx, tap * Cc + ch] == 1
    assert ci.sum() == sum(1 for tap in range(9) if 0 <= y - (tap // 3 - 1) < H and 0 <= x_ - (tap % 3 - 1) < W)


def test_new_hooks_are_in_the_abi():
    """argument counts through lib.py, which derives them from include/mvd.h"""
    from morphablediffusion_amd import lib as L
    want = {"mvd_op_attention_ex": 13, "mvd_op_attention_bwd_ex": 16, "mvd_op_train_depth_attn": 11, "mvd_op_train_depth_attn_bwd": 14,
            "mvd_op_train_im2col3": 7, "mvd_op_train_col2im3": 7, "mvd_op_train_perm_w3": 6}
    lib = L.load()
    for name, n in want.items():
        assert name in L.PROTOTYPES and L.PROTOTYPES[name][0] is C.c_int and len(L.PROTOTYPES[name][1]) == n, name
        assert len(getattr(lib, name).argtypes) == n
    I, P = C.c_int, C.c_void_p
    assert L.PROTOTYPES["mvd_op_attention_ex"][1] == [P] * 4 + [I] * 7 + [P, P]
    # bad arguments are refused before the device is touched: a null context, and (context-free hooks) null buffers
    assert lib.mvd_op_attention_ex(None, None, None, None, 1, 1, 1, 8, 0, 0, -1, None, None) != 0
    assert lib.mvd_op_train_depth_attn(None, None, None, 1, 1, 1, 1, 8, None, None, None) != 0
    assert b"null" in lib.mvd_last_error()
    assert lib.mvd_op_train_im2col3(None, 1, 1, 1, 1, None, None) != 0 and lib.mvd_op_train_perm_w3(None, 1, 1, 1, None, None) != 0

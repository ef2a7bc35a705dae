"""The LoRA kernels (csrc/k_lora.hip) on raw buffers, through the stateless hooks mvd_op_lora_project / mvd_op_lora_merge and their
grouped forms: against a float64 torch restatement on the CPU, the grouped launch against the single-target one with sentinels
around every tensor, bit reproducibility, argument checks.

Bound: the test computes e_ref, the normalised max error of torch's CPU fp32 matmul against the float64 result on the same
inputs; the kernel must stay within 8 e_ref + 2e-6 (8: another blocking of the same fp32 sums; 2e-6: the floor the AdamW op tests
use).  Both numbers are printed."""
import ctypes as C

import pytest
import torch

from morphablediffusion_amd import lib as L

pytestmark = pytest.mark.gpu

SCALE = 2.0
CASES = [(1, 1, 1), (40, 72, 4), (65, 130, 64), (64, 768, 16), (2048, 256, 8), (1280, 320, 1)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nerr(got, want):
    return ((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def _inputs(out, in_, r, seed=0):
    g = torch.Generator().manual_seed(100 + seed + out * 7 + in_ * 3 + r)
    dW = torch.randn(out, in_, generator=g) * 1e-2 * 65536.0  # a loss-scaled gradient
    W0 = torch.randn(out, in_, generator=g) * 0.05
    A = (torch.rand(r, in_, generator=g) * 2 - 1) / in_ ** 0.5
    B = torch.randn(out, r, generator=g) * 0.02
    return dW, W0, A, B


def _project(dW, A, B, r, scale=SCALE):
    out, in_ = dW.shape
    gA = torch.full((r, in_), float("nan"), device="cuda")
    gB = torch.full((out, r), float("nan"), device="cuda")
    L.check(L.load().mvd_op_lora_project(L.ptr(dW), L.ptr(A), L.ptr(B), out, in_, r, scale, L.ptr(gA), L.ptr(gB), _stream()))
    return gA, gB


def _merge(W0, A, B, r, scale=SCALE):
    out, in_ = W0.shape
    W = torch.full((out, in_), float("nan"), device="cuda")
    L.check(L.load().mvd_op_lora_merge(L.ptr(W0), L.ptr(A), L.ptr(B), out, in_, r, scale, L.ptr(W), _stream()))
    return W


@pytest.mark.parametrize("out,in_,r", CASES)
def test_project_and_merge_vs_float64(out, in_, r):
    dW, W0, A, B = _inputs(out, in_, r)
    d64, w64, a64, b64 = dW.double(), W0.double(), A.double(), B.double()
    want = {"gA": SCALE * b64.t() @ d64, "gB": SCALE * d64 @ a64.t(), "W": w64 + SCALE * b64 @ a64}
    ref32 = {"gA": SCALE * (B.t() @ dW), "gB": SCALE * (dW @ A.t()), "W": W0 + SCALE * (B @ A)}
    dev = [t.cuda() for t in (dW, W0, A, B)]
    gA, gB = _project(dev[0], dev[2], dev[3], r)
    W = _merge(dev[1], dev[2], dev[3], r)
    torch.cuda.synchronize()
    got = {"gA": gA.cpu(), "gB": gB.cpu(), "W": W.cpu()}
    fails = []
    for name in ("gA", "gB", "W"):
        assert torch.isfinite(got[name]).all(), name
        e_ref, e = _nerr(ref32[name], want[name]), _nerr(got[name], want[name])
        bound = 8 * e_ref + 2e-6
        print(f"[lora ops] ({out}, {in_}, r={r}) {name}: kernel {e:.3e}, torch CPU fp32 e_ref {e_ref:.3e}, bound {bound:.3e}")
        if not e <= bound:
            fails.append((name, e, bound))
    assert not fails, fails
    # two runs of each kernel: bit-identical (no atomic, sums ordered by indices alone)
    gA2, gB2 = _project(dev[0], dev[2], dev[3], r)
    W2 = _merge(dev[1], dev[2], dev[3], r)
    assert torch.equal(gA, gA2) and torch.equal(gB, gB2) and torch.equal(W, W2)
    # strength 0 is W0 itself
    assert torch.equal(_merge(dev[1], dev[2], dev[3], r, scale=0.0), dev[1])


def _pad64(n):
    return (n + 63) // 64 * 64


def test_grouped_launch_equals_single_targets_and_keeps_the_padding():
    """Three targets of different shapes in one arena at the 64-float-aligned offsets the engine uses; a sentinel in every padding
    slot and in the 64 floats before and after each arena."""
    lib = L.load()
    r, S = 8, -12345.0
    shapes = [(40, 72), (65, 130), (96, 257)]  # (none a multiple of the 32 x 128 tile; the last with an odd row length)
    G = 64  # guard floats at both ends
    w_off, a_off, b_off, w0_off = [], [], [], []
    wn = an = w0n = 0
    for o, i in shapes:
        w_off.append(G + wn)
        wn += _pad64(o * i) + 64  # (another tensor's worth of foreign floats between the targets, as in the full arena)
        w0_off.append(G + w0n)
        w0n += _pad64(o * i)
        a_off.append(G + an)
        an += _pad64(r * i)
        b_off.append(G + an)
        an += _pad64(o * r)
    dWa = torch.full((wn + 2 * G,), S)
    W0a = torch.full((w0n + 2 * G,), S)
    Pa = torch.full((an + 2 * G,), S)
    single = []
    for t, (o, i) in enumerate(shapes):
        dW, W0, A, B = _inputs(o, i, r, seed=t)
        dWa[w_off[t]:w_off[t] + o * i] = dW.reshape(-1)
        W0a[w0_off[t]:w0_off[t] + o * i] = W0.reshape(-1)
        Pa[a_off[t]:a_off[t] + r * i] = A.reshape(-1)
        Pa[b_off[t]:b_off[t] + o * r] = B.reshape(-1)
        dev = [x.cuda() for x in (dW, W0, A, B)]
        single.append(_project(dev[0], dev[2], dev[3], r) + (_merge(dev[1], dev[2], dev[3], r),))
    dWa, W0a, Pa = dWa.cuda(), W0a.cuda(), Pa.cuda()
    Ga = torch.full_like(Pa, S)
    Wa = torch.full_like(dWa, S)
    arr = lambda v: (C.c_int64 * len(v))(*v)
    outs, ins = arr([o for o, _ in shapes]), arr([i for _, i in shapes])
    L.check(lib.mvd_op_lora_project_grouped(L.ptr(dWa), L.ptr(Pa), L.ptr(Pa), 3, arr(w_off), outs, ins, arr(a_off), arr(b_off), r, SCALE,
                                            L.ptr(Ga), L.ptr(Ga), _stream()))
    L.check(lib.mvd_op_lora_merge_grouped(L.ptr(W0a), L.ptr(Pa), L.ptr(Pa), 3, arr(w_off), arr(w0_off), outs, ins, arr(a_off),
                                          arr(b_off), r, SCALE, L.ptr(Wa), _stream()))
    torch.cuda.synchronize()
    live_g, live_w = torch.zeros_like(Ga, dtype=torch.bool), torch.zeros_like(Wa, dtype=torch.bool)
    for t, (o, i) in enumerate(shapes):
        gA, gB, W = single[t]
        assert torch.equal(Ga[a_off[t]:a_off[t] + r * i].view(r, i), gA), t
        assert torch.equal(Ga[b_off[t]:b_off[t] + o * r].view(o, r), gB), t
        assert torch.equal(Wa[w_off[t]:w_off[t] + o * i].view(o, i), W), t
        live_g[a_off[t]:a_off[t] + r * i] = True
        live_g[b_off[t]:b_off[t] + o * r] = True
        live_w[w_off[t]:w_off[t] + o * i] = True
    assert bool((Ga[~live_g] == S).all()) and bool((Wa[~live_w] == S).all()), "a padding or guard float was written"
    assert int((~live_g).sum()) >= 2 * G and int((~live_w).sum()) >= 2 * G + 3 * 64


def test_bad_arguments_are_errors_and_launch_nothing():
    lib = L.load()
    out, in_, r = 8, 12, 4
    dW, W0, A, B = [t.cuda() for t in _inputs(out, in_, r)]
    gA, gB = torch.full((r, in_), 7.0, device="cuda"), torch.full((out, r), 7.0, device="cuda")
    W = torch.full((out, in_), 7.0, device="cuda")
    p = L.ptr
    s = _stream()
    for rank in (0, 65, -1):
        assert lib.mvd_op_lora_project(p(dW), p(A), p(B), out, in_, rank, SCALE, p(gA), p(gB), s) != 0
        assert lib.mvd_op_lora_merge(p(W0), p(A), p(B), out, in_, rank, SCALE, p(W), s) != 0
        assert b"rank" in lib.mvd_last_error()
    for k in range(5):
        args = [p(dW), p(A), p(B), p(gA), p(gB)]
        args[k] = None
        assert lib.mvd_op_lora_project(args[0], args[1], args[2], out, in_, r, SCALE, args[3], args[4], s) != 0
    for k in range(4):
        args = [p(W0), p(A), p(B), p(W)]
        args[k] = None
        assert lib.mvd_op_lora_merge(args[0], args[1], args[2], out, in_, r, SCALE, args[3], s) != 0
    assert lib.mvd_op_lora_project(p(dW), p(A), p(B), 0, in_, r, SCALE, p(gA), p(gB), s) != 0
    assert lib.mvd_op_lora_merge(p(W0), p(A), p(B), out, 0, r, SCALE, p(W), s) != 0
    torch.cuda.synchronize()
    assert bool((gA == 7.0).all()) and bool((gB == 7.0).all()) and bool((W == 7.0).all())

"""GPU: the backward kernels of the training step (k_bwd.hip) one by one, through the C ABI, against torch.autograd of the
same op in fp32 on the CPU.  Bounds: fp32 kernels 1e-5; the attention backward computes on fp16 operands (its inputs are
rounded to fp16 on both sides of the comparison, what remains is the fp16 rounding of P / dS inside the kernel): 3e-3."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig
    e = Engine(UNetConfig(model_channels=64), VolumeConfig(), workspace_gb=2.0)
    yield e
    e.close()


def rel(a, b):
    return ((a.cpu() - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("B,T,heads,d", [(2, 1024, 8, 40), (2, 256, 8, 80), (3, 64, 8, 160), (2, 1024, 8, 8), (1, 256, 8, 16),
                                         (2, 64, 8, 32), (1, 4096, 2, 64)])
def test_attention_backward(eng, B, T, heads, d):
    g = torch.Generator().manual_seed(T + d)
    C = heads * d
    q, k, v, do = [torch.randn(B, T, C, generator=g).half().float() for _ in range(4)]
    q *= 1.5  # sharper softmax than unit-variance scores
    qq, kk, vv = [t.clone().requires_grad_(True) for t in (q, k, v)]

    def split(t):
        return t.view(B, T, heads, d).transpose(1, 2)

    att = torch.softmax(split(qq) @ split(kk).transpose(-1, -2) / d ** 0.5, -1)
    out = (att @ split(vv)).transpose(1, 2).reshape(B, T, C)
    out.backward(do)
    dq, dk, dv = eng.op_attention_bwd(q, k, v, do, heads)
    errs = [rel(dq, qq.grad), rel(dk, kk.grad), rel(dv, vv.grad)]
    print(f"[parity] attention backward B={B} T={T} d={d}: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")
    assert max(errs) <= 3e-3, errs


@pytest.mark.parametrize("B,rows,C,G,act", [(2, 1024, 320, 32, 1), (3, 256, 960, 32, 1), (2, 64, 2560, 32, 1), (2, 16, 1280, 32, 0),
                                            (2, 1024, 128, 8, 2), (1, 49152, 64, 8, 2), (2, 64, 1024, 8, 1)])
def test_group_norm_backward(eng, B, rows, C, G, act):
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(B, rows, C, generator=g) * 1.3 + 0.2
    dy = torch.randn(B, rows, C, generator=g)
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    xx, gg, bb = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.group_norm(xx.transpose(1, 2), G, gg, bb, 1e-5).transpose(1, 2)
    y = torch.nn.functional.silu(y) if act == 1 else (torch.relu(y) if act == 2 else y)
    y.backward(dy)
    dx, dg, db = eng.op_group_norm_bwd(x, dy, G, gamma, beta, 1e-5, act)
    errs = [rel(dx, xx.grad), rel(dg, gg.grad), rel(db, bb.grad)]
    print(f"[parity] GroupNorm backward rows={rows} C={C} G={G} act={act}: dx {errs[0]:.2e} dgamma {errs[1]:.2e} dbeta {errs[2]:.2e}")
    assert max(errs) <= 2e-5, errs


@pytest.mark.parametrize("rows,C", [(2048, 320), (512, 640), (130, 1280), (7, 64)])
def test_layer_norm_backward(eng, rows, C):
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g) * 2.0 - 0.5
    dy = torch.randn(rows, C, generator=g)
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    xx, gg, bb = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xx, (C,), gg, bb, 1e-5).backward(dy)
    dx, dg, db = eng.op_layer_norm_bwd(x, dy, gamma)
    errs = [rel(dx, xx.grad), rel(dg, gg.grad), rel(db, bb.grad)]
    print(f"[parity] LayerNorm backward rows={rows} C={C}: dx {errs[0]:.2e} dgamma {errs[1]:.2e} dbeta {errs[2]:.2e}")
    assert max(errs) <= 2e-5, errs


# ---- adjoints of the training step's convolutions, Linears and GEMMs (engine_train.hip), one layer at a time ---------------------
# Reference: torch.autograd of the same op in float64 on the CPU.  Exact-operand cases round x, w and dy to the library's operand
# type on both sides, so that only the order of the fp32 accumulation separates kernel and reference; raw-fp32 cases take the
# operand rounding as well.  Every case runs twice, the second time with the free workspace poisoned (0xFF bytes: NaN in every
# float type): the two results must be bit-identical and finite -- a difference is a read of memory the op never wrote.
import torch.nn.functional as F  # noqa: E402

from morphablediffusion_amd import lib as _lib  # noqa: E402

OPD = torch.bfloat16 if _lib.DTYPE == "bf16" else torch.float16
U_OP = 2.0 ** -8 if _lib.DTYPE == "bf16" else 2.0 ** -11   # unit roundoff of the operand type
# Bounds from the measured values (MI355X; relative L2 / max error over max reference): exact operands, fp32 summation order only:
# at most 1.6e-7 / 4.1e-7 in fp16 and bf16.  Extended precision (xp) on raw fp32 operands: 1.9e-7 / 4.1e-7 (fp16 hi + lo parts),
# 4.5e-6 / 6.1e-6 (bf16).  FF1 GEGLU: 6.1e-6 / 5.2e-5 (rounding ties of the stored pre-activations / their gradients).  Raw fp32
# operands: 3.0e-4 (fp16), 2.4e-3 (bf16).  A result stored in the operand type (fp16 dx): 2.1e-4 / 3.7e-4 (fp16).
EXACT_REL, EXACT_MAX = 2e-6, 4e-6
XP_REL = EXACT_REL if _lib.DTYPE == "f16" else 5e-5
GEGLU_REL, GEGLU_MAX = 6e-5, 5e-4
RAW_REL = 1e-3 if _lib.DTYPE == "f16" else 8e-3
ONE_ROUND = 2 * U_OP


def qop(t):
    """t rounded to the library's MFMA operand type (exactly representable on both sides afterwards)"""
    return t.to(OPD).to(torch.float32)


def errs(got, want):
    """(relative L2, max |error| / max |reference|) of a kernel result against a float64 reference"""
    d = got.detach().cpu().double() - want
    return (d.norm() / (want.norm() + 1e-300)).item(), (d.abs().max() / (want.abs().max() + 1e-300)).item()


def clean_and_poisoned(run):
    """run(poison) -> tuple of tensors (or None); both runs must agree bit for bit and be finite"""
    a, b = run(False), run(True)
    for u, v in zip(a, b):
        if u is None:
            continue
        assert torch.isfinite(u).all(), "non-finite result"
        assert torch.equal(u, v), f"poisoned workspace changed the result (max diff {(u - v).abs().max().item():.3e})"
    return a


def asym_weight(shape, p=7):
    """asymmetric weights, exact in every operand type: a wrong tap flip or index relation cannot cancel"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, dtype=torch.float32) % p) - (p // 2)).reshape(shape) / 4 + 0.125


def prefill(g, like):
    return torch.randn(like.shape, generator=g) * (like.double().std().item() + 1e-3)


def ref_conv2d(x, w, dy, kind):
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    xi = x64.repeat_interleave(2, 2).repeat_interleave(2, 3) if kind == 2 else x64
    y = F.conv2d(xi, w64, b64, stride=2 if kind == 1 else 1, padding=w.shape[2] // 2)
    y.backward(dy.double())
    return x64.grad, w64.grad, b64.grad


def out_hw(kind, H, W):
    return ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if kind == 1 else ((2 * H, 2 * W) if kind == 2 else (H, W))


def report(tag, names, es):
    print(f"[parity] {tag}: " + " ".join(f"{n} {e[0]:.2e}/{e[1]:.2e}" for n, e in zip(names, es)))


# kind 0 plain (k 3 / 1), 1 Downsample, 2 Upsample; xh: x read as fp16 (the ResBlock's saved activations); raw: fp32 operands
CONV_CASES = [  # kind, k, B, Cin, Cout, H, xh, xp, accum, raw, need_din
    (0, 3, 2, 8, 64, 32, 0, 0, 0, 0, 1),        # conv_in
    (0, 3, 1, 8, 64, 32, 0, 1, 0, 0, 0),        # conv_in, xp, no dx (the first layer)
    (0, 3, 2, 4, 16, 32, 0, 0, 0, 0, 1),        # 2-D encoder enc_init: 4 channels padded to 8
    (0, 3, 2, 64, 4, 32, 1, 0, 0, 0, 1),        # output conv: Cout 4, Np 8
    (0, 3, 2, 64, 4, 32, 1, 1, 1, 0, 1),        # ... xp, accum
    (0, 3, 2, 64, 64, 32, 1, 0, 0, 0, 1),       # ResBlock 32x32 (reduced width)
    (0, 3, 3, 128, 128, 16, 1, 1, 0, 0, 1),     # ResBlock 16x16, xp
    (0, 3, 2, 256, 256, 8, 1, 0, 1, 0, 1),      # ResBlock 8x8, accum
    (0, 3, 3, 256, 256, 4, 1, 0, 0, 0, 1),      # ResBlock 4x4, B*16 = 48 rows: ragged Rp
    (0, 3, 1, 640, 640, 4, 1, 0, 0, 0, 1),      # full width
    (0, 3, 2, 6, 12, 8, 0, 0, 0, 0, 1),         # scalar im2colT (Cin % 4 != 0)
    (0, 3, 2, 16, 6, 8, 1, 0, 0, 0, 1),         # scalar tcast / cast_rows (Cout % 4 != 0)
    (0, 1, 2, 96, 64, 16, 0, 0, 1, 0, 1),       # ResBlock skip 1x1, accum (adds into the block's dx)
    (0, 1, 3, 64, 128, 4, 1, 1, 1, 0, 1),       # skip 1x1, xp, fp16 x, ragged rows
    (1, 3, 2, 64, 64, 32, 0, 0, 0, 0, 1),       # Downsample 32 -> 16
    (1, 3, 3, 128, 128, 8, 0, 0, 1, 0, 1),      # Downsample 8 -> 4, accum
    (2, 3, 3, 128, 128, 4, 0, 0, 0, 0, 1),      # Upsample 4 -> 8
    (2, 3, 1, 64, 64, 16, 0, 0, 1, 0, 1),       # Upsample 16 -> 32, accum
    (0, 3, 2, 64, 64, 16, 1, 0, 0, 1, 1),       # raw fp32 operands
    (1, 3, 2, 64, 96, 16, 0, 0, 0, 1, 1),       # raw, Downsample
]


@pytest.mark.parametrize("kind,k,B,Cin,Cout,H,xh,xp,accum,raw,need_din", CONV_CASES)
def test_conv2d_backward(eng, kind, k, B, Cin, Cout, H, xh, xp, accum, raw, need_din):
    g = torch.Generator().manual_seed(1000 * kind + 10 * Cin + Cout + H + B)
    W = H
    Ho, Wo = out_hw(kind, H, W)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    dy = torch.randn(B, Cout, Ho, Wo, generator=g)
    if not raw:
        x, w, dy = qop(x), qop(w), qop(dy)
    rdx, rdw, rdb = ref_conv2d(x, w, dy, kind)
    acc = (prefill(g, rdx), prefill(g, rdw), prefill(g, rdb)) if accum else None
    dx, dw, db = clean_and_poisoned(lambda p: eng.op_conv_bwd(x, w, dy, kind=kind, x_half=bool(xh), xp=bool(xp), accum=acc,
                                                              need_din=bool(need_din), poison=p))
    if acc is not None:
        dx, dw, db = dx.cpu() - acc[0], dw.cpu() - acc[1], db.cpu() - acc[2]
    got = ([dx] if need_din else []) + [dw, db]
    want = ([rdx] if need_din else []) + [rdw, rdb]
    es = [errs(a, b) for a, b in zip(got, want)]
    report(f"conv2d backward kind={kind} k={k} B={B} {Cin}->{Cout} @{H} xh={xh} xp={xp} accum={accum} raw={raw}",
           (["dx"] if need_din else []) + ["dW", "db"], es)
    for e in es:
        if raw:
            assert e[0] <= RAW_REL, es
        else:
            assert e[0] <= EXACT_REL and e[1] <= EXACT_MAX, es


def ref_conv3d(x, w, dy, kind):
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    Cout = w.shape[1] if kind == 2 else w.shape[0]
    b64 = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    if kind == 2:
        y = F.conv_transpose3d(x64, w64, b64, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv3d(x64, w64, b64, stride=1 + kind, padding=1)
    y.backward(dy.double())
    return x64.grad, w64.grad, b64.grad


def out_dhw3(kind, D, H, W):
    return (2 * D, 2 * H, 2 * W) if kind == 2 else ((D // 2, H // 2, W // 2) if kind == 1 else (D, H, W))


CONV3D_CASES = [  # kind, B, Cin, Cout, (D, H, W), xh, accum, raw
    (0, 1, 16, 16, (12, 8, 8), 1, 0, 0),     # frustum level 2 (reduced channels), fp16 saved activation as in the training step
    (0, 2, 32, 32, (6, 4, 4), 1, 1, 0),      # level 3, accum
    (0, 2, 24, 40, (6, 4, 4), 0, 0, 0),      # fp32 x, Cout 40
    (1, 1, 16, 32, (24, 16, 16), 1, 0, 0),   # stride 2 from (24, 16, 16)
    (1, 2, 32, 32, (12, 8, 8), 1, 1, 0),     # stride 2 from level 2, accum
    (2, 1, 32, 16, (12, 8, 8), 1, 0, 0),     # transposed to (24, 16, 16)
    (2, 2, 32, 32, (6, 4, 4), 1, 1, 0),      # transposed to level 2, accum
    (0, 1, 16, 16, (12, 8, 8), 0, 0, 1),     # raw fp32 operands
    (2, 1, 16, 16, (6, 4, 4), 0, 0, 1),      # raw, transposed
]


@pytest.mark.parametrize("kind,B,Cin,Cout,dhw,xh,accum,raw", CONV3D_CASES)
def test_conv3d_backward(eng, kind, B, Cin, Cout, dhw, xh, accum, raw):
    g = torch.Generator().manual_seed(77 * kind + Cin + 3 * Cout + sum(dhw))
    D, H, W = dhw
    x = torch.randn(B, Cin, D, H, W, generator=g)
    w = torch.randn(*((Cin, Cout) if kind == 2 else (Cout, Cin)), 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    dy = torch.randn(B, Cout, *out_dhw3(kind, D, H, W), generator=g)
    if not raw:
        x, w, dy = qop(x), qop(w), qop(dy)
    rdx, rdw, rdb = ref_conv3d(x, w, dy, kind)
    acc = (prefill(g, rdx), prefill(g, rdw), prefill(g, rdb)) if accum else None
    dx, dw, db = clean_and_poisoned(lambda p: eng.op_conv3d_bwd(x, w, dy, kind=kind, x_half=bool(xh), accum=acc, poison=p))
    if acc is not None:
        dx, dw, db = dx.cpu() - acc[0], dw.cpu() - acc[1], db.cpu() - acc[2]
    es = [errs(dx, rdx), errs(dw, rdw), errs(db, rdb)]
    report(f"conv3d backward kind={kind} B={B} {Cin}->{Cout} @{dhw} xh={xh} accum={accum} raw={raw}", ["dx", "dW", "db"], es)
    for e in es:
        if raw:
            assert e[0] <= RAW_REL, es
        else:
            assert e[0] <= EXACT_REL and e[1] <= EXACT_MAX, es


# one-hot dy at a corner and at an edge output pixel of the last / first sample: dx is the (flipped, strided, upsampled) weight
# footprint of that output, exactly -- a wrong flip, tap offset or o = 2 i - 1 + k relation moves or drops taps (O(1) errors)
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("where", ["corner", "edge"])
def test_conv2d_backward_impulse_footprint(eng, kind, where):
    B, Cin, Cout, H = 2, 16, 8, 8
    W = H
    Ho, Wo = out_hw(kind, H, W)
    x = qop(torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(3)))
    w = asym_weight((Cout, Cin, 3, 3))
    dy = torch.zeros(B, Cout, Ho, Wo)
    if where == "corner":
        dy[B - 1, Cout - 1, Ho - 1, Wo - 1] = 1.0
    else:
        dy[0, 2, 0, Wo // 2] = 1.0
    rdx, rdw, rdb = ref_conv2d(x, w, dy, kind)
    dx, dw, db = clean_and_poisoned(lambda p: eng.op_conv_bwd(x, w, dy, kind=kind, poison=p))
    dx = dx.cpu().double()
    print(f"[parity] conv2d impulse kind={kind} {where}: footprint {int((rdx != 0).sum())} taps, max |dx - ref| "
          f"{(dx - rdx).abs().max().item():.1e}")
    assert torch.equal(dx != 0, rdx != 0), "the footprint is in the wrong place"
    assert (dx - rdx).abs().max().item() <= 1e-6 * rdx.abs().max().item()
    assert errs(dw, rdw)[1] <= EXACT_MAX and errs(db, rdb)[1] <= EXACT_MAX


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("where", ["corner", "edge"])
def test_conv3d_backward_impulse_footprint(eng, kind, where):
    B, Cin, Cout, dhw = 2, 8, 8, (4, 4, 4)
    w = asym_weight((Cin, Cout, 3, 3, 3) if kind == 2 else (Cout, Cin, 3, 3, 3))
    x = qop(torch.randn(B, Cin, *dhw, generator=torch.Generator().manual_seed(4)))
    od = out_dhw3(kind, *dhw)
    dy = torch.zeros(B, Cout, *od)
    if where == "corner":
        dy[B - 1, Cout - 1, od[0] - 1, od[1] - 1, od[2] - 1] = 1.0
    else:
        dy[0, 3, 0, od[1] // 2, 0] = 1.0
    rdx, rdw, rdb = ref_conv3d(x, w, dy, kind)
    dx, dw, db = clean_and_poisoned(lambda p: eng.op_conv3d_bwd(x, w, dy, kind=kind, poison=p))
    dx = dx.cpu().double()
    print(f"[parity] conv3d impulse kind={kind} {where}: footprint {int((rdx != 0).sum())} taps, max |dx - ref| "
          f"{(dx - rdx).abs().max().item():.1e}")
    assert torch.equal(dx != 0, rdx != 0), "the footprint is in the wrong place"
    assert (dx - rdx).abs().max().item() <= 1e-6 * rdx.abs().max().item()
    assert errs(dw, rdw)[1] <= EXACT_MAX and errs(db, rdb)[1] <= EXACT_MAX


LINEAR_CASES = [  # B, rows, K, N, xh, dx_half, staged, xp, accum, raw
    (2, 512, 64, 64, 0, 0, 1, 0, 0, 0),    # proj_out (fp32 dy staged as rows16 + transposed image)
    (3, 48, 128, 128, 1, 0, 1, 0, 1, 0),   # ragged Rp, accum
    (2, 256, 64, 64, 1, 1, 1, 0, 0, 0),    # attention output projection: fp16 dx
    (2, 256, 256, 64, 1, 0, 1, 0, 0, 0),   # ff2
    (2, 200, 40, 20, 0, 0, 0, 0, 0, 0),    # unstaged: wgrad_linear's own transposing cast
    (1, 70, 6, 10, 0, 0, 1, 0, 1, 0),      # scalar tcast / cast_rows forms, K padded to 8
    (2, 256, 64, 64, 0, 0, 1, 1, 0, 0),    # proj_in / proj_out in the xp layout
    (2, 256, 64, 64, 0, 0, 1, 0, 0, 1),    # raw fp32 operands
]


def ref_linear(x, w, dy):
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    F.linear(x64, w64, b64).backward(dy.double())
    return x64.grad, w64.grad, b64.grad


@pytest.mark.parametrize("B,rows,K,N,xh,dxh,staged,xp,accum,raw", LINEAR_CASES)
def test_linear_backward(eng, B, rows, K, N, xh, dxh, staged, xp, accum, raw):
    g = torch.Generator().manual_seed(rows + 7 * K + N)
    x = torch.randn(rows, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    dy = torch.randn(rows, N, generator=g)
    if not raw:
        x, w, dy = qop(x), qop(w), qop(dy)
    rdx, rdw, rdb = ref_linear(x, w, dy)
    acc = (prefill(g, rdx), prefill(g, rdw), prefill(g, rdb)) if accum else None
    if acc is not None and dxh:
        acc = (qop(acc[0]),) + acc[1:]
    dx, dw, db = clean_and_poisoned(lambda p: eng.op_linear_bwd(x, w, dy, B=B, x_half=bool(xh), dx_half=bool(dxh), staged=bool(staged),
                                                                xp=bool(xp), accum=acc, poison=p))
    if acc is not None:
        dx, dw, db = dx.cpu() - acc[0], dw.cpu() - acc[1], db.cpu() - acc[2]
    es = [errs(dx, rdx), errs(dw, rdw), errs(db, rdb)]
    report(f"linear backward B={B} rows={rows} {K}->{N} xh={xh} dx_half={dxh} staged={staged} xp={xp} accum={accum} raw={raw}",
           ["dx", "dW", "db"], es)
    for i, e in enumerate(es):
        if raw:
            assert e[0] <= RAW_REL, es
        elif i == 0 and dxh:
            assert e[0] <= ONE_ROUND and e[1] <= ONE_ROUND, es
        else:
            assert e[0] <= EXACT_REL and e[1] <= EXACT_MAX, es


@pytest.mark.parametrize("B,rows,C,accum", [(2, 256, 64, 0), (3, 48, 32, 1)])
def test_ff1_geglu_backward(eng, B, rows, C, accum):
    """FF1 + GEGLU (modules/attention.py:37-45): the kernel re-computes the pre-activations and stores them in the operand type,
    and stores dL/dpre in it; the reference applies the same two roundings, so what remains is the summation order and the odd
    rounding tie"""
    g = torch.Generator().manual_seed(rows + C)
    N = 8 * C
    x = qop(torch.randn(rows, C, generator=g))
    w = qop(torch.randn(N, C, generator=g) / C ** 0.5)
    bias = torch.randn(N, generator=g) * 0.1
    dgg = qop(torch.randn(rows, N // 2, generator=g))
    pre = F.linear(x.double(), w.double(), bias.double()).to(OPD).double().requires_grad_(True)
    v, gate = pre.chunk(2, dim=-1)
    (v * F.gelu(gate)).backward(dgg.double())
    dpre = pre.grad.to(OPD).double()
    rdx, rdw, rdb = dpre @ w.double(), dpre.t() @ x.double(), dpre.sum(0)
    acc = (prefill(g, rdx), prefill(g, rdw), prefill(g, rdb)) if accum else None
    dx, dw, db = clean_and_poisoned(lambda p: eng.op_linear_bwd(x, w, dgg, B=B, bias=bias, geglu=True, accum=acc, poison=p))
    if acc is not None:
        dx, dw, db = dx.cpu() - acc[0], dw.cpu() - acc[1], db.cpu() - acc[2]
    es = [errs(dx, rdx), errs(dw, rdw), errs(db, rdb)]
    report(f"FF1 GEGLU backward B={B} rows={rows} C={C} accum={accum}", ["dx", "dW", "db"], es)
    for e in es:
        assert e[0] <= GEGLU_REL and e[1] <= GEGLU_MAX, es


TGEMM_CASES = [  # M, N, K, a_trans, b_trans, a_half, b_half, xp, accum, raw
    (67, 45, 83, 0, 1, 0, 0, 0, 0, 0),
    (67, 45, 83, 1, 0, 0, 0, 0, 0, 0),
    (33, 70, 19, 1, 1, 1, 0, 0, 1, 0),
    (50, 27, 77, 0, 0, 0, 1, 0, 0, 0),
    (64, 40, 96, 0, 1, 1, 1, 0, 0, 0),      # fp16 row-major operands used in place
    (96, 72, 1000, 1, 0, 0, 0, 0, 1, 0),    # a weight gradient: K = pixel rows
    (67, 45, 83, 0, 1, 0, 0, 1, 0, 1),      # xp on raw fp32 operands
    (45, 67, 130, 1, 0, 0, 0, 1, 1, 1),     # xp, accum
    (67, 45, 83, 0, 0, 0, 0, 0, 0, 1),      # raw fp32 operands, plain fp16 products
]


@pytest.mark.parametrize("M,N,K,at,bt,ah,bh,xp,accum,raw", TGEMM_CASES)
def test_tgemm(eng, M, N, K, at, bt, ah, bh, xp, accum, raw):
    g = torch.Generator().manual_seed(M * N + K)
    a = torch.randn(*((K, M) if at else (M, K)), generator=g)
    b = torch.randn(*((N, K) if bt else (K, N)), generator=g)
    if not raw:
        a, b = qop(a), qop(b)
    ref = (a.double().t() if at else a.double()) @ (b.double().t() if bt else b.double())
    c0 = torch.randn(M, N, generator=g) if accum else None
    out = clean_and_poisoned(lambda p: (eng.op_tgemm(a, b, a_trans=bool(at), b_trans=bool(bt), a_half=bool(ah), b_half=bool(bh), xp=bool(xp),
                                                     out=c0, poison=p),))[0]
    if c0 is not None:
        out = out.cpu() - c0
    e = errs(out, ref)
    report(f"tgemm M={M} N={N} K={K} trans={at}{bt} half={ah}{bh} xp={xp} accum={accum} raw={raw}", ["C"], [e])
    if xp:
        assert e[0] <= XP_REL and e[1] <= 2 * XP_REL, e
    elif raw:
        assert e[0] <= RAW_REL, e
    else:
        assert e[0] <= EXACT_REL and e[1] <= EXACT_MAX, e

"""CPU: the references of tests/small_ops_ref.py against torch modules or slow index loops, and the case tables of
tests/test_gpu_small_ops.py against the launchers' path predicates (restated in the reference module from csrc/k_misc.hip), so that
every case provably reaches the kernel form it names.  No GPU, no library."""
import math

import pytest
import torch
import torch.nn as nn

from tests import small_ops_ref as R

OPDS = [torch.float16, torch.bfloat16]


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a.double() - b.double()).abs().max().item() <= tol * max(1.0, b.double().abs().max().item())


# ---- 1. target encoder ----------------------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.n1, self.c1, self.n2, self.c2 = nn.GroupNorm(8, 16), nn.Conv2d(16, 16, 3, padding=1), nn.GroupNorm(8, 16), nn.Conv2d(16, 16, 3, padding=1)

    def forward(self, x, film):
        return x + self.c2(nn.functional.silu(self.n2(self.c1(nn.functional.silu(self.n1(x + film))))))


@pytest.mark.parametrize("family", R.ENC_FAMILIES)
def test_encoder_reference_is_the_module_network(family):
    """the unrounded float64 form against torch modules carrying the same parameters"""
    d = R.encoder_inputs(family, 3)
    init, blocks, fnorm, fconv = nn.Conv2d(4, 16, 3, padding=1), [_Block() for _ in range(3)], nn.GroupNorm(8, 16), nn.Conv2d(16, 16, 3, padding=1)
    convs = [init] + [m for b in blocks for m in (b.c1, b.c2)] + [fconv]
    norms = [m for b in blocks for m in (b.n1, b.n2)] + [fnorm]
    with torch.no_grad():
        for m, w, b in zip(convs, d["w"], d["bias"]):
            m.weight.copy_(w), m.bias.copy_(b)
        for m, g, b in zip(norms, d["gamma"], d["beta"]):
            m.weight.copy_(g), m.bias.copy_(b)
        for m in convs + norms:
            m.double()
        h = init(d["x"].double())
        for i, blk in enumerate(blocks):
            h = blk(h, d["pre"].double()[:, 16 * i:16 * i + 16, None, None])
        want = fconv(nn.functional.silu(fnorm(h))).permute(0, 2, 3, 1).reshape(-1, 16)
    close(R.encoder(d["x"], d["pre"], d["w"], d["bias"], d["gamma"], d["beta"], torch.float64, None), want)


@pytest.mark.parametrize("opd", OPDS)
@pytest.mark.parametrize("family", R.ENC_FAMILIES)
def test_encoder_families_are_finite_and_rounded_close_to_unrounded(family, opd):
    d = R.encoder_inputs(family)
    r64, r32 = R.encoder_refs(family, opd)
    assert r64.shape == (16 * 1024, 16) and torch.isfinite(r32).all() and torch.isfinite(r64).all()
    plain = R.encoder(d["x"], d["pre"], d["w"], d["bias"], d["gamma"], d["beta"], torch.float64, None)
    l2, _ = R.errs(r64, plain)
    assert l2 < (0.01 if opd == torch.float16 else 0.08), l2        # operand rounding is a perturbation, not another network
    e32 = R.errs(r32.double(), r64)     # a few flipped 16-bit roundings and nothing worse
    assert max(e32) < 8 * 2.0 ** -(11 if opd == torch.float16 else 8), e32


def test_encoder_views_are_rows_of_the_16_view_draw_and_differ():
    for family in R.ENC_FAMILIES:
        d16, d3 = R.encoder_inputs(family), R.encoder_inputs(family, 3)
        assert torch.equal(d16["x"][:3], d3["x"]) and torch.equal(d16["pre"][:3], d3["pre"])
        assert not torch.equal(d16["x"][0], d16["x"][1])
    d = R.encoder_inputs("random")
    for w in d["w"]:    # asymmetric: no two taps and no two channel slices alike
        taps = w.reshape(-1, 9)
        assert taps.unique(dim=1).shape[1] == 9 and w.reshape(w.shape[0], -1).unique(dim=0).shape[0] == w.shape[0]
        assert not torch.equal(w, w.flip(2)) and not torch.equal(w, w.flip(3)) and not torch.equal(w, w.transpose(2, 3))
    off = R.encoder_inputs("offset")["pre"]
    assert bool((off.abs() == 4).all()) and bool((off[:, 0::2] == off[:, 1::2]).all()) and (off > 0).any() and (off < 0).any()


def test_encoder_impulse_family_is_the_first_conv_alone():
    """zero second convs and a centre-tap identity at the end: the result is silu(gn(conv0(x))), rounded once, pixel by pixel"""
    d = R.encoder_inputs("impulse", 3)
    x = d["x"].double()
    assert int((x.abs().sum(dim=1) > 0).sum()) == 3 * len(R.ENC_IMPULSES)
    h = nn.functional.conv2d(R.r16(x, torch.float16), R.r16(d["w"][0].double(), torch.float16), d["bias"][0].double(), padding=1)
    want = R.r16(nn.functional.silu(nn.functional.group_norm(h, 8, d["gamma"][6].double(), d["beta"][6].double(), 1e-5)), torch.float16)
    got = R.encoder(d["x"], d["pre"], d["w"], d["bias"], d["gamma"], d["beta"], torch.float64, torch.float16)
    close(got, want.permute(0, 2, 3, 1).reshape(-1, 16))


# ---- 2. small linear ------------------------------------------------------------------------------------------------------------------
def test_small_linear_cases_reach_the_forms_they_name():
    c = R.SL_CASES
    for name, k in c.items():
        assert k["form"] == R.small_linear_form(k["K"], k["lda"], k["a_off"]), name
        assert k["lda"] >= k["K"] and k["ldo"] >= k["N"]
        assert name.startswith(("vec", "bc_vec")) == bool(k["form"]), name
    vec, sc = [k for k in c.values() if k["form"]], [k for k in c.values() if not k["form"]]
    assert {8, 256, 520, 1280} <= {k["K"] for k in vec}
    assert {4, 12} <= {k["K"] for k in sc} and any(k["lda"] == k["K"] + 1 for k in sc)
    assert any(k["a_off"] % 4 and k["K"] % 8 == 0 and k["lda"] % 4 == 0 for k in sc)         # scalar by the pointer alone
    assert {1, 8, 9, 17, -1, -16, -65} <= {k["rows"] for k in c.values()}
    assert {48, 6, 1} <= {k["N"] for k in c.values()}
    for key, vals in (("act", {0, 1}), ("accum", {0, 1}), ("bias", {0, 1})):
        assert {k[key] for k in vec} == vals and {k[key] for k in sc} == vals, key
    assert any(k["ldo"] > k["N"] for k in vec) and any(k["ldo"] > k["N"] for k in sc)
    # the vector loop: lane l takes k = 8 l, 8 l + 512, ...: K = 8 leaves 63 lanes idle, K = 520 gives lane 0 alone a second trip
    assert len(range(0, 8, 512)) == 1 and len(range(8, 8, 512)) == 0 and len(range(0, 520, 512)) == 2 and len(range(8, 520, 512)) == 1


@pytest.mark.parametrize("name", list(R.SL_CASES))
def test_small_linear_reference(name):
    c, d = R.SL_CASES[name], R.small_linear_inputs(name, torch.float16)
    assert torch.equal(d["w"], d["w"].half().float())
    a = nn.functional.silu(d["a"].double()) if c["act"] else d["a"].double()
    want = nn.functional.linear(a, d["w"].double(), None if d["bias"] is None else d["bias"].double())
    want = want.expand(-c["rows"], -1) if c["rows"] < 0 else want
    close(R.small_linear(d["a"], d["w"], d["bias"], c["rows"], c["act"], torch.float64), want)
    assert torch.isfinite(R.small_linear(d["a"], d["w"], d["bias"], c["rows"], c["act"], torch.float32)).all()
    assert (d["start"] is not None) == bool(c["accum"])


# ---- 3. timestep embedding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.TE_DIMS)
def test_timestep_embedding_reference(dim):
    t = torch.tensor(R.TE_STEPS[3])
    got = R.timestep_embedding(t, dim, torch.float64)
    half = dim // 2
    for b, tv in enumerate(t.tolist()):
        for j in range(dim):
            f = math.exp(-math.log(10000.0) * (j % half) / half) if half else 0.0
            want = 0.0 if j >= 2 * half else (math.cos(tv * f) if j < half else math.sin(tv * f))
            assert abs(got[b, j].item() - want) < 1e-12
    assert got.shape == (3, dim) and (dim % 2 == 0 or bool((got[:, -1] == 0).all()))
    assert torch.isfinite(R.timestep_embedding(t, dim, torch.float32)).all()


# ---- 4. layouts -----------------------------------------------------------------------------------------------------------------------
def test_layout_cases_sit_on_both_sides_of_the_tiled_threshold():
    B = R.LAYOUT_B
    for name, (C, HW, cpad, ld, form) in R.LAYOUT_CASES.items():
        assert form == R.layout_form(B, C, HW, cpad) == R.layout_form(B, C, HW, C), name
        assert C <= cpad <= ld
    forms = {(C, HW): f for C, HW, _, _, f in R.LAYOUT_CASES.values()}
    assert forms[(16, 32)] == 1 and forms[(15, 32)] == 0 and forms[(16, 31)] == 0
    assert any(C % 32 and HW % 32 and f for (C, HW), f in forms.items())                       # ragged tiles on both axes
    assert any(cpad > C and not f for C, _, cpad, _, f in R.LAYOUT_CASES.values())
    assert any(ld > cpad > C and f for C, _, cpad, ld, f in R.LAYOUT_CASES.values())


def test_layout_references():
    x = torch.randn(3, 5, 7)
    rows = R.nchw_to_nhwc(x, 8)
    for b in range(3):
        for p in range(7):
            for c in range(8):
                assert rows[b * 7 + p, c] == (x[b, c, p] if c < 5 else 0)
    padded = torch.cat([rows, torch.full((21, 3), float("nan"))], dim=1)
    assert torch.equal(R.nhwc_to_nchw(padded, 3, 5), x)


# ---- 5. packs and fills ---------------------------------------------------------------------------------------------------------------
def test_pack_weight_cases_reach_the_forms_they_name():
    c = R.PW_CASES
    for name, k in c.items():
        Cin = 3 * k["Cl"] if k["xp"] else k["Cl"]
        assert k["form"] == R.pack_weight_form(k["N"], Cin, k["taps"], k["transposed"], k["xp"], k["dst_off"]), name
        assert k["cin_src"] <= k["Cl"] and (not k["geglu"] or k["N"] % 64 == 0)
    by = lambda f: [k for k in c.values() if k["form"] == f]  # noqa: E731
    assert {1, 27} <= {k["taps"] for k in by(0)} and any(k["transposed"] and k["taps"] == 27 for k in by(0))
    assert any(k["geglu"] and k["N"] == 128 and k["taps"] == 1 for k in by(0))
    assert {9, 27} <= {k["taps"] for k in by(2)} and {3, 5} <= {k["N"] for k in by(2)}
    assert any(k["Cl"] % 8 for k in by(1)) and any(k["dst_off"] == 4 and k["Cl"] % 8 == 0 for k in by(1))  # dst_off 4 halfs = 8 bytes
    for f in (1, 2):
        assert any((k["cin_src"], k["Cl"]) == (70, 72) for k in by(f)) or f == 1 and any(k["cin_src"] < k["Cl"] for k in by(f))
        assert any(k["xp"] for k in by(f))
    assert any((k["cin_src"], k["Cl"]) == (4, 8) for k in by(2)) and any(k["xp"] for k in by(0))


@pytest.mark.parametrize("opd", OPDS)
@pytest.mark.parametrize("name", ["lin_geglu_n128", "t27_transposed", "t9_vec_xp_4to8", "t9_tap_off_70to72"])
def test_pack_weight_reference_against_the_index_loop(name, opd):
    k = R.PW_CASES[name]
    N, cs, Cl, taps = k["N"], k["cin_src"], k["Cl"], k["taps"]
    src = torch.randn(N * cs * taps, generator=torch.Generator().manual_seed(1))
    got = R.pack_weight(src, N, cs, Cl, taps, k["transposed"], k["geglu"], k["xp"], opd)
    Cin = 3 * Cl if k["xp"] else Cl
    assert got.shape == (taps, N, Cin) and got.dtype == opd
    perm = R.geglu_rows(N).tolist() if k["geglu"] else list(range(N))
    assert sorted(perm) == list(range(N))
    for t in range(0, taps, 4):
        for nd in range(0, N, 3 if N > 8 else 1):
            for cp in range(Cin):
                seg, ch = divmod(cp, Cl)
                w = torch.zeros(())
                if ch < cs:
                    w = src[(ch * N + perm[nd]) * taps + t] if k["transposed"] else src[(perm[nd] * cs + ch) * taps + t]
                hi = w.to(opd)
                want = hi if seg < 2 else (w - hi.float()).to(opd)
                assert got[t, nd, cp] == want, (t, nd, cp)


def test_geglu_rows_pairs_value_and_gate_blocks():
    p = R.geglu_rows(128).tolist()
    assert p[:32] == list(range(32)) and p[32:64] == list(range(64, 96)) and p[64:96] == list(range(32, 64)) and p[96:] == list(range(96, 128))


def test_pack_upconv_reference_is_the_conv_of_the_upsampled_image():
    """the 16 slabs, used as four 2 x 2 convs per output parity, reproduce conv3x3(nearest-x2(x)) (float64, no rounding)"""
    g = torch.Generator().manual_seed(2)
    w, x = torch.randn(3, 2, 3, 3, generator=g).double(), torch.randn(1, 2, 4, 5, generator=g).double()
    slabs = R.pack_upconv_weight(w, torch.float64)            # [16][N][Cin]
    up = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    want = nn.functional.conv2d(up, w, padding=1)
    xp = nn.functional.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            acc = torch.zeros(1, 3, 4, 5, dtype=torch.float64)
            for a in range(2):
                for b in range(2):
                    k = slabs[(py * 2 + px) * 4 + a * 2 + b]  # input offset (py + a - 1, px + b - 1)
                    win = xp[:, :, py + a:py + a + 4, px + b:px + b + 5]
                    acc += torch.einsum("nc,bchw->bnhw", k, win)
            close(acc, want[:, :, py::2, px::2])
    w32 = torch.randn(2, 3, 3, 3, generator=g)
    s32 = R.pack_upconv_weight(w32, torch.float16)
    assert s32.dtype == torch.float16 and s32[15, 1, 2] == w32[1, 2, 2, 2].half()     # py = px = a = b = 1: the corner tap alone
    assert s32[0, 1, 2] == w32[1, 2, 0, 0].half() and s32[3, 0, 0] == (((w32[0, 0, 1, 1] + w32[0, 0, 1, 2]) + w32[0, 0, 2, 1]) + w32[0, 0, 2, 2]).half()


def test_small_move_references():
    beta = torch.tensor([-1.0, 0.3, 2.00048828125])
    t = R.relu_beta_tile(beta, 2, 1, torch.float16)
    assert t.shape == (18,) and torch.equal(t[:6], t[12:]) and t[0] == 0 and t[6 + 2] == (beta[2] - beta[2].half().float()).half() != 0
    assert torch.equal(R.relu_beta_tile(beta, 2, 0, torch.float16), t[:6])
    x = torch.randn(2, 3, 1, 4)
    u = R.upsample2(x, torch.float16)
    assert u.shape == (2, 6, 2, 4) and all(torch.equal(u[:, y, xx], x[:, y // 2, xx // 2].half()) for y in range(6) for xx in range(2))
    feats, grid = torch.randn(3, 4), torch.tensor([2, -1, 0, -1, 1, 2])
    dn = R.sparse_densify(feats, grid)
    assert dn.shape == (4, 6) and all(torch.equal(dn[:, v], feats[g] if g >= 0 else torch.zeros(4)) for v, g in enumerate(grid.tolist()))


# ---- 6. folds -------------------------------------------------------------------------------------------------------------------------
def test_fold_references_against_index_loops():
    g = torch.Generator().manual_seed(3)
    heads, hd, Cc, I = 3, 5, 4, 6
    wq, wk, wv, wo = (torch.randn(*s, generator=g) for s in ((heads * hd, I), (heads * hd, Cc), (heads * hd, Cc), (I, heads * hd)))
    qk, qk_abs = R.fold_qk(wq, wk, heads, hd, Cc, 0.25)
    ov, ov_abs = R.fold_ov(wo, wv, heads, hd, Cc)
    for h in range(heads):
        for j in range(Cc):
            for i in range(I):
                want = 0.25 * sum(wk[h * hd + c, j].double() * wq[h * hd + c, i].double() for c in range(hd))
                assert abs(qk[h * Cc + j, i] - want) < 1e-13
                want = sum(wo[i, h * hd + c].double() * wv[h * hd + c, j].double() for c in range(hd))
                assert abs(ov[i, h * Cc + j] - want) < 1e-13
    assert bool((qk_abs >= qk.abs()).all()) and bool((ov_abs >= ov.abs()).all())
    a, b = torch.randn(4, 5, generator=g), torch.randn(5, 3, generator=g)
    close(R.fold_mm(a, b)[0], a.double() @ b.double())
    shapes = R.FOLD_SHAPES
    assert len(shapes) == 16 and {s[0] for s in shapes} == {1, 3} and {s[1] for s in shapes} == {8, 40} and 40 % 16
    assert any(M == 80 and N == 1 and ldb == 1 for M, N, K, lda, ldb, ldc in R.FOLD_MM) and any(ldc > N for _, N, _, _, _, ldc in R.FOLD_MM)


def test_ulp_and_fold_bounds():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 3e-6, 0.0], dtype=torch.float64)
    for dt, fmt in ((torch.float32, R.FMT32), (torch.float16, R.fmt16(torch.float16)), (torch.bfloat16, R.fmt16(torch.bfloat16))):
        near = x.to(dt)
        if dt == torch.bfloat16:
            want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -26, 2.0 ** -133], dtype=torch.float64)
        else:
            want = (torch.nextafter(near, torch.full_like(near, float("inf"))).double() - near.double())
        assert torch.equal(R.ulp(near.double(), *fmt), want), dt
    ref, ab = torch.tensor([1.0, -0.3]).double(), torch.tensor([4.0, 2.0]).double()
    b32, b16 = R.fold_bounds(ref, ab, 40, torch.float16)
    assert bool((b32 > 0.5 * R.ulp(ref, *R.FMT32)).all()) and bool((b32 < 0.5001 * R.ulp(ref, *R.FMT32)).all())
    assert bool((b16 > 0.5 * R.ulp(ref, 10, -14)).all()) and bool((b16 < 0.501 * R.ulp(ref, 10, -14)).all())


# ---- 7. CFG assembly and DDIM ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1, 2])
def test_cfg_assemble_reference(copies):
    g = torch.Generator().manual_seed(4)
    B, TN, HW, dim = 2, 3, 5, 6
    xn, xi, clip, ts = torch.randn(B, TN, 4, HW, generator=g), torch.randn(B, 4, HW, generator=g), torch.randn(B, dim, generator=g), torch.tensor([7, 481])
    xin, ctx, tt = R.cfg_assemble(xn, xi, clip, ts, copies)
    assert xin.shape == (copies * B * TN, HW, 8) and ctx.shape == (copies * B * TN, dim) and tt.tolist() == [7, 7, 7, 481, 481, 481] * copies
    k = torch.tensor(0.18215, dtype=torch.float32)
    for half in range(copies):
        for b in range(B):
            for v in range(TN):
                row = half * B * TN + b * TN + v
                assert torch.equal(xin[row, :, :4], xn[b, v].T)
                assert torch.equal(xin[row, :, 4:], (xi[b] / k).T if half == 0 else torch.zeros(HW, 4))
                assert torch.equal(ctx[row], clip[b] if half == 0 else torch.zeros(dim))


def test_cfg_ddim_reference():
    g = torch.Generator().manual_seed(5)
    ec, eu, x, z = (torch.randn(9, generator=g) for _ in range(4))
    k = R.DDIM_COEF
    f = {n: float(torch.tensor(v, dtype=torch.float32)) for n, v in k.items()}
    e, xp = R.cfg_ddim(ec, eu, x, z, k, torch.float64)
    we = eu.double() + f["scale"] * (ec.double() - eu.double())
    close(e, we)
    close(xp, f["sqrt_aprev"] * (x.double() - f["s1m"] * we) / f["sqrt_at"] + f["dir_coef"] * we + f["sigma"] * z.double())
    e, xp = R.cfg_ddim(ec, None, x, None, k, torch.float64)
    close(e, ec.double())
    close(xp, f["sqrt_aprev"] * (x.double() - f["s1m"] * ec.double()) / f["sqrt_at"] + f["dir_coef"] * ec.double())
    assert R.DDIM_N == (1, 1039, 4099)


# ---- 8. reductions --------------------------------------------------------------------------------------------------------------------
def test_fuse_views_and_mse_references():
    g = torch.Generator().manual_seed(6)
    vf, w, b = torch.randn(3, 4, 16, generator=g), torch.randn(16, 16, generator=g), torch.randn(16, generator=g)
    got = R.fuse_views(vf, w, b, 16, torch.float64)
    for v in range(4):
        for co in range(16):
            want = sum((w[co].double() * vf[view, v].double()).sum() for view in range(3)) / 16 + b[co].double()
            assert abs(got[v, co] - want) < 1e-13
    close(R.fuse_views(vf, w, None, 16, torch.float64), got - b.double())
    a, c = torch.randn(11, generator=g), torch.randn(11, generator=g)
    assert abs(R.mse(a, c) - sum((float(p) - float(q)) ** 2 for p, q in zip(a, c)) / 11) < 1e-14
    s, r = torch.randn(5), torch.randn(5)
    assert torch.equal(R.added(s, r, torch.float32), (s + r).double() - s.double())

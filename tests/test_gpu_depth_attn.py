"""GPU: the DepthTransformer's inference path per op.

(1) depth_attn_kernel (csrc/k_depth.hip) on its own through mvd_op_depth_attn, against the float64 restatement of
    tests/depth_attn_ref.py (tied to DepthAttention.forward by tests/test_depth_attn_cpu.py) on the fp16-rounded context and the
    fp32 folded query.  The block and step goldens only reach the kernel at Cc = 64 / 128 / 256 / 512 and one depth per level.
    The hook poisons what the launch must not touch: the context's pad columns (ldx > Cc) and one guard row behind z are NaN.
(2) The context-free samples of classifier-free guidance at block level (mvd_unet_block's n_ctx), in both production forms.
(3) A UNet with volume_dims = (24, 48, 96, 192): context widths whose (head, octet) pair count is no power of two.

Bounds.  Plain output (one fp16 rounding of an fp32 result): the per-op bounds of tests/test_gpu_ops.py, relative L2 <= 1e-3 and
normalised max <= 4e-3.  Split output (hi + lo of the [hi | lo | hi] rows): 4 x the worst value measured on an MI355X against the
float64 reference over PARITY + PEAKED below (the cases differ in D and peakedness; the kernel is deterministic).  Measured:
relative L2 8.8e-08 ... 3.48e-07 and normalised max 8.8e-08 ... 5.76e-07, both worst at Cc = 512, D = 24 (hi alone: 1.9e-04 ... 2.2e-04
and 2.0e-04 ... 3.6e-04); the one-hot cases return a context row and are exact in both forms.  Bounds: 1.39e-06 and 2.30e-06.
Independently of that figure every split case must put hi + lo at least 20 x closer to the reference than hi alone.
Blocks: the project's block bound, relative L2 <= 1e-3 against oracle.mvd_oracle.depth_transformer."""
import os
import subprocess
import sys

import pytest
import torch

from tests import depth_attn_ref as R
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu

REL_L2, MAX_N = 1e-3, 4e-3  # tests/test_gpu_ops.py
SPLIT_L2_MEASURED, SPLIT_MAX_MEASURED = 3.48e-07, 5.76e-07  # MI355X, worst over PARITY + PEAKED (see the module docstring)
SPLIT_REL_L2, SPLIT_MAX_N = 4 * SPLIT_L2_MEASURED, 4 * SPLIT_MAX_MEASURED
BLOCK_REL_L2 = 1e-3


@pytest.fixture(scope="module")
def small_net():
    return _net(gi.SMALL_UNET)


@pytest.fixture(scope="module")
def eng(small_net):
    return small_net[0]._engine  # the op hook needs a context only


def _net(cfg):
    from morphablediffusion_amd.model import DepthWiseAttention
    W = gi.unet_weights(cfg)
    net = DepthWiseAttention(volume_dims=cfg.volume_dims, image_size=32, in_channels=8, out_channels=4, model_channels=64,
                             attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8,
                             use_spatial_transformer=True, transformer_depth=1, context_dim=768, use_checkpoint=True, legacy=False)
    net.load_state_dict({k[len("model.diffusion_model."):]: v for k, v in W.items()})
    return net, W


def errs(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (((got - want).norm() / (want.norm() + 1e-300)).item(), ((got - want).abs().max() / (want.abs().max() + 1e-300)).item())


def inputs(Cc, D, n_cond, HW, seed=0, score_std=2.0):
    """Seeded qk / context: scores qk . ctx[d] of standard deviation ~ score_std, so the softmax is neither uniform nor one-hot.
    The context is returned as the kernel sees it (rounded to fp16)."""
    g = torch.Generator().manual_seed(1000 * Cc + 10 * D + HW + seed)
    ctx = torch.randn(n_cond, D, HW, Cc, generator=g).half().float()
    qk = torch.randn(n_cond * HW, 4, Cc, generator=g) * (score_std * Cc ** -0.5)
    return qk, ctx


def run_case(eng, name, qk, ctx, nfill=0, ldxm=1, split=False, seed=0):
    """One launch; checks the fill rows (bit for bit), the guard row (still NaN) and z against the float64 reference."""
    n_cond, D, HW, Cc = ctx.shape
    npix = n_cond * HW
    fill = torch.randn(4 * Cc, generator=torch.Generator().manual_seed(seed + Cc + nfill)) if nfill else None
    if split:
        out, hi = eng.op_depth_attn(qk, ctx, fill_row=fill, nfill=nfill, split=True, ldx=ldxm * Cc, return_hi=True)
        hi = hi.cpu()
    else:
        out, hi = eng.op_depth_attn(qk, ctx, fill_row=fill, nfill=nfill, ldx=ldxm * Cc), None
    out = out.cpu()
    assert out.shape == (npix + nfill + 1, 4 * Cc)
    assert torch.isnan(out[-1]).all(), f"{name}: the launch wrote behind its last row"
    z, want = out[:npix], R.depth_attn_ref(qk, ctx)
    assert torch.isfinite(z).all(), f"{name}: non-finite z (a read past Cc of a wide context row, or [hi | lo | hi] blocks that differ)"
    rl2, mxe = errs(z, want)
    line = f"[parity] depth_attn {name} Cc={Cc} D={D} npix={npix} nfill={nfill} ldx={ldxm * Cc} split={int(split)}: relL2={rl2:.2e} maxnorm={mxe:.2e}"
    if split:
        hl2, hmx = errs(hi[:npix], want)
        line += f" | hi alone: relL2={hl2:.2e} maxnorm={hmx:.2e} ({hl2 / max(rl2, 1e-300):.0f}x)"
    print(line)
    if nfill:
        f16 = fill.half().float()
        fill_want = f16 + (fill - f16).half().float() if split else f16
        assert torch.equal(out[npix:npix + nfill], fill_want.expand(nfill, -1)), f"{name}: fill rows differ from fill_row"
        if split:
            assert torch.equal(hi[npix:npix + nfill], f16.expand(nfill, -1)), f"{name}: fill rows' hi block"
    if split:
        assert rl2 <= SPLIT_REL_L2 and mxe <= SPLIT_MAX_N, f"{name}: split relL2={rl2:.3e} maxnorm={mxe:.3e}"
        assert 20 * rl2 <= hl2, f"{name}: hi + lo ({rl2:.3e}) is not 20x closer to the reference than hi alone ({hl2:.3e})"
        assert hl2 <= REL_L2 and hmx <= MAX_N, f"{name}: hi alone relL2={hl2:.3e} maxnorm={hmx:.3e}"
    else:
        assert rl2 <= REL_L2 and mxe <= MAX_N, f"{name}: relL2={rl2:.3e} maxnorm={mxe:.3e}"
    return rl2, mxe


# (Cc, D, n_cond, HW, nfill, ldx / Cc, split).  Every value of every axis occurs: Cc 8 ... 64 (P = 16 ... 2 depth parts in the z
# stage), 128 ... 512 (64 and more (head, octet) pairs), 24 / 48 / 96 (pair counts below 64 that are no power of two); D below, at,
# just past and several times the 16 softmax parts, up to the launcher's limit; a last workgroup with 0 ... 3 live or fill waves
# (rows = npix + nfill = 0, 1, 2, 3 mod 4, and npix itself 0 ... 3 mod 4: fill rows that start mid-workgroup); wide context rows.
PARITY = [
    (8, 1, 1, 5, 0, 1, 0), (16, 3, 1, 9, 1, 4, 1), (32, 6, 3, 16, 7, 1, 0), (64, 12, 1, 5, 7, 4, 1), (128, 16, 1, 9, 0, 1, 1),
    (256, 17, 1, 5, 1, 4, 0), (512, 24, 1, 9, 7, 1, 1), (24, 48, 1, 5, 0, 1, 0), (48, 64, 1, 9, 1, 4, 1), (96, 17, 3, 16, 7, 1, 0),
    (24, 3, 3, 16, 1, 4, 1), (48, 16, 1, 5, 7, 1, 0), (96, 64, 1, 9, 0, 4, 1), (64, 48, 3, 16, 0, 1, 0), (8, 64, 1, 9, 7, 4, 1),
    (16, 17, 1, 5, 1, 1, 0), (32, 24, 1, 9, 0, 4, 1), (128, 1, 3, 16, 1, 1, 0), (256, 48, 1, 5, 7, 4, 1), (512, 6, 1, 9, 1, 4, 0),
    (24, 12, 1, 9, 7, 1, 1), (64, 3, 1, 7, 1, 1, 0), (96, 12, 1, 6, 0, 4, 1), (128, 64, 1, 5, 1, 1, 1), (64, 16, 3, 16, 7, 4, 1),
]


def test_parity_cases_cover_every_axis_value():
    col = lambda i: {c[i] for c in PARITY}
    assert col(0) == {8, 16, 32, 64, 128, 256, 512, 24, 48, 96} and col(1) == {1, 3, 6, 12, 16, 17, 24, 48, 64}
    assert {(1, 5), (1, 9), (3, 16)} <= {(c[2], c[3]) for c in PARITY} and col(4) == {0, 1, 7} and col(5) == {1, 4} and col(6) == {0, 1}
    assert {(c[2] * c[3] + c[4]) % 4 for c in PARITY} == {0, 1, 2, 3} and {(c[2] * c[3]) % 4 for c in PARITY} == {0, 1, 2, 3}
    for cc in (24, 48, 96):
        assert {c[6] for c in PARITY if c[0] == cc} == {0, 1}


@pytest.mark.parametrize("Cc,D,n_cond,HW,nfill,ldxm,split", PARITY)
def test_depth_attn_parity(eng, Cc, D, n_cond, HW, nfill, ldxm, split):
    qk, ctx = inputs(Cc, D, n_cond, HW)
    run_case(eng, "parity", qk, ctx, nfill=nfill, ldxm=ldxm, split=bool(split))


PEAKED = [(64, 48, "first", 0), (64, 48, "last", 1), (24, 17, "first", 1), (24, 17, "last", 0), (96, 6, "last", 1), (64, 12, "equal", 1),
          (24, 64, "equal", 0)]


@pytest.mark.parametrize("Cc,D,where,split", PEAKED)
def test_depth_attn_peaked_and_uniform_softmax(eng, Cc, D, where, split):
    """One depth's score ~50 above all others, at d = 0 and at d = D - 1 (the first lane and the last softmax part that holds a
    depth); and all scores equal (qk = 0: z is the plain mean over depth)."""
    qk, ctx = inputs(Cc, D, 1, 9, score_std=0.25)  # the other channels move a score by ~ +-1
    if where == "equal":
        qk = torch.zeros_like(qk)
    else:
        d = 0 if where == "first" else D - 1
        ctx[..., 0] = 0.0  # channel 0 marks depth d alone; it adds exactly 50 to that depth's score of every head
        ctx[:, d, :, 0] = 1.0
        qk[..., 0] = 50.0
        sim = torch.einsum("phc,pdc->phd", qk.double(), ctx.double().permute(0, 2, 1, 3).reshape(9, D, Cc))
        gap = (sim[..., d:d + 1] - sim).masked_fill(torch.arange(D) == d, float("inf")).min().item()
        print(f"[parity] depth_attn peaked {where}: smallest score gap {gap:.1f}")
        assert 45 < gap < 55
    run_case(eng, f"peaked-{where}", qk, ctx, nfill=1, split=bool(split))


@pytest.mark.parametrize("Cc,D,split", [(24, 17, 0), (64, 48, 1), (512, 6, 0)])
def test_depth_attn_zero_context_gives_exact_zero(eng, Cc, D, split):
    qk, ctx = inputs(Cc, D, 1, 9)
    out = eng.op_depth_attn(qk, torch.zeros_like(ctx), split=bool(split)).cpu()
    assert torch.isnan(out[-1]).all()
    assert torch.equal(out[:-1], torch.zeros(9, 4 * Cc))


@pytest.mark.parametrize("Cc", [24, 64])
@pytest.mark.parametrize("split", [0, 1])
def test_depth_attn_which_lane_wrote_what(eng, Cc, split):
    """Asymmetric selection: ctx[p][d][c] is an integer code (a permutation of 1 ... D*Cc per pixel, exact in fp16), and qk makes
    head h of pixel p pick depth d*(p, h) with a score gap of 60 or more, so z[p][h][c] == ctx[p][d*(p, h)][c] exactly
    (exp(-60) vanishes in fp32).  A head, octet or pixel written by the wrong lane is an O(1) error."""
    D, HW = 8, 7
    g = torch.Generator().manual_seed(Cc)
    ctx = torch.stack([torch.randperm(D * Cc, generator=g).reshape(D, Cc) + 1 for _ in range(HW)], 1)[None].float()  # [1,D,HW,Cc]
    assert torch.equal(ctx.half().float(), ctx)
    c = ctx[0].permute(1, 0, 2).double()  # [HW,D,Cc]
    dstar = (torch.arange(HW)[:, None] + 3 * torch.arange(4)[None]) % D  # [HW,4]
    target = 70.0 * torch.nn.functional.one_hot(dstar, D).double()  # sim[p,h,:]
    qk = torch.einsum("pcd,phd->phc", torch.linalg.pinv(c), target).float()  # c[p] @ qk[p,h] = target[p,h]
    sim = torch.einsum("phc,pdc->phd", qk.double(), c)
    top = sim.gather(-1, dstar[..., None])
    gap = (top - sim).masked_fill(torch.nn.functional.one_hot(dstar, D).bool(), float("inf")).min().item()
    assert gap >= 60, gap
    want = c[torch.arange(HW)[:, None], dstar].reshape(HW, 4 * Cc).float()
    out = eng.op_depth_attn(qk, ctx, split=bool(split)).cpu()
    wrong = (out[:-1] != want).sum().item()
    print(f"[parity] depth_attn lane map Cc={Cc} split={split}: gap={gap:.1f} wrong={wrong}/{want.numel()} "
          f"max|err|={(out[:-1] - want).abs().nan_to_num(float('inf')).max().item():.3g}")
    assert torch.isnan(out[-1]).all()
    assert torch.equal(out[:-1], want)


REFUSED = [dict(Cc=64, D=6, heads=8), dict(Cc=12, D=6), dict(Cc=64, D=65), dict(Cc=512, D=64), dict(Cc=64, D=6, ldx=56)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_depth_attn_refusals(eng, kw):
    """The launcher's own refusals (heads != 4, Cc % 8, D > 64, the LDS budget -- 4 waves x 75 776 bytes > 160 KB --, ldx < Cc):
    reported without a launch, by the check alone and by the call itself, and the next good call is unaffected."""
    from morphablediffusion_amd.lib import MvdError
    err = eng.op_depth_attn_check(**kw)
    print(f"[refused] {kw}: {err}")
    assert err is not None and err.startswith("depth_attn:")
    assert ("LDS budget" in err) == (kw["Cc"] == 512), err
    with pytest.raises(MvdError, match="depth_attn:"):
        eng.op_depth_attn(torch.zeros(5, 4, kw["Cc"]), torch.zeros(1, kw["D"], 5, kw["Cc"]), ldx=kw.get("ldx", 0), heads=kw.get("heads", 4))
    assert eng.op_depth_attn_check(Cc=512, D=24) is None and eng.op_depth_attn_check(Cc=64, D=64, ldx=256) is None
    qk, ctx = inputs(64, 6, 1, 5)
    run_case(eng, "after-refusal", qk, ctx, nfill=1)


# ---- blocks: context-free samples, narrow context widths ----------------------------------------------------------------

BLOCKS = [("output_conditions.8", 32, 6), ("output_conditions.3", 16, 3), ("middle_conditions", 4, 2)]  # path, resolution, depth
_block_cache = {}


def block_case(W, path, res, D, tag, B=4, n_free=2):
    """x [B, C, res, res], volumes [B, Cc, D, res, res] whose last n_free samples are zero (context-free), and the oracle's output:
    computed once per block.  Samples are independent (every GroupNorm is per sample), so any selection of rows is a batch."""
    if (tag, path) not in _block_cache:
        from oracle import mvd_oracle as O
        p = "model.diffusion_model." + path
        C, Cc = W[p + ".proj_in.0.weight"].shape[1], W[p + ".proj_context.0.weight"].shape[1]
        g = torch.Generator().manual_seed(res + D)
        x = torch.randn(B, C, res, res, generator=g)
        vol = torch.randn(B, Cc, D, res, res, generator=g)
        vol[B - n_free:] = 0
        _block_cache[(tag, path)] = (x, vol, O.depth_transformer(W, p, x, vol))
    return _block_cache[(tag, path)]


def block_close(got, want, x, name):
    got = got.float().cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite"
    rl2 = ((got - want).norm() / want.norm()).item()
    branch = ((got - x) - (want - x)).norm().item() / (want - x).norm().item()
    print(f"[parity] {name}: relL2={rl2:.2e} (residual branch alone: {branch:.2e}, |y-x|/|x|={(want - x).norm().item() / x.norm().item():.3f})")
    assert rl2 <= BLOCK_REL_L2, f"{name}: relL2={rl2:.3e}"


@pytest.mark.parametrize("path,res,D", BLOCKS)
@pytest.mark.parametrize("rows,n_ctx", [((0, 1, 2), 2), ((0, 2), 1), ((2, 3), 0)], ids=["B3-ctx2", "B2-ctx1", "B2-ctx0"])
def test_blocks_context_free_samples(small_net, path, res, D, rows, n_ctx):
    """DepthTransformer blocks on B samples of which only the first n_ctx have a context volume, against the oracle with zero
    volumes for the others.  Default: those samples get x + K (mvd_ctx::CondConst); under MVD_NO_COND_CONST=1 (the subprocess
    below) their z rows are the relu(beta) fill rows of the depth-attention launch; n_ctx = 0 is launch_fill_rows_f16 alone."""
    net, W = small_net
    e = net._engine
    x, vol, want = block_case(W, path, res, D, "small")
    rows = list(rows)
    xs = x[rows].contiguous()
    got = e.unet_block(path, xs, volume=vol[rows[:n_ctx]].contiguous() if n_ctx else None, n_ctx=n_ctx)
    form = "fill rows" if os.environ.get("MVD_NO_COND_CONST") == "1" else "x + K"
    block_close(got, want[rows], xs, f"{path} B={len(rows)} n_ctx={n_ctx} ({form})")
    if 0 < n_ctx and form == "x + K":  # K must not depend on the samples that have context: other x, other volumes, same K
        x2 = xs.clone()
        x2[:n_ctx] = x[3:4] * 0.5 + 1.0
        got2 = e.unet_block(path, x2, volume=(vol[rows[:n_ctx]] * -0.7).contiguous(), n_ctx=n_ctx)
        assert torch.equal(got2[n_ctx:], got[n_ctx:]), f"{path}: the context-free samples' output moved with the other samples"
        assert not torch.equal(got2[:n_ctx], got[:n_ctx])


def test_blocks_context_free_samples_fill_row_form():
    """The same nine cases with MVD_NO_COND_CONST=1 (read once per process, hence the subprocess): every layer over all samples,
    the context-free rows' z written by the surplus waves of depth_attn_kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-k",
                        "test_blocks_context_free_samples and not fill_row_form"], cwd=root,
                       env=dict(os.environ, MVD_NO_COND_CONST="1"), capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if "[parity]" in l]
    print("\n".join(lines))
    assert r.returncode == 0 and "9 passed" in r.stdout, r.stdout[-3000:]
    assert len(lines) == 9 and all("(fill rows)" in l for l in lines)


@pytest.fixture(scope="module")
def narrow_net():
    from morphablediffusion_amd.spec import UNetConfig
    return _net(UNetConfig(model_channels=64, volume_dims=(24, 48, 96, 192)))


@pytest.mark.parametrize("path,res,D", BLOCKS)
def test_blocks_narrow_context_widths(narrow_net, path, res, D):
    """volume_dims = (24, 48, 96, 192), every sample with context: depth attention at 12 / 24 / 96 (head, octet) pairs, the context
    GroupNorm at 3 / 6 / 24 channels per group, the folded GEMMs at K = 24 / 48 / 192 (x 3 x 64 x 32 x 32 with volume
    3 x 24 x 6 x 32 x 32, 3 x 128 x 16 x 16 with 3 x 48 x 3 x 16 x 16, 3 x 256 x 4 x 4 with 3 x 192 x 2 x 4 x 4).  The residual branch is ~0.4 of the output
    norm (printed), so a wrong z cannot hide behind x."""
    net, W = narrow_net
    x, vol, want = block_case(W, path, res, D, "narrow", B=3, n_free=0)
    assert vol.shape[1] in (24, 48, 192) and (want - x).norm() / x.norm() > 0.25
    block_close(net._engine.unet_block(path, x, volume=vol), want, x, f"{path} narrow Cc={vol.shape[1]}")

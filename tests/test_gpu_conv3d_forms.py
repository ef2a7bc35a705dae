"""GPU: run_conv3d / run_convT3d (csrc/engine_unet.hip) in the forms FrustumTV3DNet and SpatialTime3DNet launch them in, one layer at
a time through mvd_op_conv3d_ex, against the fp64 reference of tests/epilogue_ref.py (conv3d): the fp16-source gather kernel with 27
taps (more than 16384 rows), the LDS-DMA tap gather with K tails and column tails, the parity-batched ConvTranspose3d with several
column tiles, its 16-bit result through the parity scatter, the eight-launch form and its split-K, odd / unit / unequal extents,
and rows on both sides of the thresholds 64, 512 and 16384.  tests/test_conv3d_forms_cpu.py checks the table without a GPU.

Every case asserts the kernel family, the number of launches and the number of splitk_reduce_kernel launches it is built to reach
(probe_config(1) / probe_report()), runs with the free workspace poisoned, and has its guard row and pad columns checked by the
wrapper.  The exact cases hold to 1e-6 (their arithmetic is exact: any index, tap, parity or row-mapping error is O(1)); a 16-bit
result is compared bit for bit with the reference, which those cases are built to hold without rounding.

The family each case ran on and its relL2 against fp64 (the [parity] lines of this file on an MI355X, fp16 library; an unbatched
transposed case is eight launches on the one family, the parity walk repeats the seven batched cases with 0.00e+00 / 2.91e-04):

  test      case                                                            family                  relL2
  exact     s1 gather_f16 17x32x32 72->40 above 16384 rows                  igemm_kernel<0,64>      0.00e+00
  exact     s1 dense 16x32x32 16->8 exactly 16384 rows                      gemm_dma_kernel<64,0>   0.00e+00
  exact     s1 gather_f16 3x4x4 64->40 48 rows                              igemm_kernel<0,64>      0.00e+00
  exact     s1 dense 4x4x4 64->40 exactly 64 rows                           gemm_dma_kernel<64,0>   0.00e+00
  exact     s1 dense B=3 5x7x9 16->40                                       gemm_dma_kernel<64,0>   0.00e+00
  exact     s1 dense B=3 5x7x9 48->200 ldc                                  gemm_dma_kernel<128,0>  0.00e+00
  exact     s1 dense B=3 5x7x9 72->320                                      gemm_dma_kernel<160,0>  0.00e+00
  exact     s1 dense B=5 1x3x5 64->40 extent 1                              gemm_dma_kernel<64,0>   0.00e+00
  exact     s1 dense B=3 5x7x9 128->40 split-K                              gemm_dma_kernel<64,0>   0.00e+00
  exact     s1 dense B=3 5x7x9 48->40 in place f16 out                      gemm_dma_kernel<64,0>   0.00e+00
  exact     s1 gather_f32 B=3 5x7x9 24->40                                  igemm_kernel<1,64>      0.00e+00
  exact     s1 gather_f32 B=3 5x7x9 128->200 split-K ldc                    igemm_kernel<1,128>     0.00e+00
  exact     s2 gather_f16 51x53x51 16->8 above 16384 rows                   igemm_kernel<0,64>      0.00e+00
  exact     s2 dense B=3 5x7x9 16->40                                       gemm_dma_kernel<64,0>   0.00e+00
  exact     s2 dense B=3 5x7x9 48->200                                      gemm_dma_kernel<128,0>  0.00e+00
  exact     s2 dense B=3 5x7x9 72->320 ldc                                  gemm_dma_kernel<160,0>  0.00e+00
  exact     s2 dense B=11 1x3x5 64->40 extent 1                             gemm_dma_kernel<64,0>   0.00e+00
  exact     s2 gather_f16 B=2 1x3x5 64->40 extent 1                         igemm_kernel<0,64>      0.00e+00
  exact     s2 gather_f16 B=2 2x2x2 72->40 one voxel                        igemm_kernel<0,64>      0.00e+00
  exact     s2 gather_f32 B=3 5x7x9 24->40                                  igemm_kernel<1,64>      0.00e+00
  exact     s2 gather_f32 B=2 2x2x2 24->40 one voxel                        igemm_kernel<1,64>      0.00e+00
  exact     T batched B=2 4x8x8 64->200 exactly 512 rows                    gemm_dma_kernel<128,0>  0.00e+00
  exact     T batched B=2 4x8x8 64->320                                     gemm_dma_kernel<160,0>  0.00e+00
  exact     T batched B=2 6x16x24 64->200 column walk                       gemm_dma_kernel<128,0>  0.00e+00
  exact     T batched B=1 5x7x15 48->40 in place                            gemm_dma_kernel<64,0>   0.00e+00
  exact     T batched B=2 4x8x8 64->40 in place f16 out ldc (level-0 form)  gemm_dma_kernel<64,0>   0.00e+00
  exact     T batched B=2 4x8x8 72->200 f16 out                             gemm_dma_kernel<128,0>  0.00e+00
  exact     T unbatched 6x7x12 64->40 504 rows                              gemm_dma_kernel<64,0>   0.00e+00
  exact     T unbatched 6x7x12 64->40 fp32 source                           igemm_kernel<1,64>      0.00e+00
  exact     T unbatched B=2 4x8x8 128->40 split-K                           gemm_dma_kernel<64,0>   0.00e+00
  exact     T unbatched B=2 4x8x8 64->200 split-K fp32 source               igemm_kernel<1,128>     0.00e+00
  exact     T unbatched B=2 2x3x4 72->40 48 rows                            igemm_kernel<0,64>      0.00e+00
  exact     T unbatched 6x7x12 48->40 fp32 source in place f16 out ldc      igemm_kernel<1,64>      0.00e+00
  footprint s1 / s2 / T (dense)                                             gemm_dma_kernel<64,0>   0.00e+00
  footprint s1 / s2 / T (gather_f32)                                        igemm_kernel<1,64>      0.00e+00
  random    s2 64->128 12x8x8                                               gemm_dma_kernel<128,0>  1.51e-04
  random    s1 128->128 6x4x4                                               gemm_dma_kernel<128,0>  1.38e-04
  random    T batched 128->64 6x4x4 in place f16 out                        gemm_dma_kernel<64,0>   2.91e-04
  random    s1 72->40 17x32x32 above 16384 rows                             igemm_kernel<0,64>      1.70e-04

The library's conversion to the 16-bit type is not put to the test by the exact cases (their results need no rounding); the random
16-bit case holds the bound of the 2-D "f16 out" form.  The exact, footprint and bad-argument tests were also run once on the
bfloat16 build (MVD_DTYPE=bf16): the same families, 0.00e+00 throughout.
"""
import os
import subprocess
import sys

import pytest
import torch

from morphablediffusion_amd import lib as L
from tests import epilogue_ref as R
from tests import golden_inputs as gi
from tests.test_gpu_epilogue_forms import EXACT, close
from tests.test_gpu_ops import MAX_N, REL_L2
from tests.test_gpu_train_ops import asym_weight

pytestmark = pytest.mark.gpu
OPD = torch.bfloat16 if L.DTYPE == "bf16" else torch.float16


@pytest.fixture(scope="module")
def eng():
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig
    e = Engine(UNetConfig(model_channels=64), VolumeConfig(), workspace_gb=2.0)
    yield e
    e.close()


def probed(eng, fn):
    """fn() with every launch booked by family: (result, {GEMM / conv family: launches}, splitk_reduce_kernel launches)"""
    eng.probe_config(1)
    try:
        res = fn()
        rep = eng.probe_report()
    finally:
        eng.probe_config(0)
    fams = {d["family"]: d["launches"] for d in rep if d["launches"] > 0 and not d["family"].startswith("(")}
    return res, fams, fams.pop("splitk_reduce_kernel", 0)


def ran_on(fams, family, launches=None):
    """every launch ran on `family` (the classes of an unbatched transposed conv may differ in their column-tile width)"""
    assert fams and all(R.family_matches(f, family) for f in fams), f"meant for {family} ({R.FAMILY[family]}), ran on {fams}"
    if launches is not None:
        assert sum(fams.values()) == launches, f"{launches} launches expected: {fams}"
    return " + ".join(sorted(fams))


def _run(eng, case, x, w, bias, resid, force_splitk):
    ldc, ldr = R.conv3d_ld(case)
    return probed(eng, lambda: eng.op_conv3d_ex(x, w, bias, stride=2 if case.kind == "s2" else 1, transposed=case.kind == "T", resid=resid,
                                                ldr=ldr, in_place=case.in_place, out_f16=case.out_f16, ldc=ldc, a_half=case.a_half,
                                                force_splitk=force_splitk, poison=True))


# ------------------------------------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("name", [c.name for c in R.CONV3D_CASES])
def test_conv3d_exact(eng, name):
    """0 / 1 / 2 activations and k / 64 weights, bias and residual: every product and partial sum is exact, so the result is the
    reference whatever the order of the sum -- and O(1) away from it for a wrong tap, parity class, sample, slice or column"""
    case = R.CONV3D_BY_NAME[name]
    x, w, bias, resid = R.conv3d_operands(case)
    out, fams, reduces = _run(eng, case, x, w, bias, resid, case.force_splitk or 1)  # 1: the kernel's own epilogue
    fam = ran_on(fams, case.family, case.launches)
    assert reduces == case.reduces, f"{case.reduces} splitk_reduce_kernel launches expected, {reduces} ran"
    want = R.conv3d_reference(name)
    close(out.out, want, f"conv3d exact {name}", fam, rel=EXACT, mx=EXACT)
    if case.out_f16:
        # the fp32 accumulator is exact and the reference is representable (tests/test_conv3d_forms_cpu.py): one rounding to the
        # library's 16-bit type must give the reference's own bits
        assert out.raw.dtype == OPD
        rows = want.permute(0, 2, 3, 4, 1).reshape(-1, case.Cout).to(OPD)
        assert torch.equal(out.raw.cpu().view(torch.int16), rows.view(torch.int16)), f"{name}: the 16-bit result is not the rounded reference"


# ----------------------------------------------------------------------------------------------------- forward impulse footprint
@pytest.mark.parametrize("family", ["dense", "gather_f32"])
@pytest.mark.parametrize("kind", ["s1", "s2", "T"])
def test_conv3d_impulse_footprint(eng, kind, family):
    """One-hot voxels at the far corner of the last sample and on an edge of the first, asymmetric weights without a zero: the
    support of the output is the footprint of the kernel, clipped by the volume and never reaching into a neighbouring sample"""
    B, Cin, Cout, dims = 3, 16, 40, (5, 7, 9)
    D, H, W = dims
    a_half = family == "dense"
    assert R.conv3d_family_ok(family, kind, B, Cin, Cout, dims, a_half, 1)
    x = torch.zeros(B, Cin, D, H, W)
    x[B - 1, Cin - 1, D - 1, H - 1, W - 1] = 1.0
    x[0, 5, 0, 3, W - 1] = 2.0
    w = asym_weight((Cin, Cout, 3, 3, 3) if kind == "T" else (Cout, Cin, 3, 3, 3))
    assert (w != 0).all() and torch.equal(w.half().float(), w) and torch.equal(w.bfloat16().float(), w)
    out, fams, reduces = probed(eng, lambda: eng.op_conv3d_ex(x, w, stride=2 if kind == "s2" else 1, transposed=kind == "T", a_half=a_half,
                                                              force_splitk=1))
    fam = ran_on(fams, family, 8 if kind == "T" and not a_half else 1)
    assert reduces == 0
    want = R.conv3d(x, w, stride=2 if kind == "s2" else 1, transposed=kind == "T")
    got = out.out.cpu()
    assert 0 < (want != 0).sum() < want.numel() // 4 and (want[1] == 0).all()
    assert torch.equal(got != 0, want != 0), f"conv3d footprint {kind} on {fam}: the support differs at {(got != 0).ne(want != 0).nonzero()[:8].tolist()}"
    close(got, want, f"conv3d footprint {kind}", fam, rel=EXACT, mx=EXACT)


# ---------------------------------------------------------------------------------------------------------- random operands
# (name, kind, B, Cin, Cout, dims, in place, 16-bit result, family): the frustum network's chain reduced to (12, 8, 8) with six views,
# and the level-0 gather form; the planner's own split (force_splitk = 0), as in production
RANDOM_CASES = [
    ("s2 64->128 12x8x8", "s2", 6, 64, 128, (12, 8, 8), False, False, "dense"),
    ("s1 128->128 6x4x4", "s1", 6, 128, 128, (6, 4, 4), False, False, "dense"),
    ("T batched 128->64 6x4x4 in place f16 out", "T", 6, 128, 64, (6, 4, 4), True, True, "dense"),
    ("s1 72->40 17x32x32 above 16384 rows", "s1", 1, 72, 40, (17, 32, 32), False, False, "gather_f16"),
]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=[c[0] for c in RANDOM_CASES])
def test_conv3d_random(eng, case):
    name, kind, B, Cin, Cout, dims, in_place, out_f16, family = case
    T = kind == "T"
    assert R.conv3d_family_ok(family, kind, B, Cin, Cout, dims, True)
    x = R.rnd(B, Cin, *dims, seed=1)
    w = R.rnd(*((Cin, Cout) if T else (Cout, Cin)), 3, 3, 3, seed=2, scale=(Cin * (27 / 8 if T else 27)) ** -0.5)
    bias, resid = R.rnd(Cout, seed=3), R.rnd(B, Cout, *R.conv3d_out_dims(kind, dims), seed=5)
    out, fams, _ = probed(eng, lambda: eng.op_conv3d_ex(x, w, bias, stride=2 if kind == "s2" else 1, transposed=T, resid=resid,
                                                        in_place=in_place, out_f16=out_f16, a_half=True))
    fam = ran_on(fams, family, 1)
    close(out.out, R.conv3d(x, w, stride=2 if kind == "s2" else 1, transposed=T, bias=bias, resid=resid), f"conv3d random {name}", fam,
          rel=REL_L2, mx=MAX_N)


# --------------------------------------------------------------------------------------------------------------- parity walk
def test_batched_transposed_cases_through_the_parity_walk():
    """k_gemm.hip PWALK: one workgroup walks the parity classes of its tile.  Forced for every parity-batched launch
    (MVD_PAR_WALK_MIN=1, read once per process, hence the child process): the batched transposed cases of this file -- several column
    tiles, a column tail, a K tail, the 16-bit result in place -- must hold on the walk too."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-k",
                        "(test_conv3d_exact or test_conv3d_random) and batched and not unbatched"], cwd=root,
                       env=dict(os.environ, MVD_PAR_WALK_MIN="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-3000:]
    lines = [l for l in r.stdout.splitlines() if "[parity] conv3d" in l and "relL2=" in l]  # (a line may start with the dot of the test before it)
    expected = sum(1 for c in R.CONV3D_CASES if R.conv3d_cell(c)[0] == "T batched") + sum(1 for c in RANDOM_CASES if "T batched" in c[0])
    assert len(lines) == expected and all("T batched" in l and "gemm_dma_kernel<" in l for l in lines), lines
    worst = max(float(l.split("relL2=")[1].split()[0]) for l in lines if " exact " in l)
    print(f"[parity] {len(lines)} parity-batched transposed convs through the parity walk: worst exact relL2={worst:.2e}")


# ------------------------------------------------------------------------------------------------------------- bad arguments
def test_conv3d_ex_refuses_bad_arguments_before_it_launches(eng):
    x, w, res = torch.zeros(1, 16, 2, 3, 4), torch.zeros(8, 16, 3, 3, 3), torch.zeros(1, 8, 2, 3, 4)
    bad = [
        ("Cin % 8", lambda: eng.op_conv3d_ex(torch.zeros(1, 12, 2, 3, 4), torch.zeros(8, 12, 3, 3, 3))),
        ("multiple of 4", lambda: eng.op_conv3d_ex(x, torch.zeros(6, 16, 3, 3, 3))),
        ("stride 1 or 2", lambda: eng.op_conv3d_ex(x, w, stride=3)),
        ("stride 1 or 2", lambda: eng.op_conv3d_ex(x, torch.zeros(16, 8, 3, 3, 3), stride=2, transposed=True)),
        ("ldc must", lambda: eng.op_conv3d_ex(x, w, ldc=10)),
        ("ldc must", lambda: eng.op_conv3d_ex(x, w, ldc=4)),
        ("ldr must", lambda: eng.op_conv3d_ex(x, w, resid=res, ldr=10)),
        ("in_place needs", lambda: eng.op_conv3d_ex(x, w, in_place=True)),
        ("force_splitk", lambda: eng.op_conv3d_ex(x, w, force_splitk=-1)),
    ]
    eng.probe_config(1)
    try:
        for text, call in bad:
            with pytest.raises(L.MvdError, match=text):
                call()
        torch.cuda.synchronize()
        rep = eng.probe_report()
    finally:
        eng.probe_config(0)
    assert not [d for d in rep if d["launches"] > 0], rep
    out = torch.zeros(64, 8).cuda()
    rc = eng.lib.mvd_op_conv3d_ex(None, L.ptr(x.cuda()), 1, 2, 3, 4, 16, L.ptr(w.cuda()), None, 8, 1, 0, 0, None, 0, 0, 0, 8, 1, 0, 0, L.ptr(out), None)
    assert rc != 0 and eng.lib.mvd_last_error() == b"null context" and (out == 0).all()
    # ... and the context takes the same shapes when the arguments are good
    assert eng.op_conv3d_ex(x, w, resid=res).out.abs().max() == 0


# ----------------------------------------------------------------------------------------------------------- geometry contract
def _cond_engine(**kw):
    from morphablediffusion_amd import synthetic
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.spec import VolumeConfig
    N = 2
    ucfg, vcfg = gi.SMALL_UNET, VolumeConfig(num_views=N, **kw)
    e = Engine(ucfg, vcfg, workspace_gb=2.0)
    e.load_state_dict(gi.full_weights(ucfg, vcfg))
    b = synthetic.make_batch(N, "perspective", 400, mesh_seed=2)
    e.set_mesh(b["vertices"][0], b["coord"][0], b["out_sh"][0], b["bounds"][0])
    e.set_cameras(b["target_K"][0], b["target_RT"][0])
    V = vcfg.spatial_volume_size
    e.set_volume(torch.zeros(64, V, V, V))
    return e, vcfg


def _frustum_refused(e, vcfg, field):
    te, ve, idx = torch.zeros(vcfg.time_dim).cuda(), torch.zeros(2, vcfg.view_dim).cuda(), torch.arange(2)
    e.probe_config(1)
    try:
        with pytest.raises(L.MvdError, match=field):
            e.frustum_volumes(te, ve, idx)
        torch.cuda.synchronize()
        rep = e.probe_report()
    finally:
        e.probe_config(0)
    assert not [d for d in rep if d["launches"] > 0], f"a refused geometry launched {rep}"


@pytest.mark.parametrize("field,kw", [("frustum_volume_depth", dict(frustum_volume_depth=20)), ("input_image_size", dict(input_image_size=72))])
def test_frustum_network_refuses_levels_that_do_not_halve(field, kw):
    """depth 20 -> 20, 10, 5, 3 (side 72 / 8 = 9 -> 9, 5, 3, 2): the up path would write 2 * 3 slices into the 5 of the level
    above, past its buffer and into the next allocation.  The reference raises a shape error at conv4 + conv7(x); here the call
    that runs the network names the field and launches nothing."""
    e, vcfg = _cond_engine(**kw)
    try:
        _frustum_refused(e, vcfg, field)
        _frustum_refused(e, vcfg, field)  # ... and leaves the context as it was
    finally:
        e.close()


def test_the_gathers_take_a_geometry_the_network_refuses():
    """input_image_size = 8 (a 1 x 1 frustum map: no level of it halves) stays a legal context for the gather hooks, which never
    run the network"""
    e, vcfg = _cond_engine(input_image_size=8)
    try:
        V = vcfg.spatial_volume_size
        vol = R.rnd(V, V, V, 64, seed=3)
        got = e.op_frustum_gather(vol.cuda(), [0, 1], 5, 6)
        assert tuple(got.shape) == (2, 5, 6, 6, 64) and torch.isfinite(got).all()
        _frustum_refused(e, vcfg, "input_image_size")
        assert torch.equal(e.op_frustum_gather(vol.cuda(), [0, 1], 5, 6), got)
    finally:
        e.close()

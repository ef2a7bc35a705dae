"""GPU: the deterministic training mode (mvd_train_set_deterministic) -- the conditioner's three gather adjoints as gathers.

1. Each adjoint on its own through the mvd_op_*_adjoint hooks, both forms, on conditioner-only stage engines, against the float64
   restatements of tests/test_train_deterministic_cpu.py: (a) the gather form repeats bit for bit, (b) it agrees with the atomic
   form to 1e-5 relative L2 (what tests/test_gpu_train.py allows between two runs of the atomic form), (c) it is as accurate:
   err_det <= 1.5 err_atomic + 1e-7, the atomic form -- the parent's behaviour -- being the yardstick, (d) every output element
   is written (the buffers start as NaN) and elements without a contribution are exactly zero.  Each case prints a "[det]" line
   with both errors before it asserts.
2. The conditioner's backward as a whole, 3. the whole training step and two optimiser steps of two models: torch.equal over the
   WHOLE gradient / parameter arena.  4. The default is untouched: which forms ran, from the engine's launch counters.

The "scaled-1.3" mesh of the vertex cases stays inside the +-0.5 cube (its radii are at most 0.364): the case whose vertices do
leave it, with the share asserted, is "leaving" (the same mesh scaled by 2)."""
import pytest
import torch

from morphablediffusion_amd import synthetic
from morphablediffusion_amd.spec import UNetConfig, VolumeConfig
from tests import golden_inputs as gi
from tests import test_train_deterministic_cpu as R
from tests.test_gpu_spatial_volume import SMALL_DIMS, stage_weights

pytestmark = pytest.mark.gpu
N = 4
S_MAP = 16  # the 2-D encoder maps of the stage engines (the vertex adjoint's output)
PARITY = 1e-5
_engines = {}


def engine_for(V, projection, D=5, S=6):
    """Conditioner-only engine for a V^3 lattice and a D x S x S frustum; cached (loading the weights dominates a case)."""
    key = (V, projection, D, S)
    if key not in _engines:
        vcfg = VolumeConfig(num_views=N, projection=projection, input_image_size=8 * S, frustum_volume_depth=D,
                            spatial_volume_size=V, frustum_dims=SMALL_DIMS)
        from morphablediffusion_amd.engine import Engine
        W = stage_weights(vcfg, "init")
        eng = Engine(UNetConfig(model_channels=64, image_size=S_MAP), vcfg, workspace_gb=1.0)
        eng.load_state_dict(W, expected={k: tuple(v.shape) for k, v in W.items()})
        _engines[key] = eng
    return _engines[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _engines.values():
        eng.close()
    _engines.clear()


def set_sample(eng, kind, K, RT):
    verts, coord, out_sh, bounds = R.mesh(kind)
    eng.select_sample(0)
    eng.set_mesh(verts, coord, out_sh, bounds)
    eng.set_cameras(K, RT)
    return verts, coord, out_sh, bounds


def check_forms(tag, run, want):
    """(a)-(d) for one case: run(deterministic) -> device tensor (a NaN-filled buffer the hook wrote), want float64."""
    det = [run(True) for _ in range(5)]
    torch.cuda.synchronize()
    atomic = run(False)
    for other in det[1:]:
        assert torch.equal(other, det[0]), f"{tag}: the gather form does not repeat bit for bit"
    got, ref = det[0].cpu(), atomic.cpu()
    assert torch.isfinite(got).all(), f"{tag}: the gather form left elements unwritten"
    assert torch.isfinite(ref).all()
    e_det, e_atomic, parity = R.rel_l2(got, want), R.rel_l2(ref, want), R.rel_l2(got, ref)
    print(f"[det] {tag}: err_det={e_det:.3e} err_atomic={e_atomic:.3e} parity={parity:.3e} "
          f"zero share={(want == 0).double().mean().item():.3f}")
    assert (got[want == 0] == 0).all(), f"{tag}: an element without a contribution is not exactly zero"
    assert parity <= PARITY
    assert e_det <= 1.5 * e_atomic + 1e-7


# ---- 1. each adjoint on its own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near", [False, True], ids=["stage-rig", "near-rig"])
@pytest.mark.parametrize("projection", ["perspective", "orthographic"])
@pytest.mark.parametrize("TN", [1, 2])
@pytest.mark.parametrize("V,D,S", [(8, 5, 6), (16, 6, 8)])
def test_frustum_adjoint(V, D, S, TN, projection, near):
    K, RT = R.rig(N, projection, 8 * S, near)
    views = [2, 1][:TN]
    d_out = torch.randn(TN, D, S, S, 64, generator=torch.Generator().manual_seed(V + TN))
    want, outside = R.frustum_adjoint64(d_out.double(), K[views], RT[views], V, projection)
    if near:
        assert 0.05 <= outside <= 0.60, outside
    eng = engine_for(V, projection, D, S)
    set_sample(eng, "v300", K, RT)
    g = d_out.cuda()
    check_forms(f"frustum V={V} D={D} S={S} TN={TN} {projection} {'near' if near else 'stage'} rig (outside {outside:.2f})",
                lambda det: eng.op_frustum_adjoint(g, views, deterministic=det), want)


@pytest.mark.parametrize("kind", ["v300", "v900", "off-centre"])
@pytest.mark.parametrize("V", [8, 16])
def test_latent_adjoint(V, kind):
    eng = engine_for(V, "perspective", *((5, 6) if V == 8 else (6, 8)))
    K, RT = R.rig(N, "perspective", 64)
    verts, coord, out_sh, bounds = set_sample(eng, kind, K, RT)
    grid, n_rows = R.rulebook_grid(coord, out_sh)
    d_vol = torch.randn(V, V, V, 64, generator=torch.Generator().manual_seed(V))
    want = R.latent_adjoint64(d_vol.double(), grid, n_rows, bounds[0], out_sh)
    assert want.abs().max() > 0
    g = d_vol.cuda()
    check_forms(f"latent V={V} mesh={kind} rows={n_rows} grid={tuple(grid.shape)}",
                lambda det: eng.op_latent_adjoint(g, deterministic=det), want)


@pytest.mark.parametrize("kind,projection", [("v300", "perspective"), ("v300", "orthographic"), ("crowded", "perspective"),
                                             ("scaled-1.3", "perspective"), ("leaving", "perspective"),
                                             ("leaving", "orthographic")])
def test_vertex_adjoint(kind, projection):
    V = 8
    eng = engine_for(V, projection)
    K, RT = R.rig(N, projection, 8 * S_MAP)
    verts = set_sample(eng, kind, K, RT)[0]
    Nv = verts.shape[0]
    d_vf = torch.randn(N, Nv, 16, generator=torch.Generator().manual_seed(Nv))
    want, leaving = R.vertex_adjoint_two_stage64(d_vf.double(), verts, K, RT, V, S_MAP, projection)
    if kind == "leaving":
        assert 1 <= leaving < Nv / 2, leaving
    if kind == "v300":
        assert Nv % 8
    g = d_vf.cuda()
    check_forms(f"vertex mesh={kind} Nv={Nv} {projection} (vertices with a corner outside: {leaving})",
                lambda det: eng.op_vertex_adjoint(g, deterministic=det), want)


# ---- 2. the conditioner's backward as a whole ----------------------------------------------------------------------------------
def _dsrc(vcfg, B, gen):
    out, d, s = {}, vcfg.frustum_volume_depth, vcfg.frustum_volume_size
    for lvl in range(4):
        out[s] = torch.randn(B, vcfg.frustum_dims[lvl], d, s, s, generator=gen) * (0.5 ** lvl)
        d, s = (d - 1) // 2 + 1, (s - 1) // 2 + 1
    return out


@pytest.mark.parametrize("mesh", ["distinct voxels", "duplicate voxels"])
def test_conditioner_backward_repeats_bit_for_bit(mesh):
    from tests.test_gpu_train import make_train_model
    vcfg = VolumeConfig(num_views=N)
    m = make_train_model(gi.SMALL_UNET, vcfg, N, workspace_gb=8.0)
    if mesh == "distinct voxels":
        batch = synthetic.make_batch(N, "perspective", 500, mesh_seed=1)
    else:  # several vertices per 5 mm voxel: the fold of their rows is part of the mode
        from morphablediffusion_amd import batch as BT
        batch = BT.build_batch(torch.zeros(256, 256, 3), synthetic.ellipsoid_mesh(900, 3, radii=(0.09, 0.11, 0.10), dedup=False),
                               num_views=N)
        batch = {k: v for k, v in batch.items() if torch.is_tensor(v)}
    gen = torch.Generator().manual_seed(9)
    x = (torch.randn(N, 4, 32, 32, generator=gen) * 0.8).cuda()
    from oracle import mvd_oracle as O
    v_embed = O.viewpoint_embedding(batch)[0].cuda()
    dsrc = {k: v.cuda() for k, v in _dsrc(vcfg, 1, gen).items()}
    m.spatial_volume._set_sample({k: v.cuda() for k, v in batch.items()}, 0)
    eng = m.engine

    def run():
        eng.zero_grad()
        out = eng.train_conditioner_backward(x, 421, v_embed, 2, dsrc, debug=True)
        torch.cuda.synchronize()
        return [t.clone() for t in out] + [eng.flat_grads.clone()]

    # the atomic mode's values: the mean of eight runs.  One run's own noise in dL/d(step embedding) -- a sum over every row with
    # heavy cancellation -- measured 4.7e-6 to 8.5e-6 between two runs, as large as the bound, and against a single run the
    # deterministic result measured 6.8e-6 to 1.13e-5 (five sessions); the other tensors 1.3e-6 to 4.3e-6
    runs = [run() for _ in range(8)]
    atomic = [torch.stack([r[i].double() for r in runs]).mean(0) for i in range(5)]
    eng.train_set_deterministic(True)
    det = [run() for _ in range(3)]
    names = ("dvol", "dfused", "dfeats", "dtemb", "gradient arena")
    for i, (name, a, first, *rest) in enumerate(zip(names, atomic, *det)):
        assert torch.isfinite(first).all() and first.abs().max() > 0, name
        for other in rest:
            assert torch.equal(other, first), f"{name} does not repeat bit for bit in the deterministic mode"
        r = R.rel_l2(first, a)
        print(f"[det] conditioner backward ({mesh}) {name}: deterministic vs atomic relL2={r:.3e} "
              f"(atomic vs atomic {R.rel_l2(runs[1][i], runs[0][i]):.3e}, deterministic vs one atomic run {R.rel_l2(first, runs[0][i]):.3e})")
        assert r <= PARITY, name
    eng.close()


# ---- 3. the whole step -----------------------------------------------------------------------------------------------------------
def _two_sample_batch():
    b0 = synthetic.make_batch(N, "perspective", 600, mesh_seed=1)
    meshes = [synthetic.ellipsoid_mesh(600, seed, dedup=False) for seed in (1, 2)]  # two different meshes, the same vertex count
    vox = [synthetic.voxelize(v) for v in meshes]
    batch = {k: v.repeat(2, *([1] * (v.dim() - 1))).clone() for k, v in b0.items() if k not in ("vertices", "coord", "out_sh", "bounds")}
    batch["vertices"] = torch.stack(meshes)
    for i, k in enumerate(("coord", "out_sh", "bounds")):
        batch[k] = torch.stack([v[i] for v in vox])
    return {k: v.cuda() for k, v in batch.items()}


def test_training_step_and_optimiser_steps_repeat_bit_for_bit():
    from tests.test_gpu_train import make_train_model
    B = 2
    vcfg = VolumeConfig(num_views=N)
    batch = _two_sample_batch()
    gen = torch.Generator().manual_seed(5)
    prepared = ((torch.randn(B, N, 4, 32, 32, generator=gen) * 0.8).cuda(), torch.randn(B, 1, 768, generator=gen).cuda(),
                {"x": (torch.randn(B, 4, 32, 32, generator=gen) * 0.18215).cuda()})
    draws = dict(time_steps=torch.tensor([301, 777]), noise=torch.randn(B, N, 4, 32, 32, generator=gen),
                 target_index=torch.tensor([[1], [3]]))
    m = make_train_model(gi.SMALL_UNET, vcfg, N, deterministic=True)  # (the parent has no such argument)
    assert m.deterministic and m.engine.deterministic
    m.model.drop_conditions = False
    outs = []
    for rec in (False, True, True):
        m.recompute = rec
        m.engine.zero_grad()
        loss = m.training_step(batch, prepared=prepared, **draws)
        torch.cuda.synchronize()
        outs.append((float(loss), m.engine.flat_grads.clone()))
    from tests.test_gpu_train import _unet_range
    hi = _unet_range(m.engine)
    assert torch.isfinite(outs[0][1]).all() and outs[0][1][hi:].abs().max() > 0
    for loss, grads in outs[1:]:
        assert loss == outs[0][0]
        assert torch.equal(grads, outs[0][1]), "the gradient arena (conditioner range included) does not repeat bit for bit"
    calls = m.engine.adjoint_calls()
    assert calls["atomic"] == (0, 0, 0) and calls["gather"] == (3 * B, 3 * B, 3 * B), calls
    m.engine.close()
    arenas = []
    for _ in range(2):
        m = make_train_model(gi.SMALL_UNET, vcfg, N, deterministic=True)  # (loads gi.full_weights: the same state dict)
        m.model.drop_conditions = False
        m.learning_rate = 5e-5
        (opt,), _ = m.configure_optimizers()
        for _ in range(2):
            opt.zero_grad()
            m.training_step(batch, prepared=prepared, **draws)
            opt.step()
        torch.cuda.synchronize()
        assert opt.steps_done == 2 and opt.steps_skipped == 0
        arenas.append(m.engine.flat_params.clone())
        m.engine.close()
    assert torch.equal(arenas[0], arenas[1]), "two models from one state dict differ after two identical optimiser steps"


# ---- 4. the default is untouched -------------------------------------------------------------------------------------------------
def test_default_runs_the_atomic_forms_and_the_switch_toggles():
    from morphablediffusion_amd import lib as L
    from tests.test_gpu_train import make_train_model
    vcfg = VolumeConfig(num_views=N)
    m = make_train_model(gi.SMALL_UNET, vcfg, N)
    assert m.deterministic is False
    m.model.drop_conditions = False
    b0 = synthetic.make_batch(N, "perspective", 500, mesh_seed=1)
    batch = {k: v.cuda() for k, v in b0.items()}
    gen = torch.Generator().manual_seed(5)
    prepared = ((torch.randn(1, N, 4, 32, 32, generator=gen) * 0.8).cuda(), torch.randn(1, 1, 768, generator=gen).cuda(),
                {"x": (torch.randn(1, 4, 32, 32, generator=gen) * 0.18215).cuda()})
    draws = dict(time_steps=torch.tensor([301]), noise=torch.randn(1, N, 4, 32, 32, generator=gen), target_index=torch.tensor([[1]]))

    def step():
        m.engine.zero_grad()
        m.training_step(batch, prepared=prepared, **draws)
        torch.cuda.synchronize()
        c = m.engine.adjoint_calls()
        return c["atomic"] + c["gather"]

    assert step() == (1, 1, 1, 0, 0, 0)
    m.deterministic = True
    assert step() == (1, 1, 1, 1, 1, 1)
    m.deterministic = False
    assert step() == (2, 2, 2, 1, 1, 1)
    m.engine.close()
    # the switch is an error on a context that is not a training context
    eng = engine_for(8, "perspective")
    with pytest.raises(L.MvdError, match="training context"):
        eng.train_set_deterministic(True)
    assert eng.deterministic is False


def test_switch_is_refused_when_the_sparse_cnn_runs_in_its_site_form(monkeypatch):
    """The site form's data gradient adds with fp32 atomics: the switch says so at once, not in the middle of a backward pass."""
    from morphablediffusion_amd import lib as L
    from tests.test_gpu_train import make_train_model
    monkeypatch.setenv("MVD_SPARSE_VALU", "1")
    m = make_train_model(gi.SMALL_UNET, VolumeConfig(num_views=N), N)
    with pytest.raises(L.MvdError, match="site form"):
        m.deterministic = True
    assert m.deterministic is False
    m.engine.close()

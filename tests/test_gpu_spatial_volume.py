"""GPU: SpatialVolumeNet(use_spatial_volume=True) -- the dense multi-view unprojection kernel, the SpatialTime3DNet executor, the
add into the mesh volume, the samplers with the switch on, and the error paths -- against the fp32 torch restatement of
tests/test_spatial_volume_cpu.py (itself pinned to the reference's fixture) and against tests/golden/spatial_time_small.npz.

Bounds.  Unprojection: the output is the fp16 operand, one rounding per value: 1e-3 relative L2.  Network output and final
volume: the rule is 1.5 x the worst relative L2 measured on an MI355X against the fp32 restatement, capped by what
tests/test_gpu_model.py::compare allows the frustum network's stage goldens (1e-3) -- the same structure at the same operand
precision, so a larger value means a bug.  NO GPU could be obtained while this file was written: nothing here has run yet, no
figure has been measured, and NET_BOUND is the cap alone.  The first GPU session prints every figure ("[spatial] ..." lines, each
before its assertion), records them in profiles/spatial_volume_parity.json and sets MEASURED_WORST from them."""
import os

import numpy as np
import pytest
import torch

from morphablediffusion_amd import synthetic
from morphablediffusion_amd.spec import UNetConfig, VolumeConfig, time_embed_manifest, volume_manifest
from morphablediffusion_amd.weights import seeded_state_dict
from tests import golden_inputs as gi
from tests import test_spatial_volume_cpu as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
UNPROJECT_BOUND = 1e-3
FRUSTUM_STAGE_BOUND = 1e-3                       # tests/test_gpu_model.py: compare(..., "frustum_*")
MEASURED_WORST = None                           # not measured yet (module docstring)
NET_BOUND = FRUSTUM_STAGE_BOUND if MEASURED_WORST is None else min(1.5 * MEASURED_WORST, FRUSTUM_STAGE_BOUND)
SMALL_DIMS = (64, 32, 64, 128)
# (V, S, spatial_dims): the coarsest level of the first is one voxel and its transposed convs go 1 -> 2 -> 4 -> 8
NET_CASES = {"v8": (8, 16, SMALL_DIMS), "v16": (16, 32, (64, 128, 256, 512))}
N = 4
_weights = {}


def stage_config(V, S, dims, projection="perspective", on=True):
    return VolumeConfig(num_views=N, projection=projection, input_image_size=8 * S, spatial_volume_size=V,
                        use_spatial_volume=on, spatial_dims=dims, frustum_dims=SMALL_DIMS)


def stage_weights(vcfg, style):
    """Conditioner + step-embedding weights of a stage engine (no UNet), seeded; cached: drawing them dominates a test's time."""
    key = (vcfg.spatial_volume_size, vcfg.spatial_dims, vcfg.use_spatial_volume, vcfg.frustum_dims, style)
    if key not in _weights:
        man = dict(volume_manifest(vcfg), **time_embed_manifest(vcfg.time_dim))
        _weights[key] = seeded_state_dict(man, gi.WEIGHT_SEED if style == "init" else gi.TRAINED_SEED, style)
    return _weights[key]


def stage_engine(vcfg, W, S):
    from morphablediffusion_amd.engine import Engine
    eng = Engine(UNetConfig(model_channels=64, image_size=S), vcfg, workspace_gb=1.0)
    eng.load_state_dict(W, expected={k: tuple(v.shape) for k, v in W.items()})
    return eng


def set_sample(eng, batch):
    eng.select_sample(0)
    eng.set_mesh(batch["vertices"][0], batch["coord"][0], batch["out_sh"][0], batch["bounds"][0])
    eng.set_cameras(batch["target_K"][0], batch["target_RT"][0])


# ---- 1. the unprojection kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("projection", ["perspective", "orthographic"])
@pytest.mark.parametrize("V,S", [(8, 16), (16, 32)])
def test_stage_unproject_matches_the_restatement(V, S, projection):
    vcfg = stage_config(V, S, SMALL_DIMS, projection)
    eng = stage_engine(vcfg, stage_weights(vcfg, "init"), S)
    batch = R.stage_batch(N, projection, 300, 8 * S)
    set_sample(eng, batch)
    feats = torch.randn(N, 16, S, S, generator=torch.Generator().manual_seed(V + S))
    want = R.unproject_views(feats, batch["target_K"][0], batch["target_RT"][0], V, vcfg.spatial_volume_length, 8 * S, projection)
    zero = (want == 0).float().mean().item()
    assert 0.0 < zero < 0.5, f"the rig must leave some, and fewer than half, of the samples outside the image: {zero}"
    got = eng.stage_unproject(feats.cuda()).cpu()
    assert got.shape == want.shape == (N * 16, V, V, V)
    r = R.rel_l2(got, want)
    print(f"[spatial] unproject V={V} S={S} {projection}: relL2={r:.2e} zero share={zero:.3f}")
    assert r <= UNPROJECT_BOUND
    # the boundary cases of tests/test_cond_gathers_cpu.py (this rig, the near rig, the rig with the cameras inside the cube) against
    # its float64 restatement: no element unwritten, exact zeros where no tap is in range, e_kernel <= 1.1 e_round + 4 e_oracle32
    # over the whole output and over the partially-outside rows alone, identical bits from two calls
    from morphablediffusion_amd import lib as L
    from tests import test_cond_gathers_cpu as GC
    from tests.test_train_deterministic_cpu import rel_l2 as rel64
    opd = torch.bfloat16 if L.DTYPE == "bf16" else torch.float16
    for case in [c for c in GC.UNPROJECT_CASES if c[:3] == (V, S, projection)]:
        c = GC.unproject_case(*case)
        if case[3] == "stage":
            assert torch.equal(c["K"], batch["target_K"][0]) and torch.equal(c["RT"], batch["target_RT"][0]) and torch.equal(c["x"], feats)
        eng.set_cameras(c["K"], c["RT"])
        x = c["x"].cuda()
        first, second = eng.stage_unproject(x), eng.stage_unproject(x)
        torch.cuda.synchronize()
        assert torch.equal(first, second)
        got, want64 = first.cpu(), c["want"]
        assert torch.isfinite(got).all()
        rows = lambda t: t.reshape(N, 16, -1).transpose(1, 2)
        taps = c["taps"]
        partial = (taps > 0) & (taps < 4)
        e_round, e32 = rel64(want64.to(opd), want64), c["e_oracle32"]
        e_all, r32 = rel64(got, want64), R.rel_l2(got, R.unproject_views(c["x"], c["K"], c["RT"], V, vcfg.spatial_volume_length, 8 * S, projection))
        e_part = e_round_p = e32_p = 0.0
        if partial.any():
            wp = rows(want64)[partial]
            e_part, e_round_p, e32_p = rel64(rows(got)[partial], wp), rel64(wp.to(opd), wp), rel64(rows(c["oracle32"])[partial], wp)
        outside, p_share, none = GC.shares(c)
        print(f"[gather] unproject {GC.case_id(case)}: e_kernel={e_all:.3e} (partial rows {e_part:.3e}) e_oracle32={e32:.3e} (partial rows "
              f"{e32_p:.3e}) e_round={e_round:.3e} (partial rows {e_round_p:.3e}) taps outside={outside:.3f} rows partial={p_share:.3f} "
              f"rows without a tap={none:.3f} relL2 vs the fp32 restatement={r32:.2e}")
        assert (rows(got)[taps == 0] == 0).all(), "a lattice point without a tap inside the map is not exactly zero"
        assert r32 <= UNPROJECT_BOUND
        assert e_all <= 1.1 * e_round + 4 * e32
        assert e_part <= 1.1 * e_round_p + 4 * e32_p
    eng.close()


# ---- 2. the network ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["init", "trained"])
@pytest.mark.parametrize("case", sorted(NET_CASES))
def test_spatial_time_net_output_matches_the_restatement(case, style):
    from oracle import mvd_oracle as O
    V, S, dims = NET_CASES[case]
    vcfg = stage_config(V, S, dims)
    W = stage_weights(vcfg, style)
    eng = stage_engine(vcfg, W, S)
    batch = R.stage_batch(N, "perspective", 300, 8 * S)
    set_sample(eng, batch)
    x, _, v_embed = R.spatial_time_inputs(N, S, 17)
    worst = 0.0
    for step in (41, 961):  # two timesteps: the 13 t_conv rows differ
        t_embed = O.embed_time(W, torch.tensor([step]))
        feats = torch.cat([O.target_encoder(W, x[:, n], t_embed, v_embed[:, n]) for n in range(N)], 0)
        unproj = R.unproject_views(feats, batch["target_K"][0], batch["target_RT"][0], V, vcfg.spatial_volume_length, 8 * S,
                                   "perspective")
        want = R.spatial_time_net(W, unproj[None], t_embed)[0]
        fused = eng.vertex_features(x[0].cuda(), t_embed[0].cuda(), v_embed[0].cuda(), torch.arange(N))
        mesh = eng.volume_from_fused(fused)
        got = eng.spatial_time_volume(x[0].cuda(), t_embed[0].cuda(), v_embed[0].cuda())
        assert got.shape == (64, V, V, V) and torch.isfinite(got).all()
        r = R.rel_l2(got.cpu(), want)
        worst = max(worst, r)
        print(f"[spatial] net {case} {style} t={step}: relL2={r:.2e}")
        assert r <= NET_BOUND
        assert mesh.shape == got.shape
    eng.close()
    print(f"[spatial] net {case} {style}: worst relL2={worst:.2e}")


# ---- 3. the add ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GOLDEN_CASES)
def test_construct_spatial_volume_adds_the_net_output(case):
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.model import SpatialVolumeNet
    g = np.load(os.path.join(G, "spatial_time_small.npz"))
    vcfg, batch, x, t_embed, v_embed, W = R.golden_config(g, case)
    S, V = x.shape[-1], vcfg.spatial_volume_size
    dev = {k: v.cuda() for k, v in batch.items()}
    nets, vols, frusta = {}, {}, {}
    idx = torch.arange(0, 2)
    for on in (True, False):
        sv = SpatialVolumeNet(vcfg.time_dim, vcfg.view_dim, N, input_image_size=8 * S, spatial_volume_size=V,
                              projection=vcfg.projection, use_spatial_volume=on).eval()
        assert sv.cfg.spatial_dims == (64, 128, 256, 512)  # the reference's hard-wired widths
        eng = Engine(UNetConfig(model_channels=64, image_size=S), sv.cfg, workspace_gb=1.0)
        eng.load_state_dict(W, expected=volume_manifest(sv.cfg))  # switch off: the new keys are ignored like any unknown key
        sv.bind(eng)
        vols[on] = sv.construct_spatial_volume(x.cuda(), t_embed.cuda(), v_embed.cuda(), dev)
        if on:  # what the engine holds is the same sum: its frustum stage reads it
            frusta["held"] = eng.frustum_volumes(t_embed[0].cuda(), v_embed[0, idx].cuda(), idx)
            nets[on] = eng.spatial_time_volume(x[0].cuda(), t_embed[0].cuda(), v_embed[0].cuda())
        else:
            eng.set_volume(vols[True][0])
            frusta["set"] = eng.frustum_volumes(t_embed[0].cuda(), v_embed[0, idx].cuda(), idx)
        eng.close()
    assert torch.equal(vols[True][0], vols[False][0] + nets[True])
    for k in frusta["held"]:
        assert torch.equal(frusta["held"][k], frusta["set"][k]), k
    for got, key in ((nets[True][None], "net_out"), (vols[True], "volume")):
        a, b, _ = gi.unpack_compare(got.cpu(), g, f"{case}.{key}")
        r = R.rel_l2(a, b)
        print(f"[spatial] golden {case}.{key}: relL2={r:.2e}")
        assert r <= NET_BOUND


# ---- 4. through the samplers ---------------------------------------------------------------------------------------------------
def full_model(**kw):
    from morphablediffusion_amd.model import SyncMultiviewDiffusion
    ucfg = gi.SMALL_UNET
    p = dict(volume_dims=list(ucfg.volume_dims), image_size=32, in_channels=8, out_channels=4, model_channels=64,
             attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8,
             use_spatial_transformer=True, transformer_depth=1, context_dim=768, use_checkpoint=True, legacy=False)
    m = SyncMultiviewDiffusion(unet_config={"target": "ldm.models.diffusion.attention.DepthWiseAttention", "params": p},
                               view_num=N, image_size=256, cfg_scale=2.0, batch_view_num=N, workspace_gb=4.0, **kw)
    key = ("full", m.spatial_volume.cfg.use_spatial_volume)
    if key not in _weights:
        _weights[key] = gi.full_weights(ucfg, m.spatial_volume.cfg)
    m.load_state_dict(_weights[key], strict=True)
    return m.eval()


@pytest.fixture(scope="module")
def model_on():
    m = full_model(use_spatial_volume=True)
    yield m
    m.engine.close()


def two_samples():
    from morphablediffusion_amd.batch import voxelize
    b0 = synthetic.make_batch(N, "perspective", 500, mesh_seed=1)
    b1 = synthetic.make_batch(N, "perspective", 500, mesh_seed=2, radii=(0.2, 0.25, 0.27))
    nv = min(b0["vertices"].shape[1], b1["vertices"].shape[1])

    def cut(b):
        v = b["vertices"][:, :nv]
        coord, out_sh, bounds = voxelize(v[0])
        return dict(b, vertices=v, coord=coord[None], out_sh=out_sh[None], bounds=bounds[None])

    b0, b1 = cut(b0), cut(b1)
    both = {k: torch.cat([b0[k], b1[k]]) for k in b0}
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, N, 4, 32, 32, generator=g)
    x_in = torch.randn(2, 4, 32, 32, generator=g) * 0.18215
    clip = torch.randn(2, 1, 768, generator=g)
    noise = torch.randn(2, N, 4, 32, 32, generator=g)
    return (b0, b1, both), x, x_in, clip, noise


def to_dev(b):
    return {k: v.cuda() for k, v in b.items()}


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_one_step_with_the_switch_on(model_on, kind):
    """B = 1, B = 2 in the per-sample loop and B = 2 batched: the loop equals the single-sample runs bit for bit, the batched
    pass equals them to the existing batched-vs-single bound (tests/test_gpu_model.py, tests/test_gpu_sampler_dpm.py), and the
    step differs from the switch-off step of the same weights (the stage is not silently skipped)."""
    from morphablediffusion_amd.model import SyncDDIMSampler, SyncDPMSolverSampler
    m = model_on
    if kind == "ddim":
        s, index, x_bound = SyncDDIMSampler(m, 50, "uniform", 1.0), 30, 1e-4
    else:
        s = SyncDPMSolverSampler(m, 6)
        index, x_bound = len(s.ddim_timesteps) - 1, 1e-3  # the first step (no history); bound: tests/test_gpu_sampler_dpm.py
    step = int(np.flip(s.ddim_timesteps)[len(s.ddim_timesteps) - 1 - index])
    (b0, b1, both), x, x_in, clip, noise = two_samples()

    def run(sel, batch, mode):
        s.sample_batching = mode
        m.spatial_volume.invalidate()
        ts = torch.full((len(sel),), step, dtype=torch.long, device="cuda")
        return s.denoise_apply(x[sel].cuda(), {"x": x_in[sel].cuda()}, clip[sel].cuda(), ts, index, 2.0, batch_view_num=N,
                               batch=to_dev(batch), noise=noise[sel].cuda(), return_eps=True)

    singles = [run([0], b0, "batched"), run([1], b1, "batched")]
    loop = run([0, 1], both, "loop")
    batched = run([0, 1], both, "batched")
    for i in range(2):
        assert torch.isfinite(singles[i][0]).all()
        assert torch.equal(loop[0][i], singles[i][0][0]) and torch.equal(loop[1][i], singles[i][1][0]), i
        rx, re = R.rel_l2(batched[0][i], singles[i][0][0]), R.rel_l2(batched[1][i], singles[i][1][0])
        print(f"[spatial] {kind} sample {i} batched vs alone: eps relL2={re:.2e} x relL2={rx:.2e}")
        assert re <= 1e-3 and rx <= x_bound
    assert not torch.allclose(loop[1][0], loop[1][1])
    # each slot's volume got its own add: swapping which sample sits in which slot swaps the results
    swapped = {k: torch.cat([b1[k], b0[k]]) for k in b0}
    s.sample_batching = "batched"
    m.spatial_volume.invalidate()
    ts = torch.full((2,), step, dtype=torch.long, device="cuda")
    sw = s.denoise_apply(x[[1, 0]].cuda(), {"x": x_in[[1, 0]].cuda()}, clip[[1, 0]].cuda(), ts, index, 2.0, batch_view_num=N,
                         batch=to_dev(swapped), noise=noise[[1, 0]].cuda(), return_eps=True)
    assert R.rel_l2(sw[1][0], singles[1][1][0]) <= 1e-3 and R.rel_l2(sw[1][1], singles[0][1][0]) <= 1e-3


def test_switch_off_step_is_bit_identical_and_switch_on_differs(model_on):
    from morphablediffusion_amd.model import SyncDDIMSampler
    (b0, _, _), x, x_in, clip, noise = two_samples()
    outs = []
    for kw in ({}, {"use_spatial_volume": False}):
        m = full_model(**kw)
        assert not m.spatial_volume.cfg.use_spatial_volume
        ts = torch.full((1,), int(m.sampler.ddim_timesteps[30]), dtype=torch.long, device="cuda")
        outs.append(m.sampler.denoise_apply(x[:1].cuda(), {"x": x_in[:1].cuda()}, clip[:1].cuda(), ts, 30, 2.0, batch_view_num=N,
                                            batch=to_dev(b0), noise=noise[:1].cuda(), return_eps=True))
        m.engine.close()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    s = SyncDDIMSampler(model_on, 50, "uniform", 1.0)
    model_on.spatial_volume.invalidate()
    on = s.denoise_apply(x[:1].cuda(), {"x": x_in[:1].cuda()}, clip[:1].cuda(), ts, 30, 2.0, batch_view_num=N, batch=to_dev(b0),
                         noise=noise[:1].cuda(), return_eps=True)
    assert R.rel_l2(on[1], outs[0][1]) > 1e-2, "the dense volume left no trace in the noise prediction"


def test_forward_only_training_step(model_on):
    (_, _, both), x, x_in, clip, noise = two_samples()
    m = model_on
    m.spatial_volume.invalidate()
    loss = m.training_step(to_dev(both), prepared=(x, clip, {"x": x_in}), time_steps=torch.tensor([601, 101]), noise=noise,
                           target_index=torch.tensor([[1], [3]]), backward=False)
    m.eval()
    assert torch.isfinite(loss) and float(loss) > 0
    assert m.last_noise_predict.shape == (2, 4, 32, 32)


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------
def test_errors():
    from morphablediffusion_amd.engine import Engine
    from morphablediffusion_amd.lib import MvdError
    from morphablediffusion_amd.model import SyncDDIMSampler, SyncDPMSolverSampler, SyncMultiviewDiffusion
    V, S = 8, 16
    vcfg = stage_config(V, S, SMALL_DIMS)
    W = stage_weights(vcfg, "init")
    missing = "spatial_volume.spatial_volume_feats.conv3.bn.bias"
    part = {k: v for k, v in W.items() if k != missing}
    eng = Engine(UNetConfig(model_channels=64, image_size=S), vcfg, workspace_gb=1.0)
    with pytest.raises(RuntimeError, match="conv3.bn.bias"):  # strict: reported before anything is uploaded
        eng.load_state_dict(part, strict=True, expected={k: tuple(v.shape) for k, v in W.items()})
    with pytest.raises(MvdError, match=missing.replace(".", r"\.")):  # not strict: finalize names the key
        eng.load_state_dict(part, expected={k: tuple(v.shape) for k, v in W.items()})
    eng.close()
    eng = stage_engine(vcfg, W, S)
    x, t_embed, v_embed = [t.cuda() for t in R.spatial_time_inputs(N, S, 3)]
    with pytest.raises(MvdError, match="mvd_set_mesh"):
        eng.spatial_time_volume(x[0], t_embed[0], v_embed[0])
    set_sample(eng, R.stage_batch(N, "perspective", 300, 8 * S))
    with pytest.raises(MvdError, match="num_views"):
        eng.spatial_time_volume(x[0, :2], t_embed[0], v_embed[0, :2])
    with pytest.raises(MvdError, match="num_views"):
        eng.stage_unproject(torch.zeros(2, 16, S, S).cuda())
    eng.close()
    off = stage_config(V, S, SMALL_DIMS, on=False)
    eng = stage_engine(off, stage_weights(off, "init"), S)
    set_sample(eng, R.stage_batch(N, "perspective", 300, 8 * S))
    with pytest.raises(MvdError, match="use_spatial_volume"):
        eng.spatial_time_volume(x[0], t_embed[0], v_embed[0])
    eng.close()
    with pytest.raises(NotImplementedError, match="train_mode.*use_spatial_volume"):
        SyncMultiviewDiffusion(unet_config={}, use_spatial_volume=True, train_mode=True)


def test_sharded_sampling_is_refused(model_on):
    from morphablediffusion_amd.model import SyncDDIMSampler, SyncDPMSolverSampler
    with pytest.raises(NotImplementedError, match="shard_views.*use_spatial_volume"):
        SyncDDIMSampler(model_on, 50, shard_views=True)
    with pytest.raises(NotImplementedError, match="shard_views.*use_spatial_volume"):
        SyncDPMSolverSampler(model_on, 6, shard_views=True)
    s = SyncDDIMSampler(model_on, 50)
    s.simulate_world = 2  # bench.py's one-rank-of-two timing aid shards the views too
    (b0, _, _), x, x_in, clip, noise = two_samples()
    ts = torch.full((1,), int(s.ddim_timesteps[30]), dtype=torch.long, device="cuda")
    with pytest.raises(NotImplementedError, match="use_spatial_volume"):
        s.denoise_apply(x[:1, :2].cuda(), {"x": x_in[:1].cuda()}, clip[:1].cuda(), ts, 30, 2.0, batch_view_num=2, batch=to_dev(b0),
                        noise=noise[:1, :2].cuda())

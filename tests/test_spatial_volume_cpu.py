"""use_spatial_volume=True without a GPU: a functional torch restatement of the dense multi-view unprojection
(morphable_diffusion.py:197-225) and of SpatialTime3DNet (network.py:209-283), pinned against the fixture the reference's
own modules produced (tests/golden/spatial_time_small.npz); the manifest keys; the VolumeConfig validation.

The restatement (``unproject_views``, ``spatial_time_net``, ``spatial_time_inputs``) is what tests/test_gpu_spatial_volume.py
holds the HIP stage against."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from morphablediffusion_amd import synthetic
from morphablediffusion_amd.spec import (SPATIAL_TIME_BLOCKS, VolumeConfig, spatial_time_manifest, volume_manifest)
from morphablediffusion_amd.weights import seeded_state_dict
from tests import golden_inputs as gi

G = os.path.join(os.path.dirname(__file__), "golden")
SV = "spatial_volume.spatial_volume_feats."
GOLDEN_CASES = ("persp", "ortho")


# ---------------------------------------------------------------------------------------------- the restatement
def lattice_points(V, length):
    """World xyz of the V^3 lattice as [3, V^3]: voxel (iz, iy, ix) sits at (lin[ix], lin[iy], lin[iz])."""
    lin = torch.linspace(-length, length, V, dtype=torch.float32)
    z, y, x = torch.meshgrid(lin, lin, lin, indexing="ij")
    return torch.stack([x, y, z], 0).reshape(3, -1)


def view_grid(pts, K, RT, S, image_size, projection):
    """Normalised grid_sample coordinates [V^3, 2] of the lattice in one view's S x S feature map."""
    if projection == "perspective":
        r = S / image_size
        P = torch.diag(torch.tensor([r, r, 1.0])) @ K[:3, :3] @ RT
        q = P[:, :3] @ pts + P[:, 3:]
        w = q[2:].clamp(min=1e-4)
        return (q[:2] / w / ((S - 1) / 2) - 1.0).t()
    P = K @ torch.cat([RT, torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    return (P[:3, :3] @ pts + P[:3, 3:])[:2].t()


def unproject_views(feats, K, RT, V, length, image_size, projection):
    """feats [N,16,S,S], K [N,4,4], RT [N,3,4] -> [N*16, V, V, V] (view-major)."""
    N, C, S, _ = feats.shape
    pts = lattice_points(V, length)
    out = []
    for n in range(N):
        g = view_grid(pts, K[n], RT[n], S, image_size, projection).view(1, V, V * V, 2)
        u = F.grid_sample(feats[n:n + 1], g, mode="bilinear", padding_mode="zeros", align_corners=True)
        out.append(u.view(C, V, V, V))
    return torch.cat(out, 0)


def spatial_time_net(W, x, t, p=SV):
    """x [1, 16N, V, V, V], t [1, time_dim] -> [1, d0, V, V, V]."""
    def block(name, h, stride=1, up=False):
        q = p + name + "."
        h = h + F.conv3d(t.view(1, -1, 1, 1, 1), W[q + "t_conv.weight"], W[q + "t_conv.bias"])
        n = "norm" if up else "bn"
        h = F.silu(F.group_norm(h, 8, W[q + n + ".weight"], W[q + n + ".bias"], 1e-5))
        if up:
            return F.conv_transpose3d(h, W[q + "conv.weight"], W[q + "conv.bias"], stride=2, padding=1, output_padding=1)
        return F.conv3d(h, W[q + "conv.weight"], W[q + "conv.bias"], stride=stride, padding=1)

    h = F.conv3d(x, W[p + "init_conv.weight"], W[p + "init_conv.bias"], padding=1)
    c0 = block("conv0", h)
    c2 = block("conv2_1", block("conv2_0", block("conv1", c0, 2)))
    c4 = block("conv4_1", block("conv4_0", block("conv3", c2, 2)))
    h = block("conv6_1", block("conv6_0", block("conv5", c4, 2)))
    h = c4 + block("conv7", h, up=True)
    h = c2 + block("conv8", h, up=True)
    return c0 + block("conv9", h, up=True)


def spatial_time_inputs(N, S, seed):
    """Seeded stage inputs: noisy latents [1,N,4,S,S], a step embedding [1,256], view embeddings [1,N,4]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, N, 4, S, S, generator=g)
    t_embed = 0.5 * torch.randn(1, 256, generator=g)
    az = torch.linspace(-math.pi / 2, math.pi / 2, N)
    v_embed = torch.stack([0.1 * torch.randn(N, generator=g), torch.sin(az), torch.cos(az), torch.zeros(N)], -1)[None]
    return x, t_embed, v_embed


ORTHO_SCALE = 2.4  # the +-0.5 cube then reaches +-1.2 in the normalised image frame: its outer lattice planes project outside


def stage_batch(N, projection, nverts, image_size):
    """synthetic.make_batch with a rig under which the lattice projects partly outside the image for BOTH projections: the
    FaceScape-style pinhole arc does as it is, the orthographic ring gets a larger scale."""
    batch = synthetic.make_batch(N, projection, nverts, mesh_seed=1, image_size=image_size)
    if projection == "orthographic":
        K, RT = synthetic.ortho_cameras(N, scale=ORTHO_SCALE)
        batch["target_K"], batch["target_RT"] = K[None].contiguous(), RT[None].contiguous()
    return batch


def golden_config(g, case):
    """VolumeConfig, batch, inputs and seeded weights of one case of spatial_time_small.npz (stored by seed, not by value)."""
    N, V, S = int(g[f"{case}.N"]), int(g[f"{case}.V"]), int(g[f"{case}.S"])
    projection = "perspective" if case == "persp" else "orthographic"
    vcfg = VolumeConfig(num_views=N, projection=projection, input_image_size=8 * S, spatial_volume_size=V, use_spatial_volume=True)
    batch = stage_batch(N, projection, int(g[f"{case}.nverts_in"]), 8 * S)
    x, t_embed, v_embed = spatial_time_inputs(N, S, int(g[f"{case}.input_seed"]))
    W = seeded_state_dict(volume_manifest(vcfg), int(g[f"{case}.weight_seed"]), str(g[f"{case}.weight_style"]))
    return vcfg, batch, x, t_embed, v_embed, W


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


# ---------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "spatial_time_small.npz"))


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_restatement_matches_reference_fixture(golden, case):
    """Unprojection and network of the restatement vs the reference's modules on the same seeded inputs: fp32 rounding."""
    from oracle import mvd_oracle as O
    g = golden
    vcfg, batch, x, t_embed, v_embed, W = golden_config(g, case)
    N, V = vcfg.num_views, vcfg.spatial_volume_size
    feats = torch.cat([O.target_encoder(W, x[:, n], t_embed, v_embed[:, n]) for n in range(N)], 0)
    unproj = unproject_views(feats, batch["target_K"][0], batch["target_RT"][0], V, vcfg.spatial_volume_length,
                             vcfg.input_image_size, vcfg.projection)
    a, b, _ = gi.unpack_compare(unproj[None], g, f"{case}.unproj")
    assert b.abs().max() > 0
    zero = (b == 0).float().mean().item()
    assert 0.0 < zero < 1.0, "the rig must put some voxels outside the image and some inside"
    r = rel_l2(a, b)
    print(f"[restatement] {case} unprojection relL2={r:.2e} zero share={zero:.3f}")
    assert r <= 1e-5
    net = spatial_time_net(W, unproj[None], t_embed)
    a, b, _ = gi.unpack_compare(net, g, f"{case}.net_out")
    r = rel_l2(a, b)
    print(f"[restatement] {case} net output relL2={r:.2e}")
    assert r <= 1e-5
    # the final volume: the project's CPU oracle for the mesh volume + the restated network
    mesh = O.construct_spatial_volume(W, vcfg, x, t_embed, v_embed, batch)
    a, b, _ = gi.unpack_compare(mesh + net, g, f"{case}.volume")
    r = rel_l2(a, b)
    print(f"[restatement] {case} final volume relL2={r:.2e}")
    assert r <= 1e-5


@pytest.mark.parametrize("view_num", [4, 16])
def test_manifest_keys_and_shapes(view_num):
    on = VolumeConfig(num_views=view_num, use_spatial_volume=True)
    off = VolumeConfig(num_views=view_num)
    m_on, m_off = volume_manifest(on), volume_manifest(off)
    assert not any("spatial_volume_feats" in k for k in m_off)
    extra = {k: v for k, v in m_on.items() if k not in m_off}
    assert set(m_off) <= set(m_on) and all(m_on[k] == m_off[k] for k in m_off)
    assert all(k.startswith(SV) for k in extra)
    assert extra == {"spatial_volume." + k: v for k, v in spatial_time_manifest(on).items()}
    assert len(extra) == 2 + 13 * 6
    d = on.spatial_dims
    assert extra[SV + "init_conv.weight"] == (64, 16 * view_num, 3, 3, 3) and extra[SV + "init_conv.bias"] == (64,)
    io = [(d[0], d[0]), (d[0], d[1]), (d[1], d[1]), (d[1], d[1]), (d[1], d[2]), (d[2], d[2]), (d[2], d[2]), (d[2], d[3]),
          (d[3], d[3]), (d[3], d[3])]
    for name, (ci, co) in zip(SPATIAL_TIME_BLOCKS, io):
        p = SV + name + "."
        assert extra[p + "t_conv.weight"] == (ci, 256, 1, 1, 1) and extra[p + "t_conv.bias"] == (ci,)
        assert extra[p + "bn.weight"] == (ci,) and extra[p + "bn.bias"] == (ci,)
        assert extra[p + "conv.weight"] == (co, ci, 3, 3, 3) and extra[p + "conv.bias"] == (co,)
    for name, (ci, co) in zip(("conv7", "conv8", "conv9"), [(d[3], d[2]), (d[2], d[1]), (d[1], d[0])]):
        p = SV + name + "."
        assert extra[p + "t_conv.weight"] == (ci, 256, 1, 1, 1)
        assert extra[p + "norm.weight"] == (ci,) and extra[p + "norm.bias"] == (ci,)
        assert extra[p + "conv.weight"] == (ci, co, 3, 3, 3) and extra[p + "conv.bias"] == (co,)  # ConvTranspose3d: (in, out, ...)
    # the restatement runs on exactly these keys
    W = seeded_state_dict(m_on, 1)
    V = 8
    out = spatial_time_net(W, torch.zeros(1, 16 * view_num, V, V, V), torch.zeros(1, 256))
    assert out.shape == (1, 64, V, V, V)


def test_volume_config_validation():
    VolumeConfig().validate()
    VolumeConfig(use_spatial_volume=True).validate()
    VolumeConfig(use_spatial_volume=True, spatial_volume_size=8, spatial_dims=(64, 32, 64, 128)).validate()
    # the constraints bind only with the switch on
    VolumeConfig(spatial_volume_size=12, spatial_dims=(32, 12, 12, 12)).validate()
    with pytest.raises(ValueError, match="64"):
        VolumeConfig(use_spatial_volume=True, spatial_dims=(32, 64, 128, 256)).validate()
    with pytest.raises(ValueError, match="multiple of 8"):
        VolumeConfig(use_spatial_volume=True, spatial_dims=(64, 100, 256, 512)).validate()
    with pytest.raises(ValueError, match="spatial_volume_size"):
        VolumeConfig(use_spatial_volume=True, spatial_volume_size=12).validate()


def test_spatial_volume_net_constructs_and_refuses_what_is_not_built():
    from morphablediffusion_amd.model import SpatialVolumeNet, SyncDDIMSampler
    sv = SpatialVolumeNet(256, 4, 4, use_spatial_volume=True)
    assert sv.cfg.use_spatial_volume and sv.cfg.spatial_dims == (64, 128, 256, 512)
    assert not SpatialVolumeNet(256, 4, 4).cfg.use_spatial_volume
    with pytest.raises(ValueError):
        SpatialVolumeNet(256, 4, 4, spatial_volume_size=12, use_spatial_volume=True)

    class Stub:  # what a sampler reads of its model at construction
        num_timesteps = 1000
        spatial_volume = sv

    with pytest.raises(NotImplementedError, match="shard_views.*use_spatial_volume"):
        SyncDDIMSampler(Stub(), 50, shard_views=True)
    SyncDDIMSampler(Stub(), 50)  # not sharded: constructs

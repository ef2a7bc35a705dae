"""Deterministic training mode, the parts that need no GPU: the C ABI of the new entry points (parsed out of include/mvd.h, resolved
in the built library), the constructor's check, and float64 restatements of the conditioner's three gather adjoints with explicit
index arithmetic -- the yardstick of tests/test_gpu_train_deterministic.py.  The vertex adjoint is restated twice, as the composite
sum over (vertex, corner, tap) and as the two stages through the lattice that the deterministic kernels run (weight = w3(vertex,
corner) * w2(voxel, view, tap)); the two must agree to float64 rounding, and every restatement must agree with autograd through the
oracle's own gather functions (fp32) to fp32 rounding."""
import ctypes as C

import pytest
import torch

from morphablediffusion_amd import lib as L, synthetic
from morphablediffusion_amd.model import SyncMultiviewDiffusion

NEW = {
    "mvd_train_set_deterministic": [C.c_void_p, C.c_int],
    "mvd_op_frustum_adjoint": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "mvd_op_latent_adjoint": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    "mvd_op_vertex_adjoint": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
    "mvd_probe_adjoint_calls": [C.c_void_p, C.c_void_p],
}
VOL_LEN, FRUSTUM_LEN, VOXEL = 0.5, 0.86603, 0.005  # VolumeConfig's defaults


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


# ---------------------------------------------------------------------------------------------- float64 restatements
def linear_scatter(pos, dims, g):
    """Adjoint of an align_corners / zero-padding linear gather.  pos [P, nd] float64 positions in index units, axis 0 the FASTEST
    of ``dims`` (given slowest first, as a tensor's shape); g [P, C].  Returns (out [prod(dims), C], number of (point, corner)
    pairs that fall outside and are skipped)."""
    nd = len(dims)
    lo = torch.floor(pos)
    fr = pos - lo
    out = torch.zeros(int(torch.tensor(dims).prod()), g.shape[1], dtype=torch.float64)
    outside = 0
    for corner in range(1 << nd):
        w = torch.ones(pos.shape[0], dtype=torch.float64)
        idx = torch.zeros(pos.shape[0], dtype=torch.long)
        ok = torch.ones(pos.shape[0], dtype=torch.bool)
        stride = 1
        for a in range(nd):  # a = 0 is x
            bit = (corner >> a) & 1
            size = dims[nd - 1 - a]
            ia = lo[:, a] + bit
            w = w * (fr[:, a] if bit else 1.0 - fr[:, a])
            ok &= (ia >= 0) & (ia <= size - 1)
            idx += ia.clamp(0, size - 1).long() * stride
            stride *= size
        out.index_add_(0, idx[ok], w[ok, None] * g[ok].double())
        outside += int((~ok).sum())
    return out, outside


def projection64(K, RT, ratio, projection):
    """construct_project_matrix in float64: one view's K [4,4], RT [3,4] -> [4,4]."""
    K, RT4 = K.double(), torch.cat([RT.double(), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], 0)
    if projection == "perspective":
        P = torch.eye(4, dtype=torch.float64)
        P[:3] = torch.diag(torch.tensor([ratio, ratio, 1.0], dtype=torch.float64)) @ K[:3, :3] @ RT4[:3]
        return P
    return K @ RT4


def lattice64(V, length=VOL_LEN):
    """[V^3, 3] world xyz of the lattice, x fastest."""
    lin = torch.linspace(-length, length, V, dtype=torch.float64)
    z, y, x = torch.meshgrid(lin, lin, lin, indexing="ij")
    return torch.stack([x, y, z], -1).reshape(-1, 3)


def frustum_positions64(K, RT, V, D, S, projection):
    """Lattice positions [TN*D*S*S, 3] (x, y, z in index units) of the frustum points of views K [TN,4,4], RT [TN,3,4]."""
    pos = []
    ys, xs = torch.meshgrid(torch.arange(S, dtype=torch.float64), torch.arange(S, dtype=torch.float64), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    for n in range(K.shape[0]):
        R = RT[n].double()
        dist = (-(R[:, :3].t() @ R[:, 3])).norm()
        depth = torch.linspace(0, 1, D, dtype=torch.float64) * (2 * FRUSTUM_LEN) + (dist - FRUSTUM_LEN)  # [D]
        if projection == "perspective":
            Pinv = torch.linalg.inv(projection64(K[n], RT[n], 1.0 / 8.0, projection))
            cam = torch.stack([xs[None] * depth[:, None], ys[None] * depth[:, None], depth[:, None].expand(D, S * S)], -1)
        else:
            Kinv = torch.linalg.inv(K[n].double())
            pix = torch.stack([2 * xs / (S - 1) - 1, 2 * ys / (S - 1) - 1, torch.ones_like(xs)], 0)
            ab = (Kinv[:3, :3] @ pix)[:2]  # [2, S*S]
            cam = torch.stack([ab[0][None].expand(D, -1), ab[1][None].expand(D, -1), depth[:, None].expand(D, S * S)], -1)
            Pinv = torch.linalg.inv(projection64(torch.eye(4), RT[n], 1.0, "orthographic"))
        world = cam.reshape(-1, 3) @ Pinv[:3, :3].t() + Pinv[:3, 3]
        pos.append((world / VOL_LEN + 1.0) * 0.5 * (V - 1))
    return torch.cat(pos, 0)


def frustum_adjoint64(d_out, K, RT, V, projection):
    """d_out [TN,D,S,S,64] -> (dL/d(volume) [V,V,V,64] float64, share of (point, corner) pairs outside the lattice)."""
    TN, D, S = d_out.shape[:3]
    pos = frustum_positions64(K, RT, V, D, S, projection)
    out, outside = linear_scatter(pos, (V, V, V), d_out.reshape(-1, 64))
    return out.view(V, V, V, 64), outside / (8.0 * pos.shape[0])


def rulebook_grid(coord, out_sh):
    """The coarsest level's index grid [gd,gh,gw] (row per cell, -1 = none) and its row count, from the host rule book."""
    lib = L.load()
    coord, out_sh = coord.to(torch.int32).contiguous(), out_sh.to(torch.int32).contiguous()
    n_sites, lens = (C.c_int32 * 3)(), (C.c_int64 * 6)()
    L.check(lib.mvd_rulebook_build(L.ptr(coord), L.ptr(out_sh), coord.shape[0], 0, n_sites, lens))
    grid = torch.empty(int(lens[5]), dtype=torch.int32)
    L.check(lib.mvd_rulebook_table(5, L.ptr(grid)))
    shape = [int(s) for s in out_sh]
    for _ in range(2):
        shape = [(s - 1) // 2 + 1 for s in shape]
    return grid.view(*shape).long(), int(n_sites[2])


def latent_positions64(V, grid_shape, min_xyz, out_sh):
    g = (lattice64(V) - min_xyz.double()[None]) / VOXEL
    g = g / torch.tensor([float(out_sh[2]), float(out_sh[1]), float(out_sh[0])], dtype=torch.float64) * 2 - 1
    gd, gh, gw = grid_shape
    return (g + 1.0) * 0.5 * torch.tensor([gw - 1, gh - 1, gd - 1], dtype=torch.float64)


def latent_adjoint64(d_vol, grid, n_rows, min_xyz, out_sh):
    """d_vol [V,V,V,64] -> dL/d(rows) [n_rows,64] float64; cells without a row drop what lands on them."""
    V = d_vol.shape[0]
    dense, _ = linear_scatter(latent_positions64(V, tuple(grid.shape), min_xyz, out_sh), tuple(grid.shape), d_vol.reshape(-1, 64))
    rows = torch.zeros(n_rows, 64, dtype=torch.float64)
    cells = grid.reshape(-1)
    rows[cells[cells >= 0]] = dense[cells >= 0]
    return rows


def vertex_positions64(verts, V):
    return (verts.double() / VOL_LEN + 1.0) * 0.5 * (V - 1)


def lattice_pixels64(K, RT, V, S, projection):
    """[V^3, 2] pixel positions (x, y) of the lattice in one view's S x S map (image size 8 S)."""
    P = projection64(K, RT, 1.0 / 8.0, projection)
    q = lattice64(V) @ P[:3, :3].t() + P[:3, 3]
    if projection == "perspective":
        return q[:, :2] / q[:, 2:3].clamp(min=1e-4)
    return (q[:, :2] + 1.0) * 0.5 * (S - 1)


def vertex_adjoint_two_stage64(d_vf, verts, K, RT, V, S, projection):
    """Stage A (vertices -> lattice, per view) then stage B (lattice -> the view's map): d_vf [N,Nv,16] -> [N,S,S,16] float64,
    plus the number of vertices with a corner outside the lattice."""
    pos3 = vertex_positions64(verts, V)
    out = []
    for n in range(d_vf.shape[0]):
        d_lat, _ = linear_scatter(pos3, (V, V, V), d_vf[n])
        d_img, _ = linear_scatter(lattice_pixels64(K[n], RT[n], V, S, projection), (S, S), d_lat)
        out.append(d_img.view(S, S, 16))
    lo = torch.floor(pos3)
    leaving = int(((lo < 0) | (lo + 1 > V - 1)).any(1).sum())
    return torch.stack(out), leaving


def vertex_adjoint_composite64(d_vf, verts, K, RT, V, S, projection):
    """The same adjoint as ONE sum over (vertex, corner, tap) of w3 * w2 * d_vf."""
    pos3 = vertex_positions64(verts, V)
    lo3, out = torch.floor(pos3), []
    fr3 = pos3 - lo3
    for n in range(d_vf.shape[0]):
        pix = lattice_pixels64(K[n], RT[n], V, S, projection)
        img = torch.zeros(S * S, 16, dtype=torch.float64)
        for corner in range(8):
            bits = [(corner >> a) & 1 for a in range(3)]
            i3 = [lo3[:, a] + bits[a] for a in range(3)]
            ok3 = (i3[0] >= 0) & (i3[0] <= V - 1) & (i3[1] >= 0) & (i3[1] <= V - 1) & (i3[2] >= 0) & (i3[2] <= V - 1)
            w3 = torch.ones(pos3.shape[0], dtype=torch.float64)
            for a in range(3):
                w3 = w3 * (fr3[:, a] if bits[a] else 1.0 - fr3[:, a])
            vox = ((i3[2].clamp(0, V - 1) * V + i3[1].clamp(0, V - 1)) * V + i3[0].clamp(0, V - 1)).long()
            p = pix[vox]
            lo2 = torch.floor(p)
            fr2 = p - lo2
            for tap in range(4):
                bx, by = tap & 1, tap >> 1
                xx, yy = lo2[:, 0] + bx, lo2[:, 1] + by
                ok = ok3 & (xx >= 0) & (xx <= S - 1) & (yy >= 0) & (yy <= S - 1)
                w2 = (fr2[:, 0] if bx else 1.0 - fr2[:, 0]) * (fr2[:, 1] if by else 1.0 - fr2[:, 1])
                idx = (yy.clamp(0, S - 1) * S + xx.clamp(0, S - 1)).long()
                img.index_add_(0, idx[ok], (w3 * w2)[ok, None] * d_vf[n][ok].double())
        out.append(img.view(S, S, 16))
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------- shared synthetic cases
def rig(N, projection, image_size, near=False):
    """The synthetic rig of tests/test_spatial_volume_cpu.py::stage_batch (K [N,4,4], RT [N,3,4]), or with near=True one whose
    frustum leaves the lattice in part (5 % to 60 % of the (point, corner) pairs, asserted where it is used).  Perspective: the
    camera distance halved.  Orthographic: the synthetic ring looks AWAY from the origin (depth d sits at distance radius + d),
    so the stage rig's frustum misses the lattice altogether -- kept as the all-outside case -- and halving the distance still
    leaves 90 % outside; the near rig pulls the ring in to radius 0.15, where the depth range [-0.72, 1.02] straddles the cube."""
    from tests.test_spatial_volume_cpu import ORTHO_SCALE
    if projection == "perspective":
        return synthetic.camera_arc(N, radius=2.25 if near else 4.5, focal=1545.23757707405 * image_size / 256.0,
                                    center=image_size / 2.0)
    return synthetic.ortho_cameras(N, radius=0.15 if near else 1.5, scale=ORTHO_SCALE)


def mesh(kind):
    """(vertices, coord, out_sh, bounds) of the test meshes, as the batch dict carries them for one sample."""
    if kind == "v300":
        v = synthetic.ellipsoid_mesh(300, 1)
    elif kind == "v900":
        v = synthetic.ellipsoid_mesh(900, 2)
    elif kind == "off-centre":  # a bounding box that is not centred: the three axes get different windows
        v = synthetic.ellipsoid_mesh(300, 3, radii=(0.12, 0.2, 0.16), dedup=False) + torch.tensor([0.17, -0.11, 0.06])
    elif kind == "crowded":  # many vertices per lattice cell and per pixel, duplicate voxels
        v = synthetic.ellipsoid_mesh(900, 3, radii=(0.09, 0.11, 0.10), dedup=False)
    elif kind == "scaled-1.3":  # radii (0.286, 0.364, 0.325): larger, but still inside the +-0.5 cube
        v = synthetic.ellipsoid_mesh(300, 1) * 1.3
    elif kind == "leaving":  # radii (0.44, 0.56, 0.50): some vertices leave the cube, their outer corners are skipped
        v = synthetic.ellipsoid_mesh(300, 1) * 2.0
    else:
        raise KeyError(kind)
    v = v.contiguous()
    coord, out_sh, bounds = synthetic.voxelize(v)
    return v, coord, out_sh, bounds


# ---------------------------------------------------------------------------------------------- tests
def test_new_entry_points_parse_out_of_the_header_and_resolve_in_the_library():
    for name, argtypes in NEW.items():
        assert name in L.PROTOTYPES, name
        restype, args = L.PROTOTYPES[name]
        assert restype is C.c_int and args == argtypes, (name, args)
    lib = L.load()  # raises when a declared symbol is missing
    for name in NEW:
        assert getattr(lib, name).argtypes == NEW[name]


def test_deterministic_needs_train_mode():
    built = []
    import morphablediffusion_amd.model as M
    orig = M.Engine
    M.Engine = lambda *a, **k: built.append(1)  # the constructor must raise before it builds anything
    try:
        with pytest.raises(ValueError, match="train_mode"):
            SyncMultiviewDiffusion(unet_config={}, deterministic=True)
    finally:
        M.Engine = orig
    assert not built


@pytest.mark.parametrize("projection", ["perspective", "orthographic"])
def test_vertex_adjoint_factorises_through_the_lattice(projection):
    from oracle import mvd_oracle as O
    V, S, N = 8, 16, 4
    verts = mesh("v300")[0]
    K, RT = rig(N, projection, 8 * S)
    d_vf = torch.randn(N, verts.shape[0], 16, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    two, _ = vertex_adjoint_two_stage64(d_vf, verts, K, RT, V, S, projection)
    one = vertex_adjoint_composite64(d_vf, verts, K, RT, V, S, projection)
    assert two.abs().max() > 0 and (two == 0).any(), "the case must reach some pixels and leave some untouched"
    assert rel_l2(two, one) <= 1e-12
    # autograd through the oracle's two gathers (fp32)
    pts = O.lattice(V, VOL_LEN)
    for n in range(N):
        f = torch.zeros(1, 16, S, S, requires_grad=True)
        uv = O.warp_coordinates(pts, S, 8 * S, K[n:n + 1], RT[n:n + 1], projection)
        vol = O.sample_zeros_align(f, uv).reshape(1, -1, V, V, V)
        vf = O.sample_zeros_align(vol, verts[None] / VOL_LEN)  # [1,16,Nv]
        vf.backward(d_vf[n].t()[None].float())
        assert rel_l2(f.grad[0].permute(1, 2, 0), two[n]) <= 2e-5


@pytest.mark.parametrize("projection", ["perspective", "orthographic"])
def test_frustum_and_latent_restatements_match_oracle_autograd(projection):
    from oracle import mvd_oracle as O
    from morphablediffusion_amd.spec import VolumeConfig
    V, D, S, N = 8, 5, 6, 2
    vcfg = VolumeConfig(num_views=N, projection=projection, input_image_size=8 * S, frustum_volume_depth=D, spatial_volume_size=V)
    K, RT = rig(N, projection, 8 * S, near=True)
    g = torch.Generator().manual_seed(5)
    d_out = torch.randn(N, D, S, S, 64, generator=g, dtype=torch.float64)
    want, outside = frustum_adjoint64(d_out, K, RT, V, projection)
    assert 0.05 <= outside <= 0.60, outside
    vol = torch.zeros(N, 64, V, V, V, requires_grad=True)
    xyz = O.frustum_points(vcfg, RT, K) / VOL_LEN
    feats = O.sample_zeros_align(vol, xyz.reshape(N, 3, -1).transpose(1, 2))  # [N,64,P]
    feats.backward(d_out.reshape(N, -1, 64).transpose(1, 2).float())
    assert rel_l2(vol.grad.sum(0).permute(1, 2, 3, 0), want) <= 2e-5
    # latent
    verts, coord, out_sh, bounds = mesh("off-centre")
    grid, n_rows = rulebook_grid(coord, out_sh)
    d_vol = torch.randn(V, V, V, 64, generator=g, dtype=torch.float64)
    rows = latent_adjoint64(d_vol, grid, n_rows, bounds[0], out_sh)
    fv = torch.zeros(1, 64, *grid.shape, requires_grad=True)
    O.latent_volume(vcfg, fv, bounds[0], out_sh).backward(d_vol.permute(3, 0, 1, 2)[None].float())
    dense = fv.grad[0].reshape(64, -1).t()
    cells = grid.reshape(-1)
    assert rows.abs().max() > 0
    assert rel_l2(dense[cells >= 0], rows[cells[cells >= 0]]) <= 2e-5

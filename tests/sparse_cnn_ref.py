"""Plain reference of the conditioner's sparse voxel CNN layers (SubMConv3d / SparseConv3d(k3, s2, p1) + BatchNorm1d + ReLU,
network.py:74-161), written from the voxel coordinates and independent of the engine's rule book -- for tests/test_sparse_cnn_cpu.py
and tests/test_gpu_sparse_cnn_ops.py.

Voxel -> row dictionaries keep the FIRST row of a voxel as its representative; every lookup, the centre tap included, goes through
them.  From the dictionaries come 27 index vectors per layer (tap k = (kd*3 + kh)*3 + kw: input voxel s + (kd, kh, kw) - 1 for a
submanifold layer, 2 o - 1 + (kd, kh, kw) for the stride-2 layer, whose output sites are sorted z, y, x), and the layer is
sum_k in_pad[idx_k] @ W[k] in torch, so autograd gives d_in and dW.  A duplicate row's input is never read (its d_in is 0), the
representative receives the gradients of all rows of its voxel: the duplicate semantics fall out of the definition.
Every function takes a dtype: float64 is the reference, the same code in float32 gives the error an fp32 evaluation makes (the
tolerances of the GPU tests are multiples of it)."""
import functools
import itertools

import torch

EPS = 1e-3        # BatchNorm1d(eps=1e-3, momentum=0.01): network.py:105
MOMENTUM = 0.01
TAPS = list(itertools.product(range(3), repeat=3))  # (kd, kh, kw) of tap k

# (name, Cin, Cout, strided, level of the input): the five layer kinds of the nine-layer stack
LAYER_KINDS = [("subm0", 16, 16, False, 0), ("down0", 16, 32, True, 0), ("subm1", 32, 32, False, 1), ("down1", 32, 64, True, 1),
               ("subm2", 64, 64, False, 2)]
KIND = {k[0]: k for k in LAYER_KINDS}
DGRAD_CHANNELS = [(32, 16), (64, 32)]  # matrix-core form only: the channel counts of the gather-form data gradient
SITE_CHANNELS = [(12, 20), (16, 48)]   # site form only: Cin % 8 != 0 (scalar branch), 256 % Cout != 0


# ---- rule book from dictionaries ------------------------------------------------------------------------------------------------
def first_rows(sites):
    idx = {}
    for i, s in enumerate(sites):
        idx.setdefault(s, i)
    return idx


def subm_index(sites):
    idx = first_rows(sites)
    return torch.tensor([[idx.get((s[0] + kd - 1, s[1] + kh - 1, s[2] + kw - 1), -1) for kd, kh, kw in TAPS] for s in sites],
                        dtype=torch.long).reshape(-1, 27)


def strided_sites(sites, shape):
    """output sites of SparseConv3d(k3, s2, p1): o is active iff an active input lies in 2o - 1 .. 2o + 1; extent (D - 1) // 2 + 1"""
    oshape = tuple((v - 1) // 2 + 1 for v in shape)
    outs = set()
    for s in set(sites):
        per_axis = [[o for o in {v // 2, (v + 1) // 2} if 0 <= o < oshape[a]] for a, v in enumerate(s)]
        outs.update(itertools.product(*per_axis))
    return sorted(outs), oshape


def strided_index(sites, osites):
    idx = first_rows(sites)
    return torch.tensor([[idx.get((2 * o[0] - 1 + kd, 2 * o[1] - 1 + kh, 2 * o[2] - 1 + kw), -1) for kd, kh, kw in TAPS] for o in osites],
                        dtype=torch.long).reshape(-1, 27)


class PointSet:
    def __init__(self, name, sites, shape):
        self.name, self.shape = name, tuple(shape)
        self.sites = [list(map(tuple, sites))]       # per level; level 0 may hold a voxel several times
        self.shapes = [self.shape]
        self.subm, self.down = [], []
        for lvl in range(3):
            self.subm.append(subm_index(self.sites[lvl]))
            if lvl == 2:
                break
            osites, oshape = strided_sites(self.sites[lvl], self.shapes[lvl])
            self.down.append(strided_index(self.sites[lvl], osites))
            self.sites.append(osites)
            self.shapes.append(oshape)
        self.n = [len(s) for s in self.sites]
        idx = first_rows(self.sites[0])
        self.rep = torch.tensor([idx[s] for s in self.sites[0]])  # representative row of every level-0 row
        self.dup_rows = (self.rep != torch.arange(self.n[0])).nonzero().flatten()

    def coords(self, lvl=0):
        return torch.tensor(self.sites[lvl], dtype=torch.long).reshape(-1, 3)

    def table(self, kind):
        """(index [n_out, 27], n_in) of a layer kind"""
        _, _, _, strided, lvl = KIND[kind]
        return (self.down[lvl] if strided else self.subm[lvl]), self.n[lvl]

    def border_row(self):
        """a representative row on a face of the level-0 grid"""
        for i, s in enumerate(self.sites[0]):
            if int(self.rep[i]) == i and any(v == 0 or v == e - 1 for v, e in zip(s, self.shape)):
                return i
        raise AssertionError("no border site")


def _random_sites(seed, shape, count=None, occupancy=None):
    g = torch.Generator().manual_seed(seed)
    cells = list(itertools.product(*[range(v) for v in shape]))
    perm = torch.randperm(len(cells), generator=g).tolist()  # random row order: the tables are no identity-like pattern
    count = int(round(occupancy * len(cells))) if count is None else count
    return [cells[i] for i in perm[:count]], g


BLOB_SEED, BLOB_DUPS = 3, 37


@functools.lru_cache(maxsize=None)
def point_set(name):
    if name == "blob":  # ~30 % of an odd-extent grid, 37 duplicate rows behind their representatives, most of them mid-array
        sites, g = _random_sites(BLOB_SEED, (11, 9, 13), occupancy=0.30)
        n = len(sites)
        reps = torch.randperm(n // 3, generator=g)[:BLOB_DUPS].tolist()
        rows = list(sites)
        for j, r in enumerate(reps):  # positions counted in the growing list: always behind row r (< n / 3)
            pos = len(rows) if j >= BLOB_DUPS - 4 else n // 2 + (j * 5) % (n // 3)
            rows.insert(pos, sites[r])
        return PointSet(name, rows, (11, 9, 13))
    if name == "tiny":  # 5 sites, the last with no active neighbour
        return PointSet(name, [(0, 0, 0), (0, 0, 1), (1, 1, 1), (0, 1, 0), (2, 2, 3)], (3, 3, 4))
    if name == "full16":  # one full weight-gradient chunk, sixteen full 16-site tiles
        return PointSet(name, _random_sites(5, (8, 8, 8), count=256)[0], (8, 8, 8))
    if name == "plus1":
        return PointSet(name, _random_sites(6, (8, 8, 8), count=257)[0], (8, 8, 8))
    raise KeyError(name)


POINT_SETS = ["blob", "tiny", "full16", "plus1"]


# ---- weights --------------------------------------------------------------------------------------------------------------------
def to_layout(w5, layout):
    """w5 [Cout, Cin, 3, 3, 3] (layout 0) -> checkpoint layout 1 [Cout, 3, 3, 3, Cin] or 2 [3, 3, 3, Cin, Cout]"""
    return (w5, w5.permute(0, 2, 3, 4, 1), w5.permute(2, 3, 4, 1, 0))[layout].contiguous()


def w27(w5):
    """[27][Cin][Cout]"""
    return w5.reshape(w5.shape[0], w5.shape[1], 27).permute(2, 1, 0)


def exact_weight(cout, cin, p=7):
    """asymmetric, never zero, exact in fp32 (multiples of 1/8): a moved tap or a transposed fragment cannot cancel"""
    n = cout * cin * 27
    return ((torch.arange(n, dtype=torch.float32) % p) - (p // 2)).reshape(cout, cin, 3, 3, 3) / 4 + 0.125


# ---- the layers -----------------------------------------------------------------------------------------------------------------
def conv(x, idx, w5, dtype=torch.float64):
    """x [n_in, Cin], idx [n_out, 27] (-1: no input), w5 [Cout, Cin, 3, 3, 3] -> [n_out, Cout]; differentiable in x and w5"""
    x, w = x.to(dtype), w27(w5.to(dtype))
    xp = torch.cat([x, torch.zeros(1, x.shape[1], dtype=dtype)])
    idx = torch.where(idx < 0, torch.full_like(idx, x.shape[0]), idx)
    out = torch.zeros(idx.shape[0], w.shape[2], dtype=dtype)
    for k in range(27):
        out = out + xp[idx[:, k]] @ w[k]
    return out


def conv_grads(x, idx, w5, d_out, dtype=torch.float64):
    """(d_in [n_in, Cin], dW [Cout, Cin, 3, 3, 3]) of conv by autograd"""
    xx, ww = x.to(dtype).requires_grad_(True), w5.to(dtype).requires_grad_(True)
    conv(xx, idx, ww, dtype).backward(d_out.to(dtype))
    return xx.grad, ww.grad


def fold_epilogue(y, scale, shift, dtype=torch.float64):
    return torch.relu(y.to(dtype) * scale.to(dtype) + shift.to(dtype))


def bn_pre(x, gamma, beta, dtype=torch.float64, eps=EPS):
    """(pre-activation g * xhat + b, mean, biased variance, rstd)"""
    x, g, b = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.sum(0) / x.shape[0]
    var = ((x - mean) ** 2).sum(0) / x.shape[0]
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * g + b, mean, var, rstd


def bn_relu(x, gamma, beta, dtype=torch.float64, running=None, momentum=MOMENTUM, eps=EPS):
    """train-mode BatchNorm1d + ReLU written out (nn.BatchNorm1d refuses n = 1): (y, stats [2, C] = [mean | rstd], (running mean,
    running var) after the update or None)"""
    pre, mean, var, rstd = bn_pre(x, gamma, beta, dtype, eps)
    n = x.shape[0]
    run = None
    if running is not None:
        run = ((1 - momentum) * running[0].to(dtype) + momentum * mean,
               (1 - momentum) * running[1].to(dtype) + momentum * var * (n / max(n - 1, 1)))
    return torch.relu(pre), torch.stack([mean, rstd]), run


def bn_relu_grads(x, gamma, beta, dy, dtype=torch.float64):
    """(d x, dgamma, dbeta) of bn_relu by autograd"""
    xx, gg, bb = (t.to(dtype).requires_grad_(True) for t in (x, gamma, beta))
    bn_relu(xx, gg, bb, dtype)[0].backward(dy.to(dtype))
    return xx.grad, gg.grad, bb.grad


def mask_near_ties(x, gamma, beta, dy, tol=1e-4):
    """dy with zeros wherever the fp64 pre-activation is within tol of the ReLU's kink (an fp32 mask may differ there); the
    fraction of elements zeroed"""
    near = bn_pre(x, gamma, beta)[0].abs() < tol
    return torch.where(near, torch.zeros_like(dy), dy), near.double().mean().item()


# ---- test data ------------------------------------------------------------------------------------------------------------------
BN_FWD_CASES = [(1, 16, 0), (2, 32, 1), (255, 64, 0), (256, 16, 1), (257, 32, 0), (6144, 64, 1), (6145, 16, 0), (12288, 32, 1),
                (12289, 64, 0), (12288, 16, 1), (6144, 32, 0), (255, 16, 1)]  # (n, C, offset: 1 = 50 + 0.1 randn)
BN_BWD_CASES = [(1, 16), (127, 32), (128, 64), (129, 16), (300, 32), (6145, 64), (128, 16), (300, 64), (1, 64)]


def bn_data(n, C, offset=0, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + C)
    x = 50 + 0.1 * torch.randn(n, C, generator=g) if offset else torch.randn(n, C, generator=g) * 1.3 + 0.2
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    rmean, rvar = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
    dy = torch.randn(n, C, generator=g)
    return x, gamma, beta, rmean, rvar, dy


def conv_data(ps, kind=None, cin=None, cout=None, seed=0):
    """(idx, x [n_in, Cin], w5, d_out [n_out, Cout], scale, shift) of a layer kind -- or of other channel counts on the level-0
    submanifold table"""
    if kind is not None:
        _, cin, cout, _, _ = KIND[kind]
        idx, n_in = ps.table(kind)
    else:
        idx, n_in = ps.table("subm0")
    g = torch.Generator().manual_seed(seed + 131 * cin + cout + 17 * n_in)
    x = torch.randn(n_in, cin, generator=g)
    w5 = torch.randn(cout, cin, 3, 3, 3, generator=g) * (27 * cin) ** -0.5
    d_out = torch.randn(idx.shape[0], cout, generator=g)
    scale, shift = torch.randn(cout, generator=g) * 0.3 + 1.0, torch.randn(cout, generator=g) * 0.3
    return idx, x, w5, d_out, scale, shift


def errs(got, want):
    """(relative L2, max |error| / max |reference|) against a float64 reference"""
    d = got.detach().cpu().double() - want
    return (d.norm() / (want.norm() + 1e-300)).item(), (d.abs().max() / (want.abs().max() + 1e-300)).item()

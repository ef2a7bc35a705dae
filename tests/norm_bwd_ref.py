"""Plain closed forms of the training backward's norms and row reductions (csrc/k_bwd.hip), evaluated in the dtype asked for: float64
is the reference of tests/test_gpu_norm_bwd_ops.py, float32 gives the error a float32 evaluation has anyway (its bound).  No autograd
in here; tests/test_norm_bwd_cpu.py holds the float64 forms against torch.autograd.  Also the launch plans restated (bwd_gn_slabs,
the LayerNorm block count), the shape tables of the two test files, and their seeded inputs.

Layouts: x, dy, dx [B, rows, C] channels-last (LayerNorm: [rows, C]); pre, dpre [B, C]; act 0 none, 1 SiLU, 2 ReLU."""
import functools

import torch

ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2


def act_f(u, act):
    return u * torch.sigmoid(u) if act == ACT_SILU else (torch.clamp(u, min=0) if act == ACT_RELU else u)


def act_d(u, act):
    if act == ACT_SILU:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    return (u > 0).to(u.dtype) if act == ACT_RELU else torch.ones_like(u)


def _gn_stats(x, pre, G, eps):
    """two-pass mean and rstd per (sample, group) of v = x + pre -> v grouped [B, rows, G, cpg], xhat alike"""
    B, rows, C = x.shape
    v = x if pre is None else x + pre[:, None, :]
    v = v.reshape(B, rows, G, C // G)
    mean = v.sum(dim=(1, 3), keepdim=True) / (rows * (C // G))
    d = v - mean
    var = (d * d).sum(dim=(1, 3), keepdim=True) / (rows * (C // G))
    return d * torch.rsqrt(var + eps), torch.rsqrt(var + eps)


def gn_forward(x, pre, gamma, beta, G, eps, act, dtype):
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    xh, _ = _gn_stats(x, None if pre is None else pre.to(dtype), G, eps)
    return act_f(xh.reshape(x.shape) * gamma + beta, act)


def gn_backward(x, pre, dy, gamma, beta, G, eps, act, dtype):
    """-> {dx, dgamma, dbeta, dpre}: du = dy act'(u), dxhat = du gamma, dx = rstd (dxhat - mean_g(dxhat) - xhat mean_g(dxhat xhat))"""
    x, dy, gamma, beta = x.to(dtype), dy.to(dtype), gamma.to(dtype), beta.to(dtype)
    B, rows, C = x.shape
    xh4, rstd = _gn_stats(x, None if pre is None else pre.to(dtype), G, eps)
    xh = xh4.reshape(x.shape)
    du = dy * act_d(xh * gamma + beta, act)
    dxh = (du * gamma).reshape(xh4.shape)
    n = rows * (C // G)
    m1 = dxh.sum(dim=(1, 3), keepdim=True) / n
    m2 = (dxh * xh4).sum(dim=(1, 3), keepdim=True) / n
    dx = (rstd * (dxh - m1 - xh4 * m2)).reshape(x.shape)
    return {"dx": dx, "dgamma": (du * xh).sum(dim=(0, 1)), "dbeta": du.sum(dim=(0, 1)), "dpre": dx.sum(dim=1)}


def ln_backward(x, dy, gamma, eps, dtype):
    x, dy, gamma = x.to(dtype), dy.to(dtype), gamma.to(dtype)
    C = x.shape[1]
    d = x - x.sum(dim=1, keepdim=True) / C
    rstd = torch.rsqrt((d * d).sum(dim=1, keepdim=True) / C + eps)
    xh, dxh = d * rstd, dy * gamma
    m1, m2 = dxh.sum(dim=1, keepdim=True) / C, (dxh * xh).sum(dim=1, keepdim=True) / C
    return {"dx": rstd * (dxh - m1 - xh * m2), "dgamma": (dy * xh).sum(dim=0), "dbeta": dy.sum(dim=0)}


def colsum(v, B, dtype):
    """v [B * rows, C] -> [B, C]"""
    return v.to(dtype).reshape(B, -1, v.shape[1]).sum(dim=1)


def sum_rows(part, dtype):
    return part.to(dtype).sum(dim=0)


def outer(a, b, dtype):
    """a [K, M], b [K, N] -> [M, N] = sum_k a[k] (x) b[k]"""
    return a.to(dtype).t() @ b.to(dtype)


def added(start, term, dtype):
    """What an accumulating kernel adds to `start`, as that dtype sees it: (start + term) - start, the difference taken exactly."""
    return (start.to(dtype) + term.to(dtype)).double() - start.double()


def errs(got, want):
    """(relative L2, max |error| / max |reference|) against a float64 reference"""
    d = got.detach().cpu().double() - want
    return (d.norm() / (want.norm() + 1e-300)).item(), (d.abs().max() / (want.abs().max() + 1e-300)).item()


# ---- launch plans, restated from csrc/k_bwd.hip ------------------------------------------------------------------------------------
def gn_slabs(B, G, rows):
    """bwd_gn_slabs: about 1024 workgroups, at least 8 rows per slab, at most 64 slabs"""
    return max(1, min(1024 // (B * G), rows // 8, 64))


def gn_empty_slabs(rows, S):
    """slabs of the plan that hold no row (rows per slab = ceil(rows / S))"""
    rps = -(-rows // S)
    return sum(1 for k in range(S) if k * rps >= rows)


def gn_row_lanes(C, G):
    return 256 // (C // G)


def ln_blocks(rows):
    return min(256, -(-rows // 4))


# ---- shape tables -----------------------------------------------------------------------------------------------------------------
# GroupNorm: name -> B, rows, C, G, act, eps and the form of the launch.  strided: ld = C + 8 with x at column 3 of a wider buffer,
# ldy = C, lddx = C + 24.  accum: dx, dgamma, dbeta start from random values.  pre: "enc" = the view encoder's FiLM rows (pre at
# column 16 i of [B][48], dpre into [B][48]), "dense" = the frustum nets' [B][C].  S_force 0 = the plan.
def _gn(B, rows, C, G, act, eps=1e-5, strided=False, accum=False, pre=None, S_force=0, poison=False, fwd=False):
    return dict(B=B, rows=rows, C=C, G=G, act=act, eps=eps, strided=strided, accum=accum, pre=pre, S_force=S_force, poison=poison, fwd=fwd)


GN_CASES = {
    "enc_1024":      _gn(3, 1024, 16, 8, ACT_SILU, pre="enc", poison=True),                 # 2 channels per group, 128 row lanes
    "enc_100":       _gn(1, 100, 16, 8, ACT_SILU, pre="enc", accum=True),                   # rows below the row-lane count
    "c64_empty":     _gn(1, 520, 64, 8, ACT_RELU, poison=True, fwd=True),                   # S = 64, rps = 9: slabs 58..63 empty
    "c128_frustum":  _gn(3, 1024, 128, 8, ACT_SILU, strided=True, accum=True, pre="dense", poison=True),
    "c320_17":       _gn(3, 17, 320, 32, ACT_SILU, strided=True, fwd=True),
    "c320_norm":     _gn(1, 1024, 320, 32, ACT_NONE, eps=1e-6, strided=True, accum=True, fwd=True),   # the transformer's norm
    "c960_16":       _gn(3, 16, 960, 32, ACT_SILU),
    "c2560_7":       _gn(1, 7, 2560, 32, ACT_SILU, poison=True, fwd=True),                  # S = 1 by plan
    "c2048_100":     _gn(1, 100, 2048, 8, ACT_RELU, eps=1e-6, fwd=True),                    # 256 channels per group: one row lane
    "c64_1":         _gn(3, 1, 64, 8, ACT_SILU, accum=True, fwd=True),
    "c64_force1":    _gn(1, 1024, 64, 8, ACT_RELU, S_force=1),
    "c320_force2":   _gn(3, 100, 320, 32, ACT_NONE, S_force=2, strided=True),
    "c128_force64":  _gn(3, 100, 128, 8, ACT_SILU, S_force=64, pre="dense", poison=True, fwd=True),  # rps = 2: slabs 50..63 empty
}

# LayerNorm: rows, C, eps, strided (ld = C + 8 at column 3, ldy = C + 4, lddx = C + 24), accum, poison
LN_CASES = {
    "r1_c64":       dict(rows=1, C=64, eps=1e-5, strided=False, accum=False, poison=True),
    "r3_c100":      dict(rows=3, C=100, eps=1e-6, strided=True, accum=True, poison=False),
    "r4_c320":      dict(rows=4, C=320, eps=1e-5, strided=False, accum=True, poison=False),
    "r5_c640":      dict(rows=5, C=640, eps=1e-5, strided=True, accum=False, poison=True),
    "r1023_c1280":  dict(rows=1023, C=1280, eps=1e-5, strided=False, accum=True, poison=True),
    "r1024_c64":    dict(rows=1024, C=64, eps=1e-6, strided=True, accum=False, poison=False),
    "r1025_c100":   dict(rows=1025, C=100, eps=1e-5, strided=False, accum=True, poison=True),
    "r2051_c320":   dict(rows=2051, C=320, eps=1e-5, strided=True, accum=True, poison=False),
}
LN_REFUSED_C = 1344  # above 64 * LN_NC = 1280

COLSUM_ROWS = (1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 200)
COLSUM_C = (1, 48, 63, 64, 65, 130)
# bwd_sum_rows_multi: per launch the jobs (R, C, accum); every R of (1, 31, 32, 33, 257) and C of (1, 7, 8, 9, 320) occurs, and the
# launches of more than one job hold jobs narrower than the widest (their workgroups past C return at once)
SUM_ROWS_LAUNCHES = (
    ((257, 320, 0),),
    ((31, 8, 1), (32, 9, 0)),
    ((33, 320, 1), (1, 1, 0), (257, 7, 1)),
    ((32, 7, 0), (33, 1, 1), (1, 320, 0), (31, 9, 1)),
)
OUTER_SHAPES = ((5, 7, 1), (320, 64, 3), (1280, 320, 2))
FAMILIES = ("centred", "offset")
RELU_MARGIN = 1e-3


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------
def _seed(name, family):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 2 + FAMILIES.index(family)


@functools.lru_cache(maxsize=None)
def gn_inputs(name, family):
    """-> dict(x, pre, dy, gamma, beta, dx0, dg0, db0), float32.  centred: x ~ 1.3 N(0,1) + 0.2 (the draw of tests/test_gpu_train_ops.py),
    pre ~ 0.3 N(0,1).  offset: x + pre ~ 0.5 N(0,1) + m with m = +-4 per (sample, group); with a pre-add, pre carries half of m.
    ReLU cases: act'(u) jumps at u = 0, where kernel and reference may legitimately land on different sides, so every element is
    kept at |u| >= RELU_MARGIN (the few closer ones are moved out by 0.02 sigma; asserted)."""
    c = GN_CASES[name]
    B, rows, C, G = c["B"], c["rows"], c["C"], c["G"]
    g = torch.Generator().manual_seed(_seed(name, family))
    dy = torch.randn(B, rows, C, generator=g)
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    if family == "centred":
        x, sigma = torch.randn(B, rows, C, generator=g) * 1.3 + 0.2, 1.3
        pre = torch.randn(B, C, generator=g) * 0.3 if c["pre"] else None
    else:
        m = (torch.randint(0, 2, (B, G), generator=g).float() * 8 - 4).repeat_interleave(C // G, dim=1)
        x, sigma = torch.randn(B, rows, C, generator=g) * 0.5, 0.5
        pre = m / 2 if c["pre"] else None
        x = x + (m / 2 if c["pre"] else m)[:, None, :]
    if c["act"] == ACT_RELU:
        for _ in range(4):
            xh, _ = _gn_stats(x.double(), None if pre is None else pre.double(), G, c["eps"])
            u = xh.reshape(x.shape) * gamma.double() + beta.double()
            close = u.abs() < RELU_MARGIN
            if not close.any():
                break
            x = torch.where(close, x + 0.02 * sigma * torch.sign(gamma)[None, None, :], x)
        assert not close.any(), f"{name} {family}: pre-activations within {RELU_MARGIN} of ReLU's kink"
    return dict(x=x, pre=pre, dy=dy, gamma=gamma, beta=beta, dx0=torch.randn(B, rows, C, generator=g), dg0=torch.randn(C, generator=g) * 3,
                db0=torch.randn(C, generator=g) * 3)


@functools.lru_cache(maxsize=None)
def ln_inputs(name, family):
    """centred: x ~ 2 N(0,1) - 0.5 (the draw of tests/test_gpu_train_ops.py); offset: x ~ 0.5 N(0,1) + m with m = +-4 per row"""
    c = LN_CASES[name]
    rows, C = c["rows"], c["C"]
    g = torch.Generator().manual_seed(_seed(name, family))
    dy = torch.randn(rows, C, generator=g)
    gamma = torch.randn(C, generator=g) * 0.3 + 1.0
    if family == "centred":
        x = torch.randn(rows, C, generator=g) * 2.0 - 0.5
    else:
        x = torch.randn(rows, C, generator=g) * 0.5 + (torch.randint(0, 2, (rows, 1), generator=g).float() * 8 - 4)
    return dict(x=x, dy=dy, gamma=gamma, dx0=torch.randn(rows, C, generator=g), dg0=torch.randn(C, generator=g) * 3,
                db0=torch.randn(C, generator=g) * 3)


@functools.lru_cache(maxsize=None)
def gn_reference(name, family, dtype):
    """the compared tensors of a GroupNorm backward case as that dtype gives them; accumulating results as what is added to the
    preset (dgamma / dbeta are always added to: zeros where the case does not preset them)"""
    c, d = GN_CASES[name], gn_inputs(name, family)
    r = gn_backward(d["x"], d["pre"], d["dy"], d["gamma"], d["beta"], c["G"], c["eps"], c["act"], dtype)
    if c["accum"]:
        r = dict(r, dx=added(d["dx0"], r["dx"], dtype), dgamma=added(d["dg0"], r["dgamma"], dtype), dbeta=added(d["db0"], r["dbeta"], dtype))
    if not c["pre"]:
        del r["dpre"]
    return r


@functools.lru_cache(maxsize=None)
def ln_reference(name, family, dtype):
    c, d = LN_CASES[name], ln_inputs(name, family)
    r = ln_backward(d["x"], d["dy"], d["gamma"], c["eps"], dtype)
    if c["accum"]:
        r = dict(r, dx=added(d["dx0"], r["dx"], dtype), dgamma=added(d["dg0"], r["dgamma"], dtype), dbeta=added(d["db0"], r["dbeta"], dtype))
    return r


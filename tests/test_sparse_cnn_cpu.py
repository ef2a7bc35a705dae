"""CPU: the reference of the sparse voxel CNN's layers (tests/sparse_cnn_ref.py) against the engine's rule book, the oracle's
layers and the hash-map restatement of tests/test_oracle_golden.py -- and the conditions the generated cases of
tests/test_gpu_sparse_cnn_ops.py have to meet (which tile and chunk edges they reach)."""
import ctypes as C

import pytest
import torch

from oracle import mvd_oracle as O
from tests import sparse_cnn_ref as R
from tests.test_oracle_golden import _hashmap_sparse_conv


def engine_tables(ps):
    """(n_sites [3], the five tables of mvd_rulebook_build: submanifold levels 0..2, strided 0 -> 1 and 1 -> 2)"""
    from morphablediffusion_amd import lib as L
    lib = L.load()
    coord = ps.coords(0).to(torch.int32).contiguous()
    out_sh = torch.tensor(ps.shape, dtype=torch.int32)
    n_sites, lens = (C.c_int32 * 3)(), (C.c_int64 * 6)()
    L.check(lib.mvd_rulebook_build(L.ptr(coord), L.ptr(out_sh), coord.shape[0], 0, n_sites, lens))
    tabs = []
    for w in range(5):
        t = torch.empty(max(int(lens[w]), 1), dtype=torch.int32)
        L.check(lib.mvd_rulebook_table(w, L.ptr(t)))
        tabs.append(t[:int(lens[w])].view(-1, 27))
    return list(n_sites), tabs


@pytest.mark.parametrize("name", R.POINT_SETS)
def test_reference_index_vectors_equal_the_engine_rule_book(name):
    """The GPU tests feed the kernels the production tables: they are the reference's index vectors, level by level."""
    ps = R.point_set(name)
    n_sites, tabs = engine_tables(ps)
    assert n_sites == ps.n
    for lvl in range(3):
        assert torch.equal(tabs[lvl].long(), ps.subm[lvl]), f"submanifold table of level {lvl}"
    for lvl in range(2):
        assert torch.equal(tabs[3 + lvl].long(), ps.down[lvl]), f"strided table {lvl} -> {lvl + 1}"


@pytest.mark.parametrize("name", R.POINT_SETS)
def test_reference_layer_equals_oracle_and_hash_map_restatement(name):
    """Three derivations of one layer: the reference's dictionaries, the oracle's index grid, spconv's pair lists.  The oracle and
    the restatement take one row per voxel; the reference's duplicate rows must repeat their representatives' outputs."""
    ps = R.point_set(name)
    keep = (ps.rep == torch.arange(ps.n[0])).nonzero().flatten()  # first occurrences, in row order
    for kind, cin, cout, strided, lvl in R.LAYER_KINDS:
        idx, x, w5, _, _, _ = R.conv_data(ps, kind)
        want = R.conv(x, idx, w5)
        if lvl == 0:
            feats, coords = x[keep], ps.coords(0)[keep]
        else:
            feats, coords = x, ps.coords(lvl)
        if strided:
            got_o, oc, osh = O._strided_conv(feats, coords, list(ps.shapes[lvl]), w5)
            got_h, hc, hsh = _hashmap_sparse_conv(feats, coords, list(ps.shapes[lvl]), w5, 2)
            assert torch.equal(oc, ps.coords(lvl + 1)) and torch.equal(hc, ps.coords(lvl + 1))
            assert tuple(osh) == ps.shapes[lvl + 1] == tuple(hsh)
            ref = want
        else:
            got_o = O._subm_conv(feats, coords, list(ps.shapes[lvl]), w5)
            got_h = _hashmap_sparse_conv(feats, coords, list(ps.shapes[lvl]), w5, 1)[0]
            ref = want[keep] if lvl == 0 else want
            if lvl == 0:
                assert torch.equal(want, want[ps.rep]), "a duplicate row computes what its representative computes"
        assert R.errs(got_o, ref)[1] <= 1e-5, kind   # the oracle computes in fp32
        assert R.errs(got_h, ref)[1] <= 1e-6, kind   # fp64, rounded to fp32 on return


def test_duplicate_rows_receive_no_gradient_and_their_representatives_all_of_it():
    ps = R.point_set("blob")
    idx, x, w5, d_out, _, _ = R.conv_data(ps, "subm0")
    d_in, dw = R.conv_grads(x, idx, w5, d_out)
    assert ps.dup_rows.numel() >= 30 and (d_in[ps.dup_rows] == 0).all()
    folded = torch.zeros_like(d_out, dtype=torch.float64).index_add_(0, ps.rep, d_out.double())  # the fold the engine does first
    d_in2, dw2 = R.conv_grads(x, idx, w5, folded)
    assert R.errs(d_in2, d_in)[1] <= 1e-12 and R.errs(dw2, dw)[1] <= 1e-12


@pytest.mark.parametrize("n,C", [(1, 16), (2, 32), (300, 64)])
def test_reference_batchnorm_equals_the_oracle(n, C):
    x, gamma, beta, rmean, rvar, _ = R.bn_data(n, C)
    p = "bn"
    W = {p + ".weight": gamma.double(), p + ".bias": beta.double(), p + ".running_mean": rmean.double(), p + ".running_var": rvar.double()}
    upd = {}
    want = O._bn_relu(W, p, x.double(), train=True, bn_update=upd)
    y, stats, run = R.bn_relu(x, gamma, beta, running=(rmean, rvar))
    assert R.errs(y, want)[1] <= 1e-12
    assert R.errs(run[0], upd[p + ".running_mean"])[1] <= 1e-12 and R.errs(run[1], upd[p + ".running_var"])[1] <= 1e-12
    assert R.errs(stats[1], 1.0 / torch.sqrt(x.double().var(0, unbiased=False) + 1e-3))[1] <= 1e-12
    if n > 1:  # nn.BatchNorm1d itself (it refuses n = 1 in train mode)
        bn = torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).double().train()
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rmean), bn.running_var.copy_(rvar)
        assert R.errs(y, torch.relu(bn(x.double())).detach())[1] <= 1e-12
        assert R.errs(run[1], bn.running_var)[1] <= 1e-12 and R.errs(run[0], bn.running_mean)[1] <= 1e-12


def test_weight_layouts_are_permutations_of_one_kernel():
    w5 = torch.arange(2 * 5 * 27, dtype=torch.float32).reshape(2, 5, 3, 3, 3)
    k, ci, co = 14, 3, 1
    assert R.w27(w5)[k, ci, co] == w5[co, ci, 1, 1, 2]
    assert R.to_layout(w5, 1)[co, 1, 1, 2, ci] == w5[co, ci, 1, 1, 2] and R.to_layout(w5, 2)[1, 1, 2, ci, co] == w5[co, ci, 1, 1, 2]
    assert (R.exact_weight(16, 16) != 0).all()


def test_generated_cases_reach_the_edges_they_are_meant_to():
    """The conditions of the GPU cases: row counts on both sides of the 16-site tile and the 256-site chunk, duplicates, faces."""
    counts = [R.point_set(name).table(kind[0])[0].shape[0] for name in R.POINT_SETS for kind in R.LAYER_KINDS]
    assert any(c < 16 for c in counts)
    assert any(c % 16 == 0 for c in counts)
    assert any(c > 16 and c % 16 for c in counts)
    assert any(c > 256 and c % 256 for c in counts)
    blob = R.point_set("blob")
    assert blob.dup_rows.numel() == R.BLOB_DUPS >= 30
    assert blob.n[0] > 256 and blob.n[0] % 16 and blob.n[0] % 256
    assert (blob.rep[blob.dup_rows] < blob.dup_rows).all(), "duplicates sit behind their representatives"
    mid = ((blob.dup_rows > blob.n[0] // 3) & (blob.dup_rows < blob.n[0] - 40)).sum().item()
    assert mid >= 20 and blob.dup_rows.max().item() == blob.n[0] - 1, "duplicates in the middle of the array and at its end"
    c0 = blob.coords(0)
    for a in range(3):
        assert (c0[:, a] == 0).any() and (c0[:, a] == blob.shape[a] - 1).any(), f"no site on a face of axis {a}"
    # (11, 9, 13) -> (6, 5, 7) -> (3, 3, 4): all extents odd at level 0, odd ones at every level (an odd extent's last output plane
    # reads one plane past the input grid)
    assert all(v % 2 for v in blob.shape) and all(any(v % 2 for v in sh) for sh in blob.shapes), "odd extents"
    assert blob.n[1] % 16 and blob.n[2] % 16
    tiny = R.point_set("tiny")
    assert tiny.n[0] == 5 and (tiny.subm[0][4] >= 0).sum() == 1, "the last site of tiny has no active neighbour"
    assert R.point_set("full16").n[0] == 256 and R.point_set("full16").dup_rows.numel() == 0
    assert R.point_set("plus1").n[0] == 257 and R.point_set("plus1").dup_rows.numel() == 0
    assert sorted({n for n, _, _ in R.BN_FWD_CASES}) == [1, 2, 255, 256, 257, 6144, 6145, 12288, 12289]
    assert {c for _, c, _ in R.BN_FWD_CASES} == {16, 32, 64} and sum(o for _, _, o in R.BN_FWD_CASES) * 2 == len(R.BN_FWD_CASES)
    assert sorted({n for n, _ in R.BN_BWD_CASES}) == [1, 127, 128, 129, 300, 6145] and {c for _, c in R.BN_BWD_CASES} == {16, 32, 64}


@pytest.mark.parametrize("n,C", R.BN_BWD_CASES)
def test_near_tie_mask_zeroes_at_most_one_percent(n, C):
    x, gamma, beta, _, _, dy = R.bn_data(n, C)
    masked, frac = R.mask_near_ties(x, gamma, beta, dy)
    assert frac <= 0.01
    assert (masked[masked != dy] == 0).all()
    # away from the kink the float32 evaluation draws the same mask as the float64 one
    pre64, pre32 = R.bn_pre(x, gamma, beta)[0], R.bn_pre(x, gamma, beta, torch.float32)[0]
    assert ((pre64 > 0) == (pre32 > 0))[masked != 0].all()

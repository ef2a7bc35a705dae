"""Training loss options, the parts that need no GPU: the float64 restatement against torch autograd, Min-SNR weights against the
closed form on the model's schedule, the derived foreground mask, argument errors, the C ABI of the new entry points."""
import ctypes as C

import pytest
import torch

from morphablediffusion_amd import lib as L
from morphablediffusion_amd import model as M
from morphablediffusion_amd import schedule
from morphablediffusion_amd.model import SyncMultiviewDiffusion, foreground_mask, pool_loss_mask  # noqa: F401  (new with the feature)
from morphablediffusion_amd.schedule import min_snr_weights  # noqa: F401
from tests import train_loss_ref as R

UNET = {"target": "ldm.models.diffusion.attention.DepthWiseAttention", "params": {}}
DELTA = 0.5


def _case(B=3, HW=7, C=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    target = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    target[0, 0, 0], pred[0, 0, 0] = 0.25, 0.75  # |d| == delta exactly, both signs (dyadic values: the difference is exact)
    target[0, 0, 1], pred[0, 0, 1] = 1.5, 1.0
    w = torch.rand(B, generator=g, dtype=torch.float64) + 0.25
    m = torch.rand(B, HW, generator=g, dtype=torch.float64)
    m[1] = 0.0  # one sample of area 0
    return pred, target, w, m


@pytest.mark.parametrize("loss_type", ["l2", "huber"])
@pytest.mark.parametrize("use_w", [False, True])
@pytest.mark.parametrize("use_m", [False, True])
def test_reference_gradient_is_autograd_of_its_own_loss(loss_type, use_w, use_m):
    pred, target, w, m = _case()
    assert float((pred[0, 0, 0] - target[0, 0, 0]).abs()) == DELTA
    w_, m_ = (w if use_w else None), (m if use_m else None)
    scale = 8.0
    ref = R.reference(pred, target, w_, m_, loss_type, DELTA, loss_scale=scale)
    p = pred.clone().requires_grad_(True)
    Lt = R.loss_t(p, target, w_, m_, loss_type, DELTA)
    (Lt * scale).backward()
    assert abs(float(Lt.detach()) - ref["L"]) <= 1e-12
    assert float((p.grad - ref["dpred"]).abs().max()) <= 1e-12
    # the vectorised float64 formula (what the GPU tests compare against at their sizes) is the same thing
    L64, lb, mb, dp = R.formula(pred, target, w_, m_, loss_type, DELTA, loss_scale=scale)
    assert abs(float(L64) - ref["L"]) <= 1e-12 and float((dp - ref["dpred"]).abs().max()) <= 1e-12
    assert float((lb - ref["loss_b"]).abs().max()) <= 1e-12 and float((mb - ref["mse_b"]).abs().max()) <= 1e-12
    if use_m:  # the zero-area sample: no loss, no gradient, no NaN
        assert float(ref["loss_b"][1]) == 0.0 and float(ref["dpred"][1].abs().max()) == 0.0
        assert float(p.grad[1].abs().max()) == 0.0
    assert torch.isfinite(ref["dpred"]).all() and torch.isfinite(ref["loss_b"]).all()
    if loss_type == "l2" and not use_w and not use_m:  # everything off: the plain mean squared error
        assert abs(ref["L"] - float(((pred - target) ** 2).mean())) <= 1e-12
        assert float((ref["loss_b"] - ref["mse_b"]).abs().max()) <= 1e-12


def test_huber_is_l2_inside_the_threshold_and_linear_outside():
    assert R.rho(0.3, "huber", DELTA) == R.rho(0.3, "l2", DELTA) == (0.3 * 0.3, 0.3)
    assert R.rho(DELTA, "huber", DELTA) == (DELTA * DELTA, DELTA)  # |d| == delta: the quadratic branch
    assert R.rho(-DELTA, "huber", DELTA) == (DELTA * DELTA, -DELTA)
    assert R.rho(2.0, "huber", DELTA) == (2 * DELTA * 2.0 - DELTA * DELTA, DELTA)
    assert R.rho(-2.0, "huber", DELTA) == (2 * DELTA * 2.0 - DELTA * DELTA, -DELTA)


def test_min_snr_weights_closed_form_on_the_models_schedule():
    ac = schedule.DDIMSchedule(50, 1.0).alphas_cumprod
    gamma = 5.0
    snr = ac.double() / (1.0 - ac.double())
    assert bool((snr[1:] < snr[:-1]).all())  # monotone: one crossing
    tc = int((snr > gamma).sum())  # the first t with SNR <= gamma
    assert 0 < tc < 999 and snr[tc - 1] > gamma >= snr[tc]
    t = torch.tensor([0, 999, tc - 1, tc, tc + 1, 500])
    got = schedule.min_snr_weights(ac, t, gamma)
    assert got.dtype == torch.float32 and got.shape == t.shape
    for ti, g in zip(t.tolist(), got.tolist()):
        a = float(ac[ti].double())
        s = a / (1.0 - a)
        want = min(s, gamma) / s
        assert abs(g - want) <= 1e-7 * want, (ti, g, want)
    assert got[1] == 1.0 and got[3] == 1.0 and got[4] == 1.0 and got[2] < 1.0 and got[0] < 1.0
    allw = schedule.min_snr_weights(ac, torch.arange(1000), gamma)
    assert bool((allw <= 1.0).all()) and bool((allw > 0.0).all())
    assert bool((allw[snr <= gamma] == 1.0).all()) and bool((allw[snr > gamma] < 1.0).all())
    with pytest.raises(ValueError, match="gamma"):
        schedule.min_snr_weights(ac, t, 0.0)


def _white_batch(B=2, N=3, H=256):
    return {"target_image": torch.ones(B, N, H, H, 3)}


def test_foreground_mask_all_white_is_the_background_weight_everywhere():
    batch = _white_batch()
    batch["target_image"][:, :, ::3] = 1.0 - 2.0 / 255.0  # still background: >= the threshold
    m = M.foreground_mask(batch, torch.tensor([[0], [2]]), 32, background_weight=0.1)
    assert m.shape == (2, 1, 32, 32) and m.dtype == torch.float32
    assert bool((m == torch.tensor(0.1)).all())


def test_foreground_mask_known_square_pools_exactly():
    """A 64 x 64 non-white square at rows 100..163, columns 36..99 of the chosen view, pooled 8 x 8 -> 32 x 32: latent rows 13..19
    are fully inside, row 12 holds 4 of 8 image rows (100..103), row 20 holds 4 (160..163); columns 5..11 inside, column 4 holds 4
    of 8 (36..39), column 12 holds 4 (96..99)."""
    bw = 0.25
    batch = _white_batch()
    batch["target_image"][1, 2, 100:164, 36:100, 1] = 0.0  # ONE channel below the threshold is enough
    batch["target_image"][1, 0, :, :, :] = -1.0  # another view of the same sample: must not matter
    m = M.foreground_mask(batch, torch.tensor([[1], [2]]), 32, background_weight=bw)
    assert bool((m[0] == bw).all())
    frac = torch.zeros(32, 32, dtype=torch.float64)
    rows = {12: 0.5, 20: 0.5, **{r: 1.0 for r in range(13, 20)}}
    cols = {4: 0.5, 12: 0.5, **{c: 1.0 for c in range(5, 12)}}
    for r, fr in rows.items():
        for c, fc in cols.items():
            frac[r, c] = fr * fc
    want = (bw + (1.0 - bw) * frac).float()  # (0.25 + 0.75 k/64: exact in fp32)
    assert torch.equal(m[1, 0], want)
    assert float(m[1].sum()) == float(want.double().sum())


def test_foreground_mask_uses_target_mask_when_the_batch_has_one():
    batch = _white_batch()
    tm = torch.zeros(2, 3, 256, 256)
    tm[0, 1, :128] = 1.0
    tm[1, 0] = 0.5
    batch["target_mask"] = tm
    m = M.foreground_mask(batch, torch.tensor([[1], [0]]), 32, background_weight=0.0)
    assert bool((m[0, 0, :16] == 1.0).all()) and bool((m[0, 0, 16:] == 0.0).all())
    assert bool((m[1] == 0.5).all())
    with pytest.raises(ValueError, match="target_image"):
        M.foreground_mask({}, torch.tensor([[0]]), 32)


def test_explicit_mask_is_pooled_or_taken_as_it_is():
    g = torch.Generator().manual_seed(1)
    m = torch.rand(2, 1, 32, 32, generator=g)
    assert torch.equal(M.pool_loss_mask(m, 32), m)
    big = torch.rand(2, 1, 256, 256, generator=g)
    assert torch.equal(M.pool_loss_mask(big, 32), torch.nn.functional.avg_pool2d(big, 8))
    for bad in (torch.rand(2, 32, 32), torch.rand(2, 3, 32, 32), torch.rand(2, 1, 48, 48), torch.rand(2, 1, 32, 64)):
        with pytest.raises(ValueError, match="loss_mask"):
            M.pool_loss_mask(bad, 32)


@pytest.mark.parametrize("kw,match", [
    (dict(loss_weighting="snr"), "loss_weighting"), (dict(loss_type="l1"), "loss_type"), (dict(loss_mask="alpha"), "loss_mask"),
    (dict(loss_weighting="min_snr", snr_gamma=0.0), "snr_gamma"), (dict(loss_type="huber", huber_delta=0.0), "huber_delta"),
    (dict(loss_type="huber", huber_delta=-1.0), "huber_delta"), (dict(loss_mask="foreground", background_weight=1.5), "background_weight"),
])
def test_constructor_rejects_unknown_loss_options(kw, match):
    with pytest.raises(ValueError, match=match):
        SyncMultiviewDiffusion(unet_config=UNET, **kw)


def _bare_model(**attrs):
    """The attributes training_step's argument checks read, on an object with no engine behind it."""
    m = SyncMultiviewDiffusion.__new__(SyncMultiviewDiffusion)
    torch.nn.Module.__init__(m)
    base = dict(train_mode=False, loss_weighting=None, snr_gamma=5.0, loss_type="l2", huber_delta=1.0, loss_mask=None,
                background_weight=0.1, _device=torch.device("cpu"))
    base.update(attrs)
    for k, v in base.items():
        setattr(m, k, v)
    return m


@pytest.mark.parametrize("attrs,step_kw", [
    (dict(loss_weighting="min_snr"), {}), (dict(loss_type="huber"), {}), (dict(loss_mask="foreground"), {}),
    ({}, dict(sample_weight=torch.ones(2))), ({}, dict(loss_mask=torch.ones(2, 1, 32, 32))),
])
def test_a_loss_option_with_a_backward_pass_needs_train_mode(attrs, step_kw):
    with pytest.raises(ValueError, match="train_mode"):
        _bare_model(**attrs).training_step({}, prepared=(torch.zeros(2, 4, 4, 32, 32), None, None), backward=True, **step_kw)


def test_options_changed_later_are_checked_at_the_step():
    m = _bare_model(train_mode=True)
    m.loss_type = "l1"
    with pytest.raises(ValueError, match="loss_type"):
        m.training_step({}, prepared=(torch.zeros(2, 4, 4, 32, 32), None, None))


def test_engine_wrappers_reject_an_unknown_loss_type_before_any_call():
    from morphablediffusion_amd import engine as E
    assert E.LOSS_TYPES == ("l2", "huber")
    with pytest.raises(ValueError, match="loss_type"):
        E.op_train_loss(torch.zeros(1, 1, 4), torch.zeros(1, 1, 4), loss_type="l1")


P, F, I = C.c_void_p, C.c_float, C.c_int
NEW = {
    "mvd_train_unet_step_ex": [P] * 4 + [I] + [P] * 4 + [I, P, F, I, P, P, I, F] + [P] * 9,
    "mvd_op_train_loss": [P, P, I, I, I, P, P, I, F, F, P, P, P, P, P],
}


def test_new_entry_points_parse_out_of_the_header_and_resolve_in_the_library():
    for name, argtypes in NEW.items():
        assert name in L.PROTOTYPES, name
        restype, args = L.PROTOTYPES[name]
        assert restype is C.c_int and args == argtypes, (name, args)
    old, ex = L.PROTOTYPES["mvd_train_unet_step"][1], L.PROTOTYPES["mvd_train_unet_step_ex"][1]
    assert len(ex) == len(old) + 6  # sample_w, pixel_w, loss_type, huber_delta, loss_per_sample, mse_per_sample
    assert L.PROTOTYPES["mvd_train_unet_step"][1] == [P] * 4 + [I] + [P] * 4 + [I, P, F, I] + [P] * 7  # the old entry: as it was
    lib = L.load()  # raises when a declared symbol is missing
    for name in NEW:
        assert getattr(lib, name).argtypes == NEW[name]

"""GPU: the training loss options -- the fused loss stage (csrc/k_loss.hip) through its hook mvd_op_train_loss against the float64
restatement tests/train_loss_ref.py, mvd_train_unet_step_ex on the small model, the model-level options (Min-SNR, foreground mask,
LoRA and the deterministic mode on top of them) and the held-out loss.

Bound ("the op bound"), for every quantity: normalised max error against float64 e <= 8 e_ref32 + 2e-6, e_ref32 being the error of
the same formula evaluated by torch on the CPU in fp32 on the same inputs (the bound of tests/test_gpu_lora_ops.py).  Each check
prints both numbers before it asserts.

Models: one module-scoped small training model serves every test but two -- an inference model (train_mode cannot be changed on
a built engine) and a use_ema model (its own EMA arena), each built once in the one test that needs it."""
import numpy as np
import pytest
import torch

from morphablediffusion_amd import lib as L
from morphablediffusion_amd.engine import LOSS_TYPES, op_train_loss
from morphablediffusion_amd.schedule import min_snr_weights
from morphablediffusion_amd.spec import VolumeConfig
from tests import golden_inputs as gi
from tests import train_loss_ref as R
from tests.test_gpu_train import _inputs, make_train_model

pytestmark = pytest.mark.gpu

DELTA = 0.5
CASES = [(1, 1, 4), (3, 63, 4), (2, 1024, 4), (2, 4096, 4), (3, 100, 5)]
NAMES = ("L", "loss_b", "mse_b", "dpred")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(tag, got, want64, ref32, names=NAMES):
    """The op bound for the tuples (L, loss_b, mse_b[, dpred]) or the leading part of them; returns the failures."""
    fails = []
    for name, g, w, r in zip(names, got, want64, ref32):
        g = torch.as_tensor(g)
        assert torch.isfinite(g).all(), f"{tag} {name}: an output element was not written (or is not finite)"
        e, e_ref = R.nerr(g, w), R.nerr(r, w)
        print(f"[train loss] {tag} {name}: kernel {e:.3e}, torch CPU fp32 e_ref32 {e_ref:.3e}, bound {R.bound(e_ref):.3e}")
        if not e <= R.bound(e_ref):
            fails.append((tag, name, e, R.bound(e_ref)))
    return fails


def _op_inputs(B, HW, C, zero_sample):
    g = torch.Generator().manual_seed(1000 + B * 131 + HW * 7 + C)
    pred, target = torch.randn(B, HW, C, generator=g), torch.randn(B, HW, C, generator=g)
    target[0, 0, 0], pred[0, 0, 0] = 0.25, 0.75  # |d| == delta exactly, both signs (dyadic values)
    target[0, 0, 1], pred[0, 0, 1] = 1.5, 1.0
    w = torch.rand(B, generator=g) + 0.25
    m = torch.rand(B, HW, generator=g)
    if zero_sample is not None:
        m[zero_sample] = 0.0
    return pred, target, w, m


# ---- the op hook ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("B,HW,C", CASES)
def test_op_against_float64(B, HW, C, loss_type):
    zero = B - 1  # the sample with an all-zero mask (B == 1: the only one -- run on its own below, with a live mask for the rest)
    pred, target, w, m = _op_inputs(B, HW, C, zero if B > 1 else None)
    d = pred - target
    assert float(d[0, 0, 0]) == DELTA and float(d[0, 0, 1]) == -DELTA
    if HW * C >= 64:
        assert bool((d.abs() > DELTA).any()) and bool((d.abs() < DELTA).any())  # both branches occur
    scale = 64.0
    dev = [t.cuda() for t in (pred, target, w, m)]
    fails = []
    for use_w in (False, True):
        for use_m in (False, True):
            kw = dict(w=w if use_w else None, m=m if use_m else None, loss_type=loss_type, delta=DELTA, loss_scale=scale)
            want, ref32 = R.formula(pred, target, dtype=torch.float64, **kw), R.formula(pred, target, dtype=torch.float32, **kw)
            run = lambda: op_train_loss(dev[0], dev[1], dev[2] if use_w else None, dev[3] if use_m else None, loss_type, DELTA, scale,
                                        want_grad=True)
            got, again = run(), run()  # (every output starts as NaN: engine.op_train_loss)
            tag = f"({B},{HW},{C}) {loss_type} w={'y' if use_w else '-'} m={'y' if use_m else '-'}"
            fails += _check(tag, [t.cpu() for t in got], want, ref32)
            for a, b in zip(got, again):
                assert torch.equal(a, b), f"{tag}: two calls differ"
            if use_m and B > 1:
                assert float(got[1][zero]) == 0.0 and float(got[3][zero].abs().max()) == 0.0, f"{tag}: the zero-area sample"
                assert float(got[2][zero]) > 0.0  # its plain mean squared error is still reported
            fwd = op_train_loss(dev[0], dev[1], dev[2] if use_w else None, dev[3] if use_m else None, loss_type, DELTA, scale)
            assert len(fwd) == 3 and all(torch.equal(a, b) for a, b in zip(fwd, got[:3])), f"{tag}: forward-only differs"
    assert not fails, fails
    if B == 1:  # a batch whose only sample has no area: L = 0, zero gradient, no NaN
        got = op_train_loss(dev[0], dev[1], None, torch.zeros(B, HW, device="cuda"), loss_type, DELTA, scale, want_grad=True)
        assert float(got[0]) == 0.0 and float(got[1][0]) == 0.0 and float(got[3].abs().max()) == 0.0
        assert abs(float(got[2][0]) - float((d.double() ** 2).mean())) <= 1e-6 * float((d.double() ** 2).mean())


@pytest.mark.parametrize("B,HW,C", [(3, 63, 4), (2, 4096, 4)])
def test_op_power_of_two_weight_and_loss_scale_commute_exactly(B, HW, C):
    pred, target, w, m = [t.cuda() for t in _op_inputs(B, HW, C, None)]
    for s in (1.0, 65536.0):
        for loss_type in LOSS_TYPES:
            a = op_train_loss(pred, target, torch.full((B,), 2.0), m, loss_type, DELTA, s, want_grad=True)[3]
            b = op_train_loss(pred, target, torch.full((B,), 1.0), m, loss_type, DELTA, 2.0 * s, want_grad=True)[3]
            assert torch.equal(a, b) and float(a.abs().max()) > 0.0


def test_op_all_off_is_the_plain_mean_squared_error():
    pred, target, _, _ = _op_inputs(2, 1024, 4, None)
    loss, lps, mps = op_train_loss(pred.cuda(), target.cuda())
    want = ((pred.double() - target.double()) ** 2)
    assert abs(float(loss) - float(want.mean())) <= 2e-6 * float(want.mean())
    assert torch.equal(lps, mps) and R.nerr(mps, want.mean((1, 2))) <= 2e-6


def test_op_bad_arguments_are_errors_and_launch_nothing():
    lib = L.load()
    B, HW, C = 2, 63, 4
    pred, target, w, m = [t.cuda() for t in _op_inputs(B, HW, C, None)]
    nan = float("nan")
    outs = [torch.full((B, HW, C), nan, device="cuda"), torch.full((1,), nan, device="cuda"), torch.full((B,), nan, device="cuda"),
            torch.full((B,), nan, device="cuda")]
    p = L.ptr

    def call(loss_type, delta, shape=(B, HW, C), pr=pred):
        return lib.mvd_op_train_loss(p(pr), p(target), shape[0], shape[1], shape[2], p(w), p(m), loss_type, delta, 1.0, p(outs[0]),
                                     p(outs[1]), p(outs[2]), p(outs[3]), _stream())

    for lt, delta, word in ((2, 1.0, b"loss_type"), (-1, 1.0, b"loss_type"), (1, 0.0, b"huber_delta"), (1, -0.5, b"huber_delta"),
                            (1, nan, b"huber_delta")):
        assert call(lt, delta) != 0
        assert word in lib.mvd_last_error(), lib.mvd_last_error()
    assert call(0, 1.0, shape=(0, HW, C)) != 0 and call(0, 1.0, shape=(B, 0, C)) != 0 and call(0, 1.0, shape=(B, HW, 0)) != 0
    assert call(0, 1.0, pr=None) != 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs), "an output was written by a call that reported an error"
    assert call(0, 0.0) == 0 and call(1, DELTA) == 0  # (l2 ignores huber_delta) -- and the same buffers are fine
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in outs)


# ---- the step ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """One small deterministic training model for the module, the golden training batch, and the arguments training_step hands
    to Engine.train_unet_step for it (recorded from one step)."""
    g, dev, prepared, draws = _inputs()
    N = int(g["N"])
    ucfg, vcfg = gi.SMALL_UNET, VolumeConfig(num_views=N)
    m = make_train_model(ucfg, vcfg, N, loss_scale=4096.0, recompute=True, deterministic=True)
    st = dict(dev=dev, prepared=prepared, draws=draws, cfg=(ucfg, vcfg, N), B=prepared[0].shape[0])
    eng = m.engine
    rec = {}
    orig = eng.train_unet_step

    def recording(*a, **kw):
        rec["a"], rec["kw"] = [t.clone() if torch.is_tensor(t) else {k: v.clone() for k, v in t.items()} for t in a], dict(kw)
        return orig(*a, **kw)

    eng.train_unet_step = recording
    try:
        eng.zero_grad()
        m.training_step(dev, prepared=prepared, **draws)
    finally:
        del eng.train_unet_step  # (the instance attribute: the class's method is back)
    assert set(rec["kw"]) == {"loss_scale", "recompute", "want_dsrc"}, "a default step must not pass loss options"
    st["args"] = rec["a"]
    yield m, st
    m.engine.close()


def _engine_step(m, st, loss_scale=4096.0, **kw):
    eng = m.engine
    eng.zero_grad()
    x, t, ctx, src, target = st["args"]
    out = eng.train_unet_step(x, t, ctx, {k: v.clone() for k, v in src.items()}, target, loss_scale=loss_scale, recompute=True,
                              want_dsrc=True, **kw)
    torch.cuda.synchronize()
    return out, eng.flat_grads.clone()


def _step_ref(st, pred, **kw):
    """(float64, CPU fp32) evaluations of the loss stage on the prediction the step returned."""
    target = st["args"][4]
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).cpu()
    return (R.formula(cl(pred), cl(target), dtype=torch.float64, **kw), R.formula(cl(pred), cl(target), dtype=torch.float32, **kw))


def test_step_default_path_is_untouched_and_sample_weights_reach_every_gradient(small):
    m, st = small
    B = st["B"]
    (pred_a, loss_a, dsrc_a), grads_a = _engine_step(m, st)
    # (b) sample weights (1, 0, ...): the second sample contributes nothing, anywhere
    w = torch.zeros(B)
    w[0] = 1.0
    (pred_b, loss_b, dsrc_b, lps, mps), grads_b = _engine_step(m, st, sample_weight=w, per_sample=True)
    assert torch.equal(pred_b, pred_a)
    for res_, d in dsrc_b.items():
        assert torch.isfinite(d).all()
        assert float(d[1:].abs().max()) == 0.0, f"dsrc level {res_}: a sample of weight 0 has a gradient"
        assert float(d[0].abs().max()) > 0.0, f"dsrc level {res_}: the sample of weight 1 has none"
    want, ref32 = _step_ref(st, pred_b, w=w)
    fails = _check("step w=(1,0,..)", (loss_b.cpu(), lps.cpu(), mps.cpu()), want, ref32)
    assert not fails, fails
    # (c) a pixel mask that is zero on one whole sample
    mask = torch.rand(B, 1, pred_a.shape[2], pred_a.shape[3], generator=torch.Generator().manual_seed(5)) + 0.1
    mask[2] = 0.0
    (pred_c, loss_c, dsrc_c, lps_c, mps_c), _ = _engine_step(m, st, pixel_weight=mask, loss_type="huber", huber_delta=DELTA,
                                                           per_sample=True)
    assert torch.equal(pred_c, pred_a) and float(lps_c[2]) == 0.0 and float(mps_c[2]) > 0.0
    for res_, d in dsrc_c.items():
        assert torch.isfinite(d).all()
        assert float(d[2].abs().max()) == 0.0, f"dsrc level {res_}: a sample without area has a gradient"
        assert all(float(d[b].abs().max()) > 0.0 for b in (0, 1, 3))
    want, ref32 = _step_ref(st, pred_c, m=mask.reshape(B, -1), loss_type="huber", delta=DELTA)
    fails = _check("step huber, masked", (loss_c.cpu(), lps_c.cpu(), mps_c.cpu()), want, ref32)
    assert not fails, fails
    # (a) the default call again, after the _ex path has run: bit for bit what it was before
    (pred_a2, loss_a2, dsrc_a2), grads_a2 = _engine_step(m, st)
    assert torch.equal(pred_a2, pred_a) and torch.equal(loss_a2, loss_a) and torch.equal(grads_a2, grads_a)
    assert all(torch.equal(dsrc_a2[k], dsrc_a[k]) for k in dsrc_a)
    # per_sample alone is the plain objective through the new stage: the same loss to rounding
    (pred_p, loss_p, _, lps_p, mps_p), _ = _engine_step(m, st, per_sample=True)
    assert torch.equal(pred_p, pred_a) and torch.equal(lps_p, mps_p)
    assert abs(float(loss_p) - float(loss_a)) <= 2e-6 * float(loss_a)


def test_step_weight_two_is_loss_scale_doubled_bit_for_bit(small):
    m, st = small
    B = st["B"]
    _, g2 = _engine_step(m, st, loss_scale=4096.0, sample_weight=torch.full((B,), 2.0))
    _, g1 = _engine_step(m, st, loss_scale=8192.0, sample_weight=torch.full((B,), 1.0))
    assert torch.equal(g2, g1) and float(g2.abs().max()) > 0.0 and torch.isfinite(g2).all()


def test_step_bad_arguments(small):
    m, st = small
    with pytest.raises(ValueError, match="loss_type"):
        _engine_step(m, st, loss_type="l1")
    with pytest.raises(L.MvdError, match="huber_delta"):
        _engine_step(m, st, loss_type="huber", huber_delta=0.0)
    with pytest.raises(ValueError, match="sample_weight"):
        _engine_step(m, st, sample_weight=torch.ones(st["B"] + 1))
    with pytest.raises(ValueError, match="pixel_weight"):
        _engine_step(m, st, pixel_weight=torch.ones(st["B"], 1, 16, 16))
    # the error names the entry point that was called
    eng, none9 = m.engine, [None] * 9
    assert eng.lib.mvd_train_unet_step_ex(eng._ctx, None, None, None, 1, None, None, None, None, 48, None, 1.0, 1, None, None, 0, 1.0,
                                          *none9) != 0
    assert eng.lib.mvd_last_error().startswith(b"mvd_train_unet_step_ex:")
    assert eng.lib.mvd_train_unet_step(eng._ctx, None, None, None, 1, None, None, None, None, 48, None, 1.0, 1, *[None] * 7) != 0
    assert eng.lib.mvd_last_error().startswith(b"mvd_train_unet_step:")


# ---- the model -----------------------------------------------------------------------------------------------------------------
TS = [3, 60, 400, 950]  # SNR above and below gamma = 5 (the crossing is near t = 220)


def _model_step(m, st, **kw):
    if m.train_mode:
        m.engine.zero_grad()
    draws = dict(st["draws"])
    draws["time_steps"] = torch.tensor(TS[:st["B"]])
    loss = m.training_step(kw.pop("batch", st["dev"]), prepared=st["prepared"], **draws, **kw)
    torch.cuda.synchronize()
    return loss, draws


def _host_mse(st, pred, draws):
    """(float64, fp32) per-sample mean squared error of a prediction against the injected noise of its target view."""
    B = st["B"]
    noise = draws["noise"]
    target = noise[torch.arange(B)[:, None], draws["target_index"]][:, 0]
    d64, d32 = pred.cpu().double() - target.double(), pred.cpu().float() - target.float()
    return (d64 * d64).mean((1, 2, 3)), (d32 * d32).mean((1, 2, 3))


def _reset_options(m):
    m.loss_weighting, m.loss_type, m.loss_mask, m.log_per_sample = None, "l2", None, False


def test_model_min_snr_loss_is_the_weighted_mean_of_the_per_sample_errors(small):
    m, st = small
    try:
        loss0, _ = _model_step(m, st)
        assert m.last_loss_per_sample is None and m.last_mse_per_sample is None  # kept only when asked for
        m.loss_weighting, m.snr_gamma = "min_snr", 5.0
        loss, draws = _model_step(m, st)
        w = min_snr_weights(m.sampler.schedule.alphas_cumprod, draws["time_steps"], 5.0)
        assert bool((w < 1.0).any()) and bool((w == 1.0).any())
        mse64, mse32 = _host_mse(st, m.last_noise_predict, draws)
        want = (w.double() * mse64).mean()
        ref32 = (w * mse32).mean()
        fails = _check("model min_snr", (loss.cpu(), m.last_loss_per_sample.cpu(), m.last_mse_per_sample.cpu()),
                       (want, mse64, mse64), (ref32, mse32, mse32))
        assert not fails, fails
        assert abs(float(loss) - float(loss0)) > 1e-3 * float(loss0)  # the weights did something
        # an explicit sample weight multiplies the Min-SNR weights
        sw = torch.tensor([0.5, 2.0, 1.0, 0.25][:st["B"]])
        loss_sw, _ = _model_step(m, st, sample_weight=sw)
        mse64, mse32 = _host_mse(st, m.last_noise_predict, draws)
        fails = _check("model min_snr x sample_weight", (loss_sw.cpu(),), ((w.double() * sw.double() * mse64).mean(),),
                       ((w * sw * mse32).mean(),))
        assert not fails, fails
    finally:
        _reset_options(m)


def test_model_foreground_mask_on_white_views_is_the_unmasked_loss(small):
    m, st = small
    try:
        batch = dict(st["dev"])
        N = st["cfg"][2]
        batch["target_image"] = torch.ones(st["B"], N, 256, 256, 3, device="cuda")
        m.loss_mask, m.background_weight = "foreground", 0.1
        loss, draws = _model_step(m, st, batch=batch)
        mse64, mse32 = _host_mse(st, m.last_noise_predict, draws)
        fails = _check("model foreground, white views", (loss.cpu(), m.last_loss_per_sample.cpu(), m.last_mse_per_sample.cpu()),
                       (mse64.mean(), mse64, mse64), (mse32.mean(), mse32, mse32))
        assert not fails, fails
        # an explicit mask replaces the derived one (here: at image resolution, pooled on the way in)
        mask = torch.zeros(st["B"], 1, 256, 256)
        mask[:, :, :128] = 1.0
        _model_step(m, st, batch=batch, loss_mask=mask)
        assert float((m.last_loss_per_sample - m.last_mse_per_sample).abs().max()) > 0.0
        m.loss_mask = None
        with pytest.raises(ValueError, match="loss_mask"):
            _model_step(m, st, loss_mask=torch.ones(st["B"], 32, 32))
    finally:
        _reset_options(m)


def test_model_deterministic_step_with_options_repeats_bit_for_bit(small):
    m, st = small
    try:
        assert m.deterministic
        m.loss_weighting, m.loss_type, m.huber_delta = "min_snr", "huber", DELTA
        mask = torch.rand(st["B"], 1, 32, 32, generator=torch.Generator().manual_seed(9))
        got = []
        for _ in range(2):
            loss, _ = _model_step(m, st, loss_mask=mask)
            got.append((loss.clone(), m.engine.flat_grads.clone(), m.last_loss_per_sample.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*got))
        assert float(got[0][1].abs().max()) > 0.0 and torch.isfinite(got[0][1]).all()
    finally:
        _reset_options(m)


def test_loss_option_without_train_mode_and_held_out_loss_on_an_inference_model(small):
    _, st = small
    ucfg, vcfg, N = st["cfg"]
    plain = make_train_model(ucfg, vcfg, N, train_mode=False, loss_weighting="min_snr")
    try:
        with pytest.raises(ValueError, match="train_mode"):
            plain.training_step(st["dev"], prepared=st["prepared"], backward=True, **st["draws"])
        loss, draws = _model_step(plain, st)  # forward only: the weighted loss through the hook
        w = min_snr_weights(plain.sampler.schedule.alphas_cumprod, draws["time_steps"], 5.0)
        mse64, mse32 = _host_mse(st, plain.last_noise_predict, draws)
        fails = _check("inference model, min_snr forward", (loss.cpu(), plain.last_loss_per_sample.cpu()),
                       ((w.double() * mse64).mean(), mse64), ((w * mse32).mean(), mse32))
        assert not fails, fails
        a = plain.validation_loss(st["dev"], timesteps=(300,), prepared=st["prepared"])
        b = plain.validation_loss(st["dev"], timesteps=(300,), prepared=st["prepared"])
        assert torch.equal(a["per_timestep"][300], b["per_timestep"][300]) and np.isfinite(a["mean"]) and a["mean"] > 0.0
    finally:
        plain.engine.close()


def test_validation_loss_is_reproducible_and_leaves_the_model_alone(small):
    m, st = small
    eng = m.engine
    sd0 = {k: v.clone() for k, v in m.state_dict().items() if torch.is_tensor(v)}
    calls0, grads0 = eng.train_bn_calls(), eng.flat_grads.clone()
    rng0 = torch.get_rng_state()
    m.train()
    ti = torch.tensor([1, 0, 3, 2][:st["B"]])
    a = m.validation_loss(st["dev"], timesteps=(100, 700), seed=3, target_index=ti, prepared=st["prepared"])
    b = m.validation_loss(st["dev"], timesteps=(100, 700), seed=3, target_index=ti, prepared=st["prepared"])
    assert m.training and torch.equal(torch.get_rng_state(), rng0)
    assert list(a["per_timestep"]) == [100, 700]
    for t in (100, 700):
        assert a["per_timestep"][t].shape == (st["B"],) and a["per_timestep"][t].is_cuda
        assert torch.equal(a["per_timestep"][t], b["per_timestep"][t])
    both = torch.stack([a["per_timestep"][t] for t in (100, 700)]).double()
    assert a["mean"] == b["mean"] and abs(a["mean"] - float(both.mean())) <= 1e-12
    assert eng.train_bn_calls() == calls0 and torch.equal(eng.flat_grads, grads0)
    sd1 = m.state_dict()
    assert all(torch.equal(sd1[k], v) for k, v in sd0.items())
    c = m.validation_loss(st["dev"], timesteps=(100,), seed=4, target_index=ti, prepared=st["prepared"])
    assert not torch.equal(c["per_timestep"][100], a["per_timestep"][100])  # another seed is another noise
    # one timestep against an explicit eval-mode forward with the same noise
    x, clip, info = st["prepared"]
    B, t = st["B"], 700
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).cuda()
    ts = torch.full((B,), t, dtype=torch.long, device="cuda")
    tix = ti.reshape(B, 1).cuda()
    ar = torch.arange(B, device="cuda")[:, None]
    m.eval()
    try:
        x_noisy, _ = m.add_noise(x, ts, noise)
        v_embed, t_embed = m.get_viewpoint_embedding(st["dev"]), m.embed_time(ts)
        sv = m.spatial_volume.construct_spatial_volume(x_noisy, t_embed, v_embed, st["dev"])
        clip_, vf, xc = m.get_target_view_feats(info["x"], sv, clip, t_embed, v_embed, tix, st["dev"])
        pred = m.model(x_noisy[ar, tix][:, 0], ts, clip_, vf, xc, is_train=False)
    finally:
        m.train()
    target = noise[ar, tix][:, 0]
    d64, d32 = (pred.double() - target.double()).cpu(), (pred - target).cpu()
    fails = _check("validation_loss t=700", (a["per_timestep"][t].cpu(),), ((d64 * d64).mean((1, 2, 3)),),
                   ((d32 * d32).mean((1, 2, 3)),), names=("mse_b",))
    assert not fails, fails


class _StubVae:
    """An injected first-stage model: deterministic moments, so that what varies is the posterior's sample() draw alone."""

    def encode(self, x):
        from morphablediffusion_amd.model import DiagonalGaussianDistribution
        mean = torch.nn.functional.avg_pool2d(x.float(), 8)  # [B,3,h,w]
        mean = torch.cat([mean, mean.mean(1, keepdim=True)], 1)
        return DiagonalGaussianDistribution(torch.cat([mean, torch.full_like(mean, -1.0)], 1))


class _StubClip:
    def encode(self, x):
        return x.float().mean((2, 3)).repeat(1, 256)[:, None]  # [B,1,768]


def test_validation_loss_default_path_runs_prepare_and_leaves_every_random_stream(small):
    """Without ``prepared``: validation_loss encodes the batch itself, and the posterior samples are random draws.  Both global
    streams -- the default CPU generator and the device's -- must be where they were, and two calls must agree bit for bit."""
    m, st = small
    B, N = st["B"], st["cfg"][2]
    g = torch.Generator().manual_seed(21)
    batch = dict(st["dev"])
    batch["target_image"] = (torch.rand(B, N, 256, 256, 3, generator=g) * 2 - 1).cuda()
    batch["input_image"] = (torch.rand(B, 256, 256, 3, generator=g) * 2 - 1).cuda()
    assert not getattr(m.engine, "has_vae_encoder", False) and not getattr(m.engine, "has_clip", False)
    m.first_stage_model, m.clip_image_encoder = _StubVae(), _StubClip()
    try:
        torch.manual_seed(77)
        torch.randn(3, device="cuda")  # the device generator is in use, somewhere past its seed
        cpu0, gpu0 = torch.get_rng_state(), torch.cuda.get_rng_state()
        calls0 = m.engine.train_bn_calls()
        a = m.validation_loss(batch, timesteps=(300,), seed=0)
        assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), gpu0)
        b = m.validation_loss(batch, timesteps=(300,), seed=0)
        assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), gpu0)
        assert torch.isfinite(a["per_timestep"][300]).all() and torch.equal(a["per_timestep"][300], b["per_timestep"][300])
        c = m.validation_loss(batch, timesteps=(300,), seed=1)
        assert not torch.equal(c["per_timestep"][300], a["per_timestep"][300])
        assert m.engine.train_bn_calls() == calls0
        # the draws really come from the default CPU generator: prepare on its own moves it
        m.prepare(batch, encode_targets=True)
        assert not torch.equal(torch.get_rng_state(), cpu0)
    finally:
        m.first_stage_model = m.clip_image_encoder = None


def test_validation_loss_runs_on_the_ema_weights_and_puts_the_parameters_back(small):
    _, st = small
    ucfg, vcfg, N = st["cfg"]
    m = make_train_model(ucfg, vcfg, N, use_ema=True)
    try:
        eng = m.engine
        kw = dict(timesteps=(500,), prepared=st["prepared"])
        same = m.validation_loss(st["dev"], **kw)["per_timestep"][500]  # the initial shadow is a copy of the parameters
        m.use_ema = False
        base = m.validation_loss(st["dev"], **kw)["per_timestep"][500]
        m.use_ema = True
        assert torch.equal(same, base)
        p0 = eng.flat_params.clone()
        eng.ensure_ema().mul_(0.9)  # another set of weights in the shadow
        e0 = eng.flat_ema.clone()
        other = m.validation_loss(st["dev"], **kw)["per_timestep"][500]
        assert torch.isfinite(other).all() and not torch.equal(other, base)
        assert torch.equal(eng.flat_params, p0) and torch.equal(eng.flat_ema, e0)
        assert torch.equal(m.validation_loss(st["dev"], **kw)["per_timestep"][500], other)
    finally:
        m.engine.close()


def test_lora_step_with_min_snr_changes_the_adapters(small):
    """Last in the file: it attaches adapters to the fixture's model (and drops them again)."""
    m, st = small
    try:
        m.enable_lora(rank=4, seed=1)
        m.learning_rate = 5e-3
        (opt,), _ = m.configure_optimizers()
        before = m.engine.lora_params.clone()
        m.loss_weighting = "min_snr"
        loss, _ = _model_step(m, st)
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and opt.steps_skipped == 0
        assert torch.isfinite(m.engine.lora_params).all() and not torch.equal(m.engine.lora_params, before)
    finally:
        _reset_options(m)
        m.disable_lora()

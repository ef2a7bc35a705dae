"""Gradient clipping by global norm and EMA weights in the optimiser step (mvd_train_adamw_step_ex): the kernels on raw buffers
against a torch restatement (fp64 norm, clip_grad_norm_, torch.optim.AdamW, LitEma's shadow update), the entry point against the
existing step, the model surface (ArenaAdamW(max_grad_norm), use_ema, ema_scope, checkpoint keys).

Bounds: the norm to 1e-6 relative (fp32 per-block partials of at most 16 squares per accumulator at these sizes, summed in
double); p / m / v / e to the normalised 2e-6 that test_adamw_step_and_repack allows the existing step against torch."""
import ctypes as C

import pytest
import torch

from morphablediffusion_amd import lib as L
from morphablediffusion_amd.model import ema_decay_at, ema_key
from morphablediffusion_amd.spec import VolumeConfig
from tests import golden_inputs as gi
from tests.test_gpu_train import P, _inputs, make_train_model

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 1e-2
STEPS = 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _norm_diff(got, want):
    return ((got - want).abs().max() / (want.abs().max() + 1e-12)).item()


def _raw_inputs(n, seed=0):
    g = torch.Generator().manual_seed(1234 + seed)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.01 for _ in range(STEPS)]
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 1e-4
    e = p + torch.randn(n, generator=g) * 0.01
    return [t.cuda() for t in (p, m, v, e)], [t.cuda() for t in grads]


def _run_hip(state, grads, max_norms, scale, use_ema, want_norm=True):
    """STEPS calls of mvd_op_adamw_ex on copies (max_norms: one per step, or None); returns (p, m, v, e, [norm per step])."""
    lib = L.load()
    p, m, v, e = [t.clone() for t in state]
    norms = []
    for k, g in enumerate(grads):
        gs = (g * scale).contiguous()
        norm = torch.full((1,), -1.0, device="cuda") if want_norm else None
        d = ema_decay_at(0.9999, k + 1) if use_ema else -1.0
        L.check(lib.mvd_op_adamw_ex(p.data_ptr(), gs.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr() if use_ema else None,
                                    p.numel(), LR, BETAS[0], BETAS[1], EPS, WD, k + 1, 1.0 / scale,
                                    0.0 if max_norms is None else max_norms[k], d, L.ptr(norm), _stream()))
        norms.append(norm)
    torch.cuda.synchronize()
    return p, m, v, e, norms


def _run_torch(state, grads, max_norms, use_ema):
    """The restatement: fp64 norm, clip_grad_norm_, torch.optim.AdamW from the same moments, then e -= (1 - d) (e - p)."""
    p, m, v, e = [t.clone() for t in state]
    q = p.requires_grad_(True)
    opt = torch.optim.AdamW([q], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    opt.state[q] = {"step": torch.tensor(0.0), "exp_avg": m, "exp_avg_sq": v}
    norms, coefs = [], []
    for k, g in enumerate(grads):
        q.grad = g.clone()
        norms.append(g.double().norm().item())
        if max_norms is not None:
            torch.nn.utils.clip_grad_norm_([q], max_norms[k])
            coefs.append((q.grad.abs().max() / g.abs().max()).item())
        opt.step()
        if use_ema:
            with torch.no_grad():
                e -= (1.0 - ema_decay_at(0.9999, k + 1)) * (e - q)
    return q.detach(), m, v, e, norms, coefs


CASES = {  # name: (max_norm as a multiple of the torch norm of the same step's gradients, loss scale, EMA)
    "clip_active": (0.5, 1.0, True),
    "clip_inactive": (2.0, 1.0, True),
    "loss_scaled": (0.5, 65536.0, True),
    "clip_without_ema": (0.5, 1.0, False),
    "ema_without_clip": (None, 1.0, True),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n", [64, 192, 64 * 1021, 2 ** 22 + 64])
def test_kernels_on_raw_buffers_vs_torch(n, case):
    """n: less than one vector per lane, less than one block, a partial last group behind several blocks, and (2^22 + 64 = one
    float4 group more than the 1024-block grid covers in one pass) a second pass of the grid-stride loops."""
    mult, scale, use_ema = CASES[case]
    state, grads = _raw_inputs(n)
    max_norm = None if mult is None else [mult * g.double().norm().item() for g in grads]
    want = _run_torch(state, grads, max_norm, use_ema)
    got = _run_hip(state, grads, max_norm, scale, use_ema, want_norm=case != "ema_without_clip")
    worst = {}
    for name, a, b in zip("pmve", got[:4], want[:4]):
        worst[name] = _norm_diff(a, b)
    if case != "ema_without_clip":
        worst["norm"] = max(abs(h.item() - w) / w for h, w in zip(got[4], want[4]))
    print(f"[clip/ema] n = {n} {case}: " + ", ".join(f"{k} {x:.2e}" for k, x in worst.items()) +
          (f", torch coefficients {want[5]}" if want[5] else ""))
    if case == "clip_inactive":
        assert all(c == 1.0 for c in want[5])
    elif mult is not None:
        assert all(abs(c - 0.5) < 1e-3 for c in want[5])
    if not use_ema:
        assert torch.equal(got[3], state[3])
    assert worst.get("norm", 0.0) <= 1e-6
    for name in "pmve":
        assert worst[name] <= 2e-6, (name, worst)
    # bit-reproducible: the grid is a function of n, the reductions have a fixed order, nothing is atomic
    again = _run_hip(state, grads, max_norm, scale, use_ema, want_norm=case != "ema_without_clip")
    for a, b in zip(got[:4], again[:4]):
        assert torch.equal(a, b)
    if case != "ema_without_clip":
        assert all(torch.equal(a, b) for a, b in zip(got[4], again[4]))


# ---- on a model ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """A small use_ema model after ONE real training_step (gradients of every group in the arena), with the state to return to."""
    g, dev, prepared, draws = _inputs()
    N = int(g["N"])
    ucfg, vcfg = gi.SMALL_UNET, VolumeConfig(num_views=N)
    m = make_train_model(ucfg, vcfg, N, loss_scale=65536.0, recompute=True, use_ema=True)
    m.learning_rate = 5e-5
    m.engine.zero_grad()
    m.training_step(dev, prepared=prepared, **draws)
    eng = m.engine
    eng.ensure_moments()
    eng.ensure_ema()
    snap = dict(p=eng.flat_params.clone(), g=eng.flat_grads.clone())
    assert torch.equal(eng.flat_ema, snap["p"]), "a new EMA arena starts as a copy of the parameters"
    yield m, snap, (ucfg, vcfg, N)
    m.engine.close()


@pytest.fixture(scope="module")
def plain(trained):
    """An inference model (no training mode, no EMA) for the tests to load state_dicts into."""
    _, _, (ucfg, vcfg, N) = trained
    m2 = make_train_model(ucfg, vcfg, N, train_mode=False)
    yield m2
    m2.engine.close()


def _restore(m, snap, finetune_unet=True, ema_decay=0.9999):
    eng = m.engine
    eng.flat_params.copy_(snap["p"])
    eng.flat_grads.copy_(snap["g"])
    eng.flat_m.zero_()
    eng.flat_v.zero_()
    eng.flat_ema.copy_(snap["p"])
    eng.repack()
    m.loss_scale, m.finetune_unet, m.ema_decay, m.ema_num_updates, m.gradient_clip_val = 65536.0, finetune_unet, ema_decay, 0, None


def _worst(eng, got, want):
    """Worst per-parameter normalised difference over the real parameter slots (the arena pads each tensor to 64 floats)."""
    worst = 0.0
    for k, (o, n, s) in eng.param_table.items():
        worst = max(worst, _norm_diff(got[o:o + n], want[o:o + n]))
    return worst


def _aux_lo(eng):
    return min(o for k, (o, n, s) in eng.param_table.items() if not k.startswith(P))


def test_step_ex_with_both_features_off_equals_the_existing_step(trained):
    m, snap, _ = trained
    eng = m.engine
    out = {}
    for name in ("old", "ex"):
        _restore(m, snap)
        sk = C.c_int(-1)
        args = (eng._ctx, 5e-5, 5e-4, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0 / 65536.0, 1, C.byref(sk))
        if name == "old":
            L.check(eng.lib.mvd_train_adamw_step(*args, _stream()))
        else:
            L.check(eng.lib.mvd_train_adamw_step_ex(*args, 0.0, -1.0, None, _stream()))
        assert sk.value == 0
        out[name] = [t.clone() for t in (eng.flat_params, eng.flat_m, eng.flat_v, eng.flat_ema)]
    worst = [_worst(eng, a, b) for a, b in zip(out["ex"][:3], out["old"][:3])]
    print(f"[clip/ema] step_ex (clipping off, EMA off) vs mvd_train_adamw_step: p / m / v worst normalised {worst}, "
          f"bit-equal {[torch.equal(a, b) for a, b in zip(out['ex'][:3], out['old'][:3])]}")
    assert max(worst) <= 2e-6
    assert (out["ex"][0] - snap["p"]).abs().max() > 0
    assert torch.equal(out["ex"][3], snap["p"]), "EMA off: the EMA arena is not touched"
    _restore(m, snap)


def test_model_step_with_clipping_and_ema_vs_torch(trained):
    m, snap, _ = trained
    eng = m.engine
    _restore(m, snap)
    lo = _aux_lo(eng)
    g0 = snap["g"] / m.loss_scale
    norm64 = g0.double().norm().item()
    m.gradient_clip_val = 0.5 * norm64
    (opt,), _ = m.configure_optimizers()
    assert opt.max_grad_norm == m.gradient_clip_val
    ref_p = [snap["p"][:lo].clone().requires_grad_(True), snap["p"][lo:].clone().requires_grad_(True)]
    ref_p[0].grad, ref_p[1].grad = g0[:lo].clone(), g0[lo:].clone()
    ref_norm = torch.nn.utils.clip_grad_norm_(ref_p, m.gradient_clip_val).item()
    ref = torch.optim.AdamW([{"params": [ref_p[0]], "lr": opt.param_groups[0]["lr"]},
                             {"params": [ref_p[1]], "lr": opt.param_groups[1]["lr"]}])
    ref.step()
    opt.step()
    assert opt.steps_done == 1 and opt.steps_skipped == 0 and m.ema_num_updates == 1
    assert torch.is_tensor(opt.last_grad_norm) and opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0
    want_p = torch.cat([ref_p[0].detach(), ref_p[1].detach()])
    d = ema_decay_at(0.9999, 1)
    want_e = snap["p"] - (1.0 - d) * (snap["p"] - want_p)
    rel = abs(opt.last_grad_norm.item() - norm64) / norm64
    wp, we = _worst(eng, eng.flat_params, want_p), _worst(eng, eng.flat_ema, want_e)
    print(f"[clip/ema] model step: norm {opt.last_grad_norm.item():.6e} vs fp64 {norm64:.6e} (rel {rel:.1e}; clip_grad_norm_ "
          f"{ref_norm:.6e}), p {wp:.2e}, ema {we:.2e}")
    assert rel <= 1e-6 and wp <= 2e-6 and we <= 2e-6
    assert (eng.flat_ema - snap["p"]).abs().max() > 0
    # finetune_unet=False: the norm covers the DepthTransformers and the aux group only; everything else is frozen
    _restore(m, snap, finetune_unet=False)
    m.gradient_clip_val = 1e-3
    (opt,), _ = m.configure_optimizers()
    live = torch.zeros_like(snap["p"], dtype=torch.bool)
    for k, (o, n, s) in eng.param_table.items():
        if not k.startswith(P) or k.startswith((P + "middle_conditions.", P + "output_conditions.")):
            live[o:o + n] = True
    want_norm = g0[live].double().norm().item()
    assert want_norm < 0.999 * norm64
    assert abs(eng.grad_norm(1.0 / m.loss_scale, finetune_unet=False).item() - want_norm) <= 1e-6 * want_norm
    assert abs(eng.grad_norm(1.0 / m.loss_scale, finetune_unet=True).item() - norm64) <= 1e-6 * norm64
    opt.step()
    assert abs(opt.last_grad_norm.item() - want_norm) <= 1e-6 * want_norm
    frozen = ~live
    assert torch.equal(eng.flat_params[frozen], snap["p"][frozen]) and torch.equal(eng.flat_ema[frozen], snap["p"][frozen])
    assert float(eng.flat_m[frozen].abs().max()) == 0.0 and float(eng.flat_v[frozen].abs().max()) == 0.0
    assert (eng.flat_params[live] - snap["p"][live]).abs().max() > 0 and (eng.flat_ema[live] - snap["p"][live]).abs().max() > 0
    _restore(m, snap)


def test_overflow_skips_parameters_moments_and_ema(trained):
    m, snap, _ = trained
    eng = m.engine
    _restore(m, snap)
    m.gradient_clip_val = 1.0
    (opt,), _ = m.configure_optimizers()
    opt.step()  # one clean step first: moments and EMA differ from their initial values
    before = [t.clone() for t in (eng.flat_params, eng.flat_m, eng.flat_v, eng.flat_ema)]
    assert m.ema_num_updates == 1
    eng.flat_grads[5] = float("inf")
    opt.step()
    assert opt.steps_skipped == 1 and opt.steps_done == 1 and m.loss_scale == 32768.0 and m.ema_num_updates == 1
    for a, b in zip((eng.flat_params, eng.flat_m, eng.flat_v, eng.flat_ema), before):
        assert torch.equal(a, b)
    _restore(m, snap)


def test_ema_scope_runs_the_engine_on_the_ema_weights(trained, plain):
    m, snap, (ucfg, vcfg, N) = trained
    eng = m.engine
    _restore(m, snap, ema_decay=0.5)
    m.learning_rate = 5e-3  # (1e-4 after the warm-up factor: four updates move fp16-rounded weights visibly)
    (opt,), _ = m.configure_optimizers()
    m.learning_rate = 5e-5
    for _ in range(4):
        opt.step()
    p_before, e_before = eng.flat_params.clone(), eng.flat_ema.clone()
    assert not torch.equal(p_before, e_before) and (p_before - e_before).abs().max() > 1e-6
    x, t, ctx, sd = gi.unet_inputs(ucfg, Bv=2)
    x, t, ctx, sd = x.cuda(), t.cuda(), ctx.cuda(), {k: v.cuda() for k, v in sd.items()}
    out_before = eng.unet_forward(x, t, ctx, sd)
    with m.ema_scope():
        for k, (o, n, s) in eng.param_table.items():
            assert torch.equal(eng.param_view(k), e_before[o:o + n].view(s)), k
        assert torch.equal(eng.flat_ema, p_before)
        out_ema = eng.unet_forward(x, t, ctx, sd)
    # the same call on a model that was LOADED with the EMA tensors as its parameters: same code on the same bits
    W2 = {k: e_before[o:o + n].view(s).cpu().clone() for k, (o, n, s) in eng.param_table.items()}
    for k, v in gi.full_weights(ucfg, vcfg).items():
        W2.setdefault(k, v)
    plain.load_state_dict(W2)
    out_fresh = plain.engine.unet_forward(x, t, ctx, sd)
    assert torch.equal(out_ema, out_fresh)
    assert not torch.equal(out_ema, out_before)
    assert torch.equal(eng.flat_params, p_before) and torch.equal(eng.flat_ema, e_before)
    assert torch.equal(eng.unet_forward(x, t, ctx, sd), out_before)
    _restore(m, snap)


def test_checkpoint_round_trips_ema_and_max_grad_norm(trained, plain):
    m, snap, (ucfg, vcfg, N) = trained
    eng = m.engine
    _restore(m, snap, ema_decay=0.5)
    m.gradient_clip_val = 0.25
    (opt,), _ = m.configure_optimizers()
    opt.step()
    opt.step()
    sd = m.state_dict()
    ema_keys = [k for k in sd if k.startswith("model_ema.")]
    assert len(ema_keys) == len(eng.param_table) + 2 and len(set(ema_key(k) for k in eng.param_table)) == len(eng.param_table)
    for k, (o, n, s) in eng.param_table.items():
        assert torch.equal(sd[ema_key(k)], eng.flat_ema[o:o + n].view(s)), k
    assert sd["model_ema.decay"].dtype == torch.float32 and sd["model_ema.decay"].item() == 0.5
    assert sd["model_ema.num_updates"].dtype == torch.int64 and sd["model_ema.num_updates"].item() == 2
    m3 = make_train_model(ucfg, vcfg, N, loss_scale=65536.0, use_ema=True, ema_decay=0.5)
    assert torch.equal(m3.engine.flat_ema, m3.engine.flat_params) and m3.ema_num_updates == 0  # no EMA keys: from the parameters
    m3.load_state_dict(sd)
    assert torch.equal(m3.engine.flat_ema, eng.flat_ema) and torch.equal(m3.engine.flat_params, eng.flat_params)
    assert m3.ema_num_updates == 2
    (opt3,), _ = m3.configure_optimizers()
    assert opt3.max_grad_norm is None
    opt3.load_state_dict(opt.state_dict())
    assert opt3.max_grad_norm == 0.25 and opt3.steps_done == 2
    m3.engine.close()
    plain.load_state_dict(sd)  # a model without use_ema ignores the EMA keys
    assert not hasattr(plain.engine, "flat_ema") or plain.engine.flat_ema is None
    _restore(m, snap)

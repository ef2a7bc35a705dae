"""LoRA fine-tuning on the small model: enable_lora leaves the model as it was, mvd_lora_step's projection against the dense
gradients (float64), three optimiser steps against torch.optim.AdamW on copies of the adapters, the overflow rule, the merged
weights in the engine and in checkpoints, adapter / optimiser round trips, determinism, errors.

Bounds: projected gradients and merged masters within the ops test's 8 e_ref + 2e-6 (e_ref: torch's CPU fp32 matmul against
float64 on the same inputs); adapters and moments to the normalised 2e-6 of test_adamw_step_and_repack; the norm to 1e-6."""
import io

import pytest
import torch

from morphablediffusion_amd.lora import DEFAULT_PATTERNS, merge_lora
from morphablediffusion_amd.spec import VolumeConfig
from tests import golden_inputs as gi
from tests.test_gpu_train import P, _inputs, make_train_model

pytestmark = pytest.mark.gpu

RANK, ALPHA = 4, 8.0
S = ALPHA / RANK
TARGETS = list(DEFAULT_PATTERNS) + ["*.proj_in.weight"]


def _nerr(got, want):
    return ((got.double().cpu() - want.cpu()).abs().max() / (want.abs().max().item() + 1e-300)).item()


def _norm_diff(got, want):
    return ((got.cpu() - want.cpu()).abs().max() / (want.abs().max().item() + 1e-12)).item()


def _step_inputs(m, st):
    m.engine.zero_grad()
    return m.training_step(st["dev"], prepared=st["prepared"], **st["draws"])


@pytest.fixture(scope="module")
def lora():
    """A small deterministic training model: one training_step before enable_lora (kept for comparison), then LoRA enabled on
    the default targets plus the SpatialTransformers' 1x1 proj_in convolutions."""
    g, dev, prepared, draws = _inputs()
    N = int(g["N"])
    ucfg, vcfg = gi.SMALL_UNET, VolumeConfig(num_views=N)
    m = make_train_model(ucfg, vcfg, N, loss_scale=65536.0, recompute=True, deterministic=True)
    m.learning_rate = 5e-3
    st = dict(dev=dev, prepared=prepared, draws=draws, cfg=(ucfg, vcfg, N))
    loss = _step_inputs(m, st)
    eng = m.engine
    st["before"] = dict(loss=loss.clone(), pred=m.last_noise_predict.clone(), g=eng.flat_grads.clone(), p=eng.flat_params.clone())
    st["keys"] = m.enable_lora(rank=RANK, alpha=ALPHA, targets=TARGETS, seed=3)
    st["A0"] = eng.lora_params.clone()  # B = 0
    gen = torch.Generator().manual_seed(17)
    noisy = st["A0"].clone()
    for k in st["keys"]:
        a, b, out, in_ = eng.lora_table[k]
        noisy[b:b + out * RANK] = (torch.randn(out * RANK, generator=gen) * 0.02).cuda()
    st["AB"] = noisy  # A as initialised, B seeded noise
    yield m, st
    m.engine.close()


@pytest.fixture(scope="module")
def plain(lora):
    _, st = lora
    ucfg, vcfg, N = st["cfg"]
    m2 = make_train_model(ucfg, vcfg, N, train_mode=False)
    yield m2
    m2.engine.close()


def _reset(m, st, noisy=True):
    """Adapters back to (A initial, B noise or 0), zero moments, the loss scale, masters merged, a fresh optimiser."""
    eng = m.engine
    eng.lora_params.copy_(st["AB"] if noisy else st["A0"])
    eng.lora_m.zero_()
    eng.lora_v.zero_()
    eng.lora_grads.zero_()
    m.loss_scale, m.gradient_clip_val = 65536.0, None
    eng.lora_set_scale(S)
    (opt,), (sched,) = m.configure_optimizers()
    return opt, sched["scheduler"]


def _views64(eng, key, flat=None):
    a, b, out, in_ = eng.lora_table[key]
    flat = eng.lora_params if flat is None else flat
    A = flat[a:a + RANK * in_].view(RANK, in_).double().cpu()
    B = flat[b:b + out * RANK].view(out, RANK).double().cpu()
    return A, B


def _projected64(eng, keys, flat_grads):
    """{key: (gA, gB)} in float64 from the dense gradients and the current adapters."""
    out = {}
    for k in keys:
        o, n, s = eng.param_table[k]
        dW = flat_grads[o:o + n].view(s[0], s[1]).double().cpu()
        A, B = _views64(eng, k)
        out[k] = (S * B.t() @ dW, S * dW @ A.t(), dW, A, B)
    return out


def test_attach_changes_nothing(lora):
    m, st = lora
    eng = m.engine
    keys = st["keys"]
    blocks = {k.split(".transformer_blocks.")[0] for k in eng.param_table if ".transformer_blocks." in k}
    assert len(keys) == 9 * len(blocks) and sum(k.endswith(".proj_in.weight") for k in keys) == len(blocks)
    assert m.lora_enabled and eng.lora_rank == RANK
    opt, _ = _reset(m, st, noisy=False)
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 2 * len(keys)
    assert all(p_.data_ptr() >= eng.lora_params.data_ptr() and p_.grad is not None for p_ in opt.param_groups[0]["params"])
    loss = _step_inputs(m, st)
    b = st["before"]
    assert torch.equal(loss, b["loss"]) and torch.equal(m.last_noise_predict, b["pred"])
    assert torch.equal(eng.flat_grads, b["g"])
    assert torch.equal(eng.flat_params, b["p"])
    sd = m.state_dict()
    assert set(sd) == set(gi.full_weights(*st["cfg"][:2]))


def test_projection_against_the_dense_gradients(lora):
    m, st = lora
    eng = m.engine
    _reset(m, st)
    _step_inputs(m, st)
    ref = _projected64(eng, st["keys"], eng.flat_grads)
    assert float(eng.lora_grads.abs().max()) == 0.0  # the backward pass does not write them: the projection does
    eng.lora_project()
    assert torch.equal(eng.lora_params, st["AB"])
    worst, nonzero = (0.0, 0.0, ""), 0
    for k in st["keys"]:
        gA64, gB64, dW, A, B = ref[k]
        for name, got, want, r32 in (("A", eng.lora_view(k, "A", grad=True), gA64, S * (B.float().t() @ dW.float())),
                                     ("B", eng.lora_view(k, "B", grad=True), gB64, S * (dW.float() @ A.float().t()))):
            e, e_ref = _nerr(got, want), _nerr(r32, want)
            nonzero += bool(want.abs().max() > 0)  # (attn2.to_k / to_v see a dropped, all-zero context: their dW is zero)
            if e / (8 * e_ref + 2e-6) >= worst[0] / (worst[1] + 1e-300):
                worst = (e, 8 * e_ref + 2e-6, f"{k}.{name}")
            assert e <= 8 * e_ref + 2e-6, (k, name, e, e_ref)
    print(f"[lora] projection vs float64, closest to its bound: {worst[2]} {worst[0]:.3e} (bound {worst[1]:.3e})")
    assert nonzero > len(st["keys"])  # more than half of the 2 x len(keys) projected gradients are not identically zero
    assert any(len(eng.param_table[k][2]) == 4 for k in st["keys"])  # the (out, in, 1, 1) targets were among them


def test_three_optimiser_steps_against_torch(lora):
    m, st = lora
    eng = m.engine
    keys = st["keys"]
    opt, sched = _reset(m, st)
    p_init = st["before"]["p"]
    W0 = {}
    for k in keys:
        o, n, shape = eng.param_table[k]
        W0[k] = p_init[o:o + n].view(shape[0], shape[1]).double().cpu()
    is_target = torch.zeros_like(p_init, dtype=torch.bool)
    for k in keys:
        o, n, _ = eng.param_table[k]
        is_target[o:o + n] = True
    # the reference: torch.optim.AdamW on float copies of A and B
    ref_p = {}
    for k in keys:
        a, b, out, in_ = eng.lora_table[k]
        ref_p[k] = (eng.lora_view(k, "A").detach().cpu().clone().requires_grad_(True),
                    eng.lora_view(k, "B").detach().cpu().clone().requires_grad_(True))
    flat_ref = [t for k in keys for t in ref_p[k]]
    # (the C ABI takes the betas as floats: the reference gets those very numbers -- with a zero second moment to start from,
    # 1 - 0.999 in double and 1 - float(0.999) differ by 1.3e-5 relative, which is all of exp_avg_sq after the first step)
    betas = tuple(float(torch.tensor(b_, dtype=torch.float32)) for b_ in opt.param_groups[0]["betas"])
    ref = torch.optim.AdamW(flat_ref, lr=1.0, betas=betas, eps=1e-8, weight_decay=1e-2)
    worst = dict(p=0.0, m=0.0, v=0.0, norm=0.0, merged=0.0)
    for step in range(3):
        _step_inputs(m, st)
        proj = _projected64(eng, keys, eng.flat_grads)
        for k in keys:
            ref_p[k][0].grad = (proj[k][0] / m.loss_scale).float()
            ref_p[k][1].grad = (proj[k][1] / m.loss_scale).float()
        norm64 = torch.sqrt(sum((proj[k][j] / m.loss_scale).pow(2).sum() for k in keys for j in (0, 1))).item()
        if step == 0:
            opt.max_grad_norm = 0.5 * norm64  # clipping active in the first step at least
        torch.nn.utils.clip_grad_norm_(flat_ref, opt.max_grad_norm)
        for gr in ref.param_groups:
            gr["lr"] = opt.param_groups[0]["lr"]
        ref.step()
        opt.step()
        sched.step()
        assert opt.steps_done == step + 1 and opt.steps_skipped == 0
        worst["norm"] = max(worst["norm"], abs(opt.last_grad_norm.item() - norm64) / norm64)
        for k in keys:
            for j, which in enumerate("AB"):
                worst["p"] = max(worst["p"], _norm_diff(eng.lora_view(k, which), ref_p[k][j].detach()))
                a, b, out, in_ = eng.lora_table[k]
                off, n = (a, RANK * in_) if which == "A" else (b, out * RANK)
                stt = ref.state[ref_p[k][j]]
                worst["m"] = max(worst["m"], _norm_diff(eng.lora_m[off:off + n], stt["exp_avg"].reshape(-1)))
                worst["v"] = max(worst["v"], _norm_diff(eng.lora_v[off:off + n], stt["exp_avg_sq"].reshape(-1)))
            A, B = _views64(eng, k)
            want = W0[k] + S * B @ A
            r32 = W0[k].float() + S * (B.float() @ A.float())
            e, e_ref = _nerr(eng.param_view(k).view(want.shape), want), _nerr(r32, want)
            worst["merged"] = max(worst["merged"], e)
            assert e <= 8 * e_ref + 2e-6, (k, e, e_ref)
        # everything that is not a target is frozen: the rest of the UNet, time_embed.*, spatial_volume.*
        assert torch.equal(eng.flat_params[~is_target], p_init[~is_target])
        assert (eng.flat_params[is_target] - p_init[is_target]).abs().max() > 0
    print(f"[lora] three steps vs torch.optim.AdamW: adapters {worst['p']:.2e}, exp_avg {worst['m']:.2e}, exp_avg_sq {worst['v']:.2e}, "
          f"norm {worst['norm']:.2e} relative, merged masters vs float64 {worst['merged']:.2e}")
    aux = [k for k in eng.param_table if not k.startswith(P)]
    assert aux and all(eng.param_view(k, grad=True).abs().max() > 0 for k in aux[:4])  # (the backward did write their gradients)
    assert worst["p"] <= 2e-6 and worst["m"] <= 2e-6 and worst["v"] <= 2e-6, worst
    assert worst["norm"] <= 1e-6, worst
    st["after3"] = dict(ab=eng.lora_params.clone(), m=eng.lora_m.clone(), v=eng.lora_v.clone(), opt=opt.state_dict(),
                        clip=opt.max_grad_norm)


def test_overflowed_step_changes_nothing_and_halves_the_scale(lora):
    m, st = lora
    eng = m.engine
    opt, _ = _reset(m, st)
    m.gradient_clip_val = None
    _step_inputs(m, st)
    opt.step()  # one clean step first: the moments are not zero
    _step_inputs(m, st)
    before = [t.clone() for t in (eng.lora_params, eng.lora_m, eng.lora_v, eng.flat_params)]
    eng.param_view(st["keys"][3], grad=True).view(-1)[5] = float("inf")
    opt.step()
    assert opt.steps_skipped == 1 and opt.steps_done == 1 and m.loss_scale == 32768.0
    for a, b in zip((eng.lora_params, eng.lora_m, eng.lora_v, eng.flat_params), before):
        assert torch.equal(a, b)
    m.loss_scale = 65536.0


def test_engine_runs_on_the_merged_weights(lora, plain):
    m, st = lora
    eng = m.engine
    ucfg, vcfg, N = st["cfg"]
    opt, _ = _reset(m, st)
    _step_inputs(m, st)
    opt.step()
    base_sd = gi.full_weights(ucfg, vcfg)
    lora_sd = m.lora_state_dict()
    assert set(lora_sd) == {f"lora.{k}.{w}" for k in st["keys"] for w in "AB"} | {"lora.rank", "lora.alpha"}
    sd = m.state_dict()
    assert set(sd) == set(base_sd)
    host = merge_lora(base_sd, lora_sd)
    d_w, bitwise = 0.0, True
    for k in st["keys"]:
        assert torch.equal(sd[k].cuda(), eng.param_view(k)) and not torch.equal(sd[k].cpu(), base_sd[k])
        bitwise = bitwise and torch.equal(sd[k].cpu(), host[k])
        d_w = max(d_w, _norm_diff(host[k], sd[k]))
    x, t, ctx, src = gi.unet_inputs(ucfg, Bv=2)
    x, t, ctx, src = x.cuda(), t.cuda(), ctx.cuda(), {k: v.cuda() for k, v in src.items()}
    plain.load_state_dict(sd)
    out_dev = plain.engine.unet_forward(x, t, ctx, src)
    assert torch.equal(out_dev, eng.unet_forward(x, t, ctx, src)), "the training engine's packs are those of its merged masters"
    plain.load_state_dict(base_sd, lora=lora_sd)
    out_host = plain.engine.unet_forward(x, t, ctx, src)
    d_out = _norm_diff(out_host, out_dev)
    print(f"[lora] device merge vs host merge: masters bitwise {bitwise}, worst normalised {d_w:.3e}; unet_forward {d_out:.3e}")
    if bitwise:
        assert torch.equal(out_host, out_dev)
    else:
        assert d_out <= 4 * d_w, (d_out, d_w)
    plain.load_state_dict(base_sd)
    out_base = plain.engine.unet_forward(x, t, ctx, src)
    assert not torch.equal(out_base, out_dev)
    plain.load_state_dict(base_sd, lora=lora_sd, lora_scale=0.0)
    assert torch.equal(plain.engine.unet_forward(x, t, ctx, src), out_base)
    # strength 0 on the training model: the initial masters, bit for bit, and back
    merged = eng.flat_params.clone()
    eng.lora_set_scale(0.0)
    assert torch.equal(eng.flat_params, st["before"]["p"])
    assert torch.equal(eng.unet_forward(x, t, ctx, src), out_base)
    eng.lora_set_scale(S)
    assert torch.equal(eng.flat_params, merged)


def test_adapter_and_optimiser_round_trip_resumes_bit_identically(lora, tmp_path):
    m, st = lora
    eng = m.engine
    ucfg, vcfg, N = st["cfg"]
    opt, _ = _reset(m, st)
    opt.max_grad_norm = 1e-3
    for _ in range(2):
        _step_inputs(m, st)
        opt.step()
    path = tmp_path / "adapter.pt"
    m.save_lora(str(path))
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    _step_inputs(m, st)
    opt.step()
    m3 = make_train_model(ucfg, vcfg, N, loss_scale=65536.0, recompute=True, deterministic=True)
    try:
        m3.learning_rate = m.learning_rate
        m3.load_lora(str(path))
        assert sorted(m3.engine.lora_table) == sorted(eng.lora_table) and m3.engine.lora_rank == RANK
        (opt3,), _ = m3.configure_optimizers()
        buf.seek(0)
        opt3.load_state_dict(torch.load(buf, weights_only=False))
        assert opt3.steps_done == 2 and opt3.max_grad_norm == 1e-3
        _step_inputs(m3, st)
        opt3.step()
        assert torch.equal(m3.engine.lora_params, eng.lora_params)
        assert torch.equal(m3.engine.lora_m, eng.lora_m) and torch.equal(m3.engine.lora_v, eng.lora_v)
        assert torch.equal(m3.engine.flat_params, eng.flat_params)
    finally:
        m3.engine.close()


def test_identical_steps_are_bit_identical(lora):
    m, st = lora
    eng = m.engine
    got = []
    for _ in range(2):
        opt, _ = _reset(m, st)
        opt.max_grad_norm = 1e-3
        for _ in range(2):
            _step_inputs(m, st)
            opt.step()
        got.append([t.clone() for t in (eng.lora_params, eng.lora_grads, eng.lora_m, eng.lora_v, eng.flat_params)])
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert (got[0][0] - st["AB"]).abs().max() > 0


def test_errors(lora, plain):
    m, st = lora
    with pytest.raises((RuntimeError, ValueError)):
        plain.enable_lora(rank=4)
    for rank in (0, 65):
        with pytest.raises(ValueError):
            m.enable_lora(rank=rank)
    with pytest.raises(ValueError):
        m.enable_lora(rank=4, targets=["*.no_such_layer.weight"])
    with pytest.raises(ValueError):
        m.enable_lora(rank=4, targets=["*.in_layers.2.weight"])  # 3x3 convolutions
    assert m.lora_enabled and m.engine.lora_rank == RANK  # the failed calls left the adapters alone
    ucfg, vcfg, N = st["cfg"]
    with pytest.raises(ValueError):
        make_train_model(ucfg, vcfg, N, use_ema=True, lora_rank=4)
    # the library checks too
    eng = m.engine
    import ctypes as C
    bad = (C.c_char_p * 1)((P + "input_blocks.1.0.in_layers.2.weight").encode())
    assert eng.lib.mvd_lora_attach(eng._ctx, bad, 1, 4, 4.0) != 0
    good = (C.c_char_p * 1)(st["keys"][0].encode())
    assert eng.lib.mvd_lora_attach(eng._ctx, good, 1, 65, 4.0) != 0
    assert eng.lib.mvd_lora_target_count(eng._ctx) == len(st["keys"])


def test_detach_restores_or_keeps_the_merged_weights(lora):
    """Last in the file: it drops the fixture's adapters."""
    m, st = lora
    eng = m.engine
    opt, _ = _reset(m, st)
    _step_inputs(m, st)
    opt.step()
    merged = eng.flat_params.clone()
    assert not torch.equal(merged, st["before"]["p"])
    m.disable_lora(keep_merged=True)
    assert not m.lora_enabled and eng.lora_params is None and torch.equal(eng.flat_params, merged)
    (opt2,), _ = m.configure_optimizers()
    assert type(opt2).__name__ == "ArenaAdamW"
    m.enable_lora(rank=2, targets=["*.attn1.to_q.weight"])  # W0 is now the merged model
    eng.lora_view(sorted(eng.lora_table)[0], "B").fill_(0.5)
    eng.lora_set_scale(1.0)
    assert not torch.equal(eng.flat_params, merged)
    m.disable_lora()
    assert torch.equal(eng.flat_params, merged)
    loss = _step_inputs(m, st)
    assert torch.isfinite(loss)

"""Optimiser step with gradient clipping + EMA on the full-width arena: fused against what a user composes today.

  (a) unfused: flat_grads.norm(); flat_grads.mul_(coef); mvd_train_adamw_step; flat_ema.lerp_(flat_params, 1 - d)
  (b) mvd_train_adamw_step_ex with max_grad_norm and ema_decay set (norm pass + one fused kernel)
  (c) mvd_train_adamw_step alone, for scale

all on the UNet group's range (one UNet backward pass marks it as carrying gradients), gradients seeded, no loss scaling.
HIP events around ITERS back-to-back repetitions, the three forms alternating, after a warm-up, in one process.  Bytes per
element by the algorithm: (a) 4 + 8 + 28 + 12 = 52, (b) 4 + 36 = 40, (c) 28.  Writes profiles/train_clip_ema.json.

python tools/train_clip_ema_bench.py [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import unet_kwargs
from morphablediffusion_amd import lib as L
from morphablediffusion_amd.model import SyncMultiviewDiffusion
from morphablediffusion_amd.spec import UNetConfig, VolumeConfig, full_manifest
from morphablediffusion_amd.weights import seeded_state_dict

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", "profiles", "train_clip_ema.json")
WARMUP, ROUNDS, ITERS = 2, 5, 4
N = 16
ucfg, vcfg = UNetConfig(), VolumeConfig(num_views=N)
m = SyncMultiviewDiffusion(unet_config={"target": "x.DepthWiseAttention", "params": unet_kwargs(ucfg)}, finetune_unet=True, view_num=N,
                           image_size=256, workspace_gb=64.0, train_mode=True, loss_scale=1.0)
m.load_state_dict(seeded_state_dict(full_manifest(ucfg, vcfg), 7))
eng = m.engine
eng.ensure_moments()
eng.ensure_ema()
# one UNet forward + backward at batch 1: the UNet group now counts as carrying gradients (values are replaced below)
g = torch.Generator().manual_seed(1)
s = ucfg.image_size
x = torch.randn(1, ucfg.in_channels, s, s, generator=g)
src = {s >> l: torch.randn(1, c, (48 * s // 32) >> l, s >> l, s >> l, generator=g) for l, c in enumerate(ucfg.volume_dims)}
eng.zero_grad()
eng.train_unet_step(x, torch.tensor([481]), torch.randn(1, 1, ucfg.context_dim, generator=g), src,
                    torch.randn(1, ucfg.out_channels, s, s, generator=g))
hi = min(o for k, (o, n, sh) in eng.param_table.items() if not k.startswith("model.diffusion_model."))
G, Pm, E = eng.flat_grads[:hi], eng.flat_params[:hi], eng.flat_ema[:hi]
G.normal_(generator=torch.Generator(device="cuda").manual_seed(2)).mul_(1e-3)
MAX_NORM, DECAY = 0.5 * G.double().norm().item(), 0.9999
ARGS = (eng._ctx, 1e-6, 1e-5, 0.9, 0.999, 1e-8, 0.01)
stream = torch.cuda.current_stream().cuda_stream
step = [0]


def unfused():
    step[0] += 1
    coef = torch.clamp(MAX_NORM / (G.norm() + 1e-6), max=1.0)  # stays on the device, as clip_grad_norm_ keeps it
    G.mul_(coef)
    L.check(eng.lib.mvd_train_adamw_step(*ARGS, step[0], 1.0, 1, None, stream))
    E.lerp_(Pm, 1.0 - DECAY)


def fused():
    step[0] += 1
    L.check(eng.lib.mvd_train_adamw_step_ex(*ARGS, step[0], 1.0, 1, None, MAX_NORM, DECAY, None, stream))


def plain():
    step[0] += 1
    L.check(eng.lib.mvd_train_adamw_step(*ARGS, step[0], 1.0, 1, None, stream))


FORMS = {"a_unfused": (unfused, 52), "b_fused": (fused, 40), "c_plain_step": (plain, 28)}
ms = {k: [] for k in FORMS}
for r in range(WARMUP + ROUNDS):
    for name, (fn, _) in FORMS.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        e1.synchronize()
        if r >= WARMUP:
            ms[name].append(e0.elapsed_time(e1) / ITERS)
res = {"elements": int(hi), "rounds": ROUNDS, "iters_per_round": ITERS, "csrc_sha16": L.csrc_sha16(), "forms": {}}
for name, (_, bpe) in FORMS.items():
    t = sorted(ms[name])[len(ms[name]) // 2]
    res["forms"][name] = {"ms_median": round(t, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                          "bytes_per_element": bpe, "tb_per_s": round(bpe * hi / (t * 1e-3) / 1e12, 3)}
res["b_over_a"] = round(res["forms"]["b_fused"]["ms_median"] / res["forms"]["a_unfused"]["ms_median"], 4)
res["b_over_a_byte_model"] = round(40 / 52, 4)
res["b_within_0.9_of_a"] = bool(res["b_over_a"] <= 0.9)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))

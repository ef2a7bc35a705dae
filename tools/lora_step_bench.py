"""LoRA optimiser step on the full-width model against the full fine-tuning step, and the two LoRA kernels on their own.

  (a) lora_step    LoraAdamW.step(): project, norm pass, AdamW on the adapter arenas, merge, re-pack
  (b) full_step    ArenaAdamW.step() with finetune_unet=True (the step of the parent commit): norm pass / AdamW over the UNet's
                   range of the four arenas, re-pack
  (c) project      mvd_lora_project alone    algorithmic bytes: dW read once, the partial sums written and read, A, B, gA, gB
  (d) merge        mvd_lora_set_scale alone  algorithmic bytes: W0 read, W written, A, B
  (e) repack       the re-pack alone, which (a) and (b) share

One model, one process: default targets, rank RANK, loss scale 65536 and clipping on in both steps.  One UNet forward + backward
at batch 1 marks the UNet group as carrying gradients; the gradient arena is then filled with seeded noise.  HIP events around ITERS
back-to-back repetitions, the forms alternating round by round after a warm-up; per form the median and the spread (max - min) of
the rounds.  Writes profiles/lora_step_time.json.

python tools/lora_step_bench.py [out.json] [rank]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import unet_kwargs
from morphablediffusion_amd import lib as L
from morphablediffusion_amd.model import ArenaAdamW, LoraAdamW, SyncMultiviewDiffusion
from morphablediffusion_amd.spec import UNetConfig, VolumeConfig, full_manifest
from morphablediffusion_amd.weights import seeded_state_dict

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", "profiles", "lora_step_time.json")
RANK = int(sys.argv[2]) if len(sys.argv) > 2 else 8
WARMUP, ROUNDS, ITERS = 2, 7, 4
N = 16
ucfg, vcfg = UNetConfig(), VolumeConfig(num_views=N)
m = SyncMultiviewDiffusion(unet_config={"target": "x.DepthWiseAttention", "params": unet_kwargs(ucfg)}, finetune_unet=True, view_num=N,
                           image_size=256, workspace_gb=64.0, train_mode=True, loss_scale=65536.0)
m.load_state_dict(seeded_state_dict(full_manifest(ucfg, vcfg), 7))
eng = m.engine
eng.ensure_moments()
g = torch.Generator().manual_seed(1)
s = ucfg.image_size
x = torch.randn(1, ucfg.in_channels, s, s, generator=g)
src = {s >> l: torch.randn(1, c, (48 * s // 32) >> l, s >> l, s >> l, generator=g) for l, c in enumerate(ucfg.volume_dims)}
eng.zero_grad()
eng.train_unet_step(x, torch.tensor([481]), torch.randn(1, 1, ucfg.context_dim, generator=g), src,
                    torch.randn(1, ucfg.out_channels, s, s, generator=g))
hi = min(o for k, (o, n, sh) in eng.param_table.items() if not k.startswith("model.diffusion_model."))
eng.flat_grads[:hi].normal_(generator=torch.Generator(device="cuda").manual_seed(2)).mul_(1e-3 * 65536.0)
full = ArenaAdamW(m, [torch.nn.Parameter(eng.flat_params[:hi])], lr=1e-7, max_grad_norm=1.0)  # (its step works on the arenas)
keys = m.enable_lora(rank=RANK)
gen = torch.Generator(device="cuda").manual_seed(3)
for k in keys:  # B != 0, so that the projection and the merge see ordinary numbers
    eng.lora_view(k, "B").normal_(generator=gen).mul_(1e-3)
eng.lora_set_scale(eng.lora_scale)
lora = LoraAdamW(m, lr=1e-7, max_grad_norm=1.0)
w_elems = sum(o * i for _, _, o, i in eng.lora_table.values())
ab_elems = sum(RANK * i + o * RANK for _, _, o, i in eng.lora_table.values())
part_elems = sum(-(-o // 32) * RANK * i + -(-i // 128) * o * RANK for _, _, o, i in eng.lora_table.values())
BYTES = {"project": 4 * (w_elems + 2 * part_elems + 2 * ab_elems), "merge": 4 * (2 * w_elems + ab_elems)}


def project():
    eng.lora_project()


def merge():
    L.check(eng.lib.mvd_lora_set_scale(eng._ctx, eng.lora_scale, torch.cuda.current_stream().cuda_stream))


FORMS = {"lora_step": lora.step, "full_step": full.step, "project": project, "merge": merge, "repack": eng.repack}
ms = {k: [] for k in FORMS}
for r in range(WARMUP + ROUNDS):
    for name, fn in FORMS.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        e1.synchronize()
        if r >= WARMUP:
            ms[name].append(e0.elapsed_time(e1) / ITERS)
assert lora.steps_skipped == 0 and full.steps_skipped == 0, "a timed step was skipped for a non-finite gradient"
res = {"rank": RANK, "targets": len(keys), "target_weights": int(w_elems), "adapter_elements": int(ab_elems),
       "unet_elements": int(hi), "rounds": ROUNDS, "iters_per_round": ITERS, "csrc_sha16": L.csrc_sha16(), "forms": {}}
for name in FORMS:
    t = sorted(ms[name])[len(ms[name]) // 2]
    res["forms"][name] = {"ms_median": round(t, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                          "ms_spread": round(max(ms[name]) - min(ms[name]), 4)}
    if name in BYTES:
        res["forms"][name]["algorithmic_bytes"] = int(BYTES[name])
        res["forms"][name]["gb_per_s"] = round(BYTES[name] / (t * 1e-3) / 1e9, 1)
f = res["forms"]
res["lora_minus_full_ms"] = round(f["lora_step"]["ms_median"] - f["full_step"]["ms_median"], 4)
res["same_arm_spread_ms"] = round(max(f["lora_step"]["ms_spread"], f["full_step"]["ms_spread"]), 4)
res["lora_no_slower_beyond_spread"] = bool(res["lora_minus_full_ms"] <= res["same_arm_spread_ms"])
res["project_plus_merge_over_repack"] = round((f["project"]["ms_median"] + f["merge"]["ms_median"]) / f["repack"]["ms_median"], 4)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))

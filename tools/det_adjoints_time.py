"""Time of the conditioner's backward pass in the atomic (default) and in the deterministic mode (development aid).

    python tools/det_adjoints_time.py [B] [--tree DIR] [--small] [--out FILE]

Full-width model, B samples of a 5023-vertex mesh, 16 views: mvd_train_conditioner_backward_batch on fixed inputs, each timed
call bracketed by device synchronisation, the two modes alternating (ROUNDS rounds of REPS calls each, after a warm-up of both).
Prints one JSON line {"atomic_ms": [per round], "deterministic_ms": [...]} (medians per round) and, with --out, writes it.
--tree DIR imports the package from another checkout (the parent commit: it has no deterministic mode, only "atomic_ms" is
reported) so that both builds can be timed on one box, one after the other, in one session.  --small: the 64-channel UNet (the
conditioner is the same; for a quick look)."""
import json
import os
import statistics
import sys
import time

args = sys.argv[1:]
tree = os.path.abspath(args[args.index("--tree") + 1]) if "--tree" in args else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = args[args.index("--out") + 1] if "--out" in args else None
small = "--small" in args
B = int(args[0]) if args and args[0].isdigit() else 8
sys.path.insert(0, tree)
import torch  # noqa: E402
from bench import unet_kwargs  # noqa: E402
from morphablediffusion_amd import synthetic  # noqa: E402
from morphablediffusion_amd.model import SyncMultiviewDiffusion  # noqa: E402
from morphablediffusion_amd.spec import UNetConfig, VolumeConfig, full_manifest  # noqa: E402
from morphablediffusion_amd.weights import seeded_state_dict  # noqa: E402

N, ROUNDS, REPS = 16, 5, 4
ucfg, vcfg = (UNetConfig(model_channels=64) if small else UNetConfig()), VolumeConfig(num_views=N)
m = SyncMultiviewDiffusion(unet_config={"target": "x.DepthWiseAttention", "params": unet_kwargs(ucfg)}, finetune_unet=True, view_num=N,
                           image_size=256, workspace_gb=16.0 if small else 96.0, train_mode=True)
m.load_state_dict(seeded_state_dict(full_manifest(ucfg, vcfg), 7))
b0 = synthetic.make_batch(N, "perspective", 5023, mesh_seed=1)
batch = {k: v.repeat(B, *([1] * (v.dim() - 1))).clone().cuda() for k, v in b0.items()}
g = torch.Generator().manual_seed(1)
x_noisy = (torch.randn(B, N, 4, 32, 32, generator=g) * 0.8).cuda()
ts = torch.randint(0, 1000, (B,), generator=g).tolist()
ti = torch.randint(0, N, (B,), generator=g).tolist()
m.train()
v_embed = m.get_viewpoint_embedding(batch)
dsrc, d, s = {}, vcfg.frustum_volume_depth, vcfg.frustum_volume_size
for lvl in range(4):
    dsrc[s] = (torch.randn(B, vcfg.frustum_dims[lvl], d, s, s, generator=g) * 0.5 ** lvl).cuda()
    d, s = (d - 1) // 2 + 1, (s - 1) // 2 + 1
m.spatial_volume._set_sample(batch, 0)  # uploads every sample's tables to its slot
eng = m.engine
has_mode = hasattr(eng, "train_set_deterministic")


def one():
    eng.zero_grad()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.train_conditioner_backward_batch(list(range(B)), x_noisy, ts, v_embed, ti, dsrc)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


modes = [("atomic_ms", False)] + ([("deterministic_ms", True)] if has_mode else [])
res = {name: [] for name, _ in modes}
for rnd in range(ROUNDS + 1):  # round 0 warms both modes up
    for name, det in modes:
        if has_mode:
            eng.train_set_deterministic(det)
        t = [one() for _ in range(REPS)]
        if rnd:
            res[name].append(round(statistics.median(t), 3))
res.update(B=B, width=ucfg.model_channels, tree=os.path.basename(tree), rounds=ROUNDS, reps=REPS)
line = json.dumps(res)
print(line)
if out:
    with open(out, "w") as f:
        f.write(line + "\n")

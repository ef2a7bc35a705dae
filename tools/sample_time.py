"""Wall time per generated sample at the headline shape (16 views, 256 x 256, CFG 2.0, one GPU, seeded random weights):
DDIM-50 (the reference's sampler) against DPM-Solver++(2M) with 15 and 20 model evaluations on the logSNR grid.

    python tools/sample_time.py [--reps 5] [--arms ddim50,dpmpp2m15,dpmpp2m20] [--timeout 300] [--out profiles/sample_time.json]

Each arm runs in a child process of its own under its own time limit; an arm that fails or runs out of time is reported as
such and ends the run (nothing more is started on the device).  In an arm: one untimed sample() warms every shape, then `reps` timed sample() calls, each
ended by a device synchronise; reported are the median and min wall time per sample and the median per model evaluation.
The VAE decode is not included (it is the same for every sampler)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = {"ddim50": ("ddim", 50), "dpmpp2m15": ("dpmpp_2m", 15), "dpmpp2m20": ("dpmpp_2m", 20), "dpmpp2msde20": ("dpmpp_2m_sde", 20)}


def run_arm(name, reps):
    sys.path.insert(0, ROOT)
    import torch
    from morphablediffusion_amd import synthetic
    from morphablediffusion_amd.model import SyncDDIMSampler, SyncDPMSolverSampler, SyncMultiviewDiffusion
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig, full_manifest
    from morphablediffusion_amd.weights import seeded_state_dict

    kind, steps = ARMS[name]
    N, dev = 16, "cuda:0"
    ucfg, vcfg = UNetConfig(image_size=32), VolumeConfig(num_views=N)
    kw = dict(volume_dims=list(ucfg.volume_dims), image_size=32, in_channels=8, out_channels=4, model_channels=ucfg.model_channels,
              attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8,
              use_spatial_transformer=True, transformer_depth=1, context_dim=768, use_checkpoint=True, legacy=False)
    model = SyncMultiviewDiffusion(unet_config={"target": "ldm.models.diffusion.attention.DepthWiseAttention", "params": kw},
                                   view_num=N, image_size=256, cfg_scale=2.0, device=dev, workspace_gb=48.0)
    model.load_state_dict(seeded_state_dict(full_manifest(ucfg, vcfg), 7))
    model.eval()
    sampler = (SyncDDIMSampler(model, steps, "uniform", 1.0, latent_size=32) if kind == "ddim"
               else SyncDPMSolverSampler(model, steps, kind, latent_size=32))
    batch = {k: v.to(dev) for k, v in synthetic.make_batch(N, "perspective", 5023, mesh_seed=1).items()}
    _, x_in, clip = [t.to(dev) for t in synthetic.make_latents(N, 32, seed=6033)]
    times = []
    with torch.no_grad():
        for r in range(reps + 1):
            gen = torch.Generator(device=dev).manual_seed(6033)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, _ = sampler.sample({"x": x_in}, clip, unconditional_scale=2.0, batch_view_num=N, batch=batch, generator=gen)
            torch.cuda.synchronize()
            if r:
                times.append(time.perf_counter() - t0)
    assert torch.isfinite(x).all()
    med = statistics.median(times)
    return {"arm": name, "sampler": kind, "evaluations": steps, "reps": reps, "sample_s_median": med, "sample_s_min": min(times),
            "sample_s_all": times, "per_evaluation_ms_median": 1e3 * med / steps, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arms", default="ddim50,dpmpp2m15,dpmpp2m20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_time.json"))
    ap.add_argument("--arm", help=argparse.SUPPRESS)  # child process: run one arm, print its JSON line
    args = ap.parse_args()
    if args.arm:
        print("ARM " + json.dumps(run_arm(args.arm, args.reps)), flush=True)
        return
    results = []
    for name in args.arms.split(","):
        if name not in ARMS:
            raise SystemExit(f"unknown arm {name!r} (one of {sorted(ARMS)})")
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", name, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=args.timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("ARM ")]
            res = json.loads(line[-1][4:]) if p.returncode == 0 and line else \
                {"arm": name, "error": f"exit {p.returncode}", "stderr_tail": p.stderr[-1500:]}
        except subprocess.TimeoutExpired:
            res = {"arm": name, "error": f"timed out after {args.timeout:.0f} s"}
        print(json.dumps(res), flush=True)
        results.append(res)
        if "error" in res:
            break  # a failed or hung arm: start nothing more on the device
    base = next((r for r in results if r.get("arm") == "ddim50" and "error" not in r), None)
    if base:
        for r in results:
            if "error" not in r:
                r["speedup_vs_ddim50"] = base["sample_s_median"] / r["sample_s_median"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"shape": "16 views, 256x256 (32x32 latents), CFG 2.0, batch_view_num 16, 1 GPU", "arms": results}, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

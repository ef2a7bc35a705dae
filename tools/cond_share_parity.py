"""Bit identity of the conditioner's forward and backward between two builds of the library (development aid).

    MVD_LIB_PATH=<library A> python tools/cond_share_parity.py --hashes a.json
    MVD_LIB_PATH=<library B> python tools/cond_share_parity.py --hashes b.json
    python tools/cond_share_parity.py --compare a.json b.json [--out profiles/cond_share_parity.json]

The first form runs a fixed seeded case at the shapes of tests/test_gpu_train_deterministic.py::
test_conditioner_backward_repeats_bit_for_bit (SMALL_UNET, N = 4, 32 x 32 latents, the 500-vertex and the 900-vertex
duplicate-voxel mesh, timestep 421, target view 2) and writes the sha256 of
 (a) the conditioner backward in the deterministic mode: dvol, dfused, dfeats, dtemb and the whole gradient arena of the
     single-sample call on either mesh, and the arena of a two-sample call and of a 17-sample call (the second chunk of the frustum
     stage) over the two meshes.  dL/d(frustum volume) of the four levels, which the call accumulates in place, lives in the
     workspace and is not visible through the C ABI; every gradient of the frustum network is computed from it;
 (b) the inference forward: the layered 2-D encoder (MVD_NO_FUSED_ENC=1, in a child process: the switch is read once), the sparse CNN
     with running and with batch statistics, the frustum volumes of one sample and of a batch of two, and SpatialTime3DNet on a
     use_spatial_volume context with either encoder form.
The atomic (default) mode does not repeat bit for bit against itself and is left to the tolerance tests."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, TIMESTEP, TARGET = 4, 421, 2


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def meshes():
    import torch
    from morphablediffusion_amd import batch as BT
    from morphablediffusion_amd import synthetic
    a = synthetic.make_batch(N, "perspective", 500, mesh_seed=1)
    b = BT.build_batch(torch.zeros(256, 256, 3), synthetic.ellipsoid_mesh(900, 3, radii=(0.09, 0.11, 0.10), dedup=False), num_views=N)
    return a, {k: v for k, v in b.items() if torch.is_tensor(v)}


def set_slot(eng, batch, slot):
    eng.select_sample(slot)
    eng.set_mesh(batch["vertices"][0], batch["coord"][0], batch["out_sh"][0], batch["bounds"][0])
    eng.set_cameras(batch["target_K"][0], batch["target_RT"][0])


def dsrc_for(vcfg, B, gen):
    import torch
    out, d, s = {}, vcfg.frustum_volume_depth, vcfg.frustum_volume_size
    for lvl in range(4):
        out[s] = (torch.randn(B, vcfg.frustum_dims[lvl], d, s, s, generator=gen) * (0.5 ** lvl)).cuda()
        d, s = (d - 1) // 2 + 1, (s - 1) // 2 + 1
    return out


def backward_hashes(H):
    import torch
    from morphablediffusion_amd.lib import MvdError
    from morphablediffusion_amd.spec import VolumeConfig
    from oracle import mvd_oracle as O
    from tests import golden_inputs as gi
    from tests.test_gpu_train import make_train_model
    vcfg = VolumeConfig(num_views=N)
    both = meshes()
    m = make_train_model(gi.SMALL_UNET, vcfg, N, workspace_gb=16.0, deterministic=True)
    eng = m.engine
    gen = torch.Generator().manual_seed(9)
    x = (torch.randn(17, N, 4, 32, 32, generator=gen) * 0.8).cuda()
    v_embed = [O.viewpoint_embedding(b)[0].cuda() for b in both]
    for name, batch, ve in zip(("500 vertices", "900 vertices, duplicate voxels"), both, v_embed):
        set_slot(eng, batch, 0)
        eng.zero_grad()
        out = eng.train_conditioner_backward(x[0], TIMESTEP, ve, TARGET, dsrc_for(vcfg, 1, gen), debug=True)
        torch.cuda.synchronize()
        for tag, t in zip(("dvol", "dfused", "dfeats", "dtemb", "gradient arena"), out + [eng.flat_grads]):
            H[f"backward, one sample, {name}: {tag}"] = sha(t)
    for B in (2, 17):
        for slot in range(B):
            set_slot(eng, both[slot % 2], slot)
        ve = torch.stack([v_embed[slot % 2] for slot in range(B)])
        eng.zero_grad()
        try:
            eng.train_conditioner_backward_batch(list(range(B)), x[:B], [TIMESTEP + 7 * i for i in range(B)], ve,
                                                 [(TARGET + i) % N for i in range(B)], dsrc_for(vcfg, B, gen))
        except MvdError as e:  # the 17-sample tape does not fit the workspace here
            H[f"backward, {B} samples: gradient arena"] = f"not run: {e}"
            continue
        torch.cuda.synchronize()
        H[f"backward, {B} samples: gradient arena"] = sha(eng.flat_grads)
    eng.close()


def forward_hashes(H):
    import torch
    from morphablediffusion_amd.spec import VolumeConfig
    from oracle import mvd_oracle as O
    from tests import golden_inputs as gi
    from tests.test_gpu_model import make_model
    vcfg = VolumeConfig(num_views=N)
    both = meshes()
    m = make_model(gi.SMALL_UNET, vcfg, N, workspace_gb=4.0)
    eng = m.engine
    gen = torch.Generator().manual_seed(11)
    x = (torch.randn(N, 4, 32, 32, generator=gen) * 0.8).cuda()
    t_embed = m.embed_time(torch.tensor([TIMESTEP, TIMESTEP + 7], device="cuda"))
    volumes, v_rows = [], []
    for slot, batch in enumerate(both):
        v_embed = O.viewpoint_embedding(batch)[0].cuda()
        set_slot(eng, batch, slot)
        fused = eng.vertex_features(x, t_embed[slot], v_embed, torch.arange(N))
        for train in (False, True):
            H[f"forward, mesh {slot}: sparse_dense train_mode={int(train)}"] = sha(eng.stage_sparse_dense(fused, train=train))
        volumes.append(eng.volume_from_fused(fused))
        idx = torch.arange(0, 2)
        for res, v in eng.frustum_volumes(t_embed[slot], v_embed[idx], idx).items():
            H[f"forward, mesh {slot}: frustum_volumes {res}"] = sha(v)
        v_rows.append(v_embed[TARGET + slot])
    fd = eng.frustum_volumes_batch([0, 1], torch.stack(volumes), t_embed, torch.stack(v_rows), torch.tensor([TARGET, TARGET + 1]))
    for res, v in fd.items():
        H[f"forward: frustum_volumes_batch {res}"] = sha(v)
    eng.close()


def encoder_hashes(H, tag):
    """The 2-D encoder alone and SpatialTime3DNet behind it, in the encoder form the environment asks for."""
    import torch
    from oracle import mvd_oracle as O
    from tests import test_spatial_volume_cpu as R
    from tests.test_gpu_spatial_volume import NET_CASES, set_sample, stage_config, stage_engine, stage_weights
    V, S, dims = NET_CASES["v16"]
    vcfg = stage_config(V, S, dims)
    W = stage_weights(vcfg, "init")
    eng = stage_engine(vcfg, W, S)
    batch = R.stage_batch(N, "perspective", 300, 8 * S)
    set_sample(eng, batch)
    x, _, v_embed = R.spatial_time_inputs(N, S, 17)
    t_embed = O.embed_time(W, torch.tensor([TIMESTEP]))
    xs, te, ve = x[0].cuda(), t_embed[0].cuda(), v_embed[0].cuda()
    H[f"forward, {tag} encoder: stage_target_encoder"] = sha(eng.stage_target_encoder(xs, te, ve))
    eng.volume_from_fused(eng.vertex_features(xs, te, ve, torch.arange(N)))
    H[f"forward, {tag} encoder: spatial_time_volume"] = sha(eng.spatial_time_volume(xs, te, ve))
    eng.close()


def compare(a_path, b_path, out):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    keys = sorted(set(a["hashes"]) | set(b["hashes"]))
    differ = [k for k in keys if a["hashes"].get(k) != b["hashes"].get(k)]
    not_run = [k for k in keys if str(a["hashes"].get(k, "")).startswith("not run")]
    what = ("sha256 of the conditioner's deterministic backward outputs and inference forward outputs under two builds of the "
            "library on one MI355X in one session (tools/cond_share_parity.py)")
    with open(out, "w") as f:
        json.dump({"what": what, "a": a, "b": b, "differ": differ, "not_run": not_run,
                   "verdict": "identical" if not differ and not not_run else "NOT identical" if differ else "identical where run"}, f, indent=1)
    print(f"{len(keys)} hashes, {len(differ)} differ, {len(not_run)} not run -> {out}")
    return 1 if differ else 0


def main():
    args = sys.argv[1:]
    if "--compare" in args:
        i = args.index("--compare")
        out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "cond_share_parity.json")
        raise SystemExit(compare(args[i + 1], args[i + 2], out))
    H = {}
    if "--layered-child" in args:  # MVD_NO_FUSED_ENC=1 is set by the parent
        encoder_hashes(H, "layered")
        print("HASHES " + json.dumps(H))
        return
    backward_hashes(H)
    forward_hashes(H)
    encoder_hashes(H, "one-launch")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--layered-child"], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, MVD_NO_FUSED_ENC="1"))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("HASHES ")]
    if r.returncode or not line:
        raise SystemExit(f"the layered-encoder child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    H.update(json.loads(line[0][len("HASHES "):]))
    from morphablediffusion_amd import lib as L
    out = args[args.index("--hashes") + 1]
    with open(out, "w") as f:
        json.dump({"library": os.path.basename(L.LIB_PATH), "hashes": H}, f, indent=1)
    print(f"{len(H)} hashes -> {out}")


if __name__ == "__main__":
    main()

"""GPU: mvd_op_image_metrics (csrc/k_metrics.hip) through metrics.image_metrics against the numpy oracle tests/image_metrics_ref.py,
and the callers built on it (evaluate_views, validation_step's val_metrics, generate_face --gt_dir).

Bounds: sse, sae and the background count are exact integers on both sides and must be EQUAL.  ssim within 1e-12: both sides
evaluate S from identical integers in float64 -- about a dozen operations per pixel and a tree over at most 62 500 terms leave
about 1e-14; the margin covers FMA contraction.  Views within one call hold different seeded data."""
import json

import numpy as np
import pytest
import torch

from morphablediffusion_amd import lib as L
from morphablediffusion_amd import metrics as M
from tests import image_metrics_ref as R
from tests.test_image_metrics_cpu import abi_error_cases

pytestmark = pytest.mark.gpu
SSIM_TOL = 1e-12
worst_ssim = [0.0]


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ssim():
    yield
    print(f"\n[image metrics] max |ssim - oracle| over the whole file: {worst_ssim[0]:.2e} (bound {SSIM_TOL:.0e})")


def _np(res):
    return {k: v.detach().cpu().numpy() for k, v in res.items() if k != "x_sample"}


# exact equality is claimed for the sums themselves, so they are read through op_image_metrics (image_metrics returns sse / 3HW)
def raw(prd, tgt, mask=None, mode=None):
    from morphablediffusion_amd.engine import op_image_metrics
    out = op_image_metrics(prd, tgt, mask, mode).cpu().numpy()
    return {k: out[:, i] for i, k in enumerate(("ssim", "sse", "sae", "background", "nonfinite"))}


def check_raw(got, ref, what):
    bad = [f"{what}: {k} {got[k]} != {ref[k]}" for k in ("sse", "sae", "background", "nonfinite")
           if not np.array_equal(got[k], ref[k], equal_nan=True)]
    d = np.abs(got["ssim"] - ref["ssim"])
    if not np.array_equal(np.isnan(got["ssim"]), np.isnan(ref["ssim"])) or (np.nan_to_num(d) > SSIM_TOL).any():
        bad.append(f"{what}: ssim {got['ssim']} vs {ref['ssim']}, |diff| {d}")
    if np.isfinite(d).any():
        worst_ssim[0] = max(worst_ssim[0], float(np.nanmax(d)))
    return bad


def _shape_case(H, W, V=3):
    prd, tgt = R.make_views(V, H, W, seed=H * 1000 + W)
    mask = (np.random.RandomState(H + W).rand(V, H, W) < 0.3).astype(np.uint8)
    bad = check_raw(raw(torch.from_numpy(prd).cuda(), torch.from_numpy(tgt).cuda()), R.image_metrics_ref(prd, tgt), f"{H}x{W}")
    # with a mask: the owned-pixel sums and the whitened halo at every tile edge
    bad += check_raw(raw(torch.from_numpy(prd).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(mask).cuda()),
                     R.image_metrics_ref(prd, tgt, mask, "explicit"), f"{H}x{W} masked")
    return bad


@pytest.mark.parametrize("H,W", [(7, 7), (8, 13), (70, 75), (129, 200), (256, 256)])
def test_shapes(H, W):
    bad = _shape_case(H, W)
    print(f"[image metrics] {H}x{W}: max |ssim - oracle| so far {worst_ssim[0]:.2e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("axis", ["W", "H"])
def test_every_tile_edge(axis):
    """(9, W) for every W in 7..80 and (H, 9) for every H in 7..80: with tiles of at most 64 centres this covers every position of
    a tile edge, the halo and the ragged last tile along each axis."""
    bad = []
    for n in range(7, 81):
        bad += _shape_case(9, n) if axis == "W" else _shape_case(n, 9)
    print(f"[image metrics] sweep along {axis}: max |ssim - oracle| so far {worst_ssim[0]:.2e}")
    assert not bad, "\n".join(bad[:20])


def test_dtype_and_layout_combinations_agree_bit_for_bit():
    H, W = 40, 37
    prd, tgt = R.make_views(3, H, W, seed=5)
    ref = R.image_metrics_ref(prd, tgt)
    pf, tf = R.bytes_to_float(prd), R.bytes_to_float(tgt)
    preds = {"float nchw": torch.from_numpy(pf).permute(0, 3, 1, 2).contiguous(), "float nhwc": torch.from_numpy(pf),
             "uint8 nchw": torch.from_numpy(prd).permute(0, 3, 1, 2).contiguous(), "uint8 nhwc": torch.from_numpy(prd)}
    targets = {"float nhwc": torch.from_numpy(tf), "uint8 nhwc": torch.from_numpy(tgt)}
    outs, bad = {}, []
    for pn, p in preds.items():
        for tn, t in targets.items():
            outs[pn, tn] = raw(p.cuda(), t.cuda())
            bad += check_raw(outs[pn, tn], ref, f"pred {pn}, target {tn}")
    assert not bad, "\n".join(bad)
    first = outs["float nchw", "float nhwc"]
    for key, o in outs.items():
        for k in first:
            assert o[k].tobytes() == first[k].tobytes(), (key, k)
    # the public function: CPU inputs, half precision is converted to fp32, leading dimensions come back
    res = M.image_metrics(preds["uint8 nchw"].reshape(3, 1, 3, H, W), targets["uint8 nhwc"].reshape(3, 1, H, W, 3))
    assert all(v.shape == (3, 1) and v.dtype == torch.float64 and v.is_cuda for v in res.values())
    got = _np({k: v.reshape(3) for k, v in res.items()})
    assert got["ssim"].tobytes() == first["ssim"].tobytes()
    d = R.derived(ref, H, W)
    for k in ("mse", "mae", "psnr"):
        assert np.allclose(got[k], d[k], rtol=1e-15, atol=0), k


def test_masks():
    H, W, V = 41, 45, 4
    prd, tgt = R.make_views(V, H, W, seed=9)
    tgt[3] = 255  # view 3: an all-white target, fully masked below
    mask = (np.random.RandomState(1).rand(V, H, W) < 0.3).astype(np.uint8)
    mask[:, 0, :] = mask[:, -1, :] = 1  # border pixels: no window centre, still owned by a tile
    mask[0, :, 0] = mask[0, :, -1] = 1
    mask[3] = 1
    p, t = torch.from_numpy(prd).cuda(), torch.from_numpy(tgt).cuda()
    bad = check_raw(raw(p, t), R.image_metrics_ref(prd, tgt), "none")
    got = raw(p, t, torch.from_numpy(mask).cuda())
    bad += check_raw(got, R.image_metrics_ref(prd, tgt, mask, "explicit"), "explicit")
    assert got["sse"][3] == 0 and got["ssim"][3] == 1.0 and got["background"][3] == H * W
    res = M.image_metrics(p, t, torch.from_numpy(mask).bool())
    assert res["psnr"][3].item() == float("inf") and res["ssim"][3].item() == 1.0 and res["mse"][3].item() == 0.0
    # derived: a white frame, and interior pixels at 253 / 254 / 255 in one, two and three channels
    tgt2 = R.make_views(V, H, W, seed=10)[1]
    tgt2[:, :5] = tgt2[:, -5:] = 255
    tgt2[:, :, :5] = tgt2[:, :, -5:] = 255
    r = np.random.RandomState(2)
    for v in range(V):
        for n_ch in (1, 2, 3):
            for val in (253, 254, 255):
                for _ in range(6):
                    y, x = r.randint(5, H - 5), r.randint(5, W - 5)
                    tgt2[v, y, x, r.permutation(3)[:n_ch]] = val
    ref = R.image_metrics_ref(prd, tgt2, None, "white")
    frame = H * W - (H - 10) * (W - 10)
    assert ((ref["background"] > frame) & (ref["background"] < frame + 54)).all()  # some of the 54 interior hits count, not all
    bad += check_raw(raw(p, torch.from_numpy(tgt2).cuda(), None, "white"), ref, "white")
    assert not bad, "\n".join(bad)


def test_quantisation_on_the_device():
    v = R.bin_edge_values()  # [3,16,17]
    pred = np.stack([v, np.roll(v, 5, 2), v[::-1].copy()])  # three views [3,3,16,17], each with every bin edge
    tgt = np.empty((3, 16, 17, 3), np.uint8)
    tgt[0], tgt[1], tgt[2] = 128, 0, 255
    got = raw(torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda())
    ref = R.image_metrics_ref(pred, tgt, pred_layout="nchw")
    assert ref["nonfinite"].sum() == 0
    bad = check_raw(got, ref, "bin edges")
    assert not bad, "\n".join(bad)


def test_non_finite_values_poison_their_view_only():
    H, W = 20, 39
    prd, tgt = R.make_views(3, H, W, seed=3)
    pf = R.bytes_to_float(prd)
    clean = raw(torch.from_numpy(pf).cuda(), torch.from_numpy(tgt).cuda())
    pf[1, 0, 0, 1], pf[1, 10, 35, 2] = np.nan, np.inf  # a border pixel without a window centre, and one in the second tile
    got = raw(torch.from_numpy(pf).cuda(), torch.from_numpy(tgt).cuda())
    assert got["nonfinite"].tolist() == [0.0, 2.0, 0.0]
    for k in ("ssim", "sse", "sae", "background"):
        assert np.isnan(got[k][1]), k
        assert got[k][[0, 2]].tobytes() == clean[k][[0, 2]].tobytes(), k
    res = M.image_metrics(torch.from_numpy(pf), torch.from_numpy(tgt))
    assert all(torch.isnan(res[k][1]) for k in ("ssim", "psnr", "mse", "mae")) and res["nonfinite"][1].item() == 2
    assert not check_raw(got, R.image_metrics_ref(pf, tgt), "non-finite")
    tf = R.bytes_to_float(tgt)
    tf[2, 5, 5, 0] = -np.inf  # in the target
    assert raw(torch.from_numpy(prd).cuda(), torch.from_numpy(tf).cuda())["nonfinite"].tolist() == [0.0, 0.0, 1.0]


def test_two_calls_agree_bit_for_bit():
    prd, tgt = R.make_views(3, 129, 200, seed=11, kind="random")
    p, t = torch.from_numpy(R.bytes_to_float(prd)).cuda(), torch.from_numpy(tgt).cuda()
    a, b = raw(p, t, None, "white"), raw(p, t, None, "white")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_argument_errors_through_the_c_abi():
    lib = L.load()
    out = torch.full((1, 5), -7.0, dtype=torch.float64, device="cuda")
    img = torch.zeros(1, 3, 7, 7, device="cuda")
    for name, args in abi_error_cases(img.data_ptr()).items():
        args = tuple(out.data_ptr() if i == 11 and a is not None else a for i, a in enumerate(args))
        assert lib.mvd_op_image_metrics(*args) != 0, name
        assert lib.mvd_last_error().decode().startswith("mvd_op_image_metrics: "), name
    torch.cuda.synchronize()
    assert (out == -7.0).all()  # nothing was launched


# ---- the callers ----------------------------------------------------------------------------------------------------------
def test_evaluate_views_and_validation_metrics(tmp_path):
    """The small seeded model smoke() builds (N = 2), with the stand-in first stage / CLIP encoder of the sampler tests."""
    from morphablediffusion_amd import synthetic
    from morphablediffusion_amd.model import SyncMultiviewDiffusion
    from morphablediffusion_amd.spec import UNetConfig, VolumeConfig, full_manifest
    from morphablediffusion_amd.weights import seeded_state_dict
    from tests.test_gpu_sampler_dpm import _Clip, _Vae
    N = 2
    ucfg, vcfg = UNetConfig(model_channels=64), VolumeConfig(num_views=N)
    kw = dict(volume_dims=list(ucfg.volume_dims), image_size=32, in_channels=8, out_channels=4, model_channels=64,
              attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8,
              use_spatial_transformer=True, transformer_depth=1, context_dim=768, use_checkpoint=True, legacy=False)
    m = SyncMultiviewDiffusion(unet_config={"target": "ldm.models.diffusion.attention.DepthWiseAttention", "params": kw},
                               view_num=N, image_size=256, cfg_scale=2.0, workspace_gb=2.0, sample_steps=4, batch_view_num=2,
                               first_stage_model=_Vae(), clip_image_encoder=_Clip())
    try:
        m.load_state_dict(seeded_state_dict(full_manifest(ucfg, vcfg), 3))
        m.eval()
        batch = {k: v.cuda() for k, v in synthetic.make_batch(N, "perspective", 400, mesh_seed=2).items()}
        g = torch.Generator().manual_seed(8)
        batch["input_image"] = (torch.rand(1, 256, 256, 3, generator=g) * 2 - 1).cuda()
        with pytest.raises(ValueError):
            m.evaluate_views(batch)
        batch["target_image"] = (torch.rand(1, N, 256, 256, 3, generator=g) * 2 - 1).cuda()
        torch.manual_seed(21)
        x = m.sample(m.sampler, batch, m.cfg_scale, m.batch_view_num)
        want = M.image_metrics(x, batch["target_image"])
        torch.manual_seed(21)
        got = m.evaluate_views(batch)
        assert torch.equal(got["x_sample"], x) and got["ssim"].shape == (1, N)
        for k in want:
            assert torch.equal(got[k], want[k]), k
        ref = R.image_metrics_ref(x[0].cpu().numpy(), batch["target_image"][0].cpu().numpy(), pred_layout="nchw")
        direct = raw(x[0], batch["target_image"][0])
        assert not check_raw(direct, ref, "model") and got["ssim"][0].cpu().numpy().tobytes() == direct["ssim"].tobytes()
        # "auto" takes the batch's mask (1 = foreground); a given x_sample is scored as it is
        batch["target_mask"] = (torch.rand(1, N, 256, 256, generator=g) < 0.6).float().cuda()
        auto = m.evaluate_views(batch, x_sample=x)
        explicit = M.image_metrics(x, batch["target_image"], batch["target_mask"] < 0.5)
        assert torch.equal(auto["ssim"], explicit["ssim"]) and torch.equal(auto["background"], explicit["background"])
        assert torch.equal(m.evaluate_views(batch, x_sample=x, mask=None)["ssim"], want["ssim"])
        assert (auto["background"] > 0).all() and not torch.equal(auto["ssim"], want["ssim"])
        # validation_step: off -> the JPEG only, as before; on -> the JSON beside it
        m.image_dir, m.global_rank, m.global_step, m.output_num = str(tmp_path), 0, 5, 1
        torch.manual_seed(21)
        m.validation_step(batch, 0)
        val = tmp_path / "images" / "val"
        assert sorted(p.name for p in val.iterdir()) == ["5.jpg"] and m.last_val_metrics is None
        m.val_metrics, m.global_step = True, 6
        torch.manual_seed(21)
        xs = m.validation_step(batch, 0)
        assert sorted(p.name for p in val.iterdir()) == ["5.jpg", "6.jpg", "6.json"]
        assert torch.equal(xs, x) and torch.equal(m.last_val_metrics["ssim"], auto["ssim"])
        js = json.loads((val / "6.json").read_text())
        assert js["ssim"] == auto["ssim"].reshape(-1).tolist() and js["global_step"] == 6
        assert js["psnr_mean"] == pytest.approx(float(auto["psnr"].mean()), rel=1e-12) and len(js["mae"]) == N
    finally:
        m.engine.close()


def test_generate_face_with_gt_dir(tmp_path):
    """generate_face --gt_dir on the synthetic checkpoint of the end-to-end test, against a folder of 16 written PNGs: the JSON's
    numbers are the oracle's on the saved strip and those files."""
    import struct
    import yaml
    from PIL import Image
    from morphablediffusion_amd import generate_face as GF
    from morphablediffusion_amd import synthetic
    from morphablediffusion_amd.spec import (ClipConfig, UNetConfig, VaeConfig, VolumeConfig, clip_manifest, full_manifest,
                                             vae_decoder_manifest, vae_encoder_manifest)
    from morphablediffusion_amd.weights import seeded_state_dict
    from tests.test_gpu_eval_caller import facescape_yaml
    ucfg, vcfg = UNetConfig(model_channels=64), VolumeConfig(num_views=16)
    Wt = seeded_state_dict(full_manifest(ucfg, vcfg), 7)
    vae = VaeConfig(ch=32)
    Wt.update(seeded_state_dict(vae_decoder_manifest(vae), 7))
    Wt.update(seeded_state_dict(vae_encoder_manifest(vae), 7))
    Wt.update({k: v.half() for k, v in seeded_state_dict(clip_manifest(ClipConfig(width=128, layers=2, heads=2, embed=768)), 7).items()})
    torch.save({"state_dict": Wt}, tmp_path / "m.ckpt")
    (tmp_path / "facescape.yaml").write_text(yaml.safe_dump(facescape_yaml(view_num=16)))
    verts = synthetic.ellipsoid_mesh(900, 4, radii=(0.09, 0.11, 0.10)).numpy()
    with open(tmp_path / "face.ply", "wb") as f:
        f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\n"
                f"property float z\nend_header\n".encode())
        for v in verts:
            f.write(struct.pack("<fff", *[float(t) for t in v]))
    r = np.random.RandomState(1)
    rgba = np.full((300, 280, 4), 255, np.uint8)
    rgba[..., :3] = r.randint(0, 255, (300, 280, 3))
    Image.fromarray(rgba, "RGBA").save(tmp_path / "subject.png")
    gt = tmp_path / "gt"
    gt.mkdir()
    for i in range(16):  # RGBA captures with a transparent band whose height differs per view
        a = r.randint(0, 256, (256, 256, 4)).astype(np.uint8)
        a[..., 3] = 255
        a[:20 + 3 * i, :, 3] = 0
        a[100:110, 50:60, 3] = 128
        Image.fromarray(a, "RGBA").save(gt / f"{i:03d}.png")
    args = ["--input_img", str(tmp_path / "subject.png"), "--exp_img", str(tmp_path / "kiss.jpg"), "--mesh", str(tmp_path / "face.ply"),
            "--cfg", str(tmp_path / "facescape.yaml"), "--ckpt", str(tmp_path / "m.ckpt"), "--output_dir", str(tmp_path / "out"),
            "--sample_steps", "2", "--batch_view_num", "8", "--sampler", "dpmpp_2m", "--gt_dir", str(gt)]
    strip, path = GF.run(GF.build_parser().parse_args(args))
    js = json.loads((tmp_path / "out" / "subject_kiss_metrics.json").read_text())
    assert js["sampler"] == "dpmpp_2m" and js["sample_steps"] == 2 and len(js["ssim"]) == 16
    saved = np.asarray(Image.open(path))
    assert np.array_equal(saved, strip)
    views = M.strip_to_views(saved, 16, 256)[0].numpy()
    tv, tm = M.load_target_views(gt, 16, 256)
    ref = R.image_metrics_ref(views, tv.numpy(), tm.numpy(), "explicit")
    assert np.abs(np.asarray(js["ssim"]) - ref["ssim"]).max() <= SSIM_TOL
    d = R.derived(ref, 256, 256)
    for k in ("psnr", "mse", "mae"):
        assert np.allclose(js[k], d[k], rtol=1e-14, atol=0), k
    assert js["ssim_mean"] == pytest.approx(ref["ssim"].mean(), abs=SSIM_TOL)
    assert not (tmp_path / "out" / "neus2_data").exists()

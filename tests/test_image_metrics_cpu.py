"""CPU: the image metrics' oracle (tests/image_metrics_ref.py) against a restatement of skimage's structural_similarity, its
quantisation against batch.views_to_uint8, the file helpers of morphablediffusion_amd.metrics, the argument checks that precede
any launch, and the C ABI's declaration."""
import numpy as np
import pytest
import torch

from morphablediffusion_amd import batch as BT
from morphablediffusion_amd import lib as L
from morphablediffusion_amd import metrics as M
from tests import image_metrics_ref as R


def _skimage_ssim(x, y):
    """skimage.metrics.structural_similarity(x, y, channel_axis=-1) at its defaults for uint8 [H,W,3] images, restated from its
    documented algorithm: float64 uniform filters of size 7, sample covariance, the border of 3 cropped, channels averaged."""
    from scipy.ndimage import uniform_filter
    vals = []
    for c in range(3):
        X, Y = x[:, :, c].astype(np.float64), y[:, :, c].astype(np.float64)
        ux, uy = uniform_filter(X, size=7), uniform_filter(Y, size=7)
        uxx, uyy, uxy = uniform_filter(X * X, size=7), uniform_filter(Y * Y, size=7), uniform_filter(X * Y, size=7)
        cov_norm = 49.0 / 48.0
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + R.C1) * (2 * vxy + R.C2)) / ((ux ** 2 + uy ** 2 + R.C1) * (vx + vy + R.C2))
        vals.append(S[3:S.shape[0] - 3, 3:S.shape[1] - 3].mean(dtype=np.float64))
    return float(np.mean(vals))


def _image_pairs(H, W):
    r = np.random.RandomState(H * 1000 + W)
    a = r.randint(0, 256, (H, W, 3)).astype(np.uint8)
    near = np.clip(a.astype(np.int64) + r.randint(-6, 7, a.shape), 0, 255).astype(np.uint8)
    flat = np.where(r.rand(H, W, 3) < 0.5, 255, 254).astype(np.uint8)
    flat[: H // 2] = 255  # piecewise flat: whole windows of one value, variance exactly 0
    checker = np.where((np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)[..., None], 0, 255).astype(np.uint8).repeat(3, 2)
    return {"random": (a, r.randint(0, 256, (H, W, 3)).astype(np.uint8)), "near": (near, a), "flat": (flat, np.full_like(flat, 255)),
            "inverted": (checker, 255 - checker)}


def test_oracle_equals_the_skimage_algorithm():
    """Bound 1e-9 absolute: both sides are float64 evaluations of the same function; the filter's running sums carry at most
    about 256 * 2^-53 * 7 * 255^2 ~ 1e-8 into a second moment, against C2 = 58.5 in the denominator."""
    pytest.importorskip("scipy.ndimage")
    worst = 0.0
    for H, W in ((7, 7), (8, 13), (40, 37), (256, 256)):
        for name, (x, y) in _image_pairs(H, W).items():
            got = R.image_metrics_ref(x[None], y[None])["ssim"][0]
            want = _skimage_ssim(x, y)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-9, (H, W, name, got, want)
    print(f"[image metrics] oracle vs the skimage algorithm: max |diff| = {worst:.2e}")


def test_oracle_on_closed_forms():
    x = np.random.RandomState(0).randint(0, 256, (1, 20, 23, 3)).astype(np.uint8)
    same = R.image_metrics_ref(x, x)
    assert same["ssim"][0] == 1.0 and same["sse"][0] == 0 and same["sae"][0] == 0
    assert R.derived(same, 20, 23)["psnr"][0] == np.inf
    black, white = np.zeros((1, 9, 9, 3), np.uint8), np.full((1, 9, 9, 3), 255, np.uint8)
    bw = R.image_metrics_ref(black, white)
    assert bw["sse"][0] == 243 * 255 ** 2 and bw["sae"][0] == 243 * 255
    assert abs(bw["ssim"][0] - R.C1 / (255.0 ** 2 + R.C1)) < 1e-15  # flat windows: S = C1 C2 / ((255^2 + C1) C2)
    masked = R.image_metrics_ref(black, white, mode="white")
    assert masked["sse"][0] == 0 and masked["background"][0] == 81 and masked["ssim"][0] == 1.0


def test_quantisation_is_views_to_uint8():
    v = R.bin_edge_values()  # [3,16,17]
    strip = BT.views_to_uint8(torch.from_numpy(v)[None, None], torch.zeros(1, 16, 17, 3))
    want = strip[:, 17:]  # the generated view's tile, [16,17,3]
    got = R.quantise(v.transpose(1, 2, 0))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert set(np.unique(got).tolist()) == set(range(256))
    k = (np.arange(256) / 255.0 * 2.0 - 1.0).astype(np.float32)
    assert not np.array_equal(R.quantise(k), np.arange(256))  # the exact grid points do NOT all land on their own byte: truncation


def test_strip_to_views_inverts_views_to_uint8():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 3, 8, 8, generator=g) * 2.4 - 1.2
    inp = torch.rand(2, 8, 8, 3, generator=g) * 2 - 1
    strip = BT.views_to_uint8(x, inp)
    assert strip.shape == (16, 32, 3)
    views = M.strip_to_views(strip, 3, 8)
    assert views.shape == (2, 3, 8, 8, 3) and views.dtype == torch.uint8
    assert np.array_equal(views.numpy(), R.quantise(x.permute(0, 1, 3, 4, 2).numpy()))
    with pytest.raises(ValueError):
        M.strip_to_views(strip, 4, 8)
    with pytest.raises(ValueError):
        M.strip_to_views(strip[:15], 3, 8)


def test_load_target_views(tmp_path):
    from PIL import Image
    r = np.random.RandomState(2)
    rgba = r.randint(0, 256, (3, 9, 9, 4)).astype(np.uint8)
    rgba[:, 0, :, 3] = 0        # a transparent row: white, masked
    rgba[:, 1, :, 3] = 255      # an opaque row: the colour itself
    rgba[0, 2, 0] = (10, 200, 77, 128)  # partial alpha: composited, truncated
    d = tmp_path / "rgba"
    d.mkdir()
    for i in (2, 0, 1):  # written out of order: the files are read sorted
        Image.fromarray(rgba[i], "RGBA").save(d / f"{i:02d}.png")
    views, mask = M.load_target_views(d, 3, 9)
    assert views.shape == (3, 9, 9, 3) and views.dtype == torch.uint8 and mask.shape == (3, 9, 9) and mask.dtype == torch.uint8
    assert (views[:, 0] == 255).all() and (mask[:, 0] == 1).all()
    assert np.array_equal(views[:, 1].numpy(), rgba[:, 1, :, :3]) and (mask[:, 1] == 0).all()
    assert np.array_equal(mask.numpy(), (rgba[..., 3] == 0).astype(np.uint8))
    a = np.float32(128) / np.float32(255)
    want = [int(np.float32(c) * a + np.float32(255) * (np.float32(1) - a)) for c in (10, 200, 77)]
    assert views[0, 2, 0].tolist() == want and want == [132, 227, 165]
    rgb = tmp_path / "rgb"
    rgb.mkdir()
    for i in range(2):
        Image.fromarray(rgba[i, :, :, :3].copy(), "RGB").save(rgb / f"v{i}.png")
    views, mask = M.load_target_views(rgb, 2, 9)
    assert mask is None and np.array_equal(views.numpy(), rgba[:2, :, :, :3])
    with pytest.raises(ValueError, match="3 expected"):
        M.load_target_views(rgb, 3, 9)
    with pytest.raises(ValueError, match="8 x 8 expected"):
        M.load_target_views(rgb, 2, 8)


def test_image_metrics_argument_checks_precede_any_launch():
    """These raise on CPU tensors on a machine without a GPU: nothing is copied or launched before the checks."""
    a = torch.zeros(2, 3, 9, 10)
    with pytest.raises(ValueError):
        M.image_metrics(a, torch.zeros(2, 3, 9, 11))
    with pytest.raises(ValueError):
        M.image_metrics(a, torch.zeros(3, 9, 10, 3))
    with pytest.raises(ValueError):
        M.image_metrics(torch.zeros(2, 3, 6, 10), torch.zeros(2, 6, 10, 3))  # H < 7
    with pytest.raises(ValueError):
        M.image_metrics(a, torch.zeros(2, 9, 10, 3), mask=torch.zeros(2, 9, 9))
    with pytest.raises(ValueError):
        M.image_metrics(a, torch.zeros(2, 9, 10, 3), mask="black")
    with pytest.raises(ValueError):
        M.image_metrics(a.long(), torch.zeros(2, 9, 10, 3))
    with pytest.raises(ValueError):
        M.image_metrics(torch.zeros(2, 4, 9, 10), torch.zeros(2, 4, 9, 10))  # no axis of size 3


def test_c_abi_declares_and_exports_the_entry_point():
    assert "mvd_op_image_metrics" in L.PROTOTYPES
    restype, argtypes = L.PROTOTYPES["mvd_op_image_metrics"]
    assert len(argtypes) == 13
    lib = L.load()
    assert hasattr(lib, "mvd_op_image_metrics") and len(lib.mvd_op_image_metrics.argtypes) == 13


def abi_error_cases(p):
    """name -> the 13 arguments of mvd_op_image_metrics with one argument error each; p: any non-null address (never read)."""
    ok = dict(pred=p, pd=0, pl=0, target=p, td=0, tl=0, mask=None, mode=0, V=1, H=7, W=7, out=p, stream=None)
    bad = {"null pred": dict(pred=None), "null target": dict(target=None), "null out": dict(out=None), "H < 7": dict(H=6),
           "W < 7": dict(W=6), "V < 1": dict(V=0), "V > 65535": dict(V=65536), "V H W 3 >= 2^31": dict(V=65535, H=105, W=105),
           "pred dtype": dict(pd=2), "target dtype": dict(td=-1), "pred layout": dict(pl=2), "target layout": dict(tl=-1),
           "mode": dict(mode=3), "explicit without a mask": dict(mode=1)}
    return {k: tuple(dict(ok, **v).values()) for k, v in bad.items()}


def test_c_abi_argument_errors_need_no_device():
    """Every argument error returns before the first HIP call, so this holds on a machine without a GPU."""
    import ctypes as C
    lib = L.load()
    buf = (C.c_double * 8)()
    for name, args in abi_error_cases(C.addressof(buf)).items():
        assert lib.mvd_op_image_metrics(*args) != 0, name
        assert lib.mvd_last_error().decode().startswith("mvd_op_image_metrics: "), name


def test_tap_reads_of_the_halo_tile_are_bank_conflict_free():
    """tools/lds_bank_model.py on the layout k_metrics.hip uses (rows of 40 bytes, 32 centres per row of lanes)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(root, "tools", "lds_bank_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.metrics_tap_read_cycles(40, 32) == 1.0

"""LoRA host plumbing (morphablediffusion_amd/lora.py): merging adapters into a state_dict, the chain-rule identity the device
projection relies on, the adapter file, target selection, the command-line flags.  No GPU."""
import pytest
import torch

from morphablediffusion_amd import lora as LR
from morphablediffusion_amd.spec import unet_manifest
from tests import golden_inputs as gi

P = "model.diffusion_model."


def _adapter(key, shape, rank, g, alpha=None):
    a = torch.randn(rank, shape[1], generator=g)
    b = torch.randn(shape[0], rank, generator=g)
    return {key: (a, b)}


@pytest.mark.parametrize("shape", [(24, 40), (24, 40, 1, 1), (24, 40, 1, 1, 1)])
def test_merge_lora_against_float64(shape):
    g = torch.Generator().manual_seed(3)
    rank, alpha, scale = 4, 6.0, 0.75
    w = torch.randn(*shape, generator=g)
    other = torch.randn(5, generator=g)
    ad = _adapter("w", shape, rank, g)
    lora = LR.pack_lora(ad, rank, alpha)
    out = LR.merge_lora({"w": w, "other": other}, lora, scale=scale)
    a, b = ad["w"]
    want = w.double() + scale * (alpha / rank) * (b.double() @ a.double()).view(shape)
    assert out["w"].shape == w.shape and out["w"].dtype == w.dtype
    err = ((out["w"].double() - want).abs().max() / want.abs().max()).item()
    # rank products + (rank - 1) sums + the scaling + the final sum: rank + 2 fp32 roundings, each at most 2^-24 of a partial result
    # that is bounded by |w| + s sum_k |b_k a_k| -- taken as twice the largest merged value, hence 2 (rank + 2) 2^-24
    assert err <= 2 * (rank + 2) * 2.0 ** -24, err
    assert out["other"] is other
    assert torch.equal(w, torch.randn(*shape, generator=torch.Generator().manual_seed(3)))  # the input is not modified
    # strength 0: the very same values
    zero = LR.merge_lora({"w": w, "other": other}, lora, scale=0.0)
    assert torch.equal(zero["w"], w)
    # fp16 checkpoints keep their dtype
    half = LR.merge_lora({"w": w.half()}, lora, scale=scale)
    assert half["w"].dtype == torch.float16 and half["w"].shape == w.shape


def test_merge_lora_rejects_what_does_not_fit():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(24, 40, generator=g)
    good = LR.pack_lora(_adapter("w", (24, 40), 4, g), 4, 4.0)
    with pytest.raises(ValueError):
        LR.merge_lora({"w": torch.randn(24, 41)}, good)  # in differs
    with pytest.raises(ValueError):
        LR.merge_lora({"w": torch.randn(25, 40)}, good)  # out differs
    with pytest.raises(ValueError):
        LR.merge_lora({"w": torch.randn(24, 40, 3, 3)}, good)  # a 3x3 convolution
    with pytest.raises(ValueError):
        LR.merge_lora({"v": w}, good)  # no such weight
    bad_rank = dict(good)
    bad_rank["lora.rank"] = torch.tensor(5)
    with pytest.raises(ValueError):
        LR.merge_lora({"w": w}, bad_rank)
    mismatched = dict(good)
    mismatched["lora.w.B"] = torch.randn(24, 3)
    with pytest.raises(ValueError):
        LR.merge_lora({"w": w}, mismatched)
    for r in (0, 65):
        with pytest.raises(ValueError):
            LR.check_rank(r)
    assert LR.check_rank(1) == 1 and LR.check_rank(64) == 64


def test_projection_of_dense_gradient_equals_autograd_through_the_adapters():
    """dA = s B^T dW, dB = s dW A^T: what mvd_lora_step computes from the dense dW the backward pass already wrote, against
    autograd through W0 + s B A on a two-layer network (float64)."""
    g = torch.Generator().manual_seed(5)
    r, s = 3, 1.5
    dims = [(7, 11), (5, 7)]
    x = torch.randn(9, 11, generator=g, dtype=torch.float64)
    W0 = [torch.randn(o, i, generator=g, dtype=torch.float64) for o, i in dims]
    A = [torch.randn(r, i, generator=g, dtype=torch.float64).requires_grad_(True) for o, i in dims]
    B = [torch.randn(o, r, generator=g, dtype=torch.float64).requires_grad_(True) for o, i in dims]

    def net(ws):
        return (torch.tanh(x @ ws[0].t()) @ ws[1].t()).pow(2).sum()

    net([W0[k] + s * B[k] @ A[k] for k in range(2)]).backward()
    W = [(W0[k] + s * B[k] @ A[k]).detach().requires_grad_(True) for k in range(2)]
    net(W).backward()
    for k in range(2):
        dW = W[k].grad
        assert torch.allclose(A[k].grad, s * B[k].detach().t() @ dW, rtol=1e-12, atol=1e-12)
        assert torch.allclose(B[k].grad, s * dW @ A[k].detach().t(), rtol=1e-12, atol=1e-12)


def test_adapter_file_keys_and_metadata(tmp_path):
    man = unet_manifest(gi.SMALL_UNET)
    keys = LR.select_targets(man)[:3]
    ad = LR.init_adapters(keys, man, rank=4, seed=7)
    sd = LR.pack_lora(ad, 4, 8.0)
    assert set(sd) == {f"lora.{k}.{w}" for k in keys for w in "AB"} | {"lora.rank", "lora.alpha"}
    assert sd["lora.rank"].dtype == torch.int64 and int(sd["lora.rank"]) == 4
    assert sd["lora.alpha"].dtype == torch.float32 and float(sd["lora.alpha"]) == 8.0
    for k in keys:
        o, i = man[k][:2]
        a, b = sd[f"lora.{k}.A"], sd[f"lora.{k}.B"]
        assert a.shape == (4, i) and b.shape == (o, 4) and a.dtype == b.dtype == torch.float32
        assert float(a.abs().max()) <= i ** -0.5 and float(a.abs().max()) > 0.5 * i ** -0.5 and not b.any()
    # one generator, sorted key order: the same seed gives the same adapters whatever order the keys come in
    again = LR.init_adapters(list(reversed(keys)), man, rank=4, seed=7)
    assert all(torch.equal(ad[k][0], again[k][0]) for k in keys)
    assert not torch.equal(ad[keys[0]][0], LR.init_adapters(keys, man, rank=4, seed=8)[keys[0]][0])
    path = tmp_path / "adapter.pt"
    torch.save(sd, path)
    back, rank, alpha = LR.unpack_lora(str(path))
    assert rank == 4 and alpha == 8.0 and sorted(back) == sorted(keys)
    assert all(torch.equal(back[k][0], ad[k][0]) and torch.equal(back[k][1], ad[k][1]) for k in keys)
    with pytest.raises(ValueError):
        LR.unpack_lora({k: v for k, v in sd.items() if k != "lora.rank"})
    with pytest.raises(ValueError):
        LR.unpack_lora({k: v for k, v in sd.items() if not k.endswith(keys[0] + ".B")})


def test_default_targets_are_eight_per_transformer_block():
    man = unet_manifest(gi.SMALL_UNET)
    blocks = {k.split(".transformer_blocks.")[0] for k in man if ".transformer_blocks." in k}
    keys = LR.select_targets(man)
    assert len(blocks) > 0 and len(keys) == 8 * len(blocks)
    assert all(k.startswith(P) and ".attn" in k and k.endswith(".weight") and LR.is_target_shape(man[k]) for k in keys)
    assert keys == sorted(keys)
    # patterns work with and without the state_dict prefix; 1x1 convolutions qualify
    extra = LR.select_targets(man, ["*.proj_in.weight"])
    assert len(extra) == len(blocks) and all(len(man[k]) == 4 for k in extra)
    assert LR.select_targets(man, [P + "*.proj_in.weight"]) == extra
    with pytest.raises(ValueError):
        LR.select_targets(man, ["*.no_such_layer.weight"])
    with pytest.raises(ValueError):
        LR.select_targets(man, ["*.in_layers.2.weight"])  # 3x3 convolutions
    with pytest.raises(ValueError):
        LR.select_targets(man, ["*.attn1.to_q.weight", "*.norm1.weight"])  # a vector


def test_generate_face_parser_accepts_the_lora_flags():
    from morphablediffusion_amd.generate_face import build_parser
    base = ["--input_img", "a.png", "--exp_img", "b.png", "--mesh", "m.obj", "--output_dir", "out"]
    flags = build_parser().parse_args(base)
    assert flags.lora is None and flags.lora_scale == 1.0
    flags = build_parser().parse_args(base + ["--lora", "adapter.pt", "--lora_scale", "0.5"])
    assert flags.lora == "adapter.pt" and flags.lora_scale == 0.5

"""Gradient clipping by global norm + EMA weights, the parts that need no GPU: the C ABI of the new entry points (parsed out of
include/mvd.h, resolved in the built library), LitEma's checkpoint key rule and warm-up of the decay, the constructor's check."""
import ctypes as C

import pytest

from morphablediffusion_amd import lib as L
from morphablediffusion_amd.model import SyncMultiviewDiffusion, ema_decay_at, ema_key

NEW = {
    "mvd_train_grad_norm": [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p],
    "mvd_train_adamw_step_ex": [C.c_void_p] + [C.c_float] * 6 + [C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_float, C.c_float,
                                                                 C.c_void_p, C.c_void_p],
    "mvd_train_last_grad_norm": [C.c_void_p, C.c_void_p, C.c_void_p],
    "mvd_train_ema_swap": [C.c_void_p, C.c_void_p],
    "mvd_op_adamw_ex": [C.c_void_p] * 5 + [C.c_size_t] + [C.c_float] * 5 + [C.c_int] + [C.c_float] * 3 + [C.c_void_p, C.c_void_p],
}


def test_new_entry_points_parse_out_of_the_header_and_resolve_in_the_library():
    for name, argtypes in NEW.items():
        assert name in L.PROTOTYPES, name
        restype, args = L.PROTOTYPES[name]
        assert restype is C.c_int and args == argtypes, (name, args)
    # the fused step takes the arguments of mvd_train_adamw_step, then the three new ones, then the stream
    old, ex = L.PROTOTYPES["mvd_train_adamw_step"][1], L.PROTOTYPES["mvd_train_adamw_step_ex"][1]
    assert ex[:len(old) - 1] == old[:-1] and len(ex) == len(old) + 3
    lib = L.load()  # raises when a declared symbol is missing
    for name in NEW:
        assert getattr(lib, name).argtypes == NEW[name]


def test_ema_checkpoint_key_is_litemas():
    assert ema_key("model.diffusion_model.input_blocks.0.0.weight") == "model_ema.diffusion_modelinput_blocks00weight"
    assert ema_key("model.diffusion_model.out.2.bias") == "model_ema.diffusion_modelout2bias"
    # trainable here, outside LitEma's ``self.model``: the same rule without a prefix to drop
    assert ema_key("spatial_volume.target_encoder.init_conv.weight") == "model_ema.spatial_volumetarget_encoderinit_convweight"
    assert ema_key("time_embed.0.weight") == "model_ema.time_embed0weight"


def test_warm_up_of_the_decay_is_litemas():
    for decay in (0.9999, 0.5):
        for n in range(1, 31):
            assert ema_decay_at(decay, n) == min(decay, (1 + n) / (10 + n))
    assert ema_decay_at(0.9999, 1) == 2 / 11 and ema_decay_at(0.9999, 30) == 31 / 40
    assert ema_decay_at(0.5, 8) == 0.5 and ema_decay_at(0.5, 7) == 8 / 17  # 9 / 18 is where the cap takes over
    assert ema_decay_at(0.9999, 10 ** 6) == 0.9999


def test_use_ema_needs_train_mode():
    with pytest.raises(ValueError, match="train_mode"):
        SyncMultiviewDiffusion(unet_config={"target": "ldm.models.diffusion.attention.DepthWiseAttention", "params": {}},
                               use_ema=True, train_mode=False)

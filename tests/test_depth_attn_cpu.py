"""CPU: the float64 restatement that tests/test_gpu_depth_attn.py measures depth_attn_kernel against (tests/depth_attn_ref.py:
folded query, softmax over depth, weighted context column) is the reference's DepthAttention.forward
(oracle.mvd_oracle.depth_attention, ldm/models/diffusion/attention.py:26-47) once the folds are undone:
qk_h = scale W_k,h^T (W_q x)_h going in, W_o [W_v,h z_h]_h coming out.  Both in float64, so they agree to rounding."""
import pytest
import torch

from oracle import mvd_oracle as O
from tests import depth_attn_ref as R


@pytest.mark.parametrize("Cc", [24, 64])
@pytest.mark.parametrize("D", [3, 17])
def test_restatement_equals_the_reference_formula(Cc, D):
    g = torch.Generator().manual_seed(100 * Cc + D)
    b, inner, h, w = 2, 32, 3, 5  # h != w: a transposed pixel order would show
    x = torch.randn(b, inner, h, w, generator=g, dtype=torch.float64)
    context = torch.randn(b, Cc, D, h, w, generator=g, dtype=torch.float64)
    w_q = torch.randn(inner, inner, generator=g, dtype=torch.float64) * inner ** -0.5
    w_k = torch.randn(inner, Cc, generator=g, dtype=torch.float64) * Cc ** -0.5 * 3.0  # scores of a few units: a softmax far from uniform
    w_v = torch.randn(inner, Cc, generator=g, dtype=torch.float64) * Cc ** -0.5
    w_o = torch.randn(inner, inner, generator=g, dtype=torch.float64) * inner ** -0.5
    W = {"a.to_q.weight": w_q[:, :, None, None], "a.to_k.weight": w_k[:, :, None, None, None],
         "a.to_v.weight": w_v[:, :, None, None, None], "a.to_out.weight": w_o[:, :, None, None]}
    want = O.depth_attention(W, "a", x, context, heads=R.HEADS)
    z = R.depth_attn_ref(R.fold_qk(w_q, w_k, x), R.ctx_rows(context))
    got = R.unfold_out(w_o, w_v, z, b, h, w)
    assert want.dtype == torch.float64 and got.shape == want.shape
    err = ((got - want).norm() / want.norm()).item()
    c = R.ctx_rows(context).permute(0, 2, 1, 3).reshape(b * h * w, D, Cc)
    spread = torch.softmax(torch.einsum("phc,pdc->phd", R.fold_qk(w_q, w_k, x), c), -1).max(-1).values.mean().item()
    print(f"[parity] depth_attn restatement vs oracle Cc={Cc} D={D}: relL2={err:.2e} (mean top probability {spread:.2f}, uniform {1 / D:.2f})")
    assert spread > 1.5 / D, "vacuous: the softmax is uniform"
    assert err <= 1e-10

"""The depth attention of csrc/k_depth.hip restated in float64, in the kernel's own layouts: the yardstick of
tests/test_gpu_depth_attn.py, tied to the reference's formula (oracle.mvd_oracle.depth_attention = DepthAttention.forward,
ldm/models/diffusion/attention.py:26-47) by tests/test_depth_attn_cpu.py.  No GPU, no engine code."""
import torch

HEADS = 4


def depth_attn_ref(qk, ctx):
    """qk [n_cond*HW, 4, Cc] (the folded query), ctx [n_cond, D, HW, Cc] -> z [n_cond*HW, 4*Cc], all float64:
    sim[h,d] = qk[h] . ctx[d];  a = softmax over d;  z[h] = sum_d a[h,d] ctx[d]."""
    n_cond, D, HW, Cc = ctx.shape
    c = ctx.double().permute(0, 2, 1, 3).reshape(n_cond * HW, D, Cc)
    q = qk.double().reshape(n_cond * HW, HEADS, Cc)
    sim = torch.einsum("phc,pdc->phd", q, c)
    a = torch.softmax(sim, dim=-1)
    return torch.einsum("phd,pdc->phc", a, c).reshape(n_cond * HW, HEADS * Cc)


def fold_qk(w_q, w_k, x):
    """qk_h = scale * W_k,h^T (W_q x)_h: x [b, inner, h, w], w_q [inner, inner], w_k [inner, Cc] -> [b*h*w, 4, Cc]."""
    b, inner, h, w = x.shape
    hd = inner // HEADS
    q = torch.einsum("oi,bihw->bhwo", w_q, x).reshape(b * h * w, HEADS, hd)
    return torch.einsum("phj,hjc->phc", q, w_k.reshape(HEADS, hd, -1)) * hd ** -0.5


def unfold_out(w_o, w_v, z, b, h, w):
    """W_o [W_v,h z_h]_h: z [b*h*w, 4*Cc], w_v [inner, Cc], w_o [inner, inner] -> [b, inner, h, w]."""
    inner = w_o.shape[0]
    hd = inner // HEADS
    v = torch.einsum("hjc,phc->phj", w_v.reshape(HEADS, hd, -1), z.reshape(b * h * w, HEADS, -1)).reshape(b, h, w, inner)
    return torch.einsum("oi,bhwi->bohw", w_o, v)


def ctx_rows(context):
    """The reference's context [b, Cc, D, h, w] in the kernel's layout [b, D, h*w, Cc]."""
    b, Cc, D, h, w = context.shape
    return context.permute(0, 2, 3, 4, 1).reshape(b, D, h * w, Cc)

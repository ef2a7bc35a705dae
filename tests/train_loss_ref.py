"""Float64 restatement of the training objective of mvd_train_unet_step_ex / mvd_op_train_loss (include/mvd.h), written from the
definitions with explicit indexing -- not from the kernel.  pred / target channels-last [B,HW,C], m [B,HW] or None, w [B] or None.

    d = pred - target
    rho(d) = d^2, rho' = 2 d                                   l2, and huber for |d| <= delta (|d| == delta included)
    rho(d) = 2 delta |d| - delta^2, rho' = 2 delta sign(d)     huber, |d| > delta
    a_b = sum_p m[b,p]     l_b = sum_{p,c} m[b,p] rho(d[b,p,c]) / (C a_b)     (a_b == 0: l_b = 0, zero gradient)
    L = (1/B) sum_b w_b l_b     mse_b = mean_{p,c} d^2
    dpred[b,p,c] = c_b m[b,p] rho'(d)/2,   c_b = 2 loss_scale w_b / (B C a_b)

``loss_t`` is the same L as a differentiable torch expression (for the autograd check of ``dpred``); ``formula`` evaluates the
vectorised formula in a given dtype (float32 on the CPU gives e_ref32 of the GPU tests' error bound)."""
import torch


def rho(d, loss_type, delta):
    """(rho(d), rho'(d) / 2) of ONE python float."""
    if loss_type == "huber" and abs(d) > delta:
        return 2.0 * delta * abs(d) - delta * delta, (delta if d > 0 else -delta)
    return d * d, d


def reference(pred, target, w=None, m=None, loss_type="l2", delta=1.0, loss_scale=1.0):
    """-> dict(L float, loss_b [B], mse_b [B], dpred [B,HW,C]) in float64, by explicit loops."""
    assert loss_type in ("l2", "huber")
    p, t = pred.detach().double().cpu(), target.detach().double().cpu()
    B, HW, C = p.shape
    mm = None if m is None else m.detach().double().cpu().reshape(B, HW)
    ww = None if w is None else w.detach().double().cpu().reshape(B)
    loss_b, mse_b = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    dpred = torch.zeros(B, HW, C, dtype=torch.float64)
    pl, tl = p.tolist(), t.tolist()
    for b in range(B):
        mb = [1.0] * HW if mm is None else mm[b].tolist()
        wb = 1.0 if ww is None else float(ww[b])
        a = sum(mb)
        cb = 0.0 if a == 0.0 else 2.0 * loss_scale * wb / (B * C * a)
        s_l = s_d = 0.0
        for q in range(HW):
            for c in range(C):
                d = pl[b][q][c] - tl[b][q][c]
                r, g = rho(d, loss_type, delta)
                s_l += mb[q] * r
                s_d += d * d
                dpred[b, q, c] = cb * mb[q] * g
        loss_b[b] = 0.0 if a == 0.0 else s_l / (C * a)
        mse_b[b] = s_d / (HW * C)
    L = sum((1.0 if ww is None else float(ww[b])) * float(loss_b[b]) for b in range(B)) / B
    return dict(L=L, loss_b=loss_b, mse_b=mse_b, dpred=dpred)


def formula(pred, target, w=None, m=None, loss_type="l2", delta=1.0, loss_scale=1.0, dtype=torch.float64):
    """The same quantities by whole-tensor torch operations on the CPU in ``dtype`` -> (L, loss_b, mse_b, dpred)."""
    p, t = pred.detach().cpu().to(dtype), target.detach().cpu().to(dtype)
    B, HW, C = p.shape
    mm = torch.ones(B, HW, dtype=dtype) if m is None else m.detach().cpu().to(dtype).reshape(B, HW)
    ww = torch.ones(B, dtype=dtype) if w is None else w.detach().cpu().to(dtype).reshape(B)
    d = p - t
    if loss_type == "huber":
        lin = d.abs() > delta
        r = torch.where(lin, 2.0 * delta * d.abs() - delta * delta, d * d)
        g = torch.where(lin, delta * torch.sign(d), d)
    else:
        r, g = d * d, d
    a = mm.sum(1)
    ok = a != 0
    a1 = torch.where(ok, a, torch.ones_like(a))
    loss_b = torch.where(ok, (mm[:, :, None] * r).sum((1, 2)) / (C * a1), torch.zeros_like(a))
    mse_b = (d * d).mean((1, 2))
    cb = torch.where(ok, (2.0 * loss_scale) * ww / (float(B * C) * a1), torch.zeros_like(a))
    dpred = cb[:, None, None] * mm[:, :, None] * g
    return (ww * loss_b).mean(), loss_b, mse_b, dpred


def loss_t(pred, target, w=None, m=None, loss_type="l2", delta=1.0):
    """L as a differentiable float64 torch scalar of ``pred`` (torch's own huber_loss doubled for the robust branch)."""
    B, HW, C = pred.shape
    d = pred - target
    if loss_type == "huber":
        r = 2.0 * torch.nn.functional.huber_loss(pred, target, reduction="none", delta=delta)
    else:
        r = d * d
    total = pred.new_zeros(())
    for b in range(B):
        mb = pred.new_ones(HW) if m is None else m[b].reshape(HW).to(pred.dtype)
        a = mb.sum()
        if float(a) == 0.0:
            continue
        wb = 1.0 if w is None else w[b].to(pred.dtype)
        total = total + wb * (mb[:, None] * r[b]).sum() / (C * a)
    return total / B


def nerr(got, want):
    """Normalised max error of ``got`` against the float64 ``want``."""
    want = torch.as_tensor(want, dtype=torch.float64)
    got = torch.as_tensor(got).detach().double().cpu().reshape(want.shape)
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def bound(e_ref32):
    """The op bound of the GPU tests: 8 x the error of torch's CPU fp32 evaluation of the same formula (another order of the same
    fp32 operations) + 2e-6 (the floor tests/test_gpu_lora_ops.py uses)."""
    return 8.0 * e_ref32 + 2e-6

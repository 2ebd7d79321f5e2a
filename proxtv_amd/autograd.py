"""Differentiable TV-L1 fibre prox and 2-D Douglas-Rachford solves for torch pipelines (unrolled / plug-and-play reconstruction, learned
penalties, choosing lambda by gradient).  Imported on request only: ``import proxtv_amd`` stays torch-free.

    from proxtv_amd import autograd
    y = autograd.tv1_fibres(x, w, dim)            # x: float64 CUDA tensor; w: float or 0-d float64 tensor; weights: per-edge tensor
    y = autograd.tv1_2d(x, w)                     # the 2-D solve; also tv1w_2d(x, w_col, w_row) and tv1_2d_batch(xs, w)
    y.sum().backward()

tv1_fibres: forward is device.tv1_fibres; backward is ONE device.tv1_fibres_vjp call on the saved output (a segmented mean, see
include/proxtv_amd.h for the step rule and where the prox is not differentiable) plus, for a scalar w, a sum.  The 2-D Douglas-Rachford
solves are differentiated as loops, natively: forward is the fused device.tv1_2d / tv1w_2d / tv1_2d_batch, only x and the penalties are
saved, and backward is ONE device.dr2_vjp call, which replays the recurrence on the device and sweeps it in reverse.  The
other 2-D / N-D solvers (PD, Yang, ...) are not differentiated: compose them from tv1_fibres and torch's pointwise operations.
"""
import torch

from . import device


class _TV1Fibres(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, weights, dim):
        y = device.tv1_fibres(_colmajor(x.detach()), float(w), dim, None if weights is None else _colmajor(weights.detach()))
        ctx.save_for_backward(y)
        ctx.dim = dim
        ctx.w_device = w.device if isinstance(w, torch.Tensor) else None
        ctx.weighted = weights is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        need_x, need_w, need_weights = ctx.needs_input_grad[:3]
        gx, gw, _ = device.tv1_fibres_vjp(y, gy, ctx.dim, need_gw=need_w or need_weights)
        gw_scalar = None
        if need_w:
            # (with per-edge weights the scalar w does not enter the prox: its gradient is zero)
            gw_scalar = (torch.zeros((), dtype=torch.float64) if ctx.weighted else gw.sum()).to(ctx.w_device)
        return (gx if need_x else None), gw_scalar, (gw if need_weights else None), None


def _colmajor(t):
    return t if device._is_colmajor(t) else device.to_colmajor(t)


def tv1_fibres(x, w, dim, weights=None):
    """``device.tv1_fibres(x, w, dim, weights)`` with a graph behind it: differentiable in x, in `weights`, and in w when w is a 0-d
    float64 tensor (its gradient comes back on that tensor's device).  When nothing asks for a gradient this IS device.tv1_fibres."""
    if isinstance(w, torch.Tensor) and (w.dim() != 0 or w.dtype != torch.float64):
        raise ValueError("w: expected a float or a 0-d float64 tensor")
    wants = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, w, weights))
    if not wants:
        return device.tv1_fibres(x, float(w), dim, weights)
    return _TV1Fibres.apply(x, w, weights, int(dim))


class _DR2(torch.autograd.Function):
    """x, then the two penalties: 0-d tensors / floats (uniform) or the two per-edge maps (`weighted`)."""

    @staticmethod
    def forward(ctx, x, p_col, p_row, max_iters, weighted):
        xd = _colmajor(x.detach())
        if weighted:
            wc, wr = _colmajor(p_col.detach()), _colmajor(p_row.detach())
            y, _ = device.tv1w_2d(xd, wc, wr, max_iters)
            ctx.save_for_backward(xd, wc, wr)
        else:
            if xd.dim() == 3:
                y, _ = device.tv1_2d_batch(xd, float(p_col), max_iters)
            else:
                y, _ = device.tv1_2d(xd, float(p_col), max_iters, w_row=float(p_row))
            ctx.save_for_backward(xd)
            ctx.lams = (float(p_col), float(p_row))
            ctx.lam_devices = tuple(p.device if isinstance(p, torch.Tensor) else None for p in (p_col, p_row))
        ctx.max_iters, ctx.weighted = max_iters, weighted
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        need_x, need_col, need_row = ctx.needs_input_grad[:3]
        if ctx.weighted:
            x, wc, wr = ctx.saved_tensors
            gx, gc, gr, _, _ = device.dr2_vjp(x, gy, 0.0, max_iters=ctx.max_iters, weights_col=wc, weights_row=wr,
                                              need_gw=need_col or need_row)
        else:
            (x,) = ctx.saved_tensors
            gx, _, _, glam, _ = device.dr2_vjp(x, gy, ctx.lams[0], ctx.lams[1], ctx.max_iters, need_gw="sums" if need_col or need_row else False)
            gc = gr = None
            if glam is not None:
                glam = glam.reshape(-1, 2).sum(axis=0)     # (a batch shares its penalties)
                gc, gr = (None if d is None else torch.tensor(v, dtype=torch.float64, device=d) for v, d in zip(glam, ctx.lam_devices))
        return (gx if need_x else None), (gc if need_col else None), (gr if need_row else None), None, None


def _scalar_penalty(w, name):
    if isinstance(w, torch.Tensor) and (w.dim() != 0 or w.dtype != torch.float64):
        raise ValueError(f"{name}: expected a float or a 0-d float64 tensor")


def _wants(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def tv1_2d(x, w, max_iters=0, w_row=None):
    """``device.tv1_2d(x, w, max_iters, w_row=w_row)[0]`` (the Douglas-Rachford solve) with a graph behind it: differentiable in x and in
    w / w_row where they are 0-d float64 tensors (the gradient comes back on that tensor's device; one tensor for both directions
    receives the sum).  The result is bit for bit device.tv1_2d's; when nothing asks for a gradient this IS device.tv1_2d."""
    _scalar_penalty(w, "w")
    _scalar_penalty(w_row, "w_row")
    if not _wants(x, w, w_row):
        return device.tv1_2d(x, float(w), max_iters, w_row=None if w_row is None else float(w_row))[0]
    return _DR2.apply(x, w, w if w_row is None else w_row, int(max_iters), False)


def tv1w_2d(x, w_col, w_row, max_iters=0):
    """``device.tv1w_2d(x, w_col, w_row, max_iters)[0]`` with a graph behind it: differentiable in x and in both weight maps."""
    if not _wants(x, w_col, w_row):
        return device.tv1w_2d(x, w_col, w_row, max_iters)[0]
    return _DR2.apply(x, w_col, w_row, int(max_iters), True)


def tv1_2d_batch(xs, w, max_iters=0):
    """``device.tv1_2d_batch(xs, w, max_iters)[0]`` on an (M, N, B) stack with a graph behind it: differentiable in xs and in a 0-d
    float64 tensor w (the sum over the images and both directions)."""
    _scalar_penalty(w, "w")
    if not _wants(xs, w):
        return device.tv1_2d_batch(xs, float(w), max_iters)[0]
    return _DR2.apply(xs, w, w, int(max_iters), False)

"""Differentiable TV-L1 fibre prox for torch pipelines (unrolled / plug-and-play reconstruction, learned penalties, choosing lambda
by gradient).  Imported on request only: ``import proxtv_amd`` stays torch-free.

    from proxtv_amd import autograd
    y = autograd.tv1_fibres(x, w, dim)            # x: float64 CUDA tensor; w: float or 0-d float64 tensor; weights: per-edge tensor
    y.sum().backward()

Forward is device.tv1_fibres; backward is ONE device.tv1_fibres_vjp call on the saved output (a segmented mean, see
include/proxtv_amd.h for the step rule and where the prox is not differentiable) plus, for a scalar w, a sum.  2-D / N-D solvers are
not differentiated as loops: compose them from this prox and torch's pointwise operations.
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

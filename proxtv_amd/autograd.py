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
N-D entry tvgen is differentiated the same way through its two Dykstra loops ('pd2' / 'pd'): forward is the fused device.tvgen, backward
ONE device.tvgen_vjp call with the iteration count the forward reported.  The other solvers (PDR, Yang, ...) are not
differentiated: compose them from tv1_fibres and torch's pointwise operations.  The TV-L2 fibre prox has its own derivative:
tv2_fibres(x, w, dim) is device.tv2_fibres with ONE device.tv2_fibres_vjp call as backward.  TV-L2 terms inside the two
differentiated solver families are covered too: tvp_2d(x, w_col, w_row, p_col, p_row) is device.tvp_2d with ONE
device.dr2_vjp(..., p_col=, p_row=) call as backward, and tvgen(..., ps=[...]) is device.tvgen(..., ps=) with ONE
device.tvgen_vjp(..., ps=) call; every p is 1 or 2.  At a TV-L2 fibre's kink the branch the forward sweep took is differentiated.
The general-p fibre prox alone has its derivative too: tvp_fibres(x, w, p, dim) is device.tvp_fibres with ONE device.tvp_fibres_vjp call
as backward, from the saved output alone; a general p inside tvp_2d / tvgen stays refused.

    y = autograd.tvgen(x, [w0, w1, w2], [1, 2, 3])   # a volume; every w a float or a 0-d float64 tensor
    y = autograd.tvgen(x, [w0, w1, w2], [1, 2, 3], ps=[1, 2, 1])
    y = autograd.tvp_2d(x, w_col, w_row, 1, 2)

Every function takes ``tape="outputs"`` (the default) or ``tape="steps"``: what is kept for the reverse sweeps.  With "steps",
tv1_fibres saves the 2-bit step codes of its output (device.tv1_fibres_steps: an int32 tensor of 1/32 of y's bytes) in the graph instead
of y, and the solver derivatives keep step codes instead of their sweep outputs while they run.  Every gradient is the same bits.

Forward mode: tv1_fibres, tv1_2d, tv1w_2d and tv1_2d_batch also work under ``torch.autograd.forward_ad.dual_level()``.  A
dual x, a dual 0-d float64 w (its tangent is the d lambda of a uniform penalty) or dual weight maps give a dual result whose primal is the
same fused solve and whose tangent is ONE device.tv1_fibres_jvp / device.dr2_jvp call: nothing is taped, so the scratch does not grow
with max_iters.  torch.func transforms and vmap are not covered; the other functions of this module have no forward mode.
"""
import torch

from . import device


class _TV1Fibres(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, weights, dim, tape, dual):
        y = device.tv1_fibres(_colmajor(x.detach()), float(w), dim, None if weights is None else _colmajor(weights.detach()))
        ctx.save_for_backward(device.tv1_fibres_steps(y, dim) if tape == "steps" else y)
        if dual:      # (forward mode reads the output itself, whatever the tape)
            ctx.save_for_forward(y)
        ctx.dim, ctx.tape, ctx.shape = dim, tape, tuple(y.shape)
        ctx.w_device = w.device if isinstance(w, torch.Tensor) else None
        ctx.weighted = weights is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        need_x, need_w, need_weights = ctx.needs_input_grad[:3]
        if ctx.tape == "steps":     # (y is the word tensor)
            gx, gw, _ = device.tv1_fibres_vjp_steps(y, gy, ctx.shape, ctx.dim, need_gw=need_w or need_weights)
        else:
            gx, gw, _ = device.tv1_fibres_vjp(y, gy, ctx.dim, need_gw=need_w or need_weights)
        gw_scalar = None
        if need_w:
            # (with per-edge weights the scalar w does not enter the prox: its gradient is zero)
            gw_scalar = (torch.zeros((), dtype=torch.float64) if ctx.weighted else gw.sum()).to(ctx.w_device)
        return (gx if need_x else None), gw_scalar, (gw if need_weights else None), None, None, None

    @staticmethod
    def jvp(ctx, dx, dw, dweights, *_):
        (y,) = ctx.saved_tensors
        # (with per-edge weights the scalar w does not enter the prox: its tangent goes nowhere)
        dlam = 0.0 if dw is None or ctx.weighted else float(dw)
        return device.tv1_fibres_jvp(y, dx, ctx.dim, dweights=dweights if ctx.weighted else None, dw=dlam)


def _colmajor(t):
    return t if device._is_colmajor(t) else device.to_colmajor(t)


def tv1_fibres(x, w, dim, weights=None, tape="outputs"):
    """``device.tv1_fibres(x, w, dim, weights)`` with a graph behind it: differentiable in x, in `weights`, and in w when w is a 0-d
    float64 tensor (its gradient comes back on that tensor's device).  When nothing asks for a gradient this IS device.tv1_fibres."""
    if isinstance(w, torch.Tensor) and (w.dim() != 0 or w.dtype != torch.float64):
        raise ValueError("w: expected a float or a 0-d float64 tensor")
    device._tape(tape)
    wants = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, w, weights))
    dual = _dual(x, w, weights)
    if not wants and not dual:
        return device.tv1_fibres(x, float(w), dim, weights)
    return _TV1Fibres.apply(x, w, weights, int(dim), tape, dual)


class _TV2Fibres(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, dim):
        y, mu = device.tv2_fibres(_colmajor(x.detach()), float(w), dim, return_mu=True)
        ctx.save_for_backward(y, mu)
        ctx.dim, ctx.w = dim, float(w)
        ctx.w_device = w.device if isinstance(w, torch.Tensor) else None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        y, mu = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[:2]
        res = device.tv2_fibres_vjp(y, mu, gy, ctx.w, ctx.dim, need_glam=need_w)
        gx, glam = res if need_w else (res, None)
        return (gx if need_x else None), (glam.sum().to(ctx.w_device) if need_w else None), None


def tv2_fibres(x, w, dim):
    """``device.tv2_fibres(x, w, dim)`` (the TV-L2 fibre prox, penalty ``w * ||diff||_2`` per fibre) with a graph behind it:
    differentiable in x, and in w when w is a 0-d float64 tensor (its gradient comes back on that tensor's device).  The forward is
    bit for bit device.tv2_fibres's and saves its output and the fibres' multipliers; backward is ONE device.tv2_fibres_vjp call plus,
    for w, a sum (at the kink the branch the forward took is differentiated).  When nothing asks for a gradient this IS
    device.tv2_fibres."""
    _scalar_penalty(w, "w")
    if not _wants(x, w):
        return device.tv2_fibres(x, float(w), dim)
    return _TV2Fibres.apply(x, w, int(dim))


class _TVpFibres(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, p, dim):
        y = device.tvp_fibres(_colmajor(x.detach()), float(w), p, dim)
        ctx.save_for_backward(y)
        ctx.dim, ctx.w, ctx.p = dim, float(w), p
        ctx.w_device = w.device if isinstance(w, torch.Tensor) else None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[:2]
        res = device.tvp_fibres_vjp(y, gy, ctx.w, ctx.p, ctx.dim, need_glam=need_w)
        gx, glam = res if need_w else (res, None)
        return (gx if need_x else None), (glam.sum().to(ctx.w_device) if need_w else None), None, None


def tvp_fibres(x, w, p, dim):
    """``device.tvp_fibres(x, w, p, dim)`` (the TV-Lp fibre prox, penalty ``w * ||diff||_p`` per fibre, 1.002 < p < 100) with a graph
    behind it: differentiable in x, and in w when w is a 0-d float64 tensor (its gradient comes back on that tensor's device); p is a
    plain number and is not differentiated.  The forward is bit for bit device.tvp_fibres's and saves its output alone; backward is ONE
    device.tvp_fibres_vjp call plus, for w, a sum (the branch the forward took is differentiated).  p = 1 and p = 2 are
    tv1_fibres and tv2_fibres.  When nothing asks for a gradient this IS device.tvp_fibres."""
    _scalar_penalty(w, "w")
    p = float(p)
    if p == 1.0:
        return tv1_fibres(x, w, dim)
    if p == 2.0:
        return tv2_fibres(x, w, dim)
    if not _wants(x, w):
        return device.tvp_fibres(x, float(w), p, dim)
    return _TVpFibres.apply(x, w, p, int(dim))


class _DR2(torch.autograd.Function):
    """x, then the two penalties: 0-d tensors / floats (uniform) or the two per-edge maps (`weighted`)."""

    @staticmethod
    def forward(ctx, x, p_col, p_row, max_iters, weighted, tape, dual):
        xd = _colmajor(x.detach())
        if weighted:
            wc, wr = _colmajor(p_col.detach()), _colmajor(p_row.detach())
            y, _ = device.tv1w_2d(xd, wc, wr, max_iters)
            ctx.save_for_backward(xd, wc, wr)
            if dual:
                ctx.save_for_forward(xd, wc, wr)
        else:
            if xd.dim() == 3:
                y, _ = device.tv1_2d_batch(xd, float(p_col), max_iters)
            else:
                y, _ = device.tv1_2d(xd, float(p_col), max_iters, w_row=float(p_row))
            ctx.save_for_backward(xd)
            if dual:
                ctx.save_for_forward(xd)
            ctx.lams = (float(p_col), float(p_row))
            ctx.lam_devices = tuple(p.device if isinstance(p, torch.Tensor) else None for p in (p_col, p_row))
        ctx.max_iters, ctx.weighted, ctx.tape = max_iters, weighted, tape
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        need_x, need_col, need_row = ctx.needs_input_grad[:3]
        if ctx.weighted:
            x, wc, wr = ctx.saved_tensors
            gx, gc, gr, _, _ = device.dr2_vjp(x, gy, 0.0, max_iters=ctx.max_iters, weights_col=wc, weights_row=wr,
                                              need_gw=need_col or need_row, tape=ctx.tape)
        else:
            (x,) = ctx.saved_tensors
            gx, _, _, glam, _ = device.dr2_vjp(x, gy, ctx.lams[0], ctx.lams[1], ctx.max_iters, need_gw="sums" if need_col or need_row else False,
                                               tape=ctx.tape)
            gc = gr = None
            if glam is not None:
                glam = glam.reshape(-1, 2).sum(axis=0)     # (a batch shares its penalties)
                gc, gr = (None if d is None else torch.tensor(v, dtype=torch.float64, device=d) for v, d in zip(glam, ctx.lam_devices))
        return (gx if need_x else None), (gc if need_col else None), (gr if need_row else None), None, None, None, None

    @staticmethod
    def jvp(ctx, dx, d_col, d_row, *_):
        if ctx.weighted:
            x, wc, wr = ctx.saved_tensors
            return device.dr2_jvp(x, dx, 0.0, max_iters=ctx.max_iters, weights_col=wc, weights_row=wr, dweights_col=d_col,
                                  dweights_row=d_row)[0]
        (x,) = ctx.saved_tensors
        return device.dr2_jvp(x, dx, ctx.lams[0], ctx.lams[1], ctx.max_iters, dw_col=0.0 if d_col is None else float(d_col),
                              dw_row=0.0 if d_row is None else float(d_row))[0]


def _scalar_penalty(w, name):
    if isinstance(w, torch.Tensor) and (w.dim() != 0 or w.dtype != torch.float64):
        raise ValueError(f"{name}: expected a float or a 0-d float64 tensor")


def _wants(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _dual(*ts):
    """Whether any of the tensors carries a forward-mode tangent (torch.autograd.forward_ad)."""
    return any(isinstance(t, torch.Tensor) and torch.autograd.forward_ad.unpack_dual(t).tangent is not None for t in ts)


def tv1_2d(x, w, max_iters=0, w_row=None, tape="outputs"):
    """``device.tv1_2d(x, w, max_iters, w_row=w_row)[0]`` (the Douglas-Rachford solve) with a graph behind it: differentiable in x and in
    w / w_row where they are 0-d float64 tensors (the gradient comes back on that tensor's device; one tensor for both directions
    receives the sum).  The result is bit for bit device.tv1_2d's; when nothing asks for a gradient this IS device.tv1_2d."""
    _scalar_penalty(w, "w")
    _scalar_penalty(w_row, "w_row")
    device._tape(tape)
    dual = _dual(x, w, w_row)
    if not _wants(x, w, w_row) and not dual:
        return device.tv1_2d(x, float(w), max_iters, w_row=None if w_row is None else float(w_row))[0]
    return _DR2.apply(x, w, w if w_row is None else w_row, int(max_iters), False, tape, dual)


def tv1w_2d(x, w_col, w_row, max_iters=0, tape="outputs"):
    """``device.tv1w_2d(x, w_col, w_row, max_iters)[0]`` with a graph behind it: differentiable in x and in both weight maps."""
    device._tape(tape)
    dual = _dual(x, w_col, w_row)
    if not _wants(x, w_col, w_row) and not dual:
        return device.tv1w_2d(x, w_col, w_row, max_iters)[0]
    return _DR2.apply(x, w_col, w_row, int(max_iters), True, tape, dual)


def tv1_2d_batch(xs, w, max_iters=0, tape="outputs"):
    """``device.tv1_2d_batch(xs, w, max_iters)[0]`` on an (M, N, B) stack with a graph behind it: differentiable in xs and in a 0-d
    float64 tensor w (the sum over the images and both directions)."""
    _scalar_penalty(w, "w")
    device._tape(tape)
    dual = _dual(xs, w)
    if not _wants(xs, w) and not dual:
        return device.tv1_2d_batch(xs, float(w), max_iters)[0]
    return _DR2.apply(xs, w, w, int(max_iters), False, tape, dual)


class _DR2p(torch.autograd.Function):
    """x, then the two uniform penalties (0-d tensors / floats); the norms, max_iters and tape ride in `spec`."""

    @staticmethod
    def forward(ctx, x, w_col, w_row, spec):
        p_col, p_row, max_iters, tape = spec
        xd = _colmajor(x.detach())
        y, _ = device.tvp_2d(xd, float(w_col), float(w_row), p_col, p_row, max_iters)
        ctx.save_for_backward(xd)
        ctx.lams, ctx.spec = (float(w_col), float(w_row)), spec
        ctx.lam_devices = tuple(w.device if isinstance(w, torch.Tensor) else None for w in (w_col, w_row))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        p_col, p_row, max_iters, tape = ctx.spec
        need_x, need_col, need_row = ctx.needs_input_grad[:3]
        gx, _, _, glam, _ = device.dr2_vjp(x, gy, ctx.lams[0], ctx.lams[1], max_iters, need_gw="sums" if need_col or need_row else False,
                                           tape=tape, p_col=p_col, p_row=p_row)
        gc = gr = None
        if glam is not None:
            gc, gr = (None if d is None else torch.tensor(float(v), dtype=torch.float64, device=d) for v, d in zip(glam, ctx.lam_devices))
        return (gx if need_x else None), (gc if need_col else None), (gr if need_row else None), None


def tvp_2d(x, w_col, w_row, p_col, p_row, max_iters=0, tape="outputs"):
    """``device.tvp_2d(x, w_col, w_row, p_col, p_row, max_iters)[0]`` (Douglas-Rachford with a TV-L1 or TV-L2 penalty per direction, p in
    {1, 2}) with a graph behind it: differentiable in x and in w_col / w_row where they are 0-d float64 tensors (the gradient comes back on
    that tensor's device; one tensor for both receives the sum).  The result is bit for bit device.tvp_2d's; backward is ONE
    device.dr2_vjp call.  When nothing asks for a gradient this IS device.tvp_2d.  A general p (1.002 < p < 100) needs
    both proxtv_amd.general_p(True), for the fused forward solve, and proxtv_amd.general_p_vjp(True), for backward; the
    error names the one that is missing."""
    _scalar_penalty(w_col, "w_col")
    _scalar_penalty(w_row, "w_row")
    device._tape(tape)
    device._norms((p_col, p_row), 2, "p_col / p_row", forward_too=True)
    if not _wants(x, w_col, w_row):
        return device.tvp_2d(x, float(w_col), float(w_row), p_col, p_row, max_iters)[0]
    return _DR2p.apply(x, w_col, w_row, (float(p_col), float(p_row), int(max_iters), tape))


class _TVGen(torch.autograd.Function):
    """x, then the penalties one by one (0-d tensors / floats); ds, max_iters, method, tape and the norms ride in `spec`."""

    @staticmethod
    def forward(ctx, x, spec, *ws):
        ds, max_iters, method, tape, ps = spec
        xd = _colmajor(x.detach())
        lams = [float(w) for w in ws]
        y, info = device.tvgen(xd, lams, ds, max_iters, method, ps=ps)
        ctx.save_for_backward(xd)
        ctx.lams, ctx.ds, ctx.method, ctx.tape, ctx.ps = lams, ds, method, tape, ps
        ctx.iters = int(info[0])
        ctx.lam_devices = tuple(w.device if isinstance(w, torch.Tensor) else None for w in ws)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        need_x, need_ws = ctx.needs_input_grad[0], ctx.needs_input_grad[2:]
        if x.numel() == 0 or ctx.iters < 1:      # (nothing was iterated: the result does not depend on anything)
            gx, glam = torch.zeros_like(x), [0.0] * len(ctx.lams)
        else:
            gx, glam, _ = device.tvgen_vjp(x, gy, ctx.lams, ctx.ds, ctx.iters, ctx.method, need_glam=any(need_ws), tape=ctx.tape, ps=ctx.ps)
        gws = tuple(torch.tensor(float(glam[i]), dtype=torch.float64, device=ctx.lam_devices[i]) if need else None
                    for i, need in enumerate(need_ws))
        return ((gx if need_x else None), None) + gws


def tvgen(x, ws, ds, max_iters=0, method=None, tape="outputs", ps=None):
    """``device.tvgen(x, ws, ds, max_iters, method)[0]`` with a graph behind it: differentiable in x and in every entry of `ws` that is a
    0-d float64 tensor (its gradient comes back on that tensor's device; a tensor that appears in several entries receives the sum).
    method: None (tvgen's dispatch), 'pd2' or 'pd'; 'pdr' and 'yang' raise NotImplementedError when a gradient is asked for.  The result
    is bit for bit device.tvgen's; when nothing asks for a gradient this IS device.tvgen.  Backward differentiates the iterations the
    forward ran (its info[0]), not the dependence of their number on the data.  ps (one of {1, 2} per term, or None = all 1): the norm
    of every term's penalty, as device.tvgen takes it; a general p (1.002 < p < 100) needs both proxtv_amd.general_p(True)
    and proxtv_amd.general_p_vjp(True)."""
    ws = list(ws)
    ps = None if ps is None else tuple(float(p) for p in device._norms(ps, len(ws), forward_too=True))
    for i, w in enumerate(ws):
        _scalar_penalty(w, f"ws[{i}]")
    device._tape(tape)
    if not _wants(x, *ws):
        return device.tvgen(x, [float(w) for w in ws], ds, max_iters, method, ps=ps)[0]
    m = method if method is not None else ("pd2" if len(ws) == 2 else "pd")
    if m not in ("pd2", "pd"):
        raise NotImplementedError(f"method {m!r} has no derivative (autograd.tvgen covers 'pd2' and 'pd')")
    return _TVGen.apply(x, (tuple(float(d) for d in ds), int(max_iters), method, tape, ps), *ws)

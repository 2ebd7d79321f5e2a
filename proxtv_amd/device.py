"""Device-resident entry points: operate on torch tensors that already live in HBM.

torch is plumbing here (device memory + streams); every solve is the HIP path of libproxtv_amd.so reached through
the ``proxtv_*_dev`` C entry points of include/proxtv_amd.h.  Arrays follow the library's column-major convention:
an (M, N) image is passed as a tensor whose *transpose* is contiguous (``colmajor_empty`` / ``to_colmajor`` build
such tensors); N-D arrays likewise have dimension 0 fastest.
"""
import numpy as np
import torch

from . import _lib

_N_INFO = 3


def colmajor_empty(shape, device="cuda", dtype=torch.float64):
    """Uninitialised tensor of logical `shape` stored column-major (dimension 0 fastest)."""
    rev = tuple(reversed(tuple(shape)))
    return torch.empty(rev, device=device, dtype=dtype).permute(*reversed(range(len(rev))))


def to_colmajor(t):
    """Copy `t` (any layout) into column-major storage on its device."""
    out = colmajor_empty(t.shape, device=t.device, dtype=torch.float64)
    out.copy_(t)
    return out


def _is_colmajor(t):
    return t.permute(*reversed(range(t.dim()))).is_contiguous()


def _check(t, name, like=None, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and _is_colmajor(t)):
        raise ValueError(f"{name}: expected a float64 CUDA tensor in column-major storage (see to_colmajor)")
    if like is not None and t.device != like.device:
        raise ValueError(f"{name}: lives on {t.device}, the input on {like.device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")


def _out(out, x, name="out"):
    """The output tensor: a fresh column-major one on x's device, or the caller's (checked: a tensor of another
    dtype / layout / shape / device would be filled with the wrong bytes or fault).  It may alias x: the library
    detects the overlap and solves through a scratch array."""
    if out is None:
        return colmajor_empty(x.shape, device=x.device)
    _check(out, name, like=x, shape=x.shape)
    return out


def _stream(dev):
    """hipStream_t handle for the C-ABI: torch's current stream ON THE TENSOR'S DEVICE (callers run under
    ``torch.cuda.device(x.device)``: the library keeps its state per device and uses the current one).  torch's legacy
    default stream has handle 0, which the library reads as "use my own per-thread (non-blocking) stream"; that stream
    does not order against the null stream, so drain torch's producers first.  Every *_dev entry point synchronises
    before returning, so consumers need no extra fence."""
    cur = torch.cuda.current_stream(dev)
    if cur.cuda_stream == 0:
        cur.synchronize()
    return cur.cuda_stream


def tv1_2d(x, w, max_iters=0, method="dr", out=None, w_row=None):
    """tv1_2d on an HBM-resident (M, N) image.  Returns (y, info)."""
    _check(x, "x")
    with torch.cuda.device(x.device):
        return _tv1_2d(x, w, max_iters, method, _out(out, x), w_row)


def _tv1_2d(x, w, max_iters, method, y, w_row):
    lib = _lib.require_device()
    info = np.zeros(_N_INFO)
    M, N = x.shape
    w_row = w if w_row is None else w_row
    _stream = lambda: globals()["_stream"](x.device)   # noqa: E731
    if method == "dr":
        lib.proxtv_DR2_TV_dev(M, N, x.data_ptr(), float(w), float(w_row), y.data_ptr(), int(max_iters),
                              info.ctypes.data, _stream())
    elif method == "pd":
        lam = np.array([w, w_row], dtype=np.float64)
        dims = np.array([1.0, 2.0])
        ns = np.array([M, N], dtype=np.int32)
        lib.proxtv_PD2_TV_dev(x.data_ptr(), lam.ctypes.data, dims.ctypes.data, y.data_ptr(), info.ctypes.data,
                              ns.ctypes.data, 2, 2, int(max_iters), _stream())
    elif method == "yang":
        lam = np.array([w, w_row], dtype=np.float64)
        ns = np.array([M, N], dtype=np.int32)
        lib.proxtv_Yang_TV_dev(ns.ctypes.data, 2, x.data_ptr(), lam.ctypes.data, y.data_ptr(), int(max_iters),
                               info.ctypes.data, _stream())
    elif method == "kolmogorov":
        lib.proxtv_Kolmogorov2_TV_dev(M, N, x.data_ptr(), float(w), y.data_ptr(), int(max_iters), info.ctypes.data, _stream())
    elif method in ("condat", "chambolle-pock", "chambolle-pock-acc"):
        alg = {"condat": 0, "chambolle-pock": 1, "chambolle-pock-acc": 2}[method]
        lib.proxtv_CondatChambollePock2_TV_dev(M, N, x.data_ptr(), float(w), y.data_ptr(), alg, int(max_iters),
                                               info.ctypes.data, _stream())
    else:
        raise NotImplementedError(method)
    _lib.check("device.tv1_2d")
    return y, info


def tv1w_2d(x, w_col, w_row, max_iters=0, out=None):
    """Weighted DR on HBM-resident arrays: w_col (M-1, N), w_row (M, N-1), all column-major."""
    _check(x, "x")
    M, N = x.shape
    _check(w_col, "w_col", like=x, shape=(M - 1, N))
    _check(w_row, "w_row", like=x, shape=(M, N - 1))
    y = _out(out, x)
    info = np.zeros(_N_INFO)
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        lib.proxtv_DR2L1W_TV_dev(M, N, x.data_ptr(), w_col.data_ptr(), w_row.data_ptr(), y.data_ptr(), int(max_iters),
                                 info.ctypes.data, _stream(x.device))
    _lib.check("device.tv1w_2d")
    return y, info


def tv1_2d_batch(xs, w, max_iters=0, out=None):
    """DR on a stack of B images held as a column-major (M, N, B) tensor (image b = xs[:, :, b])."""
    _check(xs, "xs")
    y = _out(out, xs)
    info = np.zeros(_N_INFO)
    M, N, B = xs.shape
    with torch.cuda.device(xs.device):
        lib = _lib.require_device()
        lib.proxtv_DR2_TV_batch_dev(M, N, B, xs.data_ptr(), float(w), float(w), y.data_ptr(), int(max_iters),
                                    info.ctypes.data, _stream(xs.device))
    _lib.check("device.tv1_2d_batch")
    return y, info


def _norm_array(ps, count, what):
    norms = np.array(ps, dtype=np.float64).reshape(-1)
    if norms.size != count:
        raise ValueError(f"{what}: {norms.size} norms for {count} penalties")
    return norms


def _norms(ps, count, what="ps", forward_too=False):
    """The norms of `count` terms as the derivative calls take them (float64, each 1 or 2 whatever option general_p says; with option
    general_p_vjp any 1.002 < p < 100), or None for ps = None.  `forward_too`: _lib.check_vjp_norms."""
    if ps is None:
        return None
    norms = _norm_array(ps, count, what)
    if not np.all((norms == 1) | (norms == 2)):
        try:
            _lib.check_vjp_norms(norms, forward_too)
        except NotImplementedError as e:
            if _lib.option_value("general_p_vjp") or (forward_too and _lib.option_value("general_p")):
                raise NotImplementedError(f"{what}: {e}") from None
            raise NotImplementedError(f"{what}: only p = 1 (TV-L1) and p = 2 (TV-L2) are implemented on the device, got {list(norms)}") from None
    return norms


def _forward_norms(ps, count, what="ps"):
    """The norms of `count` terms as the forward solves take them: 1 or 2, and with option general_p any 1.002 < p < 100."""
    if ps is None:
        return None
    norms = _norm_array(ps, count, what)
    if not np.all((norms == 1) | (norms == 2)):
        try:
            _lib.check_forward_norms(norms)
        except NotImplementedError as e:
            if _lib.option_value("general_p"):
                raise NotImplementedError(f"{what}: {e}") from None
            raise NotImplementedError(f"{what}: only p = 1 (TV-L1) and p = 2 (TV-L2) are implemented on the device, got {list(norms)}") from None
    return norms


def tvp_2d(x, w_col, w_row, p_col, p_row, max_iters=0, out=None):
    """Douglas-Rachford on an HBM-resident (M, N) image with the penalty ``w_col * ||diff||_{p_col}`` on every column and
    ``w_row * ||diff||_{p_row}`` on every row, p in {1, 2} -- with proxtv_amd.general_p(True) any 1.002 < p < 100 (proxtv_DR2_TVp_dev).
    Returns (y, info)."""
    _check(x, "x")
    if x.dim() != 2:
        raise ValueError(f"x: expected an (M, N) image, got {x.dim()} dimensions")
    norms = _forward_norms((p_col, p_row), 2, "p_col / p_row")
    y = _out(out, x)
    info = np.zeros(_N_INFO)
    M, N = x.shape
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        lib.proxtv_DR2_TVp_dev(M, N, x.data_ptr(), float(w_col), float(w_row), norms[0], norms[1], y.data_ptr(), int(max_iters),
                               info.ctypes.data, _stream(x.device))
    _lib.check("device.tvp_2d")
    return y, info


def tvgen(x, ws, ds, max_iters=0, method=None, out=None, ps=None):
    """N-D TV-L1 on an HBM-resident column-major array.  method: None = reference dispatch (2 terms -> 'pd2',
    otherwise 'pd'); 'pdr' = parallel Douglas-Rachford; 'yang' = Yang ADMM (2-D / 3-D, one lambda per dim).
    ps (one of {1, 2} per term, or None = all 1): the norm of every term's penalty, ``w * ||diff||_p`` per fibre
    (proxtv_PD_TVp_dev; 'pd2', 'pd' and 'pdr').  With proxtv_amd.general_p(True), 'pd2' and 'pd' also take any 1.002 < p < 100."""
    _check(x, "x")
    with torch.cuda.device(x.device):
        return _tvgen(x, ws, ds, max_iters, method, _out(out, x), ps)


def _tvgen(x, ws, ds, max_iters, method, y, ps=None):
    lib = _lib.require_device()
    info = np.zeros(_N_INFO)
    ns = np.array(x.shape, dtype=np.int32)
    lam = np.array(ws, dtype=np.float64)
    dims = np.array(ds, dtype=np.float64)
    npen = lam.size
    _stream = lambda: globals()["_stream"](x.device)   # noqa: E731
    if method is None:
        method = "pd2" if npen == 2 else "pd"
    norms = _forward_norms(ps, npen) if method in ("pd2", "pd") else _norms(ps, npen)
    if norms is not None:
        if method not in ("pd2", "pd", "pdr"):
            raise NotImplementedError(f"method {method!r} takes no norms (ps goes with 'pd2', 'pd' and 'pdr')")
        which = {"pd2": 0, "pd": 1, "pdr": 2}[method]
        scaled = lam * (1 if which == 0 else npen)
        lib.proxtv_PD_TVp_dev(which, x.data_ptr(), scaled.ctypes.data, norms.ctypes.data, dims.ctypes.data, y.data_ptr(),
                              info.ctypes.data, ns.ctypes.data, x.dim(), npen, int(max_iters), _stream())
    elif method == "pd2":
        lib.proxtv_PD2_TV_dev(x.data_ptr(), lam.ctypes.data, dims.ctypes.data, y.data_ptr(), info.ctypes.data,
                              ns.ctypes.data, x.dim(), npen, int(max_iters), _stream())
    elif method in ("pd", "pdr"):
        scaled = lam * npen     # the host entry points scale in caller memory (src/TVNDopt.cpp:100-101); here explicit
        fn = lib.proxtv_PD_TV_dev if method == "pd" else lib.proxtv_PDR_TV_dev
        fn(x.data_ptr(), scaled.ctypes.data, dims.ctypes.data, y.data_ptr(), info.ctypes.data, ns.ctypes.data,
           x.dim(), npen, int(max_iters), _stream())
    elif method == "yang":
        lib.proxtv_Yang_TV_dev(ns.ctypes.data, x.dim(), x.data_ptr(), lam.ctypes.data, y.data_ptr(), int(max_iters),
                               info.ctypes.data, _stream())
    else:
        raise NotImplementedError(method)
    _lib.check("device.tvgen")
    return y, info


def tv1_fibres(x, w, dim, weights=None, out=None):
    """Batched exact 1-D TV-L1 prox of every fibre of `x` along 0-based `dim` (the per-sweep kernel)."""
    _check(x, "x")
    y = _out(out, x)
    ns = np.array(x.shape, dtype=np.int32)
    if not 0 <= int(dim) < x.dim():
        raise ValueError(f"dim {dim} out of range for a {x.dim()}-D array")
    wp = 0
    if weights is not None:
        wshape = list(x.shape)
        wshape[int(dim)] -= 1              # one penalty per edge along the fibre
        _check(weights, "weights", like=x, shape=wshape)
        wp = weights.data_ptr()
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        lib.proxtv_tv1_fibres_dev(x.data_ptr(), y.data_ptr(), ns.ctypes.data, x.dim(), int(dim), float(w), wp,
                                  _stream(x.device))
    _lib.check("device.tv1_fibres")
    return y


def certify_fibres(x, y, w, dim, weights=None):
    """The certificate of ``y = tv1_fibres(x, w, dim)``: the number of fibres along `dim` for which `y` is NOT the exact TV-L1 prox of
    `x` (optimality conditions of the 1-D problem, fibre by fibre, within rounding).  0: `y` is the prox.  -1: nothing to check
    (w <= 0 without weights, or y is x)."""
    _check(x, "x")
    _check(y, "y", like=x, shape=x.shape)
    ns = np.array(x.shape, dtype=np.int32)
    if not 0 <= int(dim) < x.dim():
        raise ValueError(f"dim {dim} out of range for a {x.dim()}-D array")
    wp = 0
    if weights is not None:
        wshape = list(x.shape)
        wshape[int(dim)] -= 1
        _check(weights, "weights", like=x, shape=wshape)
        wp = weights.data_ptr()
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        failed = lib.proxtv_certify_fibres_dev(x.data_ptr(), y.data_ptr(), ns.ctypes.data, x.dim(), int(dim), float(w), wp,
                                               _stream(x.device))
    if failed == -2:
        _lib.check("device.certify_fibres")
    return int(failed)


def _counts_empty(shape, dim, device):
    """int32 tensor with the shape of an array without its dimension `dim`, column-major (0-d for a 1-D array)."""
    rest = tuple(s for i, s in enumerate(shape) if i != dim)
    if not rest:
        return torch.empty((), device=device, dtype=torch.int32)
    return colmajor_empty(rest, device=device, dtype=torch.int32)


def tv1_fibres_vjp(y, g, dim, need_gw=False, need_nseg=False, out=None):
    """The derivative of ``y = tv1_fibres(x, w, dim[, weights])`` applied to `g`: returns (gx, gw | None, nseg | None).

    gx = P g, where P = dy/dx replaces every sample by the mean over its segment of `y` (the runs between the steps of `y` along
    `dim`; step rule and its limits: include/proxtv_amd.h) -- P is symmetric, so this is the VJP and the JVP in x.  gw (`need_gw`) is
    the gradient in the per-edge penalties, shaped like `weights`; for a uniform penalty d/dw is ``gw.sum()``.  nseg (`need_nseg`) holds
    the segments of every fibre (int32, the shape of `y` without `dim`): trace P, the degrees of freedom.  Only `y` is needed, neither
    x nor the penalties.  A `g` in another layout is copied; `out` may be `g`."""
    _check(y, "y")
    if not 0 <= int(dim) < y.dim():
        raise ValueError(f"dim {dim} out of range for a {y.dim()}-D array")
    dim = int(dim)
    if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64):
        raise ValueError("g: expected a float64 CUDA tensor")
    if g.device != y.device:
        raise ValueError(f"g: lives on {g.device}, the input on {y.device}")
    if tuple(g.shape) != tuple(y.shape):
        raise ValueError(f"g: shape {tuple(g.shape)}, expected {tuple(y.shape)}")
    if not _is_colmajor(g):
        g = to_colmajor(g)
    gx = _out(out, y)
    ns = np.array(y.shape, dtype=np.int32)
    gw = nseg = None
    if need_gw:
        wshape = list(y.shape)
        wshape[dim] -= 1
        gw = colmajor_empty(wshape, device=y.device)
    if need_nseg:
        nseg = _counts_empty(y.shape, dim, y.device)
    with torch.cuda.device(y.device):
        lib = _lib.require_device()
        lib.proxtv_tv1_fibres_vjp_dev(y.data_ptr(), g.data_ptr(), gx.data_ptr(), gw.data_ptr() if need_gw and gw.numel() else 0,
                                      nseg.data_ptr() if need_nseg and nseg.numel() else 0, ns.ctypes.data, y.dim(), dim,
                                      _stream(y.device))
    _lib.check("device.tv1_fibres_vjp")
    return gx, gw, nseg


def tv1_fibres_steps(y, dim):
    """The step codes of ``y = tv1_fibres(x, w, dim[, weights])``: a 1-D int32 tensor, one 32-bit word per chunk of 16 samples of a fibre
    (bit k: the edge behind sample k of the chunk is a step; bit 16 + k: it steps up -- include/proxtv_amd.h).  They are all
    tv1_fibres_vjp reads of `y`, in 1/32 of its bytes: ``tv1_fibres_vjp_steps(steps, g, y.shape, dim)`` returns the bits of
    ``tv1_fibres_vjp(y, g, dim)``.  The order of the words is the library's own and holds for the same shape and `dim`."""
    _check(y, "y")
    if not 0 <= int(dim) < y.dim():
        raise ValueError(f"dim {dim} out of range for a {y.dim()}-D array")
    ns = np.array(y.shape, dtype=np.int32)
    with torch.cuda.device(y.device):
        lib = _lib.require_device()
        steps = torch.empty(lib.proxtv_tv1_steps_words(ns.ctypes.data, y.dim(), int(dim)), device=y.device, dtype=torch.int32)
        lib.proxtv_tv1_fibres_steps_dev(y.data_ptr(), steps.data_ptr() if steps.numel() else 0, ns.ctypes.data, y.dim(), int(dim),
                                        _stream(y.device))
    _lib.check("device.tv1_fibres_steps")
    return steps


def tv1_fibres_vjp_steps(steps, g, shape, dim, need_gw=False, need_nseg=False, out=None):
    """``tv1_fibres_vjp(y, g, dim, ...)`` from ``steps = tv1_fibres_steps(y, dim)`` instead of `y` (`shape` is y's): the same
    (gx, gw | None, nseg | None), bit for bit.  g = None: the segment counts alone, (None, None, nseg)."""
    shape = tuple(int(v) for v in shape)
    dim = int(dim)
    if not 0 <= dim < len(shape):
        raise ValueError(f"dim {dim} out of range for a {len(shape)}-D array")
    if not (isinstance(steps, torch.Tensor) and steps.is_cuda and steps.dtype == torch.int32 and steps.is_contiguous()):
        raise ValueError("steps: expected a contiguous int32 CUDA tensor (device.tv1_fibres_steps)")
    ns = np.array(shape, dtype=np.int32)
    lib = _lib.load()
    if steps.numel() != lib.proxtv_tv1_steps_words(ns.ctypes.data, len(shape), dim):
        raise ValueError(f"steps: {steps.numel()} words, an array of shape {shape} has "
                         f"{lib.proxtv_tv1_steps_words(ns.ctypes.data, len(shape), dim)} along dimension {dim}")
    gx = gw = nseg = None
    if g is not None:
        if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64):
            raise ValueError("g: expected a float64 CUDA tensor")
        if g.device != steps.device:
            raise ValueError(f"g: lives on {g.device}, the steps on {steps.device}")
        if tuple(g.shape) != shape:
            raise ValueError(f"g: shape {tuple(g.shape)}, expected {shape}")
        if not _is_colmajor(g):
            g = to_colmajor(g)
        gx = _out(out, g)
        if need_gw:
            wshape = list(shape)
            wshape[dim] -= 1
            gw = colmajor_empty(wshape, device=g.device)
    if need_nseg or g is None:
        nseg = _counts_empty(shape, dim, steps.device)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0   # noqa: E731
    with torch.cuda.device(steps.device):
        lib = _lib.require_device()
        lib.proxtv_tv1_fibres_vjp_steps_dev(ptr(steps), ptr(g), ptr(gx), ptr(gw), ptr(nseg), ns.ctypes.data, len(shape), dim,
                                            _stream(steps.device))
    _lib.check("device.tv1_fibres_vjp_steps")
    return gx, gw, nseg


def _tape(tape):
    if tape not in ("outputs", "steps"):
        raise ValueError(f"tape: 'outputs' or 'steps', got {tape!r}")
    return 1 if tape == "steps" else 0


def dr2_vjp(x, g, w_col, w_row=None, max_iters=0, weights_col=None, weights_row=None, need_gw=False, need_y=False, tape="outputs",
            p_col=1, p_row=1):
    """The derivative of the Douglas-Rachford solves ``tv1_2d(x, w_col, w_row=w_row)`` / ``tv1w_2d(x, weights_col, weights_row)`` /
    ``tv1_2d_batch`` applied to the cotangent `g` of their result: returns (gx, gw_col, gw_row, glam, y).

    `x` and `g` are (M, N), or (M, N, B) for a batch of independent images.  gx is the gradient in x.  With `need_gw`, gw_col / gw_row are
    the gradients in the per-edge penalties (the shapes of `weights_col` / `weights_row`, also for a uniform penalty) and glam, a numpy
    array of shape (2,) or (B, 2), their sums per image: the gradients in a uniform (w_col, w_row).  ``need_gw="sums"`` returns glam
    alone.  y (`need_y`) is the forward result of the call's own, unfused recurrence: device.tv1_2d's up to rounding.  One call:
    proxtv_DR2_TV_vjp_tape_dev (include/proxtv_amd.h), which keeps 2 (max_iters + 1) arrays of x's size in pool scratch while it runs
    -- or, with ``tape="steps"``, the step codes of those arrays (1/32 of the bytes) and two arrays of x's size; every result is the same
    bits.  A `g` in another layout is copied.

    p_col / p_row in {1, 2}: the derivative of ``tvp_2d(x, w_col, w_row, p_col, p_row)`` (proxtv_DR2_TVp_vjp_dev) -- one (M, N) image,
    uniform penalties only.  A TV-L2 direction has no per-edge gradient: gw_col / gw_row come back None and glam (`need_gw`) holds the
    gradients in (w_col, w_row).  Its sweeps keep their float64 output and one multiplier per fibre under either tape.  With
    proxtv_amd.general_p_vjp(True) a direction also takes any 1.002 < p < 100: the same conventions, its sweeps keep their
    float64 output alone; the call replays the forward itself and does not ask for option general_p."""
    _check(x, "x")
    tape = _tape(tape)
    norms = _norms((p_col, p_row), 2, "p_col / p_row")
    if np.any(norms != 1):
        if weights_col is not None or weights_row is not None:
            raise ValueError("per-edge weight maps go with p = 1 only: TV-L2 and TV-Lp have one penalty per fibre")
        return _dr2p_vjp(x, g, w_col, w_col if w_row is None else w_row, norms, max_iters, need_gw, need_y, tape)
    if x.dim() not in (2, 3):
        raise ValueError(f"x: expected an (M, N) image or an (M, N, B) batch, got {x.dim()} dimensions")
    if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64):
        raise ValueError("g: expected a float64 CUDA tensor")
    if g.device != x.device:
        raise ValueError(f"g: lives on {g.device}, the input on {x.device}")
    if tuple(g.shape) != tuple(x.shape):
        raise ValueError(f"g: shape {tuple(g.shape)}, expected {tuple(x.shape)}")
    if not _is_colmajor(g):
        g = to_colmajor(g)
    if (weights_col is None) != (weights_row is None):
        raise ValueError("weights_col and weights_row come in pairs")
    M, N = x.shape[:2]
    B = x.shape[2] if x.dim() == 3 else 1
    tail = tuple(x.shape[2:])
    shape_col, shape_row = (max(M - 1, 0), N) + tail, (M, max(N - 1, 0)) + tail
    if weights_col is not None:
        _check(weights_col, "weights_col", like=x, shape=shape_col)
        _check(weights_row, "weights_row", like=x, shape=shape_row)
    w_row = w_col if w_row is None else w_row
    gx = colmajor_empty(x.shape, device=x.device)
    y = colmajor_empty(x.shape, device=x.device) if need_y else None
    gw_col = gw_row = glam = None
    if need_gw:
        glam = np.zeros((B, 2))
        if need_gw != "sums":
            gw_col = colmajor_empty(shape_col, device=x.device)
            gw_row = colmajor_empty(shape_row, device=x.device)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0   # noqa: E731
    # (a weight map without edges -- M == 1 or N == 1 -- has no storage: any non-null address says "weighted", nothing is read through it)
    wptr = lambda t: 0 if t is None else (ptr(t) or x.data_ptr())        # noqa: E731
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        lib.proxtv_DR2_TV_vjp_tape_dev(M, N, B, ptr(x), float(w_col), float(w_row), wptr(weights_col), wptr(weights_row), ptr(g),
                                       ptr(y), ptr(gx), ptr(gw_col), ptr(gw_row), glam.ctypes.data if need_gw else 0, int(max_iters),
                                       tape, _stream(x.device))
    _lib.check("device.dr2_vjp")
    if glam is not None and x.dim() == 2:
        glam = glam[0]
    return gx, gw_col, gw_row, glam, y


def _tangent(t, name, like, shape):
    """A tangent array for the forward-mode calls: None stays None (zero); a float64 CUDA tensor of `shape` on like's device, copied
    into column-major storage when it has another layout."""
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64):
        raise ValueError(f"{name}: expected a float64 CUDA tensor")
    if t.device != like.device:
        raise ValueError(f"{name}: lives on {t.device}, the input on {like.device}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t if _is_colmajor(t) else to_colmajor(t)


def tv1_fibres_jvp(y, dx, dim, dweights=None, dw=0.0, out=None):
    """The forward-mode derivative of ``y = tv1_fibres(x, w, dim[, weights])``: the tangent dy of `y` for the tangents `dx` of x (None:
    zero), `dweights` of the per-edge penalties (shaped like `weights`, None: zero) and the float `dw` of a uniform penalty, which is
    added on every edge.

    dy = P (dx + E), where P replaces every sample by the mean over its segment of `y` and E[i] = sigma_i dr_i - sigma_{i-1} dr_{i-1}
    with dr = dweights + dw and sigma = +1 / -1 / 0 on a step up / a step down / an edge that is no step (rule and limits:
    include/proxtv_amd.h).  It is the exact transpose of tv1_fibres_vjp.  Only `y` is needed, neither x nor the penalties.  Tangents in
    another layout are copied; `out` may be `dx`.  One call: proxtv_tv1_fibres_jvp_dev."""
    _check(y, "y")
    if not 0 <= int(dim) < y.dim():
        raise ValueError(f"dim {dim} out of range for a {y.dim()}-D array")
    dim = int(dim)
    wshape = list(y.shape)
    wshape[dim] = max(wshape[dim] - 1, 0)
    dx = _tangent(dx, "dx", y, y.shape)
    dweights = _tangent(dweights, "dweights", y, wshape)
    dy = _out(out, y)
    ns = np.array(y.shape, dtype=np.int32)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0   # noqa: E731
    with torch.cuda.device(y.device):
        lib = _lib.require_device()
        lib.proxtv_tv1_fibres_jvp_dev(ptr(y), ptr(dx), ptr(dweights), float(dw), ptr(dy), ns.ctypes.data, y.dim(), dim, _stream(y.device))
    _lib.check("device.tv1_fibres_jvp")
    return dy


def dr2_jvp(x, dx, w_col, w_row=None, max_iters=0, weights_col=None, weights_row=None, dw_col=0.0, dw_row=0.0, dweights_col=None,
            dweights_row=None, need_y=False):
    """The forward-mode derivative of the Douglas-Rachford solves ``tv1_2d(x, w_col, w_row=w_row)`` / ``tv1w_2d(x, weights_col,
    weights_row)`` / ``tv1_2d_batch``: returns (dy, y), the tangent of their result for the tangents `dx` of x (None: zero), the floats
    `dw_col` / `dw_row` of uniform penalties and `dweights_col` / `dweights_row` of the per-edge penalties (the shapes of `weights_col` /
    `weights_row`, None: zero; a uniform and a per-edge tangent of one direction add up).

    `x` is (M, N), or (M, N, B) for a batch of independent images.  y (`need_y`) is the forward result of the call's own, unfused
    recurrence -- the bits of ``dr2_vjp(..., need_y=True)``, device.tv1_2d's up to rounding.  One call: proxtv_DR2_TV_jvp_dev
    (include/proxtv_amd.h), which forms the tangent of every sweep next to the sweep and keeps nothing between iterations: its scratch is
    six arrays of x's size whatever `max_iters`, where dr2_vjp keeps 2 (max_iters + 1).  Tangents in another layout are copied."""
    _check(x, "x")
    if x.dim() not in (2, 3):
        raise ValueError(f"x: expected an (M, N) image or an (M, N, B) batch, got {x.dim()} dimensions")
    if (weights_col is None) != (weights_row is None):
        raise ValueError("weights_col and weights_row come in pairs")
    M, N = x.shape[:2]
    B = x.shape[2] if x.dim() == 3 else 1
    tail = tuple(x.shape[2:])
    shape_col, shape_row = (max(M - 1, 0), N) + tail, (M, max(N - 1, 0)) + tail
    if weights_col is not None:
        _check(weights_col, "weights_col", like=x, shape=shape_col)
        _check(weights_row, "weights_row", like=x, shape=shape_row)
    dx = _tangent(dx, "dx", x, x.shape)
    dweights_col = _tangent(dweights_col, "dweights_col", x, shape_col)
    dweights_row = _tangent(dweights_row, "dweights_row", x, shape_row)
    w_row = w_col if w_row is None else w_row
    dy = colmajor_empty(x.shape, device=x.device)
    y = colmajor_empty(x.shape, device=x.device) if need_y else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0   # noqa: E731
    # (a weight map without edges -- M == 1 or N == 1 -- has no storage: any non-null address says "weighted", nothing is read through it)
    wptr = lambda t: 0 if t is None else (ptr(t) or x.data_ptr())        # noqa: E731
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        lib.proxtv_DR2_TV_jvp_dev(M, N, B, ptr(x), float(w_col), float(w_row), wptr(weights_col), wptr(weights_row), ptr(dx),
                                  ptr(dweights_col), ptr(dweights_row), float(dw_col), float(dw_row), ptr(y), ptr(dy), int(max_iters),
                                  _stream(x.device))
    _lib.check("device.dr2_jvp")
    return dy, y


def _cotangent(g, x):
    if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64):
        raise ValueError("g: expected a float64 CUDA tensor")
    if g.device != x.device:
        raise ValueError(f"g: lives on {g.device}, the input on {x.device}")
    if tuple(g.shape) != tuple(x.shape):
        raise ValueError(f"g: shape {tuple(g.shape)}, expected {tuple(x.shape)}")
    return g if _is_colmajor(g) else to_colmajor(g)


def _dr2p_vjp(x, g, w_col, w_row, norms, max_iters, need_gw, need_y, tape):
    if x.dim() != 2:
        raise ValueError(f"x: a TV-L2 or TV-Lp direction takes one (M, N) image, got {x.dim()} dimensions")
    g = _cotangent(g, x)
    M, N = x.shape
    gx = colmajor_empty(x.shape, device=x.device)
    y = colmajor_empty(x.shape, device=x.device) if need_y else None
    glam = np.zeros(2) if need_gw else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0   # noqa: E731
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        lib.proxtv_DR2_TVp_vjp_dev(M, N, ptr(x), float(w_col), float(w_row), norms[0], norms[1], ptr(g), ptr(y), ptr(gx),
                                   glam.ctypes.data if need_gw else 0, int(max_iters), tape, _stream(x.device))
    _lib.check("device.dr2_vjp")
    return gx, None, None, glam, y


def tvgen_vjp(x, g, ws, ds, iters, method=None, need_glam=False, need_y=False, tape="outputs", ps=None):
    """The derivative of ``tvgen(x, ws, ds, method=method)`` applied to the cotangent `g` of its result: returns (gx, glam, y).

    `iters` is the iteration count the forward solve reported (``info[0]``): the call runs exactly that many iterations of its own,
    unfused recurrence and differentiates those -- the dependence of the count on the data through the stopping rule is not differentiated.
    method follows tvgen's dispatch (None: 'pd2' for two terms, otherwise 'pd'); 'pdr' and 'yang' have no derivative.  gx is the gradient
    in x.  glam (`need_glam`) is a numpy array with the gradient in every entry of `ws` as the user passes them (for 'pd' the library
    works with ws * len(ws); the chain rule through that scaling is applied here).  y (`need_y`) is the forward result of the call's own
    recurrence: tvgen's up to rounding.  One call: proxtv_PD_TV_vjp_tape_dev (include/proxtv_amd.h), which keeps len(ws) * iters ('pd') or
    2 * iters ('pd2') arrays of x's size in pool scratch while it runs -- or, with ``tape="steps"``, their step codes (1/32 of the bytes)
    and one array of x's size per term; every result is the same bits.  A `g` in another layout is copied.

    ps (one of {1, 2} per term, or None = all 1): the derivative of ``tvgen(x, ws, ds, method=method, ps=ps)``
    (proxtv_PD_TVp_vjp_dev); a TV-L2 term's sweeps keep their float64 output and one multiplier per fibre under either tape.  With
    proxtv_amd.general_p_vjp(True) a term also takes any 1.002 < p < 100: its sweeps keep their float64 output alone."""
    _check(x, "x")
    tape = _tape(tape)
    if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64):
        raise ValueError("g: expected a float64 CUDA tensor")
    if g.device != x.device:
        raise ValueError(f"g: lives on {g.device}, the input on {x.device}")
    if tuple(g.shape) != tuple(x.shape):
        raise ValueError(f"g: shape {tuple(g.shape)}, expected {tuple(x.shape)}")
    if not _is_colmajor(g):
        g = to_colmajor(g)
    lam = np.array(ws, dtype=np.float64).reshape(-1)
    dims = np.array(ds, dtype=np.float64).reshape(-1)
    npen = lam.size
    if dims.size != npen:
        raise ValueError(f"ds: {dims.size} dimensions for {npen} penalties")
    norms = _norms(ps, npen)
    if method is None:
        method = "pd2" if npen == 2 else "pd"
    if method not in ("pd2", "pd"):
        raise NotImplementedError(f"method {method!r} has no derivative (tvgen_vjp covers 'pd2' and 'pd')")
    scale = float(npen) if method == "pd" else 1.0     # (device.tvgen hands PD_TV the npen-scaled penalties)
    scaled = lam * scale
    ns = np.array(x.shape, dtype=np.int32)
    gx = colmajor_empty(x.shape, device=x.device)
    y = colmajor_empty(x.shape, device=x.device) if need_y else None
    glam = np.zeros(npen) if need_glam else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0   # noqa: E731
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        if norms is None:
            lib.proxtv_PD_TV_vjp_tape_dev(0 if method == "pd2" else 1, ptr(x), scaled.ctypes.data, dims.ctypes.data, ns.ctypes.data, x.dim(),
                                          npen, int(iters), ptr(g), ptr(y), ptr(gx), glam.ctypes.data if need_glam else 0, tape,
                                          _stream(x.device))
        else:
            lib.proxtv_PD_TVp_vjp_dev(0 if method == "pd2" else 1, ptr(x), scaled.ctypes.data, norms.ctypes.data, dims.ctypes.data,
                                      ns.ctypes.data, x.dim(), npen, int(iters), ptr(g), ptr(y), ptr(gx),
                                      glam.ctypes.data if need_glam else 0, tape, _stream(x.device))
    _lib.check("device.tvgen_vjp")
    if glam is not None:
        glam *= scale
    return gx, glam, y


def _per_fibre_empty(shape, dim, device):
    """float64 tensor with the shape of an array without its dimension `dim`, column-major (0-d for a 1-D array)."""
    rest = tuple(s for i, s in enumerate(shape) if i != dim)
    if not rest:
        return torch.empty((), device=device, dtype=torch.float64)
    return colmajor_empty(rest, device=device)


def tv2_fibres(x, w, dim, out=None, return_mu=False):
    """Batched exact 1-D TV-L2 prox (penalty ``w * ||diff||_2`` per fibre) of every fibre of `x` along 0-based `dim`.  With `return_mu`
    returns (y, mu): mu, the shape of `x` without `dim`, holds every fibre's multiplier -- exactly 0 where the prox is the fibre's mean
    (the dual lies inside the ball), for a dimension of extent 1 and for w <= 0; ``||diff(y)|| / w`` otherwise.  tv2_fibres_vjp needs it:
    the case cannot be read off `y` in floating point."""
    _check(x, "x")
    y = _out(out, x)
    if not 0 <= int(dim) < x.dim():
        raise ValueError(f"dim {dim} out of range for a {x.dim()}-D array")
    dim = int(dim)
    ns = np.array(x.shape, dtype=np.int32)
    mu = _per_fibre_empty(x.shape, dim, x.device) if return_mu else None
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        lib.proxtv_tv2_fibres_dev(x.data_ptr(), y.data_ptr(), mu.data_ptr() if return_mu and mu.numel() else 0, ns.ctypes.data, x.dim(),
                                  dim, float(w), _stream(x.device))
    _lib.check("device.tv2_fibres")
    return (y, mu) if return_mu else y


def tvp_fibres(x, w, p, dim, out=None, return_gap=False):
    """Batched 1-D TV-Lp prox (penalty ``w * ||diff||_p`` per fibre) of every fibre of `x` along 0-based `dim`, for 1.002 < p < 100
    (proxtv_tvpg_fibres_dev; always available, no option needed).  p = 1 and p = 2 return the bits of tv1_fibres / tv2_fibres.  With
    `return_gap` returns (y, gap): gap, the shape of `x` without `dim`, holds every fibre's achieved duality gap (0 where the answer is a
    closed form: a copy, the fibre's mean, p in {1, 2}); the iteration stops at 1e-8."""
    _check(x, "x")
    y = _out(out, x)
    if not 0 <= int(dim) < x.dim():
        raise ValueError(f"dim {dim} out of range for a {x.dim()}-D array")
    dim, p = int(dim), float(p)
    if p not in (1.0, 2.0) and not _lib.P_GENERAL_MIN < p < _lib.P_GENERAL_MAX:
        raise NotImplementedError(f"p: the general-p solver takes {_lib.P_GENERAL_MIN} < p < {_lib.P_GENERAL_MAX}, got {p}")
    ns = np.array(x.shape, dtype=np.int32)
    gap = _per_fibre_empty(x.shape, dim, x.device) if return_gap else None
    with torch.cuda.device(x.device):
        lib = _lib.require_device()
        lib.proxtv_tvpg_fibres_dev(x.data_ptr(), y.data_ptr(), gap.data_ptr() if return_gap and gap.numel() else 0, ns.ctypes.data, x.dim(),
                                   dim, float(w), p, _stream(x.device))
    _lib.check("device.tvp_fibres")
    return (y, gap) if return_gap else y


def tv2_fibres_vjp(y, mu, g, w, dim, need_glam=False, out=None):
    """The derivative of ``y, mu = tv2_fibres(x, w, dim, return_mu=True)`` applied to `g`: returns gx, or (gx, glam) with `need_glam`.

    Per fibre, with M = tridiag(-1, 2 + mu, -1), D the difference matrix and h = D g: where mu > 0, p = M^-1 h, q = M^-1 (D y),
    kappa = h'q / (D y)'q, gx = g - D'(p - kappa q) and glam = -mu w kappa; where mu == 0, gx is the mean of g and glam = 0.  The
    Jacobian is symmetric, so this is the VJP and the JVP in x.  glam holds one value per fibre (the shape of `mu`); for one w shared by
    all fibres d/dw is ``glam.sum()``.  At the kink the prox is not differentiable and the branch the forward took (`mu`) is what comes
    out (include/proxtv_amd.h).  A `g` in another layout is copied; `out` may be `g`."""
    _check(y, "y")
    if not 0 <= int(dim) < y.dim():
        raise ValueError(f"dim {dim} out of range for a {y.dim()}-D array")
    dim = int(dim)
    rest = tuple(s for i, s in enumerate(y.shape) if i != dim)
    if not (isinstance(mu, torch.Tensor) and mu.is_cuda and mu.dtype == torch.float64 and tuple(mu.shape) == rest
            and (mu.dim() == 0 or _is_colmajor(mu))):
        raise ValueError(f"mu: expected a column-major float64 CUDA tensor of shape {rest} (tv2_fibres(..., return_mu=True))")
    if mu.device != y.device:
        raise ValueError(f"mu: lives on {mu.device}, the input on {y.device}")
    if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64):
        raise ValueError("g: expected a float64 CUDA tensor")
    if g.device != y.device:
        raise ValueError(f"g: lives on {g.device}, the input on {y.device}")
    if tuple(g.shape) != tuple(y.shape):
        raise ValueError(f"g: shape {tuple(g.shape)}, expected {tuple(y.shape)}")
    if not _is_colmajor(g):
        g = to_colmajor(g)
    gx = _out(out, y)
    ns = np.array(y.shape, dtype=np.int32)
    glam = _per_fibre_empty(y.shape, dim, y.device) if need_glam else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0   # noqa: E731
    with torch.cuda.device(y.device):
        lib = _lib.require_device()
        lib.proxtv_tv2_fibres_vjp_dev(ptr(y), ptr(mu), ptr(g), ptr(gx), ptr(glam), ns.ctypes.data, y.dim(), dim, float(w),
                                      _stream(y.device))
    _lib.check("device.tv2_fibres_vjp")
    return (gx, glam) if need_glam else gx


def tvp_fibres_vjp(y, g, w, p, dim, need_glam=False, out=None):
    """The derivative of ``y = tvp_fibres(x, w, p, dim)`` for a general p (1.002 < p < 100, p != 2) applied to `g`: returns gx, or
    (gx, glam) with `need_glam`.  It reads the prox's output, w and p only.

    Per fibre, with D the difference matrix, d = D y, N = ||d||_p, s = |d| / N and phi = sign(d) s^(p-1): gx = J g with the symmetric
    J = (I + w D' H D)^-1, H = (p-1)/N (diag s^(p-2) - phi phi') -- two solves with one tridiagonal matrix (n x n for p > 2,
    (n-1) x (n-1) for p < 2) and a rank-one correction -- and glam = -gx'D'phi.  Where y is constant along the fibre (the forward answered
    with the mean) gx is the mean of g and glam = 0; for an extent of 1 and for w <= 0, gx = g.  glam holds one value per fibre (the shape
    of `y` without `dim`); for one w shared by all fibres d/dw is ``glam.sum()``.  The branch the forward took is what is differentiated
    (include/proxtv_amd.h: proxtv_tvpg_fibres_vjp_dev).  p = 1 and p = 2 have their own derivatives, tv1_fibres_vjp and
    tv2_fibres_vjp, which need other inputs.  A `g` in another layout is copied; `out` may be `g`."""
    _check(y, "y")
    if not 0 <= int(dim) < y.dim():
        raise ValueError(f"dim {dim} out of range for a {y.dim()}-D array")
    dim, p = int(dim), float(p)
    if p in (1.0, 2.0):
        raise ValueError(f"p = {p:g} has its own derivative: {'tv1_fibres_vjp' if p == 1.0 else 'tv2_fibres_vjp'}")
    if not _lib.P_GENERAL_MIN < p < _lib.P_GENERAL_MAX:
        raise NotImplementedError(f"p: the general-p derivative takes {_lib.P_GENERAL_MIN} < p < {_lib.P_GENERAL_MAX}, got {p}")
    if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64):
        raise ValueError("g: expected a float64 CUDA tensor")
    if g.device != y.device:
        raise ValueError(f"g: lives on {g.device}, the input on {y.device}")
    if tuple(g.shape) != tuple(y.shape):
        raise ValueError(f"g: shape {tuple(g.shape)}, expected {tuple(y.shape)}")
    if not _is_colmajor(g):
        g = to_colmajor(g)
    gx = _out(out, y)
    ns = np.array(y.shape, dtype=np.int32)
    glam = _per_fibre_empty(y.shape, dim, y.device) if need_glam else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0   # noqa: E731
    with torch.cuda.device(y.device):
        lib = _lib.require_device()
        lib.proxtv_tvpg_fibres_vjp_dev(ptr(y), ptr(g), ptr(gx), ptr(glam), ns.ctypes.data, y.dim(), dim, float(w), p, _stream(y.device))
    _lib.check("device.tvp_fibres_vjp")
    return (gx, glam) if need_glam else gx


def tv1_fibres_dof(y, dim):
    """Segments of every fibre of ``y = tv1_fibres(x, w, dim)`` along `dim` (int32, the shape of `y` without `dim`): the trace of the
    prox's Jacobian, i.e. the degrees of freedom SURE needs.  One pass over `y`; nothing else is computed."""
    _check(y, "y")
    if not 0 <= int(dim) < y.dim():
        raise ValueError(f"dim {dim} out of range for a {y.dim()}-D array")
    ns = np.array(y.shape, dtype=np.int32)
    nseg = _counts_empty(y.shape, int(dim), y.device)
    with torch.cuda.device(y.device):
        lib = _lib.require_device()
        lib.proxtv_tv1_fibres_vjp_dev(y.data_ptr(), 0, 0, 0, nseg.data_ptr() if nseg.numel() else 0, ns.ctypes.data, y.dim(), int(dim),
                                      _stream(y.device))
    _lib.check("device.tv1_fibres_dof")
    return nseg

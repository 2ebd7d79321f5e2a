r"""proxtv_amd -- Total-Variation proximity operators on AMD Instinct MI355X (gfx950).

The module mirrors the Python surface of proxTV (reference: ``prox_tv/__init__.py``) for the TV-L1 solver path:
same function names, argument order, defaults, assertions, dtype / memory-order coercions and return shapes,
so ``import proxtv_amd as prox_tv`` is a drop-in for

    tv1_1d, tv1w_1d, tv1_2d (all seven methods: 'dr', 'pd', 'yang', 'condat', 'chambolle-pock',
    'chambolle-pock-acc', 'kolmogorov'), tv1w_2d, tvp_2d (p = 1), tvgen.

Every call runs hand-written HIP kernels through the C-ABI of ``libproxtv_amd.so`` (``include/proxtv_amd.h``);
there is no CPU path.  Without a gfx950 device the functions raise :class:`ProxTVError`.

New (not in the reference): :func:`tv1_2d_batch` for stacks of independent images, and :mod:`proxtv_amd.device`
for arrays that already live in HBM (torch tensors).

TV-L2 (p = 2) is covered as well: ``tv2_1d``, ``tvp_1d(p=2)``, ``tvp_2d`` and ``tvgen`` with p in {1, 2} -- the fibre prox
is solved EXACTLY on the device (trust-region / More-Sorensen on the tridiagonal dual), which the reference's own p = 2
solver is not (it stops at a duality gap of 1e-5 and warm-starts fibres from each other: its results depend on the
thread count); results agree with the reference within the reference's own guarantee, see DESIGN.md.
General p (1.002 < p < 100, the reference's own range) is opt-in: after ``proxtv_amd.general_p(True)`` (or with PROXTV_GENERAL_P=1 in
the environment) ``tvp_1d`` / ``tvp_2d`` / ``tvgen`` take such a p, and every fibre prox of that norm is solved on the device by nested
Newton iterations on the dual's KKT system to a duality gap of 1e-8 (the reference stops at 1e-5).  While the switch is off
-- the default -- a p outside {1, 2} raises ``NotImplementedError`` as it always has, and nothing else changes.
:func:`proxtv_amd.device.tvp_fibres` is that fibre prox on HBM-resident arrays, always available.  p = inf and p >= 100 are not implemented.
``tv1_1d``'s alternative method names are served by the one exact HIP solver.

Reproducibility: by default the same call returns the same bits whatever ran before -- which kernel geometry a sweep takes is a
function of sampled statistics of its input and of lambda alone (``deterministic = 1``).  Every geometry is
exact, but they round differently in the last ulps, so results may differ by ~1e-13 between calls only with
``proxtv_set_option("deterministic", 0)`` (the hill climb on measured sweep times).
"""
import numpy as np

from . import _lib
from ._lib import ProxTVError  # noqa: F401

__all__ = ["general_p", "general_p_vjp", "tv1_1d", "tv1w_1d", "tv2_1d", "tvp_1d", "tv1_2d", "tv1w_2d", "tvp_2d", "tvgen", "tv1_2d_batch",
           "force_float_scalar", "force_float_matrix", "ProxTVError"]

# The maximum number of returned info parameters (reference: prox_tv/__init__.py:67).
_N_INFO = 3


def _ptr(a):
    return a.ctypes.data


def force_float_scalar(x):
    """Forces a scalar value into float format (reference: prox_tv/__init__.py:80-96)."""
    if not isinstance(x, float):
        return float(x)
    return x


def force_float_matrix(x):
    """Forces a numpy matrix into float64 format; float64 arrays are returned as the SAME object
    (reference: prox_tv/__init__.py:99-121)."""
    if not isinstance(x, np.ndarray):
        try:
            x = np.array(x)
        except Exception:
            raise TypeError("Input must be a numpy matrix or compatible object")
    if x.dtype != np.dtype("float64"):
        return x.astype("float")
    return x


def general_p_vjp(on):
    """Switch the solver derivatives for a general norm on or off: device.dr2_vjp(p_col=, p_row=) / device.tvgen_vjp(ps=) then take any
    1.002 < p < 100 (proxtv_set_option("general_p_vjp", ...); process-wide, off by default; environment: PROXTV_GENERAL_P_VJP=1).
    autograd.tvp_2d / autograd.tvgen(ps=) want general_p(True) as well: their forward is the fused solve.  Returns the previous setting."""
    return bool(_lib.load().proxtv_set_option(b"general_p_vjp", 1 if on else 0))


def general_p(on):
    """Switch the general-p norms (1.002 < p < 100, p != 2) of tvp_1d / tvp_2d / tvgen and of the C entry points behind them on or off
    (proxtv_set_option("general_p", ...); process-wide, off by default).  Returns the previous setting."""
    return bool(_lib.load().proxtv_set_option(b"general_p", 1 if on else 0))


def _contig(x):
    """The reference hands ndarray.ctypes.data to C assuming a dense buffer; make that assumption true."""
    if x.flags.c_contiguous or x.flags.f_contiguous:
        return x
    return np.ascontiguousarray(x)


# ------------------------------------------------------------------------------------------------------------------
# 1-D
# ------------------------------------------------------------------------------------------------------------------
def tv1_1d(x, w, method="hybridtautstring", sigma=0.05, maxbacktracks=None):
    r"""1D proximal operator for :math:`\ell_1`:  min_y 1/2 ||x-y||^2 + w sum_i |y_i - y_{i+1}|.

    Mirrors prox_tv.tv1_1d (reference: prox_tv/__init__.py:124-216).  Every ``method`` name calls the C entry point
    the reference binds for it (PN_TV1, TV1D_denoise, TV1D_denoise_tautstring, SolveTVConvexQuadratic_a1_nw, dp, the
    three taut-string variants); the minimiser is unique, so in libproxtv_amd all of them are entry points of the one
    exact HIP solver.
    """
    methods = ("classictautstring", "linearizedtautstring", "hybridtautstring", "pn", "condat", "dp",
               "condattautstring", "kolmogorov")
    assert method in methods
    assert w >= 0
    w = force_float_scalar(w)
    x = _contig(force_float_matrix(x))
    y = np.zeros(np.size(x))
    lib = _lib.require_device()
    n = int(np.size(x))
    if method == "classictautstring":
        lib.classicTautString_TV1(_ptr(x), n, w, _ptr(y))
    elif method == "linearizedtautstring":
        lib.linearizedTautString_TV1(_ptr(x), w, _ptr(y), n)
    elif method == "condat":
        lib.TV1D_denoise(_ptr(x), _ptr(y), n, w)
    elif method == "pn":                      # prox_tv/__init__.py:197-200
        info = np.zeros(_N_INFO)
        lib.PN_TV1(_ptr(x), w, _ptr(y), _ptr(info), n, float(sigma), None)
    elif method == "condattautstring":        # :206-208
        lib.TV1D_denoise_tautstring(_ptr(x), _ptr(y), n, w)
    elif method == "kolmogorov":              # :210-212
        lib.SolveTVConvexQuadratic_a1_nw(n, _ptr(x), w, _ptr(y))
    elif method == "dp":                      # :214-216
        lib.dp(n, _ptr(x), w, _ptr(y))
    elif maxbacktracks is not None:
        lib.hybridTautString_TV1_custom(_ptr(x), n, w, _ptr(y), float(maxbacktracks))
    else:
        lib.hybridTautString_TV1(_ptr(x), n, w, _ptr(y))
    _lib.check("tv1_1d")
    return y


def tv1w_1d(x, w, method="tautstring", sigma=0.05):
    r"""Weighted 1D proximal operator for :math:`\ell_1` (reference: prox_tv/__init__.py:218-254).
    'tautstring' calls tautString_TV1_Weighted, 'pn' PN_TV1_Weighted; both are the exact weighted HIP solver."""
    assert np.all(w >= 0)
    assert np.size(x) - 1 == np.size(w)
    w = _contig(force_float_matrix(w))
    x = _contig(force_float_matrix(x))
    y = np.zeros(np.size(x))
    lib = _lib.require_device()
    if method == "tautstring":
        lib.tautString_TV1_Weighted(_ptr(x), _ptr(w), _ptr(y), int(np.size(x)))
    else:
        info = np.zeros(_N_INFO)
        lib.PN_TV1_Weighted(_ptr(x), _ptr(w), _ptr(y), _ptr(info), int(np.size(x)), float(sigma), None)
    _lib.check("tv1w_1d")
    return y


def tv2_1d(x, w, method="mspg"):
    r"""1D proximal operator for :math:`\ell_2`: min_y 1/2 ||x-y||^2 + w ||Dy||_2 (reference: prox_tv/__init__.py:257-310).
    The three method names ('ms', 'pg', 'mspg') call the reference's three C entry points; all are served by the
    one exact device solver."""
    assert w >= 0
    assert method in ("ms", "pg", "mspg")
    w = force_float_scalar(w)
    x = _contig(force_float_matrix(x))
    info = np.zeros(_N_INFO)
    y = np.zeros(np.size(x), order="F")
    lib = _lib.require_device()
    n = int(np.size(x))
    if method == "ms":
        lib.more_TV2(_ptr(x), w, _ptr(y), _ptr(info), n)
    elif method == "pg":
        lib.PG_TV2(_ptr(x), w, _ptr(y), _ptr(info), n)
    else:
        lib.morePG_TV2(_ptr(x), w, _ptr(y), _ptr(info), n, None)
    _lib.check("tv2_1d")
    return y


def tvp_1d(x, w, p, method="gpfw", max_iters=0):
    """1D proximal operator for the l_p norm (reference: prox_tv/__init__.py:311-352): p = 1 and p = 2 are the exact TV-L1 / TV-L2
    device solvers, whatever `method`; with general_p(True) any 1.002 < p < 100 is the one general-p device solver (all three
    methods), stopped at a duality gap of 1e-8."""
    assert method in ("gp", "fw", "gpfw")
    assert w >= 0
    assert p >= 1
    _lib.check_forward_norms((p,))
    w = force_float_scalar(w)
    x = _contig(force_float_matrix(x))
    info = np.zeros(_N_INFO)
    y = np.zeros(np.size(x), order="F")
    lib = _lib.require_device()
    entry = {"gp": lib.GP_TVp, "fw": lib.FW_TVp, "gpfw": lib.GPFW_TVp}[method]   # prox_tv/__init__.py:343-351
    entry(_ptr(x), w, _ptr(y), _ptr(info), int(np.size(x)), float(p), None)
    _lib.check("tvp_1d")
    return y


# ------------------------------------------------------------------------------------------------------------------
# 2-D
# ------------------------------------------------------------------------------------------------------------------
def tv1_2d(x, w, n_threads=1, max_iters=0, method="dr"):
    r"""2D proximal operator for :math:`\ell_1` (anisotropic TV), reference: prox_tv/__init__.py:355-407.

    ``method``: 'dr' (Douglas-Rachford, DR2_TV), 'pd' (proximal Dykstra, PD2_TV), 'yang' (Yang2_TV), 'kolmogorov'
    (Kolmogorov2_TV), 'condat' / 'chambolle-pock' / 'chambolle-pock-acc' (CondatChambollePock2_TV, algorithm 0 / 1 / 2).
    ``n_threads`` is accepted for compatibility; the GPU path ignores it.
    """
    methods = ("yang", "dr", "pd", "kolmogorov", "condat", "chambolle-pock", "chambolle-pock-acc")
    assert w >= 0
    assert method in methods
    x = np.asfortranarray(x, dtype="float64")
    w = force_float_scalar(w)
    y = np.asfortranarray(np.zeros(x.shape))
    info = np.zeros(_N_INFO)
    lib = _lib.require_device()
    if method == "dr":      # prox_tv/__init__.py:413-416
        lib.DR2_TV(x.shape[0], x.shape[1], _ptr(x), w, w, 1.0, 1.0, _ptr(y), int(n_threads), int(max_iters), _ptr(info))
    elif method == "pd":    # prox_tv/__init__.py:418-421
        lam = np.array([w, w], dtype=np.float64)
        norms = np.array([1.0, 1.0])
        dims = np.array([1.0, 2.0])
        ns = np.array(x.shape, dtype=np.int32)
        lib.PD2_TV(_ptr(x), _ptr(lam), _ptr(norms), _ptr(dims), _ptr(y), _ptr(info), _ptr(ns), 2, 2,
                   int(n_threads), int(max_iters))
    elif method == "yang":  # prox_tv/__init__.py:409-411
        lib.Yang2_TV(x.shape[0], x.shape[1], _ptr(x), w, _ptr(y), int(max_iters), _ptr(info))
    elif method == "kolmogorov":   # prox_tv/__init__.py:423-426
        lib.Kolmogorov2_TV(x.shape[0], x.shape[1], _ptr(x), w, _ptr(y), int(max_iters), _ptr(info))
    else:                   # prox_tv/__init__.py:428-443
        alg = {"condat": 0, "chambolle-pock": 1, "chambolle-pock-acc": 2}[method]
        lib.CondatChambollePock2_TV(x.shape[0], x.shape[1], _ptr(x), w, _ptr(y), alg, int(max_iters), _ptr(info))
    _lib.check("tv1_2d")
    return y


def tv1w_2d(x, w_col, w_row, max_iters=0, n_threads=1):
    r"""2D weighted proximal operator for :math:`\ell_1` using DR splitting (reference: prox_tv/__init__.py:445-481).
    ``w_col`` is (M-1) x N, ``w_row`` is M x (N-1)."""
    assert np.all(w_col >= 0)
    assert np.all(w_row >= 0)
    M, N = x.shape
    assert w_col.shape == (M - 1, N)
    assert w_row.shape == (M, N - 1)
    x = np.asfortranarray(x, dtype="float64")
    y = np.zeros(x.shape, order="F")
    w_col = np.asfortranarray(w_col, dtype="float64")
    w_row = np.asfortranarray(w_row, dtype="float64")
    info = np.zeros(_N_INFO)
    lib = _lib.require_device()
    lib.DR2L1W_TV(M, N, _ptr(x), _ptr(w_col), _ptr(w_row), _ptr(y), int(n_threads), int(max_iters), _ptr(info))
    _lib.check("tv1w_2d")
    return y


def tvp_2d(x, w_col, w_row, p_col, p_row, n_threads=1, max_iters=0):
    r"""2D proximal operator for :math:`\ell_p` norms (reference: prox_tv/__init__.py:484-530): DR2_TV with separate
    column / row penalties and norms; p in {1, 2}, and with general_p(True) any 1.002 < p < 100."""
    assert w_col >= 0
    assert w_row >= 0
    assert p_col >= 1
    assert p_row >= 1
    _lib.check_forward_norms((p_col, p_row))
    info = np.zeros(_N_INFO)
    x = np.asfortranarray(x, dtype="float64")
    w_col = force_float_scalar(w_col)
    w_row = force_float_scalar(w_row)
    y = np.zeros(np.shape(x), order="F")
    lib = _lib.require_device()
    lib.DR2_TV(x.shape[0], x.shape[1], _ptr(x), w_col, w_row, float(p_col), float(p_row), _ptr(y), int(n_threads),
               int(max_iters), _ptr(info))
    _lib.check("tvp_2d")
    return y


# ------------------------------------------------------------------------------------------------------------------
# N-D
# ------------------------------------------------------------------------------------------------------------------
def tvgen(x, ws, ds, ps, n_threads=1, max_iters=0):
    r"""General TV proximal operator for multidimensional signals (reference: prox_tv/__init__.py:533-600).

    Observable dispatch of the reference, reproduced: two penalty terms -> PD2_TV (proximal Dykstra); any other
    count -> PD_TV (parallel proximal Dykstra).  (The reference's "2-D => Douglas-Rachford" branch at
    prox_tv/__init__.py:585 can never be taken because of operator precedence, so it is not mirrored.)
    Like the reference, a float64 ndarray ``ws`` is passed to PD_TV by reference and comes back multiplied by the
    number of penalties (src/TVNDopt.cpp:100-101).
    """
    assert len(ws) == len(ds)
    assert len(ws) == len(ps)
    assert n_threads >= 1
    assert max_iters >= 0
    info = np.zeros(_N_INFO)
    x = np.asfortranarray(x, dtype="float64")
    ws = force_float_matrix(ws)
    ps = force_float_matrix(ps)
    y = np.zeros(np.shape(x), order="F")
    _lib.check_forward_norms(ps.ravel())      # (p in {1, 2}; with general_p(True) any 1.002 < p < 100)
    if not (ps.flags.c_contiguous or ps.flags.f_contiguous):
        ps = np.ascontiguousarray(ps)
    dims = np.array(ds, dtype=np.float64)            # cffi turns the `ds` sequence into a temporary double[]
    ns = np.array(x.shape, dtype=np.int32)           # ... and x.shape into a temporary int[]
    if not (ws.flags.c_contiguous or ws.flags.f_contiguous):
        ws = np.ascontiguousarray(ws)
    lib = _lib.require_device()
    if len(ws) == 2:
        lib.PD2_TV(_ptr(x), _ptr(ws), _ptr(ps), _ptr(dims), _ptr(y), _ptr(info), _ptr(ns), len(x.shape), 2,
                   int(n_threads), int(max_iters))
    else:
        lib.PD_TV(_ptr(x), _ptr(ws), _ptr(ps), _ptr(dims), _ptr(y), _ptr(info), _ptr(ns), len(x.shape), len(ws),
                  int(n_threads), int(max_iters))
    _lib.check("tvgen")
    return y


# ------------------------------------------------------------------------------------------------------------------
# new API: batches of independent images
# ------------------------------------------------------------------------------------------------------------------
def tv1_2d_batch(xs, w, max_iters=0):
    r"""Anisotropic TV-L1 prox (Douglas-Rachford, DR2_TV semantics) of a stack of independent images.

    ``xs`` has shape (B, M, N); the result has the same shape and equals ``tv1_2d(xs[b], w)`` for every b.
    All B images advance together: one kernel launch per sweep over all B*N column (B*M row) fibres.
    """
    assert w >= 0
    xs = np.asarray(xs, dtype=np.float64)
    assert xs.ndim == 3
    B, M, N = xs.shape
    # image b column-major, images back to back == a Fortran-ordered (M, N, B) array
    stack = np.asfortranarray(np.transpose(xs, (1, 2, 0)))
    out = np.zeros_like(stack, order="F")
    info = np.zeros(_N_INFO)
    lib = _lib.require_device()
    lib.proxtv_DR2_TV_batch(M, N, B, _ptr(stack), float(w), float(w), _ptr(out), int(max_iters), _ptr(info))
    _lib.check("tv1_2d_batch")
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1)))

"""The reference's GMRES options as the C ABI's ``rt_gmres_opts``.

``RomConstructor.GMRES_OPTIONS`` (rom.py:36) is what the reference hands to ``scipy.sparse.linalg.gmres`` for every
reduced system (rom.py:414-425,492).  The device solver (``ops.gmres_solve``, the sweeps' GMRES mode) takes the same
dictionary; this module is the one place that reads it."""
from __future__ import annotations

import math
import numbers

from ._lib import GmresOpts

_KEYS = ("tol", "rtol", "atol", "restart", "maxiter")
_UNSUPPORTED = ("x0", "M", "callback", "callback_type")


def _real(value, name):
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or value < 0:
        raise ValueError(f"gmres option {name}={value!r}: a finite number >= 0 is required")
    return float(value)


def _count(value, name):
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) \
            or value != int(value) or value < 1:
        raise ValueError(f"gmres option {name}={value!r}: an integer >= 1 (or an integral float such as 1e6) is required")
    return int(value)


def gmres_opts(options, r: int) -> GmresOpts:
    """``scipy.sparse.linalg.gmres`` keyword arguments (a dict, or None for SciPy's defaults) for r x r systems ->
    ``rt_gmres_opts``.

    ``tol`` (the spelling of rom.py:36, SciPy < 1.14) or ``rtol``, default 1e-5; both given with different values is an
    error.  ``atol`` defaults to 0, ``restart`` to 20 and is clamped to r, ``maxiter`` (outer cycles: an int or an
    integral float such as 1e6) to 10 r, as in SciPy.  ``x0``, ``M``, ``callback``, ``callback_type`` and unknown keys
    raise ``ValueError``: the device solver starts from zero without a preconditioner, and no key is ignored."""
    opts = dict(options or {})
    for key in opts:
        if key in _UNSUPPORTED:
            raise ValueError(f"gmres option {key!r} is not supported (the device GMRES starts from x0 = 0 without a "
                             "preconditioner or callback)")
        if key not in _KEYS:
            raise ValueError(f"unknown gmres option {key!r}")
    if "tol" in opts and "rtol" in opts and _real(opts["tol"], "tol") != _real(opts["rtol"], "rtol"):
        raise ValueError(f"gmres options tol={opts['tol']!r} and rtol={opts['rtol']!r} disagree")
    r = _count(r, "r")
    rtol = _real(opts.get("rtol", opts.get("tol", 1e-5)), "rtol")
    atol = _real(opts.get("atol", 0.0), "atol")
    restart = opts.get("restart")
    restart = 20 if restart is None else _count(restart, "restart")
    maxiter = opts.get("maxiter")
    maxiter = 10 * r if maxiter is None else _count(maxiter, "maxiter")
    return GmresOpts(rtol=rtol, atol=atol, restart=min(restart, r), maxiter=maxiter)

"""The tolerance rule shared by the fp64 edge tests (test_optim_gpu.py,
test_latent_gpu.py, test_mdn_edges_gpu.py).

Every compared quantity is computed three times on the same inputs: ``q64``
(an fp64 reference), ``q32`` (a plain fp32 PyTorch transcription of the same
formula -- not the code under test) and ``qk`` (the kernel). The kernel passes
when

    max|qk - q64| <= margin * max|q32 - q64| + 4 * 2^-24 * max|q64|

with ``margin = 4``: a different summation order and libm-versus-hardware
``exp`` each move fp32 rounding noise by a small factor, a wrong term moves
it by thousands. No tolerance here comes from what a kernel was seen to give.
Gradients go through :func:`check` one column group / one parameter tensor at
a time, each against its own ``max|q64|``.

:data:`RATIOS` keeps, per quantity name, the largest ``err_k / err_32`` seen
(and the largest share of the bound used), which the test modules print when
they finish.
"""
import math

import torch

EPS32 = 2.0 ** -24
RATIOS = {}


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def record(name, ratio, used):
    r0, u0 = RATIOS.get(name, (0.0, 0.0))
    # a NaN must not vanish in max()
    RATIOS[name] = (ratio if not ratio <= r0 else r0, used if not used <= u0 else u0)


def errors(qk, q32, q64):
    q64 = q64.detach().double()
    return (_maxabs(qk.detach().double() - q64), _maxabs(q32.detach().double() - q64), _maxabs(q64))


def check(name, qk, q32, q64, margin=4.0, extra=0.0):
    """Assert the rule for one quantity; ``extra`` is an additional absolute
    term a caller can justify (e.g. a bf16 store). Returns ``err_k / err_32``."""
    assert tuple(qk.shape) == tuple(q64.shape) == tuple(q32.shape), (name, qk.shape, q32.shape, q64.shape)
    ek, e32, top = errors(qk, q32, q64)
    bound = margin * e32 + 4.0 * EPS32 * top + extra
    ratio = ek / e32 if e32 > 0.0 else (0.0 if ek == 0.0 else math.inf)
    used = ek / bound if bound > 0.0 else (0.0 if ek == 0.0 else math.inf)
    record(name, ratio, used)
    assert ek <= bound, "%s: err_k %.3e > %g * err_32 %.3e + 4 * 2^-24 * %.3e (err_k / err_32 = %.2f)" % (
        name, ek, margin, e32, top, ratio)
    return ratio


def report(title):
    print("\n%s: largest err_k / err_32 (share of the bound used) per quantity" % title)
    for k in sorted(RATIOS):
        print("  %-28s %8.3f  (%.3f)" % (k, RATIOS[k][0], RATIOS[k][1]))
    RATIOS.clear()

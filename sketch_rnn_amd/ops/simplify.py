"""Ramer-Douglas-Peucker (RDP) simplification of stroke batches
(``csrc/simplify.hip``): each point's tolerance, the batch simplified at an
epsilon, and the batch fitted to a length.

One definition serves :func:`rdp_tolerance_reference` and
:func:`simplify_reference` (the oracles), the kernel and the tests.

**Input.** ``strokes [B, N, D]`` is floating point. ``D = 3`` is stroke-3
``(dx, dy, lift)``. ``D = 5`` is magenta stroke-5 without the start token,
lift in column 3, column 4 ignored. ``lengths [B]`` are integers; for
``D = 5``, ``None`` means ``ops.raster.stroke5_lengths``. With ``L =
clamp(lengths[b], 0, N)``, rows ``t >= L`` take part in nothing and may hold
NaN (a select before any arithmetic, as in ``ops.raster``).

**Points.** ``P_t = sum_{s <= t} (dx_s, dy_s)`` in fp64, for ``t < L``.

**Runs.** A run is a maximal range ``[s, e]`` of consecutive points. It ends at
the first ``t >= s`` with ``lift[t] >= 0.5`` or ``t = L - 1``, and the next
run starts at ``e + 1``. ``lift < 0.5`` means pen down, as in the rasteriser.

**Tolerance** ``tol [B, N]``, fp64: the largest epsilon at which RDP still
keeps the point.

* ``tol = +inf`` at both ends of every run; a one-point run is its own end.
* ``tol = -inf`` for ``t >= L``.
* For a segment ``(l, r)`` with ``r - l >= 2`` and cap ``c``, where a run
  starts as ``(s, e)`` with ``c = +inf``: let ``u = P_r - P_l`` and ``v_t =
  P_t - P_l`` for ``l < t < r``. If ``|u|^2 > 0`` the key is ``k_t = |u_x v_ty
  - u_y v_tx|`` and the distance ``d = k / sqrt(|u|^2)``, the distance to the
  infinite line. Otherwise ``k_t = v_tx^2 + v_ty^2`` and ``d = sqrt(k)``. The
  split point ``m`` is the **lowest** ``t`` with the largest key (keys are
  compared, not distances). ``tol[m] = min(c, d_m)``, and both ``(l, m)`` and
  ``(m, r)`` recurse with cap ``tol[m]``.
* Every arithmetic step is a single fp64 operation: contraction is off in the
  kernel file and there is no fused multiply-add here.

Classical RDP at ``eps`` keeps the run ends and exactly ``{t : tol[t] >
eps}`` besides: the recursion enters a segment only if every ancestor's
distance exceeded ``eps``.

**Fit.** ``fit[b]`` is the smallest ``e`` in ``{0} + {finite tol[b, :]}`` with
``#{t : tol[b, t] > e} <= max_len``, and ``+inf`` if the ``+inf`` points alone
exceed ``max_len``: that sketch cannot fit, and its new length then exceeds
``max_len``, which is how the caller sees it.

**Output at** ``eps_used[b]``: ``epsilon[b]`` without ``max_len``, else
``max(epsilon[b], fit[b])``. The kept points ``k_0 < k_1 < ...`` are those with
``tol > eps_used`` and, at every ``eps_used`` (``+inf`` too), the run ends.
``out[b, i, 0:2] = fp32(P_{k_i} - P_{k_{i-1}})``, the difference taken in fp64
with ``P_{k_{-1}}`` the origin; the pen columns are copied from row ``k_i``.
``new_lengths[b]`` is the number of kept points; rows ``i >= new_lengths[b]``
are zeros for ``D = 3`` and ``(0, 0, 0, 0, 1)`` for ``D = 5``. ``out`` is ``[B,
N, D]`` float32: the call allocates by shape and never synchronises, and the
caller trims.

On integer-valued input (sums and cross products below 2^53) every step is
exact or correctly rounded on both sides, so the kernel and the references
agree bit for bit; on general floats the kernel's scan order differs from
``cumsum`` in the last bits of the points.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np
import torch

from ..utils import native
from .raster import stroke5_lengths

MAX_N = 2048


def _check(strokes, lengths, epsilon=0.0, max_len=None):
    """Validate the arguments; returns ``(lengths [B] int64 on the strokes'
    device, clamped to [0, N]; epsilon [B] float64 on it)``."""
    if not isinstance(strokes, torch.Tensor) or strokes.dim() != 3 or strokes.shape[-1] not in (3, 5):
        raise ValueError("strokes must be [B, N, 3] or [B, N, 5]")
    if not strokes.is_floating_point():
        raise ValueError("strokes must be a floating-point tensor")
    B, N, D = strokes.shape
    if lengths is None:
        if D != 5:
            raise ValueError("stroke-3 input needs lengths")
        lengths = stroke5_lengths(strokes)
    else:
        lengths = torch.as_tensor(lengths)
        if lengths.shape != (B,) or lengths.is_floating_point() or lengths.dtype == torch.bool:
            raise ValueError("lengths must be [B] integers")
        lengths = lengths.to(device=strokes.device, dtype=torch.int64)
    if max_len is not None and (isinstance(max_len, bool) or not isinstance(max_len, int) or max_len < 1):
        raise ValueError("max_len must be None or an integer >= 1, got %r" % (max_len,))
    if isinstance(epsilon, torch.Tensor):
        if epsilon.shape != (B,) or not epsilon.is_floating_point():
            raise ValueError("epsilon must be a float or a [B] floating-point tensor")
        # reading the values back is a synchronisation: not inside a graph capture
        capturing = epsilon.is_cuda and torch.cuda.is_current_stream_capturing()
        if not capturing and B and not bool((torch.isfinite(epsilon) & (epsilon >= 0)).all()):
            raise ValueError("epsilon must be finite and >= 0")
        eps = epsilon.detach().to(device=strokes.device, dtype=torch.float64)
    else:
        if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float)) or not (
                math.isfinite(epsilon) and epsilon >= 0):
            raise ValueError("epsilon must be finite and >= 0, got %r" % (epsilon,))
        eps = torch.full((B,), float(epsilon), dtype=torch.float64, device=strokes.device)
    return lengths.clamp(0, N), eps


def _host(strokes, L):
    """fp64 rows and lengths on the host."""
    return strokes.detach().cpu().to(torch.float64).numpy(), [int(v) for v in L.cpu().tolist()]


def _points_and_runs(rows, n, D):
    """``(P [n, 2] fp64, [(s, e), ...])`` of the first ``n`` rows of one sketch."""
    xy = rows[:n, 0:2].astype(np.float64)
    P = np.cumsum(xy, axis=0)                     # sequential, fp64
    ends = rows[:n, 3 if D == 5 else 2] >= 0.5
    if n:
        ends[n - 1] = True
    runs, s = [], 0
    for e in np.nonzero(ends)[0].tolist():
        runs.append((s, e))
        s = e + 1
    return P, runs


def _split(P, l, r):
    """``(m, d)``: the split point of segment ``(l, r)`` and its distance."""
    ux, uy = P[r, 0] - P[l, 0], P[r, 1] - P[l, 1]
    vx, vy = P[l + 1:r, 0] - P[l, 0], P[l + 1:r, 1] - P[l, 1]
    uu = ux * ux + uy * uy
    if uu > 0:
        k = np.abs(ux * vy - uy * vx)
        j = int(np.argmax(k))                     # the first of equal keys
        return l + 1 + j, float(k[j] / np.sqrt(uu))
    k = vx * vx + vy * vy
    j = int(np.argmax(k))
    return l + 1 + j, float(np.sqrt(k[j]))


def _tolerance_one(P, runs, N):
    tol = np.full(N, -np.inf)
    for s, e in runs:
        tol[s] = tol[e] = np.inf
        stack = [(s, e, np.inf)]
        while stack:
            l, r, c = stack.pop()
            if r - l < 2:
                continue
            m, d = _split(P, l, r)
            tol[m] = min(c, d)
            stack.append((l, m, tol[m]))
            stack.append((m, r, tol[m]))
    return tol


def rdp_tolerance_reference(strokes, lengths=None) -> torch.Tensor:
    """The definition on the host: NumPy fp64, one sketch at a time, an explicit
    stack. Returns ``tol [B, N]`` float64 on the CPU."""
    L, _ = _check(strokes, lengths)
    B, N, D = strokes.shape
    x, n = _host(strokes, L)
    tol = np.full((B, N), -np.inf)
    for b in range(B):
        P, runs = _points_and_runs(x[b], n[b], D)
        tol[b] = _tolerance_one(P, runs, N)
    return torch.from_numpy(tol)


def _fit_one(tol, n, max_len):
    """The smallest ``e`` in ``{0} + {finite tol}`` with ``#{tol > e} <= max_len``."""
    t = tol[:n]
    if int((t == np.inf).sum()) > max_len:
        return np.inf
    for e in [0.0] + sorted(set(t[np.isfinite(t)].tolist())):
        if int((t > e).sum()) <= max_len:
            return e
    raise AssertionError("unreachable: the largest finite tolerance leaves only the run ends")


def simplify_reference(strokes, lengths=None, epsilon=2.0, max_len: Optional[int] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Classical RDP on the host at the epsilon it ends up using: keep the ends
    of every run, split a segment while its largest distance exceeds epsilon.
    Deliberately not a threshold on the tolerances, which only supply the fit.
    Returns ``(out [B, N, D] float32, new_lengths [B] int64, eps_used [B]
    float64)`` on the CPU."""
    L, eps = _check(strokes, lengths, epsilon, max_len)
    B, N, D = strokes.shape
    x, n = _host(strokes, L)
    eps = eps.cpu().numpy().copy()
    out = np.zeros((B, N, D), np.float32)
    if D == 5:
        out[..., 4] = 1.0
    new_len = np.zeros(B, np.int64)
    for b in range(B):
        P, runs = _points_and_runs(x[b], n[b], D)
        if max_len is not None:
            eps[b] = max(eps[b], _fit_one(_tolerance_one(P, runs, N), n[b], max_len))
        keep = np.zeros(n[b], bool)
        for s, e in runs:
            keep[s] = keep[e] = True
            stack = [(s, e)]
            while stack:
                l, r = stack.pop()
                if r - l < 2:
                    continue
                m, d = _split(P, l, r)
                if d > eps[b]:
                    keep[m] = True
                    stack.append((l, m))
                    stack.append((m, r))
        k = np.nonzero(keep)[0]
        Q = P[k]
        out[b, :len(k), 0:2] = (Q - np.concatenate([np.zeros((1, 2)), Q[:-1]], axis=0)).astype(np.float32)
        out[b, :len(k), 2:] = x[b][k, 2:]
        new_len[b] = len(k)
    return torch.from_numpy(out), torch.from_numpy(new_len), torch.from_numpy(eps)


def _launch(strokes, L, eps, max_len, want_tol, want_out, rounds=None):
    from ._hipapi import RdpArgs
    lib = native.require_hip()
    B, N, D = strokes.shape
    dev = strokes.device
    x = strokes.detach().contiguous().float()
    L = L.contiguous()
    tol = torch.empty(B, N, device=dev, dtype=torch.float64) if want_tol else None
    out = new_len = eps_used = None
    if want_out:
        out = torch.empty(B, N, D, device=dev, dtype=torch.float32)
        new_len = torch.empty(B, device=dev, dtype=torch.int64)
        eps_used = torch.empty(B, device=dev, dtype=torch.float64)
        eps = eps.contiguous()
    if B == 0 or N == 0:        # nothing to launch: no points, the epsilon as given
        if want_out:
            new_len.zero_()
            eps_used.copy_(eps)
        if rounds is not None:
            rounds.zero_()
        return tol, out, new_len, eps_used
    a = RdpArgs()
    a.strokes, a.lengths = x.data_ptr(), L.data_ptr()
    a.epsilon = eps.data_ptr() if want_out else None
    a.tol = tol.data_ptr() if want_tol else None
    a.out = out.data_ptr() if want_out else None
    a.new_lengths = new_len.data_ptr() if want_out else None
    a.eps_used = eps_used.data_ptr() if want_out else None
    a.rounds = rounds.data_ptr() if rounds is not None else None
    a.B, a.N, a.D, a.max_len = B, N, D, int(max_len or 0)
    with torch.cuda.device(dev):
        rc = lib.lib.skr_rdp(C.byref(a), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("skr_rdp failed (%d)" % rc)
    return tol, out, new_len, eps_used


def _check_hip(strokes, rounds=None):
    if not (isinstance(strokes, torch.Tensor) and strokes.is_cuda and strokes.dtype == torch.float32):
        raise ValueError("the kernel path takes CUDA float32 strokes")
    if strokes.dim() == 3 and strokes.shape[1] > MAX_N:
        raise ValueError("the kernel path takes N <= %d, got %d" % (MAX_N, strokes.shape[1]))
    if rounds is not None and not (isinstance(rounds, torch.Tensor) and rounds.dtype == torch.int32
                                   and rounds.device == strokes.device and rounds.is_contiguous()
                                   and strokes.dim() == 3 and rounds.shape == (strokes.shape[0],)):
        raise ValueError("rounds must be a contiguous [B] int32 tensor on the strokes' device")


def rdp_tolerance_hip(strokes, lengths=None, rounds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The kernel path: ``tol [B, N]`` float64 of CUDA float32 strokes with
    ``N <= MAX_N``. ``rounds [B]`` int32, if given, receives the levels of each
    sketch's recursion."""
    _check_hip(strokes, rounds)
    L, _ = _check(strokes, lengths)
    return _launch(strokes, L, None, None, True, False, rounds)[0]


def simplify_hip(strokes, lengths=None, epsilon=2.0, max_len: Optional[int] = None,
                 rounds: Optional[torch.Tensor] = None):
    """The kernel path: ``(out, new_lengths, eps_used)`` of CUDA float32
    strokes with ``N <= MAX_N``. Allocates by shape only and never
    synchronises (an ``epsilon`` tensor is validated by value outside a graph
    capture only), so the call can be captured in a HIP graph."""
    _check_hip(strokes, rounds)
    L, eps = _check(strokes, lengths, epsilon, max_len)
    return _launch(strokes, L, eps, max_len, False, True, rounds)[1:]


def _kernel_serves(strokes) -> bool:
    from . import use_hip
    return (isinstance(strokes, torch.Tensor) and strokes.is_cuda and strokes.dtype == torch.float32
            and strokes.dim() == 3 and strokes.shape[1] <= MAX_N and use_hip(strokes))


def rdp_tolerance(strokes, lengths=None) -> torch.Tensor:
    """``tol [B, N]`` float64 on the strokes' device: the kernel for CUDA
    float32 strokes with ``N <= MAX_N`` when the HIP backend is on, the host
    reference otherwise."""
    if _kernel_serves(strokes):
        return rdp_tolerance_hip(strokes, lengths)
    tol = rdp_tolerance_reference(strokes, lengths)
    return tol.to(strokes.device)


def simplify(strokes, lengths=None, epsilon=2.0, max_len: Optional[int] = None
             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(out [B, N, D] float32, new_lengths [B] int64, eps_used [B] float64)``
    on the strokes' device; dispatches like :func:`rdp_tolerance`."""
    if _kernel_serves(strokes):
        return simplify_hip(strokes, lengths, epsilon, max_len)
    out, new_len, eps_used = simplify_reference(strokes, lengths, epsilon, max_len)
    dev = strokes.device
    return out.to(dev), new_len.to(dev), eps_used.to(dev)

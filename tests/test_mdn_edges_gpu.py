"""One hard input table through the three hand-written copies of the MDN
loss math -- csrc/mdn.hip (``ops.mdn_loss``), the epilogue of
csrc/mdn_head.hip (``ops.mdn_head_loss``) and csrc/mdn_score.hip
(``ops.mdn_head_score``) -- against ``models.mdn`` in fp64, under the rule of
tests/fp64_rule.py with ``models.mdn`` in fp32 on the GPU as ``q32``.
Gradients are compared per column group (pen, pi, mu1, mu2, s1, s2, rho),
each against its own ``max|dz64|``.

The table (``_table``): pen logits x 10 and pi logits x 6 (peaky weights),
log-sigmas ``1.5 randn - 2`` (tiny sigmas), rho_hat x 4/3 clamped to +-5
(|rho| up to 0.99991; fp32 ``tanhf`` reaches exactly 1 from about 9, where
every implementation returns NaN by design -- not tested), targets
``3 randn`` with the first 8 rows at (50, 50): far targets, on both sides of
the reference mode's ``log(1e-20)`` clamp. ``z`` is rounded to bf16 once and
that same ``z`` is used everywhere, so the two fused kernels -- fed through
an identity projection -- see the table bit for bit.
"""
import functools
import math

import pytest
import torch

import fp64_rule as R
from sketch_rnn_amd import ops
from sketch_rnn_amd.models import mdn
from sketch_rnn_amd.ops import mdn_hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = 256
LOG_CLAMP = math.log(1e-20)
GROUPS = ("pen", "pi", "mu1", "mu2", "s1", "s2", "rho")


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_backend("auto")
    ops.set_compute_dtype("fp32")
    mdn_hip.FUSED_HEAD = True


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    R.report("MDN edges (csrc/mdn.hip, mdn_head.hip, mdn_score.hip)")


def _groups(M):
    return [slice(0, 3)] + [slice(3 + k * M, 3 + (k + 1) * M) for k in range(6)]


def _draw(N, M, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, 3 + 6 * M, generator=g, dtype=torch.float64)
    z[:, 0:3] *= 10.0
    z[:, 3:3 + M] *= 6.0
    z[:, 3 + 3 * M:3 + 5 * M] = 1.5 * torch.randn(N, 2 * M, generator=g, dtype=torch.float64) - 2.0
    z[:, 3 + 5 * M:] = (z[:, 3 + 5 * M:] * (4.0 / 3.0)).clamp(-5.0, 5.0)
    z = z.bfloat16().double()
    t = torch.zeros(N, 5)
    t[:, :2] = 3.0 * torch.randn(N, 2, generator=g)
    t[:8, :2] = 50.0
    t[torch.arange(N), 2 + (torch.arange(N) + 1) % 3] = 1.0   # one-hot pen, every state present from N = 3
    return z, t


def _clear_of_clamp(log_s):
    """No row within 0.05 of the reference clamp: there fp32 (|rho| near 1
    costs 1 - rho^2 three digits) could take the other branch than fp64."""
    return bool(((log_s - LOG_CLAMP).abs() > 0.05).all())


@functools.lru_cache(maxsize=None)
def _table(N, M):
    """``(z [N, 3 + 6M] fp64 with bf16-exact values, target [N, 5] fp32)`` on
    the GPU: the first draw (of seeds 1000 N + M, + 100003, ...) in which no
    row sits on the clamp -- a property of the fp64 inputs alone."""
    for attempt in range(16):
        z, t = _draw(N, M, 1000 * N + M + 100003 * attempt)
        if _clear_of_clamp(mdn.log_mixture_density(z, t[:, 0].double(), t[:, 1].double(), M)):
            return z.to(DEV), t.to(DEV)
    raise AssertionError("no table clear of the clamp")


def _oracle(N, M, mode, is_training, coef, dtype):
    """``mdn_loss_torch`` and ``d(coef . (total, shape, pen)) / dz`` in ``dtype`` on the GPU."""
    z, t = _table(N, M)
    zz = z.to(dtype).clone().requires_grad_()
    tot, shape, pen = mdn.mdn_loss_torch(zz, t.to(dtype), M, mode=mode, stroke_importance=200.0,
                                         is_training=is_training)
    (coef[0] * tot + coef[1] * shape + coef[2] * pen).backward()
    return tot.detach(), shape.detach(), pen.detach(), zz.grad


@functools.lru_cache(maxsize=None)
def _refs(N, M, mode, is_training, coef=(1.0, 0.0, 0.0)):
    o64 = _oracle(N, M, mode, is_training, coef, torch.float64)
    o32 = _oracle(N, M, mode, is_training, coef, torch.float32)
    assert all(bool(torch.isfinite(v).all()) for v in o64), "the fp64 oracle must be finite on the table"
    return o64, o32


@functools.lru_cache(maxsize=None)
def _log_s(N, M):
    z, t = _table(N, M)
    t = t.double()
    return mdn.log_mixture_density(z, t[:, 0], t[:, 1], M)


def _clamp_sides(N, M):
    """Rows below / above the reference clamp in fp64; none sits on it."""
    ls = _log_s(N, M)
    assert _clear_of_clamp(ls)
    below = ls < LOG_CLAMP
    if N >= 65:   # (with 9 rows or fewer and one component every row can lie below the clamp)
        assert bool(below.any()) and bool((~below).any()), "the table must hold both branches of the clamp"
    return below


def _check_terms(tag, got, o32, o64, margin=4.0):
    for name, a, b, c in zip(("total", "shape", "pen"), got, o32[:3], o64[:3]):
        R.check("%s %s" % (tag, name), a.detach().reshape(1), b.reshape(1), c.reshape(1), margin=margin)


# ---------------------------------------------------------------------------------
# csrc/mdn.hip
# ---------------------------------------------------------------------------------
# Largest err_k / err_32 measured on an MI355X over every case below (margin 4,
# none raised): dz rho 3.79, s1 3.65, mu1 3.12, mu2 2.87, pi 1.70, pen 1.63,
# s2 1.58; loss terms pen 2.04, total 1.97, shape 1.00.
@pytest.mark.parametrize("mode", ["magenta", "reference"])
@pytest.mark.parametrize("M", [1, 5, 20, 32])
@pytest.mark.parametrize("N", [1, 7, 9, 1001])
def test_mdn_loss_kernel_on_the_edge_table(N, M, mode):
    """N crosses the 8 rows of a workgroup; M from one component to all 32
    lanes; both ``is_training`` values (``mask_pen``)."""
    z, t = _table(N, M)
    below = _clamp_sides(N, M)
    for is_training in (True, False):
        o64, o32 = _refs(N, M, mode, is_training)
        ops.set_backend("hip")
        zk = z.float().clone().requires_grad_()
        got = ops.mdn_loss(zk, t, M, mode=mode, stroke_importance=200.0, is_training=is_training)
        got[0].backward()
        torch.cuda.synchronize()
        tag = "mdn.hip[%s]" % mode
        _check_terms(tag, got, o32, o64)
        for name, sl in zip(GROUPS, _groups(M)):
            R.check("%s dz %s" % (tag, name), zk.grad[:, sl], o32[3][:, sl], o64[3][:, sl])
        if mode == "reference":   # a clamped row: exactly zero mixture gradient
            assert not bool(zk.grad[below][:, 3:].any())
            assert not bool(o64[3][below][:, 3:].any())


# ---------------------------------------------------------------------------------
# csrc/mdn_head.hip through an exact projection
# ---------------------------------------------------------------------------------
def _identity_head(z):
    """``x [N, HD]``, ``W [HD, nz]``, ``b`` with ``x @ W + b == z`` exactly in
    bf16 operands: ``W[:nz, :nz] = I``, ``x[:, :nz] = z`` (bf16-exact), zeros elsewhere."""
    N, nz = z.shape
    x = torch.zeros(N, HD, device=DEV)
    x[:, :nz] = z.float()
    W = torch.zeros(HD, nz, device=DEV)
    W[:nz, :nz] = torch.eye(nz, device=DEV)
    return x, W, torch.zeros(nz, device=DEV)


# Measured on an MI355X: loss terms pen 2.04, total 1.97, shape 13.1 in magenta
# mode (1.00 in reference mode) -- the pi softmax runs on __expf / __logf, but
# err_32 there is below the rule's 4 * 2^-24 |q64| term and the shape term uses
# 0.39 of the bound, so the margin stays 4. dx uses up to 0.99 and db up to
# 0.92 of their bounds: a bf16 store does reach its half ulp, 2^-8.
def _head_case(N, M, mode, lp_rows, coef):
    z, t = _table(N, M)
    nz = z.shape[1]
    _clamp_sides(N, M)
    o64, o32 = _refs(N, M, mode, True, coef)
    x, W, b = _identity_head(z)
    assert torch.equal(x.bfloat16().double()[:, :nz], z)
    ops.set_backend("hip")
    ops.set_compute_dtype("bf16")
    xs, Ws, bs = (v.clone().requires_grad_() for v in (x, W, b))
    assert mdn_hip.head_fused_ok(xs, Ws, M)
    got = ops.mdn_head_loss(xs, Ws, bs, t, M, mode=mode, stroke_importance=200.0, drop_keep=1.0,
                            x_lp=x.bfloat16() if lp_rows else None)
    (coef[0] * got[0] + coef[1] * got[1] + coef[2] * got[2]).backward()
    torch.cuda.synchronize()
    tag = "mdn_head.hip[%s]" % mode
    if coef == (1.0, 0.0, 0.0):
        _check_terms(tag, got, o32, o64)
    dz64, dz32 = o64[3], o32[3]
    dx, db = xs.grad.double(), bs.grad.double()
    assert not bool(dx[:, nz:].any()), "dx past the identity block must be exactly 0"
    for name, sl in zip(GROUPS, _groups(M)):
        # dz is stored in bf16, one rounding (the upstream scales multiply fp32
        # sums): 2^-8 |dz64| elementwise, plus the rule's fp32 terms for the column group
        _, e32, top = R.errors(dz32[:, sl], dz32[:, sl], dz64[:, sl])
        floor = 4.0 * e32 + 4.0 * R.EPS32 * top
        bound = 2.0 ** -8 * dz64[:, sl].abs() + floor
        err = (dx[:, sl] - dz64[:, sl]).abs()
        used = float((err / bound).max()) if top > 0.0 else float(err.max())
        R.record("%s dx %s (share of bound)" % (tag, name), used, used)
        assert bool((err <= bound).all()), (name, used)
        # db: the column sums of the same bf16 dz
        s64, s32 = dz64[:, sl].sum(0), dz32[:, sl].double().sum(0)
        floor = 4.0 * float((s32 - s64).abs().max()) + 4.0 * R.EPS32 * float(s64.abs().max())
        bound = 2.0 ** -8 * dz64[:, sl].abs().sum(0) + floor
        err = (db[sl] - s64).abs()
        used = float((err / bound).max()) if float(bound.max()) > 0.0 else float(err.max())
        R.record("%s db %s (share of bound)" % (tag, name), used, used)
        assert bool((err <= bound).all()), (name, used)


@pytest.mark.parametrize("lp_rows", [False, True], ids=["fp32_rows", "bf16_rows"])
@pytest.mark.parametrize("mode", ["magenta", "reference"])
@pytest.mark.parametrize("M", [1, 20, 24])
@pytest.mark.parametrize("N", [1, 65, 200])
def test_fused_head_on_the_edge_table(N, M, mode, lp_rows):
    """N around the 64-row forward tile; fp32 rows and ``x_lp`` bf16 rows."""
    _head_case(N, M, mode, lp_rows, (1.0, 0.0, 0.0))


@pytest.mark.parametrize("mode", ["magenta", "reference"])
def test_fused_head_upstream_coefficients_on_the_edge_table(mode):
    _head_case(200, 20, mode, False, (0.7, 1.3, -0.4))


# ---------------------------------------------------------------------------------
# csrc/mdn_score.hip through the same projection
# ---------------------------------------------------------------------------------
def _score_oracle(z, t, lens, T, B, M, end, dtype):
    z, t = z.to(dtype), t.to(dtype)
    log_s = mdn.log_mixture_density(z, t[:, 0], t[:, 1], M)
    shape = -torch.logaddexp(log_s, torch.full_like(log_s, math.log(1e-6)))
    pen = -(t[:, 2:5] * torch.log_softmax(z[:, 0:3], -1)).sum(-1)
    step = torch.arange(T, device=z.device).unsqueeze(1)
    m_shape = step < lens.unsqueeze(0)
    m_pen = step < (lens + (1 if end else 0)).unsqueeze(0)
    zero = torch.zeros((), dtype=dtype, device=z.device)
    return (torch.where(m_shape, shape.view(T, B), zero).sum(0), torch.where(m_pen, pen.view(T, B), zero).sum(0))


@pytest.mark.parametrize("end", [False, True], ids=["no_end", "include_end"])
@pytest.mark.parametrize("M", [1, 20, 24])
def test_score_kernel_on_the_edge_table(M, end):
    """[T, B, Hd] = [5, 19, 256], lengths 1 .. T: per-sketch shape and pen sums
    against fp64 sums of the per-row oracle terms over each sketch's own rows;
    the rows past them are NaN-poisoned. Measured err_k / err_32 on an MI355X:
    pen 1.91, shape 1.00."""
    T, B = 5, 19
    z, t = _table(T * B, M)
    lens = (torch.arange(B, device=DEV) * 3) % T + 1
    assert int(lens.min()) == 1 and int(lens.max()) == T
    s64 = _score_oracle(z, t, lens, T, B, M, end, torch.float64)
    s32 = _score_oracle(z, t, lens, T, B, M, end, torch.float32)
    assert all(bool(torch.isfinite(v).all()) for v in s64)
    x, W, b = _identity_head(z)
    x, tt = x.view(T, B, HD).clone(), t.view(T, B, 5).clone()
    dead = torch.arange(T, device=DEV).unsqueeze(1) >= (lens + (1 if end else 0)).unsqueeze(0)
    x[dead] = float("nan")
    tt[dead] = float("nan")
    ops.set_backend("hip")
    ops.set_compute_dtype("bf16")
    from sketch_rnn_amd.ops.mdn_score import score_fused_ok
    assert score_fused_ok(x, W, M)
    for lp in (None, x.bfloat16()):
        with torch.no_grad():
            shape, pen = ops.mdn_head_score(x, W, b, tt, lens, M, include_end=end, x_lp=lp)
        torch.cuda.synchronize()
        R.check("mdn_score.hip shape", shape, s32[0], s64[0])
        R.check("mdn_score.hip pen", pen, s32[1], s64[1])

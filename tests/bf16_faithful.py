"""Rounding-faithful references for the bf16 LSTM kernels.

Plain PyTorch scans with a hand-written forward and reverse-time backward.
Each takes a ``dtype`` (fp64 or fp32 arithmetic) and a ``rounded`` flag:

* ``rounded=False``: the exact formula (equal to the torch-backend oracle and
  its autograd; tests/test_bf16_faithful.py proves that on the CPU);
* ``rounded=True``: the same formula with a round to bf16
  (``t.to(torch.bfloat16).to(t.dtype)``) at exactly the points where the host
  code hands bf16 to a kernel, or a kernel hands bf16 to the next one.

tests/test_bf16_faithful_gpu.py computes every quantity three ways -- ``q64``
(exact, fp64), ``qb`` (rounded, fp32: a transcription, not the code under
test) and ``qk`` (the kernels) -- and bounds the kernel by the rule of
tests/fp64_rule.py: ``max|qk - q64| <= 4 max|qb - q64| + 4 * 2^-24 max|q64|``.

Rounding points (read from the code, not from what a kernel returns):

========================================  =====================================================================
rounded value                             where
========================================  =====================================================================
``W_h``, cast once per sequence           sketch_rnn_amd/ops/gemm.py:35 (``lp``) from ops/recurrent.py:268,270;
                                          ops/gemm.py:727 (``cast_transpose``) from ops/persist.py:111,117
carried h, ``h0`` and the eoc-reset       buffer and ``h0``: ops/recurrent.py:273-274, ops/persist.py:139-142;
value included; operand of ``h W_h``      written per step by csrc/lstm_fused.hip:165-168,
and of ``dW = h^T dG``                    csrc/cell_fwd_body.h:312, csrc/row_cell.h:272-273,
                                          csrc/lstm_persist.hip:294-301; read by the weight gradient at
                                          ops/recurrent.py:475-479 and ops/persist.py:234-238
gate gradient ``dG`` (``dG_lp``);         written by csrc/cell_bwd_body.h:211, csrc/row_cell.h:462,
operand of ``dG W_h^T``, of ``dW`` and,   csrc/lstm_fused.hip:266, csrc/lstm_persist.hip:556; read at
in the fused encoder, of the input-       ops/recurrent.py:425,434,461,471 (``dG W_h^T``), :473-479 (``dW``),
projection gradients                      ops/persist.py:236-238 (``dW``), :304-312 (fused encoder: ``dW_x``,
                                          ``db`` from ``dg_lp``), csrc/lstm_persist.hip:465-473 (``dG W_h^T``)
stack: ``W_in1``                          ops/persist.py:116
stack: layer 0's (un-reset) h as layer    ``hup`` / ``hlp[0][0, 1:]``: ops/persist.py:143,242,
1's input and as operand of ``dW_in1``;   csrc/lstm_persist.hip:199,311-314; ``dW_in1`` and ``db1`` (column
``dG_1`` as operand of ``dW_in1``,        sums of the bf16 ``dG_1``): ops/persist.py:243; the product
``db1`` and ``dG_1 W_in1^T``              ``dG_1 W_in1^T``: csrc/lstm_persist.hip:478-489
LayerNorm-LSTM, ``LN_SAVES_LP``:          dtype of the saves: ops/recurrent.py:285-289 (forward),
``xhat``, ``chat`` saved bf16. The        :400-402 (backward); stores csrc/cell_fwd_body.h:258-260,
forward runs on the fp32 values; the      csrc/row_cell.h:264-266. EVERY backward consumer reads the
backward reads only the saves             rounded value (csrc/cell_bwd_body.h:58,63 and csrc/row_cell.h:321,326):
                                          the recomputed gate activations (cell_bwd_body.h:97-100,
                                          row_cell.h:380-383), ``tanh(chat g + b)`` (:119 / :389), both
                                          LayerNorm-backward row sums and corrections (:126,136,166,185 /
                                          :395,407,424,436) and the gamma gradients (below)
LayerNorm-LSTM, ``LN_SAVES_LP``:          stores csrc/cell_bwd_body.h:175,178, csrc/row_cell.h:428,432; their
``dlny``, ``dlncy`` saved bf16            only consumer is the gamma / beta column sums
                                          ``sum dlny * xhat``, ``sum dlny`` (ops/recurrent.py:481-489,
                                          ops/reduce.py:3), which therefore read both operands rounded; the
                                          in-step gate gradient uses the fp32 values
========================================  =====================================================================

``xp``, the cell state c, ``Hout``, the saved plain-LSTM gate activations
(``act``, fp32), the LayerNorm ``rstd`` and all pointwise math stay fp32.
The final carried ``h_T`` is returned un-rounded (ops/recurrent.py:363,
csrc/lstm_persist.hip:343), and ``dxp`` is the fp32 ``dG``.

Dropout masks come from ``models.cells.dropout_mask`` with the stream
numbering of the torch backend: one stream over the ``nd * B`` rows of a
sequence (``ops.bilstm_sequence``'s ``mask_rows``), ``stream + l`` for layer
``l`` of a stack. The kernels' own hash is part of what is under test.
"""
import torch

from sketch_rnn_amd.models.cells import LN_EPS, dropout_mask


def bf16(t, on=True):
    """Round to bf16 and back (``on=False``: identity)."""
    return t.to(torch.bfloat16).to(t.dtype) if on else t


class _Scan:
    """Plain holder of one scan's forward results and saves."""


def lstm_forward(xp, W_h, h0, c0, *, nd=1, reset=None, reset_h=None, reset_c=None, keep=1.0, seed=0, stream=0,
                 forget_bias=1.0, ln=None, ln_saves_lp=True, dtype=torch.float64, rounded=False):
    """LSTM / LayerNorm-LSTM scan over ``xp [T, nd*B, 4H]`` with ``nd``
    direction groups (``W_h [nd, H, 4H]`` or ``[H, 4H]``; ``ln`` parameters
    ``[nd, n]`` or ``[n]``), the eoc reset of ``ops.lstm_sequence``
    (``reset[t, b] != 0``: the state carried out of step t becomes
    ``(reset_h, reset_c)``) and hashed recurrent dropout. Returns a holder
    with ``out [T, nd*B, H]``, ``hT``, ``cT`` and the saves of
    :func:`lstm_backward`."""
    T, NB, G = xp.shape
    H, B = G // 4, NB // nd
    cv = lambda t: t.detach().to(dtype)   # noqa: E731
    s = _Scan()
    s.dims, s.rounded, s.wshape, s.forget_bias = (T, nd, B, H), rounded, W_h.shape, forget_bias
    s.Wq = bf16(cv(W_h).reshape(nd, H, G), rounded)
    xp = cv(xp).reshape(T, nd, B, 4, H)
    h, c = cv(h0).reshape(nd, B, H), cv(c0).reshape(nd, B, H)
    s.reset = None
    if reset is not None:
        s.reset = (reset.detach() != 0).reshape(T, nd, B, 1)
        rh, rc = cv(reset_h).reshape(nd, B, H), cv(reset_c).reshape(nd, B, H)
    s.ln = None
    if ln is not None:
        s.ln = (cv(ln[0]).reshape(nd, 1, 4, H), cv(ln[1]).reshape(nd, 1, 4, H),
                cv(ln[2]).reshape(nd, 1, H), cv(ln[3]).reshape(nd, 1, H))
        s.saves_lp = rounded and ln_saves_lp
    s.steps, outs = [], []
    for t in range(T):
        st = _Scan()
        st.hq, st.c_prev = bf16(h, rounded), c
        g = xp[t] + torch.bmm(st.hq, s.Wq).reshape(nd, B, 4, H)
        st.m = 1.0
        if keep < 1.0:
            st.m = dropout_mask(seed, stream, t, (NB, H), keep, xp.device).to(dtype).reshape(nd, B, H)
        if s.ln is not None:
            mean = g.mean(-1, keepdim=True)
            st.rstd = torch.rsqrt(((g - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
            st.xhat = (g - mean) * st.rstd
            g = st.xhat * s.ln[0] + s.ln[1]
        i, tj = torch.sigmoid(g[:, :, 0]), torch.tanh(g[:, :, 1])
        f, o = torch.sigmoid(g[:, :, 2] + forget_bias), torch.sigmoid(g[:, :, 3])
        st.act = (i, tj, f, o)
        st.cn = c * f + i * tj * st.m
        if s.ln is not None:
            mean = st.cn.mean(-1, keepdim=True)
            st.rc = torch.rsqrt(((st.cn - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
            st.chat = (st.cn - mean) * st.rc
            hn = torch.tanh(st.chat * s.ln[2] + s.ln[3]) * o
        else:
            hn = torch.tanh(st.cn) * o
        outs.append(hn)
        if s.reset is not None:
            h, c = torch.where(s.reset[t], rh, hn), torch.where(s.reset[t], rc, st.cn)
        else:
            h, c = hn, st.cn
        s.steps.append(st)
    s.out = torch.stack(outs, 0).reshape(T, NB, H)
    s.hT, s.cT = h.reshape(NB, H), c.reshape(NB, H)
    return s


def lstm_backward(s, dout=None, dhT=None, dcT=None):
    """Reverse-time backward of :func:`lstm_forward`. Returns a holder with
    ``dxp`` (the fp32 gate gradient), ``dGq`` (its bf16-rounded copy, the
    GEMM operand), ``dW`` (shape of ``W_h``), ``dh0``, ``dc0``, ``dreset_h``,
    ``dreset_c`` (zeros without resets) and ``dln`` (four LayerNorm parameter
    gradients ``[nd, n]``, or None)."""
    T, nd, B, H = s.dims
    dtype, dev = s.Wq.dtype, s.Wq.device
    z = lambda: torch.zeros(nd, B, H, dtype=dtype, device=dev)   # noqa: E731
    dh_c = dhT.detach().to(dtype).reshape(nd, B, H) if dhT is not None else z()
    dc_c = dcT.detach().to(dtype).reshape(nd, B, H) if dcT is not None else z()
    dout = dout.detach().to(dtype).reshape(T, nd, B, H) if dout is not None else None
    drh, drc = z(), z()
    dW = torch.zeros(nd, H, 4 * H, dtype=dtype, device=dev)
    dxp, dGq = [None] * T, [None] * T
    dln = None
    if s.ln is not None:
        lg, lb, lcg, lcb = s.ln
        dln = [torch.zeros(nd, 4, H, dtype=dtype, device=dev), torch.zeros(nd, 4, H, dtype=dtype, device=dev),
               torch.zeros(nd, H, dtype=dtype, device=dev), torch.zeros(nd, H, dtype=dtype, device=dev)]
    for t in range(T - 1, -1, -1):
        st = s.steps[t]
        dh = dout[t] if dout is not None else z()
        if s.reset is not None:
            r = s.reset[t]
            drh, drc = drh + torch.where(r, dh_c, 0.0), drc + torch.where(r, dc_c, 0.0)
            dh, dc = dh + torch.where(r, 0.0, dh_c), torch.where(r, 0.0, dc_c)
        else:
            dh, dc = dh + dh_c, dc_c
        if s.ln is None:
            i, tj, f, o = st.act
            th = torch.tanh(st.cn)
            dc = dc + dh * o * (1 - th * th)
        else:
            # the backward sees only the saves: gates recomputed from xhat
            xh, cx = bf16(st.xhat, s.saves_lp), bf16(st.chat, s.saves_lp)
            y = xh * lg + lb
            i, tj = torch.sigmoid(y[:, :, 0]), torch.tanh(y[:, :, 1])
            f, o = torch.sigmoid(y[:, :, 2] + s.forget_bias), torch.sigmoid(y[:, :, 3])
            th = torch.tanh(cx * lcg + lcb)
            dlc = dh * o * (1 - th * th)
            dch = dlc * lcg
            dc = dc + st.rc * (dch - dch.mean(-1, keepdim=True) - cx * (dch * cx).mean(-1, keepdim=True))
            dlcq = bf16(dlc, s.saves_lp)
            dln[2], dln[3] = dln[2] + (dlcq * cx).sum(1), dln[3] + dlcq.sum(1)
        dy = torch.stack([dc * tj * st.m * i * (1 - i), dc * i * st.m * (1 - tj * tj),
                          dc * st.c_prev * f * (1 - f), dh * th * o * (1 - o)], 2)   # [nd, B, 4, H]
        dc_c = dc * f
        if s.ln is not None:
            dyq = bf16(dy, s.saves_lp)
            dln[0], dln[1] = dln[0] + (dyq * xh).sum(1), dln[1] + dyq.sum(1)
            dg = dy * lg
            dy = st.rstd * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))
        dG = dy.reshape(nd, B, 4 * H)
        dxp[t] = dG
        dGq[t] = bf16(dG, s.rounded)
        dh_c = torch.bmm(dGq[t], s.Wq.transpose(1, 2))
        dW = dW + torch.bmm(st.hq.transpose(1, 2), dGq[t])
    g = _Scan()
    g.dxp = torch.stack(dxp, 0).reshape(T, nd * B, 4 * H)
    g.dGq = torch.stack(dGq, 0).reshape(T, nd * B, 4 * H)
    g.dW = dW.reshape(s.wshape)
    g.dh0, g.dc0 = dh_c.reshape(nd * B, H), dc_c.reshape(nd * B, H)
    g.dreset_h, g.dreset_c = drh.reshape(nd * B, H), drc.reshape(nd * B, H)
    g.dln = None
    if dln is not None:
        g.dln = [dln[0].reshape(nd, 4 * H), dln[1].reshape(nd, 4 * H), dln[2], dln[3]]
    return g


# ---- bidirectional encoder: packed layout, backward direction reversed within each length ----
def reverse_within_length(x, lengths):
    """Time-major ``x [T, B, D]`` with each row's first ``len`` steps reversed
    (steps from ``len`` on unchanged: nothing reads them)."""
    xr = x.clone()
    for b, n in enumerate(lengths.tolist()):
        if n > 1:
            xr[:n, b] = x[:n, b].flip(0)
    return xr


def encoder_forward(x, lengths, W_xf, W_xb, b_f, b_b, W_hf, W_hb, *, keep=1.0, seed=0, stream=0, forget_bias=1.0,
                    dtype=torch.float64, rounded=False):
    """The VAE encoder's recurrent part: ``xp = [x W_xf + b_f ; rev(x) W_xb +
    b_b]`` packed as ``[T, 2B, 4H]`` (forward rows first; fp32 in the kernels,
    so never rounded), both directions from a zero state, and ``last =
    [h_fw[len-1] | h_bw[len-1]]`` (``[B, 2H]``)."""
    T, B, _ = x.shape
    H = W_hf.shape[0]
    cv = lambda t: t.detach().to(dtype)   # noqa: E731
    e = _Scan()
    e.x, e.B, e.H = cv(x), B, H
    e.xr = reverse_within_length(e.x, lengths)
    xp = torch.cat([e.x @ cv(W_xf) + cv(b_f), e.xr @ cv(W_xb) + cv(b_b)], 1)
    zero = torch.zeros(2 * B, H, dtype=dtype, device=x.device)
    e.s = lstm_forward(xp, torch.stack([W_hf, W_hb], 0), zero, zero, nd=2, keep=keep, seed=seed, stream=stream,
                       forget_bias=forget_bias, dtype=dtype, rounded=rounded)
    e.idx = (lengths.to(x.device) - 1).clamp(min=0)
    e.ar = torch.arange(B, device=x.device)
    e.last = torch.cat([e.s.out[e.idx, e.ar], e.s.out[e.idx, B + e.ar]], -1)
    return e


def encoder_backward(e, dlast, proj_from_lp=True):
    """Gradients of :func:`encoder_forward` given ``dlast [B, 2H]``:
    ``(dW_xf, dW_xb, db_f, db_b, dW_hf, dW_hb)``. ``proj_from_lp``: the
    input-projection gradients read the bf16 gate gradient (the fused encoder,
    ops/persist.py:304-312); False: the fp32 one (the unfused path's ``dxp``)."""
    T, _, B, H = e.s.dims
    dlast = dlast.detach().to(e.x.dtype)
    dout = torch.zeros_like(e.s.out)
    dout[e.idx, e.ar] = dlast[:, :H]
    dout[e.idx, B + e.ar] = dlast[:, H:]
    g = lstm_backward(e.s, dout)
    dg = g.dGq if proj_from_lp else g.dxp
    IN = e.x.shape[-1]
    dgf, dgb = dg[:, :B].reshape(T * B, 4 * H), dg[:, B:].reshape(T * B, 4 * H)
    return (e.x.reshape(T * B, IN).t() @ dgf, e.xr.reshape(T * B, IN).t() @ dgb, dgf.sum(0), dgb.sum(0),
            g.dW[0], g.dW[1])


# ---- 2-layer stack: layer 1's input product inside the recurrence ----------------------------
def stack_forward(xp0, W_h0, W_in1, b1, W_h1, h0s, c0s, *, reset=None, keep=1.0, seed=0, stream=0, forget_bias=1.0,
                  dtype=torch.float64, rounded=False):
    """Two stacked LSTM layers over ``xp0 [T, B, 4H]``: layer 1 reads layer
    0's un-reset outputs through ``W_in1`` (+ ``b1``); every layer's state is
    reset to its own initial state after an eoc input. Returns a holder with
    ``out`` (layer 1's outputs) and ``finals = [(hT, cT)] * 2``."""
    k = _Scan()
    cv = lambda t: t.detach().to(dtype)   # noqa: E731
    kw = dict(keep=keep, seed=seed, forget_bias=forget_bias, dtype=dtype, rounded=rounded)
    k.s0 = lstm_forward(xp0, W_h0, h0s[0], c0s[0], reset=reset, reset_h=h0s[0], reset_c=c0s[0], stream=stream, **kw)
    k.Winq, k.up = bf16(cv(W_in1), rounded), bf16(k.s0.out, rounded)
    xp1 = k.up @ k.Winq + cv(b1)
    k.s1 = lstm_forward(xp1, W_h1, h0s[1], c0s[1], reset=reset, reset_h=h0s[1], reset_c=c0s[1], stream=stream + 1,
                        **kw)
    k.out, k.finals = k.s1.out, [(k.s0.hT, k.s0.cT), (k.s1.hT, k.s1.cT)]
    return k


def stack_backward(k, dout, dfinals):
    """Gradients of :func:`stack_forward`: a dict with ``dxp0``, ``dW_h0``,
    ``dW_in1``, ``db1``, ``dW_h1`` and ``dh0_l`` / ``dc0_l`` (the initial
    state is also the reset target: both parts summed)."""
    T, _, B, H = k.s1.dims
    g1 = lstm_backward(k.s1, dout, *dfinals[1])
    dq = g1.dGq.reshape(T * B, 4 * H)
    g0 = lstm_backward(k.s0, (dq @ k.Winq.t()).reshape(T, B, H), *dfinals[0])
    res = {"dxp0": g0.dxp, "dW_h0": g0.dW, "dW_in1": k.up.reshape(T * B, H).t() @ dq, "db1": dq.sum(0),
           "dW_h1": g1.dW}
    for l, g in enumerate((g0, g1)):
        res["dh0_%d" % l], res["dc0_%d" % l] = g.dh0 + g.dreset_h, g.dc0 + g.dreset_c
    return res


# =================================================================================================
# Case runners shared by tests/test_bf16_faithful.py (CPU: ``run_*_ops`` under the torch backend
# in fp64 is the oracle) and tests/test_bf16_faithful_gpu.py (``run_*_ops`` under the hip backend
# with bf16 compute is the kernel path). Both kinds return ``{quantity name: tensor}`` with the
# same keys: forward outputs, final states and every gradient of
# ``loss = sum(output * fixed random weight)`` over every output.
# =================================================================================================
SEED, STREAM = 7, 3


def _leaf(t, dtype):
    return t.detach().to(dtype).requires_grad_()


def seq_inputs(T, B, H, nd, device, reset=False, ln=False, seed=0):
    """fp32 inputs of one sequence case (made on the CPU generator, so the
    same on every device). ``nd = 2``: the packed bidirectional layout, one
    ``h0 / c0 [B, H]`` shared by both directions."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + 3 * B + H + nd)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    inp = {"xp": 0.5 * rn(T, nd * B, 4 * H), "W": rn(nd, H, 4 * H) / H ** 0.5, "h0": 0.3 * rn(B, H),
           "c0": 0.3 * rn(B, H)}
    if reset:
        inp["reset"] = (torch.rand(T, B, generator=g) < 0.3).float()
        inp["reset"][0, 0] = inp["reset"][T - 1, 0] = 1.0
        inp["reset"][T - 1, B - 1] = 1.0
        inp["reset_h"], inp["reset_c"] = 0.3 * rn(B, H), 0.3 * rn(B, H)
    if ln:
        inp["ln"] = [1 + 0.1 * rn(4 * H), 0.1 * rn(4 * H), 1 + 0.1 * rn(H), 0.1 * rn(H)]
    inp["wo"], inp["wh"], inp["wc"] = rn(T, nd * B, H), rn(B, H), rn(B, H)
    return {k: ([t.to(device) for t in v] if isinstance(v, list) else v.to(device)) for k, v in inp.items()}


_LN_NAMES = ("dln_gamma", "dln_beta", "dlnc_gamma", "dlnc_beta")


def run_seq_ops(inp, nd, keep, dtype):
    """``ops.lstm_sequence`` (nd = 1) / ``ops.bilstm_sequence_packed`` (nd = 2)
    under the current backend and compute dtype, on ``dtype`` leaves."""
    from sketch_rnn_amd import ops
    xp, W, h0, c0 = (_leaf(inp[k], dtype) for k in ("xp", "W", "h0", "c0"))
    q = {}
    if nd == 1:
        rst = inp.get("reset")
        rh, rc = (_leaf(inp[k], dtype) for k in ("reset_h", "reset_c")) if rst is not None else (None, None)
        ln = [_leaf(t, dtype) for t in inp["ln"]] if "ln" in inp else None
        out, (hT, cT) = ops.lstm_sequence(xp, W[0], h0, c0, reset=rst, reset_h=rh, reset_c=rc, drop_keep=keep,
                                          drop_seed=SEED, drop_stream=STREAM, ln=tuple(ln) if ln else None)
        loss = (out * inp["wo"].to(out.dtype)).sum() + (hT * inp["wh"].to(out.dtype)).sum() \
            + (cT * inp["wc"].to(out.dtype)).sum()
        q["hT"], q["cT"] = hT.detach(), cT.detach()
    else:
        of, ob = ops.bilstm_sequence_packed(xp, W[0], W[1], h0, c0, drop_keep=keep, drop_seed=SEED,
                                            drop_stream=STREAM)
        out = torch.cat([of, ob], 1)
        loss = (out * inp["wo"].to(out.dtype)).sum()
    loss.backward()
    q.update({"out": out.detach(), "dxp": xp.grad, "dW": W.grad, "dh0": h0.grad, "dc0": c0.grad})
    if nd == 1 and rst is not None:
        q["dreset_h"], q["dreset_c"] = rh.grad, rc.grad
    if nd == 1 and ln:
        q.update({n: t.grad for n, t in zip(_LN_NAMES, ln)})
    return q


def run_seq_scan(inp, nd, keep, dtype, rounded):
    B = inp["h0"].shape[0]
    rep = lambda t: torch.cat([t] * nd, 0)   # noqa: E731
    rst = inp.get("reset")
    s = lstm_forward(inp["xp"], inp["W"], rep(inp["h0"]), rep(inp["c0"]), nd=nd, reset=rst,
                     reset_h=inp.get("reset_h"), reset_c=inp.get("reset_c"), keep=keep, seed=SEED, stream=STREAM,
                     ln=inp.get("ln"), dtype=dtype, rounded=rounded)
    g = lstm_backward(s, inp["wo"], inp["wh"] if nd == 1 else None, inp["wc"] if nd == 1 else None)
    q = {"out": s.out, "dxp": g.dxp, "dW": g.dW.reshape(nd, -1, g.dW.shape[-1]),
         "dh0": g.dh0.reshape(nd, B, -1).sum(0), "dc0": g.dc0.reshape(nd, B, -1).sum(0)}
    if nd == 1:
        q["hT"], q["cT"] = s.hT, s.cT
        if rst is not None:
            q["dreset_h"], q["dreset_c"] = g.dreset_h, g.dreset_c
        if g.dln is not None:
            q.update({n: t.reshape(-1) for n, t in zip(_LN_NAMES, g.dln)})
    return q


# ---- the 2-layer SketchRNN stack (models/reference.py ``features``: no head) -----------------------
def stack_inputs(m, B, T, device, seed=0):
    """Stroke-5 input ``[B, T, 5]`` with eoc flags that include a reset at
    ``t = 0`` and at ``t = T - 1``, and a non-zero initial state."""
    H = m.cfg.rnn_size
    g = torch.Generator().manual_seed(100 * seed + B + T)
    x = torch.randn(B, T, 5, generator=g) * 0.6
    pen = torch.randint(0, 3, (B, T), generator=g)
    pen[0, 0] = pen[0, T - 1] = pen[B - 1, T - 1] = 1
    x[..., 2:] = torch.nn.functional.one_hot(pen, 3).float()
    state = [(0.3 * torch.randn(B, H, generator=g), 0.5 * torch.randn(B, H, generator=g)) for _ in m.layers]
    w = [torch.randn(T, B, H, generator=g)] + [torch.randn(B, H, generator=g) for _ in range(2 * len(m.layers))]
    return {"x": x.to(device), "state": [(h.to(device), c.to(device)) for h, c in state],
            "w": [t.to(device) for t in w]}


_STACK_PARAMS = {"layers.0.W_x": "dW_x0", "layers.0.bias": "db0", "layers.0.W_h": "dW_h0", "layers.1.W_x": "dW_in1",
                 "layers.1.bias": "db1", "layers.1.W_h": "dW_h1"}


def run_stack_ops(m, inp, dtype):
    import copy
    mm = copy.deepcopy(m).to(dtype)
    B, T, _ = inp["x"].shape
    st = [(_leaf(h, dtype), _leaf(c, dtype)) for h, c in inp["state"]]
    out, final = mm.features(inp["x"].to(dtype), st)
    out = out.reshape(T, B, -1)
    outs = [out] + [t for f in final for t in f]
    sum((o * w.to(o.dtype)).sum() for o, w in zip(outs, inp["w"])).backward()
    q = {"out": out.detach()}
    for l, (f, s_) in enumerate(zip(final, st)):
        q["hT_%d" % l], q["cT_%d" % l] = f[0].detach(), f[1].detach()
        q["dh0_%d" % l], q["dc0_%d" % l] = s_[0].grad, s_[1].grad
    params = dict(mm.named_parameters())
    q.update({name: params[n].grad for n, name in _STACK_PARAMS.items()})
    return q


def run_stack_scan(m, inp, dtype, rounded):
    p0, p1 = m.layers
    B, T, _ = inp["x"].shape
    xt = inp["x"].transpose(0, 1).to(dtype)
    Wx0, b0 = _leaf(p0.W_x, dtype), _leaf(p0.bias, dtype)
    xp0 = (xt.reshape(T * B, 5) @ Wx0 + b0).reshape(T, B, -1)   # K = 5, fp32 in the kernels: never rounded
    k = stack_forward(xp0, p0.W_h, p1.W_x, p1.bias, p1.W_h, [s_[0] for s_ in inp["state"]],
                      [s_[1] for s_ in inp["state"]], reset=(xt[:, :, 3] > 0).float(), dtype=dtype, rounded=rounded)
    w = inp["w"]
    r = stack_backward(k, w[0], [(w[1], w[2]), (w[3], w[4])])
    xp0.backward(r.pop("dxp0"))
    q = {"out": k.out, "dW_x0": Wx0.grad, "db0": b0.grad}
    for l, (hT, cT) in enumerate(k.finals):
        q["hT_%d" % l], q["cT_%d" % l] = hT, cT
    q.update(r)
    return q


# ---- the VAE encoder (models/vae.py ``Encoder``) ------------------------------------------------------
def encoder_inputs(T, B, Z, lengths, device, seed=0):
    g = torch.Generator().manual_seed(10 * seed + T + B)
    x = torch.randn(T, B, 5, generator=g) * 0.5
    return {"x": x.to(device), "lengths": torch.as_tensor(lengths, dtype=torch.int64).to(device),
            "w": [torch.randn(B, Z, generator=g).to(device) for _ in range(2)]}


_ENC_PARAMS = ("fw.W_x", "fw.W_h", "fw.bias", "bw.W_x", "bw.W_h", "bw.bias", "mu_w", "mu_b", "sig_w", "sig_b")


def run_encoder_ops(enc, inp, dtype):
    import copy
    e = copy.deepcopy(enc).to(dtype)
    mu, ps = e(inp["x"].to(dtype), inp["lengths"], True, SEED)
    ((mu * inp["w"][0].to(mu.dtype)).sum() + (ps * inp["w"][1].to(mu.dtype)).sum()).backward()
    params = dict(e.named_parameters())
    q = {"mu": mu.detach(), "presig": ps.detach()}
    q.update({"d" + n: params[n].grad for n in _ENC_PARAMS})
    return q


def run_encoder_scan(enc, inp, dtype, rounded):
    from sketch_rnn_amd.models.vae import _S_ENC_FW
    cfg = enc.cfg
    keep = cfg.recurrent_dropout_prob if cfg.use_recurrent_dropout else 1.0
    e = encoder_forward(inp["x"], inp["lengths"], enc.fw.W_x, enc.bw.W_x, enc.fw.bias, enc.bw.bias, enc.fw.W_h,
                        enc.bw.W_h, keep=keep, seed=SEED, stream=_S_ENC_FW, dtype=dtype, rounded=rounded)
    last = e.last.detach().requires_grad_()
    head = {n: _leaf(getattr(enc, n), dtype) for n in ("mu_w", "mu_b", "sig_w", "sig_b")}   # plain fp32 products
    mu, ps = last @ head["mu_w"] + head["mu_b"], last @ head["sig_w"] + head["sig_b"]
    ((mu * inp["w"][0].to(dtype)).sum() + (ps * inp["w"][1].to(dtype)).sum()).backward()
    gr = encoder_backward(e, last.grad)
    q = {"mu": mu.detach(), "presig": ps.detach()}
    q.update(zip(("dfw.W_x", "dbw.W_x", "dfw.bias", "dbw.bias", "dfw.W_h", "dbw.W_h"), gr))
    q.update({"d" + n: t.grad for n, t in head.items()})
    return q

"""
Gradients of batched log-likelihoods.

The device computes d log L / d (celerite coefficients) for B problems at once (``gf_loglike_grad``, the
reverse-mode counterpart of celerite2's ``driver.factor_rev`` / ``solve_lower_rev``), in groups under a byte cap
(:mod:`gadfly_amd.rowcall`); this module
  * restates :func:`gadfly_amd.batch.sho_coefficient_pack` in torch (float64 / complex128), so that the chain
    rule from the coefficient adjoints to (S0, w0, Q) -- exposure integration, the diagonal shift and
    ``diag_add``'s dependence on the amplitudes included -- is ONE autograd vector-Jacobian product, with no
    hand-written derivative;
  * provides :class:`LogLikelihood`, a ``torch.autograd.Function`` over a :class:`BatchedLogLikelihood`.
"""
import numpy as np
import torch

from . import _lib
from .rowcall import GroupedCall, check_pack_batch, group_plan

__all__ = ["sho_coefficient_pack_torch", "check_width", "wide_max_width", "check_pack_batch", "workspace_plan", "default_chunk_len",
           "coefficient_gradients", "parameter_vjp", "LogLikelihood", "LinearModelLogLikelihood",
           "DEFAULT_WORKSPACE_BYTES"]

#: default cap on the gradient workspace of one call (the batch is split into groups beneath it)
DEFAULT_WORKSPACE_BYTES = _lib.GF_GRAD_WORKSPACE_BYTES


def sho_coefficient_pack_torch(S0, w0, Q, delta, eps=1e-5):
    """:func:`gadfly_amd.batch.sho_coefficient_pack` on torch tensors (float64, differentiable): returns
    ``(Jr, Jc, real, comp, diag_add)`` in the engine's stacked layout, real (2, B, max(Jr, 1)), comp
    (4, B, max(Jc, 1)), diag_add (B,), with the numpy pack's values."""
    S0, w0, Q = (torch.atleast_2d(torch.as_tensor(v, dtype=torch.float64)) for v in (S0, w0, Q))
    if not (S0.shape == w0.shape == Q.shape):
        raise ValueError("dimension mismatch")
    B = S0.shape[0]
    over = (Q < 0.5).detach().cpu()
    if bool(torch.any(over != over[0])):
        raise ValueError("all problems of a batch must share the term structure "
                         "(the same terms overdamped, Q < 1/2, in every problem)")
    over = over[0].to(S0.device)
    und = ~over
    delta = torch.broadcast_to(torch.as_tensor(delta, dtype=torch.float64, device=S0.device), (B,))[:, None]
    So, wo, Qo = S0[:, over], w0[:, over], Q[:, over]
    f = torch.sqrt(torch.clamp(1.0 - 4.0 * Qo * Qo, min=eps))
    amp = 0.5 * So * wo * Qo
    ar = torch.stack([amp * (1.0 + 1.0 / f), amp * (1.0 - 1.0 / f)], dim=-1).reshape(B, -1)
    cr = torch.stack([0.5 * wo / Qo * (1.0 - f), 0.5 * wo / Qo * (1.0 + f)], dim=-1).reshape(B, -1)
    Su, wu, Qu = S0[:, und], w0[:, und], Q[:, und]
    f = torch.sqrt(torch.clamp(4.0 * Qu * Qu - 1.0, min=eps))
    a = Su * wu * Qu
    cc = 0.5 * wu / Qu
    A = torch.cat([torch.complex(ar, torch.zeros_like(ar)), torch.complex(a, -(a / f))], dim=1)
    z = torch.cat([torch.complex(cr, torch.zeros_like(cr)), torch.complex(cc, -(cc * f))], dim=1)
    zd = z * delta
    Ap = 2.0 * A * (torch.cosh(zd) - 1.0) / zd ** 2
    shift = torch.sum((2.0 * A * (zd - torch.sinh(zd)) / zd ** 2).real, dim=1)
    Jr, Jc = ar.shape[1], a.shape[1]
    zr = S0.new_zeros((B, 1))
    real = torch.stack([Ap[:, :Jr].real, z[:, :Jr].real]) if Jr else torch.stack([zr, zr])
    comp = (torch.stack([Ap[:, Jr:].real, -Ap[:, Jr:].imag, z[:, Jr:].real, -z[:, Jr:].imag]) if Jc
            else torch.stack([zr, zr, zr, zr]))
    diag_add = torch.sum(real[0, :, :Jr], dim=1) + torch.sum(comp[0, :, :Jc], dim=1) + shift
    return Jr, Jc, real, comp, diag_add


def wide_max_width():
    """The widest celerite form the wide gradient route takes (``gf_grad_wide_max_width``)."""
    return int(_lib.load().gf_grad_wide_max_width())


def check_width(W, wide=False, hint=False):
    """The gradient kernels' width limits: NotImplementedError beyond the one-wave kernel's, or with ``wide`` beyond
    the workgroup kernel's.  ``hint``: the one-wave message also names the wide route (the callers that take
    ``wide=`` ask for it)."""
    if wide:
        if W > wide_max_width():
            raise NotImplementedError(
                f"gradients take celerite widths W <= {wide_max_width()} (wide=True, one workgroup per problem); "
                f"this kernel has W = {W}")
    elif W > _lib.GF_GRAD_MAX_WIDTH:
        raise NotImplementedError(
            f"gradients take celerite widths W <= {_lib.GF_GRAD_MAX_WIDTH} (one wave per problem); this kernel "
            f"has W = {W}" + (f": pass wide=True (one workgroup per problem, W <= {wide_max_width()})" if hint else ""))


def workspace_plan(N, W, B, cap_bytes=DEFAULT_WORKSPACE_BYTES, chunk_len=None, wide=False, seg=None):
    """(doubles per problem, problems per group, number of groups) of a gradient call: the one-wave route's, or,
    with ``chunk_len``, the time-parallel route's at that chunk length, or, with ``wide``, the workgroup route's at
    ``seg`` rows per segment (None: the library's default)."""
    check_width(W, wide)
    lib = _lib.load()
    if wide:
        per = lib.gf_grad_wide_work(int(N), int(W), 0 if seg is None else int(seg))
    else:
        per = (lib.gf_grad_work(int(N), int(W)) if chunk_len is None
               else lib.gf_grad_chunked_work(int(N), int(W), int(chunk_len)))
    return group_plan(per, B, cap_bytes, f"no gradient workspace for N = {N}, W = {W}")


def default_chunk_len(B, N, W):
    """Rows per chunk of the time-parallel route for a batch of B series of N rows (``gf_grad_chunk_len``)."""
    check_width(W)
    return int(_lib.load().gf_grad_chunk_len(int(B), int(N), int(W)))


def coefficient_gradients(engine, Jr, Jc, real, comp, diag_add, cap_bytes=DEFAULT_WORKSPACE_BYTES,
                          chunk_len=None, time_parallel=False, y=None, rows=None, wide=False, seg=None):
    """Run ``gf_loglike_grad`` over an engine's data (t, y - mean, diag on the device) for stacked host
    coefficient arrays of its ORIGINAL term structure.  Returns a dict of numpy arrays: ``ll`` (B,),
    ``real`` (2, B, Jr) = d/d(a, c), ``comp`` (4, B, Jc) = d/d(a, b, c, d), ``diag_add`` (B,), ``mean`` (B,),
    ``info`` (B,), the plan (``workspace_bytes``, ``groups``, ``group_size``) and ``device_ms``, the summed
    device time of the gf_loglike_grad launches (HIP events around each).

    ``time_parallel``: the chunked route (``gf_loglike_grad_chunked``, for one long series or a few) in chunks of
    ``chunk_len`` rows (None: :func:`default_chunk_len`); the result also holds ``chunk_len`` and ``reruns``, the
    number of problems it flagged.  Those are run again through ``gf_loglike_grad``, so that log L, info and the NaN
    gradients of a matrix that is not positive definite are the one-wave route's.

    ``y``: a float64 device tensor (1 or B, N) that stands in for the engine's data (the residuals of a linear mean
    model); ``rows``: (B,) real rows per problem -- every problem is then swept on its own, over its
    real rows alone (one-wave route only), and has the bits of a call of its own.  Without them nothing changes.

    ``wide``: the workgroup route (``gf_loglike_grad_wide``) for widths up to
    :func:`wide_max_width`, narrow ones included, at ``seg`` rows per segment (None: the library's default; the
    outputs do not depend on it, to the bit).  The result also holds ``seg``.  Not together with ``time_parallel``,
    ``chunk_len`` or ``rows``."""
    W = Jr + 2 * Jc
    if wide and (time_parallel or chunk_len is not None or rows is not None):
        raise ValueError("wide=True does not combine with time_parallel, chunk_len or rows=")
    if seg is not None and (not wide or int(seg) < 1):
        raise ValueError("seg belongs to the wide route (wide=True) and is at least 1" if not wide
                         else f"seg = {seg}")
    if (Jr, Jc) != engine._struct0:
        raise ValueError("coefficient pack does not match the batch structure")
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, diag_add)
    if not time_parallel and chunk_len is not None:
        raise ValueError("chunk_len belongs to the time-parallel route (time_parallel=True)")
    name, head = "gf_loglike_grad", (N,)
    if time_parallel:
        chunk_len = default_chunk_len(B, N, W) if chunk_len is None else int(chunk_len)
        if chunk_len < 1:
            raise ValueError(f"chunk_len = {chunk_len}")
        name, head = "gf_loglike_grad_chunked", (N, min(chunk_len, N))
    if wide:
        check_width(W, True)
        seg = int(_lib.load().gf_grad_wide_seg(N, W)) if seg is None else min(int(seg), N)
        name, head = "gf_loglike_grad_wide", (N, seg)
    plan = workspace_plan(N, W, B, cap_bytes, head[1] if time_parallel else None, wide=wide, seg=seg)
    if rows is not None:
        if time_parallel:
            raise ValueError("rows= belongs to the one-wave route")
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.shape != (B,) or np.any(rows < 1) or np.any(rows > N):
            raise ValueError("dimension mismatch")
        plan = (max(workspace_plan(int(n), W, 1, cap_bytes)[0] for n in np.unique(rows)), 1, B)
    f64 = dict(dtype=torch.float64, device=engine.device)
    with torch.cuda.device(engine.device):
        rc = GroupedCall(engine, name, plan, (real, comp, diag_add), y=y)
        ll = torch.empty((B,), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device=engine.device)
        g_diag = torch.empty((B,), **f64)
        g_mean = torch.empty((B,), **f64)
        lr, lc = max(Jr, 1), max(Jc, 1)
        g_real = np.zeros((2, B, lr))
        g_comp = np.zeros((4, B, lc))

        def group(g):
            gr = torch.zeros((2, g.nb, lr), **f64)
            gc = torch.zeros((4, g.nb, lc), **f64)
            shape = head if rows is None else (int(rows[g.b0]),)
            g.launch(g.nb, *shape, Jr, Jc, *g.coef[0], *g.data, *g.work, g.at(ll), gr.data_ptr(), gc.data_ptr(),
                     g.at(g_diag), g.at(g_mean), g.at(info), g.stream)
            g_real[:, g.b0:g.b0 + g.nb] = gr.cpu().numpy()
            g_comp[:, g.b0:g.b0 + g.nb] = gc.cpu().numpy()

        events = list(rc.run(group))
        extra = dict(seg=seg) if wide else {}
        if time_parallel:
            flagged = np.flatnonzero(info.cpu().numpy() != 0)
            extra = dict(chunk_len=head[1], reruns=len(flagged))
            if len(flagged):
                # one problem per group: the one-wave kernel, whose bits do not depend on the batch around a problem
                per = workspace_plan(N, W, 1, cap_bytes)[0]
                head = (N,)
                one = GroupedCall(engine, "gf_loglike_grad", (per, 1, B), (real, comp, diag_add), y=y)
                events += one.run(group, only=flagged)
        return dict(ll=ll.cpu().numpy(), real=g_real[:, :, :Jr], comp=g_comp[:, :, :Jc],
                    diag_add=g_diag.cpu().numpy(), mean=g_mean.cpu().numpy(), info=info.cpu().numpy(),
                    device_ms=sum(a.elapsed_time(b) for a, b in events), **rc.plan, **extra)


#: terms of each kind (overdamped, underdamped) padded to a multiple of this in the chain rule's layout
_VJP_ALIGN = 8


def parameter_vjp(S0, w0, Q, delta, g_real, g_comp, g_diag_add):
    """d log L / d (S0, w0, Q), (B, J) each, from the coefficient adjoints: one vector-Jacobian product through
    :func:`sho_coefficient_pack_torch` (CPU, float64).

    A problem's result does not depend on the batch around it, to the bit: the overdamped and the underdamped terms
    are each padded with inert dummy terms to a multiple of _VJP_ALIGN per problem (every row of every intermediate
    then starts on a SIMD-vector boundary and has no tail), and the product runs on one CPU thread (no chunking of
    the rows between threads).  The thread count is torch's PROCESS-WIDE intra-op setting: other threads that run
    torch CPU work during the product run on one thread too, until it is restored.  The bit-identity rests on
    torch's CPU kernels treating equal, aligned rows alike (tested on the installed torch, not guaranteed by it)."""
    S0, w0, Q = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (S0, w0, Q))
    B, J = S0.shape
    over = Q[0] < 0.5
    io, iu = np.flatnonzero(over), np.flatnonzero(~over)
    po = -(-len(io) // _VJP_ALIGN) * _VJP_ALIGN
    pu = -(-len(iu) // _VJP_ALIGN) * _VJP_ALIGN
    cols = np.concatenate([io, np.full(po - len(io), -1), iu, np.full(pu - len(iu), -1)])
    dummy = cols < 0
    fill = np.where(np.arange(po + pu) < po, 0.25, 2.0)          # dummy Q: overdamped / underdamped side
    pad = []
    for v, d in ((S0, 1.0), (w0, 100.0), (Q, None)):
        x = np.where(dummy[None, :], d if d is not None else fill[None, :], v[:, np.where(dummy, 0, cols)])
        pad.append(np.ascontiguousarray(np.broadcast_to(x, (B, po + pu))))
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)                  # process-wide (see the docstring), restored below
    try:
        with torch.enable_grad():
            xs = [torch.tensor(x, requires_grad=True) for x in pad]
            Jr, Jc, real, comp, diag_add = sho_coefficient_pack_torch(*xs, delta)
            jr, jc = 2 * len(io), len(iu)
            gr = torch.zeros_like(real)
            gc = torch.zeros_like(comp)
            if jr:
                gr[:, :, :jr] = torch.as_tensor(np.asarray(g_real)[:, :, :jr])
            if jc:
                gc[:, :, :jc] = torch.as_tensor(np.asarray(g_comp)[:, :, :jc])
            gd = torch.as_tensor(np.asarray(g_diag_add, dtype=np.float64))
            outs, gouts = [diag_add], [gd]
            if Jr:
                outs.append(real)
                gouts.append(gr)
            if Jc:
                outs.append(comp)
                gouts.append(gc)
            grads = torch.autograd.grad(outs, xs, grad_outputs=gouts, allow_unused=True)
    finally:
        torch.set_num_threads(nthreads)
    res = []
    for g in grads:
        g = np.zeros((B, po + pu)) if g is None else g.detach().numpy()
        out = np.empty((B, J))
        out[:, cols[~dummy]] = g[:, ~dummy]
        res.append(out)
    return tuple(res)


class LogLikelihood(torch.autograd.Function):
    """``LogLikelihood.apply(S0, w0, Q, evaluator, delta[, time_parallel[, wide]])``: the (B,) log-likelihoods of a
    :class:`gadfly_amd.BatchedLogLikelihood` at (B, J) tensors of SHO hyperparameters, differentiable with
    respect to S0, w0 and Q (the device gradient of :meth:`BatchedLogLikelihood.value_and_grad`, by its
    time-parallel route where ``time_parallel`` is true, by its workgroup route for wide kernels where ``wide`` is)."""

    @staticmethod
    def forward(ctx, S0, w0, Q, evaluator, delta, time_parallel=False, wide=False):
        host = [x.detach().cpu().numpy() for x in (S0, w0, Q)]
        ll, g = evaluator.value_and_grad(*host, delta, time_parallel=bool(time_parallel), wide=bool(wide))
        ctx.save_for_backward(*(torch.as_tensor(g[k], dtype=S0.dtype, device=S0.device)
                                for k in ("S0", "w0", "Q")))
        return torch.as_tensor(ll, dtype=S0.dtype, device=S0.device)

    @staticmethod
    def backward(ctx, grad_output):
        gS0, gw0, gQ = ctx.saved_tensors
        go = grad_output[:, None]
        return go * gS0, go * gw0, go * gQ, None, None, None, None


class LinearModelLogLikelihood(torch.autograd.Function):
    """``LinearModelLogLikelihood.apply(S0, w0, Q, evaluator, basis, delta[, marginal])``: the (B,) log-likelihoods of
    the linear mean models y = A beta + eps of a :class:`gadfly_amd.BatchedLogLikelihood` at their generalised least
    squares fits -- profiled over beta, or with ``marginal`` integrated over it -- at (B, J) tensors of SHO
    hyperparameters, differentiable with respect to S0, w0 and Q
    (:meth:`BatchedLogLikelihood.linear_value_and_grad`)."""

    @staticmethod
    def forward(ctx, S0, w0, Q, evaluator, basis, delta, marginal=False):
        host = [x.detach().cpu().numpy() for x in (S0, w0, Q)]
        ll, g = evaluator.linear_value_and_grad(basis, *host, delta, marginal=bool(marginal))
        ctx.save_for_backward(*(torch.as_tensor(g[k], dtype=S0.dtype, device=S0.device)
                                for k in ("S0", "w0", "Q")))
        return torch.as_tensor(ll, dtype=S0.dtype, device=S0.device)

    @staticmethod
    def backward(ctx, grad_output):
        gS0, gw0, gQ = ctx.saved_tensors
        go = grad_output[:, None]
        return go * gS0, go * gw0, go * gQ, None, None, None, None

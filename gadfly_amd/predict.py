"""
Conditional means of batched problems.

The device computes alpha = K^-1 (y - mean), mu = y - diag alpha and, optionally, the share of the data one part of
the kernel explains for B problems at once (``gf_solve_batch``: a checkpointed forward sweep and the upper solve
backwards, no stored factor); this module stacks the component's coefficients.  ``gf_predict_batch_at`` then carries
alpha to new times t* (DESIGN.md 3.11): the two sorted-axis sums of the full kernel or of a component, no workspace.
``gf_var_batch`` is ``gf_solve_batch`` with one more backward recurrence: the inverse diagonal h, the
conditional variances at the observed times and at new ones, the staged queries counted in its workspace.
``gf_solve_batch_wide`` is ``gf_solve_batch`` without a component for kernels wider than one wave (one
workgroup per problem); their sums at new times, and a component's share, are ``gf_predict_batch_at``'s over groups of
whole terms (:func:`term_groups`).
``gf_solve_batch_rhs`` and ``gf_predict_batch_at_rhs`` are the first two for R right-hand sides per
problem through one pass over the rows, column by column the same bits.  The groups
under the byte cap, the query axes and the launches are :mod:`gadfly_amd.rowcall`'s.
"""
import numpy as np
import torch

from . import _lib
from .rowcall import GroupedCall, check_pack_batch, group_plan, query_axes

__all__ = ["check_width", "workspace_plan", "component_pack", "solve_batch", "solve_batch_wide", "term_groups",
           "predict_at", "predict_at_groups", "variance_plan",
           "variance_batch", "rhs_workspace_plan", "solve_batch_rhs", "predict_at_rhs", "DEFAULT_WORKSPACE_BYTES"]

#: default cap on the workspace of one call (the batch is split into groups beneath it)
DEFAULT_WORKSPACE_BYTES = _lib.GF_SOLVE_WORKSPACE_BYTES


def check_width(W, what="this kernel", wide=False):
    """The one-wave solve kernel's width limit: NotImplementedError beyond it.  ``wide``: the limit of the route with
    one workgroup per problem (``gf_solve_wide_max_width()``) instead."""
    if wide:
        limit = int(_lib.load().gf_solve_wide_max_width())
        if W > limit:
            raise NotImplementedError(
                f"batched conditional means with wide=True take celerite widths W <= {limit} (one workgroup per "
                f"problem); {what} has W = {W}")
        return
    if W > _lib.GF_SOLVE_MAX_WIDTH:
        raise NotImplementedError(
            f"batched conditional means take celerite widths W <= {_lib.GF_SOLVE_MAX_WIDTH} (one wave per problem); "
            f"{what} has W = {W}")


def workspace_plan(N, W, B, cap_bytes=DEFAULT_WORKSPACE_BYTES, seg=0, wide=False):
    """(doubles per problem, problems per group, number of groups) of a gf_solve_batch call -- ``wide``: of a
    gf_solve_batch_wide call."""
    check_width(W, wide=wide)
    lib = _lib.load()
    work = lib.gf_solve_wide_work if wide else lib.gf_solve_batch_work
    return group_plan(work(int(N), int(W), int(seg)), B, cap_bytes,
                      f"no solve workspace for N = {N}, W = {W}, seg = {seg}")


def component_pack(kernel, B, wide=False):
    """Stacked host coefficients (Jr', Jc', real', comp') of a component for B problems from a list of B kernels, one
    kernel for all problems, or a host pack (``sho_coefficient_pack``, ``engine._coeff_pack``) of B (or one) rows.
    ValueError when the list does not hold B kernels or they do not share one term structure; NotImplementedError
    when the component is wider than one wave -- ``wide``: than :func:`check_width` allows with ``wide``."""
    from .engine import _coeff_pack
    if isinstance(kernel, tuple) and len(kernel) >= 4 and isinstance(kernel[0], (int, np.integer)):
        Jr, Jc = int(kernel[0]), int(kernel[1])
        real, comp = np.asarray(kernel[2], dtype=np.float64), np.asarray(kernel[3], dtype=np.float64)
        if real.ndim != 3 or comp.ndim != 3 or real.shape[1] != comp.shape[1] or real.shape[1] not in (1, B):
            raise ValueError("dimension mismatch")
        if real.shape[1] == 1 and B > 1:
            real, comp = np.repeat(real, B, axis=1), np.repeat(comp, B, axis=1)
    else:
        if hasattr(kernel, "get_device_coefficients"):
            kernel = [kernel] * B
        kernel = list(kernel)
        if len(kernel) != B:
            raise ValueError(f"kernel= holds {len(kernel)} components for a batch of {B} problems")
        Jr, Jc, real, comp, _, _ = _coeff_pack([k.get_device_coefficients() for k in kernel])
    if Jr + 2 * Jc < 1:
        raise ValueError("the component has no terms")
    check_width(Jr + 2 * Jc, "the component", wide=wide)
    check_pack_batch(B, Jr, Jc, real, comp, np.zeros(B))
    return Jr, Jc, np.ascontiguousarray(real), np.ascontiguousarray(comp)


def solve_batch(engine, Jr, Jc, real, comp, diag_add, component=None, cap_bytes=DEFAULT_WORKSPACE_BYTES, seg=0,
                want_alpha=True, want_mu=True):
    """Enqueue ``gf_solve_batch`` over an engine's data (t, y - mean, diag on the device) for stacked host coefficient
    arrays of its ORIGINAL term structure; ``component`` = (Jr', Jc', real', comp') or None.  Returns a dict of
    device tensors -- ``alpha``, ``mu``, ``mu_comp`` ((B, N) each, None where not asked for), ``ll`` (B,), ``info``
    (B,) -- with the plan (``workspace_bytes``, ``groups``, ``group_size``) and ``events``, one pair of HIP events
    around each launch.  Nothing is copied back: no host synchronisation."""
    W = Jr + 2 * Jc
    if (Jr, Jc) != engine._struct0:
        raise ValueError("coefficient pack does not match the batch structure")
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, diag_add)
    plan = workspace_plan(N, W, B, cap_bytes, seg)
    jr2, jc2, real2, comp2 = (0, 0, None, None) if component is None else component
    f64 = dict(dtype=torch.float64, device=engine.device)
    with torch.cuda.device(engine.device):
        rc = GroupedCall(engine, "gf_solve_batch", plan, (real, comp, diag_add),
                         None if component is None else (real2, comp2))
        ll = torch.empty((B,), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device=engine.device)
        alpha = torch.empty((B, N), **f64) if want_alpha else None
        mu = torch.empty((B, N), **f64) if want_mu else None
        mu_comp = torch.empty((B, N), **f64) if component is not None else None
        events = rc.run(lambda g: g.launch(
            g.nb, N, Jr, Jc, *g.coef[0], jr2, jc2, *g.coef[1], *g.data, int(seg), *g.work,
            g.at(alpha, N), g.at(mu, N), g.at(mu_comp, N), g.at(ll), g.at(info), g.stream))
        return dict(alpha=alpha, mu=mu, mu_comp=mu_comp, ll=ll, info=info, events=events, **rc.plan)


def solve_batch_wide(engine, Jr, Jc, real, comp, diag_add, cap_bytes=DEFAULT_WORKSPACE_BYTES, seg=0, want_alpha=True,
                     want_mu=True):
    """:func:`solve_batch` through ``gf_solve_batch_wide``: one workgroup per problem, celerite widths
    up to ``gf_solve_wide_max_width()``, no component.  The same dict, ``mu_comp`` always None."""
    W = Jr + 2 * Jc
    if (Jr, Jc) != engine._struct0:
        raise ValueError("coefficient pack does not match the batch structure")
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, diag_add)
    plan = workspace_plan(N, W, B, cap_bytes, seg, wide=True)
    f64 = dict(dtype=torch.float64, device=engine.device)
    with torch.cuda.device(engine.device):
        rc = GroupedCall(engine, "gf_solve_batch_wide", plan, (real, comp, diag_add))
        ll = torch.empty((B,), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device=engine.device)
        alpha = torch.empty((B, N), **f64) if want_alpha else None
        mu = torch.empty((B, N), **f64) if want_mu else None
        events = rc.run(lambda g: g.launch(
            g.nb, N, Jr, Jc, *g.coef[0], *g.data, int(seg), *g.work,
            g.at(alpha, N), g.at(mu, N), g.at(ll), g.at(info), g.stream))
        return dict(alpha=alpha, mu=mu, mu_comp=None, ll=ll, info=info, events=events, **rc.plan)


def term_groups(Jr, Jc, real, comp, max_width=_lib.GF_SOLVE_MAX_WIDTH):
    """A stacked coefficient pack (real (2, B, max(Jr, 1)), comp (4, B, max(Jc, 1))) cut into consecutive groups of
    whole terms of celerite width <= ``max_width`` each, in the original order -- the real terms first, then the
    complex ones, a complex term's two columns never apart: a list of ``(Jr_g, Jc_g, real_g, comp_g)`` that
    :func:`predict_at` accepts.  K(t*, t) alpha is a sum over terms, so the groups' results add up to the whole
    kernel's.  A pack that fits comes back as one group holding the same arrays."""
    Jr, Jc = int(Jr), int(Jc)
    if Jr + 2 * Jc <= max_width:
        return [(Jr, Jc, real, comp)]
    if max_width < 2:
        raise ValueError("groups of whole terms need a width of at least 2")
    real, comp = np.asarray(real, dtype=np.float64), np.asarray(comp, dtype=np.float64)
    B = real.shape[1]
    groups, ir, ic = [], 0, 0
    while ir < Jr or ic < Jc:
        jr = min(Jr - ir, max_width)
        jc = min(Jc - ic, (max_width - jr) // 2) if ir + jr == Jr else 0
        r, c = np.zeros((2, B, max(jr, 1))), np.zeros((4, B, max(jc, 1)))
        r[:, :, :jr], c[:, :, :jc] = real[:, :, ir:ir + jr], comp[:, :, ic:ic + jc]
        groups.append((jr, jc, r, c))
        ir, ic = ir + jr, ic + jc
    return groups


def predict_at_groups(engine, groups, alpha, ts, nobs=None, nq=None):
    """:func:`predict_at` for a kernel given as :func:`term_groups`: one ``gf_predict_batch_at`` launch per group on
    the same ``alpha``, the results added on the device in group order, the events concatenated.  Returns
    dict(``mu``, ``events``) as :func:`predict_at`.  No host synchronisation."""
    if not groups:
        raise ValueError("the kernel has no terms")
    mu, events = None, []
    for g in groups:
        at = predict_at(engine, *g, alpha, ts, nobs=nobs, nq=nq)
        mu = at["mu"] if mu is None else mu.add_(at["mu"])
        events += at["events"]
    return dict(mu=mu, events=events)


def predict_at(engine, Jr, Jc, real, comp, alpha, ts, nobs=None, nq=None):
    """Enqueue ``gf_predict_batch_at`` over an engine's time axes: K*(t*, t) alpha of the B problems for stacked host
    coefficient arrays ``real`` (2, B, max(Jr, 1)), ``comp`` (4, B, max(Jc, 1)) -- the full kernel's or a component's
    -- and ``alpha`` (B, N) on the device (:func:`solve_batch`).  ``ts``: the query stamps, (M,) or (1, M) shared,
    or (B, M), ascending per problem (host array or device tensor).  ``nobs`` / ``nq``: (B,) real observed rows and
    real queries per problem, or None for N / M; result rows from ``nq[b]`` on are never written (the caller cuts them
    off).  Returns dict(``mu`` (B, M) device tensor, ``events``: one pair of HIP events around the launch).  No host
    synchronisation."""
    W = Jr + 2 * Jc
    if W < 1:
        raise ValueError("the kernel has no terms")
    check_width(W)
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, np.zeros(B))
    if tuple(alpha.shape) != (B, N) or alpha.dtype != torch.float64:
        raise ValueError(f"alpha of shape {tuple(alpha.shape)} does not hold the batch's ({B}, {N}) rows")
    dev = engine.device
    f64 = dict(dtype=torch.float64, device=dev)
    lib, p = engine.lib, _lib.ptr
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ts, M, nobs, nq = query_axes(engine, ts, nobs, nq)
        alpha = alpha.contiguous()
        mu = torch.empty((B, M), **f64)
        cr_ = torch.as_tensor(np.ascontiguousarray(real, dtype=np.float64), **f64)
        cc_ = torch.as_tensor(np.ascontiguousarray(comp, dtype=np.float64), **f64)
        t = engine.t
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = lib.gf_predict_batch_at(
            B, N, M, Jr, Jc, p(cr_[0]), p(cr_[1]), p(cc_[0]), p(cc_[1]), p(cc_[2]), p(cc_[3]),
            p(t), engine._bs(t), p(nobs), p(ts), engine._bs(ts), p(nq),
            p(alpha), N, p(mu), M, stream)
        _lib.check(st, "gf_predict_batch_at")
        e1.record()
    return dict(mu=mu, events=[(e0, e1)])


def variance_plan(N, W, B, M=0, cap_bytes=DEFAULT_WORKSPACE_BYTES, seg=0):
    """(doubles per problem, problems per group, number of groups) of a gf_var_batch call with M queries per problem:
    the solve's workspace, one slot for Y and 64 doubles per staged query (at M = N the queries dominate and the groups
    shrink)."""
    check_width(W)
    return group_plan(_lib.load().gf_var_batch_work(int(N), int(W), int(M), int(seg)), B, cap_bytes,
                      f"no variance workspace for N = {N}, W = {W}, M = {M}, seg = {seg}")


def variance_batch(engine, Jr, Jc, real, comp, diag_add, ts=None, nobs=None, nq=None,
                   cap_bytes=DEFAULT_WORKSPACE_BYTES, seg=0, want_alpha=True, want_mu=True, want_h=True,
                   want_var=True):
    """Enqueue ``gf_var_batch`` over an engine's data for stacked host coefficient arrays of its ORIGINAL term
    structure (as :func:`solve_batch`, no component).  ``ts``: query stamps (M,), (1, M) or (B, M), ascending per
    problem (host array or device tensor), or None; ``nobs`` / ``nq``: (B,) real observed rows and real queries per
    problem, or None for N / M.  Returns a dict of device tensors -- ``alpha``, ``mu``, ``hdiag``, ``var`` ((B, N)
    each, None where not asked for), ``var_at`` ((B, M), None without queries; rows from ``nq[b]`` on are never
    written), ``ll``, ``info`` (B,) -- with the plan and ``events`` as :func:`solve_batch`.  No host synchronisation."""
    W = Jr + 2 * Jc
    if (Jr, Jc) != engine._struct0:
        raise ValueError("coefficient pack does not match the batch structure")
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, diag_add)
    f64 = dict(dtype=torch.float64, device=engine.device)
    with torch.cuda.device(engine.device):
        ts, M, nobs, nq = query_axes(engine, ts, nobs, nq, empty_ok=True)
        rc = GroupedCall(engine, "gf_var_batch", variance_plan(N, W, B, M, cap_bytes, seg), (real, comp, diag_add))
        ll = torch.empty((B,), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device=engine.device)
        outs = {k: (torch.empty((B, N), **f64) if want else None) for k, want in
                (("alpha", want_alpha), ("mu", want_mu), ("hdiag", want_h), ("var", want_var))}
        var_at = torch.empty((B, M), **f64) if M else None
        qbs = 0 if ts is None else engine._bs(ts)
        events = rc.run(lambda g: g.launch(
            g.nb, N, Jr, Jc, *g.coef[0], *g.data, g.at(ts, qbs), qbs, M, g.at(nobs), g.at(nq), int(seg), *g.work,
            *(g.at(x, N) for x in outs.values()), g.at(var_at, M), g.at(ll), g.at(info), g.stream))
        return dict(ll=ll, info=info, var_at=var_at, events=events, **rc.plan, **outs)


def rhs_workspace_plan(N, W, B, R, cap_bytes=DEFAULT_WORKSPACE_BYTES, seg=0):
    """(doubles per problem, problems per group, number of groups) of a gf_solve_batch_rhs call with R right-hand
    sides per problem: every block of right-hand sides has its own checkpoints and staged rows, so R counts."""
    check_width(W)
    if int(R) < 1:
        raise ValueError("at least one right-hand side is needed")
    return group_plan(_lib.load().gf_solve_batch_rhs_work(int(N), int(W), int(R), int(seg)), B, cap_bytes,
                      f"no solve workspace for N = {N}, W = {W}, R = {R}, seg = {seg}")


def solve_batch_rhs(engine, Jr, Jc, real, comp, diag_add, y, cap_bytes=DEFAULT_WORKSPACE_BYTES, seg=0,
                    want_alpha=True, want_mu=True):
    """Enqueue ``gf_solve_batch_rhs`` over an engine's time axes and diagonal for R right-hand sides per problem:
    ``y`` a float64 device tensor (B, R, N), or (1, R, N) / (R, N) shared by all problems (the engine's own data are
    not looked at).  Coefficients as :func:`solve_batch`, no component.  Returns a dict of device tensors -- ``alpha``,
    ``mu`` ((B, R, N) each, None where not asked for), ``ll`` (B, R), ``info`` (B,) -- with the plan and ``events`` as
    :func:`solve_batch`.  Column r has the bits :func:`solve_batch` gives for ``y[:, r]`` as data.  No host
    synchronisation."""
    W = Jr + 2 * Jc
    if (Jr, Jc) != engine._struct0:
        raise ValueError("coefficient pack does not match the batch structure")
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, diag_add)
    if y.ndim == 2:
        y = y[None]
    if y.ndim != 3 or y.shape[0] not in (1, B) or y.shape[1] < 1 or y.shape[2] != N or y.dtype != torch.float64:
        raise ValueError(f"right-hand sides of shape {tuple(y.shape)} for a batch of {B} problems of {N} rows")
    R = int(y.shape[1])
    plan = rhs_workspace_plan(N, W, B, R, cap_bytes, seg)
    f64 = dict(dtype=torch.float64, device=engine.device)
    with torch.cuda.device(engine.device):
        y = y.to(engine.device).contiguous()
        ybs = 0 if y.shape[0] == 1 else R * N
        rc = GroupedCall(engine, "gf_solve_batch_rhs", plan, (real, comp, diag_add))
        ll = torch.empty((B, R), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device=engine.device)
        alpha = torch.empty((B, R, N), **f64) if want_alpha else None
        mu = torch.empty((B, R, N), **f64) if want_mu else None
        events = rc.run(lambda g: g.launch(
            g.nb, N, R, Jr, Jc, *g.coef[0], *g.data[:4], g.at(y, ybs), ybs, N, int(seg), *g.work,
            g.at(alpha, R * N), g.at(mu, R * N), R * N, N, g.at(ll, R), g.at(info), g.stream))
        return dict(alpha=alpha, mu=mu, ll=ll, info=info, events=events, **rc.plan)


def predict_at_rhs(engine, Jr, Jc, real, comp, alpha, ts, nobs=None, nq=None):
    """Enqueue ``gf_predict_batch_at_rhs``: :func:`predict_at` for ``alpha`` (B, R, N) on the device
    (:func:`solve_batch_rhs`).  Returns dict(``mu`` (B, R, M) device tensor, ``events``); rows from ``nq[b]`` on are
    never written.  Column r has the bits :func:`predict_at` gives for ``alpha[:, r]``.  No host synchronisation."""
    W = Jr + 2 * Jc
    if W < 1:
        raise ValueError("the kernel has no terms")
    check_width(W)
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, np.zeros(B))
    if alpha.ndim != 3 or alpha.shape[0] != B or alpha.shape[1] < 1 or alpha.shape[2] != N \
            or alpha.dtype != torch.float64:
        raise ValueError(f"alpha of shape {tuple(alpha.shape)} does not hold the batch's ({B}, R, {N}) rows")
    R = int(alpha.shape[1])
    dev = engine.device
    f64 = dict(dtype=torch.float64, device=dev)
    lib, p = engine.lib, _lib.ptr
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ts, M, nobs, nq = query_axes(engine, ts, nobs, nq)
        alpha = alpha.contiguous()
        mu = torch.empty((B, R, M), **f64)
        cr_ = torch.as_tensor(np.ascontiguousarray(real, dtype=np.float64), **f64)
        cc_ = torch.as_tensor(np.ascontiguousarray(comp, dtype=np.float64), **f64)
        t = engine.t
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = lib.gf_predict_batch_at_rhs(
            B, N, M, R, Jr, Jc, p(cr_[0]), p(cr_[1]), p(cc_[0]), p(cc_[1]), p(cc_[2]), p(cc_[3]),
            p(t), engine._bs(t), p(nobs), p(ts), engine._bs(ts), p(nq),
            p(alpha), R * N, N, p(mu), R * M, M, stream)
        _lib.check(st, "gf_predict_batch_at_rhs")
        e1.record()
    return dict(mu=mu, events=[(e0, e1)])

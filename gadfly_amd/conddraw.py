"""
Posterior draws of batched problems at any times: Matheron's rule, exact, no dense matrix.

For a problem with kernel K, observed stamps t (noise variances dg), data y, mean m and queries t*:

1. u = sorted union of t and t*, equal stamps merged (:func:`union_axes`);
2. w = L_u D_u^{1/2} eps, a prior draw of the NOISE-FREE process on u (``gf_sample_fused`` through
   :class:`gadfly_amd.batch.BatchedSampler` on the union axes, exact generator rows);
3. y_sim = w[obs_rows] + sqrt(dg) o eta;
4. r = (y - m) - y_sim;
5. alpha = (K + diag(dg))^-1 r on the observed axis (``gf_solve_batch_rhs``: every draw is one more right-hand side of
   a factor made once per block of draws);
6. z* = w[query_rows] + K(t*, t) alpha + m (``gf_predict_batch_at_rhs``), or at the observed stamps
   z = w[obs_rows] + (r - dg o alpha) + m, the solve's own ``mu`` output.

z* ~ N(mu*(y), K** - K*^T Sigma^-1 K*) with every cross-covariance between the queries.  The host half of this module
(:func:`union_axes` and the checks) is numpy and needs neither a GPU nor the library.
"""
from collections import namedtuple

import numpy as np

__all__ = ["UnionAxes", "union_axes", "check_exposure", "check_normals", "conditional_draws"]

#: u, obs_rows, query_rows: lists of B arrays (float64, int64, int64); nu, nobs, nq: (B,) int64 lengths of them
UnionAxes = namedtuple("UnionAxes", "u obs_rows query_rows nu nobs nq")


def _series(x, cnt, B, what):
    """B 1-D float64 series from (S,), (1, S), (B, S) or a list of B arrays, cut to ``cnt[b]`` where given."""
    if isinstance(x, (list, tuple)) or (isinstance(x, np.ndarray) and x.dtype == object):
        out = [np.ascontiguousarray(v, dtype=np.float64) for v in x]
        if len(out) == 1 and B > 1:
            out = out * B
    else:
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x[None, :]
        if x.ndim != 2:
            raise ValueError(f"{what} of shape {x.shape}: expected (S,), (B, S) or a list of series")
        out = [x[0]] * B if x.shape[0] == 1 else list(x)
    if len(out) != B or any(v.ndim != 1 for v in out):
        raise ValueError(f"{what} hold {len(out)} series for a batch of {B} problems")
    if cnt is not None:
        cnt = np.asarray(cnt, dtype=np.int64)
        if cnt.shape != (B,) or np.any(cnt < 0) or any(c > len(v) for c, v in zip(cnt, out)):
            raise ValueError("dimension mismatch")
        out = [v[:int(c)] for v, c in zip(out, cnt)]
    return out


def _batch_of(x):
    if x is None:
        return 1
    if isinstance(x, (list, tuple)) or (isinstance(x, np.ndarray) and x.dtype == object):
        return len(x)
    x = np.asarray(x)
    return x.shape[0] if x.ndim == 2 else 1


def union_axes(t, ts, nobs=None, nq=None):
    """The union axes of B problems: ``t`` observed stamps ((N,) shared, (B, N) or a list of B series), ``ts`` queries
    in the same forms or None (no queries); ``nobs`` / ``nq``: (B,) real rows of rectangular arrays, or None.  Both
    ascending per problem (``ValueError`` otherwise).  Returns :class:`UnionAxes`: per problem the sorted union ``u``
    with equal stamps merged -- a query that coincides with an observed stamp shares its row, and so do two equal
    stamps of one axis --, ``obs_rows`` (u[obs_rows] = t) and ``query_rows`` (u[query_rows] = t*), and the lengths
    ``nu``, ``nobs``, ``nq``.  Host numpy only."""
    B = max(_batch_of(t), _batch_of(ts), 1 if nobs is None else len(nobs), 1 if nq is None else len(nq))
    obs = _series(t, nobs, B, "observed stamps")
    qs = [np.zeros(0)] * B if ts is None else _series(ts, nq, B, "query times")
    u, orow, qrow = [], [], []
    for a, q in zip(obs, qs):
        if np.any(np.diff(a) < 0.0) or np.any(np.diff(q) < 0.0):
            raise ValueError("The input coordinates must be sorted")
        if not (np.all(np.isfinite(a)) and np.all(np.isfinite(q))):
            raise ValueError("time stamps must be finite")
        ub, inv = np.unique(np.concatenate([a, q]), return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
        u.append(ub)
        orow.append(inv[:len(a)])
        qrow.append(inv[len(a):])
    lens = lambda xs: np.array([len(x) for x in xs], dtype=np.int64)      # noqa: E731
    return UnionAxes(u, orow, qrow, lens(u), lens(obs), lens(qs))


def check_exposure(ax, deltas):
    """ValueError naming the first offending pair when, for a problem whose kernel is exposure-integrated (``deltas[b]``
    > 0), a query lies closer than the exposure time to a DIFFERENT observed stamp or to another query -- by the rule
    and slack of ``batch._exposure_resolved``: the union axis would leave the coefficient form's domain and its matrix
    need not be positive definite.  Coincident stamps are merged rows and are fine; so are pairs of observed stamps
    (the caller's own axis)."""
    from .batch import EXPOSURE_SLACK
    deltas = np.broadcast_to(np.asarray(deltas, dtype=np.float64), (len(ax.u),))
    for b, (u, orow, delta) in enumerate(zip(ax.u, ax.obs_rows, deltas)):
        if not delta > 0.0 or len(u) < 2:
            continue
        is_obs = np.zeros(len(u), dtype=bool)
        is_obs[orow] = True
        tol = max(1e-9 * delta, 4.0 * float(np.spacing(np.max(np.abs(u)))))
        close = (np.diff(u) < (1.0 - EXPOSURE_SLACK) * delta - tol) & ~(is_obs[:-1] & is_obs[1:])
        if np.any(close):
            i = int(np.argmax(close))
            kind = lambda k: "observed stamp" if is_obs[k] else "query"      # noqa: E731
            raise ValueError(
                f"problem {b}: {kind(i)} {float(u[i])!r} and {kind(i + 1)} {float(u[i + 1])!r} are "
                f"{u[i + 1] - u[i]:.6g} apart, closer than the exposure time {delta:.6g} of its exposure-integrated "
                f"kernel: the union axis leaves the domain of the kernel's coefficient form (move the query onto the "
                f"stamp or away from it)")


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))


def check_normals(normals, ax, size):
    """``normals=(eps, eta)`` against the shapes :func:`union_axes` reports: arrays (B, size, Nu) and (B, size, N)
    ((B, Nu), (B, N) without ``size``) when every problem has the same lengths, or lists of B arrays (size, nu_b) and
    (size, nobs_b).  ValueError otherwise."""
    if not isinstance(normals, (tuple, list)) or len(normals) != 2:
        raise ValueError("normals must be the pair (eps, eta)")
    B = len(ax.u)
    for x, lens, name in ((normals[0], ax.nu, "eps"), (normals[1], ax.nobs, "eta")):
        if isinstance(x, (list, tuple)):
            want = [((int(n),) if size is None else (int(size), int(n))) for n in lens]
            got = [_shape(v) for v in x]
        else:
            if len(set(int(n) for n in lens)) != 1:
                raise ValueError(f"normals: {name} must be a list of {B} arrays for a ragged layout (lengths "
                                 f"{[int(n) for n in lens]})")
            want = (B, int(lens[0])) if size is None else (B, int(size), int(lens[0]))
            got = _shape(x)
        if got != want:
            raise ValueError(f"normals: {name} of shape {got}, expected {want}")


class _PackKernel:
    """One row of a stacked host coefficient pack with a kernel's ``get_device_coefficients``."""

    def __init__(self, Jr, Jc, real, comp, diag_add, b):
        ar, cr = real[0, b, :Jr], real[1, b, :Jr]
        ac, bc, cc, dc = (comp[i, b, :Jc] for i in range(4))
        self._co = (ar, cr, ac, bc, cc, dc, float(diag_add[b] - np.sum(ar) - np.sum(ac)))

    def get_device_coefficients(self):
        return self._co


def _decay_rates(Jr, Jc, real, comp):
    B = real.shape[1]
    c = np.zeros((B, Jr + 2 * Jc))
    c[:, :Jr] = real[1, :, :Jr]
    c[:, Jr::2] = comp[2, :, :Jc]
    c[:, Jr + 1::2] = comp[2, :, :Jc]
    return c


def _pad_rows(rows, width, fill=0):
    out = np.full((len(rows), max(int(width), 1)), fill, dtype=np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def _stack_normals(torch, x, lens, R, width, f64):
    """(B, R, width) device tensor of a normals array or list, zero beyond each problem's length."""
    B = len(lens)
    if not isinstance(x, (list, tuple)):
        return torch.as_tensor(x).to(**f64).reshape(B, R, int(lens[0]))
    out = torch.zeros((B, R, max(int(width), 1)), **f64)
    for b, (v, n) in enumerate(zip(x, lens)):
        out[b, :, :int(n)] = torch.as_tensor(v).to(**f64).reshape(R, int(n))
    return out


def conditional_draws(bll, pack, t_obs, ts, nq, deltas, size, normals, seed, mean_at, include_mean):
    """Steps 2-6 enqueued for a :class:`gadfly_amd.batch.BatchedLogLikelihood` ``bll``.

    ``pack``: host coefficients (Jr, Jc, real, comp, diag_add) of its term structure; ``t_obs``: its observed stamps
    on the host, a list of B series (real rows only); ``ts`` (1 or B, M) host array of queries with ``nq`` (B,) or
    None, or None for draws at the observed stamps; ``deltas``: exposure times per problem (0: none) or None where
    unknown; ``mean_at``: the scalar / (B, 1) mean added at queries or None.  Every check happens before anything is
    enqueued.  Returns (z (B, R, M or N) device tensor, info (B,) int32 device tensor of the union-axis factor, the
    solve's result dict, events dict)."""
    from .batch import BatchedSampler
    from .predict import check_width, predict_at_rhs, solve_batch_rhs
    Jr, Jc, real, comp, diag_add = pack
    eng = bll.engine
    torch = eng.torch
    B, N = eng.B, eng.N
    check_width(Jr + 2 * Jc)
    R = 1 if size is None else int(size)
    if R < 1:
        raise ValueError("size must be a positive number of draws")
    M = 0 if ts is None else int(ts.shape[1])
    # the union axes, their row maps on the device and the union-axis sampler: made once per set of queries (the
    # sampler's buffers and the B sorts are the expensive part), new coefficients per call
    key = (None if ts is None else hash(ts.tobytes()), None if nq is None else tuple(int(n) for n in nq), M)
    cache = bll.__dict__.setdefault("_cond_cache", {})
    if key not in cache:
        shared = bll.rows is None and eng.t.shape[0] == 1 and (ts is None or (ts.shape[0] == 1 and nq is None))
        if shared:                          # one axis for all problems: one union
            a1 = union_axes(t_obs[0], None if ts is None else ts[0])
            ax = UnionAxes(*([x[0]] * B for x in a1[:3]), *(np.repeat(x, B) for x in a1[3:]))
        else:
            qs = None if ts is None else [ts[b if ts.shape[0] > 1 else 0, :(M if nq is None else int(nq[b]))]
                                          for b in range(B)]
            ax = union_axes(t_obs, qs)
        cache.clear()
        cache[key] = dict(ax=ax, shared=shared)
    ent = cache[key]
    ax = ent["ax"]
    if deltas is not None:
        check_exposure(ax, deltas)
    if normals is not None:
        check_normals(normals, ax, size)
    nu_max = int(ax.nu.max())
    f64 = dict(dtype=torch.float64, device=eng.device)
    rect = len(set(int(n) for n in ax.nu)) == 1
    if "sampler" not in ent:
        shims = [_PackKernel(Jr, Jc, real, comp, diag_add, b) for b in range(B)]
        axes = ax.u[0] if ent["shared"] else (np.stack(ax.u) if rect else list(ax.u))
        ent["sampler"] = BatchedSampler(shims, axes, device=eng.device)
        rows = lambda r, n: _pad_rows(r[:1] if ent["shared"] else r, n)      # noqa: E731
        ent["obs_idx"] = torch.as_tensor(rows(ax.obs_rows, N), device=eng.device)
        ent["q_idx"] = torch.as_tensor(rows(ax.query_rows, M), device=eng.device)
    sampler = ent["sampler"]
    seng = sampler.engine
    events = {}

    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        events[name] = [(e0, e1)]
        e0.record()
        return e1

    with torch.cuda.device(eng.device):
        seng.use_coefficients(seng.pack_arrays(Jr, Jc, real, comp, diag_add, _decay_rates(Jr, Jc, real, comp)))
        if normals is None:
            gen = None
            if seed is not None:
                gen = torch.Generator(device=eng.device)
                gen.manual_seed(int(seed))
            eps = torch.randn((B, R, nu_max), generator=gen, **f64)
            eta = torch.randn((B, R, N), generator=gen, **f64)
        else:
            eps = _stack_normals(torch, normals[0], ax.nu, R, nu_max, f64)
            eta = _stack_normals(torch, normals[1], ax.nobs, R, N, f64)
        done = timed("sweeps")
        w = sampler.sample_device(size=R, normals=eps if rect else [eps[b, :, :int(n)] for b, n in enumerate(ax.nu)],
                                  include_mean=False, center=False)
        if not rect:
            wl, w = w, torch.zeros((B, R, nu_max), **f64)
            for b, x in enumerate(wl):
                w[b, :, :x.shape[-1]] = x
        done.record()
        info = sampler._info

        done = timed("assembly")
        obs_idx = ent["obs_idx"][:, None, :].expand(B, R, N)
        w_obs = torch.gather(w, 2, obs_idx)
        y = eng.y.reshape(-1, N)[:, None, :]
        r = y - w_obs
        if eng.diag is not None:
            r -= torch.sqrt(eng.diag.reshape(-1, N))[:, None, :] * eta
        real_rows = None
        if bll.rows is not None:
            real_rows = (torch.arange(N, device=eng.device)[None, :]
                         < torch.as_tensor(ax.nobs, device=eng.device)[:, None])[:, None, :]
            r = torch.where(real_rows, r, torch.zeros((), **f64))
        done.record()

        res = solve_batch_rhs(eng, Jr, Jc, real, comp, diag_add, r, bll.predict_workspace_bytes,
                              want_alpha=ts is not None, want_mu=ts is None)
        events["solve"] = res["events"]
        events["at"] = []
        if ts is None:
            done = timed("assembly2")
            z = w_obs + res["mu"]
            if real_rows is not None:
                z = torch.where(real_rows, z, torch.zeros((), **f64))
            done.record()
        elif M == 0:
            z = torch.empty((B, R, 0), **f64)
        else:
            at = predict_at_rhs(eng, Jr, Jc, real, comp, res["alpha"], ts, nobs=bll.rows, nq=nq)
            events["at"] = at["events"]
            done = timed("assembly2")
            q_idx = ent["q_idx"][:, None, :].expand(B, R, M)
            z = torch.gather(w, 2, q_idx)
            if nq is None:
                z += at["mu"]
            else:               # (rows from nq[b] on are never written by the launch)
                live = (torch.arange(M, device=eng.device)[None, :]
                        < torch.as_tensor(ax.nq, device=eng.device)[:, None])[:, None, :]
                z = torch.where(live, z + at["mu"], torch.zeros((), **f64))
            if mean_at is not None:
                m = torch.as_tensor(np.array(mean_at, dtype=np.float64), **f64)
                z += m if m.ndim == 0 else m.reshape(B, 1, 1)
            done.record()
        events["assembly"] = events["assembly"] + events.pop("assembly2", [])
        if ts is None and include_mean and np.any(bll._mean != 0.0):
            m = bll._mean[:, None] if bll.rows is not None else bll._mean
            m = np.array(np.broadcast_to(m, np.broadcast_shapes(np.shape(m), (1, 1))), dtype=np.float64)
            z += torch.as_tensor(m, **f64)[:, None, :]
    return z, info, res, events

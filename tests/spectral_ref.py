"""Numpy oracle of the spectral likelihoods: the model spectrum S, the Whittle and chi-square
log-likelihoods and their analytic gradients, for B problems, in float64 or in ``np.longdouble`` (the truth the device
is held against).  Every sum comes with its SCALE: the same sum with each addend replaced by a bound of its absolute
value built from the absolute values of its parts --

    whittle  l:      n (1 + |ln S| + |P| / S)            gradients: n (1 / S + |P| / S^2) |dS/dtheta|
    chi2     l:      1/2 ((|P| + S) / e)^2               gradients: ((|P| + S) / e^2) |dS/dtheta|

with |dS/dw0| = sinc^2 sum-free per term: term (4 / w0 + (|4 w0 x| + 2 w^2 w0 / Q^2) / D), the bracket's parts taken
termwise in absolute value.  A rounding error of a few units in the last place per operation shows up as that many u
times the scale, whatever cancels in the sum itself.
"""
import numpy as np


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def _terms(S0, w0, Q, delta, omega, dtype):
    """Per problem: sinc^2 (M,), and (J, M) arrays x, D, term (without sinc^2)."""
    S0, w0, Q, omega = (np.asarray(v, dtype=np.float64).astype(dtype) for v in (S0, w0, Q, omega))
    delta = dtype(delta)
    arg = delta * omega / 2
    safe = np.where(arg == 0, dtype(1), arg)
    sinc = np.where(arg == 0, dtype(1), np.sin(safe) / safe)
    w = omega[None, :]
    a0, aw, aq = S0[:, None], w0[:, None], Q[:, None]
    x = (w - aw) * (w + aw)
    D = x * x + w * w * aw * aw / (aq * aq)
    unit = np.sqrt(dtype(2) / _pi(dtype)) * aw ** 4 / D           # dterm/dS0
    return sinc * sinc, w, a0, aw, aq, x, D, unit


def model(S0, w0, Q, delta, floor, omega, dtype=np.longdouble):
    """(B, M) model spectra; S0, w0, Q (B, J), delta, floor (B,) (floor None = 0)."""
    S0, w0, Q = (np.atleast_2d(v) for v in (S0, w0, Q))
    B = S0.shape[0]
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), (B,))
    floor = np.zeros(B) if floor is None else np.broadcast_to(np.asarray(floor, dtype=np.float64), (B,))
    out = []
    for b in range(B):
        s2, _, a0, _, _, _, _, unit = _terms(S0[b], w0[b], Q[b], delta[b], omega, dtype)
        out.append(s2 * np.sum(a0 * unit, axis=0) + dtype(floor[b]))
    return np.array(out)


def likelihood(objective, S0, w0, Q, delta, floor, omega, power, weight=None, dtype=np.longdouble):
    """The oracle of ``gf_spectral_like``.  ``power`` (M,) or (B, M); ``weight`` None (whittle: 1), (M,) or (B, M).
    Returns a dict: ``ll`` (B,), ``used`` (B,), ``info`` (B,), ``model`` (B, M), ``g`` = {S0, w0, Q: (B, J),
    floor: (B,)}, and the scales ``ll_scale`` (B,), ``g_scale`` (same keys and shapes as ``g``)."""
    assert objective in ("whittle", "chi2")
    S0, w0, Q = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (S0, w0, Q))
    B, J = S0.shape
    M = len(omega)
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), (B,))
    floor = np.zeros(B) if floor is None else np.broadcast_to(np.asarray(floor, dtype=np.float64), (B,))
    power = np.broadcast_to(np.asarray(power, dtype=np.float64), (B, M))
    weight = np.ones((B, M)) if weight is None else np.broadcast_to(np.asarray(weight, dtype=np.float64), (B, M))
    res = dict(ll=np.zeros(B, dtype=dtype), ll_scale=np.zeros(B, dtype=dtype), used=np.zeros(B, dtype=np.int64),
               info=np.zeros(B, dtype=np.int64), model=np.zeros((B, M), dtype=dtype),
               g={k: np.zeros((B, J), dtype=dtype) for k in ("S0", "w0", "Q")},
               g_scale={k: np.zeros((B, J), dtype=dtype) for k in ("S0", "w0", "Q")})
    res["g"]["floor"] = np.zeros(B, dtype=dtype)
    res["g_scale"]["floor"] = np.zeros(B, dtype=dtype)
    for b in range(B):
        s2, w, a0, aw, aq, x, D, unit = _terms(S0[b], w0[b], Q[b], delta[b], omega, dtype)
        term = a0 * unit
        S = s2 * np.sum(term, axis=0) + dtype(floor[b])
        res["model"][b] = S
        use = np.isfinite(power[b]) & np.isfinite(weight[b]) & (weight[b] > 0)
        res["used"][b] = np.count_nonzero(use)
        badk = np.flatnonzero(use & ~(S > 0))
        if len(badk):
            res["info"][b] = badk[0] + 1
            res["ll"][b] = -np.inf
            res["ll_scale"][b] = np.inf
            for k in res["g"]:
                res["g"][k][b] = np.nan
                res["g_scale"][k][b] = np.nan
            continue
        P, n, Su = power[b][use].astype(dtype), weight[b][use].astype(dtype), S[use]
        if objective == "whittle":
            res["ll"][b] = -np.sum(n * (np.log(Su) + P / Su))
            res["ll_scale"][b] = np.sum(n * (1 + np.abs(np.log(Su)) + np.abs(P) / Su))
            g = -n * (1 / Su - P / Su ** 2)
            ga = n * (1 / Su + np.abs(P) / Su ** 2)
        else:
            res["ll"][b] = -np.sum(((P - Su) / n) ** 2) / 2
            res["ll_scale"][b] = np.sum(((np.abs(P) + Su) / n) ** 2) / 2
            g = (P - Su) / n ** 2
            ga = (np.abs(P) + Su) / n ** 2
        h, ha = (g * s2[use])[None, :], (ga * s2[use])[None, :]
        xu, Du, wu, tu, uu = x[:, use], D[:, use], w[:, use], term[:, use], unit[:, use]
        dQ = tu * (2 * wu ** 2 * aw ** 2 / aq ** 3) / Du
        dw = tu * (4 / aw + (4 * aw * xu - 2 * wu ** 2 * aw / aq ** 2) / Du)
        dwa = tu * (4 / aw + (np.abs(4 * aw * xu) + 2 * wu ** 2 * aw / aq ** 2) / Du)
        for key, d, da in (("S0", uu, uu), ("Q", dQ, dQ), ("w0", dw, dwa)):
            res["g"][key][b] = np.sum(h * d, axis=1)
            res["g_scale"][key][b] = np.sum(ha * da, axis=1)
        res["g"]["floor"][b] = np.sum(g)
        res["g_scale"]["floor"][b] = np.sum(ga)
    return res

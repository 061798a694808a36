"""Numpy oracle of the spectral Fisher information, built on tests/spectral_ref.py: the Jacobian of
the model spectrum, the weighted Gram matrix

    F = sum_k v_k grad S(w_k) grad S(w_k)^T,      v_k = n_k / S_k^2 (whittle),  v_k = 1 / e_k^2 (chi2)

over the used frequencies in float64 or ``np.longdouble`` (the truth the device is held against), with the SCALE of
every entry -- sum_k v_k |d_i S_k| |d_j S_k|, the w0 bracket's parts taken termwise in absolute value as spectral_ref
does -- and a float64 restatement of the damped Fisher scoring ``SpectralLikelihood.fit`` runs, on the oracle's values.
Parameter order: S0_0 .. S0_{J-1}, w0_0 .., Q_0 .., floor.
"""
import numpy as np

from tests import spectral_ref as ref


def jacobian(S0, w0, Q, delta, omega, dtype=np.longdouble, absolute=False):
    """(P, M) Jacobian of ONE problem's model spectrum (S0, w0, Q of shape (J,)), P = 3 J + 1; ``absolute``: the bound
    of its absolute value the scales are built from."""
    s2, w, a0, aw, aq, x, D, unit = ref._terms(S0, w0, Q, delta, omega, dtype)
    term = a0 * unit
    dS0 = s2 * unit
    dQ = s2 * term * (2 * w ** 2 * aw ** 2 / aq ** 3) / D
    if absolute:
        dw = s2 * term * (4 / aw + (np.abs(4 * aw * x) + 2 * w ** 2 * aw / aq ** 2) / D)
    else:
        dw = s2 * term * (4 / aw + (4 * aw * x - 2 * w ** 2 * aw / aq ** 2) / D)
    return np.concatenate([dS0, dw, dQ, np.ones((1, len(omega)), dtype=dtype)], axis=0)


def fisher(objective, S0, w0, Q, delta, floor, omega, power, weight=None, dtype=np.longdouble):
    """The oracle of ``gf_spectral_fisher``: arguments as ``spectral_ref.likelihood``.  Returns ``(F, scale, used,
    info)``: (B, P, P), (B, P, P), (B,), (B,); a problem whose model is not positive at a used frequency is NaN."""
    assert objective in ("whittle", "chi2")
    S0, w0, Q = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (S0, w0, Q))
    B, J = S0.shape
    M, P = len(omega), 3 * J + 1
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), (B,))
    floor = np.zeros(B) if floor is None else np.broadcast_to(np.asarray(floor, dtype=np.float64), (B,))
    power = np.broadcast_to(np.asarray(power, dtype=np.float64), (B, M))
    weight = np.ones((B, M)) if weight is None else np.broadcast_to(np.asarray(weight, dtype=np.float64), (B, M))
    F = np.zeros((B, P, P), dtype=dtype)
    scale = np.zeros((B, P, P), dtype=dtype)
    used, info = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        use = np.isfinite(power[b]) & np.isfinite(weight[b]) & (weight[b] > 0)
        used[b] = np.count_nonzero(use)
        om = np.asarray(omega, dtype=np.float64)[use]
        A = jacobian(S0[b], w0[b], Q[b], delta[b], om, dtype)
        S = A[:J].T @ S0[b].astype(dtype) + dtype(floor[b]) if len(om) else np.zeros(0, dtype=dtype)
        bad = np.flatnonzero(~(S > 0))
        if len(bad):
            info[b] = np.flatnonzero(use)[bad[0]] + 1
            F[b] = np.nan
            scale[b] = np.nan
            continue
        n = weight[b][use].astype(dtype)
        v = n / S ** 2 if objective == "whittle" else 1 / n ** 2
        Aa = jacobian(S0[b], w0[b], Q[b], delta[b], om, dtype, absolute=True)
        F[b] = (A * v) @ A.T
        scale[b] = (Aa * v) @ Aa.T
    return F, scale, used, info


def _value_and_gradient(objective, th, J, delta, omega, power, weight):
    o = ref.likelihood(objective, th[:J], th[J:2 * J], th[2 * J:3 * J], delta, [th[-1]], omega, power, weight,
                       dtype=np.float64)
    g = np.concatenate([o["g"]["S0"][0], o["g"]["w0"][0], o["g"]["Q"][0], o["g"]["floor"]])
    return float(o["ll"][0]), g.astype(np.float64)


def lm_fit(objective, theta0, delta, omega, power, weight=None, max_iter=100, xtol=1e-10, damping=1e-3, max_step=1.0):
    """The iteration of ``SpectralLikelihood.fit`` for ONE problem with every parameter free, in float64 on the oracle's
    values.  ``theta0``: (3 J + 1,) in the canonical order.  Returns ``(theta, iterations, converged, g_u)``, g_u the
    gradient with respect to ln theta at the result."""
    theta0 = np.asarray(theta0, dtype=np.float64)
    J = (len(theta0) - 1) // 3
    u, lam = np.log(theta0), float(damping)
    ll, g = _value_and_gradient(objective, np.exp(u), J, delta, omega, power, weight)
    for it in range(max_iter):
        th = np.exp(u)
        F = fisher(objective, th[:J], th[J:2 * J], th[2 * J:3 * J], delta, th[-1], omega, power, weight,
                   dtype=np.float64)[0][0]
        Fu, gu = F * th[:, None] * th[None, :], g * th
        d = np.linalg.solve(Fu + lam * np.diag(np.diag(Fu)), gu)
        d = d * min(1.0, max_step / np.max(np.abs(d)))
        ll2, g2 = _value_and_gradient(objective, np.exp(u + d), J, delta, omega, power, weight)
        if np.isfinite(ll2) and ll2 >= ll:
            u, ll, g, lam = u + d, ll2, g2, max(lam / 10, 1e-9)
            if np.max(np.abs(d)) < xtol:
                return np.exp(u), it + 1, True, g * np.exp(u)
        else:
            lam = min(lam * 10, 1e9)
    return np.exp(u), max_iter, False, g * np.exp(u)


# ---- the fit cases tests/test_spectral_fisher_host.py and tests/test_gpu_spectral_fisher.py share --------------------
DT = 60.0e-6                         # one-minute cadence in 1/uHz
NYQUIST = 0.5 / DT                   # uHz
FIT_TRUTH = np.array([3.0, 0.4, 2 * np.pi * 0.08 * NYQUIST, 2 * np.pi * 0.45 * NYQUIST, 0.7, 6.0, 0.05])
#: (M, objective, noisy, seed): exact data once, noisy data for the seeds 0-5, at both sizes and objectives -- 28 cases
FIT_CASES = [(M, objective, noisy, seed) for M in (64, 256) for objective in ("whittle", "chi2")
             for noisy in (False, True) for seed in (range(6) if noisy else (0,))]


def fit_case(M, objective, noisy, seed):
    """J = 2 terms plus floor on the frequencies (k + 1) Nyquist / M, exposure = the cadence.  whittle: P = S Gamma(16,
    1/16) with weights 16; chi2: P = S (1 + 0.1 N(0, 1)) with e = 0.1 S; P = S where not ``noisy``.  The start is the
    truth x (1.3, 1/1.3, 1.3, ...) alternating over the canonical order."""
    freq = (np.arange(M) + 1) * (NYQUIST / M)
    omega = 2 * np.pi * freq
    th = FIT_TRUTH
    S = ref.model(th[0:2], th[2:4], th[4:6], DT, [th[6]], omega, np.float64)[0]
    rng = np.random.default_rng(seed)
    if objective == "whittle":
        power = S * rng.gamma(16, 1 / 16, size=S.shape) if noisy else S.copy()
        weight = np.full_like(S, 16.0)
    else:
        power = S * (1 + 0.1 * rng.normal(size=S.shape)) if noisy else S.copy()
        weight = 0.1 * S
    start = th * np.where(np.arange(7) % 2 == 0, 1.3, 1 / 1.3)
    return dict(freq=freq, omega=omega, power=power, weight=weight, truth=th.copy(), start=start, objective=objective,
                noisy=noisy)


_FITS = {}


def reference_fit(case):
    """``lm_fit`` of a case of FIT_CASES from its start, computed once per session."""
    if case not in _FITS:
        c = fit_case(*case)
        _FITS[case] = lm_fit(c["objective"], c["start"], DT, c["omega"], c["power"], c["weight"])
    return _FITS[case]

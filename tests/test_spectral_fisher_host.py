"""CPU: the oracle of the spectral Fisher information (tests/spectral_fisher_ref.py) against central differences -- its
Jacobian against differences of the model, the matrix against minus the differenced gradient where P = S --, its
restatement of the fit on every fit case, the bound C entry points and the host-side ValueErrors of
``SpectralLikelihood.fisher`` / ``covariance`` / ``fit``."""
import numpy as np
import pytest

import gadfly_amd
from gadfly_amd import _lib, spectral
from gadfly_amd.psd import PowerSpectrum
from tests import spectral_fisher_ref as fref
from tests import spectral_ref as ref

DT = fref.DT
OBJECTIVES = ("whittle", "chi2")


def _lbfgs_problem(objective, N=512):
    """test_lbfgs_step's three terms plus floor (tests/test_gpu_spectral.py) at N samples, with P = S."""
    freq = np.fft.rfftfreq(N, DT)[1:]
    S0, w0, Q, floor = np.array([40.0, 0.5, 0.02]), np.array([60.0, 2500.0, 19000.0]), np.array([0.6, 0.6, 8.0]), 0.02
    omega = 2 * np.pi * freq
    S = ref.model(S0, w0, Q, DT, [floor], omega, np.float64)[0]
    weight = np.ones_like(S) if objective == "whittle" else 0.1 * S
    return omega, S.copy(), weight, np.concatenate([S0, w0, Q, [floor]])


def test_jacobian_matches_central_differences_of_the_model():
    """Relative step 1e-6 in longdouble: the remainder is 1e-12 x the third derivative's size; bar 1e-8 of the row's
    maximum (measured 2.8e-10)."""
    ld = np.longdouble
    omega, _, _, th = _lbfgs_problem("whittle")
    J = 3
    A = fref.jacobian(th[:J], th[J:2 * J], th[2 * J:3 * J], DT, omega)
    assert A.shape == (3 * J + 1, len(omega)) and A.dtype == ld

    def model_at(t):
        # (longdouble parameters straight into the oracle's internals: no rounding of the shifted value to float64)
        s2, _, a0, _, _, _, _, unit = _terms_longdouble(t[:J], t[J:2 * J], t[2 * J:3 * J], DT, omega)
        return s2 * np.sum(a0 * unit, axis=0) + t[-1]

    worst = 0.0
    for i in range(len(th)):
        h = ld(1e-6) * ld(th[i])
        tp, tm = th.astype(ld), th.astype(ld)
        tp[i] += h
        tm[i] -= h
        fd = (model_at(tp) - model_at(tm)) / (2 * h)
        worst = max(worst, float(np.max(np.abs(fd - A[i])) / np.max(np.abs(A[i]))))
    print(f"Jacobian against central differences: worst error / row maximum {worst:.2e}")
    assert worst <= 1e-8


def _terms_longdouble(S0, w0, Q, delta, omega):
    """spectral_ref._terms at longdouble parameters (it rounds its inputs to float64 first)."""
    ld = np.longdouble
    omega = np.asarray(omega, dtype=np.float64).astype(ld)
    arg = ld(delta) * omega / 2
    safe = np.where(arg == 0, ld(1), arg)
    sinc = np.where(arg == 0, ld(1), np.sin(safe) / safe)
    w = omega[None, :]
    a0, aw, aq = S0[:, None], w0[:, None], Q[:, None]
    x = (w - aw) * (w + aw)
    D = x * x + w * w * aw * aw / (aq * aq)
    unit = np.sqrt(ld(2) / (4 * np.arctan(ld(1)))) * aw ** 4 / D
    return sinc * sinc, w, a0, aw, aq, x, D, unit


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_fisher_is_minus_the_hessian_where_the_data_equal_the_model(objective):
    """Central differences (relative step 1e-4) of the oracle's longdouble gradient: measured 1.5e-6 x scale; bar
    1e-4 x scale.  A wrong factor anywhere in the derivatives shows as O(1)."""
    omega, P, weight, th = _lbfgs_problem(objective)
    J = 3
    F, scale, used, info = fref.fisher(objective, th[:J], th[J:2 * J], th[2 * J:3 * J], DT, th[-1], omega, P, weight)
    assert used[0] == len(omega) and info[0] == 0

    def gradient(t):
        o = ref.likelihood(objective, t[:J], t[J:2 * J], t[2 * J:3 * J], DT, [t[-1]], omega, P, weight)
        return np.concatenate([o["g"]["S0"][0], o["g"]["w0"][0], o["g"]["Q"][0], o["g"]["floor"]])

    H = np.zeros_like(F[0])
    for i in range(len(th)):
        tp, tm = th.copy(), th.copy()
        tp[i] *= 1 + 1e-4
        tm[i] *= 1 - 1e-4
        H[i] = -(gradient(tp) - gradient(tm)) / np.longdouble(tp[i] - tm[i])
    worst = float(np.max(np.abs(F[0] - H) / scale[0]))
    print(f"{objective}: |F - (-Hessian)| / scale at P = S: {worst:.2e}")
    assert worst <= 1e-4
    assert float(np.max(np.abs(F[0] - F[0].T) / scale[0])) <= 1e-17


@pytest.mark.parametrize("case", fref.FIT_CASES, ids=lambda c: f"{c[1]}-M{c[0]}-{'noisy' if c[2] else 'exact'}-{c[3]}")
def test_restated_fit_converges_on_every_fit_case(case):
    """At most 40 iterations measured over the 28 cases; the cap is 60.  Exact data: the truth to 1e-9."""
    theta, iterations, converged, gu = fref.reference_fit(case)
    c = fref.fit_case(*case)
    print(f"{case}: {iterations} iterations, |g_u| {np.linalg.norm(gu):.2e}, "
          f"largest relative distance from the truth {np.max(np.abs(theta / c['truth'] - 1)):.2e}")
    assert converged and iterations <= 60
    if not c["noisy"]:
        assert np.max(np.abs(theta / c["truth"] - 1)) <= 1e-9


def test_entry_points_are_bound_and_refuse_bad_shapes():
    _lib.build()
    lib = _lib.load()
    L = lib.gf_spectral_fisher_slab()
    assert L >= 64 and L % 4 == 0
    assert lib.gf_spectral_fisher_work(1, 1, 1) > 0
    assert lib.gf_spectral_fisher_work(3, 2 * L + 3, 86) == 3 * lib.gf_spectral_fisher_work(1, 2 * L + 3, 86)
    assert lib.gf_spectral_fisher_work(1, L + 1, 5) > lib.gf_spectral_fisher_work(1, L, 5) + 1
    assert lib.gf_spectral_fisher_work(1, 100, 257) == 0 and lib.gf_spectral_fisher_work(1, 0, 5) == 0
    assert lib.gf_spectral_fisher_work(0, 100, 5) == 0
    none = [None] * 6
    st = lib.gf_spectral_fisher(1, 10, 257, 0, *none, None, 0, None, 0, *([None] * 4), None)
    assert st == -3 and b"at most 256" in lib.gf_last_error()
    st = lib.gf_spectral_fisher(1, 0, 3, 0, *none, None, 0, None, 0, *([None] * 4), None)
    assert st == -1 and b"bad shape" in lib.gf_last_error()
    st = lib.gf_spectral_fisher(1, 10, 3, 2, *none, None, 0, None, 0, *([None] * 4), None)
    assert st == -1 and b"objective" in lib.gf_last_error()
    st = lib.gf_spectral_fisher(1, 10, 3, 0, *none, None, 0, None, 0, *([None] * 4), None)
    assert st == -1 and b"null" in lib.gf_last_error()
    st = lib.gf_spectral_fisher(1, 10, 3, 1, *none, None, 0, None, 0, *([None] * 4), None)
    assert st == -1 and b"chi2" in lib.gf_last_error()
    st = lib.gf_spectral_fisher(65536, 10, 3, 0, *none, None, 0, None, 0, *([None] * 4), None)
    assert st == -1 and b"65535" in lib.gf_last_error()


def test_every_bad_selection_is_a_value_error_before_any_device_call():
    M, J = 50, 3
    ps = PowerSpectrum(np.linspace(1.0, 500.0, M), np.ones(M))
    sl = gadfly_amd.SpectralLikelihood(ps)
    ok = (np.ones((2, J)), np.full((2, J), 300.0), np.full((2, J), 2.0), DT)
    for call in (sl.fisher_device, sl.fisher, sl.covariance, sl.standard_errors):
        with pytest.raises(ValueError, match="wrt"):
            call(*ok, 0.1, wrt=("S0", "mean"))
        with pytest.raises(ValueError, match="wrt"):
            call(*ok, 0.1, wrt=())
        with pytest.raises(ValueError, match="log=True"):
            call(*ok, log=True)                                             # floor None
        with pytest.raises(ValueError, match="log=True"):
            call(*ok, 0.0, log=True)
        with pytest.raises(ValueError, match="log=True"):
            call(np.array([[1.0, 0.0, 1.0]] * 2), *ok[1:], 0.1, wrt=("S0", "Q"), log=True)
        with pytest.raises(ValueError, match="w0"):
            call(ok[0], np.zeros((2, J)), ok[2], DT, 0.1)
    with pytest.raises(ValueError, match="free"):
        sl.fit(*ok, 0.1, free=("S0", "slope"))
    with pytest.raises(ValueError, match="> 0"):
        sl.fit(*ok)                                                         # floor None, and free
    with pytest.raises(ValueError, match="> 0"):
        sl.fit(np.array([[1.0, 0.0, 1.0]] * 2), *ok[1:], 0.1)
    with pytest.raises(ValueError, match="Q"):
        sl.fit(ok[0], ok[1], -ok[2], DT, 0.1)
    # what is not free may be zero: the host checks pass, and without a GPU the first device call is what fails
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_lib.GadflyHipError):
            sl.fit(np.array([[1.0, 0.0, 1.0]] * 2), *ok[1:], 0.1, free=("w0", "floor"))
        with pytest.raises(_lib.GadflyHipError):
            sl.fisher(*ok, wrt=("S0", "w0", "Q"), log=True)
    assert list(spectral.parameter_index(("floor", "S0"), 3)) == [0, 1, 2, 9]
    assert list(spectral.parameter_index("w0", 2)) == [2, 3]


def test_scaled_inverse_flags_what_it_cannot_invert():
    """The host algebra of ``covariance``: a badly scaled positive definite matrix is inverted, an indefinite one, one
    with a zero diagonal entry and one holding NaN come back as NaN with ok = False -- each on its own."""
    rng = np.random.default_rng(2)
    A = rng.normal(size=(5, 5))
    plain = A @ A.T + 5 * np.eye(5)                                         # condition number below 10
    s = 10.0 ** np.arange(-6, 9, 3)
    good = plain * s[:, None] * s[None, :]
    indefinite = good.copy()                                                # a correlation of 2 between two parameters
    indefinite[2, 3] = indefinite[3, 2] = 2.0 * np.sqrt(good[2, 2] * good[3, 3])
    zero = good.copy()
    zero[1], zero[:, 1] = 0.0, 0.0
    nan = good.copy()
    nan[0, 0] = np.nan
    cov, ok = spectral._scaled_inverse(np.stack([good, indefinite, zero, nan, good]))
    assert list(ok) == [True, False, False, False, True]
    assert np.all(np.isnan(cov[1:4])) and np.array_equal(cov[0], cov[4]) and np.array_equal(cov[0], cov[0].T)
    want = np.linalg.inv(plain) / s[:, None] / s[None, :]
    norm = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    assert np.max(np.abs(cov[0] - want) / norm) <= 1e-12

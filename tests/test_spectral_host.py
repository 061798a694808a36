"""CPU: the spectral likelihoods' oracle (tests/spectral_ref.py) against torch autograd of an independent restatement,
Richardson central differences and ``get_psd``; the white floor against averaged periodograms; every host-side
ValueError of gadfly_amd.spectral; the bin counts; the bound C entry points."""
import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd import _lib, spectral
from gadfly_amd.psd import PowerSpectrum, _bin_starts
from gadfly_amd.synth import solar_like_hyperparameters
from tests import spectral_ref as ref

DT = 60.0e-6


def _problem(seed, B=2, J=4, M=300, over=True):
    rng = np.random.default_rng(seed)
    S0 = rng.uniform(0.5, 3.0, (B, J))
    w0 = np.sort(rng.uniform(200.0, 20000.0, (B, J)), axis=1)
    Q = rng.uniform(0.7, 12.0, (B, J))
    if over:
        Q[:, 0] = 0.3
    omega = 2 * np.pi * np.linspace(0.0, 8000.0, M)
    floor = rng.uniform(0.01, 0.1, B)
    delta = np.array([DT, 0.0])[:B]
    S = ref.model(S0, w0, Q, delta, floor, omega, np.float64)
    power = S * rng.exponential(size=S.shape)
    power[0, 7] = np.nan
    return S0, w0, Q, delta, floor, omega, power, S


def _torch_ll(objective, S0, w0, Q, floor, delta, omega, power, weight):
    """The reference's own form (core.py:33-41: w^2 - w0^2) in torch, float64; masked with nansum's rule."""
    w = omega[None, None, :]
    a, b, q = S0[:, :, None], w0[:, :, None], Q[:, :, None]
    terms = np.sqrt(2 / np.pi) * a * b ** 4 / ((w ** 2 - b ** 2) ** 2 + w ** 2 * b ** 2 / q ** 2)
    arg = delta[:, None] * omega[None, :] / 2
    one = torch.ones_like(arg)
    sinc = torch.where(arg == 0, one, torch.sin(arg) / torch.where(arg == 0, one, arg))
    S = sinc ** 2 * terms.sum(1) + floor[:, None]
    use = torch.isfinite(power) & torch.isfinite(weight) & (weight > 0)
    P = torch.where(use, power, torch.ones_like(power))
    n = torch.where(use, weight, torch.ones_like(weight))
    add = n * (torch.log(S) + P / S) if objective == "whittle" else 0.5 * ((P - S) / n) ** 2
    return -(torch.where(use, add, torch.zeros_like(add))).sum(1)


@pytest.mark.parametrize("objective", ["whittle", "chi2"])
def test_oracle_gradients_match_torch_autograd(objective):
    S0, w0, Q, delta, floor, omega, power, S = _problem(3)
    weight = np.ones_like(power) * 2.0 if objective == "whittle" else 0.3 * S
    weight[1, 11] = 0.0                                             # skipped by its weight
    o = ref.likelihood(objective, S0, w0, Q, delta, floor, omega, power, weight, np.float64)
    assert list(o["used"]) == [power.shape[1] - 1, power.shape[1] - 1] and not o["info"].any()
    t = [torch.tensor(v, requires_grad=True) for v in (S0, w0, Q, floor)]
    ll = _torch_ll(objective, *t, torch.tensor(delta), torch.tensor(omega), torch.tensor(power), torch.tensor(weight))
    grads = torch.autograd.grad(ll.sum(), t)
    # the restatement's w^2 - w0^2 loses up to Q u of relative accuracy per term; Q <= 12 here
    assert np.all(np.abs(ll.detach().numpy() - o["ll"]) <= 1e-12 * o["ll_scale"])
    for key, g in zip(("S0", "w0", "Q", "floor"), grads):
        err = np.abs(g.numpy() - o["g"][key]) / o["g_scale"][key]
        assert err.max() <= 1e-12, (key, err.max())


@pytest.mark.parametrize("objective", ["whittle", "chi2"])
def test_oracle_gradients_match_richardson_differences(objective):
    S0, w0, Q, delta, floor, omega, power, S = _problem(4, B=1, J=3, M=200)
    weight = None if objective == "whittle" else 0.2 * S
    o = ref.likelihood(objective, S0, w0, Q, delta, floor, omega, power, weight)
    pars = dict(S0=S0, w0=w0, Q=Q, floor=floor)

    def ll_at(key, idx, factor):
        p = {k: v.astype(np.longdouble) for k, v in pars.items()}
        p[key] = p[key].copy()
        p[key][idx] *= factor
        # (the oracle takes float64 inputs: evaluate in longdouble through its internals with the shifted value)
        return _ll_longdouble(objective, p, delta, omega, power, weight)

    for key, v in pars.items():
        for idx in np.ndindex(v.shape):
            h = np.longdouble(1e-3)
            d = []
            for s in (h, h / 2):
                d.append((ll_at(key, idx, 1 + s) - ll_at(key, idx, 1 - s)) / (2 * s * np.longdouble(v[idx])))
            fd = (4 * d[1] - d[0]) / 3
            got, scale = o["g"][key][(0,) + idx[1:]], o["g_scale"][key][(0,) + idx[1:]]
            # Richardson's remainder is O(h^4) of the fifth derivative: 1e-12 relative to the terms' own size
            assert abs(fd - got) <= 1e-8 * scale, (key, idx, fd, got)


def _ll_longdouble(objective, p, delta, omega, power, weight):
    """log-likelihood of ONE problem at longdouble parameters (no rounding of the shifted value to float64)."""
    ld = np.longdouble
    w = omega.astype(ld)[None, :]
    a, b, q = (p[k][0][:, None] for k in ("S0", "w0", "Q"))
    pi = 4 * np.arctan(ld(1))
    x = (w - b) * (w + b)
    term = np.sqrt(2 / pi) * a * b ** 4 / (x * x + w * w * b * b / (q * q))
    arg = ld(delta[0]) * omega.astype(ld) / 2
    safe = np.where(arg == 0, ld(1), arg)
    sinc = np.where(arg == 0, ld(1), np.sin(safe) / safe)
    S = sinc ** 2 * term.sum(0) + p["floor"][0]
    wt = np.ones(len(omega)) if weight is None else weight[0]
    use = np.isfinite(power[0]) & np.isfinite(wt) & (wt > 0)
    P, n, S = power[0][use].astype(ld), wt[use].astype(ld), S[use]
    if objective == "whittle":
        return -np.sum(n * (np.log(S) + P / S))
    return -np.sum(((P - S) / n) ** 2) / 2


@pytest.mark.parametrize("J", [6, 30])
def test_oracle_model_matches_get_psd(J):
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0)
    terms = kern.term.terms
    S0, w0, Q = (np.array([[getattr(t, k) for t in terms]]) for k in ("S0", "w0", "Q"))
    omega = 2 * np.pi * np.fft.rfftfreq(4096, DT)
    got = ref.model(S0, w0, Q, kern.delta, None, omega, np.float64)[0]
    want = kern.get_psd(omega)
    rel = np.max(np.abs(got - want) / want)
    print(f"J={J}: oracle S against get_psd, worst relative difference {rel:.2e}")
    # a positive sum of terms of a dozen roundings each, plus what get_psd's own form loses: w^2 - w0^2 carries an
    # absolute error of u w^2, which is u w^2 / |x| <= Q u w / w0 of D where it matters most (|x| = w w0 / Q, half a
    # line width from the centre), twice that in D = 2 x^2 there
    bound = (2.0 * Q.max() + 64.0) * 2.0 ** -53
    print(f"      bound {bound:.2e} (largest Q {Q.max():.0f})")
    assert rel <= bound
    truth = ref.model(S0, w0, Q, kern.delta, None, omega)[0]
    assert np.max(np.abs(got - truth) / truth) <= 1e-14


def test_white_floor_is_the_mean_periodogram_of_white_noise():
    rng = np.random.default_rng(12)
    N, draws, sigma = 4096, 400, 35.0
    y = rng.normal(size=(draws, N)) * sigma
    spec = np.fft.rfft(y, axis=-1)
    power = np.real(spec * np.conj(spec)) * (DT / np.sqrt(2 * np.pi) / N)        # PowerSpectrum's normalisation
    mean = power[:, 1:-1].mean()
    want = spectral.white_floor(sigma, DT)
    assert want == sigma ** 2 * DT / np.sqrt(2 * np.pi)
    assert abs(mean / want - 1.0) <= 0.02, mean / want


def test_every_bad_input_is_a_value_error_before_any_device_call():
    M, J = 50, 3
    freq = np.linspace(1.0, 500.0, M)
    power = np.ones(M)
    ok = dict(S0=np.ones((2, J)), w0=np.full((2, J), 300.0), Q=np.full((2, J), 2.0), delta=DT, floor=0.1)
    ps = PowerSpectrum(freq, power)
    sl = gadfly_amd.SpectralLikelihood(ps)
    assert sl.M == M and sl.rows == 1 and ps.counts is None

    def bad(match, **kw):
        args = dict(ok, **kw)
        for call in (sl.evaluate_device, sl.value_and_grad, sl.model_device):
            with pytest.raises(ValueError, match=match):
                call(args["S0"], args["w0"], args["Q"], args["delta"], args["floor"])

    bad("shape", S0=np.ones((2, J + 1)))
    bad("shape", S0=np.ones((2, 1, J)), w0=np.ones((2, 1, J)), Q=np.ones((2, 1, J)))
    bad("w0", w0=np.full((2, J), 0.0))
    bad("w0", w0=np.full((2, J), np.nan))
    bad("Q", Q=np.full((2, J), -1.0))
    bad("S0", S0=np.full((2, J), -1e-3))
    bad("floor", floor=-0.1)
    bad("floor", floor=np.ones(3))
    bad("delta", delta=-DT)
    bad("delta", delta=np.ones(5))
    bad("delta", delta=None)
    bad("at most", S0=np.ones((1, 257)), w0=np.ones((1, 257)), Q=np.ones((1, 257)))
    with pytest.raises(ValueError, match="wrt"):
        sl.value_and_grad(ok["S0"], ok["w0"], ok["Q"], DT, wrt=("S0", "mean"))
    # the spectrum's side
    with pytest.raises(ValueError, match="objective"):
        gadfly_amd.SpectralLikelihood(ps, objective="gauss")
    with pytest.raises(ValueError, match="chi2"):
        gadfly_amd.SpectralLikelihood(ps, objective="chi2")
    gadfly_amd.SpectralLikelihood(PowerSpectrum(freq, power, error=0.1 * power), objective="chi2")
    gadfly_amd.SpectralLikelihood(ps, objective="chi2", weights=0.1 * power)
    with pytest.raises(ValueError, match="ascending"):
        gadfly_amd.SpectralLikelihood(PowerSpectrum(freq[::-1], power))
    with pytest.raises(ValueError, match="weights"):
        gadfly_amd.SpectralLikelihood(ps, weights=np.ones(M + 1))
    with pytest.raises(ValueError, match="power of shape"):
        gadfly_amd.SpectralLikelihood(PowerSpectrum(freq, np.ones(M - 1)))
    with pytest.raises(ValueError, match="no frequency"):
        gadfly_amd.SpectralLikelihood(ps, frequency_min=600.0)
    cut = gadfly_amd.SpectralLikelihood(ps, frequency_min=100.0, frequency_max=200.0)
    assert cut.M == np.count_nonzero((freq >= 100.0) & (freq <= 200.0)) and cut.frequency[0] >= 100.0
    # (R, M) power: one parameter set per row
    rows = gadfly_amd.SpectralLikelihood(PowerSpectrum(freq, np.ones((3, M))))
    with pytest.raises(ValueError, match="power rows"):
        rows.evaluate_device(ok["S0"], ok["w0"], ok["Q"], DT)
    # kernels that are not sums of SHO terms, or of different lengths
    k6 = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(6), texp=60.0)
    k8 = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(8), texp=60.0)
    with pytest.raises(ValueError, match="same number"):
        sl.evaluate([k6, k8])
    S0, w0, Q, delta = spectral.kernel_parameters([k6, k6.term])
    assert S0.shape == (2, 6) and delta[0] == k6.delta and delta[1] == 0.0


def test_valid_parameters_pass_every_host_check():
    """Everything host-side passes: without a GPU the first device call is what fails, loudly."""
    sl = gadfly_amd.SpectralLikelihood(PowerSpectrum(np.linspace(1.0, 500.0, 50), np.ones(50)))
    args = (np.ones(3), np.full(3, 300.0), np.full(3, 2.0), DT)
    if torch.cuda.is_available():
        assert tuple(sl.evaluate_device(*args).shape) == (1,)
    else:
        with pytest.raises(_lib.GadflyHipError):
            sl.evaluate_device(*args)


@pytest.mark.parametrize("log", [True, False])
def test_bin_counts_are_the_bin_sizes(log):
    """What bin_power_spectrum stores as ``.counts``: np.diff of the bins' index ranges, i.e. the histogram of the
    axis over the same edges (the device statistics themselves: tests/test_gpu_spectral.py)."""
    freq = np.fft.rfftfreq(5000, DT)[1:]
    axis = np.log10(freq) if log else freq
    edges, start = _bin_starts(axis, 40)
    counts = np.diff(start)
    assert counts.sum() == len(freq) and np.array_equal(counts, np.histogram(axis, bins=edges)[0])


def test_entry_points_are_bound_and_refuse_bad_shapes():
    _lib.build()
    lib = _lib.load()
    T = lib.gf_spectral_tile()
    assert T >= 64 and T % 64 == 0
    assert lib.gf_spectral_work(1, 1, 1) > 0
    assert lib.gf_spectral_work(3, 2 * T + 3, 86) == 3 * lib.gf_spectral_work(1, 2 * T + 3, 86)
    assert lib.gf_spectral_work(1, T + 1, 5) > lib.gf_spectral_work(1, T, 5)
    assert lib.gf_spectral_work(1, 100, 257) == 0 and lib.gf_spectral_work(1, 0, 5) == 0
    none = [None] * 6
    st = lib.gf_spectral_like(1, 10, 257, 0, *none, None, 0, None, 0, *([None] * 9), None)
    assert st < 0 and b"at most 256" in lib.gf_last_error()
    st = lib.gf_spectral_like(1, 0, 3, 0, *none, None, 0, None, 0, *([None] * 9), None)
    assert st < 0 and b"bad shape" in lib.gf_last_error()
    st = lib.gf_spectral_like(1, 10, 3, 2, *none, None, 0, None, 0, *([None] * 9), None)
    assert st < 0 and b"objective" in lib.gf_last_error()
    st = lib.gf_spectral_like(1, 10, 3, 0, *none, None, 0, None, 0, *([None] * 9), None)
    assert st < 0 and b"null" in lib.gf_last_error()

"""
Batched sampling (``BatchedSampler`` / ``sample_batch`` / gf_sample_fused): light curves of B different kernels drawn
in the sweep that factors, no factor stored.

Bar: for fixed standard normals eps the draw agrees with the float64 C oracle -- ``cref.get_matrices`` ->
``cref.factor`` -> ``cref.matmul_lower(t, c, U, W, eps * sqrt(d))``, per problem, ``center=False`` and
``include_mean=False`` -- within TOL_VEC = 1e-6 of max|ref|, the project's bar for vectors and draws.  The oracle
itself sits within 3e-13 of the 80-bit recurrence on these shapes (6e-8 on a JD-based axis, where the 80-bit oracle's
unrounded phase product is the difference), so no case is left out; what the long-cadence cases are made of is
said in ``test_awkward_regimes``.  Measured on one MI355X: 8e-15 ... 2e-12 over all cases.
"""
import numpy as np
import pytest

from tests import sample_ref, util

pytestmark = pytest.mark.gpu

TOL_VEC = 1e-6
RTOL_LL = 1e-8
B = 8
JD0 = 2454833.0 * 0.0864


def _oracle(kernel, t, diag, eps):
    """(L D^1/2 eps, d, info) of one problem; eps (N,) or (N, R)."""
    from oracle import cref
    co = kernel.get_device_coefficients()
    t = np.ascontiguousarray(t, dtype=np.float64)
    c, a, U, V = cref.get_matrices(co[:6], t, np.broadcast_to(diag, t.shape) + co[6])
    d, Wm, info = cref.factor(t, c, a, U, V)
    if info:
        return None, d, info
    eps = np.asarray(eps, dtype=np.float64)
    x = eps * (np.sqrt(d) if eps.ndim == 1 else np.sqrt(d)[:, None])
    return cref.matmul_lower(t, c, U, Wm, x), d, 0


def _solar(J, cadence=60.0, seeds=range(B)):
    import gadfly_amd
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    base = solar_like_hyperparameters(J)
    return [gadfly_amd.StellarOscillatorKernel(jitter_hyperparameters(base, 300 + s), texp=cadence) for s in seeds]


def _stars(cadence=58.85, n=B):
    """n different stars from Hyperparameters.for_star: 86 underdamped terms each, W = 172."""
    import gadfly_amd
    out = []
    for i in range(n):
        f = i / max(n - 1, 1)
        hp = gadfly_amd.Hyperparameters.for_star(0.9 + 0.4 * f, 0.95 + 0.85 * f, 5500.0 + 700.0 * f,
                                                 0.75 + 3.5 * f, bandpass="SOHO VIRGO", quiet=True)
        assert len(hp) == 86
        out.append(gadfly_amd.StellarOscillatorKernel(hp, texp=cadence))
    return out


def _two_overdamped():
    """29 complex terms + two overdamped SHO terms (four real terms): W = 62 with Jr = 4, the by-column sweep."""
    import gadfly_amd
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    from gadfly_amd.terms import SHOTerm
    base = solar_like_hyperparameters(29)
    return [gadfly_amd.StellarOscillatorKernel(
        jitter_hyperparameters(base, 400 + s), texp=60.0,
        terms=[SHOTerm(S0=300.0 + 10.0 * s, w0=40.0, Q=0.3), SHOTerm(S0=100.0, w0=90.0 + s, Q=0.4)]) for s in range(B)]


def _one_real_31_complex():
    """W = 63: one real term next to 31 complex ones (the public SHO kernels only produce real terms in pairs)."""
    from gadfly_amd import terms

    class Coefficients(terms.Term):
        def __init__(self, co):
            self._co = co

        def get_coefficients(self):
            return self._co[:6]

        def get_diag_shift(self):
            return self._co[6]

    out = []
    for s, k in enumerate(_solar(31)):
        ar, cr, ac, bc, cc, dc, shift = k.get_device_coefficients()
        assert len(ar) == 0 and len(ac) == 31
        out.append(Coefficients((np.array([2000.0 + 100.0 * s]), np.array([25.0 + s]), ac, bc, cc, dc, shift)))
    return out


def _generic(kind):
    return [util.generic_kernel(kind) for _ in range(B)]


def _run(kernels, t, yerr, seed=0, label="", **kw):
    """Draws of the batch for its own eps per problem against the oracle; returns (sampler, eps, draws)."""
    import gadfly_amd
    nb = len(kernels)
    t = np.asarray(t, dtype=np.float64)
    N = t.shape[-1]
    eps = np.random.default_rng(1000 + seed).normal(size=(nb, N))
    yerr = np.broadcast_to(np.asarray(yerr, dtype=np.float64), (nb,))
    s = gadfly_amd.BatchedSampler(kernels, t, yerr=np.repeat(yerr[:, None], N, axis=1), **kw)
    got = s.sample(normals=eps, include_mean=False, center=False)
    assert got.shape == (nb, N) and got.dtype == np.float64
    assert not np.any(s.last_info)
    worst = 0.0
    for b in range(nb):
        ref, d, info = _oracle(kernels[b], t if t.ndim == 1 else t[b], yerr[b] ** 2, eps[b])
        assert info == 0
        err = np.max(np.abs(got[b] - ref)) / np.max(np.abs(ref))
        worst = max(worst, err)
    W = len(kernels[0])
    print(f"{label}: W={W} N={N} route={s.engine.kernel_used} worst={worst:.2e}")
    assert worst <= TOL_VEC, (label, worst)
    return s, eps, got


def _tj(N, cadence, seed=5):
    """time stamps with +-0.2 s of jitter (barycentric corrections)"""
    from gadfly_amd.synth import uniform_times
    return uniform_times(N, cadence) + np.random.default_rng(seed).uniform(-0.2, 0.2, N) * 1e-6


def _tgaps(N, cadence, seed=6):
    from gadfly_amd.synth import uniform_times
    rng = np.random.default_rng(seed)
    keep = np.ones(N, bool)
    keep[N // 3: N // 3 + N // 10] = False
    keep[rng.integers(0, N, N // 20)] = False
    return uniform_times(N, cadence)[keep]


PARITY = {
    "W2-overdamped": lambda: (_generic("overdamped"), util.generic_problem("overdamped", 3000)["t"], np.linspace(0.05, 0.2, B), "sample"),
    "W6-mixed": lambda: (_generic("mixed"), util.generic_problem("mixed", 3000)["t"], np.linspace(0.05, 0.2, B), "sample"),
    "W12": lambda: (_solar(6), np.arange(4000) * 60e-6, 30.0, "sample"),
    "W40-jittered-stamps": lambda: (_solar(20), _tj(3500, 60.0), np.linspace(20.0, 40.0, B), "sample"),
    "W60-gaps": lambda: (_solar(30), _tgaps(4000, 60.0), 30.0, "sample"),
    "W62-31-complex": lambda: (_solar(31), np.arange(3000) * 60e-6, 30.0, "sample"),
    "W62-29-complex-4-real": lambda: (_two_overdamped(), np.arange(3000) * 60e-6, 30.0, "sample"),
    "W63-1-real-31-complex": lambda: (_one_real_31_complex(), np.arange(3000) * 60e-6, 30.0, "sample"),
    "W80": lambda: (_solar(40), np.arange(3000) * 60e-6, 30.0, "sample-wide"),
    "W172-stars": lambda: (_stars(), np.arange(2500) * 58.85e-6, np.linspace(20.0, 40.0, B), "sample-wide"),
    "W60-tiles": lambda: (_solar(30), np.arange(3 * 8192 + 1) * 60e-6, 30.0, "sample"),
    "W172-tiles": lambda: (_stars(), np.arange(2 * 8192 + 5) * 58.85e-6, 30.0, "sample-wide"),
}


@pytest.mark.parametrize("case", list(PARITY))
def test_parity_with_the_oracle(hip, case):
    kernels, t, yerr, route = PARITY[case]()
    assert len(kernels) == B
    s, _, _ = _run(kernels, t, yerr, label=case)
    assert s.engine.kernel_used == route
    want_w = int(case.split("-")[0][1:])
    assert len(kernels[0]) == want_w
    if case.endswith("tiles"):
        assert s.engine.N > 2 * s.engine.tile_rows         # the state crosses tile borders


@pytest.mark.parametrize("wide", [False, True], ids=["W60", "W172"])
@pytest.mark.parametrize("regime", ["long-cadence", "jd-axis", "own-axes", "yerr0"])
def test_awkward_regimes(hip, regime, wide):
    """Long cadence: time stamps 1765 s apart, so every row is a reset row of the scaled coordinates.  The kernels
    keep their short-cadence exposure: integrated over 1765 s, the solar-like coefficient sets stop being a fair
    float64 input -- c * delta reaches 33, the coefficients 3e14, and the diagonal a = sum a_j + shift = 6e4 is what
    is left of their cancellation -- and the float64 C oracle itself then departs from the 80-bit oracle by up to
    8e-6 in the draw (8e-5 in d; jitter seed 300, measured on the CPU), above the bar, for reasons that lie in how
    the host sums the diagonal and not in any sweep.  With the short exposure the oracle is within 1e-13."""
    N = 2000 if wide else 3000
    cadence = 1765.0 if regime == "long-cadence" else (58.85 if wide else 60.0)
    kernels = _stars() if wide else _solar(30)
    t = np.arange(N) * cadence * 1e-6
    yerr = 30.0
    if regime == "jd-axis":
        t = t + JD0
    elif regime == "own-axes":
        starts = np.random.default_rng(3).uniform(0.0, 5e-3, B)
        t = starts[:, None] + t[None, :] * (1.0 + 1e-3 * np.arange(B))[:, None]
    elif regime == "yerr0":
        yerr = 0.0
    s, _, _ = _run(kernels, t, yerr, label=f"{regime}/{'W172' if wide else 'W60'}")
    assert s.engine.kernel_used == ("sample-wide" if wide else "sample")


@pytest.mark.parametrize("R", [1, 3, 5])
def test_size_draws_mean_and_centering(hip, R):
    import gadfly_amd
    N = 3000
    kernels = _solar(12)
    t = np.arange(N) * 60e-6
    mean = np.linspace(-50.0, 80.0, B)
    eps = np.random.default_rng(77 + R).normal(size=(B, R, N))
    s = gadfly_amd.BatchedSampler(kernels, t, yerr=30.0, mean=mean)
    raw = s.sample(normals=eps, size=R, include_mean=False, center=False)
    assert raw.shape == (B, R, N)
    for b in range(B):
        ref, _, info = _oracle(kernels[b], t, 900.0, eps[b].T)
        assert info == 0
        err = np.max(np.abs(raw[b].T - ref)) / np.max(np.abs(ref))
        assert err <= TOL_VEC, (b, err)
    scale = np.max(np.abs(raw)) + np.max(np.abs(mean))
    with_mean = s.sample(normals=eps, size=R, include_mean=True, center=False)
    assert np.max(np.abs(with_mean - (raw + mean[:, None, None]))) <= 1e-13 * scale
    centred = s.sample(normals=eps, size=R, include_mean=True, center=True)
    want = np.stack([sample_ref.center(raw[b] + mean[b], R) for b in range(B)])
    assert np.max(np.abs(centred - want)) <= 1e-12 * scale
    # one draw per problem (size=None): the time-mean goes
    one = s.sample(normals=eps[:, 0, :], include_mean=True, center=True)
    want1 = np.stack([sample_ref.center(raw[b, 0] + mean[b], None) for b in range(B)])
    assert one.shape == (B, N) and np.max(np.abs(one - want1)) <= 1e-12 * scale
    dev = s.sample_device(normals=eps, size=R)
    assert dev.is_cuda and tuple(dev.shape) == (B, R, N)


def _case4(N=20000):
    kernels = _solar(30)
    t = np.arange(N) * 60e-6
    eps = np.random.default_rng(2024).normal(size=(B, N))
    return kernels, t, eps


def test_agrees_with_the_single_kernel_api_and_feeds_the_spectrum(hip):
    import gadfly_amd
    kernels, t, eps = _case4()
    N = len(t)
    s = gadfly_amd.BatchedSampler(kernels, t, yerr=30.0)
    raw = s.sample(normals=eps, include_mean=False, center=False)
    singles = {}
    for b in (0, 3, 7):
        gp = gadfly_amd.GaussianProcess(kernels[b], t=t, yerr=30.0)
        singles[b] = gp.dot_tril(eps[b])
        err = np.max(np.abs(raw[b] - singles[b])) / np.max(np.abs(singles[b]))
        print(f"problem {b}: batched draw vs GaussianProcess.dot_tril: {err:.2e}")
        assert err <= TOL_VEC
    # straight into the spectrum: the (B, N) device tensor as R = B series
    dev = s.sample_device(normals=eps)
    assert dev.is_cuda
    ps = gadfly_amd.PowerSpectrum.from_flux(dev, 60e-6).bin(20)
    assert ps.power.shape == (B, 20)
    one = np.stack([singles[b] - singles[b].mean() for b in (0, 3, 7)])
    ps1 = gadfly_amd.PowerSpectrum.from_flux(one, 60e-6).bin(20)
    np.testing.assert_allclose(np.asarray(ps.power)[[0, 3, 7]], np.asarray(ps1.power), rtol=1e-6)
    # one-shot form: the same draws
    shot = gadfly_amd.sample_batch(kernels, t, yerr=30.0, normals=eps)
    assert shot.is_cuda and np.array_equal(shot.cpu().numpy(), dev.cpu().numpy())


def test_round_trip_with_the_evaluator(hip):
    """y = L D^1/2 eps  =>  log L(y) = -(eps^T eps + sum log d + N log 2 pi) / 2, sum log d from the oracle."""
    import gadfly_amd
    kernels, t, eps = _case4()
    N = len(t)
    y = gadfly_amd.BatchedSampler(kernels, t, yerr=30.0).sample(normals=eps, include_mean=False, center=False)
    ll = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=30.0).evaluate()
    for b in range(B):
        _, d, info = _oracle(kernels[b], t, 900.0, eps[b])
        assert info == 0
        ref = -0.5 * (float(eps[b] @ eps[b]) + float(np.sum(np.log(d))) + N * np.log(2.0 * np.pi))
        assert abs(ll[b] - ref) <= RTOL_LL * abs(ref), (b, ll[b], ref)


def test_nine_series_of_nine_lengths(hip):
    import gadfly_amd
    from gadfly_amd.synth import scale_hyperparameters, solar_like_hyperparameters
    lengths = [9000, 20011, 12345, 17000, 9001, 15500, 20000, 11111, 13000]
    rng = np.random.default_rng(7)
    base = solar_like_hyperparameters(20)
    nb = len(lengths)
    kernels = [gadfly_amd.StellarOscillatorKernel(scale_hyperparameters(base, f), texp=58.85)
               for f in np.geomspace(0.4, 1.0, nb)]
    t = [rng.uniform(0.0, 1e-3) + np.arange(n) * 58.85e-6 * (1.0 + 1e-3 * i) for i, n in enumerate(lengths)]
    yerr = [np.full(n, rng.uniform(20.0, 40.0)) for n in lengths]
    eps = [rng.normal(size=n) for n in lengths]
    mean = np.linspace(1.0, 9.0, nb)
    s = gadfly_amd.BatchedSampler(kernels, t, yerr=yerr, mean=mean)
    assert list(s.rows) == lengths and s.N == max(lengths)
    got = s.sample_device(normals=eps, include_mean=False, center=False)
    assert isinstance(got, list) and len(got) == nb
    for b, n in enumerate(lengths):
        assert got[b].is_cuda and tuple(got[b].shape) == (n,)
        ref, _, info = _oracle(kernels[b], t[b], yerr[b] ** 2, eps[b])
        assert info == 0
        err = np.max(np.abs(got[b].cpu().numpy() - ref)) / np.max(np.abs(ref))
        assert err <= TOL_VEC, (b, err)
    assert not np.any(s.last_info)
    # mean and centring follow each series' own rows; `size` draws come back as (size, N_b)
    cen = s.sample(normals=eps, include_mean=True, center=True)
    for b in range(nb):
        raw = got[b].cpu().numpy()
        assert np.max(np.abs(cen[b] - sample_ref.center(raw + mean[b], None))) <= 1e-12 * np.max(np.abs(raw))
    eps2 = [rng.normal(size=(2, n)) for n in lengths]
    two = s.sample(normals=eps2, size=2, include_mean=False, center=False)
    for b, n in enumerate(lengths):
        assert two[b].shape == (2, n)
        ref, _, _ = _oracle(kernels[b], t[b], yerr[b] ** 2, eps2[b].T)
        assert np.max(np.abs(two[b].T - ref)) <= TOL_VEC * np.max(np.abs(ref))


@pytest.mark.parametrize("wide", [False, True], ids=["W60", "W172"])
def test_a_failing_problem_is_isolated(hip, wide):
    import gadfly_amd
    N = 3000
    kernels = _stars() if wide else _solar(30)
    t = np.arange(N) * (58.85e-6 if wide else 60e-6)
    diag = np.full((B, N), 900.0)
    diag[5, 1234] = -1.0e9                              # one problem of eight is not positive definite
    eps = np.random.default_rng(9).normal(size=(B, N))
    s = gadfly_amd.BatchedSampler(kernels, t, diag=diag)
    got = s.sample(normals=eps, include_mean=False, center=False)
    info = s.last_info
    for b in range(B):
        ref, _, oinfo = _oracle(kernels[b], t, diag[b], eps[b])
        if b == 5:
            assert oinfo > 0 and info[b] == oinfo
            assert np.all(np.isnan(got[b]))
        else:
            assert oinfo == 0 and info[b] == 0
            assert np.max(np.abs(got[b] - ref)) <= TOL_VEC * np.max(np.abs(ref))


def test_reproducibility_and_packs(hip):
    import gadfly_amd
    N = 5000
    kernels = _solar(20)
    t = np.arange(N) * 60e-6
    eps = np.random.default_rng(31).normal(size=(B, N))
    s = gadfly_amd.BatchedSampler(kernels, t, yerr=30.0)
    a = s.sample(normals=eps, center=False)
    b = s.sample(normals=eps, center=False)
    assert np.array_equal(a, b)
    s1 = s.sample(seed=5)
    s2 = s.sample(seed=5)
    s3 = s.sample(seed=6)
    assert np.array_equal(s1, s2) and not np.array_equal(s1, s3)
    assert np.all(np.isfinite(s1)) and np.max(np.abs(s1.mean(axis=1))) <= 1e-9 * np.max(np.abs(s1))
    m1 = s.sample(seed=5, size=2)
    assert m1.shape == (B, 2, N) and np.array_equal(m1, s.sample(seed=5, size=2))
    # new kernels per call through an O(B J) upload: pack(kernels) and pack_parameters of the same kernels
    others = _solar(20, seeds=range(50, 50 + B))
    hp = [k.hyperparameters for k in others]
    S0, w0, Q = (np.array([[p["hyperparameters"][key] for p in h] for h in hp]) for key in ("S0", "w0", "Q"))
    p1 = s.sample(pack=s.pack(others), normals=eps, center=False)
    p2 = s.sample(pack=s.pack_parameters(S0, w0, Q, others[0].delta), normals=eps, center=False)
    scale = np.max(np.abs(p1))
    assert np.max(np.abs(p1 - p2)) <= TOL_VEC * scale
    assert np.max(np.abs(p1 - a)) > 1e-3 * scale           # (they ARE other kernels)
    for k in (0, B - 1):
        ref, _, _ = _oracle(others[k], t, 900.0, eps[k])
        assert np.max(np.abs(p1[k] - ref)) <= TOL_VEC * np.max(np.abs(ref))


def test_generator_period_is_the_callers_to_set(hip):
    """Exact rows by default; the evaluator's rule (period from the measured conditioning, with its re-run) on
    request -- both within the bar."""
    import gadfly_amd
    N = 6000
    kernels = _solar(30)
    t = np.arange(N) * 60e-6
    eps = np.random.default_rng(8).normal(size=(B, N))
    refs = [_oracle(kernels[b], t, 900.0, eps[b])[0] for b in range(B)]
    s = gadfly_amd.BatchedSampler(kernels, t, yerr=30.0)
    assert s.generator_period == 1 and not s.auto_generator_period
    s.auto_generator_period = True
    for call in range(2):                                   # (the second call runs at the calibrated period)
        got = s.sample(normals=eps, include_mean=False, center=False)
        err = max(np.max(np.abs(got[b] - refs[b])) / np.max(np.abs(refs[b])) for b in range(B))
        print(f"automatic period, call {call}: period {s.engine.generator_period}, worst {err:.2e}")
        assert err <= TOL_VEC
    assert s._auto_period in (1, 2, 4, 8, 16, 32, 64)
    s.auto_generator_period = False
    s.generator_period = 4
    got = s.sample(normals=eps, include_mean=False, center=False)
    assert s.engine.generator_period == 4
    err = max(np.max(np.abs(got[b] - refs[b])) / np.max(np.abs(refs[b])) for b in range(B))
    print(f"period 4: worst {err:.2e}")
    assert err <= TOL_VEC


def test_phases_out_of_range_are_refused(hip):
    import gadfly_amd
    t = 1.0e9 + np.arange(500) * 60e-6                      # phases of 2e13 rad: beyond the in-kernel sincos
    s = gadfly_amd.BatchedSampler(_solar(6), t, yerr=30.0)
    with pytest.raises(NotImplementedError, match="phases"):
        s.sample_device(seed=1)

"""GPU: spectral likelihoods (``gf_spectral_like``) against the longdouble oracle of
tests/spectral_ref.py -- boundary shapes, awkward inputs, masks, bit identity across batches, groups and call kinds,
the failure path, the stationary point, the autograd Function, the device-to-device pipeline and an LBFGS step.

Bars (all against the longdouble truth): model 1e-12 relative, l 1e-12 x its scale, gradients 1e-11 x their scale.  A
per-addend error of (J + a few tens) u plus log2(M) u for the tree sums is about 1e-14 x scale, so the bars leave two
to three orders of margin; the worst ratios seen are printed by every test (run with -s) and recorded in DESIGN.md."""
import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd import spectral
from gadfly_amd.psd import PowerSpectrum, _bin_starts
from tests import spectral_ref as ref

pytestmark = pytest.mark.gpu

DT = 60.0e-6                         # one-minute cadence in 1/uHz
NYQUIST = 0.5 / DT                   # uHz
BAR_MODEL, BAR_LL, BAR_GRAD = 1e-12, 1e-12, 1e-11
OBJECTIVES = ("whittle", "chi2")
KEYS = ("S0", "w0", "Q", "floor")

_BASE86 = None


def _axis(M):
    """M frequencies from 0 to the Nyquist frequency of a one-minute cadence (omega = 0 present)."""
    return np.arange(M) * (NYQUIST / max(M - 1, 1))


def _params(seed, B, J, freq):
    """B different parameter sets of J terms on the axis ``freq``.  J = 86: gadfly's solar kernel, jittered per
    problem.  Otherwise random terms inside the band; with J >= 2 term 0 is overdamped (Q = 0.3), and the last term
    is a p-mode of Q = 1600 a tenth of its line width above a frequency of the axis."""
    global _BASE86
    rng = np.random.default_rng(seed)
    if J == 86:
        if _BASE86 is None:
            hp = gadfly_amd.Hyperparameters.for_star(1, 1, 5777, 1, bandpass="SOHO VIRGO", quiet=True)
            _BASE86 = np.array([[p["hyperparameters"][k] for p in hp] for k in ("S0", "w0", "Q")])
        assert _BASE86.shape == (3, 86)
        jit = np.exp(0.05 * rng.normal(size=(3, B, J)))
        return tuple(_BASE86[i][None, :] * jit[i] for i in range(3))
    S0 = rng.uniform(0.5, 3.0, (B, J))
    w0 = 2 * np.pi * rng.uniform(0.02, 0.9, (B, J)) * NYQUIST
    Q = rng.uniform(0.7, 20.0, (B, J))
    if J >= 2:
        Q[:, 0] = 0.3
    k = np.minimum(len(freq) - 1, np.maximum(1, (len(freq) * np.array([0.31, 0.52, 0.77, 0.4, 0.6])).astype(int)))
    wk = 2 * np.pi * freq[k[np.arange(B) % 5]]
    good = wk > 0
    Q[good, -1] = 1600.0
    w0[good, -1] = wk[good] * (1.0 + 0.1 / 1600.0)
    return S0, w0, Q


def _case(seed, objective, B, J, M, per_problem_power=False):
    """A problem set: parameters, exposures (0 and the cadence), floors (0 and positive), Exp(1)-scattered power."""
    freq = _axis(M)
    omega = 2 * np.pi * freq
    S0, w0, Q = _params(seed, B, J, freq)
    delta = np.array([0.0, DT, DT])[:B]
    floor = np.array([0.02, 0.0, 0.5])[:B]
    rng = np.random.default_rng(seed + 1000)
    S = ref.model(S0, w0, Q, delta, floor, omega, np.float64)
    rows = B if per_problem_power else 1
    if objective == "whittle":
        power = S[:rows] * rng.exponential(size=(rows, M))
        weight = None
    else:
        power = S[:rows] * (1.0 + 0.1 * rng.normal(size=(rows, M)))
        weight = 0.1 * S[:rows]
    return dict(freq=freq, omega=omega, S0=S0, w0=w0, Q=Q, delta=delta, floor=floor, power=power, weight=weight,
                objective=objective)


def _evaluator(c, rows=None):
    power, weight = c["power"], c["weight"]
    if rows is not None:
        power = power[rows] if power.shape[0] > 1 else power
        weight = weight if weight is None or weight.shape[0] == 1 else weight[rows]
    squeeze = (lambda x: x[0] if x is not None and x.shape[0] == 1 else x)
    ps = PowerSpectrum(c["freq"], squeeze(power))
    return gadfly_amd.SpectralLikelihood(ps, objective=c["objective"], weights=squeeze(weight))


def _oracle(c, sel=slice(None)):
    power = c["power"] if c["power"].shape[0] == 1 else c["power"][sel]
    weight = c["weight"]
    if weight is not None and weight.shape[0] > 1:
        weight = weight[sel]
    return ref.likelihood(c["objective"], c["S0"][sel], c["w0"][sel], c["Q"][sel], c["delta"][sel],
                          None if c["floor"] is None else c["floor"][sel], c["omega"], power, weight)


def _ratios(o, ll, g, model=None):
    """Worst error / scale ratios of a device result against the oracle ``o``: dict(ll=, grad=, model=)."""
    r = dict(ll=float(np.max(np.abs(ll - o["ll"]) / np.maximum(o["ll_scale"], np.finfo(float).tiny))))
    if g is not None:
        worst = 0.0
        for k, v in g.items():
            s = o["g_scale"][k]
            err = np.abs(v - o["g"][k])
            worst = max(worst, float(np.max(np.where(s > 0, err / np.where(s > 0, s, 1), err))))
        r["grad"] = worst
    if model is not None:
        r["model"] = float(np.max(np.abs(model - o["model"]) / o["model"]))
    return r


def _within_bars(r):
    return r["ll"] <= BAR_LL and r.get("grad", 0.0) <= BAR_GRAD and r.get("model", 0.0) <= BAR_MODEL


def _args(c, sel=slice(None)):
    return (c["S0"][sel], c["w0"][sel], c["Q"][sel], c["delta"][sel], None if c["floor"] is None else c["floor"][sel])


def _tile_sizes(hip):
    T = hip.load().gf_spectral_tile()
    return T, (1, 2, T - 1, T, T + 1, 2 * T + 3)


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_boundary_shapes(hip, objective, which):
    """M in {1, 2, T-1, T, T+1, 2T+3} x J in {1, 2, 5, 33, 86} x B in {1, 3}, with and without gradients."""
    T, sizes = _tile_sizes(hip)
    M = sizes[which]
    worst = dict(ll=0.0, grad=0.0, model=0.0)
    for J in (1, 2, 5, 33, 86):
        c = _case(100 * which + J, objective, 3, J, M)
        o = _oracle(c)
        sl = _evaluator(c)
        ll, g = sl.value_and_grad(*_args(c))
        used, info = sl.last_used, sl.last_info
        value = sl.evaluate_device(*_args(c)).cpu().numpy()
        model = sl.model_device(*_args(c)).cpu().numpy()
        assert model.shape == (3, M) and ll.shape == (3,) and g["w0"].shape == (3, J)
        assert np.array_equal(used, o["used"]) and not info.any() and np.all(used == M)
        assert np.array_equal(value, ll)                                    # value only = the gradient call's value
        r = _ratios(o, ll, g, model)
        assert _within_bars(r), (J, M, r)
        # B = 1: problem 0 alone, bit for bit what it is inside the batch
        one = slice(0, 1)
        l1, g1 = sl.value_and_grad(*_args(c, one))
        assert l1[0] == ll[0] and all(np.array_equal(g1[k][0], g[k][0]) for k in KEYS)
        assert sl.evaluate_device(*_args(c, one)).cpu().numpy()[0] == ll[0]
        worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"boundary shapes {objective} M={M}: worst error / scale: l {worst['ll']:.2e}, gradients "
          f"{worst['grad']:.2e}, model (relative) {worst['model']:.2e}")


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_masks_and_awkward_inputs(hip, objective):
    """omega = 0, delta = 0 and the cadence, floor None, an overdamped term, a Q = 1600 line with frequencies inside
    its width, power per problem, NaN power at a tile's first and last frequency and across a whole tile, zero and
    NaN weights: ``used`` is the oracle's count and the sums skip what the oracle skips."""
    T, _ = _tile_sizes(hip)
    M = 2 * T + 3
    c = _case(7, objective, 3, 5, M, per_problem_power=True)
    c["floor"] = None
    # frequencies inside the line width of problem 0's p-mode: w0 / Q = 1.5 line widths cover these neighbours
    w_line = c["w0"][0, -1]
    assert np.count_nonzero(np.abs(c["omega"] - w_line) < w_line / 1600.0) >= 1
    c["power"][0, [T, 2 * T - 1]] = np.nan
    c["power"][1, T:2 * T] = np.nan
    c["power"][2, 0] = np.inf
    if c["weight"] is None:
        c["weight"] = np.tile(np.arange(1.0, M + 1.0) % 7 + 1.0, (3, 1))     # binned-spectrum-like counts
    c["weight"][2, [5, T + 1]] = 0.0
    c["weight"][2, 9] = np.nan
    c["weight"][0, 11] = -1.0
    o = _oracle(c)
    assert list(o["used"]) == [M - 3, M - T, M - 4]
    sl = _evaluator(c)
    ll, g = sl.value_and_grad(*_args(c))
    model = sl.model_device(*_args(c)).cpu().numpy()
    assert np.array_equal(sl.last_used, o["used"]) and not sl.last_info.any()
    r = _ratios(o, ll, g, model)
    print(f"masks {objective}: worst error / scale: l {r['ll']:.2e}, gradients {r['grad']:.2e}, model {r['model']:.2e}")
    assert _within_bars(r), r
    # a p-mode of Q = 1600 whose centre sits on a frequency of the axis, and one between two frequencies
    c2 = _case(8, objective, 3, 2, T + 1)
    c2["w0"][0, -1] = c2["omega"][T // 2]
    c2["w0"][1, -1] = 0.5 * (c2["omega"][T // 3] + c2["omega"][T // 3 + 1])
    c2["Q"][:2, -1] = 1600.0
    o2 = _oracle(c2)
    sl2 = _evaluator(c2)
    ll2, g2 = sl2.value_and_grad(*_args(c2))
    r2 = _ratios(o2, ll2, g2, sl2.model_device(*_args(c2)).cpu().numpy())
    print(f"line centres {objective}: worst error / scale: l {r2['ll']:.2e}, gradients {r2['grad']:.2e}, "
          f"model {r2['model']:.2e}")
    assert _within_bars(r2), r2


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_all_frequencies_masked(hip, objective):
    T, _ = _tile_sizes(hip)
    c = _case(9, objective, 3, 5, T + 1)
    c["power"][:] = np.nan
    sl = _evaluator(c)
    ll, g = sl.value_and_grad(*_args(c))
    assert np.all(ll == 0.0) and np.all(sl.last_used == 0) and not sl.last_info.any()
    for k in KEYS:
        assert np.all(g[k] == 0.0), k
    assert np.all(sl.evaluate_device(*_args(c)).cpu().numpy() == 0.0)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_bit_identity(hip, objective):
    """A problem alone = inside B = 3 = under any group cap; two runs agree; value only = the gradient call's value;
    the model call leaves l unchanged."""
    T, _ = _tile_sizes(hip)
    M, J = 2 * T + 3, 33
    c = _case(21, objective, 3, J, M, per_problem_power=True)
    sl = _evaluator(c)
    ll, g = sl.value_and_grad(*_args(c))
    assert sl.last_plan[1:] == (1, 3)
    ll_again, g_again = sl.value_and_grad(*_args(c))
    assert np.array_equal(ll, ll_again) and all(np.array_equal(g[k], g_again[k]) for k in KEYS)
    assert np.array_equal(sl.evaluate_device(*_args(c)).cpu().numpy(), ll)
    out = sl.run_device(*_args(c), grad=True, model=True)                   # gradients and model in one call
    assert np.array_equal(out["ll"].cpu().numpy(), ll)
    assert np.array_equal(out["model"].cpu().numpy(), sl.model_device(*_args(c)).cpu().numpy())
    per = sl.last_plan[0] // 3
    for cap, plan in ((per, (3, 1)), (2 * per + 8, (2, 2))):
        sl.workspace_bytes = cap
        l2, g2 = sl.value_and_grad(*_args(c))
        assert sl.last_plan[1:] == plan
        assert np.array_equal(l2, ll) and all(np.array_equal(g2[k], g[k]) for k in KEYS)
        assert np.array_equal(sl.evaluate_device(*_args(c)).cpu().numpy(), ll)
    for b in range(3):
        alone = _evaluator(c, rows=slice(b, b + 1))
        l1, g1 = alone.value_and_grad(*_args(c, slice(b, b + 1)))
        assert l1[0] == ll[b] and all(np.array_equal(g1[k][0], g[k][b]) for k in KEYS), b


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_failure_is_isolated(hip, objective):
    """S0 = 0 with floor = 0 (S = 0 everywhere): l = -inf, NaN gradients, info = first used index + 1; the neighbours
    in the batch keep their bits."""
    T, _ = _tile_sizes(hip)
    M = T + 5
    c = _case(31, objective, 3, 5, M, per_problem_power=True)
    c["floor"] = np.array([0.02, 0.0, 0.5])
    c["S0"][1] = 0.0
    c["power"][1, :3] = np.nan                                              # the first used frequency is k = 3
    o = _oracle(c)
    assert o["info"][1] == 4 and o["ll"][1] == -np.inf
    sl = _evaluator(c)
    ll, g = sl.value_and_grad(*_args(c))
    assert ll[1] == -np.inf and list(sl.last_info) == [0, 4, 0] and np.array_equal(sl.last_used, o["used"])
    assert all(np.all(np.isnan(g[k][1])) for k in KEYS)
    assert sl.evaluate_device(*_args(c)).cpu().numpy()[1] == -np.inf
    # a failure in the second tile reports the index in the whole axis
    c["power"][1, :T + 2] = np.nan
    sl_late = _evaluator(c)
    assert sl_late.evaluate_device(*_args(c)).cpu().numpy()[1] == -np.inf and sl_late.last_info[1] == T + 3
    keep = [0, 2]
    r = _ratios(_oracle(c, keep), ll[keep], {k: v[keep] for k, v in g.items()})
    assert _within_bars(r), r
    for b in keep:
        alone = _evaluator(c, rows=slice(b, b + 1))
        l1, g1 = alone.value_and_grad(*_args(c, slice(b, b + 1)))
        assert l1[0] == ll[b] and all(np.array_equal(g1[k][0], g[k][b]) for k in KEYS), b


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_stationary_point(hip, objective):
    """With P = S(theta*) every gradient at theta* vanishes to rounding (below 1e-11 x scale); at 1.3 theta* none of
    the parameter blocks does."""
    T, _ = _tile_sizes(hip)
    M, J = T + 1, 5
    c = _case(41, objective, 3, J, M, per_problem_power=True)
    truth = ref.model(c["S0"], c["w0"], c["Q"], c["delta"], c["floor"], c["omega"])
    c["power"] = truth.astype(np.float64)
    c["weight"] = None if objective == "whittle" else 0.1 * c["power"]
    sl = _evaluator(c)
    ll, g = sl.value_and_grad(*_args(c))
    o = _oracle(c)
    worst = max(float(np.max(np.abs(g[k]) / o["g_scale"][k])) for k in KEYS)
    print(f"stationary point {objective}: worst |gradient| / scale at theta* {worst:.2e}")
    assert worst <= BAR_GRAD
    off = dict(c, S0=1.3 * c["S0"], w0=1.3 * c["w0"], Q=1.3 * c["Q"], floor=1.3 * c["floor"])
    _, g_off = sl.value_and_grad(*_args(off))
    o_off = _oracle(off)
    for k in KEYS:
        assert float(np.max(np.abs(g_off[k]) / np.where(o_off["g_scale"][k] > 0, o_off["g_scale"][k], np.inf))) \
            > 1e3 * BAR_GRAD, k


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_autograd_function(hip, objective):
    M, J = 257, 2
    fn = gadfly_amd.SpectralLogLikelihood
    assert fn is spectral.SpectralLogLikelihood
    for B in (1, 3):
        c = _case(51 + B, objective, B, J, M, per_problem_power=B > 1)
        c["Q"][:, -1] = 6.0                       # (no Q = 1600 line: the difference quotient's step is 1e-6)
        c["floor"] = np.array([0.02, 0.05, 0.5])[:B]
        sl = _evaluator(c)
        args = tuple(torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in KEYS)
        f = lambda a, b, q, fl: fn.apply(a, b, q, fl, sl, c["delta"])      # noqa: E731
        assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-5, rtol=1e-3)
        if B == 3:                                # backward weights each problem with its own grad_output
            ll, g = sl.value_and_grad(*_args(c))
            wts = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
            out = f(*args)
            assert np.array_equal(out.detach().numpy(), ll)
            out.backward(wts)
            for t, k in zip(args, KEYS):
                want = g[k] * (wts.numpy()[:, None] if g[k].ndim == 2 else wts.numpy())
                assert np.array_equal(t.grad.numpy(), want), k
    # (J,) parameters and a scalar floor against a shared spectrum: the gradients take the inputs' shapes
    c = _case(55, objective, 1, J, M)
    sl = _evaluator(c)
    a, b, q = (torch.tensor(c[k][0], requires_grad=True) for k in ("S0", "w0", "Q"))
    fl = torch.tensor(0.02, dtype=torch.float64, requires_grad=True)
    fn.apply(a, b, q, fl, sl, DT).sum().backward()
    assert a.grad.shape == (J,) and fl.grad.shape == () and torch.isfinite(b.grad).all()


def test_device_to_device_pipeline(hip):
    """sample_device -> PowerSpectrum.from_flux -> SpectralLikelihood: the launches read the spectrum's own device
    copy; the binned spectrum carries its counts, the Whittle weights by default."""
    from gadfly_amd.synth import solar_like_hyperparameters
    N = 8192
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(6), texp=60.0)
    gp = gadfly_amd.GaussianProcess(kern, t=np.arange(N) * DT, yerr=30.0, device="cuda:0")
    np.random.seed(3)
    draw = gp.sample_device()
    assert draw.is_cuda
    ps = PowerSpectrum.from_flux(draw, DT)
    assert ps.counts is None
    sl = gadfly_amd.SpectralLikelihood(ps)
    floor = spectral.white_floor(30.0, DT)
    ll = sl.evaluate([kern], floor=floor)
    assert sl.last_power_ptr == ps._power_dev.data_ptr() == sl.power_device.data_ptr()
    S0, w0, Q, delta = spectral.kernel_parameters([kern])
    o = ref.likelihood("whittle", S0, w0, Q, delta, floor, ps.omega, ps.power)
    assert abs(ll[0] - o["ll"][0]) <= BAR_LL * o["ll_scale"][0] and sl.last_used[0] == N // 2
    # a band of the same spectrum: a view of the same device buffer
    band = gadfly_amd.SpectralLikelihood(ps, frequency_min=100.0, frequency_max=4000.0)
    keep = (ps.frequency >= 100.0) & (ps.frequency <= 4000.0)
    lb = band.evaluate([kern], floor=floor)
    ob = ref.likelihood("whittle", S0, w0, Q, delta, floor, ps.omega[keep], ps.power[keep])
    assert band.last_power_ptr == ps._power_dev.data_ptr() + 8 * int(np.argmax(keep))
    assert abs(lb[0] - ob["ll"][0]) <= BAR_LL * ob["ll_scale"][0] and band.last_used[0] == keep.sum()
    # binned: counts = the bin sizes, NaN bins skipped, both objectives from the spectrum's own error / counts
    binned = ps.bin(bins=40)
    _, start = _bin_starts(np.log10(ps.frequency), 40)
    assert np.array_equal(binned.counts, np.diff(start)) and binned.counts.sum() == len(ps.frequency)
    for objective, weight in (("whittle", binned.counts), ("chi2", binned.error)):
        sb = gadfly_amd.SpectralLikelihood(binned, objective=objective)
        l2 = sb.evaluate([kern], floor=floor)
        o2 = ref.likelihood(objective, S0, w0, Q, delta, floor, binned.omega, binned.power, weight)
        assert sb.last_used[0] == o2["used"][0] < 40
        assert abs(l2[0] - o2["ll"][0]) <= BAR_LL * o2["ll_scale"][0], objective


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_lbfgs_step(hip, objective):
    """One torch.optim.LBFGS step on log-parameters from 1.3 x the truth: the criterion of tests/test_gpu_grad.py."""
    N = 8192
    freq = np.fft.rfftfreq(N, DT)[1:]
    S0 = np.array([[40.0, 0.5, 0.02]])
    w0 = np.array([[60.0, 2500.0, 19000.0]])
    Q = np.array([[0.6, 0.6, 8.0]])
    floor = np.array([0.02])
    S = ref.model(S0, w0, Q, DT, floor, 2 * np.pi * freq, np.float64)[0]
    rng = np.random.default_rng(5)
    if objective == "whittle":
        ps = PowerSpectrum(freq, S * rng.exponential(size=S.shape))
    else:
        ps = PowerSpectrum(freq, S * (1.0 + 0.1 * rng.normal(size=S.shape)), error=0.1 * S)
    sl = gadfly_amd.SpectralLikelihood(ps, objective=objective)
    x = torch.tensor(np.log(np.concatenate([S0[0], w0[0], Q[0], floor]) * 1.3), requires_grad=True)
    opt = torch.optim.LBFGS([x], max_iter=50, line_search_fn="strong_wolfe")

    def nll():
        opt.zero_grad()
        e = torch.exp(x)
        loss = -gadfly_amd.SpectralLogLikelihood.apply(e[None, 0:3], e[None, 3:6], e[None, 6:9], e[9:10], sl, DT).sum()
        loss.backward()
        return loss

    l0 = nll().item()
    g0 = float(x.grad.norm())
    opt.step(nll)
    l1 = nll().item()
    g1 = float(x.grad.norm())
    print(f"LBFGS {objective}: l {l0:.6g} -> {l1:.6g}, |g| {g0:.3g} -> {g1:.3g} (ratio {g1 / g0:.2e})")
    assert l1 < l0 and g1 <= 1e-2 * g0, (l0, l1, g0, g1)

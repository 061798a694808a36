"""GPU: the spectral Fisher information (``gf_spectral_fisher``) against the longdouble oracle of
tests/spectral_fisher_ref.py -- boundary shapes, masks and awkward inputs, bit identity across batches and groups, the
failure path, ``wrt`` / ``log``, covariances -- and the batched fitter against the oracle's restatement of it.

The bar on every entry is |F_dev - F_longdouble| <= 1e-11 x scale, scale = sum_k v_k |d_i S_k| |d_j S_k| (the project's
gradient bar): a few tens of u per addend, up to slab / 4 sequential accumulator adds and the slab-order sum stay below
about 1e-13 x scale at the sizes here.  The worst ratios are printed (run with -s) and recorded in DESIGN.md."""
import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd.psd import PowerSpectrum
from tests import spectral_fisher_ref as fref
from tests import spectral_ref as ref

pytestmark = pytest.mark.gpu

DT = fref.DT
NYQUIST = fref.NYQUIST
BAR = 1e-11
OBJECTIVES = ("whittle", "chi2")

_BASE86 = None


# ---- the case generators of tests/test_gpu_spectral.py (a copy) ------------------------------------------------------
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


def _args(c, sel=slice(None)):
    return (c["S0"][sel], c["w0"][sel], c["Q"][sel], c["delta"][sel], None if c["floor"] is None else c["floor"][sel])


def _oracle(c, sel=slice(None)):
    power = c["power"] if c["power"].shape[0] == 1 else c["power"][sel]
    weight = c["weight"]
    if weight is not None and weight.shape[0] > 1:
        weight = weight[sel]
    return fref.fisher(c["objective"], *_args(c, sel), c["omega"], power, weight)


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _ratio(F, want, scale):
    """Worst |F - want| / scale over the entries (an entry of scale 0 must be exactly the oracle's 0)."""
    err = np.abs(F - want)
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1), err))) if F.size else 0.0


def _check_structure(Fd):
    """Exactly symmetric, diagonal >= 0 (a device tensor (B, P, P))."""
    assert torch.equal(Fd, Fd.transpose(1, 2))
    assert bool((torch.diagonal(Fd, dim1=1, dim2=2) >= 0).all())


def _slab(hip):
    return hip.load().gf_spectral_fisher_slab()


def _sizes(L):
    return (1, 2, 3, 4, 5, L - 1, L, L + 1, 2 * L + 3)


def _check_case(c, label):
    """One problem set against the oracle: the bar, the structure, used / info against a likelihood call's, and
    problem 0 alone against problem 0 in the batch.  Returns the worst ratio."""
    want, scale, used, info = _oracle(c)
    sl = _evaluator(c)
    Fd = sl.fisher_device(*_args(c))
    B, J = c["S0"].shape
    assert tuple(Fd.shape) == (B, 3 * J + 1, 3 * J + 1)
    fu, fi = sl.last_used, sl.last_info
    out = sl.run_device(*_args(c))
    assert np.array_equal(fu, out["used"].cpu().numpy()) and np.array_equal(fi, out["info"].cpu().numpy())
    assert np.array_equal(fu, used) and not fi.any() and not info.any()
    _check_structure(Fd)
    F = Fd.cpu().numpy()
    r = _ratio(F, want, scale)
    assert r <= BAR, (label, r)
    alone = sl.fisher(*_args(c, slice(0, 1)))
    assert np.array_equal(alone[0], F[0]), label
    return r


# ---- the tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(9))
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_boundary_shapes(hip, objective, which):
    """M in {1, 2, 3, 4, 5, L-1, L, L+1, 2L+3} x J in {1, 5, 6, 15, 16, 17, 33}, B = 3: P = 16 exactly (J = 5), a
    partial k-slice of 4, the edges of the term tiles."""
    M = _sizes(_slab(hip))[which]
    worst = 0.0
    for J in (1, 5, 6, 15, 16, 17, 33):
        worst = max(worst, _check_case(_case(100 * which + J, objective, 3, J, M), (objective, M, J)))
    print(f"boundary shapes {objective} M={M}: worst |F - truth| / scale {worst:.2e}")


@pytest.mark.parametrize("J,which", [(86, 4), (86, 7), (256, 4)])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_many_terms(hip, objective, J, which):
    """J = 86 (19 parameter tiles: the blocks of the tile triangle) at M in {5, L+1}, J = 256 at M = 5."""
    M = _sizes(_slab(hip))[which]
    r = _check_case(_case(900 + J + which, objective, 3, J, M), (objective, M, J))
    print(f"J={J} {objective} M={M}: worst |F - truth| / scale {r:.2e}")


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_masks_and_awkward_inputs(hip, objective):
    """omega = 0, delta = 0 and the cadence, floor None, an overdamped term, a Q = 1600 line, power per problem, NaN
    power at a slab's first and last frequency and across a whole slab, zero, NaN and negative weights."""
    L = _slab(hip)
    M = 2 * L + 3
    c = _case(7, objective, 3, 5, M, per_problem_power=True)
    c["floor"] = None
    c["power"][0, [L, 2 * L - 1]] = np.nan
    c["power"][1, L:2 * L] = np.nan
    c["power"][2, 0] = np.inf
    if c["weight"] is None:
        c["weight"] = np.tile(np.arange(1.0, M + 1.0) % 7 + 1.0, (3, 1))     # binned-spectrum-like counts
    c["weight"][2, [5, L + 1]] = 0.0
    c["weight"][2, 9] = np.nan
    c["weight"][0, 11] = -1.0
    want, scale, used, info = _oracle(c)
    assert list(used) == [M - 3, M - L, M - 4]
    sl = _evaluator(c)
    Fd = sl.fisher_device(*_args(c))
    assert np.array_equal(sl.last_used, used) and not sl.last_info.any()
    _check_structure(Fd)
    r = _ratio(Fd.cpu().numpy(), want, scale)
    print(f"masks {objective}: worst |F - truth| / scale {r:.2e}")
    assert r <= BAR
    # a p-mode of Q = 1600 whose centre sits on a frequency of the axis, and one between two frequencies
    c2 = _case(8, objective, 3, 2, L + 1)
    c2["w0"][0, -1] = c2["omega"][L // 2]
    c2["w0"][1, -1] = 0.5 * (c2["omega"][L // 3] + c2["omega"][L // 3 + 1])
    c2["Q"][:2, -1] = 1600.0
    r2 = _check_case(c2, "line centres")
    print(f"line centres {objective}: worst |F - truth| / scale {r2:.2e}")


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_all_frequencies_masked(hip, objective):
    L = _slab(hip)
    c = _case(9, objective, 3, 5, L + 1)
    c["power"][:] = np.nan
    sl = _evaluator(c)
    F = sl.fisher(*_args(c))
    assert np.all(F == 0.0) and np.all(sl.last_used == 0) and not sl.last_info.any()
    cov, ok = sl.covariance(*_args(c))
    assert not ok.any() and np.all(np.isnan(cov))


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_bit_identity(hip, objective):
    """A problem alone = inside B = 3 = under any group cap; two runs agree."""
    L = _slab(hip)
    M, J = 2 * L + 3, 33
    c = _case(21, objective, 3, J, M, per_problem_power=True)
    sl = _evaluator(c)
    F = sl.fisher(*_args(c))
    assert sl.last_plan[1:] == (1, 3)
    assert np.array_equal(sl.fisher(*_args(c)), F)
    per = sl.last_plan[0] // 3
    assert per == 8 * hip.load().gf_spectral_fisher_work(1, M, J)
    for cap, plan in ((per, (3, 1)), (2 * per + 8, (2, 2))):
        sl.workspace_bytes = cap
        assert np.array_equal(sl.fisher(*_args(c)), F)
        assert sl.last_plan[1:] == plan
    for b in range(3):
        alone = _evaluator(c, rows=slice(b, b + 1))
        assert np.array_equal(alone.fisher(*_args(c, slice(b, b + 1)))[0], F[b]), b


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_failure_is_isolated(hip, objective):
    """S0 = 0 with floor = 0 (S = 0 everywhere): the problem's matrix is NaN, info = first used index + 1 as the
    likelihood call reports it; the neighbours in the batch keep their bits."""
    L = _slab(hip)
    M = L + 5
    c = _case(31, objective, 3, 5, M, per_problem_power=True)
    c["floor"] = np.array([0.02, 0.0, 0.5])
    c["S0"][1] = 0.0
    c["power"][1, :3] = np.nan                                              # the first used frequency is k = 3
    want, scale, used, info = _oracle(c)
    assert info[1] == 4 and np.all(np.isnan(want[1]))
    sl = _evaluator(c)
    F = sl.fisher(*_args(c))
    fu, fi = sl.last_used, sl.last_info
    out = sl.run_device(*_args(c))
    assert list(fi) == [0, 4, 0] and np.array_equal(fi, out["info"].cpu().numpy())
    assert np.array_equal(fu, used) and np.array_equal(fu, out["used"].cpu().numpy())
    assert np.all(np.isnan(F[1]))
    # a failure in the second slab reports the index in the whole axis
    c["power"][1, :L + 2] = np.nan
    late = _evaluator(c)
    assert np.all(np.isnan(late.fisher(*_args(c))[1])) and late.last_info[1] == L + 3
    assert late.run_device(*_args(c))["info"].cpu().numpy()[1] == L + 3
    keep = [0, 2]
    assert _ratio(F[keep], want[keep], scale[keep]) <= BAR
    for b in keep:
        alone = _evaluator(c, rows=slice(b, b + 1))
        assert np.array_equal(alone.fisher(*_args(c, slice(b, b + 1)))[0], F[b]), b


def test_wrt_and_log(hip):
    """A selection is the index-selected full matrix, bit for bit; log=True is F theta theta^T within 4 u."""
    J, M = 5, 301
    c = _case(61, "whittle", 3, J, M)
    c["floor"] = np.array([0.02, 0.05, 0.5])
    sl = _evaluator(c)
    F = sl.fisher(*_args(c))
    theta = np.concatenate([c["S0"], c["w0"], c["Q"], c["floor"][:, None]], axis=1)
    for wrt in (("S0",), ("floor",), ("w0", "Q"), ("floor", "S0"), ("S0", "w0", "Q", "floor")):
        idx = gadfly_amd.spectral.parameter_index(wrt, J)
        got = sl.fisher(*_args(c), wrt=wrt)
        assert got.shape == (3, len(idx), len(idx))
        assert np.array_equal(got, F[:, idx][:, :, idx]), wrt
        logged = sl.fisher(*_args(c), wrt=wrt, log=True)
        th = theta[:, idx]
        want = got * th[:, :, None] * th[:, None, :]
        assert np.all(np.abs(logged - want) <= 4 * np.finfo(float).eps * np.abs(want)), wrt
    se = sl.standard_errors(*_args(c), wrt=("S0", "floor"))
    assert sorted(se) == ["S0", "floor"] and se["S0"].shape == (3, J) and se["floor"].shape == (3,)
    with pytest.raises(ValueError, match="log=True"):
        sl.fisher(c["S0"], c["w0"], c["Q"], c["delta"], None, log=True)


def _inverse_longdouble(F):
    """inv(F) in longdouble: the float64 inverse refined by Newton's X <- X (2 I - F X), three times."""
    F = F.astype(np.longdouble)
    X = np.linalg.inv(F.astype(np.float64)).astype(np.longdouble)
    I2 = 2 * np.eye(len(F), dtype=np.longdouble)
    for _ in range(3):
        X = X @ (I2 - F @ X)
    return X


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_covariance(hip, objective):
    """The fit case at its truth (cond of the scaled matrix about 3e3): |cov - inv(F_longdouble)|_ij / sqrt(cov_ii
    cov_jj) <= 1e-6, which is cond x the entry bar (3e-8) with 30 x margin.  A problem with one S0 = 0 (its w0 and Q
    rows are exactly zero) gets NaN and ok = False; its neighbours stay within the bar."""
    worst = 0.0
    for M in (64, 256):
        c = fref.fit_case(M, objective, False, 0)
        th = c["truth"]
        S0 = np.array([th[0:2], [0.0, th[1]], 1.1 * th[0:2]])
        w0 = np.array([th[2:4], th[2:4], 0.9 * th[2:4]])
        Q = np.array([th[4:6], th[4:6], 1.2 * th[4:6]])
        floor = np.array([th[6], th[6], 2 * th[6]])
        ps = PowerSpectrum(c["freq"], c["power"])
        sl = gadfly_amd.SpectralLikelihood(ps, objective=objective, weights=c["weight"])
        cov, ok = sl.covariance(S0, w0, Q, DT, floor)
        assert list(ok) == [True, False, True] and np.all(np.isnan(cov[1]))
        F = sl.fisher(S0, w0, Q, DT, floor)
        assert np.all(F[1, [2, 4]] == 0.0) and np.all(F[1][:, [2, 4]] == 0.0)
        want, _, _, _ = fref.fisher(objective, S0, w0, Q, DT, floor, c["omega"], c["power"], c["weight"])
        for b in (0, 2):
            truth = _inverse_longdouble(want[b])
            norm = np.sqrt(np.outer(np.diag(cov[b]), np.diag(cov[b])))
            worst = max(worst, float(np.max(np.abs(cov[b] - truth) / norm)))
            assert np.array_equal(cov[b], cov[b].T)
        d = np.sqrt(np.diag(F[0]))
        print(f"covariance {objective} M={M}: cond of the scaled matrix {np.linalg.cond(F[0] / np.outer(d, d)):.2e}")
        se = sl.standard_errors(S0, w0, Q, DT, floor)
        assert np.array_equal(se["S0"][0], np.sqrt(np.diag(cov[0])[0:2])) and se["floor"][2] == np.sqrt(cov[2][6, 6])
        assert np.all(np.isnan(se["w0"][1]))
    print(f"covariance {objective}: worst |cov - truth| / sqrt(cov_ii cov_jj) {worst:.2e}")
    assert worst <= 1e-6


def _fit_batch(M, objective):
    """The seven cases of one size and objective (exact data, then the seeds 0-5) as one batch with a spectrum row per
    problem."""
    cases = [k for k in fref.FIT_CASES if k[0] == M and k[1] == objective]
    cs = [fref.fit_case(*k) for k in cases]
    return cases, cs, np.array([c["power"] for c in cs]), np.array([c["weight"] for c in cs])


def _start(cs):
    st = np.array([c["start"] for c in cs])
    return st[:, 0:2], st[:, 2:4], st[:, 4:6], DT, st[:, 6]


def _flat(fit):
    return np.concatenate([fit.S0, fit.w0, fit.Q, fit.floor[:, None]], axis=1)


@pytest.mark.parametrize("M", [64, 256])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_fit(hip, objective, M):
    """The 28 fit cases in batches of seven (so the lockstep and the freezing are exercised): every problem converges
    within 60 iterations (the restatement needs at most 40); exact data give the truth to 1e-9, noisy data the
    restatement's result to 1e-6 with |g_u| at most 1e-8 of its starting value; cov_ok everywhere."""
    cases, cs, power, weight = _fit_batch(M, objective)
    sl = gadfly_amd.SpectralLikelihood(PowerSpectrum(cs[0]["freq"], power), objective=objective, weights=weight)
    fit = sl.fit(*_start(cs))
    print(f"fit {objective} M={M}: iterations {list(fit.iterations)}")
    assert fit.converged.all() and np.all(fit.iterations <= 60) and fit.cov_ok.all()
    assert fit.cov.shape == (7, 7, 7) and fit.ll.shape == (7,) and fit.S0.shape == (7, 2) and fit.floor.shape == (7,)
    got = _flat(fit)
    truth = cs[0]["truth"]
    _, g0 = sl.value_and_grad(*_start(cs))
    _, g1 = sl.value_and_grad(fit.S0, fit.w0, fit.Q, DT, fit.floor)
    gu0 = np.concatenate([g0[k].reshape(7, -1) for k in ("S0", "w0", "Q", "floor")], axis=1) \
        * np.array([c["start"] for c in cs])
    gu1 = np.concatenate([g1[k].reshape(7, -1) for k in ("S0", "w0", "Q", "floor")], axis=1) * got
    z = []
    for b, (case, c) in enumerate(zip(cases, cs)):
        if not c["noisy"]:
            rel = np.max(np.abs(got[b] / truth - 1))
            print(f"   exact data: largest relative distance from the truth {rel:.2e}")
            assert rel <= 1e-9
            continue
        theta, iterations, converged, _ = fref.reference_fit(case)
        rel = np.max(np.abs(got[b] / theta - 1))
        ratio = np.linalg.norm(gu1[b]) / np.linalg.norm(gu0[b])
        print(f"   seed {case[3]}: {fit.iterations[b]} iterations (restatement {iterations}), relative distance from "
              f"the restatement {rel:.2e}, |g_u| / |g_u at the start| {ratio:.2e}")
        assert converged and rel <= 1e-6 and ratio <= 1e-8
        z.append(np.max(np.abs(got[b] - truth) / np.sqrt(np.diag(fit.cov[b]))))
    print(f"   largest |fit - truth| / standard error over the seeds: {np.round(z, 2)}")


def test_fit_free_subset_and_a_dead_row(hip):
    """free = (S0, floor) leaves w0 and Q bitwise unchanged; a batch with one all-NaN spectrum row reports
    converged = False for that row and fits the others as the batch without it does (to 1e-9)."""
    cases, cs, power, weight = _fit_batch(64, "whittle")
    sl = gadfly_amd.SpectralLikelihood(PowerSpectrum(cs[0]["freq"], power), objective="whittle", weights=weight)
    S0, w0, Q, delta, floor = _start(cs)
    truth = cs[0]["truth"]
    w0t, Qt = np.tile(truth[2:4], (7, 1)), np.tile(truth[4:6], (7, 1))
    part = sl.fit(S0, w0t, Qt, delta, floor, free=("S0", "floor"))
    assert part.converged.all() and part.free == ("S0", "floor") and part.cov.shape == (7, 3, 3) and part.cov_ok.all()
    assert np.array_equal(part.w0, w0t) and np.array_equal(part.Q, Qt)
    assert np.max(np.abs(part.S0[0] / truth[0:2] - 1)) <= 1e-9 and abs(part.floor[0] / truth[6] - 1) <= 1e-9
    full = sl.fit(S0, w0, Q, delta, floor)
    dead = power.copy()
    dead[3] = np.nan
    sd = gadfly_amd.SpectralLikelihood(PowerSpectrum(cs[0]["freq"], dead), objective="whittle", weights=weight)
    fd = sd.fit(S0, w0, Q, delta, floor)
    keep = [0, 1, 2, 4, 5, 6]
    assert not fd.converged[3] and fd.converged[keep].all() and fd.iterations[3] == 0 and not fd.cov_ok[3]
    assert np.array_equal(_flat(fd)[3], np.exp(np.log(np.array(cs[3]["start"]))))
    without = gadfly_amd.SpectralLikelihood(PowerSpectrum(cs[0]["freq"], power[keep]), objective="whittle",
                                            weights=weight[keep])
    fw = without.fit(S0[keep], w0[keep], Q[keep], delta, floor[keep])
    assert np.max(np.abs(_flat(fd)[keep] / _flat(fw) - 1)) <= 1e-9
    assert np.max(np.abs(_flat(fd)[keep] / _flat(full)[keep] - 1)) <= 1e-9
    # a start of -inf (S0 = 0 under no floor, neither of them free): that row is frozen, the others go their way
    S0z, flz = S0.copy(), floor.copy()
    S0z[2], flz[2] = 0.0, 0.0
    fz = sl.fit(S0z, w0, Q, delta, flz, free=("w0", "Q"))
    assert not fz.converged[2] and fz.ll[2] == -np.inf and fz.iterations[2] == 0
    rest = [0, 1, 3, 4, 5, 6]
    fr = gadfly_amd.SpectralLikelihood(PowerSpectrum(cs[0]["freq"], power[rest]), objective="whittle",
                                                 weights=weight[rest]).fit(S0[rest], w0[rest], Q[rest], delta,
                                                                           floor[rest], free=("w0", "Q"))
    assert np.array_equal(fz.converged[rest], fr.converged) and np.array_equal(fz.iterations[rest], fr.iterations)
    assert np.max(np.abs(_flat(fz)[rest] / _flat(fr) - 1)) <= 1e-9

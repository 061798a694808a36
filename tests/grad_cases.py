"""Edge shapes of the gradient kernel shared by tests/test_grad_host.py and tests/test_gpu_grad_edges.py: raw
coefficient problems of any term structure (odd widths cannot be had from SHO terms: an overdamped one gives two real
terms), at the widths where k_grad's register layout changes and the lengths where its segments end."""
import numpy as np
import torch

from tests.grad_ref import dense_coefficient_loglike

#: (Jr, Jc): W = Jr + 2 Jc = 1, 2, 16, 16, 17, 32, 32, 33, 62, 63, 63 -- both sides of k_grad<16> | <32> | <64>, the
#: smallest and the largest widths, with and without real terms
STRUCTURES = ((1, 0), (0, 1), (2, 7), (0, 8), (1, 8), (2, 15), (0, 16), (1, 16), (0, 31), (1, 31), (3, 30))
#: N against the segments of K = ceil(sqrt(N)) rows: a single row (1); full last segments, N = K^2 (4, 16, 100); one
#: past a square, where K steps up (2, 5, 10, 17, 26, 101, 197: last segments of two rows); a last segment of
#: exactly one row, N = K (K - 1) + 1 (3, 13)
LENGTHS = (1, 2, 3, 4, 5, 10, 13, 16, 17, 26, 100, 101, 197)
DT = 60e-6


def edge_problem(Jr, Jc, N, B=3, seed=0):
    """B problems of different coefficients on one jittered one-minute axis with a gap in the middle (N > 6): dict with
    t (N,), y, diag (B, N), real (2, B, max(Jr, 1)), comp (4, B, max(Jc, 1)), diag_add (B,).  Complex terms are SHO
    terms (w0 50-1500, Q 0.7-20, S0 0.5-3), real ones a 10-500, c 5-800; white noise of 5-6 % of the amplitude
    amp = sum a on top of diag_add = amp, data of variance amp: conditions of a few tens."""
    rng = np.random.default_rng([seed, Jr, Jc, N])
    t = (np.arange(N) + rng.uniform(-0.2, 0.2, N)) * DT
    if N > 6:
        t[N // 2:] += 30 * DT
    real, comp = np.zeros((2, B, max(Jr, 1))), np.zeros((4, B, max(Jc, 1)))
    real[0, :, :Jr], real[1, :, :Jr] = rng.uniform(10.0, 500.0, (B, Jr)), rng.uniform(5.0, 800.0, (B, Jr))
    w0, Q, S0 = rng.uniform(50.0, 1500.0, (B, Jc)), rng.uniform(0.7, 20.0, (B, Jc)), rng.uniform(0.5, 3.0, (B, Jc))
    f = np.sqrt(4.0 * Q * Q - 1.0)
    a, c = S0 * w0 * Q, 0.5 * w0 / Q
    comp[0, :, :Jc], comp[1, :, :Jc], comp[2, :, :Jc], comp[3, :, :Jc] = a, a / f, c, c * f
    amp = np.sum(real[0, :, :Jr], axis=1) + np.sum(a, axis=1)
    diag = 0.05 * amp[:, None] + rng.uniform(0.0, 0.01, (B, N)) * amp[:, None]
    y = np.sqrt(amp)[:, None] * rng.normal(size=(B, N))
    return dict(t=t, y=y, diag=diag, real=real, comp=comp, diag_add=amp.copy(), Jr=Jr, Jc=Jc, N=N, B=B)


def coefficients(prob, b):
    """(ar, cr, ac, bc, cc, dc) of problem b, unpadded."""
    Jr, Jc = prob["Jr"], prob["Jc"]
    return tuple(prob["real"][i, b, :Jr] for i in range(2)) + tuple(prob["comp"][i, b, :Jc] for i in range(4))


def scaled_error(theta, got, ref):
    """max |theta g - theta g_ref| / max(1, max |theta g_ref|) of one coefficient array: the error of the gradient
    with respect to log theta against its largest entry (0 for an empty array)."""
    theta, got, ref = (np.asarray(x, dtype=np.float64) for x in (theta, got, ref))
    if theta.size == 0:
        return 0.0
    a, r = theta * got, theta * ref
    return float(np.max(np.abs(a - r)) / max(1.0, float(np.max(np.abs(r)))))


NAMES = ("ar", "cr", "ac", "bc", "cc", "dc")


def dense_grad(prob, b):
    """(ll, dict of the six coefficient adjoints + diag_add + mean) of problem b of a grad_cases.edge_problem by
    autograd through the dense log-likelihood."""
    co = [torch.tensor(x, requires_grad=True) for x in coefficients(prob, b)]
    mean = torch.zeros((), dtype=torch.float64, requires_grad=True)
    shift = torch.zeros((), dtype=torch.float64, requires_grad=True)
    ll = dense_coefficient_loglike(prob["t"], prob["y"][b], prob["diag"][b], prob["Jr"], prob["Jc"], *co,
                                   float(prob["diag_add"][b]), mean, shift)
    gr = torch.autograd.grad(ll, co + [mean, shift], allow_unused=True)
    g = {k: (np.zeros(len(c)) if v is None else v.numpy()) for k, c, v in zip(NAMES, co, gr)}
    g["mean"], g["diag_add"] = gr[6].item(), gr[7].item()
    return ll.item(), g

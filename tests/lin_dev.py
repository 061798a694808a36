"""TEST INFRASTRUCTURE (GPU tests only): device plumbing of tests/test_gpu_chunk_linear.py,
test_gpu_chunk_linear_combine.py and test_gpu_chunk_transition.py -- uploads with sentinel guards, the raw calls,
per-problem errors against tests/lin_ref.py."""
import numpy as np
import torch

from tests import lin_cases as C
from tests import lin_ref as R

SENTINEL = -7.25e77                  # what every output holds before a call: no result of these problems
GUARD = 192                          # doubles in front of and behind every guarded array
TAIL = 8                             # rows the transition sweep may read past the end of its row arrays


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


class Guarded:
    """A device array of ``n`` doubles between two runs of GUARD sentinels; ``fill``: what it holds before a call."""

    def __init__(self, n, fill=SENTINEL):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float64).reshape(-1)))
        elif fill != SENTINEL:
            self.t.fill_(fill)

    def host(self):
        """The array on the host, after checking that the guards still hold the sentinel."""
        b = self.buf.cpu().numpy()
        assert np.all(b[:GUARD] == SENTINEL) and np.all(b[-GUARD:] == SENTINEL), "a guard was overwritten"
        return b[GUARD:-GUARD].copy()


class DevRows:
    """The stored rows of a case on the device: c [B][W], Ut, Wt [B * N + TAIL][64], d, de [B * N + TAIL] (the tail:
    zeros, d = 1, or ``tail`` everywhere), problems ``sel`` only."""

    def __init__(self, rows, sel=None, tail=None):
        sel = list(range(rows["c"].shape[0])) if sel is None else sel
        self.B, self.N, self.W = len(sel), rows["d"].shape[1], rows["c"].shape[1]
        n = self.B * self.N

        def up(x, width, pad):
            a = np.full((n + TAIL,) + ((width,) if width else ()), pad if tail is None else tail)
            a[:n] = x[sel].reshape((n,) + ((width,) if width else ()))
            return dev(a)

        self.host = {k: v[sel] for k, v in rows.items()}
        self.c = dev(rows["c"][sel])
        self.Ut, self.Wt = up(rows["Ut"], 64, 0.0), up(rows["Wt"], 64, 0.0)
        self.d, self.de = up(rows["d"], 0, 1.0), up(rows["de"], 0, 0.0)


def nchunks(N, L):
    return -(-N // L)


def linear(hip, mode, dr, L, R, scale, store, Y, Z, F, check=True):
    """gf_chunk_linear on device tensors; returns the status."""
    lib, p = hip.load(), hip.ptr
    rc = lib.gf_chunk_linear(mode, dr.B, dr.N, L, nchunks(dr.N, L), dr.W, R, scale, store, p(dr.c), p(dr.Ut),
                             p(dr.Wt), p(dr.d), p(dr.de), p(Y), p(Z), p(F), None)
    if check:
        hip.check(rc, "gf_chunk_linear")
        torch.cuda.synchronize()
    return rc


def errors(got, ref, axis, floor=1.0):
    """[B] scaled errors max |got - ref| / max(floor, max |ref|) per problem (problem axis ``axis``), in 80 bits."""
    ref = np.moveaxis(np.asarray(ref, dtype=R.LD), axis, 0)
    got = np.moveaxis(np.asarray(got, dtype=R.LD), axis, 0)
    B = ref.shape[0]
    e = np.max(np.abs(got - ref).reshape(B, -1), axis=1)
    return (e / np.maximum(R.LD(floor), np.max(np.abs(ref).reshape(B, -1), axis=1))).astype(np.float64)


def judge(worst, key, what, got, ref, ref64, axis, W, gam, floor=1.0):
    """Per problem: the device's error against the bar max(100 x float64 restatement, W eps gamma).  ``floor`` = 0:
    errors relative to the largest element of the reference, however small (results far below 1)."""
    e, e64 = errors(got, ref, axis, floor), errors(ref64, ref, axis, floor)
    for b in range(len(e)):
        worst.add(key, what + (b,), float(e[b]), C.bar(float(e64[b]), W, float(np.atleast_1d(gam)[b % np.size(gam)])))

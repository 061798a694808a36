"""Shared cases of the group phase of the steady tail's finishing launch (not a conftest): the cases of
tests/steady_cases.py on a longer series -- the same forced switch at ANCHOR, tiles of T rows, seed 47 --, so that a
tail crosses the boundaries of the groups of 16 blocks in which k_steady_finish forms u = H y: tails of up to 2113 rows,
two full groups, a block and a row.  J = 1, 2 (the narrowest instances), 30 (the flagship's) and 31 (the widest)."""
import functools
from types import SimpleNamespace

import numpy as np

from tests.random_cases import oracle_loglikes
from tests.steady_cases import B_FIN, SW, _fast_terms, _series, oracle_rows, tail_sums

GROUP = 16              # blocks per group: the N dimension of the f64 MFMA
LONGEST_G = 2113        # two groups (2048 rows), a block and a row
N_G = SW + LONGEST_G
J_GROUP = (1, 2, 30, 31)
# a lone partial block; exactly one group; a group and a row; a partial group of one full block and of one block and a
# row (behind one full group); two groups; past two groups -- and their neighbours
TAILS_G = (1, 64, 65, 1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049, LONGEST_G)


@functools.lru_cache(maxsize=None)
def series():
    return _series(N_G, seed=47)


@functools.lru_cache(maxsize=None)
def case(J):
    """tests/steady_cases.py::case on the long series: B_FIN kernels of J terms, the oracle's d, z and log-likelihood,
    max |z| and the sums of every tail of 1 .. LONGEST_G rows.  Computed once per J and shared: nobody writes to it."""
    t, y = series()
    hps = [_fast_terms(J, k0) for k0 in range(B_FIN)]
    rows = [oracle_rows(hp, t, y) for hp in hps]            # (asserts info == 0 and the switch at ANCHOR)
    coeffs = [r.co for r in rows]
    ll, info = oracle_loglikes(coeffs, t, np.full(N_G, 900.0), y)
    assert np.all(info == 0)
    d, z = np.stack([r.d for r in rows]), np.stack([r.z for r in rows])
    for a in (d, z, ll):
        a.setflags(write=False)
    return SimpleNamespace(J=J, hps=hps, t=t, y=y, rows=rows, coeffs=coeffs, d=d, z=z, loglike=ll,
                           zmax=np.max(np.abs(z), axis=1),
                           sums=[tail_sums(d[b], z[b], longest=LONGEST_G) for b in range(B_FIN)])

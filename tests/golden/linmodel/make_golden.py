"""Writes tests/golden/linmodel/walkers_dense80.npz: [A | y]^T Sigma^-1 [A | y] and log det Sigma of the five walkers
of tests/linmodel_ref.walkers() from the DENSE matrix in 80-bit arithmetic (tests/linmodel_ref.dense_K_ld,
dense_gram_ld; about twenty seconds), each value as a float64 pair hi + lo.  Run from the repository root:
    python tests/golden/linmodel/make_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import linmodel_ref as lr  # noqa: E402


def split(x):
    x = np.asarray(x, dtype=np.longdouble)
    hi = x.astype(np.float64)
    return hi, (x - hi.astype(np.longdouble)).astype(np.float64)


def main():
    w = lr.walkers()
    amp = [np.sum(co[0]) + np.sum(co[2]) for co in w["co"]]
    noise = [w["yerr"] ** 2 + w["diag_add"][b] - amp[b] for b in range(w["B"])]
    Ks = lr.dense_K_ld(w["co"], w["t"], noise)
    out = [lr.dense_gram_ld(K, w["A"], w["y"][b]) for b, K in enumerate(Ks)]
    ghi, glo = split(np.stack([o[0] for o in out]))
    lhi, llo = split(np.array([o[1] for o in out]))
    np.savez(os.path.join(ROOT, "tests", "golden", "linmodel", "walkers_dense80.npz"), gram_hi=ghi, gram_lo=glo,
             logdet_hi=lhi, logdet_lo=llo, y_check=w["y"][:, ::97])


if __name__ == "__main__":
    main()

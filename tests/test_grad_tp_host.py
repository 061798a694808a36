"""CPU: the time-parallel gradient's algebra in numpy (tests/grad_tp_ref.py) against the sequential
numpy pass (tests/grad_ref.py) at the edge shapes of tests/grad_cases.py: the plain-coordinate chunk maps through
oracle/lft.py reproduce the sequential state at every chunk boundary, the two scans give the adjoint sweep 3 returns
at every boundary, and log L and every adjoint agree with the sequential pass."""
import numpy as np
import pytest

from tests import grad_cases as gc
from tests.grad_ref import loglike_grad
from tests.grad_tp_ref import loglike_grad_chunked, sequential_states

#: (N, chunk_len): a short last chunk (197 = 12 * 16 + 5), four chunks, one row per chunk, a last chunk of one row,
#: full chunks only, nine chunks with a last one of four rows
SHAPES = ((197, 16), (197, 50), (100, 1), (101, 100), (64, 8), (300, 37))


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b)))))


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_chunked_pass_matches_the_sequential_one(Jr, Jc):
    worst = [0.0, 0.0, 0.0, 0.0]
    for N, L in SHAPES:
        prob = gc.edge_problem(Jr, Jc, N, B=1, seed=3)
        co = gc.coefficients(prob, 0)
        args = (prob["t"], prob["y"][0], prob["diag"][0], Jr, Jc, *co, prob["diag_add"][0])
        ll0, g0 = loglike_grad(*args)
        ll1, g1, st = loglike_grad_chunked(*args, L)
        assert len(st["bounds"]) == -(-N // L)
        # the maps through lft.start_states: the sequential (M, H) at every boundary
        for (X, Y), (Xs, Ys) in zip(st["starts"][1:], sequential_states(st, prob["y"][0])[1:]):
            worst[0] = max(worst[0], _rel(X, Xs), _rel(Y, Ys))
        # sweep 3's start adjoints: the scans' values of the chunk before
        for i in range(1, len(st["bounds"])):
            worst[1] = max(worst[1], _rel(st["Min"][i], st["Mout"][i - 1]), _rel(st["Hin"][i], st["Hout"][i - 1]))
        worst[2] = max(worst[2], abs(ll1 - ll0) / abs(ll0))
        adj = [gc.scaled_error(c_, g1[k], g0[k]) for k, c_ in zip(gc.NAMES, co)]
        adj += [abs(g1[k] - g0[k]) / max(1.0, abs(g0[k])) for k in ("mean", "diag_add")]
        worst[3] = max(worst[3], *adj)
    print(f"(Jr, Jc) = ({Jr}, {Jc}): boundary states {worst[0]:.1e}, boundary adjoints {worst[1]:.1e}, "
          f"log L {worst[2]:.1e}, adjoints {worst[3]:.1e}")
    assert worst[0] < 1e-10 and worst[1] < 1e-10 and worst[2] < 1e-10 and worst[3] < 1e-10, worst

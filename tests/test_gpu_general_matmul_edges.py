"""GPU: gf_general_matmul (the conditional mean at new times) through its raw C entry point: the sequential kernel
k_gmm<1|2|4> at lengths around its blocks of eight rows, and the chunk-parallel kernels k_gmm_chunk / k_gmm_scan at one
chunk, two, two ragged, three, four per problem and where the cap 1024 / B forces a single one -- with queries before
the first and after the last observed time, exactly on the first and last row of every chunk and between them,
repeated, all on one side, all inside one chunk, and a single one (tests/sweep_cases.query_set).  mu and the whole
workspace are NaN before the call; every mu[m] must come back finite and within 1e-10 of the largest entry of
oracle/cref.py's general_matmul in float64."""
import numpy as np
import pytest
import torch

from tests import sweep_cases as sc
from tests.sweep_dev import SENTINEL, dev, stack

pytestmark = pytest.mark.gpu


def _general_matmul(hip, refs, t1, shared):
    """One call for the problems ``refs`` at the query times t1 ((M,) shared by all problems -- the observed axis is
    then shared too, both with stride 0 -- or (B, M) with strides M and N).  Returns (mu (B, M), reference (B, M))."""
    lib, p = hip.load(), hip.ptr
    B, (N, W) = len(refs), refs[0]["U"].shape
    ld = sc.leading_dim(W)
    M = t1.shape[-1]
    alpha = np.stack([sc.rhs(N, 1, seed=30 + b)[:, 0] for b in range(B)])
    want, U1, V1, qidx = [], [], [], []
    for b, ref in enumerate(refs):
        tq = t1 if shared else t1[b]
        mu, u1, v1 = sc.general_matmul_reference(ref, tq, alpha[b])
        want.append(mu), U1.append(sc.pad(u1, ld)), V1.append(sc.pad(v1, ld))
        qidx.append(sc.qidx_of(ref["t"], tq))
    need = int(lib.gf_general_matmul_work(B, M, N, W))
    assert need == sc.gmm_work(B, M, N, W), (B, M, N, W)
    work = torch.full((need + 1,), float("nan"), dtype=torch.float64, device="cuda")
    work[need] = SENTINEL
    mu = torch.full(((B + 1) * M,), float("nan"), dtype=torch.float64, device="cuda")
    mu[B * M:] = SENTINEL
    t2 = refs[0]["t"] if shared else stack(refs, "t")
    dv = [dev(x) for x in (stack(refs, "c"), t1, np.stack(U1), np.stack(V1), t2, stack(refs, "U", ld),
                           stack(refs, "V", ld), stack(refs, "P", ld, 1.0), alpha)]
    qd = dev(np.stack(qidx), dtype=np.int64)
    c, t1d, U1d, V1d, t2d, U2d, V2d, P2d, ad = (p(x) for x in dv)
    rc = lib.gf_general_matmul(B, M, N, W, ld, c, t1d, 0 if shared else M, U1d, V1d, t2d, 0 if shared else N, U2d,
                               V2d, P2d, ad, p(qd), p(work), p(mu), None)
    hip.check(rc, "gf_general_matmul")
    torch.cuda.synchronize()
    got = mu.cpu().numpy()
    assert np.all(got[B * M:] == SENTINEL) and work[need].item() == SENTINEL
    return got[:B * M].reshape(B, M), np.array(want)


def _check(hip, refs, name, own, worst, bad, tag):
    B = len(refs)
    if own:
        t1 = np.stack([sc.query_set(name, r["t"], B) for r in refs])
    else:
        t1 = sc.query_set(name, refs[0]["t"], B)
    got, want = _general_matmul(hip, refs, t1, shared=not own)
    assert np.all(np.isfinite(got)), (tag, name, own)
    for b in range(B):
        err = sc.relerr(got[b], want[b])
        if err > worst[0]:
            worst[0], worst[1] = err, name
        if not err <= sc.TOL:
            bad.append((tag, name, own, b, err))


@pytest.mark.parametrize("W", [1, 64, 65, 128, 129, 256])
def test_sequential_kernel(hip, W):
    """N in {1, 7, 8, 9, 17, 70}, the full query set, B = 3 on per-problem axes (strides M and N) and on shared ones
    (stride 0)."""
    worst, bad = [0.0, ""], []
    for N in (1, 7, 8, 9, 17, 70):
        for own in (True, False):
            refs = sc.reference(*sc.structure_of(W), N, 3, own_axes=own)
            assert sc.gmm_chunking(3, N)[0] == 1
            _check(hip, refs, "full", own, worst, bad, N)
    print(f"gf_general_matmul sequential W = {W}: worst {worst[0]:.1e} ({worst[1]})")
    assert not bad, bad


@pytest.mark.parametrize("N", [511, 512, 513, 769])
@pytest.mark.parametrize("W", [17, 65, 129])
def test_chunked_kernels(hip, W, N):
    """One chunk (N = 511, the sequential kernel), two, two ragged, three; every named query set."""
    worst, bad = [0.0, ""], []
    refs = sc.reference(*sc.structure_of(W), N, 1)
    assert sc.gmm_chunking(1, N)[0] == {511: 1, 512: 2, 513: 2, 769: 3}[N]
    for name in sc.QUERY_SETS:
        _check(hip, refs, name, False, worst, bad, N)
    print(f"gf_general_matmul chunked W = {W}, N = {N}: worst {worst[0]:.1e} ({worst[1]})")
    assert not bad, bad


@pytest.mark.parametrize("W", [17, 65, 129])
def test_four_chunks_per_problem_of_five(hip, W):
    """B = 5 at N = 1024, per-problem and shared axes: blockIdx.z = chunk, the slots of (problem, direction, chunk)."""
    worst, bad = [0.0, ""], []
    assert sc.gmm_chunking(5, 1024) == (4, 256)
    for own in (True, False):
        refs = sc.reference(*sc.structure_of(W), 1024, 5, own_axes=own)
        for name in sc.QUERY_SETS:
            _check(hip, refs, name, own, worst, bad, 1024)
    print(f"gf_general_matmul B = 5, N = 1024, W = {W}: worst {worst[0]:.1e} ({worst[1]})")
    assert not bad, bad


def test_cap_forces_a_single_chunk(hip):
    """B = 600 at N = 520, W = 2: 1024 / B = 1 chunk, so the sequential kernel runs a series it would otherwise cut."""
    worst, bad = [0.0, ""], []
    assert sc.gmm_chunking(600, 520) == (1, 520) and sc.gmm_chunking(1, 520)[0] == 2
    refs = sc.reference(0, 1, 520, 600)
    for name in sc.QUERY_SETS:
        _check(hip, refs, name, False, worst, bad, 520)
    print(f"gf_general_matmul B = 600, N = 520, W = 2: worst {worst[0]:.1e} ({worst[1]})")
    assert not bad, bad

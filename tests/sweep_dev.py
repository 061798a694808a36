"""Device side of the sweep edge tests (test_gpu_sweep_edges.py, test_gpu_solve_chunk_edges.py,
test_gpu_general_matmul_edges.py, test_gpu_fused_rows.py): the oracle's factor of tests/sweep_cases.reference on the
device, and raw calls of gf_solve / gf_solve_chunk[_rhs] whose outputs are one problem too long and pre-filled with a
sentinel that must survive past the end."""
import numpy as np
import torch

from tests import sweep_cases as sc

SENTINEL = -7.25e77                  # what every output holds before a call: no result of these problems
INFO_SENTINEL = -77


def dev(x, dtype=np.float64):
    return torch.as_tensor(np.array(x, dtype=dtype, order="C")).cuda()      # (a copy: the references are read-only)


def sentinel(n):
    return torch.full((int(n),), SENTINEL, dtype=torch.float64, device="cuda")


def zeroed_with_sentinel(n, extra):
    """n zeros (a state the caller must zero) with ``extra`` sentinel elements behind them."""
    buf = sentinel(n + extra)
    buf[:n] = 0.0
    return buf


def info_with_sentinel(B):
    """B zeroed info entries and one more that holds INFO_SENTINEL."""
    info = torch.full((B + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    info[:B] = 0
    return info


def take_info(info, B, what=""):
    x = info.cpu().numpy()
    assert x[B] == INFO_SENTINEL, f"{what}: info written past the end"
    return x[:B].copy()


def take(buf, n, what=""):
    """The first n elements of a sentinel-filled output on the host; the rest must still hold the sentinel."""
    x = buf.cpu().numpy()
    assert np.all(x[n:] == SENTINEL), f"{what}: written past the end"
    return x[:n].copy()


def stack(refs, key, ld=None, fill=0.0):
    """(B, N[, ld]) host array of one entry of every problem, padded to ld columns."""
    return np.stack([r[key] if ld is None else sc.pad(r[key], ld, fill) for r in refs])


class Factor:
    """The oracle's U, V, W, P (padded to ld; pads 0, 1 for P) and d of B problems on the device."""

    def __init__(self, refs):
        self.refs = refs
        self.B, (self.N, self.W) = len(refs), refs[0]["U"].shape
        self.ld = sc.leading_dim(self.W)
        self.U, self.V, self.Wm = (dev(stack(refs, k, self.ld)) for k in ("U", "V", "W"))
        self.P = dev(stack(refs, "P", self.ld, 1.0))
        self.d = dev(stack(refs, "d"))

    def only(self, b):
        """The factor of problem b alone (views: no copy)."""
        f = object.__new__(Factor)
        f.refs, f.B, f.N, f.W, f.ld = self.refs[b:b + 1], 1, self.N, self.W, self.ld
        f.U, f.V, f.Wm, f.P, f.d = (x[b:b + 1] for x in (self.U, self.V, self.Wm, self.P, self.d))
        return f


def solve(hip, mode, fac, Y, scaled, inplace=False):
    """gf_solve on the host right-hand sides Y (B, N, R): Z (B, N, R).  inplace: Z aliases Y."""
    lib, p = hip.load(), hip.ptr
    B, N, R = Y.shape
    assert (B, N) == (fac.B, fac.N)
    Z = sentinel((B + 1) * N * R)
    if inplace:
        Z[:B * N * R] = dev(Y).reshape(-1)
        Yd = Z
    else:
        Yd = dev(Y)
    rc = lib.gf_solve(mode, B, N, fac.W, fac.ld, R, p(fac.U), p(fac.Wm), p(fac.P), p(fac.d) if scaled else None,
                      p(Yd), p(Z), None)
    hip.check(rc, "gf_solve")
    torch.cuda.synchronize()
    return take(Z, B * N * R, "gf_solve").reshape(B, N, R)


def solve_chunk(hip, mode, fac, Y, scaled, chunk_len, states, store, multi):
    """gf_solve_chunk (multi = False: Y (B, N, 1)) or gf_solve_chunk_rhs on host arrays: ``states`` (B, nch, W, R)
    are the start states, padded here to [B * nch][ld][R] (pad rows 0).  Returns (Z (B, N, R) -- still all sentinel
    when store = 0 --, end states (B, nch, W, R)); pad rows of the states must come back 0, the slot past the last
    one untouched."""
    lib, p = hip.load(), hip.ptr
    B, N, R = Y.shape
    nch = states.shape[1]
    W, ld = fac.W, fac.ld
    S = np.zeros((B, nch, ld, R))
    S[:, :, :W] = states
    Sd = sentinel((B * nch + 1) * ld * R)
    Sd[:B * nch * ld * R] = dev(S).reshape(-1)
    Z = sentinel((B + 1) * N * R)
    Yd = dev(Y)
    sd = p(fac.d) if scaled else None
    if multi:
        rc = lib.gf_solve_chunk_rhs(mode, B, N, chunk_len, nch, W, ld, R, p(fac.U), p(fac.Wm), p(fac.P), sd, p(Yd),
                                    p(Z), p(Sd), store, None)
    else:
        assert R == 1
        rc = lib.gf_solve_chunk(mode, B, N, chunk_len, nch, W, ld, p(fac.U), p(fac.Wm), p(fac.P), sd, p(Yd), p(Z),
                                p(Sd), store, None)
    hip.check(rc, "gf_solve_chunk")
    torch.cuda.synchronize()
    out = take(Sd, B * nch * ld * R, "F_state").reshape(B, nch, ld, R)
    assert not np.any(out[:, :, W:]), "pad rows of the chunk states"
    Zh = Z.cpu().numpy()
    assert np.all(Zh[B * N * R:] == SENTINEL), "Z: written past the end"
    return Zh[:B * N * R].reshape(B, N, R), out[:, :, :W]

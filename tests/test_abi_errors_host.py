"""CPU: every argument check of the entry points defined in gadfly_hip.hip, gadfly_stored.hip, gadfly_linear.hip and
gadfly_series.hip, and of gf_dense_solve (gadfly_dense.hip), by exact status and exact gf_last_error() text.

A case whose pointers are all NULL can never reach a launch: every entry point refuses NULL required pointers at
the latest.  A case that has to pass the NULL check hands over the dummy address `D`; it runs only where there is
no device (as test_no_gpu_fails_loudly does), where a mistaken launch is a -2 status and a failed assertion.
Messages no caller can reach are not listed: the "internal dispatch error"s (every supported width has an
instance) and "acc goes with the steady sweep alone" (the one entry point that passes acc runs without the tail).
"""
import ctypes

import pytest

from gadfly_amd import _lib

D = ctypes.c_void_p(0x1000)         # never dereferenced: see above
Z = None
COLUMN, TILED, ZERO_START, LONG_SPAN = 1, 2, 0x100, 0x200
BIG = 1 << 50


def sweep(B=1, N=16, n_first=0, Jr=0, Jc=2, block=8, gen=1, variant=0, p=Z, y_bs=0, tail=()):
    """The arguments the streamed sweeps share, `tail` between info and the stream."""
    return (B, N, n_first, Jr, Jc, block, gen, variant) + (p,) * 8 + (p, 0, p, 0, p, y_bs) + (p,) * 5 + tail + (Z,)


def chunk_sweep(B=1, N=128, chunk_len=64, nch=2, first=0, count=2, Jr=0, Jc=2, block=8, gen=1, variant=0, p=Z,
                rows=(Z, Z, Z, Z)):
    return ((B, N, chunk_len, nch, first, count, Jr, Jc, block, gen, variant) + (p,) * 8 + (p, 0, p, 0, p, 0)
            + (p, p) + rows + (p, p, p) + (Z,))


def finish(B=1, N=16, Jr=0, Jc=2, block=8, variant=0, p=Z, tail=()):
    return (B, N, Jr, Jc, block, variant) + (p,) * 5 + (p, 0, p, 0) + (p,) * 3 + tail + (Z,)


def transition(B=1, N=128, chunk_len=64, nch=2, first=0, count=2, Jr=0, Jc=2, variant=0, p=Z):
    return (B, N, chunk_len, nch, first, count, Jr, Jc, variant) + (p,) * 9 + (Z,)


def transition_wide(B=1, N=128, chunk_len=64, nch=2, first=0, count=2, Jc=40, p=Z):
    return (B, N, chunk_len, nch, first, count, Jc) + (p,) * 7 + (Z,)


def build_matrices(B=1, N=16, n_first=0, Jr=0, Jc=2, ld=16, p=Z, a=Z):
    return (B, N, n_first, Jr, Jc, ld) + (Z,) * 7 + (p, 0, Z, 0) + (a, p, p, Z) + (Z,)


def build_scaled(B=1, N=16, n_first=0, Jr=0, Jc=2, ld=16, block=8, p=Z):
    return (B, N, n_first, Jr, Jc, ld) + (p,) * 8 + (block,) + (p, 0, p, 0) + (p,) * 4 + (Z,)


def factor(B=1, N=16, W=4, ld=16, p=Z, y=Z, z=Z, S=Z, F=Z):
    return (B, N, 0, W, ld) + (p,) * 4 + (y, 0) + (p, p, z, S, F, p) + (Z,)


def factor_scaled(B=1, N=16, W=4, ld=16):
    return (B, N, 0, W, ld) + (Z,) * 5 + (Z, 0) + (Z,) * 5 + (Z,)


def chunk_linear(mode=0, B=1, N=128, chunk_len=64, nch=2, W=4, R=1):
    return (mode, B, N, chunk_len, nch, W, R, 0, 0) + (Z,) * 8 + (Z,)


def solve_chunk(mode=0, B=1, N=128, chunk_len=64, nch=2, W=4, ld=16, p=Z):
    return (mode, B, N, chunk_len, nch, W, ld) + (p,) * 7 + (0, Z)


def solve_chunk_rhs(mode=0, B=1, N=128, chunk_len=64, nch=2, W=4, ld=16, R=2, p=Z):
    return (mode, B, N, chunk_len, nch, W, ld, R) + (p,) * 7 + (0, Z)


def solve(mode=0, B=1, N=16, W=4, ld=16, R=1, p=Z):
    return (mode, B, N, W, ld, R) + (p,) * 6 + (Z,)


def cross(B=1, N=16, R=4, Jr=0, Jc=2, p=Z):
    return (B, N, R, Jr, Jc) + (p,) * 6 + (p, 0, p, 0, p, Z)


def matmul(B=1, M=8, N=16, W=4, ld=16):
    return (B, M, N, W, ld, Z, Z, 0, Z, Z, Z, 0) + (Z,) * 8


STEADY = (D, 0)
REDUCED = (D, 0, D, 1)
RANK1 = (D, 0, D, 1, D)
W65 = dict(Jr=1, Jc=32)
WIDE_CHUNKS = dict(N=64 << 20, chunk_len=64, nch=1 << 20)

# (entry point, arguments, status, gf_last_error() -- None where the call succeeds without a launch)
CASES = [
    ("gf_build_matrices", build_matrices(B=0), -1, "gf_build_matrices: empty problem (B=0, N=16)"),
    ("gf_build_matrices", build_matrices(Jc=129), -1, "gf_build_matrices: width 258 unsupported (max 256)"),
    ("gf_build_matrices", build_matrices(ld=8), -1, "gf_build_matrices: ld=8 must be a multiple of 16 and >= W=4"),
    ("gf_build_matrices", build_matrices(ld=24), -1, "gf_build_matrices: ld=24 must be a multiple of 16 and >= W=4"),
    ("gf_build_matrices", build_matrices(), -1, "gf_build_matrices: null pointer"),
    ("gf_build_matrices", build_matrices(p=D, a=D), -1, "gf_build_matrices: null pointer"),
    ("gf_build_matrices", build_matrices(n_first=-1, p=D), -1, "gf_build_matrices: negative n_first"),
    ("gf_build_matrices", build_matrices(N=BIG, p=D), -1, "gf_build_matrices: problem too large"),

    ("gf_factor", factor(N=0), -1, "gf_factor: empty problem (B=1, N=0)"),
    ("gf_factor", factor(W=300, ld=304), -1, "gf_factor: width 300 unsupported (max 256)"),
    ("gf_factor", factor(W=20, ld=16), -1, "gf_factor: ld=16 must be a multiple of 16 and >= W=20"),
    ("gf_factor", factor(), -1, "gf_factor: null pointer"),
    ("gf_factor", factor(p=D, z=D), -1, "gf_factor: z requested without y"),
    ("gf_factor", factor(p=D, F=D), -1, "gf_factor: F_state without S_state"),

    ("gf_build_scaled", build_scaled(B=-1), -1, "gf_build_scaled: empty problem (B=-1, N=16)"),
    ("gf_build_scaled", build_scaled(Jc=97, ld=208), -1, "gf_build_scaled: width 194 unsupported"),
    ("gf_build_scaled", build_scaled(ld=20), -1, "gf_build_scaled: ld=20 must be a multiple of 16 and >= W=4"),
    ("gf_build_scaled", build_scaled(block=3), -1, "gf_build_scaled: block=3 must be a power of two in 1..64"),
    ("gf_build_scaled", build_scaled(block=128), -1, "gf_build_scaled: block=128 must be a power of two in 1..64"),
    ("gf_build_scaled", build_scaled(n_first=3), -1,
     "gf_build_scaled: n_first=3 must be a non-negative multiple of block=8"),
    ("gf_build_scaled", build_scaled(n_first=-8), -1,
     "gf_build_scaled: n_first=-8 must be a non-negative multiple of block=8"),
    ("gf_build_scaled", build_scaled(), -1, "gf_build_scaled: null pointer"),
    ("gf_build_scaled", build_scaled(N=BIG, p=D), -1, "gf_build_scaled: problem too large"),

    ("gf_factor_scaled", factor_scaled(B=0, N=0), -1, "gf_factor_scaled: empty problem (B=0, N=0)"),
    ("gf_factor_scaled", factor_scaled(W=193, ld=208), -1, "gf_factor_scaled: width 193 unsupported"),
    ("gf_factor_scaled", factor_scaled(W=0), -1, "gf_factor_scaled: width 0 unsupported"),
    ("gf_factor_scaled", factor_scaled(ld=0), -1, "gf_factor_scaled: ld=0 must be a multiple of 16 and >= W=4"),
    ("gf_factor_scaled", factor_scaled(), -1, "gf_factor_scaled: null pointer"),

    ("gf_loglike_fused", sweep(N=0), -1, "gf_loglike_fused: empty problem (N=0)"),
    ("gf_loglike_fused", sweep(**W65), -1,
     "gf_loglike_fused: width 65 unsupported (1..63 any terms; 64..176 complex terms only)"),
    ("gf_loglike_fused", sweep(block=3), -1, "gf_loglike_fused: block=3 must be a power of two in 1..64"),
    ("gf_loglike_fused", sweep(n_first=3), -1,
     "gf_loglike_fused: n_first=3 must be a non-negative multiple of block=8"),
    ("gf_loglike_fused", sweep(), -1, "gf_loglike_fused: null pointer"),
    ("gf_loglike_fused", sweep(Jc=32, variant=LONG_SPAN, p=D), -1,
     "gf_loglike_fused: GF_SWEEP_LONG_SPAN is for the streamed one-wave sweep only (W <= 63, one chunk, no row outputs)"),
    ("gf_loglike_fused", sweep(gen=3, p=D), -1, "gf_loglike_fused: gen_period=3 must be a power of two in 1..64"),
    ("gf_loglike_fused", sweep(variant=3, p=D), -1, "gf_loglike_fused: unknown sweep variant 3"),
    ("gf_loglike_fused", sweep(Jr=1, variant=TILED, p=D), -1,
     "gf_loglike_fused: GF_SWEEP_TILED needs complex terms only (Jr = 0) and Jc <= 31 (Jc=2)"),

    ("gf_loglike_steady", sweep(tail=(Z, 0)), -1, "gf_loglike_steady: null pointer"),
    ("gf_loglike_steady", sweep(B=0, tail=STEADY), -1, "gf_loglike_steady: empty problem (N=16)"),
    ("gf_loglike_steady", sweep(tail=STEADY, **W65), -1,
     "gf_loglike_steady: width 65 unsupported (1..63 any terms; 64..176 complex terms only)"),
    ("gf_loglike_steady", sweep(block=0, tail=STEADY), -1, "gf_loglike_steady: block=0 must be a power of two in 1..64"),
    ("gf_loglike_steady", sweep(n_first=12, tail=STEADY), -1,
     "gf_loglike_steady: n_first=12 must be a non-negative multiple of block=8"),
    ("gf_loglike_steady", sweep(tail=STEADY), -1, "gf_loglike_steady: null pointer"),
    ("gf_loglike_steady", sweep(gen=128, p=D, tail=STEADY), -1,
     "gf_loglike_steady: gen_period=128 must be a power of two in 1..64"),
    ("gf_loglike_steady", sweep(variant=COLUMN, p=D, tail=STEADY), -1,
     "gf_loglike_steady: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=2)"),
    ("gf_loglike_steady", sweep(p=D, tail=(D, -1)), -1,
     "gf_loglike_steady: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=2)"),

    ("gf_steady_sweep", sweep(tail=(Z, 0)), -1, "gf_steady_sweep: null pointer"),
    ("gf_steady_sweep", sweep(N=-1, tail=STEADY), -1, "gf_steady_sweep: empty problem (N=-1)"),
    ("gf_steady_sweep", sweep(Jr=64, Jc=0, tail=STEADY), -1,
     "gf_steady_sweep: width 64 unsupported (1..63 any terms; 64..176 complex terms only)"),
    ("gf_steady_sweep", sweep(block=48, tail=STEADY), -1, "gf_steady_sweep: block=48 must be a power of two in 1..64"),
    ("gf_steady_sweep", sweep(n_first=-8, tail=STEADY), -1,
     "gf_steady_sweep: n_first=-8 must be a non-negative multiple of block=8"),
    ("gf_steady_sweep", sweep(tail=STEADY), -1, "gf_steady_sweep: null pointer"),
    ("gf_steady_sweep", sweep(Jc=32, variant=LONG_SPAN, p=D, tail=STEADY), -1,
     "gf_steady_sweep: GF_SWEEP_LONG_SPAN is for the streamed one-wave sweep only (W <= 63, one chunk, no row outputs)"),
    ("gf_steady_sweep", sweep(variant=7, p=D, tail=STEADY), -1, "gf_steady_sweep: unknown sweep variant 7"),
    ("gf_steady_sweep", sweep(Jc=40, p=D, tail=STEADY), -1,
     "gf_steady_sweep: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=40)"),
    ("gf_steady_sweep", sweep(variant=ZERO_START, p=D, tail=STEADY), -1,
     "gf_steady_sweep: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=2)"),

    ("gf_steady_sweep_reduced", sweep(tail=(D, 0, Z, 0)), -1, "gf_steady_sweep_reduced: null pointer"),
    ("gf_steady_sweep_reduced", sweep(tail=(Z, 0, D, 0)), -1, "gf_steady_sweep_reduced: null pointer"),
    ("gf_steady_sweep_reduced", sweep(N=0, tail=REDUCED), -1, "gf_steady_sweep_reduced: empty problem (N=0)"),
    ("gf_steady_sweep_reduced", sweep(Jr=0, Jc=0, tail=REDUCED), -1,
     "gf_steady_sweep_reduced: width 0 unsupported (1..63 any terms; 64..176 complex terms only)"),
    ("gf_steady_sweep_reduced", sweep(block=-4, tail=REDUCED), -1,
     "gf_steady_sweep_reduced: block=-4 must be a power of two in 1..64"),
    ("gf_steady_sweep_reduced", sweep(n_first=1, tail=REDUCED), -1,
     "gf_steady_sweep_reduced: n_first=1 must be a non-negative multiple of block=8"),
    ("gf_steady_sweep_reduced", sweep(tail=REDUCED), -1, "gf_steady_sweep_reduced: null pointer"),
    ("gf_steady_sweep_reduced", sweep(Jr=2, variant=TILED, p=D, tail=REDUCED), -1,
     "gf_steady_sweep_reduced: GF_SWEEP_TILED needs complex terms only (Jr = 0) and Jc <= 31 (Jc=2)"),
    ("gf_steady_sweep_reduced", sweep(Jr=1, p=D, tail=REDUCED), -1,
     "gf_steady_sweep_reduced: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=2)"),

    ("gf_steady_sweep_rank1", sweep(B=0, tail=RANK1), -1, "gf_steady_sweep_rank1: empty problem (N=16)"),
    ("gf_steady_sweep_rank1", sweep(block=5, tail=RANK1), -1,
     "gf_steady_sweep_rank1: block=5 must be a power of two in 1..64"),
    ("gf_steady_sweep_rank1", sweep(n_first=4, tail=RANK1), -1,
     "gf_steady_sweep_rank1: n_first=4 must be a non-negative multiple of block=8"),
    ("gf_steady_sweep_rank1", sweep(tail=RANK1), -1, "gf_steady_sweep_rank1: null pointer"),
    ("gf_steady_sweep_rank1", sweep(p=D, tail=(Z, 0, D, 1, D)), -1, "gf_steady_sweep_rank1: null pointer"),
    ("gf_steady_sweep_rank1", sweep(p=D, tail=(D, 0, D, 1, Z)), -1, "gf_steady_sweep_rank1: null pointer"),
    ("gf_steady_sweep_rank1", sweep(gen=0, p=D, tail=RANK1), -1,
     "gf_steady_sweep_rank1: gen_period=0 must be a power of two in 1..64"),
    ("gf_steady_sweep_rank1", sweep(variant=3, p=D, tail=RANK1), -1, "gf_steady_sweep_rank1: unknown sweep variant 3"),
    ("gf_steady_sweep_rank1", sweep(Jr=1, variant=TILED | LONG_SPAN, p=D, tail=RANK1), -1,
     "gf_steady_sweep_rank1: GF_SWEEP_TILED needs complex terms only (Jr = 0) and Jc <= 31 (Jc=2)"),
    ("gf_steady_sweep_rank1", sweep(variant=COLUMN, p=D, tail=RANK1), -1,
     "gf_steady_sweep_rank1: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=2)"),
    ("gf_steady_sweep_rank1", sweep(variant=ZERO_START, p=D, tail=RANK1), -1,
     "gf_steady_sweep_rank1: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=2)"),
    ("gf_steady_sweep_rank1", sweep(Jc=0, p=D, tail=RANK1), -1,
     "gf_steady_sweep_rank1: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=0)"),
    ("gf_steady_sweep_rank1", sweep(Jr=1, Jc=40, p=D, tail=RANK1), -1,
     "gf_steady_sweep_rank1: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=40)"),
    ("gf_steady_sweep_rank1", sweep(p=D, tail=(D, -1, D, 1, D)), -1,
     "gf_steady_sweep_rank1: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=2)"),

    ("gf_sample_fused", sweep(N=0), -1, "gf_sample_fused: empty problem (N=0)"),
    ("gf_sample_fused", sweep(B=2, y_bs=0), -1,
     "gf_sample_fused: one chunk, no row outputs, and a batch stride for eps / out (eps_bs=0)"),
    ("gf_sample_fused", sweep(variant=ZERO_START, y_bs=16), -1,
     "gf_sample_fused: one chunk, no row outputs, and a batch stride for eps / out (eps_bs=16)"),
    ("gf_sample_fused", sweep(**W65), -1,
     "gf_sample_fused: width 65 unsupported (1..63 any terms; 64..176 complex terms only)"),
    ("gf_sample_fused", sweep(block=6), -1, "gf_sample_fused: block=6 must be a power of two in 1..64"),
    ("gf_sample_fused", sweep(n_first=20), -1, "gf_sample_fused: n_first=20 must be a non-negative multiple of block=8"),
    ("gf_sample_fused", sweep(), -1, "gf_sample_fused: null pointer"),
    ("gf_sample_fused", sweep(Jc=32, variant=LONG_SPAN, p=D), -1,
     "gf_sample_fused: GF_SWEEP_LONG_SPAN is for the streamed one-wave sweep only (W <= 63, one chunk, no row outputs)"),
    ("gf_sample_fused", sweep(gen=24, p=D), -1, "gf_sample_fused: gen_period=24 must be a power of two in 1..64"),
    ("gf_sample_fused", sweep(variant=-1 & 0xff, p=D), -1, "gf_sample_fused: unknown sweep variant 255"),
    ("gf_sample_fused", sweep(Jr=3, variant=TILED, p=D), -1,
     "gf_sample_fused: GF_SWEEP_TILED needs complex terms only (Jr = 0) and Jc <= 31 (Jc=2)"),

    ("gf_chunk_sweep", chunk_sweep(B=0), -1, "gf_chunk_sweep: empty problem (N=128)"),
    ("gf_chunk_sweep", chunk_sweep(rows=(Z, D, Z, Z)), -1,
     "gf_chunk_sweep: Ut_out and de_out go together, Wt_out needs them"),
    ("gf_chunk_sweep", chunk_sweep(rows=(Z, Z, Z, D)), -1,
     "gf_chunk_sweep: Ut_out and de_out go together, Wt_out needs them"),
    ("gf_chunk_sweep", chunk_sweep(rows=(Z, Z, D, Z)), -1,
     "gf_chunk_sweep: Ut_out and de_out go together, Wt_out needs them"),
    ("gf_chunk_sweep", chunk_sweep(Jr=2, Jc=31), -1,
     "gf_chunk_sweep: width 64 unsupported (1..63 any terms; 64..176 complex terms only)"),
    ("gf_chunk_sweep", chunk_sweep(Jc=89), -1,
     "gf_chunk_sweep: width 178 unsupported (1..63 any terms; 64..176 complex terms only)"),
    ("gf_chunk_sweep", chunk_sweep(block=12), -1, "gf_chunk_sweep: block=12 must be a power of two in 1..64"),
    ("gf_chunk_sweep", chunk_sweep(N=100, chunk_len=60), -1, "gf_chunk_sweep: bad chunking (chunk_len=60, nch=2)"),
    ("gf_chunk_sweep", chunk_sweep(nch=0), -1, "gf_chunk_sweep: bad chunking (chunk_len=64, nch=0)"),
    ("gf_chunk_sweep", chunk_sweep(chunk_len=0), -1, "gf_chunk_sweep: bad chunking (chunk_len=0, nch=2)"),
    ("gf_chunk_sweep", chunk_sweep(N=129), -1, "gf_chunk_sweep: bad chunking (chunk_len=64, nch=2)"),
    ("gf_chunk_sweep", chunk_sweep(N=64), -1, "gf_chunk_sweep: bad chunking (chunk_len=64, nch=2)"),
    ("gf_chunk_sweep", chunk_sweep(first=1, count=2), -1, "gf_chunk_sweep: bad chunk range (first=1, count=2)"),
    ("gf_chunk_sweep", chunk_sweep(first=-1, count=1), -1, "gf_chunk_sweep: bad chunk range (first=-1, count=1)"),
    ("gf_chunk_sweep", chunk_sweep(count=-1), -1, "gf_chunk_sweep: bad chunk range (first=0, count=-1)"),
    ("gf_chunk_sweep", chunk_sweep(), -1, "gf_chunk_sweep: null pointer"),
    ("gf_chunk_sweep", chunk_sweep(variant=LONG_SPAN, p=D), -1,
     "gf_chunk_sweep: GF_SWEEP_LONG_SPAN is for the streamed one-wave sweep only (W <= 63, one chunk, no row outputs)"),
    ("gf_chunk_sweep", chunk_sweep(N=64, nch=1, count=1, variant=LONG_SPAN, p=D, rows=(D, Z, Z, Z)), -1,
     "gf_chunk_sweep: GF_SWEEP_LONG_SPAN is for the streamed one-wave sweep only (W <= 63, one chunk, no row outputs)"),
    ("gf_chunk_sweep", chunk_sweep(gen=3, p=D), -1, "gf_chunk_sweep: gen_period=3 must be a power of two in 1..64"),
    ("gf_chunk_sweep", chunk_sweep(variant=3 | ZERO_START, p=D), -1, "gf_chunk_sweep: unknown sweep variant 3"),
    ("gf_chunk_sweep", chunk_sweep(Jc=32, Jr=0, variant=3, p=D, count=0), 0, None),     # wide: the variant is not read
    ("gf_chunk_sweep", chunk_sweep(Jr=0, Jc=32, variant=TILED, p=D, count=0), 0, None),
    ("gf_chunk_sweep", chunk_sweep(Jr=1, variant=TILED, p=D), -1,
     "gf_chunk_sweep: GF_SWEEP_TILED needs complex terms only (Jr = 0) and Jc <= 31 (Jc=2)"),
    ("gf_chunk_sweep", chunk_sweep(count=0, p=D, rows=(D, D, D, D)), 0, None),

    ("gf_steady_finish", finish(B=0), -1, "gf_steady_finish: empty problem (B=0, N=16)"),
    ("gf_steady_finish", finish(Jr=1), -1,
     "gf_steady_finish: steady mode is for the lane-tiled sweep only (Jr = 0, Jc <= 31; Jr=1, Jc=2)"),
    ("gf_steady_finish", finish(Jc=32), -1,
     "gf_steady_finish: steady mode is for the lane-tiled sweep only (Jr = 0, Jc <= 31; Jr=0, Jc=32)"),
    ("gf_steady_finish", finish(block=3), -1, "gf_steady_finish: block=3 must be a power of two in 1..64"),
    ("gf_steady_finish", finish(), -1, "gf_steady_finish: null pointer"),

    ("gf_steady_finish_window", finish(N=0, tail=(0, 4)), -1, "gf_steady_finish_window: empty problem (B=1, N=0)"),
    ("gf_steady_finish_window", finish(Jc=0, tail=(0, 4)), -1,
     "gf_steady_finish_window: steady mode is for the lane-tiled sweep only (Jr = 0, Jc <= 31; Jr=0, Jc=0)"),
    ("gf_steady_finish_window", finish(block=65, tail=(0, 4)), -1,
     "gf_steady_finish_window: block=65 must be a power of two in 1..64"),
    ("gf_steady_finish_window", finish(tail=(0, 4)), -1, "gf_steady_finish_window: null pointer"),
    ("gf_steady_finish_window", finish(p=D, tail=(-1, 4)), -1,
     "gf_steady_finish_window: the window of switch rows needs 0 <= sw_lo <= sw_hi (sw_lo=-1, sw_hi=4)"),
    ("gf_steady_finish_window", finish(p=D, tail=(5, 4)), -1,
     "gf_steady_finish_window: the window of switch rows needs 0 <= sw_lo <= sw_hi (sw_lo=5, sw_hi=4)"),
    ("gf_steady_finish_window", finish(p=D, tail=(4, 4)), 0, None),

    ("gf_steady_finish_chunked", finish(B=0, N=0, tail=(0, 4, 16, Z)), -1,
     "gf_steady_finish_chunked: empty problem (B=0, N=0)"),
    ("gf_steady_finish_chunked", finish(Jr=2, Jc=40, tail=(0, 4, 16, Z)), -1,
     "gf_steady_finish_chunked: steady mode is for the lane-tiled sweep only (Jr = 0, Jc <= 31; Jr=2, Jc=40)"),
    ("gf_steady_finish_chunked", finish(block=24, tail=(0, 4, 16, Z)), -1,
     "gf_steady_finish_chunked: block=24 must be a power of two in 1..64"),
    ("gf_steady_finish_chunked", finish(tail=(0, 4, 16, Z)), -1, "gf_steady_finish_chunked: null pointer"),
    ("gf_steady_finish_chunked", finish(p=D, tail=(0, 4, 16, Z)), -1, "gf_steady_finish_chunked: null pointer"),
    ("gf_steady_finish_chunked", finish(p=D, tail=(7, 4, 16, D)), -1,
     "gf_steady_finish_chunked: the window of switch rows needs 0 <= sw_lo <= sw_hi (sw_lo=7, sw_hi=4)"),
    ("gf_steady_finish_chunked", finish(p=D, tail=(0, 4, 8, D)), -1,
     "gf_steady_finish_chunked: chunk_blocks=8 must be a power of two >= 16 (chunks start on the groups' grid)"),
    ("gf_steady_finish_chunked", finish(p=D, tail=(0, 4, 48, D)), -1,
     "gf_steady_finish_chunked: chunk_blocks=48 must be a power of two >= 16 (chunks start on the groups' grid)"),
    ("gf_steady_finish_chunked", finish(p=D, tail=(4, 4, 16, D)), 0, None),
    ("gf_steady_finish_chunked", finish(N=1 << 40, p=D, tail=(0, 4, 16, D)), -1,
     "gf_steady_finish_chunked: 1073741824 chunks per problem are more than a launch takes"),

    ("gf_chunk_transition", transition(N=0), -1, "gf_chunk_transition: empty problem (N=0)"),
    ("gf_chunk_transition", transition(Jc=32), -1, "gf_chunk_transition: width 64 unsupported (1..63)"),
    ("gf_chunk_transition", transition(Jc=0), -1, "gf_chunk_transition: width 0 unsupported (1..63)"),
    ("gf_chunk_transition", transition(N=100, chunk_len=56), -1,
     "gf_chunk_transition: bad chunking (chunk_len=56, nch=2)"),
    ("gf_chunk_transition", transition(N=129), -1, "gf_chunk_transition: bad chunking (chunk_len=64, nch=2)"),
    ("gf_chunk_transition", transition(N=64), -1, "gf_chunk_transition: bad chunking (chunk_len=64, nch=2)"),
    ("gf_chunk_transition", transition(nch=0), -1, "gf_chunk_transition: bad chunking (chunk_len=64, nch=0)"),
    ("gf_chunk_transition", transition(first=2, count=1), -1, "gf_chunk_transition: bad chunk range (first=2, count=1)"),
    ("gf_chunk_transition", transition(first=-1), -1, "gf_chunk_transition: bad chunk range (first=-1, count=2)"),
    ("gf_chunk_transition", transition(), -1, "gf_chunk_transition: null pointer"),
    ("gf_chunk_transition", transition(variant=5, p=D), -1, "gf_chunk_transition: unknown sweep variant 5"),
    ("gf_chunk_transition", transition(Jr=1, variant=TILED, p=D), -1,
     "gf_chunk_transition: GF_SWEEP_TILED needs complex terms only (Jr = 0) and Jc <= 31 (Jc=2)"),
    ("gf_chunk_transition", transition(count=0, p=D), 0, None),

    ("gf_chunk_transition_wide", transition_wide(first=1), -1,
     "gf_chunk_transition_wide: bad chunk range (first=1, count=2)"),
    ("gf_chunk_transition_wide", transition_wide(N=0, count=0), 0, None),
    ("gf_chunk_transition_wide", transition_wide(N=0), -1, "gf_chunk_transition_wide: empty problem (N=0)"),
    ("gf_chunk_transition_wide", transition_wide(Jc=31), -1, "gf_chunk_transition_wide: width 62 unsupported (64..176)"),
    ("gf_chunk_transition_wide", transition_wide(Jc=89), -1,
     "gf_chunk_transition_wide: width 178 unsupported (64..176)"),
    ("gf_chunk_transition_wide", transition_wide(N=100, chunk_len=50), -1,
     "gf_chunk_transition_wide: bad chunking (chunk_len=50, nch=2)"),
    ("gf_chunk_transition_wide", transition_wide(N=200), -1,
     "gf_chunk_transition_wide: bad chunking (chunk_len=64, nch=2)"),
    ("gf_chunk_transition_wide", transition_wide(), -1, "gf_chunk_transition_wide: null pointer"),
    ("gf_chunk_transition_wide", transition_wide(B=1 << 20, count=1 << 20, p=D, **WIDE_CHUNKS), -1,
     "gf_chunk_transition_wide: problem too large"),

    ("gf_chunk_combine", (0, 2, 4, Z, Z, Z, Z, Z, Z), -1, "gf_chunk_combine: empty problem"),
    ("gf_chunk_combine", (1, 2, 65, Z, Z, Z, Z, Z, Z), -1, "gf_chunk_combine: width 65 unsupported (1..64)"),
    ("gf_chunk_combine", (1, 2, 4, Z, Z, Z, Z, Z, Z), -1, "gf_chunk_combine: null pointer"),
    ("gf_chunk_combine", (1, 2, 4, D, D, D, D, D, Z), -1, "gf_chunk_combine: cannot opt in to 35840 bytes of LDS"),
    ("gf_chunk_combine", (1, 2, 40, D, D, D, D, D, Z), -1, "gf_chunk_combine: cannot opt in to 77312 bytes of LDS"),
    ("gf_chunk_combine", (1, 2, 64, D, D, D, D, D, Z), -1, "gf_chunk_combine: cannot opt in to 135168 bytes of LDS"),

    ("gf_chunk_combine_tree", (1, 3, 2, 4) + (Z,) * 9, -1, "gf_chunk_combine_tree: P=3 must be a power of two >= 2"),
    ("gf_chunk_combine_tree", (0, 4, 3, 4) + (Z,) * 9, -1, "gf_chunk_combine_tree: P=4 must be a power of two >= 2"),
    ("gf_chunk_combine_tree", (1, 4, 2, 4) + (Z,) * 9, -1, "gf_chunk_combine_tree: nch=2 must lie in (P / 2, P]"),
    ("gf_chunk_combine_tree", (1, 4, 5, 4) + (Z,) * 9, -1, "gf_chunk_combine_tree: nch=5 must lie in (P / 2, P]"),
    ("gf_chunk_combine_tree", (1, 4, 3, 0) + (Z,) * 9, -1, "gf_chunk_combine_tree: width 0 unsupported (1..64)"),
    ("gf_chunk_combine_tree", (1, 4, 3, 4) + (Z,) * 9, -1, "gf_chunk_combine_tree: null pointer"),
    ("gf_chunk_combine_tree", (1, 4, 3, 48) + (D,) * 8 + (Z,), -1,
     "gf_chunk_combine_tree: cannot opt in to 77312 bytes of LDS"),

    ("gf_scaled_propagator", (1, 0, 4, 16, Z, Z, Z, Z), -1, "gf_scaled_propagator: empty problem (N=0)"),
    ("gf_scaled_propagator", (1, 16, 4, 3, Z, Z, Z, Z), -1, "gf_scaled_propagator: bad width / ld (W=4, ld=3)"),
    ("gf_scaled_propagator", (1, 16, 0, 16, Z, Z, Z, Z), -1, "gf_scaled_propagator: bad width / ld (W=0, ld=16)"),
    ("gf_scaled_propagator", (1, 16, 4, 16, Z, Z, Z, Z), -1, "gf_scaled_propagator: null pointer"),
    ("gf_scaled_propagator", (1, BIG, 4, 16, D, D, D, Z), -1, "gf_scaled_propagator: problem too large"),

    ("gf_chunk_linear", chunk_linear(mode=3), -1, "gf_chunk_linear: bad mode 3"),
    ("gf_chunk_linear", chunk_linear(R=0), -1, "gf_chunk_linear: empty problem (N=128, R=0)"),
    ("gf_chunk_linear", chunk_linear(W=64), -1, "gf_chunk_linear: width 64 unsupported (1..63)"),
    ("gf_chunk_linear", chunk_linear(N=129), -1, "gf_chunk_linear: bad chunking (chunk_len=64, nch=2)"),
    ("gf_chunk_linear", chunk_linear(chunk_len=0), -1, "gf_chunk_linear: bad chunking (chunk_len=0, nch=2)"),
    ("gf_chunk_linear", chunk_linear(N=100, chunk_len=50), -1, "gf_chunk_linear: null pointer"),   # any chunk length
    ("gf_chunk_linear", chunk_linear(), -1, "gf_chunk_linear: null pointer"),

    ("gf_chunk_linear_combine", (-1, 1, 128, 64, 2, 4, 1) + (Z,) * 6, -1, "gf_chunk_linear_combine: bad mode -1"),
    ("gf_chunk_linear_combine", (0, 1, 128, 64, 0, 4, 1) + (Z,) * 6, -1, "gf_chunk_linear_combine: empty problem"),
    ("gf_chunk_linear_combine", (0, 1, 128, 64, 2, 4, 1) + (Z,) * 6, -1, "gf_chunk_linear_combine: null pointer"),
    ("gf_chunk_linear_combine", (2, 1, 128, 64, 2, 4, 1, Z, Z, D, Z, D, Z), -1,
     "gf_chunk_linear_combine: null pointer"),

    ("gf_chunk_segment_transitions", (1, 4, 0, Z, Z, Z, Z, Z), -1, "gf_chunk_segment_transitions: empty problem"),
    ("gf_chunk_segment_transitions", (1, 4, 2, Z, Z, Z, Z, Z), -1,
     "gf_chunk_segment_transitions: null pointer (PhiT_out and PsiT_out go together)"),
    ("gf_chunk_segment_transitions", (1, 4, 2, D, D, D, Z, Z), -1,
     "gf_chunk_segment_transitions: null pointer (PhiT_out and PsiT_out go together)"),

    ("gf_chunk_linear_combine_seg", (2, 1, 4, 2, 1) + (Z,) * 7, -1,
     "gf_chunk_linear_combine_seg: bad mode 2 (the solves only)"),
    ("gf_chunk_linear_combine_seg", (0, 1, 4, 2, 1, Z, Z, D, Z, Z, Z, Z), -1,
     "gf_chunk_linear_combine_seg: PhiT and PsiT go together"),
    ("gf_chunk_linear_combine_seg", (0, 1, 4, 2, 0) + (Z,) * 7, -1, "gf_chunk_linear_combine_seg: empty problem"),
    ("gf_chunk_linear_combine_seg", (1, 1, 4, 2, 1) + (Z,) * 7, -1, "gf_chunk_linear_combine_seg: null pointer"),

    ("gf_dense_solve", (1, 0, 1, Z, Z, Z), -1, "gf_dense_solve: empty problem (n=0, nrhs=1)"),
    ("gf_dense_solve", (1, 200, 1, Z, Z, Z), -1, "gf_dense_solve: n=200 unsupported (max 192)"),
    ("gf_dense_solve", (1, 8, 1, Z, Z, Z), -1, "gf_dense_solve: null pointer"),
    ("gf_dense_solve_logdet", (1, 8, 0, Z, Z, Z, Z), -1, "gf_dense_solve: empty problem (n=8, nrhs=0)"),
    ("gf_dense_solve_logdet", (1, 193, 2, Z, Z, Z, Z), -1, "gf_dense_solve: n=193 unsupported (max 192)"),
    ("gf_dense_solve_logdet", (1, 8, 1, Z, Z, Z, Z), -1, "gf_dense_solve: null pointer"),

    ("gf_reduce_tile", (0, 16, Z, Z, Z, Z, 1, Z), -1, "gf_reduce_tile: empty problem (B=0, N=16)"),
    ("gf_reduce_tile", (1, 16, Z, Z, Z, Z, 1, Z), -1, "gf_reduce_tile: null pointer"),
    ("gf_reduce_tile_steady", (1, 16, -1, Z, Z, Z, Z, Z, 1, Z), -1,
     "gf_reduce_tile_steady: empty problem or negative n_first (N=16, n_first=-1)"),
    ("gf_reduce_tile_steady", (1, 16, 0, Z, Z, Z, Z, Z, 1, Z), -1, "gf_reduce_tile_steady: null pointer"),
    ("gf_loglike_finish", (1, 0, Z, Z, Z, Z, Z), -1, "gf_loglike_finish: empty problem (B=1, N=0)"),
    ("gf_loglike_finish", (1, 16, Z, Z, Z, Z, Z), -1, "gf_loglike_finish: null pointer"),
    ("gf_loglike_finish", (1, 16, D, D, Z, Z, Z), -1, "gf_loglike_finish: null pointer"),

    ("gf_solve_chunk", solve_chunk(mode=3), -1, "gf_solve_chunk: bad mode 3"),
    ("gf_solve_chunk", solve_chunk(N=0), -1, "gf_solve_chunk: empty problem (N=0)"),
    ("gf_solve_chunk", solve_chunk(W=257, ld=272), -1, "gf_solve_chunk: width 257 unsupported (max 256)"),
    ("gf_solve_chunk", solve_chunk(ld=17), -1, "gf_solve_chunk: ld=17 must be a multiple of 16 and >= W=4"),
    ("gf_solve_chunk", solve_chunk(N=64), -1, "gf_solve_chunk: bad chunking (chunk_len=64, nch=2)"),
    ("gf_solve_chunk", solve_chunk(), -1, "gf_solve_chunk: null pointer"),
    ("gf_solve_chunk", solve_chunk(B=1 << 12, N=1 << 20, chunk_len=1, nch=1 << 20, p=D), -1,
     "gf_solve_chunk: problem too large"),

    ("gf_solve_chunk_rhs", solve_chunk_rhs(mode=-2), -1, "gf_solve_chunk_rhs: bad mode -2"),
    ("gf_solve_chunk_rhs", solve_chunk_rhs(R=0), -1, "gf_solve_chunk_rhs: empty problem (N=128, R=0)"),
    ("gf_solve_chunk_rhs", solve_chunk_rhs(W=0), -1, "gf_solve_chunk_rhs: width 0 unsupported (max 256)"),
    ("gf_solve_chunk_rhs", solve_chunk_rhs(W=40, ld=32), -1,
     "gf_solve_chunk_rhs: ld=32 must be a multiple of 16 and >= W=40"),
    ("gf_solve_chunk_rhs", solve_chunk_rhs(nch=3), -1, "gf_solve_chunk_rhs: bad chunking (chunk_len=64, nch=3)"),
    ("gf_solve_chunk_rhs", solve_chunk_rhs(), -1, "gf_solve_chunk_rhs: null pointer"),
    ("gf_solve_chunk_rhs", solve_chunk_rhs(B=40000, p=D), -1,
     "gf_solve_chunk_rhs: too many chunks (B * nch = 80000 > 65535)"),

    ("gf_chunk_diag_scan", (1, 2, 64, 65, Z, Z, Z), -1, "gf_chunk_diag_scan: bad shape (rows=64, R=65)"),
    ("gf_chunk_diag_scan", (1, 2, 0, 4, Z, Z, Z), -1, "gf_chunk_diag_scan: bad shape (rows=0, R=4)"),
    ("gf_chunk_diag_scan", (1, 2, 64, 4, Z, Z, Z), -1, "gf_chunk_diag_scan: null pointer"),

    ("gf_solve", solve(mode=7), -1, "gf_solve: bad mode 7"),
    ("gf_solve", solve(R=0), -1, "gf_solve: empty problem (N=16, R=0)"),
    ("gf_solve", solve(W=300, ld=304), -1, "gf_solve: width 300 unsupported (max 256)"),
    ("gf_solve", solve(ld=8), -1, "gf_solve: ld=8 must be a multiple of 16 and >= W=4"),
    ("gf_solve", solve(), -1, "gf_solve: null pointer"),
    ("gf_solve", solve(mode=2, p=D), -1, "gf_solve: GF_MATMUL_LOWER cannot run in place"),

    ("gf_cross_covariance", cross(R=4097), -1, "gf_cross_covariance: bad shape (N=16, R=4097)"),
    ("gf_cross_covariance", cross(N=0), -1, "gf_cross_covariance: bad shape (N=0, R=4)"),
    ("gf_cross_covariance", cross(Jr=0, Jc=0), -1, "gf_cross_covariance: bad term counts"),
    ("gf_cross_covariance", cross(Jr=1, Jc=128), -1, "gf_cross_covariance: bad term counts"),
    ("gf_cross_covariance", cross(), -1, "gf_cross_covariance: null pointer"),
    ("gf_cross_covariance", cross(N=BIG, p=D), -1, "gf_cross_covariance: problem too large"),

    ("gf_interp_plan", (0, Z, Z, 1.0, Z, Z, Z), -1, "gf_interp_plan: empty series (N=0)"),
    ("gf_interp_plan", (16, Z, Z, 1.0, Z, Z, Z), -1, "gf_interp_plan: null pointer"),
    ("gf_interp_plan", (16, D, Z, 0.0, D, D, Z), -1, "gf_interp_plan: the cadence must be positive"),
    ("gf_interp_plan", (16, D, Z, float("nan"), D, D, Z), -1, "gf_interp_plan: the cadence must be positive"),
    ("gf_interp_plan", (16, D, Z, 1.0, D, D, Z), -1, "gf_interp_plan: cannot read the first time"),
    ("gf_interp_fill", (-3, Z, Z, Z, 1.0, Z, Z, Z, Z), -1, "gf_interp_fill: empty series (N=-3)"),
    ("gf_interp_fill", (16, Z, Z, Z, 1.0, Z, Z, Z, Z), -1, "gf_interp_fill: null pointer"),
    ("gf_interp_fill", (16, D, D, Z, 1.0, D, D, D, Z), -1, "gf_interp_fill: cannot read the first time"),

    ("gf_psd_power", (1, 16, 16, 1.0, Z, Z, Z), -1, "gf_psd_power: bad shape (M=16, first=16)"),
    ("gf_psd_power", (0, 16, 0, 1.0, Z, Z, Z), -1, "gf_psd_power: bad shape (M=16, first=0)"),
    ("gf_psd_power", (1, 16, 0, 1.0, Z, Z, Z), -1, "gf_psd_power: null pointer"),
    ("gf_psd_power", (65536, 16, 0, 1.0, D, D, Z), -1, "gf_psd_power: more than 65535 series"),
    ("gf_psd_bin", (1, 16, 0, Z, Z, Z, 0.0, Z, Z, Z), -1, "gf_psd_bin: bad shape (M=16, bins=0)"),
    ("gf_psd_bin", (1, 16, 4, Z, Z, Z, 0.0, Z, Z, Z), -1, "gf_psd_bin: null pointer"),
    ("gf_psd_bin", (65536, 16, 4, D, D, D, 0.0, D, D, Z), -1, "gf_psd_bin: more than 65535 series"),

    ("gf_general_matmul", matmul(M=0), -1, "gf_general_matmul: empty problem (M=0, N=16)"),
    ("gf_general_matmul", matmul(W=257, ld=272), -1, "gf_general_matmul: width 257 unsupported (max 256)"),
    ("gf_general_matmul", matmul(ld=40), -1, "gf_general_matmul: ld=40 must be a multiple of 16 and >= W=4"),
    ("gf_general_matmul", matmul(), -1, "gf_general_matmul: null pointer"),
]


def _needs_no_device(args):
    return any(a is D for a in args)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_every_case_names_a_declared_entry_point():
    assert {c[0] for c in CASES} <= set(_lib.SIGNATURES)
    for name, args, _, _ in CASES:
        assert len(args) == len(_lib.SIGNATURES[name][1]), name


def test_null_pointer_cases(lib):
    ran = 0
    for name, args, status, text in CASES:
        if _needs_no_device(args):
            continue
        assert getattr(lib, name)(*args) == status, (name, args, lib.gf_last_error())
        assert text is None or lib.gf_last_error().decode() == text, (name, args)
        ran += 1
    assert ran > 150


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="dummy addresses: only where nothing can launch")
def test_dummy_pointer_cases(lib):
    ran = 0
    for name, args, status, text in CASES:
        if not _needs_no_device(args):
            continue
        assert getattr(lib, name)(*args) == status, (name, args, lib.gf_last_error())
        assert text is None or lib.gf_last_error().decode() == text, (name, args)
        ran += 1
    assert ran > 80


def test_a_message_does_not_outlive_its_slot(lib):
    # gf_last_error() is one thread-local buffer: a later, shorter message replaces a longer one entirely
    lib.gf_sample_fused(*sweep(B=2, y_bs=0))
    lib.gf_reduce_tile(1, 16, Z, Z, Z, Z, 1, Z)
    assert lib.gf_last_error() == b"gf_reduce_tile: null pointer"

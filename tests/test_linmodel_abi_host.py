"""CPU: every argument check of gf_linear_gram and gf_linear_gram_work (gadfly_linmodel.hip), by exact status and
exact gf_last_error() text.  Every pointer is NULL: the null-pointer check is the last one, so no case can reach a
launch."""
import pytest

from gadfly_amd import _lib

Z = None


def gram(B=1, N=16, R=3, Jr=0, Jc=2, t_bs=0, d_bs=0, y_bs=0, lda=None, a_bs=0, work_bs=1 << 40):
    lda = R if lda is None else lda
    return ((B, N, R, Jr, Jc) + (Z,) * 7 + (Z, t_bs, Z, d_bs, Z, y_bs, Z) + (Z, lda, a_bs, Z, work_bs) + (Z,) * 3
            + (Z,))


SHAPE = "gf_linear_gram: bad shape (B={B}, N={N}, R={R} of 1..255, Jr={Jr}, Jc={Jc})"
CASES = [
    (dict(B=0), -1, SHAPE.format(B=0, N=16, R=3, Jr=0, Jc=2)),
    (dict(N=0), -1, SHAPE.format(B=1, N=0, R=3, Jr=0, Jc=2)),
    (dict(R=0), -1, SHAPE.format(B=1, N=16, R=0, Jr=0, Jc=2)),
    (dict(R=256), -1, SHAPE.format(B=1, N=16, R=256, Jr=0, Jc=2)),
    (dict(Jr=-1), -1, SHAPE.format(B=1, N=16, R=3, Jr=-1, Jc=2)),
    (dict(Jr=0, Jc=0), -1, SHAPE.format(B=1, N=16, R=3, Jr=0, Jc=0)),
    (dict(Jr=0, Jc=32), -3, "gf_linear_gram: width W=64 exceeds the one-wave limit 63"),
    (dict(Jr=2, Jc=31), -3, "gf_linear_gram: width W=64 exceeds the one-wave limit 63"),
    (dict(work_bs=16 * 8 - 1), -1, "gf_linear_gram: work_bs=127 < gf_linear_gram_work(N, W, R)=128"),
    (dict(R=8, work_bs=16 * 8), -1, "gf_linear_gram: work_bs=128 < gf_linear_gram_work(N, W, R)=256"),
    (dict(lda=2), -1, "gf_linear_gram: bad stride (t_bs=0, diag_bs=0, y_bs=0, lda=2, a_bs=0 for R=3, N=16)"),
    (dict(a_bs=47), -1, "gf_linear_gram: bad stride (t_bs=0, diag_bs=0, y_bs=0, lda=3, a_bs=47 for R=3, N=16)"),
    (dict(a_bs=-1), -1, "gf_linear_gram: bad stride (t_bs=0, diag_bs=0, y_bs=0, lda=3, a_bs=-1 for R=3, N=16)"),
    (dict(t_bs=-1), -1, "gf_linear_gram: bad stride (t_bs=-1, diag_bs=0, y_bs=0, lda=3, a_bs=0 for R=3, N=16)"),
    (dict(y_bs=-16), -1, "gf_linear_gram: bad stride (t_bs=0, diag_bs=0, y_bs=-16, lda=3, a_bs=0 for R=3, N=16)"),
    (dict(d_bs=-2), -1, "gf_linear_gram: bad stride (t_bs=0, diag_bs=-2, y_bs=0, lda=3, a_bs=0 for R=3, N=16)"),
    (dict(), -1, "gf_linear_gram: null pointer"),
    (dict(a_bs=255, R=255, lda=255, N=1), -1, "gf_linear_gram: null pointer"),
]


@pytest.mark.parametrize("kw,status,text", CASES, ids=[f"{i}-{'-'.join(c[0]) or 'null'}" for i, c in enumerate(CASES)])
def test_linear_gram_refuses_before_any_launch(kw, status, text):
    lib = _lib.load()
    assert lib.gf_linear_gram(*gram(**kw)) == status
    assert _lib.last_error() == text


def test_linear_gram_work_sizes():
    """N rows of the R + 1 columns rounded up to whole tiles of 8; 0 for what gf_linear_gram refuses."""
    lib = _lib.load()
    for R, ld in ((1, 8), (6, 8), (7, 8), (8, 16), (63, 64), (64, 72), (255, 256)):
        for W in (1, 16, 17, 63):
            assert lib.gf_linear_gram_work(1000, W, R) == 1000 * ld
    assert lib.gf_linear_gram_work(1 << 40, 5, 255) == (1 << 40) * 256
    for N, W, R in ((0, 4, 3), (16, 0, 3), (16, 64, 3), (16, 4, 0), (16, 4, 256), (-1, 4, 3)):
        assert lib.gf_linear_gram_work(N, W, R) == 0

"""What the start-up of the linkage (csrc/ahc_startup.hip) has to leave behind, restated in numpy for tests/test_gpu_ahc_startup.py: the squared
distances and squared norms of a point set beyond double precision, the reference's sequential float64 sum, and the three numbers a row of a
matrix yields (minimum, lowest-index argmin, smallest entry elsewhere).  Nothing here is shared with oracle/ or with the package under test."""
import numpy as np

U = 2.0 ** -53                      # unit roundoff of float64
DEAD = np.iinfo(np.int32).max       # node id of an empty slot


def exact_sqdist(x, rows=32):
    """D[i][j] = sum_k (x_ik - x_jk)^2 and |x_i|^2 in numpy.longdouble (64-bit significand on x86-64: every operation rounds at 2^-64, so a sum
    of d <= 256 terms carries a relative error below (d + 2) * 2^-64 — 1/2048 of u times the same factor, which is the smallest term of any
    bound the test holds it against).  Broadcast over k, `rows` rows of the lower triangle at a time; the upper one is its mirror."""
    xl = np.asarray(x, np.float64).astype(np.longdouble)
    n = xl.shape[0]
    D = np.zeros((n, n), np.longdouble)
    for i0 in range(0, n, rows):
        i1 = min(i0 + rows, n)
        diff = xl[i0:i1, None, :] - xl[None, :i1, :]
        D[i0:i1, :i1] = np.einsum("ijk,ijk->ij", diff, diff)
    D = np.tril(D) + np.tril(D, -1).T
    return D, np.einsum("ik,ik->i", xl, xl)


def sequential_sqdist(x):
    """The reference's own sum: float64, k ascending, one rounding per subtraction, product and addition."""
    x = np.asarray(x, np.float64)
    acc = np.zeros((x.shape[0], x.shape[0]))
    for k in range(x.shape[1]):
        diff = x[:, None, k] - x[None, :, k]
        acc = acc + diff * diff
    return acc


def row_minima(M):
    """Per row of M: the minimum, the lowest index that attains it, and the smallest entry of the row with that index removed (the second
    smallest value; equal to the minimum when the minimum occurs twice)."""
    M = np.asarray(M)
    nn = M.argmin(axis=1)               # the first occurrence
    rows = np.arange(M.shape[0])
    d1 = M[rows, nn]
    rest = M.copy()
    rest[rows, nn] = np.inf
    return d1, nn, rest.min(axis=1)

"""Exact-integer reference for the K10 tests (tests/test_marlin_index_host.py, tests/test_gpu_marlin_index.py): the entry order of the
index (row by row, stable ascending column), the arithmetisation of tests/marlin_reference.py applied in that order plus row_col, and
the rules for |K| and |B|.  Coefficients and evaluations on B come from the C++ oracle's transforms of these integers (or, for a small
K, from mr.interpolate); domain elements from the oracle's transform of the unit vector, never from the library."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marlin_reference as mr  # noqa: E402


def index_order(entries):
    """(r, c, v) entries in the index's order: by row; inside a row by ascending column, equal columns in the order given (a stable
    sort, as upstream sorts a row that is not ascending); duplicates and explicit zeros stay"""
    return sorted(entries, key=lambda e: (e[0], e[1]))  # sorted() is stable: ties keep the order of `entries`


def csr_order(entries):
    """the order in which a CSR built from `entries` lists them: by row, inside a row as given"""
    return sorted(entries, key=lambda e: e[0])


def arithmetize(entries, dom_h, h_n, x_n, k_n, p):
    """(row, col, row_col, val) on K of one matrix, entries taken in the index's order"""
    row, col, val = mr.arithmetize(index_order(entries), dom_h, h_n, x_n, k_n, p)
    return row, col, [r * c % p for r, c in zip(row, col)], val


def domain_k(co, field, nnz):
    """|K| for the three matrices' entry counts"""
    return co.domain_size(field, max(max(nnz), 1))


def domain_b(co, field, k_n):
    """|B|: the smallest domain of at least 3 |K| - 3 elements (upstream's rule, restated from memory in include/pcdhip.h)"""
    return co.domain_size(field, max(3 * k_n - 3, 1))


def odd_part(field, n):
    """m of n = m 2^a, the `m` argument of the oracle's fft_general"""
    while n % 2 == 0:
        n //= 2
    return n


def transform(co, field, mont, inverse=False, nthreads=1):
    """the oracle's transform over the domain of len(mont) elements, radix-2 or mixed-radix"""
    n = mont.shape[0]
    if n == 1:
        return mont.copy()
    m = odd_part(field, n)
    return co.fft(field, mont, inverse=inverse, nthreads=nthreads) if m == 1 else co.fft_general(field, mont, m, inverse=inverse, nthreads=nthreads)

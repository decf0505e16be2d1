"""GPU: the top-1 filter scan with the half-sum first pass (fscan_mx_kernel_cascade, option scan_cascade) against the scan
without it (fscan_mx_kernel), ids and distance bits exactly, on the shapes where the first pass decides differently: the bench
shape, small and ragged batches, N ending inside a group / a trip / a chunk, appends, the subset path, tied codes, an
overflowing candidate buffer, and a set where every code passes the first pass."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.util import make_problem, assert_same_result

pytestmark = pytest.mark.gpu
M, Ks, Ds = 32, 256, 4


def both(g, Q, tids=None):
    """(cascade off, cascade forced on) results of one batch; the option is put back to its default."""
    g.set_option("scan_cascade", 0)
    off = g.query_linear_batch(Q, 1, tids)
    g.set_option("scan_cascade", 2)
    on = g.query_linear_batch(Q, 1, tids)
    g.set_option("scan_cascade", 1)
    return off, on


def assert_equal_runs(off, on, what):
    assert np.array_equal(off[0], on[0]), "%s: ids differ" % what
    assert np.array_equal(off[1].view(np.uint32), on[1].view(np.uint32)), "%s: distances differ (bitwise)" % what


def engine(cw):
    from rii_amd import RiiGpu
    g = RiiGpu(cw, False, simd_arch="avx512")
    g.set_option("fast_min_batch", 1)            # every batch size takes the filter scan
    assert g.get_option("scan_cascade") == 1
    return g


def test_bench_shape_1m():
    """N = 1M, B = 1024 (the bench shape; the default option selects the cascade there), and the subset path on it."""
    N, B = 1_000_000, 1024
    cw, codes, qs = make_problem(2024, M, Ks, Ds, N, "sift", dup=5000)
    rng = np.random.default_rng(5)
    Q = np.round(rng.random((B, M * Ds)) * 255).astype(np.float32)
    Q[:16] = qs
    g = engine(cw)
    g.add_codes(codes, False)
    off, on = both(g, Q)
    assert_equal_runs(off, on, "N=1M B=1024")
    default = g.query_linear_batch(Q, 1, None)
    assert_equal_runs(off, default, "N=1M B=1024 default options")
    tids = np.sort(rng.choice(N, 100_000, replace=False)).astype(np.int64)
    assert_equal_runs(*both(g, Q, tids), "N=1M B=1024 subset")


@pytest.mark.parametrize("B", [1, 16, 17, 256, 1024])
def test_batch_sizes(B):
    cw, codes, qs = make_problem(11 + B, M, Ks, Ds, 70_000, "sift", dup=300)
    g = engine(cw)
    g.add_codes(codes, False)
    rng = np.random.default_rng(B)
    Q = np.round(rng.random((B, M * Ds)) * 255).astype(np.float32)
    Q[:min(B, 16)] = qs[:min(B, 16)]
    assert_equal_runs(*both(g, Q), "B=%d" % B)


def test_ragged_ends_appends_and_subset():
    """Appends whose running N ends inside a group of 16, inside a trip of 1024 and inside a chunk; the subset path after each."""
    cw, codes, qs = make_problem(77, M, Ks, Ds, 300_000, "sift", dup=2000)
    g = engine(cw)
    rng = np.random.default_rng(3)
    Q = np.round(rng.random((300, M * Ds)) * 255).astype(np.float32)
    Q[:16] = qs
    done = 0
    for n in (9, 1024 + 16 * 5 + 3, 40_000 + 7, 131_072 + 1000 + 5, 300_000):
        g.add_codes(codes[done:n], False)
        done = n
        assert_equal_runs(*both(g, Q), "N=%d" % n)
        tids = np.sort(rng.choice(n, max(1, n // 3), replace=False)).astype(np.int64)
        assert_equal_runs(*both(g, Q, tids), "N=%d subset" % n)


def test_tied_codes_and_overflowing_candidate_buffer():
    """Thousands of duplicates of the nearest code of some queries: exact ties, and (with a small candidate buffer) overflow."""
    N = 100_000
    cw, codes, qs = make_problem(5, M, Ks, Ds, N, "sift")
    rng = np.random.default_rng(9)
    codes[rng.integers(0, N, 6000)] = codes[17]
    Q = np.round(rng.random((64, M * Ds)) * 255).astype(np.float32)
    Q[:16] = qs
    Q[16:24] = cw[np.arange(M), codes[17]].reshape(-1)      # queries sitting on the duplicated code
    g = engine(cw)
    g.add_codes(codes, False)
    assert_equal_runs(*both(g, Q), "ties")
    g.set_option("cand_cap", 64)
    off, on = both(g, Q)
    assert_equal_runs(off, on, "ties, cand_cap=64")
    o = O.OracleRii(cw, False, simd_arch="avx512")
    o.add_codes(codes, False)
    for b in (0, 16, 20, 23):
        assert_same_result((on[0][b], on[1][b]), o.query_linear(Q[b], 1, np.array([], np.int64)), "ties b=%d" % b)


def test_every_code_passes_the_first_pass():
    """Subspaces 0..15 hold one and the same codeword in every code, so every code's half sum equals the minimum one and every
    group goes through the finish path; the full sums still decide."""
    N = 50_000 + 11
    cw, codes, qs = make_problem(8, M, Ks, Ds, N, "sift")
    codes[:, :16] = codes[0, :16]
    rng = np.random.default_rng(4)
    Q = np.round(rng.random((48, M * Ds)) * 255).astype(np.float32)
    Q[:16] = qs
    Q[16:32] = cw[np.arange(M), codes[rng.integers(0, N, 16)]].reshape(16, -1)     # queries on codes of the set
    g = engine(cw)
    g.add_codes(codes, False)
    off, on = both(g, Q)
    assert_equal_runs(off, on, "every code survives")
    o = O.OracleRii(cw, False, simd_arch="avx512")
    o.add_codes(codes, False)
    for b in (0, 7, 16, 31, 47):
        assert_same_result((on[0][b], on[1][b]), o.query_linear(Q[b], 1, np.array([], np.int64)), "every code survives b=%d" % b)

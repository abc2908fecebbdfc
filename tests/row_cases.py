"""Row lists shared by tests/test_row_cases_cpu.py and tests/test_gpu_rows.py: the src_rows / dst_rows inputs of the
row-copy kernels of csrc/stream.hip.  Every generator takes (n, rows, seed) and returns n int32 row numbers of a
source table of `rows` rows (rows >= 2 n + 4 suits them all); the same arguments give the same list.

The compaction kernel (k_rows_compact) moves one aligned 16-byte chunk of the destination per lane and takes its four
source words with one load when the chunk's rows are consecutive in the source.  The lists below are the shapes that
decision can meet: all consecutive, none consecutive, long runs with seams, and lists whose chunks look consecutive
from their two ends only (endpoints_lie, and by chance permutation and with_repeats)."""
import numpy as np


def _rng(seed):
    return np.random.default_rng(seed)


def identity(n, rows, seed=0):
    return np.arange(n, dtype=np.int32)


def one_run(n, rows, seed=0):
    """arange plus an offset: one run that does not start at row 0."""
    return (np.arange(n) + int(_rng(seed).integers(1, rows - n + 1))).astype(np.int32)


def alternating(n, rows, seed=0):
    """Every second row: strictly increasing, no two consecutive."""
    return (2 * np.arange(n) + int(_rng(seed).integers(0, 2))).astype(np.int32)


def increasing_dense(n, rows, seed=0):
    """A random strictly increasing subset that keeps about 90% of a window: long runs with seams."""
    m = min(rows, n + max(1, n // 9))
    return np.sort(_rng(seed).permutation(m)[:n]).astype(np.int32)


def descending(n, rows, seed=0):
    return (rows - 1 - np.arange(n)).astype(np.int32)


def permutation(n, rows, seed=0):
    """n distinct rows in random order."""
    return _rng(seed).permutation(rows)[:n].astype(np.int32)


def with_repeats(n, rows, seed=0):
    """Non-decreasing with duplicates: n draws with replacement from a window of about n rows, sorted."""
    return np.sort(_rng(seed).integers(0, min(rows, n + 3), n)).astype(np.int32)


# the 1-word patterns fill one chunk (four rows) each; the 2-word patterns are three rows (a chunk and a half)
_LIES = {1: ((0, 2, 1, 3), (0, 0, 1, 3)), 2: ((0, 0, 2), (0, 3, 2))}


def endpoints_lie(words):
    """Lists tiled from patterns whose first and last row differ by exactly the pattern's span while the rows between
    are not consecutive.  The tiling starts at list position 0, a chunk boundary for every row width, and a 1-word
    pattern is four rows long, so every 1-word pattern is exactly one destination chunk.  The 2-word patterns would
    deceive a chunk that starts in the middle of a row and ends in the next but one; chunks start at multiples of four
    words, so no such chunk exists at any phase (tests/test_row_cases_cpu.py) and these lists are hostile in shape
    only.  A remainder shorter than a pattern is filled with the pattern's head."""
    pats = _LIES[words]

    def gen(n, rows, seed=0):
        rng = _rng(seed)
        out = np.empty(n, np.int32)
        i = 0
        while i < n:
            p = np.array(pats[int(rng.integers(0, len(pats)))]) + int(rng.integers(0, rows - 3))
            k = min(len(p), n - i)
            out[i:i + k] = p[:k]
            i += k
        return out

    gen.__name__ = f"endpoints_lie{words}"
    return gen


INCREASING = (identity, one_run, alternating, increasing_dense)  # strictly increasing: what SPTCache.step passes
ANY_ORDER = (descending, permutation, with_repeats)
GENERATORS = INCREASING + ANY_ORDER
LIES = {w: endpoints_lie(w) for w in _LIES}
BY_NAME = {g.__name__: g for g in GENERATORS + tuple(LIES.values())}


def source_rows(n):
    """The source table's row count the tests pair with a list of n rows."""
    return 2 * n + 8


# (generator name, n, seed): lists of 1-word rows in which at least one full chunk has consecutive-looking end rows and
# other rows between (tests/test_row_cases_cpu.py proves it of each).  A uniform permutation has such a chunk with
# probability of about n / (4 rows) only, so its seeds were searched for on the CPU; sorted draws with replacement
# have many at any seed.  The compaction test of tests/test_gpu_rows.py runs every one of these.
ADVERSARIAL = (("permutation", 8, 42), ("permutation", 1027, 2), ("permutation", 4100, 0),
               ("with_repeats", 8, 3), ("with_repeats", 1027, 0), ("with_repeats", 4100, 0),
               ("endpoints_lie1", 4, 0), ("endpoints_lie1", 8, 0), ("endpoints_lie1", 1027, 0),
               ("endpoints_lie1", 4100, 0))

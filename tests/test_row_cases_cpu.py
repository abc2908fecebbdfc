"""The row lists of tests/row_cases.py against a numpy restatement of k_rows_compact's chunk geometry (csrc/stream.hip):
which lists hold a chunk that looks contiguous from its two end rows and is not, so that the adversarial inputs of
tests/test_gpu_rows.py are proven adversarial, and the harmless ones harmless, without a GPU."""
import itertools

import numpy as np
import pytest

import row_cases as RC

WIDTHS = (1, 2, 3, 4, 5, 45, 48)  # the compaction test's row widths, in 32-bit words


def chunks(n, words):
    """(r, r_end) of every full chunk: chunk c covers destination words [4c, 4c + 4), whose first word lies in list
    row r = 4c // words and whose last in r_end = (4c + 3) // words.  A partial last chunk never takes the 16-byte
    load, so it cannot be deceived."""
    c = np.arange(n * words // 4, dtype=np.int64)
    return 4 * c // words, (4 * c + 3) // words


def lying_chunks(rows, words):
    """Number of full chunks whose end rows differ by the chunk's span (the kernel's test before this change) while
    some adjacent pair of rows inside the chunk is not consecutive in the source."""
    rows = np.asarray(rows, np.int64)
    r, r_end = chunks(len(rows), words)
    passes = rows[r_end] - rows[r] == r_end - r
    step_ok = np.concatenate([np.diff(rows) == 1, [True]])
    bad = np.concatenate([[0], np.cumsum(~step_ok)])  # bad[j] = non-consecutive pairs (i, i + 1) with i < j
    consecutive = bad[r_end] - bad[r] == 0
    return int(np.count_nonzero(passes & ~consecutive))


def test_lying_chunks_on_the_hand_examples():
    assert lying_chunks([5, 9, 2, 8], 1) == 1 and lying_chunks([5, 5, 6, 8], 1) == 1
    assert lying_chunks([5, 6, 7, 8], 1) == 0 and lying_chunks([5, 9, 2, 7], 1) == 0
    assert lying_chunks([5, 9, 2, 8, 1, 3, 2], 1) == 1  # rows 4..6: a partial chunk
    assert lying_chunks([0, 1, 3, 4], 3) == 0  # (0, 1) consecutive, (1, 3) fails the end test, (3, 4) consecutive


@pytest.mark.parametrize("gen", RC.GENERATORS + tuple(RC.LIES.values()), ids=lambda g: g.__name__)
def test_lists_are_valid_and_repeatable(gen):
    for n in (1, 2, 3, 4, 5, 97, 4100):
        rows = RC.source_rows(n)
        a = gen(n, rows, 7)
        assert a.dtype == np.int32 and a.shape == (n,)
        assert a.min() >= 0 and a.max() < rows
        np.testing.assert_array_equal(a, gen(n, rows, 7))


def test_list_shapes():
    n, rows = 4100, RC.source_rows(4100)
    for gen in RC.INCREASING:
        assert np.all(np.diff(gen(n, rows, 1).astype(np.int64)) > 0), gen.__name__
    np.testing.assert_array_equal(np.diff(RC.one_run(n, rows, 1)), 1)
    assert RC.one_run(n, rows, 1)[0] > 0
    assert np.all(np.diff(RC.alternating(n, rows, 1)) == 2)
    d = np.diff(RC.increasing_dense(n, rows, 1))
    assert 0.85 < np.mean(d == 1) < 0.95  # long runs, and seams between them
    assert np.all(np.diff(RC.descending(n, rows, 1)) == -1)
    p = RC.permutation(n, rows, 1)
    assert len(np.unique(p)) == n and np.any(np.diff(p) < 0)
    w = np.diff(RC.with_repeats(n, rows, 1))
    assert np.all(w >= 0) and np.any(w == 0) and np.any(w > 1)


@pytest.mark.parametrize("name,n,seed", RC.ADVERSARIAL)
def test_adversarial_lists_deceive_the_end_row_test(name, n, seed):
    assert lying_chunks(RC.BY_NAME[name](n, RC.source_rows(n), seed), 1) >= 1


def test_every_one_word_pattern_is_a_lying_chunk():
    """endpoints_lie(1): every full chunk of the list is one, at every length and seed."""
    for n, seed in itertools.product((4, 7, 8, 1024, 4099), range(3)):
        assert lying_chunks(RC.LIES[1](n, RC.source_rows(n), seed), 1) == n // 4


@pytest.mark.parametrize("gen", RC.INCREASING, ids=lambda g: g.__name__)
def test_strictly_increasing_lists_hold_none(gen):
    """Between strictly increasing rows every step is >= 1, so end rows that differ by the span force every step to
    be 1: the lists SPTCache.step passes (nonzero of a mask) were always copied right."""
    for words, n, seed in itertools.product(WIDTHS, (1, 4, 97, 1027, 4100), range(3)):
        assert lying_chunks(gen(n, RC.source_rows(n), seed), words) == 0


def test_only_one_word_rows_have_chunks_of_more_than_two_rows():
    """A chunk starts at word 4c.  Rows of k >= 2 words: its first word is word j = 4c % k of row r, its last is word
    j + 3, so it ends in row r + (j + 3) // k; enumerating j shows when that is more than one row on.  For k >= 3 it
    never is (j + 3 < 2k).  For k = 2, 4c is even, j = 0 and the chunk is exactly two whole rows: the odd phase that
    would span three rows does not occur when chunks start at multiples of four words.  So the end-row test was
    exact for every width but one word, where a chunk is four rows."""
    for k in range(2, 64):
        spans = {(4 * c % k + 3) // k for c in range(k)}
        assert max(spans) <= 1, k
    r, r_end = chunks(1000, 1)
    assert np.all(r_end - r == 3)
    # hence no list, however hostile, deceives a width >= 2: its chunks have no interior row
    for words in WIDTHS[1:]:
        for gen in RC.ANY_ORDER + tuple(RC.LIES.values()):
            for n, seed in itertools.product((4, 97, 1027, 4100), range(3)):
                assert lying_chunks(gen(n, RC.source_rows(n), seed), words) == 0, (words, gen.__name__)

"""The certification criterion of sst_table_certify (tests/_certify_model.py)
against tables the CPU oracle builds and the reference's own words: built
tables pass under every last-column mask, and every damage the criterion is
meant to catch is flagged at the right word.  CPU only."""
import numpy as np
import pytest

import _certify_model as model
import _oracle as oracle

COMPRESSIONS = (4, 8, 16, 32)


def _alphabets(C):
    # shift 0, shift C - 1, step 1 (C <= w < 2C) and a mass beyond most tables
    return ([0, C], [0, 2 * C - 1, 3 * C], [0, C + 1, 2 * C + 3, 5 * C - 1], [0, C, C + 2, 3 * C + 1, 40 * C + 5])


def test_reference_tiny_tables(golden_tables):
    seen = 0
    for tiny in golden_tables["tiny"]:
        C, ms = tiny["compression"], tiny["masses"]
        if not model.certifiable(ms, C):
            continue
        words = np.array(tiny["words"], dtype=model.DT[C])
        assert model.first_violation(words, ms, C) is None, (ms, tiny["max_mass"], C)
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_built_tables_pass_under_every_mask(C):
    ks = set()
    for ms in _alphabets(C):
        for n_cols in (1, 2, C, C + 3):
            for max_mass in range((n_cols - 1) * C, n_cols * C):  # all share n_cols
                words = oracle.build_table(ms, max_mass, C)
                assert words.shape == (len(ms), n_cols)
                assert model.first_violation(words, ms, C) is None, (ms, max_mass)
                # the reference's mask (mass_table.py:246, numpy shifts) is a member of the family
                k = min(C, n_cols - (max_mass + 1) % n_cols)
                exp = model.expected_words(words, ms, C)
                assert all(k in model.admissible_k(words[r, -1], exp[r, -1], C) for r in range(len(ms)))
                ks.add(k)
    assert ks == set(range(1, C + 1))  # k = C: the all-zero mask


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_every_single_bit_flip_below_the_last_column_is_flagged(C):
    rng = np.random.default_rng(C)
    for ms in _alphabets(C):
        n_cols = int(rng.integers(2, 11))
        max_mass = int(rng.integers((n_cols - 1) * C, n_cols * C))
        words = oracle.build_table(ms, max_mass, C)
        assert words.shape[0] <= 5 and words.shape[1] == n_cols
        for r in range(words.shape[0]):
            for c in range(n_cols - 1):
                for bit in range(2 * C):
                    assert model.first_violation(model.flip(words, r, c, bit), ms, C) == (r, c), (ms, r, c, bit)


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_last_column_bit_outside_the_closure_is_flagged(C):
    ms = [0, 3 * C + 1, 3 * C + 2]
    words = oracle.build_table(ms, 3 * C - 2, C)  # 3 columns, mask k = 1; nothing but mass 0 is reachable
    bad = model.stray_last_column_bit(words, ms, C)
    assert model.first_violation(bad, ms, C) == (len(ms) - 1, words.shape[1] - 1)


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_one_mass_off_by_one_is_flagged(C):
    ms = [0, C + 1, 2 * C + 3, 5 * C - 1]
    words = oracle.build_table(ms, 12 * C - 2, C)
    for r in range(1, len(ms)):
        for d in (-1, 1):
            other = list(ms)
            other[r] += d
            assert model.certifiable(other, C)
            at = model.first_violation(words, other, C)
            assert at is not None and at[0] == r, (other, at)


def test_another_alphabets_table_of_the_same_shape_is_flagged():
    C, ms, other = 32, [0, 40, 52, 70], [0, 41, 55, 70]
    words = oracle.build_table(other, 35 * 70, C)
    assert model.first_violation(words, other, C) is None
    assert model.first_violation(words, ms, C) is not None

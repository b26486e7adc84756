"""CPU: the cases of row_auc_util hold what the GPU test relies on, and the oracle's row_auc tells the `>=` mutant apart on them."""
import numpy as np
import pytest

import row_auc_util as ru
from oracle import user_model_oracle as orc


def test_cases_hold_what_they_name():
    cases = ru.all_cases()
    assert {c.score.shape[1] for c in ru.grid_cases()} == set(ru.T_VALUES)
    assert {c.score.shape[0] for c in ru.grid_cases()} >= set(ru.B_VALUES)
    seen = set()
    for c in cases:
        assert c.score.dtype == np.float32 and c.label.dtype == np.float32 and np.isfinite(c.score).all()
        auc, top1, pairs = ru.reference(c)
        assert pairs.max() < 2 ** 24, c.name                        # gt, eq and the class counts are exact integers in fp32
        assert np.all((auc == -1) == (pairs == 0)) and np.all((auc[pairs > 0] >= 0) & (auc[pairs > 0] <= 1)), c.name
        if c.length is not None:
            assert np.all(top1[c.length <= 0] == 0) and np.all(auc[c.length <= 1] == -1), c.name
            seen |= {"zero" if n == 0 else "negative" if n < 0 else "beyond" if n > c.score.shape[1] else "one" if n == 1 else "some"
                     for n in c.length}
            T = c.score.shape[1]
            for b, n in enumerate(np.clip(c.length, 0, T)):          # the padding would win the argmax and count as positive
                assert np.all(c.score[b, n:] == 9.0) and np.all(c.label[b, n:] == 1.0)
        seen |= {"half"} if (c.label == 0.5).any() else set()
        seen |= {"single class"} if (pairs == 0).any() else set()
    assert seen == {"zero", "negative", "beyond", "one", "some", "half", "single class"}
    for c in ru.tie_cases():
        assert list(ru.reference(c)[1]) == [1, 0], c.name            # first index wins: a hit at 5, a miss at the later one
        assert (70 % 64 != 5 % 64) and (69 % 64 == 5 % 64)


def test_labels_of_one_half_are_negatives():
    assert orc.row_auc([0.5, 1.0, 0.75, 0.5], [0.9, 0.8, 0.1, 0.2]) == (1 + 0) / 4
    c = ru.Case("half", np.array([[0.9, 0.8, 0.1, 0.2]], dtype=np.float32), np.array([[0.5, 1.0, 0.75, 0.5]], dtype=np.float32), None)
    auc, top1, pairs = ru.reference(c)
    assert auc[0] == 0.25 and pairs[0] == 4 and top1[0] == 0


@pytest.mark.parametrize("mutant", ru.MUTANTS)
def test_the_oracle_tells_the_mutant_apart(mutant):
    """on every case that has a row with both classes: scores on four levels always tie somewhere"""
    for c in ru.all_cases():
        good, _, pairs = ru.reference(c)
        bad = ru.reference(c, mutant=mutant)[0]
        if (pairs > 0).any() and c.score.shape[1] >= 63:
            assert np.max(np.abs(good - bad)) > 1e-3, c.name

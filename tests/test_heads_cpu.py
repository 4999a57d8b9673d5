"""The host-side checks the heads share (gae_dgl_amd/ops/_heads.py), on CPU tensors: the lambda path and its messages,
the default folds (values recorded from ops.logreg's and ops.ridge's own copies before they moved), the fold lists and
the choice among scores."""
import pytest
import torch

from gae_dgl_amd.ops._heads import _choose, _default_fold, _fold_lists, _lambda_path

PATH13 = [10.0 ** (e / 2.0) for e in range(-6, 7)]
CPU = torch.device("cpu")


def test_lambda_path_forms():
    assert _lambda_path(None, 5, 64, PATH13) == (PATH13, 5)
    assert _lambda_path(None, 1, 64, [1.0]) == ([1.0], 1)
    lam, F = _lambda_path(torch.tensor([[0.5, 2.0], [0.0, 8.0]]), 3.0, 64, PATH13)
    assert lam == [0.5, 2.0, 0.0, 8.0] and F == 3 and type(F) is int
    assert _lambda_path(0.25, 1, 64, PATH13) == ([0.25], 1)
    assert _lambda_path((1, 2), 2, 2, PATH13) == ([1.0, 2.0], 2)
    assert all(type(v) is float for v in _lambda_path((1, 2), 2, 2, PATH13)[0])


@pytest.mark.parametrize("lambdas, folds, text", [
    (None, 0, "folds: an integer in 1..32, not 0"),
    (None, 33, "folds: an integer in 1..32, not 33"),
    (None, True, "folds: an integer in 1..32, not True"),
    (None, 2.5, "folds: an integer in 1..32, not 2.5"),
    ([], 5, "lambdas: 1..64 values, not 0"),
    ([1.0] * 65, 5, "lambdas: 1..64 values, not 65"),
    ([1.0, -1.0], 5, "lambdas: finite values >= 0, not [1.0, -1.0]"),
    ([float("inf")], 5, "lambdas: finite values >= 0, not [inf]"),
    (torch.tensor([float("nan")]), 5, "lambdas: finite values >= 0, not [nan]"),
    (None, 1, "folds=1 is a plain fit without CV: it takes exactly one lambda, not 13"),
    ([1.0, 2.0], 1, "folds=1 is a plain fit without CV: it takes exactly one lambda, not 2"),
])
def test_lambda_path_errors(lambdas, folds, text):
    with pytest.raises(ValueError) as e:
        _lambda_path(lambdas, folds, 64, PATH13)
    assert str(e.value) == text


def test_lambda_path_limits_are_the_callers():
    with pytest.raises(ValueError) as e:
        _lambda_path([1.0] * 3, 2, 2, PATH13)
    assert str(e.value) == "lambdas: 1..2 values, not 3"
    with pytest.raises(ValueError) as e:
        _lambda_path(None, 9, 64, PATH13, 8)
    assert str(e.value) == "folds: an integer in 1..8, not 9"


FOLD_64_32_1 = [8, 12, 30, 5, 4, 3, 9, 27, 29, 16, 2, 31, 18, 12, 23, 8, 9, 26, 29, 10, 22, 25, 16, 24, 24, 26, 17, 14, 28, 22, 10,
                6, 5, 11, 11, 19, 13, 0, 6, 31, 25, 2, 19, 27, 20, 28, 14, 4, 15, 7, 1, 21, 30, 17, 20, 0, 15, 13, 18, 21, 1, 3,
                23, 7]


@pytest.mark.parametrize("n, F, seed, want", [
    (10, 3, 0, [0, 1, 0, 1, 0, 0, 2, 2, 1, 2]),
    (7, 1, 5, [0, 0, 0, 0, 0, 0, 0]),
    (64, 32, 1, FOLD_64_32_1),
])
def test_default_fold_is_the_recorded_permutation(n, F, seed, want):
    fold = _default_fold(n, F, seed)
    assert fold.dtype == torch.int64 and fold.device == CPU and fold.tolist() == want
    assert torch.bincount(fold, minlength=F).tolist() == [n // F + (f < n % F) for f in range(F)]


def test_fold_lists():
    fold = torch.tensor([2, 0, -1, 1, 0, 2, 1, -1, 0, 2])
    rows, fold_ptr, counts = _fold_lists(fold, 10, 3, 0, CPU)
    assert rows.tolist() == [1, 4, 8, 3, 6, 0, 5, 9]                   # ascending inside a fold (a stable sort), -1 dropped
    assert fold_ptr.tolist() == [0, 3, 5, 8] and counts.tolist() == [3, 2, 3]
    assert fold_ptr.tolist()[1:] == counts.cumsum(0).tolist()
    assert (rows.dtype, fold_ptr.dtype, counts.dtype) == (torch.int32, torch.int32, torch.int64)
    rows, fold_ptr, counts = _fold_lists(None, 10, 3, 0, CPU)          # the default fold of (10, 3, 0)
    assert rows.tolist() == [0, 2, 4, 5, 1, 3, 8, 6, 7, 9] and fold_ptr.tolist() == [0, 4, 7, 10]
    assert counts.tolist() == [4, 3, 3]
    rows, fold_ptr, counts = _fold_lists(torch.tensor([0, 0, 0], dtype=torch.int32), 3, 1, 0, CPU)
    assert rows.tolist() == [0, 1, 2] and fold_ptr.tolist() == [0, 3] and counts.tolist() == [3]


@pytest.mark.parametrize("fold, n, F, text", [
    (torch.tensor([0, 2, 2, 0]), 4, 3, "fold: fold 1 holds no rows (sizes [2, 0, 2])"),
    (torch.tensor([-1, -1]), 2, 2, "fold: fold 0 holds no rows (sizes [0, 0])"),
    (torch.tensor([0.0, 1.0]), 2, 2, "fold: an int tensor [2] with values in -1..1"),
    (torch.tensor([True, False]), 2, 2, "fold: an int tensor [2] with values in -1..1"),
    ([0, 1], 2, 2, "fold: an int tensor [2] with values in -1..1"),
    (torch.tensor([0, 1, 0]), 2, 2, "fold: an int tensor [2] with values in -1..1"),
    (torch.tensor([0, 2]), 2, 2, "fold: values in -1..1 (-1 = left out), got 0..2"),
    (torch.tensor([-2, 1]), 2, 2, "fold: values in -1..1 (-1 = left out), got -2..1"),
])
def test_fold_lists_errors(fold, n, F, text):
    with pytest.raises(ValueError) as e:
        _fold_lists(fold, n, F, 0, CPU)
    assert str(e.value) == text


def test_choose():
    nan = float("nan")
    assert _choose([True, True, True], [2.0, 1.0, 1.0]) == 1           # a tie: the lower index
    assert _choose([True, True, True], [1.0, 1.0, 1.0]) == 0
    assert _choose([True, True], [nan, 3.0]) == 1                      # NaN is never chosen
    assert _choose([True, True], [3.0, nan]) == 0
    assert _choose([False, True, True], [0.0, nan, nan]) == -1
    assert _choose([False, False], [1.0, 2.0]) == -1 and _choose([], []) == -1

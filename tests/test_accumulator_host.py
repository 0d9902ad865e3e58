"""The streaming analyses' shared row check without a GPU (pyhillfit_amd/accumulator.py): on CPU tensors, the ValueError texts the
accumulator classes raise for a wrong rank, problem count, chain count, too few columns, dtype, layout and device."""
import pytest
import torch

from pyhillfit_amd import accumulator

CPU = torch.device("cpu")
Q, C, COLS = 2, 70, 3


def good():
    return torch.zeros((9, Q, COLS + 1, C), dtype=torch.float64)


def test_accepts_the_rows_of_a_sampler():
    accumulator.check_rows(good(), Q, C, COLS, CPU)
    accumulator.check_rows(good()[:0], Q, C, COLS, CPU)
    accumulator.check_rows(good()[2:5], Q, C, COLS + 1, CPU)              # a cut along the rows stays contiguous


@pytest.mark.parametrize("name,rows", [
    ("rank", good()[0]),
    ("Q", torch.zeros((9, Q + 1, COLS + 1, C), dtype=torch.float64)),
    ("C", torch.zeros((9, Q, COLS + 1, C - 6), dtype=torch.float64)),
    ("columns", torch.zeros((9, Q, COLS - 1, C), dtype=torch.float64)),
])
def test_shape(name, rows):
    with pytest.raises(ValueError) as e:
        accumulator.check_rows(rows, Q, C, COLS, CPU)
    assert str(e.value) == "rows must be [n][%d][>= %d][%d], got %s" % (Q, COLS, C, tuple(rows.shape))


@pytest.mark.parametrize("name,rows,device", [
    ("float32", good().float(), CPU),
    ("non-contiguous", good()[:, :, :, ::2], CPU),
    ("non-contiguous columns", good()[:, :, 1:], CPU),
    ("device", good(), torch.device("cuda:0")),
])
def test_tensor(name, rows, device):
    chains = rows.shape[3]
    with pytest.raises(ValueError) as e:
        accumulator.check_rows(rows, Q, chains, COLS, device)
    assert str(e.value) == "rows must be a contiguous float64 tensor on %s" % device
    if device.type == "cuda":
        assert str(e.value).endswith("on cuda:0")


def test_the_shape_is_reported_before_the_tensor():
    with pytest.raises(ValueError, match=r"rows must be \[n\]"):
        accumulator.check_rows(good().float()[0], Q, C, COLS, CPU)


def test_classes_refuse_a_cpu_device_by_their_own_name():
    from pyhillfit_amd import batch_means, correlations, design, diagnostics
    for cls, args in ((diagnostics.ChainDiagnostics, (1, 64, 3, 100)), (batch_means.BatchMeans, (1, 64, 3, 100)),
                      (correlations.PosteriorCorrelations, (1, 64, 3, 100)), (design.NextDose, (2, 1, 64, [[1.0, 2.0]]))):
        with pytest.raises(ValueError) as e:
            cls(*args, device="cpu")
        assert str(e.value) == "%s runs on a GPU device, not cpu" % cls.__name__

"""CPU-only checks of the dropout keep function through its NumPy mirror (phenaki_pytorch_amd/dropout.py: the definition the device
function in csrc/common.hpp has to reproduce byte for byte, tests/test_dropout_gpu.py)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from phenaki_pytorch_amd import dropout as D  # noqa: E402

ROWS, COLS = 1024, 1024                     # N = 2^20 decisions
N = ROWS * COLS
PS = (0.1, 0.25, 0.5)


@pytest.fixture(scope='module')
def masks():
    return {p: D.keep_mask(1234, 8, ROWS, COLS, p) for p in PS}


def test_mirror_is_deterministic(masks):
    again = D.keep_mask(1234, 8, ROWS, COLS, 0.25)
    assert again.dtype == np.uint8 and again.shape == (ROWS, COLS)
    assert np.array_equal(again, masks[0.25])
    # the decision of an element does not depend on the range it is asked in
    assert np.array_equal(D.keep_mask(1234, 8, 37, 1001, 0.25), masks[0.25][:37, :1001])
    # another seed / another offset: another mask
    assert not np.array_equal(D.keep_mask(1235, 8, ROWS, COLS, 0.25), masks[0.25])
    assert not np.array_equal(D.keep_mask(1234, 12, ROWS, COLS, 0.25), masks[0.25])
    assert not np.array_equal(D.keep_mask(1234 + (1 << 32), 8, ROWS, COLS, 0.25), masks[0.25])
    assert not np.array_equal(D.keep_mask(1234, 8 + (1 << 32), ROWS, COLS, 0.25), masks[0.25])


@pytest.mark.parametrize('p', PS)
def test_effective_probability(p):
    thr, p_eff, scale = D.quantize(p)
    assert abs(p_eff - p) <= 2.0 ** -9
    assert p_eff == thr / 256.
    assert scale == 1. / (1. - p_eff)


def test_effective_probability_everywhere():
    for p in np.linspace(0., 1., 4097):
        thr, p_eff, scale = D.quantize(p)
        assert abs(p_eff - p) <= 2.0 ** -9 and 0 <= thr <= 256
    assert D.quantize(0.)[0] == 0 and D.quantize(1.) == (256, 1., 0.)
    with pytest.raises(ValueError):
        D.quantize(1.5)


@pytest.mark.parametrize('p', PS)
def test_keep_fraction(masks, p):
    p_eff = D.quantize(p)[1]
    sigma = math.sqrt(p_eff * (1. - p_eff) / N)
    frac = masks[p].mean(dtype=np.float64)
    assert abs(frac - (1. - p_eff)) <= 5. * sigma, (frac, 1. - p_eff, sigma)


def _lag1(m, axis):
    x = m.astype(np.float64)
    x = x - x.mean()
    a, b = (x[:, :-1], x[:, 1:]) if axis == 1 else (x[:-1], x[1:])
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize('p', PS)
def test_lag1_correlation(masks, p):
    bound = 5. / math.sqrt(N)
    along_rows, along_cols = _lag1(masks[p], 1), _lag1(masks[p], 0)
    assert abs(along_rows) < bound, (along_rows, bound)
    assert abs(along_cols) < bound, (along_cols, bound)


def test_extremes():
    assert D.keep_mask(1, 0, 16, 33, 0.).all()
    assert not D.keep_mask(1, 0, 16, 33, 1.).any()

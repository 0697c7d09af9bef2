"""The importance-sampling entries check num_pred / R and adapt_rounds over the
whole int32 range: every value outside [25, 1024] and [0, ADAPT_MAX_ROUNDS],
the extremes of int32 among them, is MDFIT_E_ARG with the argument's message
before any launch (no device needed: the pointers are never read)."""

from __future__ import annotations

import ctypes

import pytest

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
D = ctypes.c_void_p(16)
D4 = (D, D, D, D)


@pytest.fixture(scope="module")
def lib():
    from metadamage_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("R", [INT32_MIN, INT32_MIN + 1, -1, 0, 24, 1025, INT32_MAX])
def test_num_pred_out_of_range_is_an_argument_error(lib, R):
    assert lib.mdfit_map_pred(*D4, 1, 256, R, 0, 0, D, D, None, None, None) == -1
    assert lib.mdfit_last_error() == b"num_pred must be in [25, 1024]"
    assert lib.mdfit_map_pred_adapt(*D4, 1, 256, R, 3, 0, 0, D, D, None, None, None, None) == -1
    assert lib.mdfit_last_error() == b"num_pred must be in [25, 1024]"
    assert lib.mdfit_resample(D, 1, 256, R, D, D, None) == -1
    assert lib.mdfit_last_error() == b"R must be in [25, 1024]"


@pytest.mark.parametrize("rounds", [INT32_MIN, INT32_MIN + 1, -1, 5, INT32_MAX])
def test_adapt_rounds_out_of_range_is_an_argument_error(lib, rounds):
    from metadamage_amd import _lib

    assert _lib.ADAPT_MAX_ROUNDS == 4
    assert lib.mdfit_map_psis_adapt(*D4, 1, 256, rounds, 0, 0, D, None, None, None) == -1
    assert lib.mdfit_last_error() == b"adapt_rounds must be in [0, 4]"
    assert lib.mdfit_map_waic_adapt(*D4, 1, 256, rounds, 0, 0, D, None, None, None, None) == -1
    assert lib.mdfit_last_error() == b"adapt_rounds must be in [0, 4]"
    assert lib.mdfit_map_evidence_adapt(*D4, 1, 256, rounds, 0, 0, D, None, None, None) == -1
    assert lib.mdfit_last_error() == b"adapt_rounds must be in [0, 4]"
    assert lib.mdfit_map_pred_adapt(*D4, 1, 256, 1000, rounds, 0, 0, D, D, None, None, None, None) == -1
    assert lib.mdfit_last_error() == b"adapt_rounds must be in [0, 4]"


@pytest.mark.parametrize("S", [INT32_MIN, -1, 24, 1025, INT32_MAX])
def test_num_draws_out_of_range_is_an_argument_error(lib, S):
    assert lib.mdfit_map_psis(*D4, 1, S, 0, 0, D, None, None) == -1
    assert lib.mdfit_last_error() == b"num_draws must be in [25, 1024]"
    assert lib.mdfit_map_pred(*D4, 1, S, 1000, 0, 0, D, D, None, None, None) == -1
    assert lib.mdfit_last_error() == b"num_draws must be in [25, 1024]"
    assert lib.mdfit_psis_weights(D, 1, S, D, D, None) == -1
    assert lib.mdfit_last_error() == b"S must be in [25, 1024]"

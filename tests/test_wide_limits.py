"""The input-dimension limit of the engine (CPU test: tgp_create checks d before it looks for a device)."""
import pytest


def test_input_dimension_limit_is_1024_and_a_shape_error():
    from trieste_amd import _lib
    from trieste_amd.engine import GPEngine

    assert _lib.MAX_D == 1024 and _lib.NARROW_MAX_D == 32
    for d in (0, _lib.MAX_D + 1):
        with pytest.raises(ValueError, match=r"d must be in 1\.\.1024"):
            GPEngine(d)

"""Host-side checks of the row-tiled adaptive render (no GPU needed): the two new entry points'
argument checks, and the condition of DESIGN.md §18's "Row tiles" invariant, stated once in code.
"""
import ctypes

import numpy as np
import pytest

from cpppathtracer_amd import _lib, tiling

INVALID_ARG = 1


def test_null_arguments():
    L = _lib.load()
    active = ctypes.c_int(7)
    cam = np.zeros(136, dtype=np.uint8)
    assert L.cpt_adaptive_step(None, ctypes.byref(active)) == INVALID_ARG
    assert L.cpt_adaptive_step(None, None) == INVALID_ARG
    assert active.value == 7
    assert L.cpt_adaptive_begin(None, ctypes.c_void_p(cam.ctypes.data), 8, 32, 4, ctypes.c_float(0.1), 8, 0) == INVALID_ARG
    assert L.cpt_adaptive_begin(None, None, 8, 32, 4, ctypes.c_float(0.1), 8, 0) == INVALID_ARG


@pytest.mark.parametrize("height", [12, 44, 64, 1080])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_partition_rows_deals_whole_ascending_blocks(world, height):
    """Each rank's rows are whole 8-row blocks of the frame (the last one possibly partial, as in
    the frame itself) in ascending order, and the ranks' rows partition the frame.  Then local rows
    8i .. 8i+7 of a rank are one block of the frame, so each 8x8 tile of the rank's context is an
    8x8 tile of the monolithic frame with the same pixels: the adaptive criterion, which is per
    tile, stops it at the same round."""
    B = tiling.BLOCK_ROWS
    assert B == 8
    seen = []
    for rank in range(world):
        rows = tiling.partition_rows(height, world, rank)
        assert (np.diff(rows) > 0).all()
        for i in range(0, rows.size, B):
            local = rows[i:i + B]                                   # one row of the context's 8x8 tiles
            b = int(local[0]) // B
            want = np.arange(b * B, min((b + 1) * B, height))       # one whole block of the frame
            np.testing.assert_array_equal(local, want)
        seen.append(rows)
    np.testing.assert_array_equal(np.sort(np.concatenate(seen)), np.arange(height))

"""The arithmetic that sizes a persistent launch, on the host (cpt_launch_grid_host, no GPU): the
function every megakernel launch runs with its context's own CU count, blocks per CU and cap
(cpt_internal.hpp megakernel_want, grid_workgroups, consolidation_chains).  The expected values
follow from  want = ceil(tiles * 64 * ceil(64 / per_wave) / block),  per_wave = max(1, lanes /
max(1, replicate)),  grid = min(want, blocks_per_cu * cus), then the cap when it is positive."""
import ctypes

import pytest

from cpppathtracer_amd import _lib

LDS_BLOCK = 1024
HO_SLOTS = (LDS_BLOCK // 256 - 1) * 256   # ho_slots<LDS_BLOCK>(): hand-over slots per workgroup


def _grid(cus, per_cu, block, tiles, lanes=64, replicate=1, cap=0):
    wg, chains = ctypes.c_int(-1), ctypes.c_uint64(0)
    st = _lib.load().cpt_launch_grid_host(cus, per_cu, block, tiles, lanes, replicate, cap, ctypes.byref(wg),
                                          ctypes.byref(chains))
    assert st == 0
    return wg.value, chains.value


@pytest.mark.parametrize("cus,per_cu,block,tiles,lanes,replicate,cap,want", [
    (256, 1, 1024, 40, 64, 1, 0, 3),        # 64 x 40: ceil(2560 / 1024)
    (256, 1, 1024, 40, 64, 1, 1, 1),        # the cap
    (256, 1, 1024, 32400, 64, 1, 0, 256),   # 1920 x 1080: every resident slot once
    (32, 1, 1024, 32400, 64, 1, 0, 32),     # a partition of 32 CUs
    (256, 1, 1024, 40, 4, 1, 0, 40),        # 4 lanes of a wave take pixels: 16 waves per tile
    (256, 1, 1024, 40, 64, 2, 0, 5),        # two lanes per pixel
    (256, 3, 256, 40, 64, 1, 0, 10),        # the kernels of 256 lanes
    (256, 3, 256, 32400, 64, 1, 0, 768),
    (256, 1, 1024, 0, 64, 1, 0, 0),         # nothing to launch
])
def test_workgroups(cus, per_cu, block, tiles, lanes, replicate, cap, want):
    assert _grid(cus, per_cu, block, tiles, lanes, replicate, cap)[0] == want


@pytest.mark.parametrize("cus", [1, 32, 256, 304])
def test_slab_matches_the_resident_workgroups(cus):
    """The hand-over slab holds ho_slots chains for each workgroup the consolidating launch can get
    (one LDS workgroup per CU: 768 x CUs), so the kernel's (blockIdx.x + 1) * ho_slots <= resume_cap
    holds for every workgroup of a grid that fills the device."""
    wg, chains = _grid(cus, 1, LDS_BLOCK, 10 ** 6)
    assert wg == cus
    assert chains == wg * HO_SLOTS == 768 * cus


def test_degenerate_arguments():
    """lanes and replicate below 1 count as 1 (as the launch treats them); a device without CUs,
    a kernel without a block and a null output are refused."""
    assert _grid(256, 1, 1024, 40, lanes=0)[0] == 40 * 64 * 64 // 1024
    assert _grid(256, 1, 1024, 40, replicate=0)[0] == 3
    L = _lib.load()
    wg = ctypes.c_int(0)
    for bad in ((0, 1, 1024, 40), (256, 0, 1024, 40), (256, 1, 0, 40), (256, 1, 1024, -1)):
        assert L.cpt_launch_grid_host(*bad, 64, 1, 0, ctypes.byref(wg), None) == 1   # CPT_ERR_INVALID_ARG
    assert L.cpt_launch_grid_host(256, 1, 1024, 40, 64, 1, 0, None, None) == 1
    assert L.cpt_launch_grid_host(256, 1, 1024, 40, 64, 1, 0, ctypes.byref(wg), None) == 0 and wg.value == 3

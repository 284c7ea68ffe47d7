"""The host scheduler's integer arithmetic, checked without a GPU: which normals tiles ride in which tracker launch of a
tracked frame (normals_tile_split in csrc/gsdf_capi.hip, exported by the test build only)."""
import ctypes as C

import pytest

SIZES = [(160, 120), (640, 480), (1280, 960), (333, 77)]          # the last one ragged: no multiple of the 32 x 16 tile
SPLITS = [(30, 40), (0, 0), (100, 0), (50, 50)]                    # GSDF_NRM_SPLIT: per cent of the tiles in launch 0, launch 1


@pytest.fixture(scope="module")
def split(pkg):
    L = pkg.binding.load_test_lib()
    f = L.gsdf_debug_normals_tile_split
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int)] * 2

    def call(tiles, k, launches, iters, batch, s1, s2):
        lo, hi = C.c_int(-1), C.c_int(-1)
        return (lo.value, hi.value) if f(tiles, k, launches, iters, batch, s1, s2, C.byref(lo), C.byref(hi)) else None
    return call


def _first_batch(iters, batch, head):
    """enqueue_track's first batch: launches 0 .. last; with the stand-in head the fusion launch replaces launch `last`.
    Returns the number of tracker launches issued before the frame's first fusion launch."""
    last = min(iters, batch - 1)
    return last if (head and last >= 1) else last + 1


@pytest.mark.parametrize("W,H", SIZES)
def test_normals_tiles_are_all_computed_before_the_first_fusion_launch(split, W, H):
    tiles = ((W + 31) // 32) * ((H + 15) // 16)
    for iters in range(1, 26):
        for batch in list(range(2, 9)) + [iters + 1]:              # GSDF_FIRST_BATCH 2 .. 8; GSDF_ADAPTIVE=0: one batch of iters + 1
            for s1, s2 in SPLITS:
                for head in (False, True):
                    nl = _first_batch(iters, batch, head)
                    case = (W, H, iters, batch, s1, s2, head)
                    assert nl >= 1, case
                    ranges = []
                    for k in range(nl):
                        r = split(tiles, k, nl, iters, batch, s1, s2)
                        if r is None:
                            continue
                        assert 0 <= r[0] < r[1] <= tiles, (case, k, r)
                        assert k <= 2, (case, k, r)
                        assert (r[0] == 0) == (k == 0), (case, k, r)       # tile 0 (it resets the deferred list): launch 0 only
                        ranges.append(r)
                    # every tile, once: the ranges follow each other from 0 to `tiles`
                    assert ranges and ranges[0][0] == 0 and ranges[-1][1] == tiles, (case, ranges)
                    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), (case, ranges)
                    # the launches a later batch may repeat (k <= 2, three riders' launches) never take tile 0 either
                    for k in (1, 2):
                        r = split(tiles, k, 3, iters, 8, s1, s2)
                        assert r is None or (1 <= r[0] < r[1] <= tiles), (case, k, r)

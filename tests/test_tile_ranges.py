"""gs_tile_ranges alone, through the C ABI, exactly: every tile's [start, end)
is np.searchsorted of the sorted keys, for both kernels (four positions per
thread with 16-B aligned keys and no flags or the default tile's four; one
position per thread otherwise), with the backward's slot flags cleared for
exactly the live entries, and with the entry count read from a device word."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENTRIES = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 70001)
TILES = (19200, 300, 1200, 40, 5000, 7)  # cycled over ENTRIES; 19200 = 160 x 120 tiles
GUARD = 256


def make_keys(rng, T, ntiles):
    """T sorted tile ids below ntiles.  Large tile counts get empty runs longer
    than a wave fill's threshold (32 tiles) at the start, in the middle, before
    the last two entries and after them (the last position's thread: in the
    partial last wave)."""
    if ntiles <= 400:
        return np.sort(rng.integers(0, ntiles, T)).astype(np.uint32)
    ok = np.ones(ntiles - 150, bool)
    ok[:40] = False
    ok[ntiles // 2:ntiles // 2 + 70] = False
    keys = np.sort(rng.choice(np.nonzero(ok)[0], T))
    keys[max(T - 2, 0):] = ntiles - 51
    return keys.astype(np.uint32)


def expected(keys, ntiles):
    t = np.arange(ntiles)
    return np.stack([np.searchsorted(keys, t, "left"), np.searchsorted(keys, t, "right")], 1).astype(np.int32)


def run(pkg, cuda, keys, ntiles, cells=0, offset=0, capacity=None, dev_count=None):
    """One gs_tile_ranges call.  keys: the live entries; capacity: num_pairs
    (default: len(keys)), the entries past the live ones unsorted garbage;
    offset: words the key pointer is moved off its 16-B alignment; cells > 0:
    slot flags pre-filled with 0xFF.  Returns (ranges, flags or None)."""
    N = pkg._native
    lib = N.load()
    cap = len(keys) if capacity is None else capacity
    buf = np.random.default_rng(1).integers(0, max(ntiles, 1), cap + offset + 4).astype(np.uint32)  # (valid tile ids)
    buf[offset:offset + len(keys)] = keys
    kbuf = torch.tensor(buf.view(np.int32), device=cuda)
    k = kbuf[offset:]
    assert (k.data_ptr() % 16 == 0) == (offset % 4 == 0)
    ranges = torch.full((ntiles + GUARD, 2), -7, dtype=torch.int32, device=cuda)
    flags = None
    if cells:
        flags = torch.full((cap * cells + GUARD,), 0xFF, dtype=torch.uint8, device=cuda)
        assert flags.data_ptr() % 16 == 0
    cnt = None if dev_count is None else torch.tensor([dev_count], dtype=torch.int32, device=cuda)
    ra = N.GsRangeArgs(cap, ntiles, N.ptr(k), N.ptr(ranges), N.ptr(flags), cells, N.ptr(cnt))
    N.check(lib.gs_tile_ranges(C.byref(ra), torch.cuda.current_stream().cuda_stream), "gs_tile_ranges")
    torch.cuda.synchronize()
    r = ranges.cpu().numpy()
    assert (r[ntiles:] == -7).all(), "ranges written past the last tile"
    return r[:ntiles], None if flags is None else flags.cpu().numpy()


def check_flags(flags, live, cells, what):
    assert not flags[:live * cells].any(), f"{what}: a live entry's flag is not cleared"
    assert (flags[live * cells:] == 0xFF).all(), f"{what}: a flag past the live entries was written"


# (cells, key offset in words): no flags and the default tile's four take the
# four-position kernel when the keys are 16-B aligned; the rest the one-position kernel
VARIANTS = [(0, 0), (4, 0), (1, 0), (9, 0), (4, 1), (0, 1), (0, 2)]


@pytest.mark.parametrize("cells,offset", VARIANTS)
def test_tile_ranges_exact(pkg, cuda, cells, offset):
    rng = np.random.default_rng(70)
    for i, T in enumerate(ENTRIES):
        for ntiles in (TILES[i % len(TILES)], 19200 if T in (0, 257, 70001) else 64):
            keys = make_keys(rng, T, ntiles)
            want = expected(keys, ntiles)
            if ntiles == 19200 and T > 4:
                empty = want[:, 0] == want[:, 1]
                assert empty[:40].all() and empty[-50:].all() and empty[ntiles // 2:ntiles // 2 + 70].all()
            got, flags = run(pkg, cuda, keys, ntiles, cells, offset)
            assert np.array_equal(got, want), (T, ntiles, cells, offset)
            if cells:
                check_flags(flags, T, cells, (T, ntiles, cells, offset))


@pytest.mark.parametrize("cells,offset", [(0, 0), (4, 0), (9, 0), (4, 3)])
def test_tile_ranges_device_count(pkg, cuda, cells, offset):
    """num_pairs_dev: the entries are min(*num_pairs_dev, num_pairs)."""
    rng = np.random.default_rng(71)
    ntiles = 19200
    for cap, count in ((1025, 1023), (1025, 4), (1024, 0), (70001, 257), (70001, 69999), (257, 257), (257, 100000),
                       (5, 2 ** 31 + 5)):
        live = min(cap, count)
        keys = make_keys(rng, live, ntiles)
        got, flags = run(pkg, cuda, keys, ntiles, cells, offset, capacity=cap,
                         dev_count=int(np.uint32(count).view(np.int32)))
        assert np.array_equal(got, expected(keys, ntiles)), (cap, count, cells, offset)
        if cells:
            check_flags(flags, live, cells, (cap, count, cells, offset))

"""The block -> (tile, z-chunk) map of k_pd_fusedk and k_pd_shift3 (pdk_block_tile in
nsol_pd_common.hpp), read on the host through nsol_pdk_block_map: no GPU.

Mode 1 deals WHOLE tile rows to the XCDs (block b runs on XCD b mod 8 under the round-robin
dispatch), balanced by the volume rows they cover; mode 2 is the earlier map in slabs of
ceil(tiles / 8) tiles, whose formula is written out here; mode 0 is the plain order."""
import ctypes

import pytest

# (name, ny, ntx, footprint rows, rows lost to overlap, z-chunks)
TILINGS = [
    ("512^3 shifted 12:4:256, 22 rows", 512, 4, 22, 5, 2),
    ("512^3 shifted 12:4:256, 21 rows", 512, 4, 21, 5, 2),
    ("512^3 unshifted 12:2:103", 512, 2, 11, 4, 5),
    ("three x-tiles, 43 tile rows", 43 * 6 - 2, 3, 10, 4, 3),
    ("nine tile rows", 9 * 7 - 5, 2, 12, 5, 1),
    ("seven tile rows: plain order", 7 * 17, 4, 22, 5, 2),
]


@pytest.fixture(scope="module")
def lib():
    from nsol_amd import _lib
    return _lib.load()


def _nty(ny, rows, lost):
    valid = rows - lost
    return -(-ny // valid), valid


def _map(lib, mode, ntx, nty, nzc):
    cap = 8 * (nty // 8 + 1) * ntx * nzc + 8 * nzc
    out = (ctypes.c_int * (2 * cap))()
    blocks = lib.nsol_pdk_block_map(mode, ntx, nty, nzc, out, cap)
    assert blocks > 0, (mode, ntx, nty, nzc, blocks)
    return [(out[2 * b], out[2 * b + 1]) for b in range(blocks)]


def test_tilings_are_the_ones_meant():
    got = {name: _nty(ny, rows, lost)[0] for name, ny, ntx, rows, lost, nzc in TILINGS}
    assert list(got.values()) == [31, 32, 74, 43, 9, 7]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name,ny,ntx,rows,lost,nzc", TILINGS)
def test_every_tile_and_chunk_exactly_once(lib, name, ny, ntx, rows, lost, nzc, mode):
    nty, _ = _nty(ny, rows, lost)
    blocks = _map(lib, mode, ntx, nty, nzc)
    live = [t for t in blocks if t != (-1, -1)]
    assert all(t == (-1, -1) or (t[0] >= 0 and t[1] >= 0) for t in blocks)
    assert sorted(live) == [(t, z) for t in range(ntx * nty) for z in range(nzc)]


@pytest.mark.parametrize("name,ny,ntx,rows,lost,nzc", TILINGS)
def test_whole_tile_rows_balanced_by_volume_rows(lib, name, ny, ntx, rows, lost, nzc):
    nty, valid = _nty(ny, rows, lost)
    blocks = _map(lib, 1, ntx, nty, nzc)
    if nty < 8:                               # trivially uniform: today's plain order
        assert blocks == [(b % (ntx * nty), b // (ntx * nty)) for b in range(len(blocks))]
        return
    xcd_of_row = {}
    for b, (tile, zc) in enumerate(blocks):
        if tile >= 0:
            xcd_of_row.setdefault(tile // ntx, set()).add(b & 7)
    # all tiles of a tile row (every z-chunk of them) share one XCD
    assert all(len(x) == 1 for x in xcd_of_row.values())
    owner = [next(iter(xcd_of_row[ty])) for ty in range(nty)]
    assert owner == sorted(owner) and set(owner) == set(range(8))   # contiguous runs
    # volume rows per XCD, the last tile row clipped to ny
    vol = [0] * 8
    for ty in range(nty):
        vol[owner[ty]] += min(valid, ny - ty * valid)
    assert sum(vol) == ny
    assert max(vol) - min(vol) <= valid, vol
    # no split of whole tile rows has a lighter heaviest XCD
    assert max(vol) <= -(-nty // 8) * valid
    # inside an XCD: x-fastest, then y, then z-chunk
    for x in range(8):
        mine = [t for b, t in enumerate(blocks) if b & 7 == x and t[0] >= 0]
        assert mine == sorted(mine, key=lambda t: (t[1], t[0]))
        # ... and the surplus blocks come last
        flags = [t[0] >= 0 for b, t in enumerate(blocks) if b & 7 == x]
        assert flags == sorted(flags, reverse=True)


def test_512_cubed_shares(lib):
    """22-row footprints: 31 tile rows, seven XCDs with four and one with three (68 volume
    rows at the most, 51 at the least); 21-row footprints: four each, 64 volume rows."""
    for rows, want in ((22, [51] + [68] * 6 + [53]), (21, [64] * 8)):
        nty, valid = _nty(512, rows, 5)
        vol = [0] * 8
        for b, (tile, zc) in enumerate(_map(lib, 1, 4, nty, 2)):
            if tile >= 0 and zc == 0 and tile % 4 == 0:
                vol[b & 7] += min(valid, 512 - (tile // 4) * valid)
        assert vol == want


@pytest.mark.parametrize("name,ny,ntx,rows,lost,nzc", TILINGS)
def test_mode_2_is_the_earlier_formula(lib, name, ny, ntx, rows, lost, nzc):
    nty, _ = _nty(ny, rows, lost)
    tiles = ntx * nty
    blocks = _map(lib, 2, ntx, nty, nzc)
    if tiles < 16:
        want = [(b % tiles, b // tiles) for b in range(tiles * nzc)]
    else:
        slab = (tiles + 7) // 8
        want = []
        for b in range(8 * slab * nzc):
            xcd, j = b & 7, b >> 3
            tile = xcd * slab + j % slab
            want.append((tile, j // slab) if tile < tiles else (-1, -1))
    assert blocks == want


def test_invalid_arguments(lib):
    out = (ctypes.c_int * 16)()
    assert lib.nsol_pdk_block_map(3, 2, 9, 1, out, 8) == -1
    assert lib.nsol_pdk_block_map(1, 0, 9, 1, out, 8) == -1
    assert lib.nsol_pdk_block_map(1, 2, 9, 1, None, 8) == -1
    assert lib.nsol_pdk_block_map(1, 2, 9, 1, out, 7) == -1      # 32 blocks do not fit

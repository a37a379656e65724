"""The dealing of blocks to (tile, frame) with the host's constants (csrc/trt_deal.h), through the
library's host-only diagnostic entries: no GPU.

The map must be, value for value, what the kernels computed before the constants moved to the
host: `old_xcd_deal` / `old_inter_tile` below restate that code (integer `//` and `%` on the
launch's shape, nothing precomputed).  The magic divisions are checked against the host compiler's
`/` over every dividend below 2^26 (block indices; tiles stay below 2^24) for each divisor the
shapes here meet, and against Python's `//` and `%` on samples of the whole 32-bit range.

(The row order of pair launches that this file's name speaks of, deal_order, did not meet its
gate and is not built: DESIGN.md 7.)"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

from vkcomputeshader_tinyraytracer_amd._lib import lib

SHAPES = [(1024, 768), (128, 96), (136, 104), (256, 96), (100, 52)]
FRAMES = [2, 3, 20, 33, 64]
U32P = ctypes.POINTER(ctypes.c_uint32)


def shape(width, height):
    ntx, tyn = (width + 7) // 8, (height + 7) // 8
    return ntx, ntx * tyn


def host_mult(ntx, ntiles):
    """fill_args' xcd_mult: near 0.618 of the dealt chunks, coprime to them."""
    nfull = ((ntx // 2) * (ntiles // ntx // 2) // 8) * 8
    if nfull == 0 or nfull >= 65536:
        return 1
    m = int(0.6180339887 * nfull) | 1
    while math.gcd(m, nfull) != 1:
        m += 2
    return m % nfull or 1


# ---- the dealing as the kernels computed it before (vectorised over the blocks) -------------

def old_xcd_deal(ntx, ntiles, b, roff, skew=0, mult=1, perm=False):
    b = np.asarray(b, np.int64)
    roff = np.broadcast_to(np.asarray(roff, np.int64), b.shape)
    tyn = ntiles // ntx
    cw, ch = ntx // 2, tyn // 2
    nchunk = cw * ch
    nfull = (nchunk // 8) * 8

    def chunk_tile(chunk, sub):
        cx, cy = chunk % max(cw, 1), chunk // max(cw, 1)
        if skew:
            cx = (cx + skew * cy) % max(cw, 1)
        return (cy * 2 + sub // 2) * ntx + cx * 2 + sub % 2

    j, x = b // 8, (b % 8 + roff) & 7
    k = (j // 4) * 8 + x
    if perm:
        k = (k * mult) % max(nfull, 1)
    even = chunk_tile(k, j % 4)
    r = b - nfull * 4
    nc = (nchunk - nfull) * 4
    last_chunks = chunk_tile(nfull + r // 4, r % 4)
    r1 = r - nc
    na = ch * 2 if ntx & 1 else 0
    right = r1 * ntx + (ntx - 1)
    bottom = (ch * 2) * ntx + (r1 - na)
    return np.where(b < nfull * 4, even, np.where(r < nc, last_chunks, np.where(r1 < na, right, bottom)))


def old_xcd_tile(ntx, ntiles, b, f, rot, skew):
    return old_xcd_deal(ntx, ntiles, b, (np.asarray(f) >> (rot - 1)) if rot else 0, skew)


def old_inter_tile(ntx, ntiles, F, inter, skew=0, mult=1):
    """(tile, frame) of blocks [0, ntiles * F)."""
    vb = np.arange(ntiles * F, dtype=np.int64)
    nfull = ((ntx // 2) * (ntiles // ntx // 2) // 8) * 8
    per = nfull * 4
    x, i = vb % 8, vb // 8
    q = i // 4
    f = q % F
    g = q // F
    fixed = inter == 2
    c = x if fixed else (x + f) & 7
    even = old_xcd_deal(ntx, ntiles, (g * 4 + i % 4) * 8 + c, 0, skew, mult, fixed)
    r, nl = vb - F * per, max(ntiles - per, 1)
    left = old_xcd_deal(ntx, ntiles, per + r % nl, 0, skew, mult)
    head = vb < F * per
    return np.where(head, even, left), np.where(head, f, r // nl)


# ---- the library's --------------------------------------------------------------------------

def deal_map(ntx, ntiles, F, rot=1, skew=0, inter=1, mult=1):
    fn = lib().trt_diag_deal_map
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint32] * 7 + [U32P, U32P]
    tile, frame = np.zeros(ntiles * F, np.uint32), np.zeros(ntiles * F, np.uint32)
    rc = fn(ntx, ntiles, F, rot, skew, inter, mult, tile.ctypes.data_as(U32P), frame.ctypes.data_as(U32P))
    assert rc == 0, rc
    return tile.astype(np.int64), frame.astype(np.int64)


# ---- the map is the old one, value for value --------------------------------------------------

@pytest.mark.parametrize("width,height", SHAPES)
def test_single_frame_map_is_the_old_xcd_tile(width, height):
    ntx, ntiles = shape(width, height)
    for skew in (0, 3):
        tile, frame = deal_map(ntx, ntiles, 1, rot=1, skew=skew, inter=0)
        assert np.array_equal(tile, old_xcd_tile(ntx, ntiles, np.arange(ntiles), 0, 1, skew))
        assert not frame.any()
        assert np.array_equal(np.sort(tile), np.arange(ntiles))


@pytest.mark.parametrize("width,height", SHAPES)
@pytest.mark.parametrize("rot", [0, 1, 3])
def test_frame_major_map_is_the_old_xcd_tile(width, height, rot):
    ntx, ntiles = shape(width, height)
    F = 5
    tile, frame = deal_map(ntx, ntiles, F, rot=rot, skew=0, inter=0)
    vb = np.arange(ntiles * F)
    assert np.array_equal(frame, vb // ntiles)
    assert np.array_equal(tile, old_xcd_tile(ntx, ntiles, vb % ntiles, vb // ntiles, rot, 0))


@pytest.mark.parametrize("width,height", SHAPES)
@pytest.mark.parametrize("nframes", FRAMES)
@pytest.mark.parametrize("inter", [1, 2])
def test_interleaved_map_is_the_old_inter_tile(width, height, nframes, inter):
    ntx, ntiles = shape(width, height)
    mult = host_mult(ntx, ntiles)
    for F in ((nframes + 1) // 2, nframes):  # frame pairs, and frames (TRT_FRAME_GROUP=1)
        tile, frame = deal_map(ntx, ntiles, F, inter=inter, mult=mult)
        want_t, want_f = old_inter_tile(ntx, ntiles, F, inter, mult=mult)
        assert np.array_equal(tile, want_t) and np.array_equal(frame, want_f)
        # a bijection of (tile, frame)
        assert np.array_equal(np.sort(frame * ntiles + tile), np.arange(ntiles * F))


# ---- the magic divisions ---------------------------------------------------------------------

def divisors():
    """Every divisor the shapes and frame counts above meet: ntx, cw, F, ntiles - per."""
    d = set()
    for width, height in SHAPES:
        ntx, ntiles = shape(width, height)
        cw, ch = ntx // 2, ntiles // ntx // 2
        d |= {ntx, cw, ntiles - (cw * ch // 8) * 8 * 4}
    for n in FRAMES:
        d |= {n, (n + 1) // 2}
    return sorted(d - {0})


def test_magic_division_is_exact():
    rng_fn = lib().trt_diag_deal_div_range
    rng_fn.restype = ctypes.c_uint64
    rng_fn.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]
    at_fn = lib().trt_diag_deal_div
    at_fn.restype = None
    at_fn.argtypes = [ctypes.c_uint32, U32P, ctypes.c_uint32, U32P]
    rng = np.random.default_rng(7)
    edge = np.array([0, 1, 2, 2**24 - 1, 2**24, 2**26 - 1, 2**26, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1], np.uint64)
    for d in divisors() + [1, 2, 3, 7, 641, 2**16, 2**26 - 1, 2**31, 2**32 - 1]:
        # every block index and tile the kernels can form, against the host compiler's n / d ...
        assert rng_fn(d, 0, 1 << 26) == 0, d
        # ... and against Python's // and % on samples of the whole 32-bit range and multiples' edges
        k = rng.integers(0, 2**32 // d + 1, 2000, dtype=np.uint64) * np.uint64(d)
        n = np.concatenate([edge, rng.integers(0, 2**32, 20000, dtype=np.uint64), k, k + np.uint64(d - 1), k - np.uint64(1)])
        n = (n % np.uint64(2**32)).astype(np.uint32)
        q = np.zeros(len(n), np.uint32)
        at_fn(d, n.ctypes.data_as(U32P), len(n), q.ctypes.data_as(U32P))
        n64, q64 = n.astype(np.int64), q.astype(np.int64)
        assert np.array_equal(q64, n64 // d) and np.array_equal(n64 - q64 * d, n64 % d), d

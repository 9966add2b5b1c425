"""Inputs, exact reference and expected dispatch for the masked Gram pass of the L-BFGS-B
backend (nsol_amd/csrc/nsol_lbfgsb.hip: k_masked_gram, k_masked_gram_dma,
k_masked_gram_mfma, closed by k_gram_final / k_gram2_final).  Plain NumPy, shared by
test_gram_kernels_host.py (which proves what is claimed here) and test_gram_kernels_gpu.py.

LATTICE INPUTS.  Vector k at voxel i is a non-zero integer in [-31, -1] u [1, 31] taken
from a 32-bit integer hash of (i, k); the three base vectors of the reduced gradient come
from the same hash.  BCOEF3 = (-0.75, 0.75, -1), WCOEF[k] are multiples of 1/8 in [-1, 1].
Then, whatever the order of the additions and with or without FMA,
  * a Gram entry is a sum of integers |v_i v_j| <= 961: every partial sum is an integer of
    magnitude <= 961 n < 2^53  (n <= NMAX: < 2^31);
  * W'Z b with b = b0 base0 + b1 base1 + b2 base2: 4 b is an integer, |4 b| <= 310, b is
    exact in float32, every partial sum is a multiple of 1/4 below 31 * 77.5 n < 2^53;
  * r = b + sum_k WCOEF[k] v_k: every term and partial sum is a multiple of 1/8 of
    magnitude <= 77.5 + 24 * 31 = 821.5, and 8 * 821.5 < 2^24: exact in float32.
So the expected values are integer sums, the same for float32 and float64 and for every
kernel, and the gate is equality.  (test_gram_kernels_host.py checks each bound on the
arrays themselves.)

THE MASK holds {-128, -1, 0} (free, about 60 %) and {1, 2, 127} (not free) from another
hash of i alone.  It has no period: were it periodic in a tile (256 .. 2048 voxels) or in
a 1 KiB staging piece, a kernel that used the mask of the tile staged before would give
the right sums.

LENGTHS.  A staged kernel runs 256 workgroups over tiles of K = TB / sizeof(T) voxels and
keeps three tiles in LDS; lengths(K) names the lengths where that can go wrong.
"""
import functools

import numpy as np

MAXVEC = 24
BCOEF3 = (-0.75, 0.75, -1.0)
# multiples of 1/8 in [-1, 1]; WCOEF[1] and WCOEF[18] are zero (0 * NaN is still NaN)
WCOEF = tuple((((5 * k + 3) % 17) - 8) / 8.0 for k in range(MAXVEC))
NMAX = 1027 * 2048                  # the longest length of lengths(K): K = 2048
MASK_VALUES = np.array([0, 0, -1, -1, -128, -128, 1, 1, 2, 127], dtype=np.int8)
DECLINED = -2                       # no staged kernel applies: nothing launched
EINVAL = -1
WORKGROUPS = 256                    # of the staged kernels (one per CU)
_CHUNK = 1 << 16
SALT = 16       # of the data hash: the first with which all entries differ pairwise at the
                # fourth_partial lengths (random signs make equal entries likely otherwise)
_M32 = np.uint64(0xFFFFFFFF)


def _mix(x):
    """A 32-bit integer hash (two xor-shift-multiply rounds) of a uint64 array < 2^32."""
    x = ((x ^ (x >> np.uint64(16))) * np.uint64(0x7FEB352D)) & _M32
    x = ((x ^ (x >> np.uint64(15))) * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def lattice_row(k, lo, hi):
    """Row k (0 .. 23: the vectors, 24 .. 26: the base vectors) at voxels lo .. hi - 1:
    int8 in [-31, -1] u [1, 31]."""
    i = np.arange(lo, hi, dtype=np.uint64)
    h = _mix((i * np.uint64(32) + np.uint64(k)) ^ np.uint64(SALT)) % np.uint64(62)
    h = h.astype(np.int16)
    return np.where(h < 31, h - 31, h - 30).astype(np.int8)


def mask_values(lo, hi):
    i = np.arange(lo, hi, dtype=np.uint64)
    return MASK_VALUES[(_mix(i ^ np.uint64(0x9E3779B9)) % np.uint64(10)).astype(np.intp)]


@functools.lru_cache(maxsize=None)
def lattice(nmax=NMAX):
    """(rows int8 [27, nmax], mask int8 [nmax]); a shorter problem is a prefix."""
    rows = np.stack([lattice_row(k, 0, nmax) for k in range(MAXVEC + 3)])
    mask = mask_values(0, nmax)
    rows.setflags(write=False)
    mask.setflags(write=False)
    return rows, mask


def b4_of(base):
    """4 b = -3 base0 + 3 base1 - 4 base2 (an integer array) of int rows [3, m]."""
    base = base.astype(np.int64)
    return -3 * base[0] + 3 * base[1] - 4 * base[2]


def gram_of(rows, keep):
    """(G [nv, nv] int64, 4 W'Z b [nv] int64) of int8 rows [nv + 3, m] (the last three
    the base vectors) over the voxels where keep: float64 BLAS products, exact because
    every partial sum is an integer below 2^53 (the module's docstring)."""
    nv = rows.shape[0] - 3
    a = rows[:nv].astype(np.float64) * keep.astype(np.float64)
    g = a.dot(a.T)
    w = a.dot(b4_of(rows[nv:]).astype(np.float64))
    return np.rint(g).astype(np.int64), np.rint(w).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _cumulative(masked, nmax):
    """Sums of gram_of over whole chunks: entry c covers voxels [0, c * _CHUNK)."""
    rows, mask = lattice(nmax)
    gs = [np.zeros((MAXVEC, MAXVEC), np.int64)]
    bs = [np.zeros(MAXVEC, np.int64)]
    for lo in range(0, nmax - _CHUNK + 1, _CHUNK):
        keep = mask[lo:lo + _CHUNK] <= 0 if masked else np.ones(_CHUNK, bool)
        g, w = gram_of(rows[:, lo:lo + _CHUNK], keep)
        gs.append(gs[-1] + g)
        bs.append(bs[-1] + w)
    return gs, bs


class GramRef(object):
    """gram: int64 [24, 24], the Gram matrix of the 24 vectors over the first n voxels
    (the free ones if masked); the matrix of the first nvec vectors is its leading block.
    wzb: float64 [24], sum vec_k * b over the same voxels (exact dyadics).
    r(nvec): float64 [n], the reduced gradient of the first nvec vectors (exact)."""

    def __init__(self, n, masked, nmax):
        rows, mask = lattice(nmax)
        self.n, self.masked = n, masked
        self.keep = mask[:n] <= 0 if masked else np.ones(n, bool)
        gs, bs = _cumulative(masked, nmax)
        c = n // _CHUNK
        g, w = gram_of(rows[:, c * _CHUNK:n], self.keep[c * _CHUNK:])
        self.gram = gs[c] + g
        self.wzb4 = bs[c] + w
        self.wzb = self.wzb4.astype(np.float64) / 4.0
        self.kept = int(self.keep.sum())
        self._rows = rows
        self._r8 = None

    def pairs(self, nvec):
        """The nvec (nvec + 1) / 2 entries i <= j, row by row (the kernels' order)."""
        return self.gram[:nvec, :nvec][np.triu_indices(nvec)]

    def r(self, nvec):
        # 8 r as int32, extended one vector at a time (the tests ask in rising order)
        if self._r8 is None or self._r8[0] > nvec:
            self._r8 = (0, 2 * b4_of(self._rows[MAXVEC:, :self.n]).astype(np.int32))
        have, acc = self._r8
        for k in range(have, nvec):
            acc = acc + np.int32(round(8 * WCOEF[k])) * self._rows[k, :self.n]
        self._r8 = (nvec, acc)
        return np.where(self.keep, acc.astype(np.float64) / 8.0, 0.0)


@functools.lru_cache(maxsize=8)
def gram_ref(n, masked, nmax=NMAX):
    assert 1 <= n <= nmax
    return GramRef(n, masked, nmax)


# ---- which kernel takes a call, and with what tile -----------------------------------
DEFAULT_KNOBS = {"lb_gram_dma": 1, "lb_gram_mfma": 1}
FORM_KNOBS = {
    "register": {"lb_gram_dma": 0, "lb_gram_mfma": 1},
    "dma": {"lb_gram_dma": 1, "lb_gram_mfma": 0},
    "mfma": {"lb_gram_dma": 1, "lb_gram_mfma": 1},
}
FORM_INDEX = {"register": 0, "dma": 1, "mfma": 2}
_LDS_LIMIT = 160 * 1024
_THREADS2 = 1024                    # of a staged workgroup


def expected_form(knobs, dtype, nvec, n, masked, rg):
    """(form, TB): form 0 (k_masked_gram), 1 (k_masked_gram_dma), 2 (k_masked_gram_mfma)
    with the bytes per vector and tile of the instantiation that runs, or (DECLINED, 0)
    when the entry returns -2 having launched nothing, or (EINVAL, 0).  The rules of
    masked_gram_impl, masked_gram_dma_launch and masked_gram_mfma_dispatch, for aligned
    arrays."""
    size = np.dtype(dtype).itemsize
    vec = 16 // size
    if nvec < 1 or nvec > MAXVEC or n < 1:
        return EINVAL, 0
    staged = n % vec == 0 and (not masked or n % 16 == 0)
    nb = (nvec + 3) // 4
    if knobs.get("lb_gram_dma", 1) and staged:
        if knobs.get("lb_gram_mfma", 1):
            if rg and nb <= 5:
                return 2, {1: 4096, 2: 4096, 3: 2048, 4: 2048, 5: 2048}[nb]
            if not rg:
                return 2, {1: 8192, 2: 4096, 3: 4096, 4: 2048, 5: 2048, 6: 2048}[nb]
        rows = 4 * nb + (3 if rg else 0)
        if rg:
            tb = 8192 if rows <= 6 else (4096 if rows <= 12 else 2048)
        else:
            tb = 8192 if rows <= 4 else (4096 if rows <= 12 else 2048)
        tile = tb // size
        lds = 3 * (rows * (tb + 16) + ((tile + 15) & ~15))
        lds = max(lds, _THREADS2 * 16 * 8)
        if lds <= _LDS_LIMIT:
            return 1, tb
    if rg:
        return DECLINED, 0
    return 0, 4096


def tile_voxels(tb, dtype):
    return tb // np.dtype(dtype).itemsize


LENGTH_CLASSES = ("one_partial", "one_full", "full_and_partial", "second_partial",
                  "third_partial", "fourth_partial", "steady")
RAGGED = (1, 5, 1023, 1025, 4097)   # the register-staged kernel alone takes these


def lengths(k):
    """The lengths of the module's table for tiles of k voxels."""
    w = WORKGROUPS
    return {
        "one_partial": 16,
        "one_full": k,
        "full_and_partial": k + 16,
        # workgroup 0's second tile is partial: the prologue waits for everything
        "second_partial": w * k + 16,
        # its third tile is partial, staged inside the loop
        "third_partial": 2 * w * k + (k // 2 + 15) // 16 * 16,
        # its fourth tile is partial and lands in buffer 0 over a full tile
        "fourth_partial": 3 * w * k + 16,
        # steady state: 5 and 4 tiles per workgroup
        "steady": 4 * w * k + 3 * k,
    }


def unmasked_twin(n, dtype):
    """Without a mask n need only be a multiple of 16 bytes: a 16-voxel group straddles
    the end."""
    return n - 16 + 16 // np.dtype(dtype).itemsize


MODES = {            # name: (rg, masked, r_out given)
    "gram_masked": (False, True, False),
    "gram_all": (False, False, False),
    "rg_r": (True, True, True),
    "rg_no_r": (True, True, False),
    "rg_all": (True, False, True),
}
NVEC_SHORT = (3, 4, 6, 10, 13, 18, 23, 24)     # a value per block count, padded and not
NVEC_ALL = tuple(range(1, MAXVEC + 1))


def plan(form, dtype, length_class):
    """The calls of one (form, dtype, length class): a list of (n, nvec, mode, expected
    (form, TB)), sorted by n then nvec so that one upload serves a run of them.  The
    length of a call follows from the tile of the kernel that takes it; a call no staged
    kernel takes is made at the length of the 2 KiB tile and must be declined."""
    knobs = FORM_KNOBS[form]
    out = set()
    nvecs = NVEC_ALL if length_class == "fourth_partial" else NVEC_SHORT
    for mode, (rg, masked, _) in MODES.items():
        for nvec in nvecs:
            if length_class == "ragged":
                ns = list(RAGGED)
            else:
                # the tile does not depend on n among the lengths the staged kernels take
                f, tb = expected_form(knobs, dtype, nvec, 16, masked, rg)
                n = lengths(tile_voxels(tb if tb else 2048, dtype))[length_class]
                ns = [n] if masked else [n, unmasked_twin(n, dtype)]
            for n in ns:
                out.add((n, nvec, mode) + (expected_form(knobs, dtype, nvec, n, masked, rg),))
    return sorted(out, key=lambda c: (c[0], c[1], c[2]))


def random_gate(terms_abs_sum, kept):
    """|got - fsum(terms)| <= (kept + 2) u sum |terms|, u = 2^-53.  A sum of m = kept
    terms in ANY order of additions errs by at most ((1 + u)^(m-1) - 1) sum |terms|; a
    product that is rounded before it is added (float64 data without FMA) costs one more
    factor (1 + u), an FMA none: (1 + u)^m - 1 <= m u + (m u)^2 in all.  The second-order
    part stays below u for m < 2^26 and fsum rounds once, so m + 2 covers both; the masked
    terms are exact zeros and add nothing."""
    return (kept + 2) * 2.0 ** -53 * terms_abs_sum

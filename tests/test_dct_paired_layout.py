"""CPU: the two LDS exchanges of the paired pass-0 layout (csrc/dct_fused.hip: exchange_pairs_fwd, exchange_pairs_inv),
modelled in numpy with the index formulas read off the source.

Pass 0 of a transform is column-independent, so a thread of the wide row / column kernels carries through it two
neighbouring columns of two polynomials (16-byte global accesses) instead of one column of four.  With TP threads,
h = tid / (TP/2), u = tid % (TP/2), a thread owns, for j = 0, 1, polynomial 2h + j, coefficients r TP + 2u + {0, 1},
r = 0..7.  The exchange next to pass 0 converts between that and the ordinary pass-1 layout g_index<LO1>(tid, r) of four
polynomials per thread, using both LDS buffers at once: polynomial j travels through buffer 0 and polynomial 2 + j
through buffer 1, so threads with h = 0 touch buffer 0 on the paired side and threads with h = 1 buffer 1."""
import os
import re

import numpy as np
import pytest

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fully-homomorphic-image-processing_amd", "csrc", "dct_fused.hip")
LE = 3
SHAPES = [11, 12, 13]


def test_the_index_formulas_in_the_source_are_the_ones_modelled():
    src = open(SRC).read()
    assert "return ((tid >> LO) << (LO + LE)) | (r << LO) | (tid & ((1 << LO) - 1));" in src            # g_index
    assert re.search(r"g_pad\(int j\) \{ return j \+ \(\(j >> \(LO \+ LE\)\) << LO\); \}", src)          # g_pad
    assert "LDS_WORDS = N + (N >> LE)" in src
    assert "int pair_half(int tid) { return __builtin_amdgcn_readfirstlane(tid) / (TP / 2); }" in src      # paired ownership
    assert src.count("const int h = pair_half<TP>(tid), u = tid % (TP / 2);") == 2
    assert "WAVE_LOCAL = (Shape<L, LE>::TP <= 64) || (LO_FROM <= 6 && LO_TO <= 6)" in src


def g_index(lo, tid, r):
    return ((tid >> lo) << (lo + LE)) | (r << lo) | (tid & ((1 << lo) - 1))


def g_pad(lo, j):
    return j + ((j >> (lo + LE)) << lo)


def g_lo(L, p):
    return max(L - LE * p - LE, 0)


class Model:
    """one exchange step j: (buffer, word) touched by every (thread, r, c) on the paired side and by every (thread, r,
    buffer) on the ordinary side, with the (polynomial, coefficient) each access carries"""

    def __init__(self, L):
        self.L, self.N, self.TP = L, 1 << L, (1 << L) >> LE
        self.words = self.N + (self.N >> LE)
        self.lo1, self.lo2 = g_lo(L, 1), g_lo(L, 2)
        tid = np.arange(self.TP)
        self.h, self.u = tid // (self.TP // 2), tid % (self.TP // 2)

    def paired(self, j):
        """arrays [TP, 8, 2]: buffer, word, polynomial, coefficient"""
        r = np.arange(8).reshape(1, 8, 1)
        c = np.arange(2).reshape(1, 1, 2)
        coeff = r * self.TP + 2 * self.u.reshape(-1, 1, 1) + c
        buf = np.broadcast_to(self.h.reshape(-1, 1, 1), coeff.shape)
        return buf, g_pad(self.lo1, coeff), 2 * buf + j, coeff

    def ordinary(self, j):
        """arrays [TP, 8, 2] (last axis: buffer): buffer, word, polynomial, coefficient"""
        tid = np.arange(self.TP).reshape(-1, 1, 1)
        r = np.arange(8).reshape(1, 8, 1)
        coeff = np.broadcast_to(g_index(self.lo1, tid, r), (self.TP, 8, 2))
        buf = np.broadcast_to(np.arange(2).reshape(1, 1, 2), coeff.shape)
        return buf, g_pad(self.lo1, coeff), 2 * buf + j, coeff


@pytest.mark.parametrize("L", SHAPES)
def test_every_word_is_written_by_one_thread_and_read_by_one(L):
    """both directions: the paired side and the ordinary side each touch every used word of both buffers exactly once, and
    the word carries the same (polynomial, coefficient) on either side"""
    m = Model(L)
    used = np.unique(g_pad(m.lo1, np.arange(m.N)))
    assert used.size == m.N and used.max() < m.words
    for j in range(2):
        seen = {}
        for side in (m.paired(j), m.ordinary(j)):
            buf, word, poly, coeff = (a.reshape(-1) for a in side)
            key = buf * m.words + word
            assert np.unique(key).size == key.size == 2 * m.N
            assert np.array_equal(np.unique(key), np.concatenate([used, m.words + used]))
            order = np.argsort(key)
            seen[len(seen)] = (poly[order], coeff[order])
        assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])


@pytest.mark.parametrize("L", SHAPES)
def test_every_16_byte_access_is_aligned(L):
    """LDS: the pair (c = 0, 1) is two neighbouring words starting at an even word of an even-sized buffer.  Global: byte
    offset 16 u + r TP 8 inside a polynomial of N words"""
    m = Model(L)
    assert m.words % 2 == 0
    _, word, _, coeff = m.paired(0)
    assert np.all(word[:, :, 0] % 2 == 0) and np.all(word[:, :, 1] == word[:, :, 0] + 1)
    assert np.all(coeff[:, :, 0] % 2 == 0) and m.N % 2 == 0 and (m.TP * 8) % 16 == 0


@pytest.mark.parametrize("L", SHAPES)
def test_the_thread_to_coefficient_map_covers_each_polynomial_once(L):
    m = Model(L)
    got = {p: [] for p in range(4)}
    for j in range(2):
        _, _, poly, coeff = m.paired(j)
        for p in range(4):
            got[p].append(coeff[poly == p])
    for p in range(4):
        assert np.array_equal(np.sort(np.concatenate(got[p])), np.arange(m.N))


@pytest.mark.parametrize("L", SHAPES)
def test_ordinary_side_stays_inside_the_wave_that_owns_the_word_afterwards(L):
    """The row kernel puts no barrier between the last read of its exchange and the first write of the next one, and the
    column kernel none between the last read of the previous exchange and the first write of its own -- where that
    neighbouring exchange is wave-local (n = 2048, 4096).  That is safe because, on the ordinary side, a wave touches only
    words inside the region that the same wave -- and no other -- uses in the wave-local exchanges: under either padding
    (g_pad<LO1> here, g_pad<LO2> there) wave w stays inside words [w 576, (w + 1) 576).  At n = 8192 the neighbouring
    exchange crosses waves (LO1 = 7), the regions overlap, and the source takes a barrier instead."""
    m = Model(L)
    wave_local = m.TP <= 64 or (m.lo1 <= 6 and m.lo2 <= 6)
    assert wave_local == (L != 13)
    tid = np.arange(m.TP).reshape(-1, 1)
    r = np.arange(8).reshape(1, 8)
    wave = np.broadcast_to(tid >> 6, (m.TP, 8)).reshape(-1)
    here = g_pad(m.lo1, g_index(m.lo1, tid, r)).reshape(-1)                 # ordinary side of the paired exchange
    nxt_from = g_pad(m.lo2, g_index(m.lo1, tid, r)).reshape(-1)             # the neighbouring exchange, either side
    nxt_to = g_pad(m.lo2, g_index(m.lo2, tid, r)).reshape(-1)
    owner = {}
    for words in (nxt_from, nxt_to):
        for w, a in zip(wave, words):
            assert owner.setdefault(int(a), int(w)) == int(w) or not wave_local
    if wave_local:
        lo = {w: min(here[wave == w].min(), nxt_from[wave == w].min(), nxt_to[wave == w].min()) for w in np.unique(wave)}
        hi = {w: max(here[wave == w].max(), nxt_from[wave == w].max(), nxt_to[wave == w].max()) for w in np.unique(wave)}
        for w in np.unique(wave):
            assert lo[w] >= w * 576 and hi[w] < (w + 1) * 576
    else:
        src = open(SRC).read()
        assert src.count("if constexpr (!NEIGHBOUR_WAVE_LOCAL) __syncthreads();") == 2

"""The 32-bit code of a read pointer (csrc/read_ptr.h) restated on numpy arrays: ptr_encode, ptr_decode, ptr_advance,
ptr_advance_long, the tier constants, and ptr_range(hint) -> (lo, span): the store positions lo .. lo + span - 1 at one of which the
occurrence starts.  tests/test_read_pointers_model.py pins every function to what `mc_hosttest pointers` prints from the header."""
import numpy as np

EXACT_END = 1 << 31
SLACK = 16
SLACK_LONG = 32
LONG_WINDOWS = 32
T1_LG, T2_LG, T3_LG = 2, 4, 6
T1_N, T2_N, T3_N = 1 << 30, 1 << 29, (1 << 29) - 2
T1_POS = EXACT_END
T2_POS = T1_POS + (T1_N << T1_LG)
T3_POS = T2_POS + (T2_N << T2_LG)
END = T3_POS + (T3_N << T3_LG)
assert (T2_POS, T3_POS, END) == (6442450944, 15032385536, 49392123776)
# tiers as (first position, end, lg of the granule, reader's span): the exact tier's "granule" is one base
TIERS = [(0, EXACT_END, 0, 1), (T1_POS, T2_POS, T1_LG, (1 << T1_LG) + SLACK), (T2_POS, T3_POS, T2_LG, (1 << T2_LG) + SLACK),
         (T3_POS, END, T3_LG, (1 << T3_LG) + SLACK_LONG)]


def _i64(x):
    return np.atleast_1d(np.asarray(x)).astype(np.int64)


def ptr_encode(pos):
    """codes (int64 array, 0 .. 2^32 - 2) of store positions; 0 past the end"""
    pos = _i64(pos)
    v = np.where(pos < EXACT_END, pos,
                 np.where(pos < T2_POS, EXACT_END + ((pos - T1_POS) >> T1_LG),
                          np.where(pos < T3_POS, EXACT_END + T1_N + ((pos - T2_POS) >> T2_LG),
                                   EXACT_END + T1_N + T2_N + ((pos - T3_POS) >> T3_LG))))
    return np.where(pos < END, v + 1, 0)


def ptr_decode(aux):
    """(lo, span) of codes != 0: the first base of the range the occurrence starts in, the number of candidate offsets"""
    v = _i64(aux) - 1
    w = v - EXACT_END
    lo = np.where(v < EXACT_END, v,
                  np.where(w < T1_N, T1_POS + (w << T1_LG),
                           np.where(w < T1_N + T2_N, T2_POS + ((w - T1_N) << T2_LG), T3_POS + ((w - T1_N - T2_N) << T3_LG))))
    span = np.where(v < EXACT_END, 1, np.where(w < T1_N, TIERS[1][3], np.where(w < T1_N + T2_N, TIERS[2][3], TIERS[3][3])))
    return lo, span


def ptr_range(hint):
    """ptr_decode under the name the tests use; hints must be != 0"""
    assert (_i64(hint) != 0).all()
    return ptr_decode(hint)


def ptr_advance(aux, j):
    """the code of the window j <= 15 bases behind the one aux names (super-k-mer records)"""
    aux, j = np.broadcast_arrays(_i64(aux), _i64(j))
    v = aux - 1
    out = np.where(v + 16 < EXACT_END, aux + j, np.where(v < EXACT_END, ptr_encode(v + j), aux))
    return np.where(aux == 0, 0, out)


def ptr_advance_long(aux, j):
    """... and j <= 31 bases behind (long records)"""
    aux, j = np.broadcast_arrays(_i64(aux), _i64(j))
    lo, _ = ptr_decode(np.maximum(aux, 1))
    out = np.where(aux - 1 + LONG_WINDOWS < EXACT_END, aux + j, ptr_encode(lo + j))
    return np.where(aux == 0, 0, out)


def holds(hint, pos):
    """does the range of every hint (!= 0) hold the position beside it?"""
    lo, span = ptr_range(hint)
    pos = _i64(pos)
    return (lo <= pos) & (pos < lo + span)


def not_found(keys, hints, at, wk, valid, n_bases):
    """Indices of the (key, hint) pairs with a hint whose range holds no store position where a window with that key starts; an
    exact hint's range is one position.  The batch lies at store position `at` and is n_bases long; wk[q] = the key of the window
    at batch position q, valid[q] = that window lies inside one read.  No range may begin at or past the end of the code's range,
    and every range meets the batch."""
    some = np.nonzero(hints != 0)[0]
    lo, span = ptr_range(hints[some])
    assert (lo < END).all() and (lo + span > at).all() and (lo < at + n_bases).all()
    found = np.zeros(len(some), dtype=bool)
    n = len(wk)
    for o in range(int(span.max()) if len(some) else 0):
        q = lo - at + o
        qq = np.clip(q, 0, n - 1)
        found |= (o < span) & (q >= 0) & (q < n) & valid[qq] & (wk[qq] == keys[some])
    return some[~found]

"""Reference of the wraparound alignment for units of up to 256 bases (trew_hip_monomers).  Independent of the library and of
oracle/.  The definition is align_ref.py's, word for word, with 3 <= k <= 256; only strand_codes there asserts k <= 32, so
the codes of a strand are made here.

Two forms that must agree: monomer_read (align_ref.align_strand, the definition in plain Python tuples, O(n k^2)) and
monomers (the maximum over d deleted unit bases in the linear-plus-wrap form, vectorised over the phases and over many reads
with numpy, O(n k) with O(n log k) numpy steps):

  L[j] = max over j' <= j of V[j'] shifted by j - j'     the prefix closure without the wrap, doubling steps 1, 2, 4, ... < k
  W    = L[k-1]
  H[j] = max(L[j], W shifted by j + 1)

Shifting by d (score - P d, consumed + d) is monotone in the tuple order, a source j' <= j reached through W has gone a
whole turn further than its direct path (P k lower: it loses strictly), a source j' > j is reached through W with exactly
d = j + k - j'.  A candidate whose score is negative is dropped (it loses to the fresh start)."""
import numpy as np

import align_ref as A

FIELDS, DTYPE, COLUMNS, codes, columns, cli_lines = A.FIELDS, A.DTYPE, A.COLUMNS, A.codes, A.columns, A.cli_lines
MAX = 256


def strand_codes(unit, strand):
    c = codes(unit)
    assert 3 <= len(c) <= MAX and max(c) < 4
    return [3 - x for x in reversed(c)] if strand else c


def monomer_read(read, unit, penalty=3, strands=(0, 1)):
    """the fields of one (read, unit) from the definition; strands: those computed (the others are left out)"""
    x = codes(read)
    out = ()
    for s in strands:
        out += A.align_strand(x, strand_codes(unit, s), penalty)
    return out


def _strand_many(X, lens, t, P):
    """X: (R, n_max) codes, lens: (R,), t: target codes -> (R, 5) int64 records; the keys are align_ref._strand_many's"""
    R, n_max = X.shape
    k = len(t)
    t = np.asarray(t, dtype=np.int64)[None, :]
    A_ = np.zeros((R, k), dtype=np.int64)
    B_ = np.zeros((R, k), dtype=np.int64)
    b_score = np.zeros((R, k), dtype=np.int64)
    b_end = np.zeros((R, k), dtype=np.int64)
    b_A = np.zeros((R, k), dtype=np.int64)
    b_B = np.zeros((R, k), dtype=np.int64)
    one, pen = np.int64(1) << 32, np.int64(P) << 32
    wrap_d = np.arange(1, k + 1, dtype=np.int64)[None, :]  # phase j takes W shifted by j + 1
    better = A._better
    for i in range(1, n_max + 1):
        live = (lens >= i)[:, None]
        c = X[:, i - 1][:, None]
        hit = c == t
        dA, dB = np.roll(A_, 1, axis=1), np.roll(B_, 1, axis=1)
        dA = np.where(hit, dA + one, dA - pen)
        dB = np.where(hit, dB + one + 1, dB + one)
        VA = np.full((R, k), i, dtype=np.int64)
        VB = np.zeros((R, k), dtype=np.int64)
        for cA, cB in ((dA, dB), (A_ - pen, B_)):
            take = (cA >= 0) & better((cA, cB), (VA, VB))
            VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
        s = 1
        while s < k:  # the prefix closure: no wrap, a phase below s has no source
            cA = np.full((R, k), -1, dtype=np.int64)
            cB = np.zeros((R, k), dtype=np.int64)
            cA[:, s:] = VA[:, :-s] - np.int64(P * s) * one
            cB[:, s:] = VB[:, :-s] + np.int64(s) * one
            take = (cA >= 0) & better((cA, cB), (VA, VB))
            VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
            s *= 2
        cA = VA[:, -1:] - (np.int64(P) * wrap_d) * one
        cB = VB[:, -1:] + wrap_d * one
        take = (cA >= 0) & better((cA, cB), (VA, VB))
        VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
        A_, B_ = np.where(live, VA, A_), np.where(live, VB, B_)
        # the best cell of a phase: a strictly larger score, or within the row (an equal end) the larger tuple
        up = live & ((VA >> 32) > b_score)
        b_score = np.where(up, VA >> 32, b_score)
        b_end = np.where(up, i, b_end)
        b_A, b_B = np.where(up, VA, b_A), np.where(up, VB, b_B)
    out = np.zeros((R, 5), dtype=np.int64)
    for r in range(R):
        key = max((int(b_score[r, j]), -int(b_end[r, j]), int(b_A[r, j]) & 0xFFFFFFFF, int(b_B[r, j]) >> 32, int(b_B[r, j]) & 0xFFFFFFFF)
                  for j in range(k))
        if key[0] > 0:
            out[r] = (key[0], key[2], -key[1], key[3], key[4])
    return out


def monomers(reads, units, penalty=3):
    """DTYPE records of shape (n_reads, n_units), the O(n k) form"""
    out = np.zeros((len(reads), len(units)), dtype=DTYPE)
    if not len(reads):
        return out
    cs = [codes(r) for r in reads]
    lens = np.array([len(c) for c in cs], dtype=np.int64)
    X = np.full((len(cs), max(int(lens.max()), 1)), 4, dtype=np.int64)
    for r, c in enumerate(cs):
        X[r, :len(c)] = c
    for m, unit in enumerate(units):
        for s, sfx in enumerate(("_fwd", "_rev")):
            rec = _strand_many(X, lens, strand_codes(unit, s), penalty)
            for f, name in enumerate(("score", "start", "end", "consumed", "matches")):
                out[name + sfx][:, m] = rec[:, f]
    return out

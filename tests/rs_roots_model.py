"""The equivalence that checks RS decoding with roots alpha^(mu + i step), in numpy.

With s' = step^-1 mod nf and m = mu s' mod nf (nf = 2^q - 1), the map

    T:  w''[step p mod nf] = w[p] alpha^((step p mod nf) (m - 1))

carries the (mu, step) code onto the (1, 1) code of the same q and t: sum_p w[p] alpha^((mu + i step) p) =
sum_j w''[j] alpha^((1 + i) j) with j = step p.  T permutes the positions and scales every symbol by a non-zero constant, so
it keeps Hamming distances and erasure sets, and correct_{mu,step}(w) = T^-1(correct_{1,1}(T(w))) frame for frame -- nerr,
the status class and miscorrections beyond the capability included.  For step = 1 positions stay where they are, so the
same holds for a shortened code once the word is padded to nf symbols.

Symbols are uint8 (q <= 8) or uint16 (q > 8); the field comes as its antilog / log tables (exp[i] = alpha^i for
i < nf at least, log[v] for v != 0).
"""
import numpy as np


def field_tables(q, poly):
    """(exp, log) of GF(2^q) = GF(2)[x] / poly, alpha = x; exp has 2 nf entries."""
    nf = (1 << q) - 1
    exp = np.zeros(2 * nf, np.uint32)
    log = np.zeros(nf + 1, np.uint32)
    v = 1
    for i in range(nf):
        exp[i] = exp[i + nf] = v
        log[v] = i
        v <<= 1
        if v >> q:
            v ^= poly
    assert v == 1, "polynomial is not primitive"
    return exp, log


def _scale(w, e, exp, log, nf):
    """w[..., j] * alpha^e[j]"""
    w = np.asarray(w)
    lw = np.asarray(log, np.int64)[w.astype(np.int64)]
    r = np.asarray(exp, np.int64)[(lw + e) % nf]
    return np.where(w != 0, r, 0).astype(w.dtype)


def _maps(nf, mu, step):
    m = (mu * pow(step, -1, nf)) % nf
    p = np.arange(nf)
    j = (step * p) % nf
    return p, j, (j * (m - 1)) % nf


def position(p, nf, step):
    """where T sends position p (erasure lists go through this)"""
    return (step * int(p)) % nf


def T(w, exp, log, nf, mu, step):
    """(B, n) words of the (mu, step) code, n <= nf -> (B, nf) words of the (1, 1) code (n < nf: step = 1, zero padded)"""
    w = np.atleast_2d(np.asarray(w))
    n = w.shape[1]
    assert n == nf or step == 1
    full = np.zeros((w.shape[0], nf), w.dtype)
    full[:, :n] = w
    p, j, e = _maps(nf, mu, step)
    out = np.zeros_like(full)
    out[:, j] = _scale(full[:, p], e, exp, log, nf)
    return out


def T_inv(w2, exp, log, nf, mu, step, n=None):
    """the inverse of T; n < nf cuts the word back to the shortened length"""
    w2 = np.atleast_2d(np.asarray(w2))
    p, j, e = _maps(nf, mu, step)
    out = np.zeros_like(w2)
    out[:, p] = _scale(w2[:, j], (nf - e) % nf, exp, log, nf)
    return out if n is None else out[:, :n]


# (q, t, mu, step) of the parity tests: first root alpha^0 at two capabilities of GF(2^8) (DVB / ATSC style), a first
# root beyond alpha^1, a small field, a step other than 1 in a small and in the byte field
SETS = ((8, 8, 0, 1), (8, 16, 0, 1), (8, 4, 2, 1), (4, 3, 0, 1), (4, 2, 3, 2), (8, 3, 7, 7))


def make_frames(rng, cw, t, q, with_erasures):
    """Received words for the parity tests: 0 .. t + 3 random symbol errors per frame; with_erasures: mixes of rho
    erasures and e errors up to and one past 2 e + rho = 2 t.  Returns rx, the per-frame erasure lists (or None) and
    within = "2 e + rho <= 2 t" per frame."""
    B, n = cw.shape
    rx = cw.copy()
    per, within = [], np.zeros(B, bool)
    for f in range(B):
        if with_erasures:
            rho = int(rng.integers(0, min(2 * t, n) + 1))
            room = (2 * t - rho) // 2
            e = int(rng.integers(0, room + 1)) if f % 4 else room + 1  # every fourth frame: one error too many
            e = min(e, n - rho)
        else:
            rho, e = 0, int(rng.integers(0, t + 4))
            e = min(e, n)
        pos = rng.choice(n, rho + e, replace=False)
        for p in pos[:rho]:  # an erased symbol carries anything
            rx[f, p] = int(rng.integers(0, 1 << q))
        for p in pos[rho:]:
            rx[f, p] ^= int(rng.integers(1, 1 << q))
        per.append(sorted(int(p) for p in pos[:rho]))
        within[f] = 2 * e + rho <= 2 * t
    return rx, (per if with_erasures else None), within

"""What the contracts of the reliability-based decoders share (cc_correct_chase_batch, cc_correct_gmd_batch; DESIGN 4.11,
4.12): the key of a position is bits(v_i) & 0x7fffffff of its channel value or reliability, ties go to the lower
position; the metric of a candidate is the float32 sum, in ascending position, of |v_i| where it differs from the
received word; the smallest metric wins, equal metrics go to the first candidate.  chase_model and gmd_model say what
the candidates are.
"""
import numpy as np

FRAME_OK, FRAME_LOCATOR = 0, 2


def least_reliable(v, count):
    """(B, min(count, n)) positions in the order of the contract"""
    keys = np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.argsort(keys, axis=1, kind="stable")[:, : min(count, keys.shape[1])]


def metric(v, z, c):
    """float32 sum of |v_i| over c_i != z_i, from +0.0 in ascending i; rows of 2-d inputs"""
    terms = np.where(np.asarray(c) != np.asarray(z), np.abs(np.asarray(v, np.float32)), np.float32(0.0)).astype(np.float32)
    acc = np.zeros(terms.shape[:-1], np.float32)
    with np.errstate(over="ignore"):  # (batches near FLT_MAX overflow to inf, as the device's sum does)
        for i in range(terms.shape[-1]):  # one float32 add per position (adding +0.0 changes nothing)
            acc = (acc + terms[..., i]).astype(np.float32)
    return acc


def pick(cand, count, key):
    """the contract's outputs over the first `count` candidates of every frame, cand[key] being the received words:
    out (B, n) u8, nerr (B,) i32, status (B,) i32, metric (B,) f32, winner (B,) (-1: none)"""
    ok, M, z = cand["ok"][:, :count], cand["M"][:, :count], cand[key]
    B = z.shape[0]
    out, nerr = z.copy(), np.full(B, -1, np.int32)
    status, met = np.full(B, FRAME_LOCATOR, np.int32), np.zeros(B, np.float32)
    winner = np.full(B, -1, np.int64)
    for f in range(B):
        js = np.flatnonzero(ok[f])
        if js.size == 0:
            continue
        j = js[np.argmin(M[f, js])]  # argmin returns the first minimum: equal M goes to the smallest index
        winner[f], out[f], met[f], status[f] = j, cand["words"][f, j], M[f, j], FRAME_OK
        nerr[f] = int((out[f] != z[f]).sum())
    return dict(out=out, nerr=nerr, status=status, metric=met, winner=winner)

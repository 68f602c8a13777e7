"""The contract of the Chase-Pyndiah soft output (cc_correct_chase_soft_batch) on top of chase_model: with D
the winner of `pick`, M_D its metric and s_i = +1 where D_i = 0, else -1, the competitor metric of position i is
K_i = min M(c_j) over the patterns j < 2^p that have a candidate with (c_j)_i != D_i, and
    ext_i = s_i (K_i - M_D) - y_i   where there is such a pattern (two float32 subtractions),
    ext_i = s_i beta                where there is none,
    ext_i = +0.0                    at every i of a frame in which no pattern has a candidate.
`product_decode` is channelcoding_amd.product_decode with this model as the component decoder.
"""
import numpy as np

import chase_model as M


def soft(cand, p, beta):
    """pick(cand, p) plus ext (B, n) f32 and has (B, n) bool: the positions with a competitor"""
    res = M.pick(cand, p)
    J, y, beta = 1 << p, cand["y"], np.float32(beta)
    B, n = y.shape
    ext, has = np.zeros((B, n), np.float32), np.zeros((B, n), bool)
    for f in np.flatnonzero(res["winner"] >= 0):
        js = np.flatnonzero(cand["ok"][f, :J])
        differs = cand["words"][f, js] != res["out"][f][None, :]  # (candidates, n)
        has[f] = differs.any(axis=0)
        K = np.where(differs, cand["M"][f, js][:, None], np.float32(np.inf)).min(axis=0).astype(np.float32)
        s = np.where(res["out"][f] == 0, np.float32(1.0), np.float32(-1.0))
        with np.errstate(invalid="ignore", over="ignore"):
            gap = (K - res["metric"][f]).astype(np.float32)
            ext[f] = np.where(has[f], (s * gap).astype(np.float32) - y[f], s * beta).astype(np.float32)
    return dict(res, ext=ext, has=has)


def chase_soft(dec, y, p, beta):
    return soft(M.candidates(dec, y, max(p, 0)), min(p, dec.n), beta)


def product_decode(rows, cols, y, p, alpha, beta, decode=chase_soft):
    """the loop of channelcoding_amd.product_decode over model decoders `rows` and `cols`; the list of
    dict(out=, ext=, status=) after every half-iteration, in the orientation of y"""
    y = np.ascontiguousarray(y, np.float32)
    B, n2, n1 = y.shape
    W, steps = np.zeros_like(y), []
    for h, (a, b) in enumerate(zip(alpha, beta)):
        X = y + (W * np.float32(a)).astype(np.float32)
        if h % 2 == 0:
            r = decode(rows, X.reshape(B * n2, n1), p, b)
            out, W, status = r["out"].reshape(B, n2, n1), r["ext"].reshape(B, n2, n1), r["status"].reshape(B, n2)
        else:
            r = decode(cols, np.ascontiguousarray(X.transpose(0, 2, 1)).reshape(B * n1, n2), p, b)
            out = np.ascontiguousarray(r["out"].reshape(B, n1, n2).transpose(0, 2, 1))
            W = np.ascontiguousarray(r["ext"].reshape(B, n1, n2).transpose(0, 2, 1))
            status = r["status"].reshape(B, n1)
        steps.append(dict(out=out, ext=W, status=status))
    return steps

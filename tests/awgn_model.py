"""A float64 restatement of the device AWGN channel (mc.hip: the Philox counter layout and box_muller).

Symbol j of global frame gf takes Philox4x32-10 counter (gf_lo, gf_hi, j >> 2, 0) under key (seed_lo, seed_hi); words
(0, 1) give the Box-Muller pair of symbols 4q and 4q + 1, words (2, 3) the pair of 4q + 2 and 4q + 3:
u1 = ((a >> 8) + 1) / 2^24 in (0, 1], u2 = (b >> 8) / 2^24 in [0, 1), z0 = sqrt(-2 ln u1) cos(2 pi u2),
z1 = sqrt(-2 ln u1) sin(2 pi u2), and y = (1 - 2c) + sigma z with sigma the float32 value the launcher passes.
The device evaluates log, sqrt, cos and sin with the hardware approximations; this model does not."""
import numpy as np

from test_discrete_host import MASK, philox4x32_10

Z_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -24)))  # the largest |z| the 24-bit u1 can give


def box_muller(a, b):
    """the float64 pair of two Philox words (uint64 arrays < 2^32)"""
    u1 = ((np.asarray(a, np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) / 2.0 ** 24
    u2 = (np.asarray(b, np.uint64) >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def awgn_normals(code_n, seed, first, frames):
    """z of frames [first, first + frames): (frames, code_n) float64"""
    quads = (code_n + 3) // 4
    gf = np.uint64(first) + np.arange(frames, dtype=np.uint64)[:, None]
    qd = np.arange(quads, dtype=np.uint64)[None, :]
    w0, w1, w2, w3 = philox4x32_10(gf & MASK, gf >> np.uint64(32), qd, 0, seed & 0xFFFFFFFF, seed >> 32)
    z = np.empty((frames, quads, 4), np.float64)
    z[:, :, 0], z[:, :, 1] = box_muller(w0, w1)
    z[:, :, 2], z[:, :, 3] = box_muller(w2, w3)
    return z.reshape(frames, 4 * quads)[:, :code_n]


def awgn_reference(code_n, sigma_f32, seed, first, frames, sent=None):
    """y = (1 - 2c) + sigma z in float64 for the words `sent` ((frames, code_n) bits; None: the all-zero word)"""
    z = awgn_normals(code_n, seed, first, frames)
    x = np.ones_like(z) if sent is None else 1.0 - 2.0 * np.asarray(sent, np.float64)
    return x + float(np.float32(sigma_f32)) * z

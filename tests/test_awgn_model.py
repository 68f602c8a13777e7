"""CPU tests of the float64 AWGN model (tests/awgn_model.py) that tests/test_gpu_mc.py holds the device channel to."""
import numpy as np

from awgn_model import Z_MAX, awgn_normals, awgn_reference, box_muller
from test_discrete_host import MASK, philox4x32_10, symbol_words


def test_counter_layout_matches_the_discrete_conventions():
    """Same frame and key handling as symbol_words / bch_message_bits: word (j & 3) of counter (gf, j >> 2, 0), the
    pair (words 0, 1) for symbols 4q, 4q + 1 and (2, 3) for 4q + 2, 4q + 3.  The frames cross 2^32, the seed is
    >= 2^32."""
    seed, first, frames, n = (5 << 32) + 0x1234, (1 << 32) - 3, 7, 31
    z = awgn_normals(n, seed, first, frames)
    assert z.shape == (frames, n)
    w = symbol_words(seed, first, frames, 32, 0)
    za, zb = box_muller(w[:, 0::2], w[:, 1::2])  # pairs (0, 1), (2, 3), ...
    full = np.empty((frames, 32))
    full[:, 0::2], full[:, 1::2] = za, zb
    assert np.array_equal(z, full[:, :n])
    # frame 2^32 is counter (0, 1, q, 0); the low key word is seed & (2^32 - 1), the high one seed >> 32
    w0, w1, w2, w3 = (int(x[()]) for x in philox4x32_10(0, 1, 7, 0, 0x1234, 5))
    a0, a1 = box_muller(w0, w1)
    a2, a3 = box_muller(w2, w3)
    assert np.array_equal(z[3, 28:31], [a0, a1, a2])
    # the seed's high word matters, the frame's high word too
    assert not np.array_equal(awgn_normals(n, seed & int(MASK), first, frames), z)
    assert not np.array_equal(awgn_normals(n, seed, first + (1 << 32), frames), z)
    # sharding: the noise of a frame depends on (seed, global frame) only, not on the call or on n beyond the quad
    assert np.array_equal(awgn_normals(n, seed, first + 2, 5), z[2:])
    assert np.array_equal(awgn_normals(28, seed, first, frames), z[:, :28])


def test_box_muller_mapping():
    assert box_muller(0, 0) == (np.sqrt(-2.0 * np.log(2.0 ** -24)), 0.0)  # u1 = 2^-24, u2 = 0
    z0, z1 = box_muller(0xFFFFFFFF, 0xFFFFFFFF)  # u1 = 1: r = 0
    assert z0 == 0.0 and z1 == 0.0
    z0, z1 = box_muller(0x7FFFFFFF, 0x40000000)  # u1 = 1/2, u2 = 1/4: a quarter turn
    r = np.sqrt(2.0 * np.log(2.0))
    assert abs(z0) < 1e-15 and abs(z1 - r) < 1e-15
    # the low 8 bits of both words do not enter
    assert box_muller(0x12345678, 0x9ABCDEF0) == box_muller(0x123456FF, 0x9ABCDE00)


def test_reference_is_bpsk_plus_scaled_noise():
    sent = np.random.default_rng(1).integers(0, 2, (40, 15)).astype(np.uint8)
    sigma = 0.6123456789
    y = awgn_reference(15, sigma, 9, 77, 40, sent)
    z = awgn_normals(15, 9, 77, 40)
    assert np.array_equal(y, (1.0 - 2.0 * sent) + float(np.float32(sigma)) * z)
    assert np.array_equal(awgn_reference(15, sigma, 9, 77, 40), 1.0 + float(np.float32(sigma)) * z)


def test_noise_moments_and_independence():
    z = awgn_normals(256, 0xDEADBEEF12, 1 << 40, 4096)  # 2^20 symbols
    N = z.size
    assert abs(z.mean()) < 5 / np.sqrt(N)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / N)
    assert abs((z ** 3).mean()) < 5 * np.sqrt(15.0 / N) and abs((z ** 4).mean() - 3.0) < 5 * np.sqrt(96.0 / N)

    def corr(a, b):
        a, b = a.ravel(), b.ravel()
        return float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std())), a.size

    q = z.reshape(z.shape[0], -1, 4)
    for a, b in ((q[:, :, 0], q[:, :, 1]),      # the two values of one pair
                 (q[:, :, 2], q[:, :, 3]),
                 (q[:, :, 1], q[:, :, 2]),      # the two pairs of one quad
                 (q[:, :-1, 3], q[:, 1:, 0]),   # neighbouring quads
                 (q[:, :-1, 0], q[:, 1:, 0]),
                 (q[:-1], q[1:])):              # neighbouring frames
        c, m = corr(a, b)
        assert abs(c) < 6 / np.sqrt(m), c
    # the two values of a pair are independent, not merely uncorrelated: E[z0^2 z1^2] = E[z0^2] E[z1^2] = 1
    assert abs(float((q[:, :, 0] ** 2 * q[:, :, 1] ** 2).mean()) - 1.0) < 0.03


def test_noise_is_bounded():
    z = awgn_normals(255, 3, 0, 4096)
    assert np.abs(z).max() <= Z_MAX
    assert abs(Z_MAX - np.sqrt(48.0 * np.log(2.0))) < 1e-14
    assert 5.76 < Z_MAX < 5.77

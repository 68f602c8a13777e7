"""Host-side mirror of the reference's code classes on top of the C ABI.

Names and argument meaning follow the reference (file:line relative to its repo):

* ``errors`` / ``dmin``                     src/codes/codes.h:7-26
* algorithm tags                             src/codes/hard_decision.h:15-24, src/codes/soft_decision.h:20-73
* ``primitive_bch`` / ``rs``                 src/codes/bch.h:16-19, src/codes/rs.h:6-10
* ``encode`` / ``decode`` / ``correct``      src/codes/cyclic.h:289-344
* ``H`` / ``to_string`` / ``rate`` / ``n`` / ``t``   src/codes/cyclic.h:94-95,:111,:282-287,:346-359
* ``decoding_failure``                       src/codes/codes.h:28-36

Input-sequence convention (cyclic.h:163-184, :220-222): a *signed* element type
(float / signed-int numpy arrays or torch tensors) is a soft value, bit = (x < 0);
an *unsigned* one (uint8 / bool arrays, or plain lists of non-negative ints) holds
symbols.  All decoding runs on the GPU through libchannelcoding_amd.so; there is
no CPU path here.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _capi as capi
from ._capi import CcError


class decoding_failure(RuntimeError):
    """codes.h:28-36"""


class errors:  # codes.h:7-9
    def __init__(self, e):
        self.value = int(e)
        self.t = int(e)


class dmin:  # codes.h:11-13, correction_capability :19-21
    def __init__(self, d):
        self.value = int(d)
        self.t = (int(d) - 1) // 2


def _ratio(r):
    if isinstance(r, Fraction):
        return r.numerator, r.denominator
    if isinstance(r, (tuple, list)):
        return int(r[0]), int(r[1])
    f = Fraction(r).limit_denominator(1 << 20)
    return f.numerator, f.denominator


class _tag:
    soft = False
    iterations = 0
    alpha = 1.0
    beta = 0.0


class peterson_gorenstein_zierler_tag(_tag):
    alg = capi.ALG_PGZ


class berlekamp_massey_tag(_tag):
    alg = capi.ALG_BM


class euklid_tag(_tag):
    alg = capi.ALG_EUKLID


class min_sum_tag(_tag):  # soft_decision.h:20-23
    alg, soft = capi.ALG_MS, True

    def __init__(self, iterations=50):
        self.iterations = int(iterations)


class normalized_min_sum_tag(_tag):  # :36-42  alpha = num/den
    alg, soft = capi.ALG_NMS, True

    def __init__(self, iterations, ratio=(1, 1)):
        num, den = _ratio(ratio)
        self.iterations, self.alpha = int(iterations), num / den


class offset_min_sum_tag(_tag):  # :44-50  beta = num/den
    alg, soft = capi.ALG_OMS, True

    def __init__(self, iterations=50, ratio=(0, 1)):
        num, den = _ratio(ratio)
        self.iterations, self.beta = int(iterations), num / den


class self_correcting_1_min_sum_tag(_tag):  # :52-56
    alg, soft = capi.ALG_SCMS1, True

    def __init__(self, iterations=50):
        self.iterations = int(iterations)


class self_correcting_2_min_sum_tag(_tag):  # :58-62
    alg, soft = capi.ALG_SCMS2, True

    def __init__(self, iterations=50):
        self.iterations = int(iterations)


class normalized_2d_min_sum_tag(_tag):  # :64-73
    alg, soft = capi.ALG_2DNMS, True

    def __init__(self, iterations=50, alpha=(1, 1), beta=(1, 10)):
        an, ad = _ratio(alpha)
        bn, _bd = _ratio(beta)
        self.iterations = int(iterations)
        self.alpha = an / ad
        # soft_decision.h:71 divides Beta::num by Alpha::den (sic): the defaults give alpha = beta = 1
        self.beta = bn / ad


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ptr(a):
    if a is None:
        return None
    if _is_torch(a):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _stream_handle(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _erasure_csr(erasures, B, n):
    """None | flat list (one frame, or shared by every frame) | list of per-frame lists -> (values, offsets)."""
    if erasures is None:
        return None, None
    erasures = list(erasures)
    if len(erasures) and isinstance(erasures[0], (list, tuple, np.ndarray)):
        per = [list(map(int, e)) for e in erasures]
        if len(per) != B:
            raise ValueError("need one erasure list per frame")
    else:
        if not len(erasures):
            return None, None
        per = [list(map(int, erasures))] * B
    off = np.zeros(B + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in per])
    vals = np.array([e for p in per for e in p], np.uint16)
    if len(vals) and (vals >= n).any():
        raise IndexError("erasure position out of range")  # copy.at(erasure), cyclic.h:261
    return vals, off


def _torch_symbol_dtypes(cache=[]):
    if not cache:
        import torch
        cache.append((torch.uint8, torch.int16) + ((torch.uint16,) if hasattr(torch, "uint16") else ()))
    return cache[0]


_TORCH_DTYPE = {}


def _torch_dtype(dtype):
    """the tensor type of an output of numpy type `dtype`; uint16 (iters) is int16 on the device"""
    if not _TORCH_DTYPE:
        import torch
        _TORCH_DTYPE.update({np.uint8: torch.uint8, np.uint16: torch.int16, np.int32: torch.int32,
                             np.float32: torch.float32})
    return _TORCH_DTYPE[dtype]


class _host:
    """A batch call on numpy arrays: the C call as it is named, outputs zeroed, the erasure list of _erasure_csr."""
    dev = ""
    in_place_needs = {True: "uint8 array", False: "array of the code's symbol type"}  # by packed=
    out_must_be = {True: "writable uint8 array of shape (B, packed_bytes)",
                   False: "writable array of the input's shape and the code's symbol type"}
    asarray = staticmethod(np.asarray)
    symbols = staticmethod(lambda x, dtype, itemsize, any16: np.ascontiguousarray(x, dtype))

    @staticmethod
    def size(x):
        return x.size

    @staticmethod
    def alloc(like, shape, dtype):
        return np.zeros(shape, dtype or like.dtype)

    @staticmethod
    def erasure_list(like, vals, off):
        return vals, off

    @staticmethod
    def stream(like):
        return ()

    @staticmethod
    def is_symbols(x):
        return isinstance(x, np.ndarray) and x.dtype.kind not in "fi"

    @staticmethod
    def is_contiguous(x, dtype):
        return isinstance(x, np.ndarray) and x.dtype == dtype and x.flags.c_contiguous

    @staticmethod
    def is_buffer(a, like, shape):
        return (isinstance(a, np.ndarray) and a.dtype == like.dtype and a.flags.c_contiguous and a.flags.writeable
                and a.shape == shape)

    @staticmethod
    def as_type(x, kind, dtype):
        x = np.asarray(x)
        return np.ascontiguousarray(x, dtype) if x.dtype.kind == kind else None

    @staticmethod
    def channel_input(b, soft_alg):
        """-> (which cc_correct_*_batch, its input): a signed element type holds soft values, an unsigned one symbols"""
        signed = b.dtype.kind in "fi"
        if soft_alg and not signed:
            raise TypeError("min-sum needs a signed (soft) input sequence")
        if signed:
            return "soft" if soft_alg else "hard_f32", np.ascontiguousarray(b, np.float32)
        return "hard", np.ascontiguousarray(b, np.uint8)


class _device:
    """A batch call on torch tensors: the _dev call on the current stream, outputs on the input's device."""
    dev = "_dev"
    in_place_needs = {True: "tensor", False: "tensor"}
    out_must_be = {True: "uint8 tensor of shape (B, packed_bytes) on the input's device",
                   False: "tensor of the input's shape, dtype and device"}
    asarray = staticmethod(lambda x: x)
    is_symbols = staticmethod(lambda x: True)  # (symbols() decides)

    @staticmethod
    def size(x):
        return x.numel()

    @staticmethod
    def alloc(like, shape, dtype):
        return like.new_empty(shape, dtype=_torch_dtype(dtype)) if dtype else like.new_empty(shape)

    @staticmethod
    def erasure_list(like, vals, off):
        import torch
        if vals.size == 0:  # an empty tensor has a null data pointer: keep the list addressable
            vals = np.zeros(1, vals.dtype)
        return (torch.from_numpy(vals.astype(np.int16)).to(like.device),
                torch.from_numpy(off.astype(np.int32)).to(like.device))

    @staticmethod
    def stream(like):
        return (_stream_handle(like),)

    @staticmethod
    def is_contiguous(x, dtype):
        return x.is_contiguous()

    @staticmethod
    def is_buffer(a, like, shape):
        return (_is_torch(a) and a.dtype == like.dtype and a.device == like.device and a.is_contiguous()
                and tuple(a.shape) == shape)

    @staticmethod
    def symbols(x, dtype, itemsize, any16):
        """x contiguous, or None where it does not hold symbols of dtype's width (any16: any 2-byte type does)"""
        x = x.contiguous()
        return x if x.element_size() == itemsize and (any16 or x.dtype in _torch_symbol_dtypes()) else None

    @staticmethod
    def as_type(x, kind, dtype):
        return x.contiguous() if x.dtype == _torch_dtype(dtype) else None

    @staticmethod
    def channel_input(b, soft_alg):
        import torch
        if soft_alg:
            if b.dtype != torch.float32:
                raise TypeError("min-sum needs float32 LLRs")
            return "soft", b.contiguous()
        if b.dtype == torch.float32:
            return "hard_f32", b.contiguous()
        if b.dtype == torch.uint8:
            return "hard", b.contiguous()
        raise TypeError("hard decoding takes uint8 symbols or float32 soft values")


def _side(x):
    return _device if _is_torch(x) else _host


_PER_FRAME = {"nerr": np.int32, "status": np.int32, "iters": np.uint16, "metric": np.float32}  # (iters: int16 in torch)
_KEYS = ("out", "msg", "status", "nerr", "iters", "metric", "L", "ext")  # the order of a result dict


def symbol_reliability(y, q):
    """(B, n q) BPSK channel values (numpy array or torch tensor) -> (w, rel) for correct_batch(w, gmd=, reliability=rel):
    bit b of symbol i is value i q + b, w_i = sum_b (y < 0) << b, and rel_i is the |y| with the smallest key
    bits(y) & 0x7fffffff among the symbol's q bits (the rule of cc_awgn_symbols_dev)."""
    q = int(q)
    if not 1 <= q <= 8:
        raise ValueError("symbol_reliability serves q = 1 .. 8")
    if y.shape[-1] % q:
        raise CcError(capi.ERR_LENGTH, "symbol_reliability")
    if _is_torch(y):
        import torch
        v = y.to(torch.float32).reshape(-1, y.shape[-1] // q, q)
        weights = (1 << torch.arange(q, device=v.device, dtype=torch.int32))
        w = ((v < 0).to(torch.int32) * weights).sum(dim=2).to(torch.uint8)
        keys = v.contiguous().view(torch.int32) & 0x7FFFFFFF  # non-negative: signed order = unsigned order
        return w, keys.min(dim=2).values.view(torch.float32)
    v = np.ascontiguousarray(y, np.float32).reshape(-1, y.shape[-1] // q, q)
    w = ((v < 0).astype(np.uint32) << np.arange(q, dtype=np.uint32)).sum(axis=2).astype(np.uint8)
    keys = v.view(np.uint32) & np.uint32(0x7FFFFFFF)
    return w, np.ascontiguousarray(keys.min(axis=2)).view(np.float32)


def extend(words):
    """(..., n) words of 0/1 symbols -> (..., n + 1): the overall parity bit w_0 ^ .. ^ w_(n-1) appended, which makes a
    codeword of a binary BCH code one of its extended code (correct_batch(chase=p, extended=True)).  numpy array or torch
    tensor, any integer type; the result has the type of the input."""
    if _is_torch(words):
        import torch
        parity = (words.to(torch.int64).sum(dim=-1, keepdim=True) & 1).to(words.dtype)
        return torch.cat([words, parity], dim=-1)
    words = np.asarray(words)
    parity = (words.astype(np.int64).sum(axis=-1, keepdims=True) & 1).astype(words.dtype)
    return np.concatenate([words, parity], axis=-1)


def unextend(words):
    """(..., n + 1) extended words -> (..., n): the parity column dropped (a contiguous copy)."""
    if words.shape[-1] < 1:
        raise CcError(capi.ERR_LENGTH, "unextend")
    inner = words[..., :-1]
    return inner.contiguous() if _is_torch(words) else np.ascontiguousarray(inner)


def _product_loop(rows, cols, y, p, alpha, beta, extended):
    """the loop of product_decode over any two objects with n and correct_batch(X, chase=, soft=[, extended=True])"""
    kw = dict(extended=True) if extended else {}
    torch_in = _is_torch(y)
    if torch_in:
        y = y.contiguous()
        import torch
        W = torch.zeros_like(y)
        turn = lambda a: a.transpose(1, 2).contiguous()
    else:
        y = np.ascontiguousarray(y, np.float32)
        W = np.zeros_like(y)
        turn = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    B, n2, n1 = y.shape
    for h, (a, b) in enumerate(zip(alpha, beta)):
        scaled = W * a if torch_in else W * np.float32(a)
        X = y + scaled
        code, lines, length = (rows, n2, n1) if h % 2 == 0 else (cols, n1, n2)
        res = code.correct_batch((X if h % 2 == 0 else turn(X)).reshape(B * lines, length), chase=p, soft=b, **kw)
        out, W = res["out"].reshape(B, lines, length), res["ext"].reshape(B, lines, length)
        if h % 2:
            out, W = turn(out), turn(W)
        status = res["status"].reshape(B, lines)
    return dict(out=out, ext=W, status=status)


def product_decode(rows, cols, y, p, alpha, beta, extended=False):
    """Iterative (turbo) decoding of a product code with the Chase-Pyndiah component decoder,
    correct_batch(chase=p, soft=beta).  y: (B, n2, n1) float32 channel values, numpy array or device tensor, positive
    meaning bit 0; every row y[b, i, :] is a received word of `rows` (n1 = rows.n), every column y[b, :, k] one of `cols`
    (n2 = cols.n).  alpha and beta are sequences of equal length with one entry per half-iteration.  W starts at zero;
    half-iteration h forms X = y + (alpha[h] * W), a float32 product and a float32 sum, decodes the rows of X (h even)
    or its columns (h odd), and W becomes the ext of that pass.  Returns dict(out=, ext=, status=) of the last
    half-iteration: out (B, n2, n1) u8 and ext (B, n2, n1) f32 in the orientation of y, status (B, n2) after a row pass
    and (B, n1) after a column pass, one entry per component word.
    W is not normalised and there is no default schedule: good values depend on the scaling of y.  For y = +-1 + noise
    R. Pyndiah (IEEE Trans. Commun. 46 (8), 1998) gives for eight half-iterations alpha = 0, 0.2, 0.3, 0.5, 0.7, 0.9, 1,
    1 and beta = 0.2, 0.4, 0.6, 0.8, 1, 1, 1, 1 -- with W normalised to mean magnitude one, so a starting point only.
    extended=True: the product of the two extended codes (see extend), y of shape (B, cols.n + 1, rows.n + 1); every row
    and column goes through correct_batch(chase=p, soft=beta, extended=True), and out, ext and status are those of the
    extended words.
    Two codes of this package are decoded by one call of the library, product_code(rows, cols, extended).correct_batch
    (cc_product_decode); any other pair of objects with n and correct_batch is looped over here.  The outputs are the
    same bits either way."""
    alpha, beta = [float(np.float32(a)) for a in alpha], [float(np.float32(b)) for b in beta]
    e = 1 if extended else 0
    if len(alpha) != len(beta) or not alpha:
        raise ValueError("product_decode takes one alpha and one beta per half-iteration, at least one")
    if len(y.shape) != 3 or y.shape[1] != cols.n + e or y.shape[2] != rows.n + e:
        raise CcError(capi.ERR_LENGTH, "product_decode")
    if _is_torch(y):
        import torch
        if y.dtype != torch.float32:
            raise TypeError("product_decode takes float32 channel values")
    else:
        y = np.asarray(y)
        if y.dtype.kind != "f":
            raise TypeError("product_decode takes float32 channel values")
    if isinstance(rows, cyclic) and isinstance(cols, cyclic):
        return product_code(rows, cols, extended).correct_batch(y, p, alpha, beta)
    return _product_loop(rows, cols, y, p, alpha, beta, extended)


def pack_bits(a):
    """One symbol per bit, shape (..., n) -> packed uint8, shape (..., ceil(n / 8)): the coefficient of x^p in bit p & 7
    of byte p >> 3 (numpy.packbits(bitorder="little")); bit 0 of each symbol counts, pad bits are 0.  numpy arrays on the
    host; torch device tensors (uint8, or 16-bit for the symbols of q > 8) through cc_pack_bits_dev on the current
    stream."""
    if _is_torch(a) and a.is_cuda:
        import torch
        a = a.contiguous()
        if a.dtype not in _torch_symbol_dtypes():
            raise TypeError("pack_bits takes uint8 symbols or 16-bit integer symbols")
        n = a.shape[-1]
        B = a.numel() // n if n else 0
        out = torch.empty(a.shape[:-1] + ((n + 7) // 8,), dtype=torch.uint8, device=a.device)
        with torch.cuda.device(a.device):
            capi.check(capi.lib().cc_pack_bits_dev(_ptr(a), a.element_size(), n, _ptr(out), B, _stream_handle(a)),
                       "cc_pack_bits_dev")
        return out
    if _is_torch(a):
        import torch
        return torch.from_numpy(pack_bits(a.numpy()))
    a = np.asarray(a)
    return np.packbits((a & 1).astype(np.uint8), axis=-1, bitorder="little")


def unpack_bits(a, n, dtype=None):
    """Packed uint8, shape (..., ceil(n / 8)) -> one symbol per bit, shape (..., n); pad bits are ignored.  dtype: uint8
    (default) or a 16-bit type for the symbols of q > 8."""
    n = int(n)
    if a.shape[-1] != (n + 7) // 8:
        raise CcError(capi.ERR_LENGTH, "unpack_bits")
    if _is_torch(a) and a.is_cuda:
        import torch
        a = a.contiguous()
        if a.dtype != torch.uint8:
            raise TypeError("packed words are uint8")
        dtype = dtype or torch.uint8
        if dtype not in _torch_symbol_dtypes():
            raise TypeError("unpack_bits gives uint8 symbols or 16-bit integer symbols")
        out = torch.empty(a.shape[:-1] + (n,), dtype=dtype, device=a.device)
        B = out.numel() // n if n else 0
        with torch.cuda.device(a.device):
            capi.check(capi.lib().cc_unpack_bits_dev(_ptr(a), n, _ptr(out), out.element_size(), B, _stream_handle(a)),
                       "cc_unpack_bits_dev")
        return out
    if _is_torch(a):
        import torch
        return torch.from_numpy(unpack_bits(a.numpy(), n)).to(dtype or torch.uint8)
    a = np.ascontiguousarray(a, np.uint8)
    return np.unpackbits(a, axis=-1, count=n, bitorder="little").astype(dtype or np.uint8)


def _interleave_move(x, I, to_interleaved):
    I = int(I)
    if I < 1 or I > 256:
        raise CcError(capi.ERR_INVALID_ARGUMENT, "interleave")
    if to_interleaved:
        if x.ndim != 2 or x.shape[0] % I:
            raise CcError(capi.ERR_INVALID_ARGUMENT, "interleave")
        B, n = x.shape
        shape = (B // I, n, I)
    else:
        if x.ndim != 3 or x.shape[2] != I:
            raise CcError(capi.ERR_INVALID_ARGUMENT, "deinterleave")
        n = x.shape[1]
        B = x.shape[0] * I
        shape = (B, n)
    if _is_torch(x) and x.is_cuda:
        import torch
        x = x.contiguous()
        if x.dtype not in _torch_symbol_dtypes():
            raise TypeError("interleave / deinterleave take uint8 symbols or 16-bit integer symbols")
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
        fn = "cc_interleave_dev" if to_interleaved else "cc_deinterleave_dev"
        with torch.cuda.device(x.device):
            capi.check(getattr(capi.lib(), fn)(_ptr(x), x.element_size(), n, I, _ptr(out), B, _stream_handle(x)), fn)
        return out
    if _is_torch(x):
        import torch
        return torch.from_numpy(_interleave_move(x.numpy(), I, to_interleaved))
    x = np.asarray(x)
    if to_interleaved:
        return np.ascontiguousarray(x.reshape(B // I, I, n).transpose(0, 2, 1))
    return np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(B, n)


def interleave(x, I):
    """Frame-major symbols, shape (B, n), B a multiple of I -> symbol-interleaved blocks, shape (B / I, n, I): symbol p of
    frame b I + j at [b, p, j].  numpy arrays on the host; torch device tensors (uint8, or 16-bit for the
    symbols of q > 8) through cc_interleave_dev on the current stream."""
    return _interleave_move(x, I, True)


def deinterleave(x, I):
    """Symbol-interleaved blocks, shape (B / I, n, I) -> frame-major symbols, shape (B, n); see interleave."""
    return _interleave_move(x, I, False)


def burst_channel(code, interleave=1, p_gb=0.0, p_bg=1.0, p_error_good=0.0, p_error_bad=0.5, seed=0, first_frame=0,
                  frames=0, random_codewords=False):
    """Frames [first_frame, first_frame + frames) of the Gilbert-Elliott burst channel (cc_burst_channel_dev) along
    blocks of depth `interleave` on the current device; frames and first_frame are multiples of the depth.  Returns
    (recv, sent, state): torch uint8 tensors of shape (frames / interleave, n, interleave) -- recv and sent in the
    interleaved layout (deinterleave() gives the frames), state 0 good / 1 bad for every transmitted symbol."""
    import torch
    I, frames = int(interleave), int(frames)
    ch = capi.BurstChannel(I, p_gb, p_bg, p_error_good, p_error_bad)
    dev = torch.device("cuda", torch.cuda.current_device())
    shape = (frames // I if 1 <= I <= 256 else 0, code.n, I)
    recv, sent, state = (torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(3))
    rc = capi.lib().cc_burst_channel_dev(code._h, C.byref(ch), int(seed), int(first_frame), frames,
                                         int(bool(random_codewords)), _ptr(recv), _ptr(sent), _ptr(state),
                                         _stream_handle(recv))
    capi.check(rc, "cc_burst_channel_dev")
    return recv, sent, state


def burst_erasure_channel(code, interleave, p_gb, p_bg, p_error_good, p_error_bad, p_detect, p_false_alarm, seed=0,
                          first_frame=0, frames=0, random_codewords=True):
    """burst_channel with a burst detector (cc_burst_erasure_channel_dev): a symbol is flagged with probability p_detect
    in the bad state and p_false_alarm in the good one, and a flagged symbol is received as 0.  Returns a dict of torch
    tensors: recv, sent, state and flag (0 / 1), uint8 of shape (frames / interleave, n, interleave) in transmission
    order, and the erasure list per frame in frame-major numbering f = b I + j (the rows of deinterleave(recv)) as
    discrete_channel gives it: erasures (int16 positions, ascending within a frame, trimmed to off[-1]) and
    erasure_offsets (frames + 1,) int32.  The int32 offsets bound one call to frames * n < 2^31."""
    import torch
    I, frames = int(interleave), int(frames)
    if frames * code.n >= 1 << 31:
        raise ValueError("burst_erasure_channel: frames * n must stay below 2^31 (int32 offsets)")
    ch = capi.BurstChannel(I, p_gb, p_bg, p_error_good, p_error_bad)
    det = capi.BurstDetector(p_detect, p_false_alarm)
    dev = torch.device("cuda", torch.cuda.current_device())
    shape = (frames // I if 1 <= I <= 256 else 0, code.n, I)
    recv, sent, state, flag = (torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(4))
    off = torch.zeros(frames + 1, dtype=torch.int32, device=dev)
    er = torch.empty(max(1, frames * code.n), dtype=torch.int16, device=dev)
    rc = capi.lib().cc_burst_erasure_channel_dev(code._h, C.byref(ch), C.byref(det), int(seed), int(first_frame), frames,
                                                 int(bool(random_codewords)), _ptr(recv), _ptr(sent), _ptr(state),
                                                 _ptr(flag), _ptr(er), _ptr(off), _stream_handle(recv))
    capi.check(rc, "cc_burst_erasure_channel_dev")
    return dict(recv=recv, sent=sent, state=state, flag=flag, erasures=er[:int(off[-1])], erasure_offsets=off)


def bsc_packed_channel(code, p, seed=0, first_frame=0, frames=0, random_codewords=False):
    """Frames [first_frame, first_frame + frames) of the binary symmetric channel on packed words
    (cc_bsc_packed_channel_dev) on the current device, for any binary BCH code, q = 3 .. 15: bit for bit the BSC of
    discrete_channel(p, 0), in the container of pack_bits.  Returns recv, a torch uint8 tensor of shape
    (frames, code.packed_bytes) with the pad bits 0 -- and with random_codewords the pair (recv, sent), sent the packed
    words transmitted (without, the all-zero word is sent)."""
    import torch
    frames = int(frames)
    dev = torch.device("cuda", torch.cuda.current_device())
    recv = torch.empty((frames, code.packed_bytes), dtype=torch.uint8, device=dev)
    sent = torch.empty_like(recv) if random_codewords else None
    rc = capi.lib().cc_bsc_packed_channel_dev(code._h, float(p), int(seed), int(first_frame), frames,
                                              int(bool(random_codewords)), _ptr(recv), _ptr(sent), _stream_handle(recv))
    capi.check(rc, "cc_bsc_packed_channel_dev")
    return (recv, sent) if random_codewords else recv


class cyclic:
    """Common part of primitive_bch and rs (cyclic::cyclic<...>, cyclic.h:67-386)."""
    family = None

    def __init__(self, q, capability, algorithm=None, coding="division", mu=1, step=1,
                 stop_rule=capi.STOP_PARITY, device=None, H=None, modular_polynomial=None, n=None):
        """modular_polynomial: math::modular_polynomial<> (galois.h:23-25), bit i = coefficient of x^i; None = the
        default of galois.h:18-20, which exists for q <= 8 only.  q > 8: symbols are numpy uint16 / torch int16.
        n: code length; None (or 2^q - 1) = full length, k < n < 2^q - 1 = the code shortened to n symbols (the
        words of the full code that are zero at positions n .. 2^q - 2, cut to n symbols)."""
        if isinstance(capability, int):
            capability = errors(capability)
        algorithm = algorithm if algorithm is not None else peterson_gorenstein_zierler_tag()
        if isinstance(algorithm, type):
            algorithm = algorithm()
        self.algorithm = algorithm
        self.capability = capability
        lib = capi.lib()
        d = capi.Desc()
        lib.cc_desc_init(C.byref(d))
        d.family, d.q, d.t = self.family, int(q), int(capability.t)
        d.mu, d.step = int(mu), int(step)
        d.coding = capi.CODING_MULTIPLICATION if coding in ("multiplication", capi.CODING_MULTIPLICATION) \
            else capi.CODING_DIVISION
        d.algorithm = algorithm.alg
        d.iterations = algorithm.iterations
        d.alpha, d.beta = float(algorithm.alpha), float(algorithm.beta)
        d.stop_rule = int(stop_rule)
        d.device = capi.DEVICE_CURRENT if device is None else int(device)
        d.modular_polynomial = int(modular_polynomial or 0)
        d.n = int(n or 0)
        self.wide = int(q) > 8
        self._desc = d
        h = C.c_void_p()
        if H is None:
            capi.check(lib.cc_code_create(C.byref(d), C.byref(h)), "cc_code_create")
        else:  # min_sum<float, U>(matrix, y, tag) on a caller-supplied parity-check matrix, e.g. H_alt()
            Hm = np.ascontiguousarray(H, np.uint8)
            if Hm.ndim != 2 or Hm.shape[1] != (int(n) if n else (1 << int(q)) - 1):
                raise ValueError("H must be a (rows, n) matrix")
            capi.check(lib.cc_code_create_with_H(C.byref(d), _ptr(Hm), Hm.shape[0], C.byref(h)),
                       "cc_code_create_with_H")
        self._h = h
        self.q = int(q)
        self.n, self.k, self.l = lib.cc_n(h), lib.cc_k(h), lib.cc_l(h)
        self.t, self.dmin, self.rate = lib.cc_t(h), lib.cc_dmin(h), lib.cc_rate(h)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                capi.lib().cc_code_destroy(h)
            except Exception:
                pass

    # ---- introspection ----
    def to_string(self):
        buf = C.create_string_buffer(128)
        capi.check(capi.lib().cc_to_string(self._h, buf, 128), "cc_to_string")
        return buf.value.decode()

    def _poly(self, which):
        if self.wide:
            out = np.zeros(1 << 16, np.uint16)
            m = capi.lib().cc_get_poly_u16(self._h, which, _ptr(out), out.size)
            if m < 0:
                raise CcError(capi.ERR_INVALID_ARGUMENT, "cc_get_poly_u16")
            return out[:m].copy()
        out = np.zeros(512, np.uint8)
        m = capi.lib().cc_get_poly(self._h, which, _ptr(out), 512)
        if m < 0:
            raise CcError(capi.ERR_INVALID_ARGUMENT, "cc_get_poly")
        return out[:m].copy()

    @property
    def g(self):
        return self._poly(0)

    @property
    def h(self):
        return self._poly(1)

    @property
    def roots(self):
        return self._poly(2)

    def H(self):
        H = np.zeros((self.k, self.n), np.uint8)
        capi.check(capi.lib().cc_get_H(self._h, _ptr(H)), "cc_get_H")
        return H

    def kernel_info(self):
        """Which device kernel cc_correct_*_batch dispatches to for this handle (diagnostics, bench.py)."""
        name = C.create_string_buffer(160)
        fpw, thr, lds = C.c_uint32(), C.c_uint32(), C.c_uint32()
        capi.check(capi.lib().cc_kernel_info(self._h, name, 160, C.byref(fpw), C.byref(thr), C.byref(lds)),
                   "cc_kernel_info")
        return {"kernel": name.value.decode(), "frames_per_workgroup": fpw.value, "threads": thr.value,
                "lds_bytes": lds.value}

    def H_alt(self):
        """cyclic::H_alt<uint8_t>() (cyclic.h:361-385), t*q rows."""
        H = np.zeros((self.t * self.q, self.n), np.uint8)
        rows = C.c_uint32()
        capi.check(capi.lib().cc_get_H_alt(self._h, _ptr(H), C.byref(rows)), "cc_get_H_alt")
        return H[: rows.value]

    def sigma(self, ebno_db):
        return capi.lib().cc_sigma(self._h, float(ebno_db))

    def discrete_channel(self, p_error, p_erasure, seed, first_frame, frames, random_codewords=False):
        """Frames [first_frame, first_frame + frames) of the discrete memoryless channel (cc_discrete_channel_dev) on
        the current device: a dict of torch tensors recv (frames, n) uint8, erasures (int16 positions, the CSR values
        trimmed to off[-1]), erasure_offsets (frames + 1,) int32 and sent (frames, n) uint8.  With p_erasure > 0 the
        int32 offsets bound one call to frames * n < 2^31 (ValueError otherwise: split the call)."""
        import torch
        frames = int(frames)
        if p_erasure > 0 and frames * self.n >= 1 << 31:
            raise ValueError("discrete_channel: frames * n must stay below 2^31 with erasures (int32 offsets)")
        dev = torch.device("cuda", torch.cuda.current_device())
        recv = torch.empty((frames, self.n), dtype=torch.uint8, device=dev)
        sent = torch.empty((frames, self.n), dtype=torch.uint8, device=dev)
        off = torch.zeros(frames + 1, dtype=torch.int32, device=dev)
        er = torch.empty(max(1, frames * self.n), dtype=torch.int16, device=dev) if p_erasure > 0 else None
        rc = capi.lib().cc_discrete_channel_dev(self._h, float(p_error), float(p_erasure), int(seed), int(first_frame),
                                                frames, int(bool(random_codewords)), _ptr(recv), _ptr(er),
                                                _ptr(off) if er is not None else None, _ptr(sent),
                                                _stream_handle(recv))
        capi.check(rc, "cc_discrete_channel_dev")
        total = int(off[-1]) if er is not None else 0
        erasures = er[:total] if er is not None else torch.empty(0, dtype=torch.int16, device=dev)
        return dict(recv=recv, erasures=erasures, erasure_offsets=off, sent=sent)

    # ---- packed bits (binary BCH codes with a hard algorithm): uint8 (B, ceil(n / 8)), see pack_bits ----
    def _packed_width(self, which):
        p = capi.lib().cc_packed_bytes(self._h, which)
        if p < 0:
            raise CcError(-p, "cc_packed_bytes")
        return p

    @property
    def packed_bytes(self):
        """Bytes of a packed codeword, ceil(n / 8)."""
        return self._packed_width(0)

    @property
    def packed_message_bytes(self):
        """Bytes of a packed message, ceil(l / 8)."""
        return self._packed_width(1)

    def packed_route(self, B):
        """1 if correct_batch(packed=True) of B frames without erasures decodes the packed words natively, 0 if it goes
        through unpack / byte route / pack (cc_packed_route).  Native: the GF(2^8) calls of the bit-plane chain, and for
        q = 9 .. 15 the BM and PGZ tags with t <= 31 in calls of at least CC_AMD_PACKED_LONG_MIN_FRAMES (default 1024)
        frames; the Euklid tag, t = 32 and smaller calls of those codes answer 0.  Both routes return the same result."""
        r = capi.lib().cc_packed_route(self._h, int(B))
        if r < 0:
            raise CcError(-r, "cc_packed_route")
        return r

    def hard_route(self, B, erasures=False):
        """The kernels a hard-decode call of B frames takes (cc_hard_route): capi.HARD_ROUTE_WAVE / CHUNK / PLANES / LONG /
        WIDE / TRIALS; raises where the call itself would be refused."""
        r = capi.lib().cc_hard_route(self._h, int(B), int(bool(erasures)))
        if r < 0:
            raise CcError(-r, "cc_hard_route")
        return r

    def packed_map_route(self, which):
        """1 if encode_batch (which = 0) / extract_batch (which = 1) with packed=True works on the packed words
        themselves, 0 if it goes through unpack / byte route / pack (cc_packed_map_route)."""
        r = capi.lib().cc_packed_map_route(self._h, int(which))
        if r < 0:
            raise CcError(-r, "cc_packed_map_route")
        return r

    # ---- symbol-interleaved blocks: arrays of shape (B / I, n, I), messages (B / I, l, I) ----
    def interleaved_route(self, B, I, erasures=False):
        """1 if correct_batch(interleave=I) of B frames decodes the interleaved blocks natively, 0 if it goes through
        de-interleave / plain route / interleave (cc_interleaved_route); raises where the call would be refused."""
        r = capi.lib().cc_interleaved_route(self._h, int(B), int(I), int(bool(erasures)))
        if r < 0:
            raise CcError(-r, "cc_interleaved_route")
        return r

    def interleaved_map_route(self, which, I):
        """The same for encode_batch (which = 0) / extract_batch (which = 1) with interleave=I."""
        r = capi.lib().cc_interleaved_map_route(self._h, int(which), int(I))
        if r < 0:
            raise CcError(-r, "cc_interleaved_map_route")
        return r

    # ---- batch API (numpy host arrays or torch CUDA tensors) ----
    def _batch_call(self, name, ins, B, outs, per_frame=(), args=(), tail=(), erasures=False, head=()):
        """One batch call of the library, for host arrays and device tensors alike: `name`(handle, *head, *ins[, erasure
        list], *args, *outs, *per_frame, B, *tail), for tensors `name`_dev with the stream last.  ins: the contiguous inputs.
        outs: the call's leading outputs in its order, key -> (shape, dtype), dtype None being that of ins[0]; a buffer
        of the caller's in place of the pair is used as it is, None passes a null pointer.  per_frame: the keys of
        _PER_FRAME that follow, (B,) each.  erasures: as correct_batch takes them, False for a call without the list.
        Returns the dict of the outputs, in the order of _KEYS."""
        x = ins[0]
        side = _side(x)
        call = [self._h] + list(head) + [_ptr(a) for a in ins]
        if erasures is not False:
            lists = _erasure_csr(erasures, B, self.n)
            if lists[0] is not None:
                lists = side.erasure_list(x, *lists)
            call += [_ptr(lists[0]), _ptr(lists[1])]
        call += args
        res = {k: side.alloc(x, *s) if type(s) is tuple else s for k, s in outs.items()}
        for k in per_frame:
            res[k] = side.alloc(x, (B,), _PER_FRAME[k])
        call += [_ptr(a) for a in res.values()]
        call.append(B)
        call += tail
        call += side.stream(x)
        name += side.dev
        capi.check(getattr(capi.lib(), name)(*call), name)
        return {k: res[k] for k in _KEYS if k in res and res[k] is not None}

    def _symbols(self, op, x, which, packed, I, out=None):
        """The symbol input of a batch call in its layout -- packed=True (uint8 words, see pack_bits), interleave=I
        (blocks of shape (B / I, width, I)) or plain, 8-bit symbols or for q > 8 16-bit ones (numpy uint16 on the host,
        torch int16 / uint16 on the device) -- holding codewords (which = 0) or messages (1).  Checks shape and type and
        returns (the C name of `op`, x contiguous in the layout's type, B, the call's arguments after B, shape), with
        shape(which) the layout's shape of B codewords / messages.  out: correct_batch's out=, for the in-place rule."""
        side, wide, depth = _side(x), self.wide and not packed, I is not None
        name = "cc_" + op + ("_packed_batch" if packed else "_interleaved_batch" if depth else "_batch") \
            + ("_u16" if wide else "")

        def wrong_length():
            # named after the method, but after the C call for blocks (the fused decode apart) and packed or 16-bit maps
            if (depth and op != "decode_hard") or (op in ("encode", "extract") and (packed or wide)):
                return CcError(capi.ERR_LENGTH, name + (side.dev if wide and not depth else ""))
            return CcError(capi.ERR_LENGTH, op.split("_")[0] + "_batch")
        width = self._packed_width if packed else (self.n, self.l).__getitem__
        w = width(which)
        if depth:
            I = int(I)
            if x.ndim != 3 or x.shape[1] != w or x.shape[2] != I:
                raise wrong_length()
            if not side.is_symbols(x):
                raise TypeError("interleave= takes unsigned symbols")
        else:
            x = side.asarray(x)
            if x.shape[-1] != w:
                raise wrong_length()
        dtype, itemsize = (np.uint16, 2) if wide else (np.uint8, 1)
        if out is x and not side.is_contiguous(x, dtype):
            raise TypeError("decoding in place needs a contiguous " + side.in_place_needs[bool(packed)])
        x = side.symbols(x, dtype, itemsize, wide and not depth)
        if x is None:
            if depth:
                raise TypeError("interleave= takes uint8 symbols (16-bit integer symbols for q > 8)")
            if packed and op == "correct_hard":
                raise TypeError("packed words are uint8")
            raise wrong_length()
        B = side.size(x) // w
        if depth:
            blocks = x.shape[0]
            return name, x, B, (I,), lambda which: (blocks, width(which), I)
        return name, x, B, (), lambda which: (B, width(which))

    def _map(self, op, x, which, packed, interleave):
        """encode_batch (messages in, which = 1) and extract_batch (codewords in, which = 0) in every layout"""
        if interleave is not None and packed:
            raise TypeError("interleave= does not combine with packed=True")
        name, x, B, tail, shape = self._symbols(op, x, which, packed, interleave)
        return self._batch_call(name, [x], B, {"out": (shape(1 - which), None)}, tail=tail)["out"]

    def encode_batch(self, msg, packed=False, interleave=None):
        """packed=True: uint8 (B, packed_message_bytes) -> uint8 (B, packed_bytes), see pack_bits.
        interleave=I: symbol-interleaved blocks, (B / I, l, I) -> (B / I, n, I), see interleave()."""
        return self._map("encode", msg, 1, packed, interleave)  # a wrong length: cyclic.h:291-296

    def extract_batch(self, cw, packed=False, interleave=None):
        """interleave=I: symbol-interleaved blocks, (B / I, n, I) -> (B / I, l, I), see interleave()."""
        return self._map("extract", cw, 0, packed, interleave)

    def correct_batch(self, b, erasures=None, want_L=False, packed=False, out=None, interleave=None, chase=None, gmd=None,
                      reliability=None, soft=None, extended=False, osd=None):
        """Returns a dict: out (B,n) u8, status (B,) i32, and nerr (hard) or iters [+ L] (soft).
        gmd=m, reliability=r (RS, hard algorithms, q <= 8, 2t <= 32, step = 1): b holds the received symbols, r float32
        reliabilities of the same shape, and the frames are decoded by GMD with m trials (cc_correct_gmd_batch; gmd=True:
        all t + 1); the dict also carries metric (B,) f32.  It does not combine with erasures, packed, interleave, want_L,
        out= or chase=.
        chase=p (binary BCH, hard algorithms, q <= 8, 2t <= 32): b holds float32 channel values and is decoded by
        Chase's algorithm 2 over the p least reliable positions (cc_correct_chase_batch); the dict also carries
        metric (B,) f32.  It does not combine with erasures, packed, interleave or want_L.
        chase=p, soft=beta (beta a finite float >= 0): the same with the Chase-Pyndiah soft output
        (cc_correct_chase_soft_batch); the dict also carries ext (B,n) f32, the extrinsic value of every bit, beta in
        magnitude where no candidate disagrees with the decision.  soft= needs chase= and combines with nothing else.
        chase=p, extended=True[, soft=beta]: the extended code, every word with its overall parity bit appended (see
        extend): b, out and ext have rows of n + 1, position n carrying the parity bit, which enters the metric and
        the soft output (cc_correct_chase_extended_batch).  extended= needs chase=.
        osd=order (binary BCH, hard algorithms, q <= 8, any t): b holds float32 channel values and is decoded by
        ordered-statistics decoding of order 0 .. 2 (cc_correct_osd_batch); the dict is that of chase=, status always 0.
        It combines with nothing chase= is refused with, nor with chase=, gmd=, soft= or extended=.
        packed=True (binary BCH codes, hard algorithms): b and out are uint8 (B, packed_bytes), see pack_bits; out= names
        the buffer the corrected packed words go to (b itself decodes in place).  The long codes (q = 9 .. 15, BM / PGZ,
        t <= 31, no erasures) are decoded from the packed words themselves in calls of device tensors of at least
        CC_AMD_PACKED_LONG_MIN_FRAMES frames, see packed_route.
        interleave=I (hard algorithms): b and out are symbol-interleaved blocks of shape (B / I, n, I), see interleave();
        status, nerr and the erasure lists are per frame f = b I + j, as without it; out= as with packed=True."""
        if osd is not None:
            if (erasures is not None or want_L or packed or out is not None or interleave is not None or chase is not None
                    or gmd is not None or reliability is not None or soft is not None or extended):
                raise TypeError("osd= does not combine with erasures, want_L, packed=True, out=, interleave=, chase=, gmd=, "
                                "reliability=, soft= or extended=")
            return self._osd(b, osd)
        if soft is not None and (chase is None or gmd is not None or reliability is not None):
            raise TypeError("soft= goes with chase= and with nothing else")
        if extended and (chase is None or gmd is not None or reliability is not None):
            raise TypeError("extended= goes with chase=[, soft=] and with nothing else")
        if gmd is not None or reliability is not None:
            if (erasures is not None or want_L or packed or out is not None or interleave is not None
                    or chase is not None):
                raise TypeError("gmd= does not combine with erasures, want_L, packed=True, out=, interleave= or chase=")
            if gmd is None or reliability is None:
                raise TypeError("gmd= and reliability= go together")
            return self._gmd(b, reliability, gmd)
        if chase is not None:
            if erasures is not None or want_L or packed or out is not None or interleave is not None:
                raise TypeError("chase= does not combine with erasures, want_L, packed=True, out= or interleave=")
            return self._chase(b, chase, soft, bool(extended))
        if interleave is not None and packed:
            raise TypeError("interleave= does not combine with packed=True")
        if interleave is None and not packed and out is not None:
            raise TypeError("out= goes with packed=True or interleave=")
        side, soft_alg = _side(b), self.algorithm.soft
        if interleave is not None or packed or (self.wide and not soft_alg):  # symbols, whatever the algorithm
            name, x, B, tail, shape = self._symbols("correct_hard", b, 0, packed, interleave, out)
            if out is None:
                out = (shape(0), None)
            elif out is b and side is _device:  # decoding in place: the (contiguous) input itself
                out = x
            elif not side.is_buffer(out, x, shape(0)):
                raise TypeError("out= must be a contiguous " + side.out_must_be[bool(packed)])
            return self._batch_call(name, [x], B, {"out": out}, ("nerr", "status"), tail=tail, erasures=erasures)
        # (min-sum takes LLRs and returns bits whatever the symbol width)
        b = side.asarray(b)
        if b.shape[-1] != self.n:
            raise CcError(capi.ERR_LENGTH, "correct_batch")  # cyclic.h:213-218
        kind, x = side.channel_input(b, soft_alg)
        B = side.size(x) // self.n
        outs = {"out": ((B, self.n), np.uint8)}
        if soft_alg:
            outs["L"] = ((B, self.n), np.float32) if want_L else None
        return self._batch_call("cc_correct_%s_batch" % kind, [x], B, outs, ("iters" if soft_alg else "nerr", "status"),
                                erasures=erasures)

    def _chase(self, b, p, beta=None, extended=False):
        """correct_batch(chase=p[, soft=beta][, extended=True]): float32 channel values, host array or device tensor."""
        p = int(p)
        if p < 0:
            raise ValueError("chase= takes p >= 0")
        if beta is not None:
            if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)):
                raise TypeError("soft= takes beta, a float")
            with np.errstate(over="ignore"):  # (beyond float32: +inf, which the call refuses)
                beta = float(np.float32(beta))
        w = self.n + 1 if extended else self.n
        if b.shape[-1] != w:
            raise CcError(capi.ERR_LENGTH, "correct_batch")
        side = _side(b)
        y = side.as_type(b, "f", np.float32)
        if y is None:
            raise TypeError("chase= takes float32 channel values")
        B = side.size(y) // w
        outs = {"out": ((B, w), np.uint8)}
        if extended:  # one call for both outputs: a null ext selects the hard output, and beta is then not read
            outs["ext"] = ((B, w), np.float32) if beta is not None else None
            return self._batch_call("cc_correct_chase_extended_batch", [y], B, outs, ("nerr", "metric", "status"),
                                    (p, 0.0 if beta is None else beta))
        if beta is None:
            return self._batch_call("cc_correct_chase_batch", [y], B, outs, ("nerr", "metric", "status"), (p,))
        outs["ext"] = ((B, self.n), np.float32)
        return self._batch_call("cc_correct_chase_soft_batch", [y], B, outs, ("nerr", "metric", "status"), (p, beta))

    def _osd(self, b, order):
        """correct_batch(osd=order): float32 channel values, host array or device tensor."""
        order = int(order)
        if order < 0:
            raise ValueError("osd= takes order >= 0")
        if b.shape[-1] != self.n:
            raise CcError(capi.ERR_LENGTH, "correct_batch")
        side = _side(b)
        y = side.as_type(b, "f", np.float32)
        if y is None:
            raise TypeError("osd= takes float32 channel values")
        B = side.size(y) // self.n
        return self._batch_call("cc_correct_osd_batch", [y], B, {"out": ((B, self.n), np.uint8)},
                                ("nerr", "metric", "status"), (order,))

    def _gmd(self, b, rel, m):
        """correct_batch(gmd=m, reliability=rel): uint8 symbols and float32 reliabilities, host arrays or device tensors."""
        m = capi.gmd_trials(m)
        if b.shape[-1] != self.n or tuple(rel.shape) != tuple(b.shape):
            raise CcError(capi.ERR_LENGTH, "correct_batch")
        side = _side(b)
        if side is not _side(rel):
            raise TypeError("gmd= takes the symbols and the reliabilities both on the host or both on the device")
        w, r = side.as_type(b, "u", np.uint8), side.as_type(rel, "f", np.float32)
        if w is None or r is None or (side is _device and r.device != w.device):
            raise TypeError("gmd= takes uint8 symbols and float32 reliabilities"
                            + (" on one device" if side is _device else ""))
        B = side.size(w) // self.n
        return self._batch_call("cc_correct_gmd_batch", [w, r], B, {"out": ((B, self.n), np.uint8)},
                                ("nerr", "metric", "status"), (m,))

    def decode_batch(self, b, erasures=None, packed=False, interleave=None, chase=None, gmd=None, reliability=None,
                     soft=None, extended=False, osd=None):
        """decode = correct + message extraction (cyclic.h:313-327); host arrays go through cc_decode_*_batch.
        chase=p[, soft=beta]: correct_batch(b, chase=p[, soft=beta]), then the messages of its words.
        chase=p, extended=True[, soft=beta]: the same on extended words; msg comes from their inner n columns.
        gmd=m, reliability=r: correct_batch(b, gmd=m, reliability=r), then the messages of its words.
        osd=order: correct_batch(b, osd=order), then the messages of its words.
        packed=True: b, out and msg are packed uint8 words, see pack_bits.
        interleave=I: b and out are blocks of shape (B / I, n, I), msg (B / I, l, I), see interleave()."""
        if chase is not None or gmd is not None or reliability is not None or soft is not None or extended or osd is not None:
            res = self.correct_batch(b, erasures, packed=packed, interleave=interleave, chase=chase, gmd=gmd,
                                     reliability=reliability, soft=soft, extended=extended, osd=osd)
            res["msg"] = self.extract_batch(unextend(res["out"]) if extended else res["out"])
            return res
        if interleave is not None and packed:
            raise TypeError("interleave= does not combine with packed=True")
        fused = _side(b) is _host  # the fused calls take host arrays; 16-bit blocks have none
        if fused and (interleave is not None or packed):
            if not self.wide or packed:
                name, x, B, tail, shape = self._symbols("decode_hard", b, 0, packed, interleave)
                return self._batch_call(name, [x], B, {"msg": (shape(1), None), "out": (shape(0), None)},
                                        ("nerr", "status"), tail=tail, erasures=erasures)
        elif fused:
            b = np.asarray(b)
            if b.shape[-1] != self.n:
                raise CcError(capi.ERR_LENGTH, "decode_batch")
            signed = b.dtype.kind in "fi"
            if self.algorithm.soft or not signed:
                x = np.ascontiguousarray(b, np.float32 if signed else np.uint8)
                B = x.size // self.n
                return self._batch_call("cc_decode_soft_batch" if signed else "cc_decode_hard_batch", [x], B,
                                        {"msg": ((B, self.l), np.uint8), "out": ((B, self.n), np.uint8)},
                                        ("iters" if signed else "nerr", "status"), erasures=erasures)
            # (a hard algorithm on channel values: bit = (x < 0), cyclic.h:163-173)
        res = self.correct_batch(b, erasures, packed=packed, interleave=interleave)
        res["msg"] = self.extract_batch(res["out"], packed, interleave)
        return res

    # ---- single-frame API with the reference's exception behaviour ----
    _MESSAGES = {
        capi.FRAME_NOT_CONVERGED: "Decoding failure",
        capi.FRAME_LOCATOR: "Sigma(x) does not have as many distinct zeroes as its degree",
        capi.FRAME_RECHECK: "Corrected word is not a codeword",
        capi.FRAME_ERASURES: "Number of erasures exceed error correction capability.",
    }

    def _as_frame(self, seq, length, what):
        if isinstance(seq, (list, tuple)):
            arr = np.asarray(seq)
            if arr.dtype.kind == "i" and (arr >= 0).all():
                arr = arr.astype(np.uint8) if (arr < 256).all() else arr
        else:
            arr = np.asarray(seq)
        if arr.ndim != 1 or arr.shape[0] != length:
            raise RuntimeError("%s has the wrong size (%d). Expected %d" % (what, arr.shape[0] if arr.ndim else 0,
                                                                           length))
        return arr

    def encode(self, a):
        a = self._as_frame(a, self.l, "Source code word")
        return self.encode_batch(a.astype(np.uint8)[None, :])[0]

    def correct(self, b, erasures=None):
        b = self._as_frame(b, self.n, "Channel code word")
        res = self.correct_batch(b[None, :], None if not erasures else list(erasures))
        st = int(res["status"][0])
        if st != capi.FRAME_OK:
            raise decoding_failure(self._MESSAGES.get(st, "decoding failure %d" % st))
        return res["out"][0]

    def decode(self, b, erasures=None):
        return self.extract_batch(self.correct(b, erasures)[None, :])[0]


class primitive_bch(cyclic):
    """cyclic::primitive_bch<q, Capability, Sigma, N, Coding> (bch.h:16-19)."""
    family = capi.FAMILY_BCH

    def __init__(self, q, capability, algorithm=None, coding="division", **kw):
        super().__init__(q, capability, algorithm, coding, 1, 1, **kw)


class rs(cyclic):
    """cyclic::rs<q, Capability, Sigma, N, Coding, mu, step> (rs.h:6-10)."""
    family = capi.FAMILY_RS

    def __init__(self, q, capability, algorithm=None, coding="division", mu=1, step=1, **kw):
        super().__init__(q, capability, algorithm, coding, mu, step, **kw)


def _sr_weights(weights):
    """the weights of an iBDD-SR call as C floats, one per half-iteration and at least one (inf is a weight; what the
    library refuses -- NaN, a negative weight, too many distinct ones -- is left to it)"""
    with np.errstate(over="ignore"):
        w = [float(np.float32(a)) for a in weights]
    if not w:
        raise ValueError("one weight per half-iteration, at least one")
    return (C.c_float * len(w))(*w)


def _anchor_delta(delta):
    """delta of the anchor decoder as the uint32 of the C calls"""
    if isinstance(delta, bool) or int(delta) != delta:
        raise TypeError("delta takes an integer")
    delta = int(delta)
    if not 1 <= delta < 1 << 32:
        raise ValueError("delta = 1 .. 2^32 - 1")
    return delta


class _product_handle:
    """what cyclic._batch_call reads of a code, for a call whose first argument is a cc_product"""

    def __init__(self, pc):
        self._h, self.n = C.byref(pc), 0


class product_code:
    """The product of two binary BCH codes (cc_product): a block is (n2, n1) symbols whose rows are words of
    `rows` and whose columns are words of `cols`; extended=True the product of the two extended codes, (n2 + 1, n1 + 1).
    Both are handles correct_batch(chase=p) accepts, on one device.  n1, n2, k1, k2: lengths and message lengths of the
    components; n = values per block, l = k1 k2 message bits per block."""

    def __init__(self, rows, cols, extended=False):
        if not isinstance(rows, cyclic) or not isinstance(cols, cyclic):
            raise TypeError("product_code takes two codes of this package")
        self.rows, self.cols, self.extended = rows, cols, bool(extended)
        e = 1 if self.extended else 0
        self.n1, self.n2, self.k1, self.k2 = rows.n + e, cols.n + e, rows.l, cols.l
        self.n, self.l = self.n1 * self.n2, self.k1 * self.k2
        self.rate = self.l / self.n

    def to_string(self):
        return "%sx%s%s" % (self.rows.to_string(), self.cols.to_string(), "-ext" if self.extended else "")

    def _pc(self, p=0, alpha=(), beta=()):
        """the cc_product of a call (the schedule arrays live as long as the object returned)"""
        with np.errstate(over="ignore"):
            alpha, beta = [float(np.float32(a)) for a in alpha], [float(np.float32(b)) for b in beta]
        if len(alpha) != len(beta):
            raise ValueError("one alpha and one beta per half-iteration")
        p = int(p)
        if p < 0:
            raise ValueError("p >= 0")
        fa, fb = (C.c_float * max(1, len(alpha)))(*alpha), (C.c_float * max(1, len(beta)))(*beta)
        pc = capi.Product(self.rows._h, self.cols._h, int(self.extended), p, len(alpha), fa, fb)
        pc._keep = (fa, fb, self.rows, self.cols)
        return pc

    def sigma(self, ebno_db):
        return capi.lib().cc_product_sigma(C.byref(self._pc()), float(ebno_db))

    def _bytes(self, x, inner, what):
        """x as contiguous uint8 blocks of shape (B,) + inner"""
        side = _side(x)
        if tuple(x.shape[1:]) != inner or len(x.shape) != 3:
            raise CcError(capi.ERR_LENGTH, what)
        if side is _host:
            x = np.asarray(x)
            if x.dtype.kind not in "ub":
                raise TypeError(what + " takes uint8 symbols")
            return np.ascontiguousarray(x, np.uint8)
        import torch
        if x.dtype != torch.uint8:
            raise TypeError(what + " takes uint8 symbols")
        return x.contiguous()

    def encode_batch(self, msg):
        """(B, k2, k1) message bits -> (B, n2, n1) code blocks; numpy array or device tensor"""
        msg = self._bytes(msg, (self.k2, self.k1), "encode_batch")
        B = msg.shape[0]
        return cyclic._batch_call(_product_handle(self._pc()), "cc_product_encode_batch", [msg], B,
                                  {"out": ((B, self.n2, self.n1), np.uint8)})["out"]

    def extract_batch(self, cw):
        """(B, n2, n1) code blocks -> (B, k2, k1) message bits"""
        cw = self._bytes(cw, (self.n2, self.n1), "extract_batch")
        B = cw.shape[0]
        return cyclic._batch_call(_product_handle(self._pc()), "cc_product_extract_batch", [cw], B,
                                  {"msg": ((B, self.k2, self.k1), np.uint8)})["msg"]

    def correct_batch(self, y, p, alpha, beta, ext=True):
        """cc_product_decode: y (B, n2, n1) float32 -> dict(out=, status=[, ext=]) of the last of len(alpha)
        half-iterations (see product_decode); ext=False skips the soft output: the last half-iteration then runs the
        hard-output decoder."""
        if not len(alpha):
            raise ValueError("one alpha and one beta per half-iteration, at least one")
        pc = self._pc(p, alpha, beta)
        if len(y.shape) != 3 or tuple(y.shape[1:]) != (self.n2, self.n1):
            raise CcError(capi.ERR_LENGTH, "correct_batch")
        yy = _side(y).as_type(y, "f", np.float32)
        if yy is None:
            raise TypeError("product decoding takes float32 channel values")
        B = yy.shape[0]
        lines = self.n2 if pc.halves % 2 else self.n1
        outs = {"out": ((B, self.n2, self.n1), np.uint8), "ext": ((B, self.n2, self.n1), np.float32) if ext else None,
                "status": ((B, lines), np.int32)}
        return cyclic._batch_call(_product_handle(pc), "cc_product_decode", [yy], B, outs)

    def decode_batch(self, y, p, alpha, beta):
        """correct_batch plus msg (B, k2, k1): the message bits of out"""
        res = self.correct_batch(y, p, alpha, beta)
        res["msg"] = self.extract_batch(res["out"])
        return {k: res[k] for k in _KEYS if k in res}

    def _pc_hard(self, halves):
        """the cc_product of the hard-decision calls: they read rows, cols, extended and halves alone"""
        halves = int(halves)
        if halves < 1:
            raise ValueError("halves >= 1")
        pc = capi.Product(self.rows._h, self.cols._h, int(self.extended), 0, halves, None, None)
        pc._keep = (self.rows, self.cols)
        return pc

    def correct_hard_batch(self, z, halves):
        """cc_product_decode_hard: z (B, n2, n1) uint8 hard decisions -> dict(out=, nflip=, last=, status=) after
        `halves` half-iterations of bounded-distance row / column decoding; numpy array or device tensor."""
        pc = self._pc_hard(halves)
        z = self._bytes(z, (self.n2, self.n1), "correct_hard_batch")
        B = z.shape[0]
        side = _side(z)
        res = {"out": side.alloc(z, (B, self.n2, self.n1), np.uint8)}
        for k in ("nflip", "last", "status"):
            res[k] = side.alloc(z, (B,), np.int32)
        cyclic._batch_call(_product_handle(pc), "cc_product_decode_hard", [z], B, res)
        return res

    def decode_hard_batch(self, z, halves):
        """correct_hard_batch plus msg (B, k2, k1): the message bits of out"""
        res = self.correct_hard_batch(z, halves)
        res["msg"] = self.extract_batch(res["out"])
        return res

    def correct_anchor_batch(self, z, delta, halves):
        """cc_product_decode_anchor: z (B, n2, n1) uint8 hard decisions -> dict(out=, nflip=, last=, status=, nback=,
        nconf=) after `halves` half-iterations of anchor decoding: a correction that meets a converged crossing line is
        refused (nconf counts them), a converged line with `delta` >= 1 conflicts in one pass is taken back (nback).
        There is no default for delta; numpy array or device tensor."""
        delta = _anchor_delta(delta)
        pc = self._pc_hard(halves)
        z = self._bytes(z, (self.n2, self.n1), "correct_anchor_batch")
        B = z.shape[0]
        side = _side(z)
        res = {"out": side.alloc(z, (B, self.n2, self.n1), np.uint8)}
        for k in ("nflip", "last", "status", "nback", "nconf"):
            res[k] = side.alloc(z, (B,), np.int32)
        cyclic._batch_call(_product_handle(pc), "cc_product_decode_anchor", [z], B, res, head=[delta])
        return res

    def decode_anchor_batch(self, z, delta, halves):
        """correct_anchor_batch plus msg (B, k2, k1): the message bits of out"""
        res = self.correct_anchor_batch(z, delta, halves)
        res["msg"] = self.extract_batch(res["out"])
        return res

    def correct_sr_batch(self, y, weights):
        """cc_product_decode_sr: y (B, n2, n1) float32 channel values -> dict(out=, nflip=, last=, status=) after
        len(weights) half-iterations of iBDD with scaled reliability, weights[h] the threshold below which |y| yields to
        the component decoder in half-iteration h (inf: always); numpy array or device tensor."""
        fw = _sr_weights(weights)
        pc = self._pc_hard(len(fw))
        pc._keep += (fw,)
        if len(y.shape) != 3 or tuple(y.shape[1:]) != (self.n2, self.n1):
            raise CcError(capi.ERR_LENGTH, "correct_sr_batch")
        yy = _side(y).as_type(y, "f", np.float32)
        if yy is None:
            raise TypeError("product decoding takes float32 channel values")
        B = yy.shape[0]
        side = _side(yy)
        res = {"out": side.alloc(yy, (B, self.n2, self.n1), np.uint8)}
        for k in ("nflip", "last", "status"):
            res[k] = side.alloc(yy, (B,), np.int32)
        cyclic._batch_call(_product_handle(pc), "cc_product_decode_sr", [yy], B, res, head=[fw])
        return res

    def decode_sr_batch(self, y, weights):
        """correct_sr_batch plus msg (B, k2, k1): the message bits of out"""
        res = self.correct_sr_batch(y, weights)
        res["msg"] = self.extract_batch(res["out"])
        return res

    def channel(self, ebno_db, seed, first_block, blocks, random_codewords=False):
        """Blocks [first_block, first_block + blocks) of the AWGN channel on the current device (cc_awgn_product_dev):
        dict(y=(blocks, n2, n1) float32, sent=(blocks, n2, n1) uint8) of torch tensors."""
        import torch
        blocks = int(blocks)
        dev = torch.device("cuda", torch.cuda.current_device())
        y = torch.empty((blocks, self.n2, self.n1), dtype=torch.float32, device=dev)
        sent = torch.empty((blocks, self.n2, self.n1), dtype=torch.uint8, device=dev)
        rc = capi.lib().cc_awgn_product_dev(C.byref(self._pc()), float(ebno_db), int(seed), int(first_block), blocks,
                                            int(bool(random_codewords)), _ptr(y), _ptr(sent), _stream_handle(y))
        capi.check(rc, "cc_awgn_product_dev")
        return dict(y=y, sent=sent)


class staircase_code:
    """A staircase code of one binary BCH component (cc_staircase): a stream is (blocks, m, m) bits, line j
    of step i runs down column j of block i - 1 and along row j of block i and is a word of `code` (extended=True: of
    its extended code); block 0 is the zero block.  `code` is a handle correct_batch(chase=0) accepts with n + e even.
    window (blocks, the zero block included) and iters are the sliding-window decoder's.  m: block side, k_b: message
    bits per row, rate = k_b / m."""

    def __init__(self, code, blocks, window, iters, extended=False):
        if not isinstance(code, cyclic):
            raise TypeError("staircase_code takes a code of this package")
        self.code, self.extended = code, bool(extended)
        self.blocks, self.window, self.iters = int(blocks), int(window), int(iters)
        if self.blocks < 1:
            raise ValueError("blocks >= 1")
        if not 2 <= self.window <= capi.STAIRCASE_MAX_WINDOW:
            raise ValueError("window = 2 .. %d" % capi.STAIRCASE_MAX_WINDOW)
        if self.iters < 1:
            raise ValueError("iters >= 1")
        e = 1 if self.extended else 0
        if (code.n + e) % 2:
            raise ValueError("n + e must be even: a line splits into two halves of m bits")
        self.m = (code.n + e) // 2
        self.k_b = self.m - ((code.n - code.l) + e)
        if self.k_b < 1:
            raise ValueError("the parity bits of a line leave no message bit in a row of m")
        self.n, self.l = self.blocks * self.m * self.m, self.blocks * self.m * self.k_b
        self.rate = self.k_b / self.m

    def to_string(self):
        return "staircase(%s%s, L=%d, W=%d, I=%d)" % (self.code.to_string(), "-ext" if self.extended else "", self.blocks,
                                                      self.window, self.iters)

    def _sc(self):
        sc = capi.Staircase(self.code._h, int(self.extended), self.blocks, self.window, self.iters)
        sc._keep = self.code
        return sc

    def sigma(self, ebno_db):
        return capi.lib().cc_staircase_sigma(C.byref(self._sc()), float(ebno_db))

    def lds_bytes(self, weights=None):
        """LDS of one workgroup of the decoder; with weights (2 * iters of them), of the soft-aided decoder under them"""
        if weights is None:
            return capi.lib().cc_staircase_lds_bytes(C.byref(self._sc()))
        return capi.lib().cc_staircase_sr_lds_bytes(C.byref(self._sc()), self._weights(weights))

    def _weights(self, weights):
        """the weights of an iBDD-SR call as C floats: one per half-pass of a window position"""
        fw = _sr_weights(weights)
        if len(fw) != 2 * self.iters:
            raise ValueError("one weight per half-pass of a window position: 2 * iters = %d" % (2 * self.iters))
        return fw

    def _bytes(self, x, inner, what):
        """x as contiguous uint8 streams of shape (B,) + inner"""
        if tuple(x.shape[1:]) != inner or len(x.shape) != 4:
            raise CcError(capi.ERR_LENGTH, what)
        if _side(x) is _host:
            x = np.asarray(x)
            if x.dtype.kind not in "ub":
                raise TypeError(what + " takes uint8 symbols")
            return np.ascontiguousarray(x, np.uint8)
        import torch
        if x.dtype != torch.uint8:
            raise TypeError(what + " takes uint8 symbols")
        return x.contiguous()

    def encode_batch(self, msg):
        """(B, blocks, m, k_b) message bits -> (B, blocks, m, m) code streams; numpy array or device tensor"""
        msg = self._bytes(msg, (self.blocks, self.m, self.k_b), "encode_batch")
        B = msg.shape[0]
        return cyclic._batch_call(_product_handle(self._sc()), "cc_staircase_encode_batch", [msg], B,
                                  {"out": ((B, self.blocks, self.m, self.m), np.uint8)})["out"]

    def extract_batch(self, cw):
        """(B, blocks, m, m) code streams -> (B, blocks, m, k_b) message bits"""
        cw = self._bytes(cw, (self.blocks, self.m, self.m), "extract_batch")
        B = cw.shape[0]
        return cyclic._batch_call(_product_handle(self._sc()), "cc_staircase_extract_batch", [cw], B,
                                  {"msg": ((B, self.blocks, self.m, self.k_b), np.uint8)})["msg"]

    def correct_batch(self, z):
        """cc_staircase_decode: z (B, blocks, m, m) uint8 hard decisions -> (out, nflip, status) of the sliding-window
        decoder; numpy array or device tensor."""
        z = self._bytes(z, (self.blocks, self.m, self.m), "correct_batch")
        B = z.shape[0]
        side = _side(z)
        res = {"out": side.alloc(z, (B, self.blocks, self.m, self.m), np.uint8), "nflip": side.alloc(z, (B,), np.int32),
               "status": side.alloc(z, (B,), np.int32)}
        cyclic._batch_call(_product_handle(self._sc()), "cc_staircase_decode", [z], B, res)
        return res["out"], res["nflip"], res["status"]

    def decode_batch(self, z):
        """correct_batch, then the message bits of out: (msg, nflip, status)"""
        out, nflip, status = self.correct_batch(z)
        return self.extract_batch(out), nflip, status

    def correct_sr_batch(self, y, weights):
        """cc_staircase_decode_sr: y (B, blocks, m, m) float32 channel values -> dict(out=, nflip=, status=) of the
        sliding-window decoder with scaled reliability, weights[h] the threshold below which |y| yields to the component
        decoder in half-pass h of every window position (inf: always), 2 * iters of them; numpy array or device tensor."""
        fw = self._weights(weights)
        sc = self._sc()
        sc._keep = (self.code, fw)
        if len(y.shape) != 4 or tuple(y.shape[1:]) != (self.blocks, self.m, self.m):
            raise CcError(capi.ERR_LENGTH, "correct_sr_batch")
        yy = _side(y).as_type(y, "f", np.float32)
        if yy is None:
            raise TypeError("staircase decoding with scaled reliability takes float32 channel values")
        B = yy.shape[0]
        side = _side(yy)
        res = {"out": side.alloc(yy, (B, self.blocks, self.m, self.m), np.uint8), "nflip": side.alloc(yy, (B,), np.int32),
               "status": side.alloc(yy, (B,), np.int32)}
        cyclic._batch_call(_product_handle(sc), "cc_staircase_decode_sr", [yy], B, res, head=[fw])
        return res

    def decode_sr_batch(self, y, weights):
        """correct_sr_batch plus msg (B, blocks, m, k_b): the message bits of out"""
        res = self.correct_sr_batch(y, weights)
        res["msg"] = self.extract_batch(res["out"])
        return res

    def channel(self, ebno_db, seed, first_stream, streams, random_codewords=False, values=False):
        """Streams [first_stream, first_stream + streams) of the AWGN channel on the current device, as hard decisions
        (cc_awgn_staircase_dev): dict(z=, sent=) of (streams, blocks, m, m) uint8 torch tensors.  values=True: the channel
        values whose signs they are (cc_awgn_staircase_values_dev), dict(y= float32, sent=)."""
        import torch
        streams = int(streams)
        dev = torch.device("cuda", torch.cuda.current_device())
        shape = (streams, self.blocks, self.m, self.m)
        sent = torch.empty(shape, dtype=torch.uint8, device=dev)
        if values:
            y = torch.empty(shape, dtype=torch.float32, device=dev)
            rc = capi.lib().cc_awgn_staircase_values_dev(C.byref(self._sc()), float(ebno_db), int(seed), int(first_stream),
                                                         streams, int(bool(random_codewords)), _ptr(y), _ptr(sent),
                                                         _stream_handle(y))
            capi.check(rc, "cc_awgn_staircase_values_dev")
            return dict(y=y, sent=sent)
        z = torch.empty(shape, dtype=torch.uint8, device=dev)
        rc = capi.lib().cc_awgn_staircase_dev(C.byref(self._sc()), float(ebno_db), int(seed), int(first_stream), streams,
                                              int(bool(random_codewords)), _ptr(z), _ptr(sent), _stream_handle(z))
        capi.check(rc, "cc_awgn_staircase_dev")
        return dict(z=z, sent=sent)


class min_sum_decoder(cyclic):
    """The free functions min_sum<R, U>(H, y, tag) of soft_decision.h:220-295 bound to one parity-check matrix
    (any rows x cols 0/1 matrix, cols <= 2048; cc_minsum_create).  correct_batch(), correct(), H(), to_string()
    and kernel_info() work; there is no code to encode with."""

    def __init__(self, H, algorithm=None, stop_rule=capi.STOP_PARITY, device=None):
        algorithm = algorithm if algorithm is not None else min_sum_tag()
        if isinstance(algorithm, type):
            algorithm = algorithm()
        Hm = np.ascontiguousarray(H, np.uint8)
        if Hm.ndim != 2:
            raise ValueError("H must be a (rows, cols) matrix")
        self.algorithm = algorithm
        self.capability = None
        lib = capi.lib()
        d = capi.Desc()
        lib.cc_desc_init(C.byref(d))
        d.algorithm = algorithm.alg
        d.iterations = algorithm.iterations
        d.alpha, d.beta = float(algorithm.alpha), float(algorithm.beta)
        d.stop_rule = int(stop_rule)
        d.device = capi.DEVICE_CURRENT if device is None else int(device)
        self.wide = False
        self._desc = d
        h = C.c_void_p()
        capi.check(lib.cc_minsum_create(C.byref(d), _ptr(Hm), Hm.shape[0], Hm.shape[1], C.byref(h)),
                   "cc_minsum_create")
        self._h = h
        self.q = 0
        self.n, self.k, self.l = lib.cc_n(h), lib.cc_k(h), lib.cc_l(h)
        self.t, self.dmin, self.rate = 0, 0, lib.cc_rate(h)


def min_sum(H, y, tag=None, stop_rule=capi.STOP_PARITY):
    """min_sum<float, uint8_t>(H, y, tag): returns (b, L, iteration) like the reference's tuple and raises
    decoding_failure when no iteration satisfies the stop rule (soft_decision.h:199-201).  One frame per call;
    build a min_sum_decoder and use correct_batch for throughput."""
    dec = min_sum_decoder(H, tag, stop_rule)
    y = np.asarray(y, np.float32)
    if y.ndim != 1 or y.shape[0] != dec.n:
        raise CcError(capi.ERR_LENGTH, "min_sum")
    res = dec.correct_batch(y[None, :], want_L=True)
    if int(res["status"][0]) != capi.FRAME_OK:
        raise decoding_failure(cyclic._MESSAGES[capi.FRAME_NOT_CONVERGED])
    return res["out"][0], res["L"][0], int(res["iters"][0])

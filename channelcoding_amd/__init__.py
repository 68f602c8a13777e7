"""channelcoding_amd -- MI355X-native BCH / Reed-Solomon decoding (min-sum belief
propagation and the algebraic syndrome / Berlekamp-Massey / Chien / error-value
chain) behind the API surface of hannesweisbach/channelcoding.

The compute lives in libchannelcoding_amd.so (hand-written HIP for gfx950,
include/channelcoding_amd.h).  This package is the host-side mirror of the
reference's classes plus the torch.distributed Monte-Carlo harness.
"""
from . import _capi as capi
from ._capi import CcError
from .codes import (berlekamp_massey_tag, bsc_packed_channel, burst_channel, burst_erasure_channel, cyclic, decoding_failure, deinterleave, dmin, errors, euklid_tag, extend, interleave, min_sum, min_sum_decoder, min_sum_tag,
                    normalized_2d_min_sum_tag, normalized_min_sum_tag, offset_min_sum_tag, pack_bits,
                    peterson_gorenstein_zierler_tag, primitive_bch, product_code, product_decode, rs, self_correcting_1_min_sum_tag,
                    self_correcting_2_min_sum_tag, staircase_code, symbol_reliability, unextend, unpack_bits)

__all__ = [
    "capi", "CcError", "cyclic", "primitive_bch", "rs", "errors", "dmin", "decoding_failure",
    "peterson_gorenstein_zierler_tag", "berlekamp_massey_tag", "euklid_tag", "min_sum_tag",
    "normalized_min_sum_tag", "offset_min_sum_tag", "self_correcting_1_min_sum_tag",
    "self_correcting_2_min_sum_tag", "normalized_2d_min_sum_tag", "min_sum", "min_sum_decoder",
    "pack_bits", "unpack_bits", "interleave", "deinterleave", "burst_channel", "burst_erasure_channel",
    "bsc_packed_channel", "symbol_reliability", "product_decode", "extend", "unextend", "product_code",
    "staircase_code",
]

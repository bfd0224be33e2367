"""
The identity behind acc_to_frag<S, true> (csrc/fused_chain.h): the fused kernels convert an fp32 accumulator pair
to bf16 first and apply ReLU afterwards as the signed 16-bit maximum with 0 on the packed pair, instead of
max(x, 0) in fp32 followed by the conversion.  Both give the same 16 bits for every x that is not a NaN:

    bf16(max(x, 0)) == max_i16(bf16(x), 0)

because round-to-nearest-even never changes a sign, a negative bf16 (-0 included) has its sign bit set and is a
negative int16, and a non-negative bf16 is a non-negative int16.  (A NaN differs: the fp32 form turns it into 0, the
packed form keeps a positive NaN.  -0 becomes +0 under both.)

Exhaustive over the 16-bit side: every bf16 bit pattern b that is not a NaN, with fp32 inputs around every rounding
boundary of it.  The conversion is the oracle's (oracle.model.bf16_round).  No tolerance.
"""
import numpy as np
import torch

from oracle import model as OM


def _bf16_bits(x_bits: np.ndarray) -> np.ndarray:
    """bf16 bit pattern (as int16) of the fp32 values with bit patterns x_bits, by the oracle's rounding."""
    x = torch.from_numpy(x_bits.astype(np.uint32).view(np.float32).copy())
    r = OM.bf16_round(x).numpy().view(np.uint32)
    assert np.all((r & 0xFFFF) == 0), "bf16_round must return values that are exact in bf16"
    return (r >> 16).astype(np.uint16).view(np.int16)


def _relu_then_convert(x_bits: np.ndarray) -> np.ndarray:
    x = x_bits.astype(np.uint32).view(np.float32)
    y = np.where(x > 0, x, np.float32(0.0)).astype(np.float32)  # max(x, 0); -0 and every negative give +0
    return _bf16_bits(y.view(np.uint32))


def _convert_then_max_i16(x_bits: np.ndarray) -> np.ndarray:
    return np.maximum(_bf16_bits(x_bits), np.int16(0))


def _not_nan(bits: np.ndarray) -> np.ndarray:
    return (bits & 0x7FFFFFFF) <= 0x7F800000


def _inputs() -> np.ndarray:
    b = np.arange(1 << 16, dtype=np.int64)
    b = b[(b & 0x7FFF) <= 0x7F80]  # every bf16 that is not a NaN (+-inf included)
    wide = b << 16
    sign = wide & 0x80000000
    cols = [wide]
    # the two rounding midpoints of b (towards the next bf16 of larger and of smaller magnitude), each with its two
    # fp32 neighbours and the tie itself
    for mid in (wide + 0x8000, wide - 0x8000):
        for d in (-1, 0, 1):
            v = mid + d
            ok = ((v & 0x80000000) == sign) & (v >= 0) & (v <= 0xFFFFFFFF)  # stayed on b's side of zero
            cols.append(v[ok])
    special = np.array([0x00000000, 0x80000000,                          # +-0
                        0x00000001, 0x80000001, 0x00000002, 0x80000002,  # smallest denormals
                        0x00007FFF, 0x80007FFF, 0x00008000, 0x80008000, 0x00008001, 0x80008001,  # around bf16's first tie
                        0x00400000, 0x80400000, 0x007FFFFF, 0x807FFFFF,  # large denormals
                        0x00800000, 0x80800000,                          # smallest normals
                        0x7F7FFFFF, 0xFF7FFFFF,                          # largest finite (rounds to inf in bf16)
                        0x7F800000, 0xFF800000], dtype=np.int64)         # +-inf
    cols.append(special)
    x = np.unique(np.concatenate(cols))
    x = x[_not_nan(x)]
    return x.astype(np.uint32)


def test_inputs_cover_every_non_nan_bf16():
    x = _inputs()
    got = np.unique(_bf16_bits(x).view(np.uint16))
    want = np.array([b for b in range(1 << 16) if (b & 0x7FFF) <= 0x7F80], dtype=np.uint16)
    assert np.array_equal(got, want)
    # per b: the widened value and the three values around each midpoint; a midpoint is shared by two neighbouring b
    assert x.size > 3 * want.size


def test_relu_commutes_with_bf16_rounding_bit_for_bit():
    x = _inputs()
    a = _relu_then_convert(x)
    b = _convert_then_max_i16(x)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, [(hex(int(x[i])), hex(int(a[i]) & 0xFFFF), hex(int(b[i]) & 0xFFFF)) for i in bad[:8]]


def test_relu_mask_agrees():
    # the ReLU mask the saving forward writes is "bf16 output != 0": the same under both forms, -0 never appears
    x = _inputs()
    b = _convert_then_max_i16(x)
    assert np.all(b >= 0)
    assert np.array_equal(b != 0, _relu_then_convert(x) != 0)

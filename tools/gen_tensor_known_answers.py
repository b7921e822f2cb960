"""Derives tests/golden/tensor_out_known_answers.json: (u, scale, bias, dtype) -> bits of the tensor element that
include/h263mi.h defines (h263mi_tensor_out), in exact rational arithmetic -- no floating-point operation of the machine takes
part, so neither numpy's nor the library's rounding can leak into the answers.

    python tools/gen_tensor_known_answers.py > tests/golden/tensor_out_known_answers.json

round_to(x, p, emin, emax): the IEEE round-to-nearest-even of the rational x into a binary format with p significand bits,
smallest normal exponent emin and largest emax -- subnormals kept, overflow to infinity.  The cases are chosen by hand (ties in
both directions, subnormals, overflow); the triples on which a fused multiply-add would differ are found by a search over a
fixed list of scale / bias pairs, and each carries the bits a fused evaluation would have given, as data."""
import json
import struct
from fractions import Fraction

FORMATS = {"f32": (24, -126, 127, 8), "f16": (11, -14, 15, 5), "bf16": (8, -126, 127, 8)}


def round_to(x, p, emin, emax):
    """-> (sign, rational value or 'inf')"""
    sign = x < 0
    x = abs(x)
    if x == 0:
        return sign, Fraction(0)
    e = 0
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    while Fraction(2) ** e > x:
        e -= 1
    e = max(e, emin)
    ulp = Fraction(2) ** (e - (p - 1))
    q, r = divmod(x, ulp)
    q = int(q)
    if r * 2 > ulp or (r * 2 == ulp and q & 1):
        q += 1
    v = q * ulp
    if v >= Fraction(2) ** (emax + 1):
        return sign, "inf"
    return sign, v


def bits_of(sign, v, fmt):
    p, emin, emax, ebits = FORMATS[fmt]
    s = (1 << (ebits + p - 1)) if sign else 0
    if v == "inf":
        return s | (((1 << ebits) - 1) << (p - 1))
    if v == 0:
        return s
    if v < Fraction(2) ** emin:
        return s | int(v / Fraction(2) ** (emin - (p - 1)))
    e = emin
    while Fraction(2) ** (e + 1) <= v:
        e += 1
    m = int(v / Fraction(2) ** (e - (p - 1))) - (1 << (p - 1))
    return s | ((e - emin + 1) << (p - 1)) | m


def f32_value(bits):
    """the rational value of binary32 bits (finite)"""
    s, e, m = bits >> 31, (bits >> 23) & 0xff, bits & 0x7fffff
    v = Fraction(m, 1 << 23) * Fraction(2) ** -126 if e == 0 else (1 + Fraction(m, 1 << 23)) * Fraction(2) ** (e - 127)
    return -v if s else v


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def element(u, scale_bits, bias_bits, dtype):
    """-> (bits of the element, binary32 bits of a FUSED evaluation)"""
    s, b = f32_value(scale_bits), f32_value(bias_bits)
    s_neg, b_neg = scale_bits >> 31 == 1, bias_bits >> 31 == 1
    # the product: its sign is the scale's (u >= 0), also where it is zero
    _, m = round_to(abs(u * s), 24, -126, 127)
    if m == "inf":
        v32 = (s_neg, "inf")
    else:
        total = (-m if s_neg else m) + b
        if total == 0:
            # an exact zero: -0 only when both terms are negative (zeros); opposite terms cancel to +0 under round to nearest
            v32 = (s_neg and b_neg, Fraction(0))
        else:
            v32 = round_to(total, 24, -126, 127)
    fused = round_to(u * s + b, 24, -126, 127)
    if u * s + b == 0:
        fused = (s_neg and b_neg, Fraction(0))
    if dtype == "f32":
        out = bits_of(v32[0], v32[1], "f32")
    else:
        p, emin, emax, _ = FORMATS[dtype]
        if v32[1] == "inf":
            out = bits_of(v32[0], "inf", dtype)
        else:
            r = round_to(-v32[1] if v32[0] else v32[1], p, emin, emax)
            out = bits_of(v32[0], r[1], dtype)
    return out, bits_of(fused[0], fused[1], "f32")


def case(name, u, scale, bias, dtype, why):
    sb = scale if isinstance(scale, int) else f32_bits(scale)
    bb = bias if isinstance(bias, int) else f32_bits(bias)
    bits, fused = element(u, sb, bb, dtype)
    return {"name": name, "u": u, "scale_bits": "0x%08x" % sb, "bias_bits": "0x%08x" % bb, "dtype": dtype,
            "bits": "0x%0*x" % (8 if dtype == "f32" else 4, bits), "fused_f32_bits": "0x%08x" % fused, "why": why}


def main():
    cases = [
        case("f16_tie_down_to_even", 1, 1.0, 2.0 ** -11, "f16", "1 + 2^-11 lies halfway between 0x3c00 and 0x3c01: even is 0x3c00"),
        case("f16_tie_up_to_even", 1, 1.0, 3 * 2.0 ** -11, "f16", "1 + 3*2^-11 lies halfway between 0x3c01 and 0x3c02: even is 0x3c02"),
        case("bf16_tie_down_to_even", 1, 1.0, 2.0 ** -8, "bf16", "1 + 2^-8 lies halfway between 0x3f80 and 0x3f81: even is 0x3f80"),
        case("bf16_tie_up_to_even", 1, 1.0, 3 * 2.0 ** -8, "bf16", "1 + 3*2^-8 lies halfway between 0x3f81 and 0x3f82: even is 0x3f82"),
        case("f16_subnormal", 3, 2.0 ** -24, 0.0, "f16", "3 * 2^-24: three units of the smallest binary16 subnormal"),
        case("f16_subnormal_tie", 5, 2.0 ** -25, 0.0, "f16", "2.5 units of 2^-24: ties to even, 2"),
        case("f16_subnormal_rounds_to_normal", 255, 0x36808081, 0.0, "f16", "255 * (2^-14 / 255 rounded up) just reaches the smallest normal"),
        case("bf16_subnormal", 3, 0x00010000, 0.0, "bf16", "3 * 2^-133, a binary32 subnormal 0x00030000: bfloat16 subnormal 0x0003"),
        case("bf16_subnormal_tie", 3, 0x00008000, 0.0, "bf16", "0x00018000 lies halfway between 0x0001 and 0x0002: even is 0x0002"),
        case("f32_subnormal", 255, 0x00000001, 0.0, "f32", "255 * 2^-149: binary32 bits 0x000000ff, kept"),
        case("f32_subnormal_sum", 200, 0x00000003, 0x80000064, "f32", "600 * 2^-149 - 100 * 2^-149 = 500 units, exact"),
        case("f16_overflow", 255, 257.0, 0.0, "f16", "65535 >= 65520, the halfway point above the largest binary16 65504: +inf"),
        case("f16_overflow_negative", 255, -257.0, 0.0, "f16", "-65535: -inf"),
        case("f16_below_overflow", 1, 65519.0, 0.0, "f16", "65519 < 65520: the largest finite binary16, 0x7bff"),
        case("f16_overflow_at_tie", 1, 65520.0, 0.0, "f16", "65520 ties between 65504 (odd significand) and 2^16: to even, +inf"),
        case("bf16_overflow", 255, 0x7f000000, 0x7f000000, "bf16", "255 * 2^127 overflows binary32 already: +inf"),
        case("bf16_rounds_to_inf", 1, 0x7f7fffff, 0.0, "bf16", "the largest binary32 rounds up past the largest bfloat16: +inf"),
        case("imagenet_red_255", 255, f32_bits(1 / (255 * 0.229)), f32_bits(-0.485 / 0.229), "f32", "ImageNet red, u = 255"),
        case("zero_times_negative_scale", 0, -1.0, 0.0, "f32", "0 * -1 = -0, and -0 + +0 = +0 under round to nearest"),
        case("minus_zero_kept", 0, -1.0, 0x80000000, "f16", "-0 + -0 = -0"),
    ]
    # triples on which one rounding (a fused multiply-add) gives another binary32 than two: searched, kept as data
    pairs = [(1 / (255 * 0.229), -0.485 / 0.229), (1 / (255 * 0.224), -0.456 / 0.224), (1 / (255 * 0.225), -0.406 / 0.225),
             (1 / 127.5, -1.0), (0.1, 0.7)]
    found = 0
    for k, (s, b) in enumerate(pairs):
        per_pair = 0
        for u in range(256):
            bits, fused = element(u, f32_bits(s), f32_bits(b), "f32")
            if bits != fused and per_pair < 2:
                cases.append(case("fused_would_differ_%d_%d" % (k, u), u, s, b, "f32",
                                  "two roundings give %#010x, one rounding (fma) %#010x" % (bits, fused)))
                per_pair += 1
                found += 1
    assert found >= 1
    print(json.dumps({"comment": "tools/gen_tensor_known_answers.py: exact rational arithmetic; scale, bias and the f32 answers as "
                                 "binary32 bits, the 16-bit answers as binary16 / bfloat16 bits", "cases": cases}, indent=1))


if __name__ == "__main__":
    main()

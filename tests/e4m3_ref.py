"""TEST INFRASTRUCTURE: OCP e4m3 ("e4m3fn") stated from the format definition, in float64 and without torch.float8_e4m3fn.

A byte is sign (1 bit) | exponent (4 bits, bias 7) | mantissa (3 bits):
    exponent 0       subnormal, value m * 2^-9
    exponent 1..15   (1 + m / 8) * 2^(exponent - 7)
    0x7F / 0xFF      NaN (there are no infinities); the largest finite value is 0x7E = 1.75 * 2^8 = 448.
`encode` is the conversion every operand producer of the library promises: clamp to +-448, round to nearest, ties to even, sign kept
(-0 included), NaN -> a NaN code.  Everything runs on the device of its argument, so the GPU tests keep large references there.
"""
import torch

MAX = 448.0
NAN_CODES = (0x7F, 0xFF)


def _value(code: int) -> float:
    e, m = (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return float("nan")
    mag = m * 2.0 ** -9 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return -mag if code & 0x80 else mag


DECODE = torch.tensor([_value(c) for c in range(256)], dtype=torch.float64)          # value of every byte
MAGS = DECODE[:127].clone()                                                          # the 127 finite magnitudes, ascending: code == index
MIDS = (MAGS[:-1] + MAGS[1:]) / 2                                                    # the 126 midpoints between adjacent codes (exact)
assert float(MAGS[126]) == MAX and bool((MAGS[1:] > MAGS[:-1]).all())

_cache = {}


def _on(t: torch.Tensor, device) -> torch.Tensor:
    key = (id(t), str(device))
    if key not in _cache:
        _cache[key] = t.to(device)
    return _cache[key]


def decode(b: torch.Tensor) -> torch.Tensor:
    """uint8 -> float64 value (NaN codes -> NaN)"""
    return _on(DECODE, b.device)[b.long()]


def is_nan_code(b: torch.Tensor) -> torch.Tensor:
    return (b & 0x7F) == 0x7F


def _bracket(x64: torch.Tensor):
    """clamped magnitude a and the adjacent codes lo <= hi with MAGS[lo] <= a <= MAGS[hi] (lo == hi only at 0), NaN treated as 0"""
    assert x64.dtype == torch.float64
    mags = _on(MAGS, x64.device)
    a = torch.nan_to_num(x64.abs(), nan=0.0, posinf=MAX).clamp(max=MAX)
    hi = torch.searchsorted(mags, a.contiguous()).clamp(max=126)
    lo = (hi - 1).clamp(min=0)
    return a, lo, hi, (mags[lo] + mags[hi]) / 2


def encode(x64: torch.Tensor) -> torch.Tensor:
    """float64 -> e4m3 byte (uint8): round to nearest, ties to even, on the magnitude table"""
    a, lo, hi, mid = _bracket(x64)
    even = torch.where(lo % 2 == 0, lo, hi)
    code = torch.where(a < mid, lo, torch.where(a > mid, hi, even))
    code = torch.where(torch.isnan(x64), torch.full_like(code, 0x7F), code)
    return (code + 128 * torch.signbit(x64).long()).to(torch.uint8)


def encode_truncate(x64: torch.Tensor) -> torch.Tensor:
    """A deliberately WRONG encoder (round towards zero) for the tests that check that the assertions bite."""
    a, lo, hi, _ = _bracket(x64)
    mags = _on(MAGS, x64.device)
    code = torch.where(a >= mags[hi], hi, lo)
    code = torch.where(torch.isnan(x64), torch.full_like(code, 0x7F), code)
    return (code + 128 * torch.signbit(x64).long()).to(torch.uint8)


def near_midpoint_abs(x64: torch.Tensor, margin: torch.Tensor):
    """(mask, byte_lo, byte_hi): inputs whose clamped magnitude lies within `margin` (a tensor, absolute) of the midpoint between two
    adjacent finite codes, and the two bytes admissible there.  A non-zero input within `margin` of zero has no decided sign: the two zeros."""
    a, lo, hi, mid = _bracket(x64)
    s = 128 * torch.signbit(x64).long()
    mask = ((a - mid).abs() <= margin) & (lo != hi) & ~torch.isnan(x64)
    zero = (a <= margin) & (a > 0) & ~torch.isnan(x64)
    blo = torch.where(zero, torch.zeros_like(lo), lo + s)
    bhi = torch.where(zero, torch.full_like(hi, 128), hi + s)
    return mask | zero, blo.to(torch.uint8), bhi.to(torch.uint8)


def near_midpoint(x64: torch.Tensor, rel: float):
    """near_midpoint_abs with the margin rel * |x|"""
    return near_midpoint_abs(x64, rel * torch.nan_to_num(x64.abs(), nan=0.0, posinf=MAX))


def spacing(x64: torch.Tensor) -> torch.Tensor:
    """distance between adjacent e4m3 codes at magnitude |x| (clamped to the finite range)"""
    a = x64.abs().clamp(min=2.0 ** -6, max=MAX)
    return torch.exp2(torch.floor(torch.log2(a)) - 3)

"""TEST INFRASTRUCTURE: CRC-32 from its definition, written without looking at csrc/crc32_core.h.

The message, its first 32 bits complemented, is a polynomial over GF(2) with the first bit of the first byte (its least significant
one) as the highest power; it is multiplied by x^32 and divided by P = x^32 + x^26 + x^23 + x^22 + x^16 + x^12 + x^11 + x^10 + x^8 + x^7 +
x^5 + x^4 + x^2 + x + 1; the remainder, complemented, is the CRC.  In a register that holds the coefficient of x^31 in bit 0 ("reflected")
P's low 32 coefficients read 0xEDB88320, and one message bit is: XOR it into bit 0, shift right, XOR 0xEDB88320 if a one fell out.
`crc_bitwise` is that loop.  `combine` is the identity crc(A + B) = crc(A) x^(8 |B|) + crc(B) (mod P), which holds because the
complemented head of B and the complement at the end of crc(A) cancel; `crc` uses it to run the bit loop over many chunks of a long
message in lockstep (numpy), so that a mebibyte takes a fraction of a second.  An empty message gives 0."""
from __future__ import annotations

import numpy as np

P = 0xEDB88320


def crc_bitwise(data: bytes) -> int:
    if not data:
        return 0
    r = 0xFFFFFFFF
    for byte in data:
        for k in range(8):
            bit = (r ^ (byte >> k)) & 1
            r >>= 1
            if bit:
                r ^= P
    return r ^ 0xFFFFFFFF


def times_x(a: int) -> int:
    """a(x) x mod P; bit 31 of a word is the coefficient of x^0."""
    return (a >> 1) ^ (P if a & 1 else 0)


def mul(a: int, b: int) -> int:
    """a(x) b(x) mod P: for every power x^i in a (bit 31 - i), add b x^i."""
    out = 0
    for i in range(32):
        if (a >> (31 - i)) & 1:
            out ^= b
        b = times_x(b)
    return out


def x_to(n: int) -> int:
    """x^n mod P by square and multiply."""
    out, base = 1 << 31, 1 << 30
    while n:
        if n & 1:
            out = mul(out, base)
        base = mul(base, base)
        n >>= 1
    return out


def combine(crc_a: int, crc_b: int, len_b: int) -> int:
    return mul(x_to(8 * len_b), crc_a) ^ crc_b


def crc(data: bytes, chunk: int = 1024) -> int:
    """crc_bitwise(data), with the whole chunks of a long message run through the bit loop side by side and joined by `combine`."""
    n = len(data) // chunk
    if n < 4:
        return crc_bitwise(data)
    a = np.frombuffer(data, np.uint8, n * chunk).reshape(n, chunk).astype(np.uint32)
    r = np.full(n, 0xFFFFFFFF, np.uint32)
    poly = np.uint32(P)
    for j in range(chunk):
        r ^= a[:, j]
        for _ in range(8):
            r = (r >> np.uint32(1)) ^ (poly * (r & np.uint32(1)))
    r ^= np.uint32(0xFFFFFFFF)
    shift = x_to(8 * chunk)
    out = 0
    for v in r.tolist():
        out = mul(shift, out) ^ v
    tail = data[n * chunk:]
    return combine(out, crc_bitwise(tail), len(tail))

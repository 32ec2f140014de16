"""Raw deflate members, intact and damaged in named ways, for the device BGZF inflater (k_inflate_bgzf): shared by the
CPU check of its decoder core and the GPU tests.  A member here is the deflate payload followed by the gzip trailer
(CRC-32, ISIZE); bgzf_wrap puts BGZF headers around a list of them."""
import struct
import zlib

# the decoder's status words (F2Q_INF_* in 2fast2q_amd/csrc/f2q_inflate_kernels.h)
OK, OVERRUN, BAD_BLOCK, BAD_CODE, DIST_FAR, OUT_OVERFLOW, ISIZE, CRC, TRAILING = range(9)


class Bits:
    """LSB-first bit writer (RFC 1951 3.1.1); huff() writes a Huffman code MSB-first"""
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val, n):
        self.v |= val << self.n
        self.n += n
        return self

    def huff(self, code, n):
        return self.put(int(format(code, f"0{n}b")[::-1], 2), n)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def trailer(text, crc=None, isize=None):
    return struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc, len(text) if isize is None else isize)


def deflate_raw(text, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(text) + co.flush()


def member(text, level=6):
    return deflate_raw(text, level) + trailer(text)


def damaged(text):
    """{name: (member bytes, expected status)}: every way the issue names, plus a flipped payload byte (status not fixed)"""
    body = deflate_raw(text)
    crc = zlib.crc32(text) & 0xFFFFFFFF
    flip = bytearray(body)
    flip[len(flip) // 2] ^= 0x5A
    # fixed block: literal 'A', then length 3 at distance 2 -- one byte before the member's start
    far = Bits().put(1, 1).put(1, 2).huff(0x30 + 65, 8).huff(1, 7).huff(1, 5).huff(0, 7).bytes()
    # dynamic block whose code-length code has four codes of length 1: over-subscribed
    oversub = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(1, 3).put(1, 3).put(1, 3).bytes()
    return {
        "flipped_payload_byte": (bytes(flip) + trailer(text), None),
        "wrong_crc": (body + trailer(text, crc=crc ^ 0x10), CRC),
        "isize_above": (body + trailer(text, isize=len(text) + 1), ISIZE),
        "isize_below": (body + trailer(text, isize=len(text) - 1), ISIZE),
        "block_type_3": (b"\x07" + trailer(b""), BAD_BLOCK),
        "oversubscribed_lengths": (oversub + trailer(b"AAAA"), BAD_CODE),
        "distance_before_start": (far + trailer(b"AAAA"), DIST_FAR),
        "bytes_before_trailer": (body + b"\x00" + trailer(text), TRAILING),
    }


def bgzf_wrap(members, pad=None):
    """BGZF headers ('BC' subfield = member size - 1) around raw members (payload + trailer).  pad (0..3, or one per
    member): an extra subfield 'PD' of that many bytes in front of 'BC', which shifts the payload by 4 + pad bytes"""
    out = bytearray()
    pads = pad if isinstance(pad, (list, tuple)) else [pad] * len(members)
    for m, k in zip(members, pads):
        extra = b"" if k is None else b"PD" + struct.pack("<H", k) + b"\0" * k
        bsize = 18 + len(extra) + len(m)
        out += b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", 6 + len(extra)) + extra + b"BC" + struct.pack("<HH", 2, bsize - 1) + m
    return bytes(out)

"""A DEFLATE (RFC 1951) writer for tests: streams that zlib's encoder never writes, for the three inflaters of the
ingest path (k_inflate_bgzf, f2qz::Inflater, the parallel gunzip).  Plain Python.  A stream is written block by block
from tokens -- ('L', byte) and ('M', length, distance) -- with every choice an encoder has left open: stored, fixed
and dynamic blocks in any order, explicit code lengths on both tables, the run-length coding of a dynamic header, 258
written as symbol 284 + 31.  zlib is the reference throughout: every member this module hands out has been decoded
by zlib.decompressobj(-15) and compared with its text.

scan() reads a member back, independently of the writer, and reports what is in it (block types and where their
headers lie, code lengths the tokens used, header repeat codes, (distance, length) pairs): the tests assert their
preconditions from it.

A member is the deflate payload followed by the gzip trailer (CRC-32, ISIZE), as in inflate_cases."""
import base64
import functools
import hashlib
import json
import os
import random
import struct
import zlib

import inflate_cases as IC
from inflate_cases import Bits

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
FOREIGN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foreign_deflate.json")


class ByteBits:
    """Bits with the whole bytes flushed as they fill: linear where the big-int writer is quadratic"""
    def __init__(self):
        self.out, self.v, self.k, self.n = bytearray(), 0, 0, 0

    def put(self, val, n):
        self.v |= val << self.k
        self.k += n
        self.n += n
        if self.k >= 8:
            nb = self.k >> 3
            self.out += (self.v & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
            self.v >>= 8 * nb
            self.k -= 8 * nb
        return self

    def huff(self, code, n):
        return self.put(int(format(code, f"0{n}b")[::-1], 2), n)

    def raw(self, data):
        assert self.k == 0
        self.out += data
        self.n += 8 * len(data)
        return self

    def bytes(self):
        return bytes(self.out) + (bytes([self.v]) if self.k else b"")


def canon(lens):
    """code lengths per symbol -> {symbol: (canonical code, length)} (RFC 1951 3.2.2)"""
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def len_sym(n, p284=False):
    """(symbol, extra-bit value, extra bits) of a match length; p284: 258 as symbol 284 with extra bits 31"""
    if n == 258 and p284:
        return 284, 31, 5
    k = max(k for k in range(29) if LBASE[k] <= n)
    return 257 + k, n - LBASE[k], LEXT[k]


def dist_sym(d):
    k = max(k for k in range(30) if DBASE[k] <= d)
    return k, d - DBASE[k], DEXT[k]


def apply_tokens(o, tokens):
    """append the text of the tokens to the bytearray o, whose bytes the distances may reach back into"""
    for t in tokens:
        if t[0] == "L":
            o.append(t[1])
            continue
        _, n, d = t
        s = len(o) - d
        assert s >= 0 and 3 <= n <= 258 and d <= 32768, t
        if d >= n:
            o += o[s:s + n]
        else:
            for k in range(n):
                o.append(o[s + k])


def tokens_text(tokens, prefix=b""):
    """the text the tokens stand for, after `prefix`"""
    o = bytearray(prefix)
    apply_tokens(o, tokens)
    return bytes(o[len(prefix):])


def ladder(symbols):
    """16 symbols -> {symbol: length} with lengths 1, 2, ..., 14, 15, 15: complete, the longest codes 15 bits"""
    assert len(symbols) == 16 and len(set(symbols)) == 16
    return {s: (i + 1 if i < 15 else 15) for i, s in enumerate(symbols)}


def ladder_over(symbols, spare):
    """any number of symbols (the most frequent first) -> {symbol: length}, complete and 15 bits deep: the last 15 take
    the ladder 2, 3, ..., 14, 15, 15, the others a balanced code behind a 1-bit prefix.  Fewer than 17 symbols are
    filled up from `spare` (symbols that get a code and are never sent)."""
    symbols = list(symbols) + [s for s in spare if s not in symbols][:max(0, 17 - len(symbols))]
    head, tail = symbols[:-15], symbols[-15:]
    k = len(head).bit_length() - 1
    short = (1 << (k + 1)) - len(head)
    out = {s: 1 + (k if i < short else k + 1) for i, s in enumerate(head)}
    out.update({s: (i + 2 if i < 14 else 15) for i, s in enumerate(tail)})
    return out


def lens_list(mapping, n):
    out = [0] * n
    for s, l in mapping.items():
        out[s] = l
    return out


def _zero_chunks(n):
    """n >= 3 zeros as runs of 3..138 (symbols 17 and 18)"""
    out = []
    while n:
        r = min(n, 138)
        if 0 < n - r < 3:
            r -= 3 - (n - r)
        out.append(r)
        n -= r
    return out


def header_ops(seq, zero_run=None):
    """The code lengths of both tables as one sequence -> code-length symbols [(symbol, extra value, extra bits)].  Runs
    are coded wherever they are, the border between the two tables included.  zero_run: None codes a run of zeros with
    17 / 18 alone; '18,16' ends it with a 16 (a repeat of the zero that a 17 or 18 left as the previous length); '0,16'
    writes it as a literal 0 and 16s."""
    ops, i = [], 0
    zop = lambda r: (17, r - 3, 3) if r <= 10 else (18, r - 11, 7)
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and zero_run == "18,16" and run >= 6:
            t = min(6, run - 3)
            ops += [zop(r) for r in _zero_chunks(run - t)] + [(16, t - 3, 2)]
        elif v == 0 and zero_run != "0,16" and run >= 3:
            ops += [zop(r) for r in _zero_chunks(run)]
        elif run >= 4:
            ops.append((v, 0, 0))
            rest = run - 1
            while rest >= 3:
                r = min(rest, 6)
                ops.append((16, r - 3, 2))
                rest -= r
            ops += [(v, 0, 0)] * rest
        else:
            ops += [(v, 0, 0)] * run
        i = j
    return ops


class Deflate:
    """one deflate stream, written block by block; .text is what it stands for so far"""
    def __init__(self, bits=None):
        self.b = bits if bits is not None else Bits()
        self.text = bytearray()
        self.block_bytes = []                  # byte offset of each block's header (of the byte that holds its first bit)

    def _head(self, last, btype):
        self.block_bytes.append(self.b.n // 8)
        self.b.put(1 if last else 0, 1).put(btype, 2)

    def _tokens(self, tokens, lc, dc, p284):
        b = self.b
        for t in tokens:
            if t[0] == "L":
                b.huff(*lc[t[1]])
            else:
                s, x, nb = len_sym(t[1], p284)
                b.huff(*lc[s]).put(x, nb)
                s, x, nb = dist_sym(t[2])
                b.huff(*dc[s]).put(x, nb)
        b.huff(*lc[256])
        apply_tokens(self.text, tokens)

    def stored(self, data, last=False):
        b = self.b
        self._head(last, 0)
        if b.n % 8:
            b.put(0, 8 - b.n % 8)
        b.put(len(data), 16).put(len(data) ^ 0xFFFF, 16)
        if hasattr(b, "raw"):
            b.raw(data)
        else:
            b.put(int.from_bytes(data, "little"), 8 * len(data))
        self.text += data
        return self

    def fixed(self, tokens, last=False, p284=False):
        self._head(last, 1)
        self._tokens(tokens, canon(FIXED_LL), canon(FIXED_DL), p284)
        return self

    def dynamic_header(self, ll, dl, last=False, zero_run=None, nlen=None, ndist=None):
        """block header and the two sets of code lengths (ll: up to 286 litlen lengths, dl: up to 30 distance lengths);
        nlen / ndist send more lengths than the last used symbol needs"""
        b = self.b
        nlen = max(257, max([i + 1 for i, l in enumerate(ll) if l] + [0]), nlen or 0)
        ndist = max(1, max([i + 1 for i, l in enumerate(dl) if l] + [0]), ndist or 0)
        assert nlen <= 286 and ndist <= 30
        seq = (list(ll) + [0] * 286)[:nlen] + (list(dl) + [0] * 30)[:ndist]
        ops = header_ops(seq, zero_run)
        used = sorted({s for s, _, _ in ops})
        if len(used) == 1:
            used.append((used[0] + 1) % 19)
        k = len(used).bit_length() - 1                     # a complete code-length code: k bits, or k + 1
        short = (1 << (k + 1)) - len(used)
        cll = [0] * 19
        for i, s in enumerate(used):
            cll[s] = k if i < short else k + 1
        cc = canon(cll)
        ncl = max(4, max(i for i, s in enumerate(CL_ORDER) if cll[s]) + 1)
        self._head(last, 2)
        b.put(nlen - 257, 5).put(ndist - 1, 5).put(ncl - 4, 4)
        for s in CL_ORDER[:ncl]:
            b.put(cll[s], 3)
        for s, x, nb in ops:
            b.huff(*cc[s]).put(x, nb)
        return self

    def dynamic(self, tokens, ll, dl, last=False, p284=False, **header):
        self.dynamic_header(ll, dl, last, **header)
        self._tokens(tokens, canon(ll), canon(dl), p284)
        return self

    def payload(self):
        return self.b.bytes()

    def member(self):
        """(payload + trailer, text), once zlib has read the payload back as that text"""
        raw, text = self.payload(), bytes(self.text)
        z = zlib.decompressobj(-15)
        assert z.decompress(raw) == text and z.eof and not z.unused_data
        return raw + IC.trailer(text), text


def zlib_rejects(member):
    try:
        z = zlib.decompressobj(-15)
        t = z.decompress(member[:-8])
        return not z.eof or z.unused_data != b"" or IC.trailer(t) != member[-8:]
    except zlib.error:
        return True


# ---- reading a member back ------------------------------------------------------------------------------------------
def scan(member):
    """What a member holds, read from its bytes: a bit-by-bit inflate that keeps notes.
      types          block types in order           header_bytes   byte offset of each block header
      llens, dlens   code lengths of the litlen / distance codes that tokens used
      l284_31        258 came as symbol 284 + 31
      rep16_after    the code-length symbols that a 16 followed (17 / 18: a repeat of zero)
      straddle       the repeat symbols whose run crosses from the litlen lengths into the distance lengths
      single_dist, no_dist   a block had one distance code of length 1 / none
      pairs          (distance, length) of every match;    text   the bytes"""
    data = member[:-8]
    v, pos = int.from_bytes(data, "little"), 0
    f = dict(types=[], header_bytes=[], llens=set(), dlens=set(), l284_31=False, rep16_after=set(), straddle=set(), single_dist=False,
             no_dist=False, pairs=set())
    out = bytearray()

    def take(n):
        nonlocal pos
        x = (v >> pos) & ((1 << n) - 1)
        pos += n
        return x

    def sym(tab):
        nonlocal pos
        p, code = (v >> pos) & 0x7FFF, 0
        for L in range(1, 16):
            code = (code << 1) | ((p >> (L - 1)) & 1)
            s = tab.get((L, code))
            if s is not None:
                pos += L
                return s, L
        raise ValueError("no such code")

    table = lambda lens: {(l, c): s for s, (c, l) in canon(lens).items()}
    last = 0
    while not last:
        f["header_bytes"].append(pos // 8)
        last, t = take(1), take(2)
        f["types"].append(t)
        if t == 0:
            pos = (pos + 7) // 8 * 8
            n, nn = take(16), take(16)
            assert n == nn ^ 0xFFFF
            out += data[pos // 8:pos // 8 + n]
            pos += 8 * n
            continue
        assert t != 3
        if t == 1:
            ll, dl = FIXED_LL, FIXED_DL
        else:
            nlen, ndist, ncl = take(5) + 257, take(5) + 1, take(4) + 4
            cll = [0] * 19
            for s in CL_ORDER[:ncl]:
                cll[s] = take(3)
            ct, seq, prev_op = table(cll), [], None
            while len(seq) < nlen + ndist:
                s, _ = sym(ct)
                if s < 16:
                    seq.append(s)
                else:
                    rep = 3 + take(2) if s == 16 else 3 + take(3) if s == 17 else 11 + take(7)
                    if s == 16:
                        f["rep16_after"].add(prev_op)
                    if len(seq) < nlen < len(seq) + rep:
                        f["straddle"].add(s)
                    seq += [seq[-1] if s == 16 else 0] * rep
                prev_op = s
            assert len(seq) == nlen + ndist
            ll, dl = seq[:nlen], seq[nlen:]
            used = [l for l in dl if l]
            f["single_dist"] |= used == [1]
            f["no_dist"] |= not used
        lt, dt = table(ll), table(dl)
        while True:
            s, L = sym(lt)
            f["llens"].add(L)
            if s < 256:
                out.append(s)
                continue
            if s == 256:
                break
            x = take(LEXT[s - 257])
            n = LBASE[s - 257] + x
            f["l284_31"] |= s == 284 and x == 31
            s, L = sym(dt)
            f["dlens"].add(L)
            d = DBASE[s] + take(DEXT[s])
            f["pairs"].add((d, n))
            apply_tokens(out, [("M", n, d)])
    assert (pos + 7) // 8 == len(data)
    f["text"] = bytes(out)
    return f


# ---- the families: {name: (member, text)} ---------------------------------------------------------------------------
LADDER_LENGTHS = [3, 4, 11, 19, 115, 227, 257, 258]
LADDER_DISTANCES = [1, 2, 3, 4, 5, 8, 33, 49, 64, 65, 97, 129, 193, 257, 1025, 8193, 16385, 24577, 32767, 32768]
LADDER_LITS = list(b"ACGT\nIF@")
# 8 literals, end-of-block and the 7 length symbols of LADDER_LENGTHS; the distance symbols of LADDER_DISTANCES are 17,
# so each order leaves one of them out (193 / 129), and the one it keeps of the two sits behind the 8-bit root
# (position i of a ladder has length i + 1: the first six litlen symbols lie behind the 10-bit root in the reversed order,
# the last six in this one; the four literals in between never do)
LADDER_LSYMS = [257, 265, 284, 256, 65, 67] + [10, 73, 70, 64] + [71, 84, 258, 269, 280, 285]
LADDER_DSYMS = ([0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 15, 16, 20, 26, 28, 29], [0, 1, 2, 3, 4, 5, 14, 10, 11, 12, 13, 16, 20, 26, 28, 29])


def ladder_tables(order):
    ls, ds = LADDER_LSYMS, LADDER_DSYMS[order]
    if order:
        ls, ds = ls[::-1], ds[::-1]
    return lens_list(ladder(ls), 286), lens_list(ladder(ds), 30)


def ladder_tokens(rng, ll, dl, p284, have, want):
    """tokens for `want` bytes after `have` bytes of text: every literal, every length of LADDER_LENGTHS at every
    distance of LADDER_DISTANCES that the tables code and the text allows, random ones in between"""
    toks, n = [("L", c) for c in LADDER_LITS], len(LADDER_LITS)
    okl = [L for L in LADDER_LENGTHS + [12, 20, 130] if ll[len_sym(L, p284)[0]]]
    okd = [d for d in LADDER_DISTANCES + [48, 128, 12289] if dl[dist_sym(d)[0]]]
    grid = [(L, d) for d in okd for L in okl if L in LADDER_LENGTHS and d in LADDER_DISTANCES]
    while n < want:
        if rng.random() < 0.3:
            toks.append(("L", rng.choice(LADDER_LITS)))
            n += 1
            continue
        pick = [g for g in grid if g[1] <= have + n and g[0] <= want - n]
        if pick and rng.random() < 0.5:
            L, d = pick[0]
            grid.remove(pick[0])
        else:
            L, d = rng.choice(okl), rng.choice(okd)
        if d > have + n or L > want - n + 258:
            continue
        toks.append(("M", L, d))
        n += L
    return toks, grid


@functools.lru_cache(None)
def ladder_family():
    out, rng = {}, random.Random(1)
    for order in (0, 1):
        for p284 in (False, True):
            ll, dl = ladder_tables(order)
            toks, left = ladder_tokens(rng, ll, dl, p284, 0, 65536 - 300)
            assert not left, left
            out[f"ladder_order{order}_p284_{int(p284)}"] = Deflate().dynamic(toks, ll, dl, True, p284).member()
    return out


def flat_litlen():
    """every literal in 9 bits, end-of-block in 2, lengths 3 and 258 in 3 bits each: complete"""
    ll = [9] * 256 + [0] * 30
    ll[256], ll[257], ll[285] = 2, 3, 3
    return ll


@functools.lru_cache(None)
def one_dist():
    """a distance table of one code of length 1 (zlib's encoder always sends two), at distance symbol 0 and 3"""
    lits = [("L", c) for c in b"ACGT"]
    return {"one_dist_sym3": Deflate().dynamic(lits + [("M", 258, 4), ("M", 3, 4), ("L", 10), ("M", 258, 4)], flat_litlen(), [0, 0, 0, 1], True).member(),
            "one_dist_sym0": Deflate().dynamic(lits + [("M", 258, 1), ("L", 67), ("M", 3, 1)] * 3, flat_litlen(), [1], True).member()}


@functools.lru_cache(None)
def no_dist():
    """no distance code at all: HDIST = 0 and that one length is zero; literals only"""
    return {"no_dist": Deflate().dynamic([("L", c) for c in b"@r\nACGT\n+\nIIII\n"], flat_litlen(), [0], True).member()}


@functools.lru_cache(None)
def repeat_zero():
    """dynamic headers with a 16 after a 17 and after an 18 (a repeat of zero), a literal 0 repeated by 16s, and runs
    that cross from the litlen lengths into the distance lengths"""
    out, rng = {}, random.Random(2)
    for order in (0, 1):
        for zr in ("18,16", "0,16"):
            ll, dl = ladder_tables(order)
            toks, _ = ladder_tokens(rng, ll, dl, False, 0, 3000)
            out[f"zero_run_{zr.replace(',', '_')}_order{order}"] = Deflate().dynamic(toks, ll, dl, True, zero_run=zr).member()
    # zeros 258..285 of the litlen lengths run on into the first three distance lengths
    toks = [("L", c) for c in b"GATTACA\n"] + [("M", 3, 4), ("M", 3, 4)]
    for zr in (None, "18,16", "0,16"):
        out[f"zero_straddle_{zr}"] = Deflate().dynamic(toks, [9] * 256 + [2, 2], [0, 0, 0, 1], True, zero_run=zr, nlen=286).member()
    # lengths of 4 bits at 283..285 and at distances 1..4: one literal 4 and a 16 across the border
    ll = [9] * 256 + [0] * 30
    ll[256], ll[257], ll[283], ll[284], ll[285] = 2, 4, 4, 4, 4
    toks = [("L", c) for c in b"ACGTACGTTT"] + [("M", 227, 1), ("M", 258, 2), ("M", 3, 4), ("M", 257, 5), ("M", 200, 8)]
    out["nonzero_straddle"] = Deflate().dynamic(toks, ll, [4, 4, 4, 4, 1, 2], True).member()
    return out


GRID_D = [1, 2, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 257, 258, 259]
GRID_L = [3, 4, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 257, 258]


@functools.lru_cache(None)
def grid():
    """fixed blocks; every distance of GRID_D with every length of GRID_L: the wave width and its multiples on both
    sides of d >= len"""
    out, rng = {}, random.Random(3)
    for d in GRID_D:
        toks = [("L", rng.choice(b"ACGTN")) for _ in range(300)]
        for L in GRID_L:
            toks += [("M", L, d), ("L", rng.choice(b"ACGT"))]
        out[f"grid_d{d}"] = Deflate().fixed(toks, True).member()
    return out


@functools.lru_cache(None)
def mixed():
    """fixed, stored, fixed, empty stored, stored, fixed: the later blocks copy from the text of the earlier ones"""
    out, rng = {}, random.Random(4)
    for slen in (0, 1, 2, 3, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073):
        z = Deflate()
        z.fixed([("L", rng.choice(b"ACGT")) for _ in range(rng.randrange(1, 50))])
        z.stored(bytes(rng.choice(b"ACGTN\n") for _ in range(slen)))
        z.fixed([("L", c) for c in b"GATTACA"] + [("M", 20, len(z.text) + 7), ("M", 258, 1), ("M", 5, 3)] + ([("M", 3 + slen % 200, 270)] if slen > 300 else []))
        z.stored(b"")
        z.stored(bytes(rng.choice(b"ACGT") for _ in range(slen)))
        z.fixed([("M", 9, 2), ("L", 10)] + ([("M", 258, slen + 100), ("M", 65, slen), ("M", 64, len(z.text))] if slen > 300 else []), True)
        out[f"mixed_stored{slen}"] = z.member()
    return out


SWEEP_LENS = list(range(2000, 2070)) + list(range(3024, 3094))


@functools.lru_cache(None)
def ring_sweep():
    """one literal in a fixed block, a stored block of every length of SWEEP_LENS, a fixed block: the third block's header
    lies 7 + length bytes into the payload, on every byte around the edges at which the kernel's 2 KiB input ring moves
    on by half (ring_advance) and starts again (ring_reset)"""
    out, rng = {}, random.Random(5)
    for slen in SWEEP_LENS:
        z = Deflate().fixed([("L", 65)]).stored(bytes(rng.choice(b"ACGTN\n") for _ in range(slen)))
        z.fixed([("L", c) for c in b"GATTACA"] + [("M", 258, 1), ("M", 5, 3), ("M", 40, slen)], True)
        out[f"sweep{slen}"] = z.member()
    return out


def sweep_pads(members, residue, start=0):
    """the extra-subfield size (0..3) per member with which bgzf_wrap places every payload at an offset = residue mod 4"""
    pads, pos = [], start
    for m in members:
        k = (residue - (pos + 22)) % 4
        pads.append(k)
        pos += 22 + k + len(m)
    return pads


def payload_offsets(members, pad=None, start=0):
    """offset of each member's deflate payload in bgzf_wrap(members, pad)"""
    offs, pos = [], start
    pads = pad if isinstance(pad, (list, tuple)) else [pad] * len(members)
    for m, k in zip(members, pads):
        h = 18 if k is None else 22 + k
        offs.append(pos + h)
        pos += h + len(m)
    return offs


@functools.lru_cache(None)
def foreign():
    """members written by another encoder (libdeflate: what bgzip links), from the committed fixture"""
    with open(FOREIGN) as f:
        doc = json.load(f)
    out = {}
    for row in doc["members"]:
        m = base64.b64decode(row["member"])
        z = zlib.decompressobj(-15)
        text = z.decompress(m[:-8])
        assert z.eof and not z.unused_data and IC.trailer(text) == m[-8:] and hashlib.sha256(text).hexdigest() == row["sha256"], row["names"]
        for name in row["names"]:
            out[name] = (m, text)
    return out


def good_families():
    return {"ladder": ladder_family(), "one_dist": one_dist(), "no_dist": no_dist(), "repeat_zero": repeat_zero(), "grid": grid(),
            "mixed": mixed(), "ring_sweep": ring_sweep(), "foreign": foreign()}


def good_members():
    """every good member of every family, {name: (member, text)}"""
    out = {}
    for fam in good_families().values():
        assert not set(fam) & set(out)
        out.update(fam)
    return out


@functools.lru_cache(None)
def crafted_damage():
    """{name: (member, expected status of the kernel core; None: any but OK)}; zlib rejects every one"""
    B, T = Bits, IC.trailer
    out = {}
    # fixed block: literal 'A', then litlen 286 (8-bit code 0xC6); then length 3 with distance symbol 30
    out["fixed_litlen_286"] = (B().put(1, 1).put(1, 2).huff(0x30 + 65, 8).huff(0xC6, 8).bytes() + T(b"A"), IC.BAD_CODE)
    out["fixed_dist_30"] = (B().put(1, 1).put(1, 2).huff(0x30 + 65, 8).huff(1, 7).huff(30, 5).bytes() + T(b"AAAA"), IC.BAD_CODE)
    out["hlit_287"] = (B().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).put(0, 12).bytes() + T(b""), IC.BAD_BLOCK)
    out["hdist_32"] = (B().put(1, 1).put(2, 2).put(0, 5).put(31, 5).put(0, 4).put(0, 12).bytes() + T(b""), IC.BAD_BLOCK)
    # code-length code of 16 and 0, one bit each; the first symbol sent is 16: nothing to repeat
    b = B().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(0, 3).put(0, 3).put(1, 3)
    b.huff(*canon([1] + [0] * 15 + [1, 0, 0])[16]).put(0, 2)
    out["repeat_first"] = (b.bytes() + b"\0\0" + T(b""), IC.BAD_CODE)
    # 257 + 1 lengths, and 18 x 138 twice
    b = B().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(0, 3).put(0, 3).put(1, 3).put(1, 3)
    c18 = canon([1] + [0] * 17 + [1])[18]
    b.huff(*c18).put(127, 7).huff(*c18).put(127, 7)
    out["repeat_past_end"] = (b.bytes() + b"\0" + T(b""), IC.BAD_CODE)
    ll = [0] * 286
    ll[65] = ll[66] = 1
    out["no_eob"] = (Deflate().dynamic_header(ll, [1], True).payload() + b"\0" + T(b""), IC.BAD_CODE)
    ll = lens_list(ladder(LADDER_LSYMS), 286)
    ll[LADDER_LSYMS[-1]] = 0                                       # one of the two 15-bit codes
    out["incomplete_litlen"] = (Deflate().dynamic_header(ll, [1, 1], True).payload() + b"\0\0" + T(b""), IC.BAD_CODE)
    out["stored_nlen"] = (B().put(1, 1).put(0, 2).put(0, 5).put(5, 16).put(5, 16).bytes() + b"ACGTA" + T(b"ACGTA"), IC.BAD_BLOCK)
    out["stored_past_end"] = (B().put(1, 1).put(0, 2).put(0, 5).put(9, 16).put(9 ^ 0xFFFF, 16).bytes() + b"ACGTA" + T(b"ACGTAACGT"), IC.OVERRUN)
    z = Deflate().fixed([("L", 65)] + [("M", 258, 1)] * 255, True)     # 1 + 255 * 258 = 65791 bytes
    out["text_over_64k"] = (z.payload() + T(bytes(z.text[:65536])), IC.OUT_OVERFLOW)
    out["match_past_isize"] = (Deflate().fixed([("L", 65), ("M", 258, 1)], True).payload() + T(b"A" * 100), IC.ISIZE)
    out["no_last_block"] = (Deflate().fixed([("L", 65)]).payload() + T(b"A"), None)
    for name, (m, _) in out.items():
        assert zlib_rejects(m), name
    return out


# ---- whole files ----------------------------------------------------------------------------------------------------
def greedy_tokens(text, max_len=258):
    """a plain greedy LZ77 of `text` on its own (no window before it): the most recent earlier place with the same three
    bytes, extended as far as it matches"""
    toks, last, i, n = [], {}, 0, len(text)
    while i < n:
        key = text[i:i + 3]
        j = last.get(key) if len(key) == 3 else None
        L = 0
        if j is not None and i - j <= 32768:
            L, cap = 3, min(max_len, n - i)
            while L < cap and text[j + L] == text[i + L]:
                L += 1
        if L >= 3:
            toks.append(("M", L, i - j))
        else:
            toks.append(("L", text[i]))
            L = 1
        for k in range(i, min(i + L, n - 2)):
            last[text[k:k + 3]] = k
        i += L
    return toks


def ladder_lens_for(tokens, p284=False):
    """15-bit-deep code lengths (ladder_over) for the symbols these tokens use, the most frequent first"""
    lf, df = {256: 1}, {}
    for t in tokens:
        if t[0] == "L":
            lf[t[1]] = lf.get(t[1], 0) + 1
        else:
            s = len_sym(t[1], p284)[0]
            lf[s] = lf.get(s, 0) + 1
            s = dist_sym(t[2])[0]
            df[s] = df.get(s, 0) + 1
    by = lambda fr: sorted(fr, key=lambda s: (-fr[s], s))
    return lens_list(ladder_over(by(lf), range(285, 0, -1)), 286), lens_list(ladder_over(by(df), range(29, -1, -1)), 30)


def crafted_members_of(text, rng, max_member=65280):
    """`text` as BGZF members cut at arbitrary byte positions; each member's greedy tokens are cut at arbitrary token
    positions into fixed, stored and ladder-coded dynamic blocks (a stored block takes the text of its tokens)"""
    members, i = [], 0
    while i < len(text):
        part = text[i:i + rng.choice([1, 77, 3000, 20011, 40000, max_member, rng.randrange(1, max_member)])]
        toks, z, k, pos = greedy_tokens(part), Deflate(), 0, 0
        while k < len(toks):
            blk = toks[k:k + rng.choice([1, 5, 60, 700, 4000, 20000])]
            k += len(blk)
            last, kind = k >= len(toks), rng.randrange(5)
            if kind == 0:
                z.stored(tokens_text(blk, bytes(z.text)), last)
            elif kind == 1:
                z.fixed(blk, last, p284=True)
            else:
                p284 = bool(kind & 1)
                ll, dl = ladder_lens_for(blk, p284)
                z.dynamic(blk, ll, dl, last, p284, zero_run=(None, "18,16", "0,16")[kind - 2])
            if kind == 0 and last is False and rng.randrange(3) == 0:
                z.stored(b"")
        m, t = z.member()
        assert t == part
        if len(m) + 22 > 65536:                                    # (too large for a BGZF member: the next draw is another)
            continue
        i += len(part)
        members.append(m)
    return members


def big_gzip(rng, size=6_000_000):
    """(gzip file bytes, text, notes): one member of about `size` bytes of text in some 400 blocks drawn from the families --
    ladder-coded blocks with distances up to 32768 into earlier blocks, single-distance-code blocks, fixed blocks,
    stored blocks of 0, 1, 5, 700 and 65535 bytes"""
    z, notes = Deflate(ByteBits()), dict(blocks=0, stored=set(), reach_back=0, max_distance=0)
    while len(z.text) < size:
        kind, toks, start = rng.randrange(5), [], len(z.text)
        if kind < 2:
            ll, dl = ladder_tables(kind)
            p284 = bool(rng.randrange(2))
            toks, _ = ladder_tokens(rng, ll, dl, p284, len(z.text), rng.randrange(2000, 60000))
            z.dynamic(toks, ll, dl, False, p284, zero_run=rng.choice([None, "18,16", "0,16"]))
        elif kind == 2:
            toks = [("L", rng.choice(b"ACGTN\n@+IF")) for _ in range(rng.randrange(4, 3000))] + [("M", 258, 4), ("M", 3, 4)] * rng.randrange(1, 40)
            z.dynamic(toks, flat_litlen(), [0, 0, 0, 1], False)
        elif kind == 3:
            z.stored(bytes(rng.choice(b"ACGTN\n") for _ in range(rng.choice([0, 0, 1, 5, 700, 65535]))))
            notes["stored"].add(len(z.text) - start)
        else:
            toks = [("L", rng.choice(b"ACGT")) for _ in range(rng.randrange(0, 200))]
            if len(z.text) > 300:
                toks += [("M", rng.choice([3, 64, 65, 258]), rng.choice([1, 63, 64, 65, 258]))]
            z.fixed(toks, False, p284=True)
        notes["blocks"] += 1
        pos = start                                            # matches that begin before their own block
        for t in toks:
            if t[0] == "M":
                notes["reach_back"] += t[2] > pos - start
                notes["max_distance"] = max(notes["max_distance"], t[2])
            pos += 1 if t[0] == "L" else t[1]
    z.fixed([], True)
    raw, text = z.payload(), bytes(z.text)
    zd = zlib.decompressobj(-15)
    assert zd.decompress(raw) == text and zd.eof
    return b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF), text, notes


def crafted_fastq_file(guides, n_reads=3000, seed=8):
    """(BGZF file bytes with the end marker, FASTQ text, members): n_reads synthetic reads against `guides`, written by
    crafted_members_of"""
    import synth
    fq = synth.make_fastq(synth.Spec(seed=seed, n_reads=n_reads, read_len=50), guides)
    members = crafted_members_of(fq, random.Random(seed))
    return IC.bgzf_wrap(members + [IC.member(b"")]), fq, members

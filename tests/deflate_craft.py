"""Hand-built raw DEFLATE streams for the tests: fixed-Huffman and dynamic-Huffman blocks from an explicit token list, the code
generators and the table search that go with the dynamic ones, and a plain reference decoder (inflate_ref).

Token = int (literal byte) or (length, distance).  Lets a test place back-references at exact output
positions -- e.g. the resolve-pass regression of ADVICE r01 (hole at p with p % 1024 in 1021..1023,
distance 32766..32768, next hole 2048 further).  RFC 1951 section 3.2.5 / 3.2.6 tables, written out here.
"""

_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
          8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class _Bits:
    def __init__(self):
        self.acc = 0
        self.n = 0
        self.out = bytearray()

    def put(self, val, nbits):            # LSB first (extra bits, header fields)
        self.acc |= val << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, nbits):      # Huffman codes go MSB first
        rev = int(bin(code)[2:].zfill(nbits)[::-1], 2)
        self.put(rev, nbits)

    def finish(self):
        if self.n:
            self.out.append(self.acc & 0xFF)
        return bytes(self.out)


def _lit_code(s):
    if s < 144:
        return 0x30 + s, 8
    if s < 256:
        return 0x190 + (s - 144), 9
    if s < 280:
        return s - 256, 7
    return 0xC0 + (s - 280), 8


def fixed_block(tokens, final=True):
    """raw deflate stream: one fixed-Huffman block holding `tokens`"""
    b = _Bits()
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    put_fixed(b, tokens)
    return b.finish()


def put_fixed(b, tokens, eob=True):
    """the tokens of a fixed-Huffman block (behind its three header bits) into a _Bits that may stand at any bit"""
    for t in tokens:
        if isinstance(t, int):
            b.put_code(*_lit_code(t))
            continue
        length, dist = t
        li = max(i for i in range(29) if _LBASE[i] <= length)
        if length == 258:
            li = 28
        b.put_code(*_lit_code(257 + li))
        b.put(length - _LBASE[li], _LEXT[li])
        di = max(i for i in range(30) if _DBASE[i] <= dist)
        b.put_code(di, 5)
        b.put(dist - _DBASE[di], _DEXT[di])
    if eob:
        b.put_code(*_lit_code(256))


def expand(tokens):
    """what the token list decodes to"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] != "raw":                   # (raw bits stand for nothing here: they are padding, or an error)
            length, dist = t[0], t[1]
            if length <= dist <= len(out):
                out += out[len(out) - dist:len(out) - dist + length]
                continue
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


# ---- dynamic-Huffman blocks (RFC 1951 section 3.2.7) from explicit code lengths --------------------------------------------------
# Lets a test put the decoder on its limits, which no compressor does: 15-bit codes on the symbols with the most extra bits (a
# 48-bit token), length 258 as code 284 + 31, code sets whose two-level tables are as large as they can get, the single-code
# forms, headers of every shape.  `inflate_ref` below is the judge that goes with it: a plain bit-by-bit decoder.
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _pos(b):
    """bit position a _Bits stands at"""
    return 8 * len(b.out) + b.n


def canonical(lengths):
    """RFC 1951 section 3.2.2: the code of every symbol (MSB first, 0 where the length is 0)"""
    cnt = [0] * 16
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return out


def _kraft(lengths, top=15):
    return sum(1 << (top - l) for l in lengths if l)


def _cl_code(freq, spread):
    """lengths (<= 7) of a COMPLETE code-length code over the symbols with freq > 0 (zlib refuses an incomplete one).
    spread False: a Huffman-like code (frequent symbols short).  spread True: 7-bit codes on as many of the used symbols as a
    complete code allows, the short codes on symbols that are never sent."""
    used = [s for s in range(19) if freq[s]]
    lens = [0] * 19
    if spread:
        free = [s for s in range(19) if not freq[s]]
        seven = list(used)
        while True:
            rest = 128 - len(seven)
            terms = [7 - k for k in range(7) if rest >> k & 1]            # lengths whose weights add up to the rest
            if len(terms) <= len(free):
                break
            free.append(seven.pop(0))
        for s in seven:
            lens[s] = 7
        for s, l in zip(free, sorted(terms)):
            lens[s] = l
        assert _kraft(lens, 7) == 128
        return lens
    if len(used) < 2:                                                      # one symbol: a partner that is never sent
        used = used + [s for s in (0, 8, 18) if s not in used][:2 - len(used)]
    order = sorted(used, key=lambda s: (-freq[s], s))
    total = sum(freq[s] for s in used) or 1
    for s in order:                                                        # Shannon lengths, then make the code exactly complete
        l, f = 1, max(freq[s], 1)
        while l < 7 and (f << l) < total:
            l += 1
        lens[s] = l
    while _kraft(lens, 7) > 128:
        s = max((s for s in order if lens[s] < 7), key=lambda s: (lens[s], -freq[s]))
        lens[s] += 1
    while _kraft(lens, 7) < 128:
        room = 128 - _kraft(lens, 7)
        s = next(s for s in order if lens[s] > 1 and (1 << (7 - lens[s])) <= room)
        lens[s] -= 1
    return lens


def _cl_symbols(seq, header):
    """the code-length symbols of the length sequence: [(symbol, extra value, extra bits)]"""
    if header in ("plain", "min"):
        return [(l, 0, 0) for l in seq]
    syms, i, n = [], 0, len(seq)
    once = set()
    while i < n:
        run = 1
        while i + run < n and seq[i + run] == seq[i]:
            run += 1
        v = seq[i]
        if header == "long":
            # every length costs its 7 bits; each repeat symbol once, with its smallest count: the most bits per length it can cost
            if v == 0 and run >= 11 and 18 not in once:
                once.add(18); syms.append((18, 0, 7)); i += 11
            elif v == 0 and run >= 3 and 17 not in once:
                once.add(17); syms.append((17, 0, 3)); i += 3
            elif v != 0 and run >= 4 and 16 not in once:
                once.add(16); syms += [(v, 0, 0), (16, 0, 2)]; i += 4
            else:
                syms.append((v, 0, 0)); i += 1
            continue
        if v == 0 and run >= 3:                    # "rle": greedy; the runs take no notice of where the distance lengths begin
            k = min(run, 138)
            syms.append((18, k - 11, 7) if k >= 11 else (17, k - 3, 3))
            i += k
        elif v != 0 and run >= 4:
            syms.append((v, 0, 0))
            k = min(run - 1, 6)
            syms.append((16, k - 3, 2))
            i += 1 + k
        else:
            syms.append((v, 0, 0))
            i += 1
    return syms


def dynamic_block(tokens, ll_lens, d_lens, final=True, bits=None, header="rle", eob=True):
    """Append one dynamic-Huffman block to `bits` (a _Bits shared by the blocks of a stream) and return the bit position of its
    first header bit.  ll_lens: 257..286 literal/length code lengths (shorter lists are padded to 257), d_lens: 1..30 distance code
    lengths; nothing is checked, so the code sets may be invalid on purpose.
    Tokens: int literal | (length, dist) | (length, dist, index of the length symbol: 258 as (258, d, 27) is code 284 + 31) |
    ("raw", value, nbits): arbitrary bits in place of a token.  The end-of-block code follows unless eob is False or it has none.
    header: "plain" no repeat symbols, a 4-bit code-length code over 0..15 | "rle" symbols 16 / 17 / 18 greedily, runs crossing
    from the literal/length lengths into the distance lengths | "long" (about) the longest header these lengths can have: 7-bit
    codes on the code-length symbols that are used, each repeat symbol once with its smallest count | "min" no repeat symbols
    and a code over the lengths that occur only.  HCLEN is always the smallest the code-length code allows, down to 4."""
    b = bits if bits is not None else _Bits()
    at = _pos(b)
    ll = list(ll_lens) + [0] * (257 - len(ll_lens))
    dl = list(d_lens)
    assert 257 <= len(ll) <= 286 and 1 <= len(dl) <= 30
    syms = _cl_symbols(ll + dl, header)
    if header == "plain":
        cl = [4] * 16 + [0, 0, 0]
    else:
        freq = [0] * 19
        for s, _, _ in syms:
            freq[s] += 1
        cl = _cl_code(freq, header == "long")
    hclen = max([4] + [i + 1 for i in range(19) if cl[_ORDER[i]]])
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(len(ll) - 257, 5)
    b.put(len(dl) - 1, 5)
    b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl[_ORDER[i]], 3)
    cc = canonical(cl)
    for s, v, n in syms:
        assert cl[s]
        b.put_code(cc[s], cl[s])
        b.put(v, n)
    put_tokens(b, tokens, ll, dl, eob)
    return at


def put_tokens(b, tokens, ll, dl, eob=True):
    """the tokens of a block in the codes of these lengths (dynamic_block without the header)"""
    lc, dc = canonical(ll), canonical(dl)
    for t in tokens:
        if isinstance(t, int):
            assert ll[t], t
            b.put_code(lc[t], ll[t])
            continue
        if t[0] == "raw":
            b.put(t[1], t[2])
            continue
        length, dist = t[0], t[1]
        li = t[2] if len(t) > 2 else (28 if length == 258 else max(i for i in range(29) if _LBASE[i] <= length))
        assert ll[257 + li] and 0 <= length - _LBASE[li] < (1 << _LEXT[li]) or (length == _LBASE[li] and ll[257 + li]), t
        b.put_code(lc[257 + li], ll[257 + li])
        b.put(length - _LBASE[li], _LEXT[li])
        di = max(i for i in range(30) if _DBASE[i] <= dist)
        assert dl[di], t
        b.put_code(dc[di], dl[di])
        b.put(dist - _DBASE[di], _DEXT[di])
    if eob and len(ll) > 256 and ll[256]:
        b.put_code(lc[256], ll[256])


# ---- code generators: lists of lengths ---------------------------------------------------------------------------------------------
def random_complete(n, rng, deep=False):
    """the lengths of a complete code of n symbols: leaves are split until there are n of them, none deeper than 15; `deep` splits
    the deepest leaf that can still be split three times out of four, which gives long codes and many second-level tables"""
    assert 2 <= n <= 1 << 15
    leaves = [1, 1]
    while len(leaves) < n:
        ok = [i for i, d in enumerate(leaves) if d < 15]
        if deep and rng.random() < 0.75:
            top = max(leaves[i] for i in ok)
            i = rng.choice([i for i in ok if leaves[i] == top])
        else:
            i = rng.choice(ok)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    assert _kraft(leaves) == 1 << 15
    return leaves


def comb(symbols, n):
    """n lengths in which symbols[i] has length i + 1 and the last two share the longest: 1, 2, ..., k - 1, k - 1"""
    k = len(symbols)
    assert 2 <= k <= 16 and len(set(symbols)) == k
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, k - 1)
    return lens


def from_counts(counts, rng, n=None):
    """the count vector (counts[l - 1] codes of length l) dealt out to shuffled symbols; n pads with unused symbols"""
    lens = [l + 1 for l, c in enumerate(counts) for _ in range(c)]
    lens += [0] * ((n or len(lens)) - len(lens))
    rng.shuffle(lens)
    return lens


def table_size(lengths, root):
    """entries of the two-level table of these lengths: 2^root, and for every root prefix that longer codes share a sub-table of
    2^(the longest of them - root) -- in canonical order those codes are neighbours"""
    codes = canonical(lengths)
    longest = {}
    for c, l in zip(codes, lengths):
        if l > root:
            p = c >> (l - root)
            longest[p] = max(longest.get(p, 0), l)
    return (1 << root) + sum(1 << (l - root) for l in longest.values())


_WORST = {}


def worst_table(root, nsym, maxlen=15):
    """(entries, counts for lengths 1..maxlen) of the complete code of nsym symbols whose two-level table (table_size) is largest.
    A search over count vectors, memoised as a table per length: canonical codes fill the code space from the left, so behind
    the codes shorter than l all that matters is (symbols left, code space still free in units of 2^-l); free <= left, or the
    code cannot be completed.  A root prefix that holds codes longer than the root fills up at the length of its LAST code, which
    is the one that sizes its sub-table: c codes of length l > root cost 2^(l - root) for every prefix boundary they reach."""
    import numpy as np
    if (root, nsym, maxlen) in _WORST:
        return _WORST[root, nsym, maxlen]
    N, NEG = nsym + 1, -(1 << 40)
    V = np.full((N, N), NEG, dtype=np.int64)            # [symbols left, free]: best cost still to come, behind length l
    V[0, 0] = 0
    picks = []
    for l in range(maxlen, 0, -1):
        W = np.full((N, N), NEG, dtype=np.int64)
        arg = np.zeros((N, N), dtype=np.int16)
        for c in range(N):                              # c codes of length l: (left, free) -> (left - c, 2 (free - c))
            f = np.arange(c, min(nsym, c + nsym // 2) + 1)
            if l > root:
                used = (1 << l) - f
                cost = (((used + c) >> (l - root)) - (used >> (l - root))) << (l - root)
            else:
                cost = np.zeros(len(f), dtype=np.int64)
            cand = V[:N - c][:, 2 * (f - c)] + cost[None, :]
            tgt, ta = W[c:, c:c + len(f)], arg[c:, c:c + len(f)]
            better = cand > tgt
            tgt[better] = cand[better]
            ta[better] = c
        W[:, (1 << l) + 1:] = NEG                       # more free space than there is at this length
        W[0, 0] = 0
        V = W
        picks.append(arg)
    assert V[nsym, 2] >= 0
    counts, left, free = [], nsym, 2
    for arg in reversed(picks):
        c = int(arg[left, free]) if left else 0
        counts.append(c)
        left, free = left - c, 2 * (free - c)
    assert left == 0 and free == 0 and sum(counts) == nsym
    _WORST[root, nsym, maxlen] = ((1 << root) + int(V[nsym, 2]), counts)
    return _WORST[root, nsym, maxlen]


# ---- the judge: RFC 1951 decoded one bit at a time -----------------------------------------------------------------------------------
class _Stop(Exception):
    def __init__(self, status, kind):
        self.status, self.kind = status, kind


class _Code:
    """canonical code as counts and symbols in (length, symbol) order; no tables"""
    def __init__(self, lengths):
        self.count = [0] * 16
        for l in lengths:
            self.count[l] += 1
        self.count[0] = 0
        self.syms = [s for l in range(1, 16) for s, x in enumerate(lengths) if x == l]
        self.maxlen = max([l for l in range(16) if self.count[l]] or [0])
        left = 1
        for l in range(1, 16):
            left = 2 * left - self.count[l]
            if left < 0:
                break
        self.left = left                                 # < 0 over-subscribed, > 0 incomplete


class _Reader:
    def __init__(self, data, pos):
        self.d, self.pos, self.end = data, pos, 8 * len(data)

    def need(self, n):
        if self.pos + n > self.end:
            self.pos = self.end                          # everything there was has been taken
            raise _Stop(-5, "need input")

    def take(self, n):
        self.need(n)
        p = self.pos
        v = (int.from_bytes(self.d[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << n) - 1)
        self.pos = p + n
        return v

    def symbol(self, code, kind):
        """first code and count per length (RFC 1951 3.2.2 read backwards).  Past the longest code nothing can match: the pattern is
        invalid with that many bits read -- ONE bit for the unused half of a one-symbol code and for a code with no symbol, as the
        reference's tables have it; with fewer bits left the decoder asks for more input"""
        p = self.pos
        w = int.from_bytes(self.d[p >> 3:(p >> 3) + 3], "little") >> (p & 7)
        have = self.end - p
        c = first = index = 0
        top = max(code.maxlen, 1)
        for l in range(1, top + 1):
            if l > have:
                self.pos = self.end
                raise _Stop(-5, "need input")
            c |= w & 1
            w >>= 1
            n = code.count[l]
            if c - n < first:
                self.pos = p + l
                return code.syms[index + c - first]
            index += n
            first = (first + n) << 1
            c <<= 1
        self.pos = p + top
        raise _Stop(-3, kind)


_FIXED_CODES = None


def inflate_ref(stream, cap, start_bit=0, history=b""):
    """Decode a raw deflate stream from bit `start_bit` with `history` in front of the output and room for `cap` bytes ->
    (status, output, bits used, kind).  status in zlib numbering: 0 done, -3 data error, -5 more input or more room needed; bits
    used counts from bit 0 of the stream up to where the decoder stopped (all of the input when it ran out; the bits of the invalid
    entry when a code is invalid; bytes used are that rounded up); kind says what stopped it: None, or one of KINDS.
    The order of the checks is the reference's: a repeat's extra bits are read before the repeat is judged, a distance is
    judged before the room, and a match that does not fit produces none of its bytes."""
    global _FIXED_CODES
    if _FIXED_CODES is None:
        _FIXED_CODES = (_Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _Code([5] * 32))   # (286, 287, 30, 31: codes for no symbol)
    r = _Reader(bytes(stream), start_bit)
    out = bytearray(history)
    h = len(history)
    cap += h
    try:
        last = 0
        while not last:
            r.need(3)
            last, typ = r.take(1), r.take(2)
            if typ == 0:
                r.pos = (r.pos + 7) & ~7
                r.need(32)
                n, nn = r.take(16), r.take(16)
                if n ^ 0xFFFF != nn:
                    raise _Stop(-3, "stored lengths")
                at = r.pos >> 3
                have, room = len(r.d) - at, cap - len(out)
                k = min(n, have, room)
                out += r.d[at:at + k]
                r.pos += 8 * k
                if k < n:
                    raise _Stop(-5, "need room" if room < min(n, have) else "need input")
                continue
            if typ == 3:
                raise _Stop(-3, "invalid block type")
            if typ == 1:
                lc, dc = _FIXED_CODES
            else:
                r.need(14)
                nlen, ndist, ncode = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
                if nlen > 286 or ndist > 30:
                    raise _Stop(-3, "too many symbols")
                cl = [0] * 19
                for i in range(ncode):
                    cl[_ORDER[i]] = r.take(3)
                cc = _Code(cl)
                if cc.left != 0:
                    raise _Stop(-3, "code lengths set")
                lens = []
                while len(lens) < nlen + ndist:
                    s = r.symbol(cc, "code lengths set")
                    if s < 16:
                        lens.append(s)
                        continue
                    val = 0
                    if s == 16:
                        rep = 3 + r.take(2)              # (the two bits are read before the repeat is judged)
                        if not lens:
                            raise _Stop(-3, "bit length repeat")
                        val = lens[-1]
                    elif s == 17:
                        rep = 3 + r.take(3)
                    else:
                        rep = 11 + r.take(7)
                    if len(lens) + rep > nlen + ndist:
                        raise _Stop(-3, "bit length repeat")
                    lens += [val] * rep
                if lens[256] == 0:
                    raise _Stop(-3, "missing end-of-block")
                lc, dc = _Code(lens[:nlen]), _Code(lens[nlen:])
                if lc.left < 0 or (lc.left > 0 and lc.maxlen != 1):
                    raise _Stop(-3, "literal/lengths set")
                if dc.left < 0 or (dc.left > 0 and dc.maxlen > 1):
                    raise _Stop(-3, "distances set")
            while True:
                s = r.symbol(lc, "literal/length code")
                if s < 256:
                    if len(out) >= cap:
                        raise _Stop(-5, "need room")
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise _Stop(-3, "literal/length code")
                s -= 257
                length = _LBASE[s] + r.take(_LEXT[s])
                d = r.symbol(dc, "distance code")
                if d > 29:
                    raise _Stop(-3, "distance code")
                dist = _DBASE[d] + r.take(_DEXT[d])
                if dist > len(out):
                    raise _Stop(-3, "distance too far back")
                if len(out) + length > cap:
                    raise _Stop(-5, "need room")
                if dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
    except _Stop as e:
        return e.status, bytes(out[h:]), r.pos, e.kind
    return 0, bytes(out[h:]), r.pos, None


KINDS = ["invalid block type", "stored lengths", "too many symbols", "code lengths set", "bit length repeat", "missing end-of-block",
         "literal/lengths set", "distances set", "literal/length code", "distance code", "distance too far back", "need input",
         "need room"]

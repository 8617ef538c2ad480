"""Hand-built dynamic-Huffman streams at the decoder's table and token limits (tests/deflate_craft.py) and the checks that send them
through every decode entry point: shared by tests/test_deflate_craft.py (CPU: the streams against the oracle, system zlib and
deflate_craft.inflate_ref), tests/test_emu_dynamic_blocks.py (the emulator build) and tests/test_gpu_dynamic_blocks.py (the MI355X).

No compressor emits these: 15-bit codes on the symbols with the most extra bits (a 48-bit token: 15 + 5 + 15 + 13), length 258 as
code 284 + 31, code sets whose tables are exactly 852 and 400 entries (csrc/inflate.hip INF_LSIZE / INF_DSIZE), the single-code
forms, HCLEN 5 and 4, repeats that run from the literal/length lengths into the distance lengths, the longest headers, hundreds of
blocks that are nearly all header.  Everything is seeded (random.Random only).  A stream meant for the lane-serial fast pass
(inf_fast_pass) has more than 4 KiB of compressed bytes behind its first header; the small ones go through the token rounds.

The judge is never the library: expected bytes come from deflate_craft.expand and inflate_ref, and tests/test_deflate_craft.py
holds both to the oracle (pinned on the reference) and to system zlib before a kernel sees a stream."""
import functools
import random

import deflate_craft as D

Z_DATA_ERROR, Z_BUF_ERROR = -3, -5
RAW = 0

# inflate_ref's `kind` -> the detail word of the size pass / the packed decode / zmi_inflate_batch_dev_ex: 16 + k, k the index of the
# reference's message (csrc/inflate.hip DE_*, the strings of zlib-rs/src/inflate.rs State::bad), 1 = more input, 2 = more room.
# The two "invalid ... code" messages share one word (DE_CODE): the kernel does not say which of the two codes was the bad one.
DETAIL = {"stored lengths": 16 + 1, "invalid block type": 16 + 2, "too many symbols": 16 + 3, "code lengths set": 16 + 4,
          "bit length repeat": 16 + 5, "missing end-of-block": 16 + 6, "literal/lengths set": 16 + 7, "distances set": 16 + 8,
          "distance too far back": 16 + 9, "literal/length code": 16 + 11, "distance code": 16 + 11, "need input": 1, "need room": 2}
# ... and -> the oracle's message
MESSAGE = {"stored lengths": "invalid stored block lengths", "invalid block type": "invalid block type",
           "too many symbols": "too many length or distance symbols", "code lengths set": "invalid code lengths set",
           "bit length repeat": "invalid bit length repeat", "missing end-of-block": "invalid code -- missing end-of-block",
           "literal/lengths set": "invalid literal/lengths set", "distances set": "invalid distances set",
           "literal/length code": "invalid literal/length code", "distance code": "invalid distance code",
           "distance too far back": "invalid distance too far back", "need input": None, "need room": None}


class Case:
    """name; stream; raw: the bytes it decodes to (a failing stream: None); blocks: bit position of every block's first header
    bit; klass: the error class of a failing stream; bad: bit position of the code that is wrong; hist: history in front"""
    def __init__(self, name, stream, raw=None, blocks=(), klass=None, bad=None, hist=b""):
        self.name, self.stream, self.raw, self.blocks, self.klass, self.bad, self.hist = name, stream, raw, list(blocks), klass, bad, hist

    def __repr__(self):
        return "Case(%s, %d bytes)" % (self.name, len(self.stream))


def _clone(b):
    c = D._Bits()
    c.acc, c.n, c.out = b.acc, b.n, bytearray(b.out)
    return c


# ---- codes ---------------------------------------------------------------------------------------------------------------------------
WIDE_LITS = [0x61, 0x20, 0x65, 0x74, 0x0A, 0x00, 0xFF, 0x80, 0x7F, 0x31]


def wide_codes():
    """combs: literal/length 1 .. 15, 15 with 285 and end-of-block in the middle and 281 .. 284 at 13, 14, 15, 15 bits;
    distance 1 .. 15, 15 with 28 and 29 at 15 bits"""
    L = WIDE_LITS
    ll = D.comb(L[:6] + [285, L[6], 256] + L[7:] + [281, 282, 283, 284], 286)
    dl = D.comb([0, 1, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 29], 30)
    assert [ll[s] for s in (281, 282, 283, 284)] == [13, 14, 15, 15] and dl[28] == dl[29] == 15
    return ll, dl


@functools.lru_cache(maxsize=None)
def worst_codes(seed):
    """a 286-symbol code whose table is 852 entries and a 30-symbol code whose table is 400, dealt to shuffled symbols"""
    rng = random.Random(seed)
    e9, c9 = D.worst_table(9, 286)
    e8, c8 = D.worst_table(8, 30)
    ll, dl = D.from_counts(c9, rng), D.from_counts(c8, rng)
    assert (e9, e8) == (852, 400) and D.table_size(ll, 9) == 852 and D.table_size(dl, 8) == 400
    return ll, dl


def random_codes(rng, deep, nll=286, nd=30):
    return D.random_complete(nll, rng, deep), D.random_complete(nd, rng, deep)


def eob15_codes(rng):
    """a deep code whose end-of-block symbol has one of the 15-bit codes"""
    while True:
        ll, dl = random_codes(rng, True)
        if 15 in ll:
            i = ll.index(15)
            ll[i], ll[256] = ll[256], ll[i]
            return ll, dl


def rand_tokens(rng, ntok, ll, dl, n0=0, p_match=0.3, short=True):
    """ntok random tokens over the symbols these codes have: literals, and matches of length 3 .. 258 at distance 1 .. min(n, 32768)
    (short: most lengths small, so that a stream's output stays a few times its size); n0 = bytes in front"""
    lits = [s for s in range(256) if s < len(ll) and ll[s]]
    lens = [k for k in range(3, 259) if ll[257 + (28 if k == 258 else max(i for i in range(29) if D._LBASE[i] <= k))]] if len(ll) > 257 else []
    toks, n, ok = [], n0, set(lens)
    for _ in range(ntok):
        if n and lens and rng.random() < p_match:
            for _ in range(8):
                dist = rng.randint(1, min(n, 32768)) if rng.random() < 0.5 else rng.randint(1, min(n, 64))
                if dl[max(i for i in range(30) if D._DBASE[i] <= dist)]:
                    break
            else:
                continue
            length = rng.choice(lens)
            if short and rng.random() < 0.9:
                k = 3 + min(int(rng.expovariate(1 / 8.0)), 255)
                length = k if k in ok else length
            toks.append((length, dist))
            n += length
        elif lits:
            toks.append(rng.choice(lits))
            n += 1
    return toks


def _finish(name, b, toks, blocks, **kw):
    return Case(name, b.finish(), D.expand(toks), blocks, **kw)


def one_block(name, toks, ll, dl, header="rle"):
    b = D._Bits()
    at = D.dynamic_block(toks, ll, dl, bits=b, header=header)
    return _finish(name, b, toks, [at])


# ---- 1. wide tokens ---------------------------------------------------------------------------------------------------------------------
def _wide_mix(rng, ntok):
    L = WIDE_LITS
    toks = []
    for _ in range(ntok):
        x = rng.random()
        if x < 0.7:
            toks.append((258, 32768, 27))                                    # 284 + 31 | 29 + 8191: 15 + 5 + 15 + 13 = 48 bits
        elif x < 0.85:
            toks.append((rng.randint(195, 226), rng.randint(16385, 32768)))  # 281: 13 + 5 bits, 28 / 29: 15 + 13
        else:
            toks.append(rng.choice(L))
    return toks


def wide_tokens():
    """about 33 000 literals, then about 6 000 tokens of which 70 % are the 48-bit one"""
    rng = random.Random(4801)
    ll, dl = wide_codes()
    toks = [WIDE_LITS[min(int(rng.expovariate(0.5)), 9)] for _ in range(33000)] + _wide_mix(rng, 6000)
    return one_block("wide_tokens", toks, ll, dl)


def _wide_placed(name, off, cut_at_last=False):
    """one block in the wide codes whose first fast pass (64 sub-sequences of 480 bits from the block's first token bit) meets a
    48-bit token that starts `off` bits in front of a sub-sequence boundary, at four boundaries; the padding is the 1-bit literal.
    cut_at_last: no end-of-block, and the last 48-bit token ends with the last byte of the input."""
    rng = random.Random(4802 + off)
    ll, dl = wide_codes()
    b = D._Bits()
    at = D.dynamic_block([], ll, dl, bits=b, eob=False)
    t0 = D._pos(b)
    toks = []

    def put(ts):
        D.put_tokens(b, ts, ll, dl, eob=False)
        toks.extend(ts)

    put([WIDE_LITS[0]] + [(258, 1)] * 130)                    # 33 541 bytes of output in about 1 100 bits
    for k in (5, 18, 40, 63):
        want = k * 480 - off
        while want - (D._pos(b) - t0) > 600:
            put(_wide_mix(rng, 1))
        assert D._pos(b) - t0 <= want
        put([WIDE_LITS[0]] * (want - (D._pos(b) - t0)))
        put([(258, 32768, 27)])
        assert D._pos(b) - t0 == want + 48
    put(_wide_mix(rng, 1200))
    if cut_at_last:
        put([WIDE_LITS[0]] * (-(D._pos(b) + 48) % 8) + [(258, 32768, 27)])
        assert D._pos(b) % 8 == 0
        c = Case(name, b.finish(), None, [at], klass="cut behind a 48-bit token")
        c.prefix = D.expand(toks)
        return c
    D.put_tokens(b, [], ll, dl)
    return _finish(name, b, toks, [at])


# ---- 2. worst tables --------------------------------------------------------------------------------------------------------------------
def worst_tables():
    out = []
    for i, (seed, ntok) in enumerate(((851, 40), (852, 17000), (853, 17000))):
        ll, dl = worst_codes(seed)
        out.append(one_block("worst_tables/%d" % ntok if i == 0 else "worst_tables/%d/%d" % (ntok, i),
                             rand_tokens(random.Random(seed), ntok, ll, dl), ll, dl, header=("rle", "plain", "long")[i]))
    # the two vectors as the only long-code block among ordinary blocks
    rng = random.Random(854)
    b, toks, blocks = D._Bits(), [], []
    for k in range(5):
        ll, dl = worst_codes(851) if k == 2 else random_codes(rng, False)
        t = rand_tokens(rng, 2500, ll, dl, n0=len(D.expand(toks)))
        blocks.append(D.dynamic_block(t, ll, dl, final=k == 4, bits=b))
        toks += t
    out.append(_finish("worst_tables/among ordinary blocks", b, toks, blocks))
    return out


# ---- 3. random codes --------------------------------------------------------------------------------------------------------------------
def random_code_streams():
    out = []
    for i in range(6):
        rng = random.Random(900 + i)
        deep = i >= 3
        ll, dl = random_codes(rng, deep, nll=257)
        toks = [rng.randrange(256) for _ in range(20000)]         # uniform literals: the long codes come as often as the short ones
        out.append(one_block("random_codes/literals/%s/%d" % ("deep" if deep else "shallow", i), toks, ll, dl))
    for i in range(6):
        rng = random.Random(950 + i)
        deep = i >= 3
        ll, dl = random_codes(rng, deep)
        out.append(one_block("random_codes/tokens/%s/%d" % ("deep" if deep else "shallow", i),
                             rand_tokens(rng, 9000 if deep else 12000, ll, dl), ll, dl, header=("rle", "plain", "long")[i % 3]))
    return out


# ---- 4. single-code forms ---------------------------------------------------------------------------------------------------------------
def _one_dist(rng, ntok):
    ll, _ = random_codes(rng, False)
    toks = [rng.randrange(256)]
    for _ in range(ntok):
        toks.append((rng.randint(3, 258), 1) if rng.random() < 0.2 else rng.randrange(256))
    return toks, ll, [1]


def _no_dist(rng, ntok):
    ll, _ = random_codes(rng, True, nll=257)
    return [rng.randrange(256) for _ in range(ntok)], ll, [0]


ONLY_EOB = [0] * 256 + [1]


def single_code_forms():
    out = []
    rng = random.Random(1001)
    for n in (60, 6000):
        out.append(one_block("single_code/one distance code of length 1/%d" % n, *_one_dist(rng, n)))
        out.append(one_block("single_code/no distance code/%d" % n, *_no_dist(rng, n)))
        ll, dl = eob15_codes(rng)
        out.append(one_block("single_code/end-of-block at 15 bits/%d" % n, rand_tokens(rng, n, ll, dl), ll, dl))
    out.append(one_block("single_code/only end-of-block", [], ONLY_EOB, [0]))
    return out


# ---- 5. headers, 6. tiny blocks ---------------------------------------------------------------------------------------------------------
HCLEN5 = [8] * 255 + [0, 8]          # 256 codes of 8 bits (no literal 255), no distance code: with "min" the header has HCLEN 5


def headers():
    """40 blocks cycling through the forms above and through the four header shapes; every fifth block holds no token"""
    rng = random.Random(1100)
    forms = [lambda: wide_codes(), lambda: worst_codes(851), lambda: random_codes(rng, True), lambda: (_one_dist(rng, 0)[1], [1]),
             lambda: (_no_dist(rng, 0)[1], [0]), lambda: (ONLY_EOB, [0]), lambda: eob15_codes(rng), lambda: (HCLEN5, [0]),
             lambda: random_codes(rng, False)]
    shapes = ["plain", "rle", "long", "min"]
    b, toks, blocks = D._Bits(), [], []
    for k in range(40):
        ll, dl = forms[k % len(forms)]()
        n = len(D.expand(toks))
        if k % 5 == 4 or ll is ONLY_EOB:
            t = []
        elif dl == [1]:
            t = [rng.randrange(256)] + [(rng.randint(3, 258), 1) for _ in range(rng.randint(1, 30))]
        else:
            t = rand_tokens(rng, rng.randint(1, 400), ll, dl, n0=n)
        blocks.append(D.dynamic_block(t, ll, dl, final=k == 39, bits=b, header=shapes[(k + k // len(forms)) % 4]))
        toks += t
    return _finish("headers", b, toks, blocks)


def tiny_blocks():
    """300 dynamic blocks of 0 .. 39 literals in deep codes: nearly all bits are header bits, so header and table build meet the
    1 KiB input chunk boundary (INF_CHUNK) at every alignment"""
    rng = random.Random(1200)
    b, toks, blocks = D._Bits(), [], []
    for k in range(300):
        ll, dl = random_codes(rng, True)
        t = [rng.randrange(256) for _ in range(rng.randint(0, 39))]
        blocks.append(D.dynamic_block(t, ll, dl, final=k == 299, bits=b, header=("rle", "plain", "long", "min")[k % 4]))
        toks += t
    return _finish("tiny_blocks", b, toks, blocks)


@functools.lru_cache(maxsize=None)
def valid():
    """every valid stream, by name"""
    cases = [wide_tokens()] + [_wide_placed("wide_tokens/%d bits in front of a boundary" % off, off) for off in (1, 47, 48)]
    cases += worst_tables() + random_code_streams() + single_code_forms() + [headers(), tiny_blocks()]
    assert len({c.name for c in cases}) == len(cases)
    return cases


# ---- failing streams --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deep_prefix():
    """more than 8 KiB of ordinary dynamic blocks for an error to stand behind: (_Bits, tokens, block starts)"""
    rng = random.Random(1300)
    b, toks, blocks = D._Bits(), [], []
    for k in range(3):
        ll, dl = random_codes(rng, k == 1)
        t = rand_tokens(rng, 3000, ll, dl, n0=len(D.expand(toks)), p_match=0.05)
        blocks.append(D.dynamic_block(t, ll, dl, final=False, bits=b))
        toks += t
    assert D._pos(b) > 8 * 8300
    return b, toks, blocks


SMALL_LITS = [0x41, 0x42, 0x43, 0x44, 0x45, 0x46]


def small_codes():
    """codes with a header of a few bytes, for the errors that stand inside the first 200 bytes of a stream"""
    return D.comb(SMALL_LITS + [256, 257, 258, 285], 286), D.comb([0, 1, 2, 3, 4, 5, 6, 7], 30)


def _failing_pair(klass, build):
    """the error behind the deep prefix and inside the first 200 bytes: build(b, rng, deep) appends the bad block(s) to b and returns
    the bit position of the bad code (None: the error is no single code); 200 bytes of zeros follow; then the same streams cut 1, 2 and 14 bits behind the start of the bad code"""
    out = []
    for deep in (True, False):
        for align in (None, 1, 2, 14):
            pb, ptoks, pblocks = _deep_prefix() if deep and not getattr(build, "own_prefix", False) else (D._Bits(), [], [])
            for pad in range(64):
                rng = random.Random(1400)
                b = _clone(pb)
                if pad:                                             # a few literals in a block of their own move the error by `pad` codes
                    ll, dl = small_codes()
                    D.dynamic_block([SMALL_LITS[0]] * pad, ll, dl, final=False, bits=b)     # (its code is 1 bit long)
                bad = build(b, rng, deep, len(D.expand(ptoks)) + pad)
                if align is None or bad is None or (bad + align) % 8 == 0:
                    break
            else:
                raise AssertionError((klass, align))
            if bad is None and align is not None:
                continue
            b.put(0, 1600)
            s = b.finish()
            if align is not None:
                s = s[:(bad + align) // 8]
            name = "%s/%s%s" % (klass, "deep" if deep else "early", "" if align is None else "/cut %d bits in" % align)
            assert deep or bad is None or bad < 8 * 200, (name, bad)
            assert not deep or bad is None or bad > 8 * 8192
            out.append(Case(name, s, None, pblocks, klass=klass, bad=bad))
    return out


def _bad_one_distance(b, rng, deep, before=0):
    toks, ll, dl = _one_dist(rng, 20)
    if not deep:
        ll, toks = small_codes()[0], [SMALL_LITS[0], (3, 1), SMALL_LITS[1]]
    D.dynamic_block(toks, ll, dl, final=True, bits=b, eob=False)
    b.put_code(D.canonical(ll)[257], ll[257])                        # length 3 ...
    bad = D._pos(b)
    b.put(1, 1)                                                      # ... and the unused code of the one-symbol distance code
    return bad


def _bad_only_eob(b, rng, deep, before=0):
    D.dynamic_block([], ONLY_EOB, [0], final=True, bits=b, eob=False)
    bad = D._pos(b)
    b.put(1, 1)                                                      # the unused half of the single literal/length code
    return bad


def _bad_fixed(sym):
    def build(b, rng, deep, before=0):
        b.put(1, 1)
        b.put(1, 2)                                                  # a fixed block: its codes 286, 287 (and distance 30, 31) exist, and are errors
        D.put_fixed(b, [0x41, 0x42, 0x43], eob=False)
        if sym >= 286:
            bad = D._pos(b)
            b.put_code(*D._lit_code(sym))
        else:
            b.put_code(*D._lit_code(257))
            bad = D._pos(b)
            b.put_code(sym, 5)
        return bad
    return build


def _bad_far(extra, n_out=20000, hist=0):
    """a match whose distance is the number of bytes in front of it (+ extra: one more is too far back), at output position n_out
    (early: 5) of a stream of its own: the 20 000 bytes in deep codes are more than 8 KiB of input by themselves"""
    def build(b, rng, deep, before=0):
        if deep:
            want = n_out - before
            ll, dl = random_codes(rng, True)
            toks = rand_tokens(rng, want + 1, ll, dl, p_match=0.1)
            n, k = 0, 0
            while n + (1 if isinstance(toks[k], int) else toks[k][0]) <= want:
                n += 1 if isinstance(toks[k], int) else toks[k][0]
                k += 1
            toks = toks[:k] + [toks[0]] * (want - n)
        else:
            ll, dl = small_codes()
            toks = [SMALL_LITS[k % 6] for k in range(5)]
        D.dynamic_block(toks, ll, dl, final=True, bits=b, eob=False)
        bad = D._pos(b)
        tail = [(17 if deep else 3, before + len(D.expand(toks)) + hist + extra), next(s for s in range(256) if ll[s])]
        D.put_tokens(b, tail, ll, dl)
        build.toks = toks + (tail if extra == 0 else [])
        return bad
    build.own_prefix = True
    return build


def _bad_lengths(which):
    def build(b, rng, deep, before=0):
        ll, dl = random_codes(rng, deep) if deep else small_codes()
        ll, dl = list(ll), list(dl)
        if which == "no end-of-block":
            ll[256] = 0
        elif which == "literal/length over-subscribed":
            i = max(range(256), key=lambda s: ll[s])
            ll[i] -= 1
        elif which == "literal/length incomplete":
            i = max(range(256), key=lambda s: ll[s])
            ll[i] += 1 if ll[i] < 15 else -15
        elif which == "distance over-subscribed":
            i = max(range(len(dl)), key=lambda s: dl[s])
            dl[i] -= 1
        elif which == "distance incomplete":
            i = max(range(len(dl)), key=lambda s: dl[s])
            dl[i] += 1 if dl[i] < 15 else -15
        D.dynamic_block([], ll, dl, final=True, bits=b, eob=False)
        return None
    return build


def _bad_repeat(which):
    def build(b, rng, deep, before=0):
        hdr = [(16, 0, 2), (8, 0, 0)] if which == "first" else [(8, 0, 0)] * 200 + [(18, 127, 7)]      # 200 + 138 > 257 + 1
        b.put(1, 1)
        b.put(2, 2)
        b.put(0, 5)
        b.put(0, 5)
        cl = [0] * 19
        cl[8], cl[16 if which == "first" else 18] = 1, 1
        hclen = max(i + 1 for i in range(19) if cl[D._ORDER[i]])
        b.put(hclen - 4, 4)
        for i in range(hclen):
            b.put(cl[D._ORDER[i]], 3)
        cc = D.canonical(cl)
        bad = None
        for s, v, n in hdr:
            if s >= 16:
                bad = D._pos(b)
            b.put_code(cc[s], cl[s])
            b.put(v, n)
        return bad
    return build


def _bad_raw_header(bits):
    def build(b, rng, deep, before=0):
        for v, n in bits:
            b.put(v, n)
        return None
    return build


# The two "unused code" classes: the reference's table gives the unused half of a single-code form, and both entries of a code with
# no symbol, an invalid entry of ONE bit (zlib-rs/src/inflate/inftrees.rs:61-67 and :230-241), and its lookup loops break once
# here.bits <= bits_in_buffer (inflate.rs:640-652, :747-758).  So the error is reported with one bit in hand and one bit is read: the
# cuts 1, 2 and 14 bits behind the start of such a pattern are data errors like the uncut streams, not requests for more input.
CLASSES = {
    "unused code of a one-symbol distance code": (_bad_one_distance, "distance code"),
    "unused code of the only-end-of-block code": (_bad_only_eob, "literal/length code"),
    "fixed block, length symbol 286": (_bad_fixed(286), "literal/length code"),
    "fixed block, length symbol 287": (_bad_fixed(287), "literal/length code"),
    "fixed block, distance symbol 30": (_bad_fixed(30), "distance code"),
    "fixed block, distance symbol 31": (_bad_fixed(31), "distance code"),
    "distance one too far back": (_bad_far(1), "distance too far back"),
    "no end-of-block code": (_bad_lengths("no end-of-block"), "missing end-of-block"),
    "literal/length code over-subscribed": (_bad_lengths("literal/length over-subscribed"), "literal/lengths set"),
    "literal/length code incomplete": (_bad_lengths("literal/length incomplete"), "literal/lengths set"),
    "distance code over-subscribed": (_bad_lengths("distance over-subscribed"), "distances set"),
    "distance code incomplete": (_bad_lengths("distance incomplete"), "distances set"),
    "repeat with no length in front": (_bad_repeat("first"), "bit length repeat"),
    "repeat past the last length": (_bad_repeat("past"), "bit length repeat"),
    # HCLEN 4: only 16, 17, 18 and 0 can have codes, so every length is 0
    "all lengths zero, HCLEN 4": (_bad_raw_header([(1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (0, 3), (0, 3), (1, 3), (1, 3), (127 << 1 | 1, 8),
                                                   (109 << 1 | 1, 8)]), "missing end-of-block"),
    "one-symbol code-length code": (_bad_raw_header([(1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (0, 3), (0, 3), (1, 3), (0, 3)]), "code lengths set"),
    "HLIT 30": (_bad_raw_header([(1, 1), (2, 2), (30, 5), (0, 5), (0, 4)]), "too many symbols"),
    "HDIST 31": (_bad_raw_header([(1, 1), (2, 2), (0, 5), (31, 5), (0, 4)]), "too many symbols"),
}


@functools.lru_cache(maxsize=None)
def failing():
    """every failing stream; klass names the class, CLASSES[klass][1] the kind the uncut streams of the class must stop with"""
    out = []
    for klass, (build, _) in CLASSES.items():
        out += _failing_pair(klass, build)
    out.append(_wide_placed("wide_tokens/the last 48-bit token ends with the input", 1, cut_at_last=True))
    assert len({c.name for c in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def exact_distance():
    """the valid half of the too-far-back pair: the distance is exactly the number of bytes produced (deep: 20 000, early: 5)"""
    out = []
    for deep in (True, False):
        f = _bad_far(0)
        b = _clone(_deep_prefix()[0]) if deep else D._Bits()
        f(b, random.Random(1400), deep)
        toks = (_deep_prefix()[1] if deep else []) + f.toks
        out.append(Case("distance equal to the bytes produced/%s" % ("deep" if deep else "early"), b.finish(), D.expand(toks)))
    return out


@functools.lru_cache(maxsize=None)
def history_pairs():
    """the pair with 32 and with 32 768 bytes of history in front: [(valid Case, failing Case or None)], hist = the history.
    With 32 bytes the match stands at output position 20 000.  With 32 768 it is the block's first token: 32 768 is the farthest
    a distance reaches, so the failing half of that pair is the same stream with one byte of history less (resume_exact)."""
    out = []
    for nh in (32, 32768):
        hist = random.Random(1500 + nh).getrandbits(8 * nh).to_bytes(nh, "little")
        pair = []
        for extra in ((0, 1) if nh == 32 else (0,)):
            f = _bad_far(extra, n_out=0 if nh == 32768 else 20000, hist=nh)
            b = D._Bits()
            f(b, random.Random(1501), True)
            if extra == 0:
                full = D.expand(list(hist) + f.toks)
                pair.append(Case("history %d/exact" % nh, b.finish(), full[nh:], hist=hist))
            else:
                pair.append(Case("history %d/one too far" % nh, b.finish(), None, klass="distance one too far back", hist=hist))
        out.append(tuple(pair + [None])[:2])
    return out


# ---- the expected words of a stream, from inflate_ref -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(stream, cap, hist=b""):
    return D.inflate_ref(stream, cap, 0, hist)


AMPLE = 4 << 20


def expected(case, cap=AMPLE):
    """(status, bytes, bytes used, kind) of inflate_ref"""
    st, out, bits, kind = _ref(case.stream, cap, case.hist)
    return st, out, (bits + 7) // 8, kind


# ---- the checks -------------------------------------------------------------------------------------------------------------------------
def _oracle(o, stream, cap):
    rc, out, used, msg = o.inflate(stream, cap, RAW)
    return (0 if rc == 1 else rc), out, used, msg


def batch_cases():
    return valid() + exact_distance() + failing()


ONE_BY_ONE = ["wide_tokens", "worst_tables/17000/1", "single_code/one distance code of length 1/6000", "tiny_blocks",
              "headers", "random_codes/tokens/deep/4", "unused code of a one-symbol distance code/deep", "distance one too far back/deep"]


def batch_exact(inflate_fn, o):
    """zmi_inflate_batch: every stream in one launch of more than 16 streams (the one-wave kernel under "onewave", the multi-wave
    kernel under "product"), then eight of them one by one (the 16-wave kernel with INF_MW_SUB shares).  Status = the oracle's; the
    bytes where it is 0; for a failing stream the produced prefix is the oracle's, in length and in bytes.  Capacities: ample (the
    failing streams), exact, one short, and for wide_tokens also len - 258, len - 257 and 1: the oracle's code."""
    cases = batch_cases()
    assert len(cases) > 16
    streams = [c.stream for c in cases]
    caps = [len(c.raw) if c.raw is not None else len(expected(c)[1]) + 600 for c in cases]
    outs, st = inflate_fn(streams, caps, RAW)
    for c, cap, out, s in zip(cases, caps, outs, st):
        rc, want, _, msg = _oracle(o, c.stream, cap)
        assert int(s) == rc, (c.name, int(s), rc, msg)
        assert (rc == 0) == (c.raw is not None), (c.name, rc, msg)
        assert out == want, (c.name, len(out), len(want))          # (a failing stream: the produced prefix, in length and in bytes)
        if rc == 0:
            assert out == c.raw, c.name
    by = {c.name: c for c in cases}
    for name in ONE_BY_ONE:
        c = by[name]
        cap = len(c.raw) if c.raw is not None else len(expected(c)[1]) + 600
        rc, want, _, msg = _oracle(o, c.stream, cap)
        outs, st = inflate_fn([c.stream], [cap], RAW)
        assert int(st[0]) == rc and outs[0] == want and (rc != 0 or want == c.raw), (name, int(st[0]), rc, msg, len(outs[0]), len(want))
    # too little room
    good = [c for c in cases if c.raw]
    caps = [len(c.raw) - 1 for c in good]
    extra = [(by["wide_tokens"], len(by["wide_tokens"].raw) - k) for k in (258, 257)] + [(by["wide_tokens"], 1)]
    outs, st = inflate_fn([c.stream for c in good] + [c.stream for c, _ in extra], caps + [k for _, k in extra], RAW)
    for (c, cap), s in zip(list(zip(good, caps)) + extra, st):
        rc, _, _, msg = _oracle(o, c.stream, cap)
        assert rc == Z_BUF_ERROR and int(s) == rc, (c.name, cap, int(s), rc, msg)
    return len(cases)


SHIFTS = (0, 1, 3, 15)


def words_exact(target, o, shifts=SHIFTS):
    """zmi_inflate_batch_dev_ex, zmi_inflate_sizes_dev and zmi_inflate_batch_packed_dev on the same streams, every stream 0, 1, 3 and
    15 bytes behind a 16-byte boundary (the size pass; the two decodes place their input themselves).  A valid stream: (size,
    status, in_used, detail) = (len(raw), 0, len(stream), 0).  A failing stream: status and size are inflate_ref's and the oracle's,
    in_used the oracle's bytes used, detail the fixed map DETAIL from inflate_ref's kind -- the library's own batch call is not the
    judge here.  (Every kind these streams stop with has a word in DETAIL; the two "invalid code" kinds share DE_CODE.)"""
    cases = batch_cases()
    streams = [c.stream for c in cases]
    want = []
    for c in cases:
        st, out, used, kind = expected(c)
        rc, oout, oused, msg = _oracle(o, c.stream, AMPLE)
        assert (st, out, used) == (rc, oout, oused) and msg == MESSAGE.get(kind), (c.name, st, rc, used, oused, kind, msg)
        want.append((len(out), st, used, DETAIL[kind] if kind else 0))
        if c.raw is not None:
            assert want[-1] == (len(c.raw), 0, len(c.stream), 0), c.name
    names = [c.name for c in cases]

    def same(words, what):
        bad = [(n, w, x) for n, w, x in zip(names, words, want) if w.key() != x]
        assert not bad, (what, len(bad), bad[:8])

    for shift in shifts:                        # (None: the four shifts dealt out over the streams of one call, the emulator's subset)
        at = [SHIFTS[i % 4] for i in range(len(streams))] if shift is None else [shift] * len(streams)
        same(target.sizes(streams, RAW, shifts=at), "sizes, shift %s" % shift)
    sizes = [w[0] for w in want]
    ref = target.batch(streams, RAW, [s + 600 if w[1] else s for s, w in zip(sizes, want)])
    assert ref.rc == 0 and ref.guard_ok
    same(ref.words, "batch")
    p = target.packed(streams, RAW, sum(sizes))
    assert p.rc == 0 and p.guard_ok
    same(p.words, "packed")
    for i, c in enumerate(cases):
        assert p.piece(i) == expected(c)[1] == ref.piece(i), c.name
    return len(cases)


def resume_exact(e):
    """zmi_inflate_resume on `headers` and `wide_tokens` with room for about a third of the output, restarted from the reported
    checkpoint until done: the concatenation is the expected bytes and every checkpoint is one of the crafter's block starts (byte
    and bit).  Then the too-far-back pair with 32 and 32 768 bytes of history: the distance that reaches the first history byte
    decodes, one more is the data error, with inflate_ref's bytes and positions."""
    by = {c.name: c for c in valid()}
    done = 0
    for name in ("headers", "wide_tokens"):
        c = by[name]
        room = len(c.raw) // 3 + 1
        out, byte, bit, calls = bytearray(), 0, 0, 0
        while True:
            hist = bytes(out[-32768:])
            got, st, det, used, res = e.inflate_resume(c.stream[byte:], bit, hist, cap=room)
            calls += 1
            assert calls < 40, name
            if st == 0:
                out += got
                assert res[3] == 1 and used == len(c.stream) - byte
                break
            assert (st, det) == (Z_BUF_ERROR, 2), (name, st, det)
            at = 8 * (byte + res[0]) + res[1]
            assert at in c.blocks and res[3] == 0, (name, at)
            assert got[:res[2]] == c.raw[len(out):len(out) + res[2]]
            if res[2] == 0 and at == 8 * byte + bit:
                room *= 2                                     # (a block larger than the room: wide_tokens is one block)
            out += got[:res[2]]
            byte, bit = at >> 3, at & 7
        assert bytes(out) == c.raw, name
        done += calls
    for good, bad in history_pairs():
        want = D.inflate_ref(good.stream, AMPLE, 0, good.hist)
        assert want[0] == 0 and want[1] == good.raw
        got, st, det, used, res = e.inflate_resume(good.stream, 0, good.hist, cap=len(good.raw) + 64)
        assert (st, det, got, used, res[3]) == (0, 0, good.raw, len(good.stream), 1), (good.name, st, det)
        if bad is not None:
            st0, out0, bits0, kind0 = D.inflate_ref(bad.stream, AMPLE, 0, bad.hist)
            assert (st0, kind0) == (Z_DATA_ERROR, "distance too far back") and out0 == good.raw[:len(out0)]
            got, st, det, used, res = e.inflate_resume(bad.stream, 0, bad.hist, cap=len(good.raw) + 64)
            assert (st, det, got) == (Z_DATA_ERROR, DETAIL[kind0], out0), (bad.name, st, det, len(got), len(out0))
        # the valid stream with one byte of history less reaches in front of it
        st0, out0, bits0, kind0 = D.inflate_ref(good.stream, AMPLE, 0, good.hist[1:])
        assert (st0, kind0) == (Z_DATA_ERROR, "distance too far back") and out0 == good.raw[:len(out0)]
        got, st, det, used, res = e.inflate_resume(good.stream, 0, good.hist[1:], cap=len(good.raw) + 64)
        assert (st, det, got) == (Z_DATA_ERROR, DETAIL[kind0], out0), (good.name, st, det)
        done += 3
    return done


def scan_exact(ctx, e):
    """zmi_stream_find_blocks_dev(stream, raw, min_gap 1) on `headers` and `tiny_blocks`: exactly the crafter's block starts behind
    the first, as in test_proposals_are_exact (the seeds above give no false header; the scan finds true blocks only, so a false
    one would show as an extra entry here).  Then zmi_inflate_blocks (which scans for itself) and zmi_inflate_stream_bits_dev with
    those proposals against zmi_inflate_resume on the same arguments, for `headers` and two failing streams.  zmi_inflate_blocks:
    status, detail, length, in_used, bytes and checkpoint are zmi_inflate_resume's.  zmi_inflate_stream_bits_dev on the valid stream:
    all five words and the bytes.  On a failing stream it decodes piece by piece and keeps whole pieces only (include/zmi355.h), so:
    its status is zmi_inflate_resume's; its detail is ZMI_SI_DATA for the bad code and ZMI_SI_FAR for the distance too far back,
    with the index of the piece that holds the error; its length is the output in front of that piece -- what zmi_inflate_resume
    reports as the checkpoint of a stop at that block boundary -- and its bytes are zmi_inflate_resume's up to there.  Its in_used
    is not compared on a failing stream: the call defines it for a stream that ended (header + data + trailer) and reports 0."""
    by = {c.name: c for c in valid() + failing()}
    for name in ("headers", "tiny_blocks"):
        c = by[name]
        got = ctx.find_blocks(c.stream, RAW, 1)
        assert got == [0] + c.blocks[1:], (name, len(got), len(c.blocks))
    done = 0
    si = {"headers": 0, "unused code of a one-symbol distance code/deep": 5, "distance one too far back/deep": 6}
    for name in si:
        c = by[name]
        cap = len(expected(c)[1]) + 600
        want = e.inflate_resume(c.stream, 0, b"", cap=cap)
        got = e.inflate_blocks(c.stream, 0, b"", cap=cap)
        assert got[:5] == want, (name, want[1:], got[1:])
        assert (want[1], want[0], want[3]) == expected(c)[:3], (name, want[1], want[3])
        cuts = ctx.find_blocks(c.stream, RAW, 1)
        # (a failing stream records the blocks in front of the bad one; the bad block's header is a true header too)
        assert (cuts if c.raw is not None else cuts[:max(1, len(c.blocks))]) == [0] + c.blocks[1:], (name, cuts, c.blocks)
        st, det, olen, used, out, canary = ctx.inflate_bits(c.stream, RAW, cuts, 1 << 20, cap)
        assert canary and st == want[1], (name, st, det)
        if c.raw is not None:
            assert (st, det, olen, used, out) == (0, 0, len(c.raw), len(c.stream), c.raw), (name, st, det, olen, used)
        else:
            piece = len(cuts) - 1                                # the error stands in the last block
            assert (det & 0xFF, det >> 8) == (si[name], piece), (name, det)
            front = 0
            if piece:
                stop = e.inflate_resume(c.stream, piece << 8, b"", cap=cap)          # stop behind `piece` complete blocks
                assert (stop[1], stop[2]) == (Z_BUF_ERROR, 3) and 8 * stop[4][0] + stop[4][1] == cuts[piece], (name, stop[1:])
                front = stop[4][2]
            assert olen == front and out == want[0][:front], (name, olen, front)
        done += 1
    return done

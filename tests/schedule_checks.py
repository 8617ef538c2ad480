"""Is the compressed output a function of the input and the level alone -- not of how the waves of the match search (csrc/lz77.hip:
producer waves that build the hash chains, searcher waves that claim positions, LDS flags and spin waits between them) happen to be
scheduled?  Shared by tests/test_emu_schedule.py (CPU: the emulator build under perturbed schedules, tests/emu/hip_emu.h
ZMI_EMU_SCHED) and tests/test_gpu_schedule.py (the MI355X: repeated calls, producer counts, and the emulator's bytes), both through
zmi_deflate_batch_dev on buffers a `mem` object owns (put / full / read / stream, as in tests/bgzf_checks.py).

The judge of a stream is zlib.decompress; the judge of invariance is byte equality.  tests/golden/deflate_digests.json holds length
and SHA-256 of the emulator's stream per (input, level) for the set of inputs(); tools/make_deflate_digests.py writes it.  The
emulator test asserts that the emulator reproduces the file, the GPU test that the device does: the device and the emulator run the
same algorithm, so a pull request that changes compressed bytes regenerates the file, and one that claims "output unchanged" is
checked by it."""
import ctypes as C
import functools
import hashlib
import json
import os
import zlib

import numpy as np

import bgzf_checks as B
import oracle_lib
import parity_checks

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "golden", "deflate_digests.json")
WRAP_ZLIB = 1

LEVELS = [1, 2, 3, 6, 9]
PRODUCERS = [None, "1", "2", "3", "4"]             # ZMI_PRODUCERS (read per call under ZMI_TUNING); None: the product's count
# hold:<wave>:<from_pass>:<passes> / seed:<s>[:<permille>], tests/emu/hip_emu.h.  Wave 0 is a producer at every count, waves 1 and 2
# are producers or searchers, wave 3 is a searcher below four producers.  A hold from pass 1 stands in front of the block's first
# barrier (nobody starts); the long holds from pass 3 stop one wave in the steady state while the others run on until they need it:
# with the parent commit's lz77.hip hold:3:3:3000 at three producers and seed:3:500 / seed:6:800 at four / three changed the bytes of
# the 40 000-byte text (a producer hashed the first 16 positions of a tile before the chunk of the round before last was in the ring).
HOLDS = ["hold:0:1:1", "hold:0:1:50", "hold:1:1:5", "hold:2:1:5", "hold:2:3:3000", "hold:3:3:3000"]
SEEDS = ["seed:1", "seed:2", "seed:3:500", "seed:6:800"]
SCHEDULES = [None] + HOLDS + SEEDS


@functools.lru_cache(maxsize=None)
def text():
    return dict(parity_checks.real_fixtures())["lcet10.txt"]


@functools.lru_cache(maxsize=None)
def inputs():
    """[(name, bytes)] in batch order.  Cuts of lcet10.txt: one tile of the search (1024 positions) and four, each also with a partial
    last tile (+17), and two that cross the wrap of the 32 KiB ring; the 4113-byte cut a second time (layout() puts it at an unaligned
    address); two classes of the benchmark's generator; a long run in front of text."""
    t, o = text(), oracle_lib.load(rebuild=False)
    out = [("lcet10[:%d]" % n, t[:n]) for n in (1024, 1041, 4096, 4113, 40000, 65280)]
    out.append(("lcet10[:4113] unaligned", t[:4113]))
    out.append(("gen_shard(3, 40000)", o.gen_shard(3, 40000)))
    out.append(("gen_shard(4, 32768)", o.gen_shard(4, 1 << 15)))
    out.append(("zeros(5000) + lcet10[:3000]", bytes(5000) + t[:3000]))
    return out


def layout(shards, unaligned=6):
    """-> (blob, offsets): the shards one behind the other from offset 0 of a 16-byte aligned buffer; shard `unaligned` starts at
    an address that is 7 modulo 16 (the search's 16-byte loads take their byte path there)"""
    blob, offs = bytearray(), []
    for i, s in enumerate(shards):
        if i == unaligned:
            blob += b"\xEE" * ((7 - len(blob)) % 16)
        offs.append(len(blob))
        blob += s
    assert unaligned >= len(shards) or offs[unaligned] % 16 == 7
    return bytes(blob), offs


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = B.bind(L), ctx, mem

    def deflate(self, shards, level, offs_blob=None, wrap=WRAP_ZLIB):
        """one zmi_deflate_batch_dev call -> the streams"""
        m, n = self.mem, len(shards)
        blob, offs = offs_blob if offs_blob else layout(shards, unaligned=n)
        lens = [len(s) for s in shards]
        stride = int(self.L.zmi_deflate_bound(max(lens), wrap))
        inp = m.put(np.frombuffer(blob + b"\0" * 16, dtype=np.uint8), 0)
        out, ol, st = m.full(n * stride, 0), m.full(4 * n, 0), m.full(4 * n, 0x77)
        od, ld = m.put(np.array(offs, dtype=np.uint64)), m.put(np.array(lens, dtype=np.uint32))
        rc = self.L.zmi_deflate_batch_dev(self.ctx, inp.ptr, od.ptr, ld.ptr, n, max(lens), level, 0, wrap, out.ptr, stride, ol.ptr, st.ptr, m.stream)
        assert rc == 0, self.L.zmi_last_error()
        assert (m.read(st, np.int32)[:n] == 0).all()
        host, l = m.read(out, np.uint8), m.read(ol, np.uint32)
        return [host[i * stride:i * stride + int(l[i])].tobytes() for i in range(n)]

    def golden_set(self, level):
        """the streams of inputs() at one level, every one inflated by zlib back to its input"""
        shards = [b for _, b in inputs()]
        comp = self.deflate(shards, level, layout(shards))
        for (name, raw), c in zip(inputs(), comp):
            assert zlib.decompress(c) == raw, (name, level)
        return comp


def setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def digest(stream):
    return {"bytes": len(stream), "sha256": hashlib.sha256(stream).hexdigest()}


def digests_of(target, levels=LEVELS):
    """{level: {input name: {"bytes", "sha256"}}} of the target's streams"""
    return {str(level): {name: digest(c) for (name, _), c in zip(inputs(), target.golden_set(level))} for level in levels}


def load_digests():
    with open(DIGESTS) as f:
        doc = json.load(f)
    assert doc["wrap"] == WRAP_ZLIB and doc["levels"] == LEVELS and doc["inputs"] == [[name, len(b)] for name, b in inputs()]
    return doc["digests"]


def check_digests(target, levels=LEVELS):
    """the target's streams are the committed ones"""
    want, got = load_digests(), digests_of(target, levels)
    for level in levels:
        for name, _ in inputs():
            assert got[str(level)][name] == want[str(level)][name], (level, name, got[str(level)][name], want[str(level)][name])
    return len(levels) * len(inputs())


def differing(a, b, names):
    """(name, bytes in a, bytes in b) of the streams that differ: what a failing comparison reports"""
    return [(name, len(x), len(y)) for name, x, y in zip(names, a, b) if x != y]


# ---- the emulator under perturbed schedules -----------------------------------------------------------------------------------------------
def schedule_invariance(target, level, producers=PRODUCERS, schedules=SCHEDULES):
    """for every input: the same bytes under every schedule and every producer count -> the number of calls compared"""
    names = [name for name, _ in inputs()]
    first, done = None, 0
    try:
        for p in producers:
            setenv("ZMI_PRODUCERS", p)
            for sched in schedules:
                setenv("ZMI_EMU_SCHED", sched)
                comp = target.golden_set(level)
                first = first or comp
                assert comp == first, (level, p, sched, differing(first, comp, names))
                done += 1
    finally:
        setenv("ZMI_PRODUCERS", None)
        setenv("ZMI_EMU_SCHED", None)
    return done


# ---- the device: repeated calls and producer counts -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_sets():
    """{name: shards}: the inputs of profiles/bgzf_level1_reproducibility.txt (text of 3 x 65 280 + 17 bytes cut at 65 280, 48 text shards
    of 4096 bytes), the eight classes of the benchmark's generator at 256 KiB, and ragged sizes"""
    o = oracle_lib.load(rebuild=False)
    return {"4 x 65280": B.cut(B.make("text", 3 * 65280 + 17), 65280), "48 x 4096": B.cut(B.make("text", 48 * 4096), 4096),
            "8 classes": [o.gen_shard(c, 1 << 18) for c in range(8)], "ragged": [text()[:n] for n in (1, 65, 4097, 70001)]}


def repeat_calls(target, level, calls=5):
    """five calls give the same bytes (checked once to be streams of the input) -> {set name: streams}"""
    out = {}
    for name, shards in device_sets().items():
        first = target.deflate(shards, level)
        for raw, c in zip(shards, first):
            assert zlib.decompress(c) == raw, (name, level)
        for k in range(1, calls):
            again = target.deflate(shards, level)
            assert again == first, (name, level, k, [i for i, (x, y) in enumerate(zip(first, again)) if x != y])
        out[name] = first
    return out


def producer_counts(target, level, counts=("1", "2", "3", "4")):
    """the bytes do not depend on the number of producer waves -> calls compared"""
    done = 0
    try:
        setenv("ZMI_PRODUCERS", None)
        want = {name: target.deflate(shards, level) for name, shards in device_sets().items()}
        for p in counts:
            setenv("ZMI_PRODUCERS", p)
            for name, shards in device_sets().items():
                got = target.deflate(shards, level)
                assert got == want[name], (name, level, p, [i for i, (x, y) in enumerate(zip(want[name], got)) if x != y])
                done += 1
    finally:
        setenv("ZMI_PRODUCERS", None)
    return done

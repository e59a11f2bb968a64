"""Small streams drawn BY DESIGN under a foreign codebook, through every producer and consumer of a
packed stream, against the plain host model (tests/ref_stream.py): hz_pack's payload and block
index, hz_index_build, hz_index_expand, hz_decode, hz_decode_indexless (whole and a prefix), the
split parts hz_indexless_scan / _refix / _decode, and hz_decode_range from the seek table and from
the full index. hz_pack and the decoders take any uploaded prefix code, so a few thousand symbols
chosen for their lengths reach what natural data reaches only at tens of gigabytes: blocks of
2048 x 56 bits (the largest decode slot), blocks past 65 536 bits in every consumer
(dec_chain_offsets' rebuild), 35..56-bit codes through the index-less walk, the pack's slot overflow,
cold list and direct path, chains past the stream's end, and prefix codes that never resynchronise.
One test walks every ordered pair of the five table classes on one context (what a re-upload must
reset or re-alias), not left to the order of the cases.

Every device result is compared with the model (never only with another device result); every
output and index buffer sits between 64-byte guards of 0xA5. A device-side status at hz_ctx_sync
counts as a failure of the check that raised it.

Run as a script (`python tests/test_gpu_designed_streams.py pipe`) it runs the fib57, hot25,
dense16 and zipf21 cases once and prints "ok": the tests start it in a fresh process per HZ_DEC_PIPE value,
which the library reads once.

Tolerance: none -- every check is bit-exact."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_stream  # noqa: E402
import table_model  # noqa: E402
from table_books import book  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 2048
GUARD = 64
HZ_EHIP = -3
UNKNOWN_ENTRY = (1 << 64) - 1
LEAD_BITS = 1024  # HZ_INDEXLESS_LEAD_BITS

BOOKS = ["fib57", "fib41", "hot25", "dense16", "dense12", "even", "fixed16", "zipf21", "sq32"]
FULL_BOOKS = ["zipf21", "sq32"]   # whole 65 536-symbol alphabets: the benchmark's table classes (tests/table_books.py)
KINDS = ["longest", "shortest", "blocks", "chains", "uniform"]
FULL_KINDS = ["sweep", "escapes"]  # the kinds of the full books only
EDGE_SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 3 * BLK + 5]
START_BITS = [0, 5, 31, 32, 45]
WAVES = 40 * BLK + 777       # about 40 blocks and a ragged tail: several waves
ALL_CUS = 600 * BLK + 1234   # about 600 blocks: every CU (below 2^21 symbols)
SWEEP = 2 * 65536 + 5        # a full book's sweep: the alphabet twice and a ragged tail, about 64 blocks


# ---- codebooks: tests/table_books.py (book(name) -> name, cb, ln, code) --------------------------
# ---- streams ----------------------------------------------------------------------------------
def _stream(bk, kind, nsym, rng):
    """u16 symbols drawn by design, not from the codebook's histogram."""
    alphabet = np.nonzero(bk.ln)[0].astype(np.uint16)
    lens = bk.ln[alphabet].astype(np.int64)
    eighth = np.sort(lens)[::-1][min(7, lens.size - 1)]
    longest = alphabet[lens >= eighth]          # the (at least) eight longest codes
    maxlen = alphabet[lens == lens.max()]
    shortest = alphabet[lens == lens.min()]
    draw = lambda pool, n: pool[rng.integers(0, pool.size, n)]  # noqa: E731
    i = np.arange(nsym)
    if kind == "longest":
        sym = draw(longest, nsym)
        sym[:BLK] = draw(maxlen, min(nsym, BLK))    # and one block of the longest code alone: 2048 x max_len bits
    elif kind == "shortest":
        sym = draw(shortest, nsym)
    elif kind == "blocks":      # whole blocks alternating longest and shortest
        sym = np.where((i // BLK) % 2 == 0, draw(longest, nsym), draw(shortest, nsym))
    elif kind == "chains":      # alternation inside the 8-symbol chains, the phase flipping every chain
        sym = np.where((i + i // 8) % 2 == 0, draw(longest, nsym), draw(shortest, nsym))
    elif kind == "uniform":
        sym = draw(alphabet, nsym)
    elif kind == "sweep":
        # the whole alphabet once in a seeded permutation (every symbol, followed by arbitrary codes), then
        # again sorted by code length, descending (whole blocks of only-longest codes from thousands of
        # distinct symbols, every symbol followed by a long code), and a ragged tail
        by_len = alphabet[np.argsort(-lens, kind="stable")]
        sym = np.concatenate([rng.permutation(alphabet), by_len, by_len[:5]])
        assert sym.size == nsym == 2 * alphabet.size + 5
    elif kind == "escapes":
        pool = escape_pool(bk)
        sym = draw(pool if pool.size else longest, nsym)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(sym, dtype="<u2")


def escape_pool(bk):
    """The symbols that sit on the tables' rare paths: they resolve past level 1 of the decode LUT (codes
    longer than its 13 bits) and, under a HOT book, also miss their slot (tests/table_model.py's ownership
    rule under its own choice of the pairing mask). Empty for the older books: `escapes` is `longest` there."""
    if bk.name not in FULL_BOOKS:
        return np.zeros(0, np.uint16)
    ln = bk.ln
    past = ln > table_model.K_DEC_LUT_MAX_K1
    if int(ln.max()) <= table_model.K_HOT_MAX_LEN:    # ENC_HOT
        miss = [table_model.hot_miss_mass(ln, m) for m in table_model.HOT_MASKS]
        past &= ~table_model.hot_owner(ln, table_model.HOT_MASKS[int(np.argmin(miss))])
    pool = np.nonzero(past)[0].astype(np.uint16)
    assert pool.size >= 1000, (bk.name, pool.size)
    return pool


def _lead(start_bit):
    k = start_bit % 32
    return ((0x15a5f3c7 & ((1 << k) - 1)) | 1) if k else 0


def _cases():
    out = []
    # every codebook meets every stream kind
    for bi, b in enumerate(BOOKS):
        for ki, kind in enumerate(KINDS):
            nsym = WAVES if kind in ("blocks", "uniform") else 3 * BLK + 5
            out.append((b, kind, nsym, START_BITS[(bi + ki) % 5]))
    # every size edge and every start bit with fib57, hot25 and dense16
    for bi, b in enumerate(("fib57", "hot25", "dense16")):
        for si, nsym in enumerate(EDGE_SIZES):
            case = (b, KINDS[(si + bi) % 5], nsym, START_BITS[(si + 2 * bi) % 5])
            if case not in out:
                out.append(case)
        out.append((b, "blocks", ALL_CUS, START_BITS[(3 + bi) % 5]))
    # the full books meet the two kinds of their own as well
    for bi, b in enumerate(FULL_BOOKS):
        out.append((b, "sweep", SWEEP, START_BITS[(bi + 1) % 5]))
        out.append((b, "escapes", WAVES, START_BITS[(bi + 3) % 5]))
    # every size edge and every start bit with zipf21 (no case of a full book is larger than its sweep)
    sized = KINDS + ["escapes"]
    for si, nsym in enumerate(EDGE_SIZES):
        case = ("zipf21", sized[(si + 3) % 6], nsym, START_BITS[(si + 1) % 5])
        if case not in out:
            out.append(case)
    out.append(("zipf21", "sweep", SWEEP, 45))
    return out


CASES = _cases()


def _case_id(case):
    return "%s-%s-%d-s%d" % case


def test_case_matrix_is_complete():
    """The cross product is not run in full; this is what must appear."""
    for b in BOOKS:
        assert {k for bb, k, _, _ in CASES if bb == b} == set(KINDS + FULL_KINDS if b in FULL_BOOKS else KINDS), b
    for b in ("fib57", "hot25", "dense16"):
        assert {n for bb, _, n, _ in CASES if bb == b} >= set(EDGE_SIZES) | {WAVES, ALL_CUS}, b
        assert {s for bb, _, _, s in CASES if bb == b} == set(START_BITS), b
    assert {n for bb, _, n, _ in CASES if bb == "zipf21"} >= set(EDGE_SIZES) | {WAVES, SWEEP}
    assert {s for bb, _, _, s in CASES if bb == "zipf21"} == set(START_BITS)
    assert ("zipf21", "sweep", SWEEP, 45) in CASES and len([c for c in CASES if c[:2] == ("zipf21", "sweep")]) == 2
    assert max(n for bb, _, n, _ in CASES if bb in FULL_BOOKS) <= SWEEP
    assert len(set(CASES)) == len(CASES)
    assert max(n for _, _, n, _ in CASES) <= 1 << 21


# ---- device helpers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def _guarded(nbytes):
    """nbytes between two 64-byte guards, all 0xA5: (whole buffer, the region)."""
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


def _host(t):
    return t.cpu().numpy()


def _u64(t):
    return [int(v) for v in t.cpu().numpy().view(np.uint64)]


class Checks:
    """Runs the checks of one case; a check that raises a device-side status fails alone."""

    def __init__(self, codec):
        self.codec = codec
        self.failed = []

    def run(self, name, fn):
        from huffman_amd import HZError
        try:
            fn()
            self.codec.sync()
        except HZError as e:
            if e.status == HZ_EHIP:   # a HIP runtime error: nothing more runs on this device
                pytest.exit(f"{name}: {e}", returncode=3)
            self.failed.append(f"{name}: {e}")
        except AssertionError as e:
            self.failed.append(f"{name}: {e}")

    def expect(self, name, ok, what=""):
        if not ok:
            self.failed.append(f"{name}: {what}" if what else name)


_uploaded = [None]


def _upload(codec, bk):
    if _uploaded[0] != (id(codec), bk.name):
        codec.dev.upload(bk.cb)
        _uploaded[0] = (id(codec), bk.name)


def _cuts(m, ln):
    """Two payload bits (after start_bit) to cut at: inside a longest codeword of the stream, at an odd
    bit of it, and at a codeword boundary. None where the stream is too short for parts."""
    L = ln[m.sym].astype(np.int64)
    P = m.end_bit - m.start_bit
    if m.nsym < 4 or P < 64:
        return None
    third = m.nsym // 3
    i = third + int(np.argmax(L[third:2 * third + 1]))          # a longest codeword of the middle third
    inside = int(m.pos[i]) - m.start_bit + (((int(L[i]) // 2) | 1) if L[i] > 1 else 0)
    j = min(m.nsym - 1, 2 * third + 2)
    boundary = int(m.pos[j]) - m.start_bit
    if not 0 < inside < boundary < P:
        return None
    return inside, boundary


def run_case(codec, case):
    """Every check of one case against the model; returns the list of failures."""
    import torch
    b, kind, nsym, start_bit = case
    bk = book(b)
    dev = codec.dev
    rng = np.random.default_rng(zlib.crc32(_case_id(case).encode()))
    sym = _stream(bk, kind, nsym, rng)
    m = ref_stream.model(sym, bk.ln, bk.code, start_bit, _lead(start_bit))
    blocks = np.diff(m.start.astype(np.int64))
    if b in ("fib57", "fib41") and kind == "longest" and nsym >= BLK:
        assert int(blocks[:nsym // BLK].min()) >= 65536          # the case itself: blocks past 2^16 bits
        assert m.max_bits == BLK * int(bk.ln.max())              # and the largest block there is
    if b in ("fib57", "fib41") and kind == "blocks" and nsym >= BLK:
        assert int(blocks[0]) >= 65536 and (nsym < 2 * BLK or int(blocks[1]) < 65536)
    ck = Checks(codec)
    _upload(codec, bk)
    nbytes = m.payload.size                       # whole words: hz_pack's zero bits to the word's end included
    ibytes = m.index.size
    first = 4 * (start_bit // 32)                 # the word of start_bit: nothing before it is pack's
    x = torch.from_numpy(sym.view(np.uint8)).cuda()
    want = torch.from_numpy(sym.view(np.uint8).copy()).cuda()
    model_index = torch.from_numpy(m.index).cuda()
    model_seek = torch.from_numpy(m.start.view(np.uint8).copy()).cuda()
    paybuf, pay = _guarded(nbytes)
    idxbuf, idx = _guarded(ibytes)

    # 1, 2: hz_pack's payload and index
    ck.run("pack", lambda: dev.pack(x.data_ptr(), x.numel(), start_bit, m.lead, pay.data_ptr(), nbytes, idx.data_ptr()))
    got = _host(pay)
    ck.expect("1 pack payload", np.array_equal(got[first:], m.payload[first:]),
              "first differing byte %s" % (np.nonzero(got[first:] != m.payload[first:])[0][:1] + first))
    ck.expect("1 pack wrote before start_bit's word", bool((got[:first] == 0xA5).all()))
    ck.expect("1 pack payload guards", _guards_intact(paybuf, nbytes))
    ck.expect("2 pack index", np.array_equal(_host(idx), m.index), _index_diff(_host(idx), m, nsym))
    ck.expect("2 pack index guards", _guards_intact(idxbuf, ibytes))
    # from here on every consumer reads the MODEL's payload and index, so one wrong producer does not hide the rest
    paybuf, pay = _guarded(nbytes)
    pay.copy_(torch.from_numpy(m.payload))

    # 3: hz_index_build from the payload alone
    i3buf, i3 = _guarded(ibytes)
    ck.run("3 index_build", lambda: dev.index_build(pay.data_ptr(), nbytes, start_bit, nsym, i3.data_ptr()))
    ck.expect("3 index_build", np.array_equal(_host(i3), m.index), _index_diff(_host(i3), m, nsym))
    ck.expect("3 index_build guards", _guards_intact(i3buf, ibytes))

    # 4: hz_index_expand from start[]
    i4buf, i4 = _guarded(ibytes)
    ck.run("4 index_expand", lambda: dev.index_expand(pay.data_ptr(), nbytes, model_seek.data_ptr(), nsym, i4.data_ptr()))
    ck.expect("4 index_expand", np.array_equal(_host(i4), m.index), _index_diff(_host(i4), m, nsym))
    ck.expect("4 index_expand guards", _guards_intact(i4buf, ibytes))

    # 5: hz_decode through the index
    obuf, out = _guarded(2 * nsym)
    ck.run("5 decode", lambda: dev.decode(pay.data_ptr(), nbytes, nsym, model_index.data_ptr(), out.data_ptr()))
    ck.expect("5 decode", torch.equal(out, want))
    ck.expect("5 decode guards", _guards_intact(obuf, 2 * nsym))

    # 6: hz_decode_indexless, whole and a prefix
    for count in sorted({nsym, max(1, nsym // 2), max(1, nsym - 1)}, reverse=True):
        obuf, out = _guarded(2 * count)
        end = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
        ck.run(f"6 indexless {count}", lambda: dev.decode_indexless(pay.data_ptr(), nbytes, start_bit, count,
                                                                    out.data_ptr(), end.data_ptr()))
        ck.expect(f"6 indexless {count} symbols", torch.equal(out, want[:2 * count]))
        ck.expect(f"6 indexless {count} end bit", _u64(end)[0] == int(m.pos[count]), f"{_u64(end)[0]} != {int(m.pos[count])}")
        ck.expect(f"6 indexless {count} guards", _guards_intact(obuf, 2 * count))

    # 7: the split parts
    cuts = _cuts(m, bk.ln) if nbytes >= 16 else None
    if cuts:
        _parts(ck, codec, bk, m, pay, want, [0, cuts[0], m.end_bit - start_bit], slices=False)
        _parts(ck, codec, bk, m, pay, want, [0, cuts[0], cuts[1], m.end_bit - start_bit], slices=True)

    # 8: hz_decode_range from the seek table and from the full index
    ranges = [(0, min(nsym, 100)), (nsym - 1, 1)]
    if nsym > BLK:
        ranges.append((BLK - 1, min(BLK + 3, nsym - (BLK - 1))))
    for r, (begin, count) in enumerate(ranges):
        for full in (False, True):
            rbuf = torch.full((GUARD + 16 + 2 * count + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            lo = GUARD + (0, 2, 14)[(r + full) % 3]
            table = model_index if full else model_seek
            ck.run(f"8 range {begin}+{count} full={full}",
                   lambda: dev.decode_range(pay.data_ptr(), nbytes, table.data_ptr(), nsym, begin, count,
                                            rbuf[lo:].data_ptr(), full))
            ck.expect(f"8 range {begin}+{count} full={full}",
                      torch.equal(rbuf[lo:lo + 2 * count], want[2 * begin:2 * (begin + count)]))
            ck.expect(f"8 range {begin}+{count} full={full} guards",
                      bool((rbuf[:lo] == 0xA5).all()) and bool((rbuf[lo + 2 * count:] == 0xA5).all()))
    ck.expect("payload (an input) changed", np.array_equal(_host(pay), m.payload) and _guards_intact(paybuf, nbytes))
    return ck.failed


def _index_diff(got, m, nsym):
    """Where an index differs from the model's, in its own terms."""
    nb = ref_stream.nblocks(nsym)
    if got.size != m.index.size:
        return "size"
    start = got[:8 * (nb + 1)].view(np.uint64)
    if not np.array_equal(start, m.start):
        k = int(np.nonzero(start != m.start)[0][0])
        return f"start[{k}] = {int(start[k])}, model {int(m.start[k])}"
    mb = int(got[8 * (nb + 1):8 * (nb + 2)].view(np.uint64)[0])
    if mb != m.max_bits:
        return f"max_bits = {mb}, model {m.max_bits}"
    sub = got[8 * (nb + 2):].view("<u2").reshape(nb, 256)
    bad = np.argwhere(sub != m.sub)
    return f"sub{bad[0].tolist()} = {int(sub[tuple(bad[0])])}, model {int(m.sub[tuple(bad[0])])}" if bad.size else ""


def _parts(ck, codec, bk, m, pay, want, bounds, slices):
    """The stream in len(bounds) - 1 parts cut at payload bits `bounds`: each part scanned from the whole
    payload or from a 16-byte aligned slice of it (its lead-in, its bits and max_len bits after), first
    from its walked entry (then refixed to the true one where they differ), its summary -- codewords,
    exit bit, entry bit -- equal to the serial walk of the model's payload from the true entry, and its
    codewords decoded at the sum of the counts before it."""
    import torch
    dev = codec.dev
    tag = "7 parts=%d" % (len(bounds) - 1)
    start, nsym, nbytes = m.start_bit, m.nsym, m.payload.size
    max_len = int(bk.ln.max())
    summ = torch.zeros(32, dtype=torch.uint8, device="cuda")
    obuf, out = _guarded(2 * nsym)
    entry, first = start, 0
    for k, (pb, pe) in enumerate(zip(bounds, bounds[1:])):
        lo_bit = start + pb - min(LEAD_BITS, pb)
        b0 = lo_bit // 8 // 16 * 16 if slices else 0
        b1 = min(nbytes, ((start + pe + max_len + 7) // 8 + 16 + 15) // 16 * 16) if slices else nbytes
        if b1 - b0 < 16:
            b0 = max(0, b1 - 16) // 16 * 16
        ref_n, ref_exit, _ = ref_stream.span_decode(m.payload, bk.ln, bk.code, entry, start + pe)
        given = entry if k == 2 else UNKNOWN_ENTRY     # the third part is handed its true entry
        ck.run(f"{tag} scan {k}", lambda: dev.indexless_scan(pay.data_ptr() + b0, b1 - b0, start, pb, pe, given,
                                                             summ.data_ptr(), nsym=nsym, payload_bit_base=8 * b0))
        cnt, xit, ent = _u64(summ)[:3]
        if k == 0:
            ck.expect(f"{tag} first part's walked entry", ent == start, f"{ent} != {start}")
        if ent != entry:
            ck.run(f"{tag} refix {k}", lambda: dev.indexless_refix(entry, summ.data_ptr()))
            cnt, xit, ent = _u64(summ)[:3]
        ck.expect(f"{tag} summary {k}", (cnt, xit, ent) == (ref_n, ref_exit, entry),
                  f"(count, exit, entry) = {(cnt, xit, ent)}, serial walk {(ref_n, ref_exit, entry)}")
        take = min(ref_n, nsym - first)
        tbuf, tmp = _guarded(2 * take)
        end = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
        ck.run(f"{tag} decode {k}", lambda: dev.indexless_decode(take, tmp.data_ptr(), end.data_ptr()))
        ck.expect(f"{tag} decode {k} guards", _guards_intact(tbuf, 2 * take))
        if first + take == nsym:
            ck.expect(f"{tag} end bit", _u64(end)[0] == m.end_bit, f"{_u64(end)[0]} != {m.end_bit}")
        out[2 * first:2 * (first + take)] = tmp
        first += ref_n
        entry = ref_exit
    assert first == nsym and entry == m.end_bit        # the model's own walk covers the stream
    ck.expect(f"{tag} output", torch.equal(out, want))
    ck.expect(f"{tag} output guards", _guards_intact(obuf, 2 * nsym))


# ---- the tests --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_designed_stream(codec, case):
    failed = run_case(codec, case)
    assert not failed, "\n".join(failed)


TOUR_CLASSES = ["hot25", "fib57", "dense16", "fixed16", "zipf21"]
TOUR_NSYM = 3 * BLK + 5     # three blocks and a ragged tail: the least that has a middle block


def _tour(n):
    """A closed walk over every ordered pair of n classes (n prime): for each step d = 1 .. n - 1 the
    cycle 0, d, 2d, ... (mod n) back to 0 takes the n pairs (i, i + d) once."""
    walk = [0]
    for d in range(1, n):
        walk += [(d * k) % n for k in range(1, n + 1)]
    return walk


def test_reupload_between_table_classes(codec):
    """Every ordered pair of table classes uploaded one after the other on ONE context: hot25 (LUT with
    walker tables, HOT encode), fib57 (codes past kWalkMaxLen: no walker, its own chain escape table,
    WIDE encode), dense16 (DENSE with its chain LUT beside), fixed16 (no index-less tables at all) and
    zipf21 (a full alphabet). A closed tour of the 20 pairs takes 21 uploads; after each one a `chains`
    stream of three blocks and a ragged tail is packed at a nonzero start bit and goes through hz_decode,
    hz_decode_indexless and hz_index_build, each bit-exact against the model with its guards intact. A
    re-upload that leaves behind what the previous class set -- walk_lds_bytes, the chain_* views, the
    FIXED16 part state, a table smaller than its capacity -- decodes through the wrong tables here."""
    import torch
    dev = codec.dev
    walk = _tour(len(TOUR_CLASSES))
    pairs = set(zip(walk, walk[1:]))
    assert len(walk) == 21 and walk[0] == walk[-1]
    assert pairs == {(i, j) for i in range(5) for j in range(5) if i != j}
    models = {}
    failed = []
    for step, ci in enumerate(walk):
        bk = book(TOUR_CLASSES[ci])
        if ci not in models:
            start_bit = START_BITS[1 + ci % 4]      # 5, 31, 32 or 45: never 0
            rng = np.random.default_rng(zlib.crc32(("tour-" + bk.name).encode()))
            sym = _stream(bk, "chains", TOUR_NSYM, rng)
            models[ci] = (sym, ref_stream.model(sym, bk.ln, bk.code, start_bit, _lead(start_bit)))
        sym, m = models[ci]
        nsym, start_bit, nbytes, ibytes = TOUR_NSYM, m.start_bit, m.payload.size, m.index.size
        first = 4 * (start_bit // 32)
        tag = "upload %d (%s after %s)" % (step, bk.name, TOUR_CLASSES[walk[step - 1]] if step else "-")
        ck = Checks(codec)
        dev.upload(bk.cb)
        _uploaded[0] = (id(codec), bk.name)
        x = torch.from_numpy(sym.view(np.uint8)).cuda()
        want = torch.from_numpy(sym.view(np.uint8).copy()).cuda()
        model_index = torch.from_numpy(m.index).cuda()
        paybuf, pay = _guarded(nbytes)
        idxbuf, idx = _guarded(ibytes)
        ck.run("pack", lambda: dev.pack(x.data_ptr(), x.numel(), start_bit, m.lead, pay.data_ptr(), nbytes, idx.data_ptr()))
        ck.expect("pack payload", np.array_equal(_host(pay)[first:], m.payload[first:]))
        ck.expect("pack index", np.array_equal(_host(idx), m.index), _index_diff(_host(idx), m, nsym))
        ck.expect("pack guards", _guards_intact(paybuf, nbytes) and _guards_intact(idxbuf, ibytes))
        # the consumers read the MODEL's payload and index
        paybuf, pay = _guarded(nbytes)
        pay.copy_(torch.from_numpy(m.payload))
        obuf, out = _guarded(2 * nsym)
        ck.run("decode", lambda: dev.decode(pay.data_ptr(), nbytes, nsym, model_index.data_ptr(), out.data_ptr()))
        ck.expect("decode", torch.equal(out, want))
        ck.expect("decode guards", _guards_intact(obuf, 2 * nsym))
        obuf, out = _guarded(2 * nsym)
        end = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
        ck.run("indexless", lambda: dev.decode_indexless(pay.data_ptr(), nbytes, start_bit, nsym, out.data_ptr(),
                                                         end.data_ptr()))
        ck.expect("indexless symbols", torch.equal(out, want))
        ck.expect("indexless end bit", _u64(end)[0] == m.end_bit, f"{_u64(end)[0]} != {m.end_bit}")
        ck.expect("indexless guards", _guards_intact(obuf, 2 * nsym))
        i3buf, i3 = _guarded(ibytes)
        ck.run("index_build", lambda: dev.index_build(pay.data_ptr(), nbytes, start_bit, nsym, i3.data_ptr()))
        ck.expect("index_build", np.array_equal(_host(i3), m.index), _index_diff(_host(i3), m, nsym))
        ck.expect("index_build guards", _guards_intact(i3buf, ibytes))
        ck.expect("payload (an input) changed", np.array_equal(_host(pay), m.payload) and _guards_intact(paybuf, nbytes))
        failed += [tag + ": " + f for f in ck.failed]
    assert not failed, "\n".join(failed)


def test_romeo_seek_table_equals_model(hz):
    """hz.build_seek (hz_index_build inside) on the golden romeo.txt.compressed: the model's start[] for the
    file's symbols under the file's codebook, from the header's payload bit."""
    from huffman_amd import codebook_arrays
    with open(os.path.join(GOLD, "romeo.txt"), "rb") as f:
        data = np.frombuffer(f.read(), dtype=np.uint8)
    with open(os.path.join(GOLD, "romeo.txt.compressed"), "rb") as f:
        blob = f.read()
    cb, info = hz.parse_header(blob)
    _, ln, code = codebook_arrays(cb)
    sym = data[:2 * (data.size // 2)].view("<u2")
    pos = ref_stream.positions(sym, ln, info.payload_bit)
    start, _, _ = ref_stream.index_arrays(pos, sym.size)
    assert np.array_equal(hz.build_seek(blob), start)


def _child(env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "pipe"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_decoder_forms(built_lib, pipe):
    """HZ_DEC_PIPE=0 / 1 (2 is the default, every other test): the plain and the one-block pipelined forms
    of the block decoder on the fib57, hot25, dense16 and zipf21 cases."""
    _child({"HZ_DEC_PIPE": pipe})


if __name__ == "__main__":
    assert sys.argv[1:] == ["pipe"], sys.argv
    from huffman_amd.pipeline import StreamCodec
    _c = StreamCodec(0)
    _bad = []
    for _case in CASES:
        if _case[0] in ("fib57", "hot25", "dense16", "zipf21") and _case[2] != ALL_CUS:
            _bad += [_case_id(_case) + " " + f for f in run_case(_c, _case)]
    if _bad:
        print("\n".join(_bad))
        sys.exit(1)
    print("ok")
